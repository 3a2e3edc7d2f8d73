"""Net_2's convolutional half (MNIST/models_mnist/Net2.py:13-14) in float64, and MNIST-like inputs for it (host only: numpy / torch CPU).

    a1 = relu(max_pool2d(conv1(x), 2))                     [B,1,28,28]  -> [B,32,12,12]
    a2 = relu(max_pool2d(drop / keep * conv2(a1), 2))      [B,32,12,12] -> [B,64,4,4]

Nothing here calls an ee_* kernel.  Two statements of the network:

  forward64   the FREE forward: both convolutions as explicit tap loops in float64 (every output pixel by the same operation sequence, so
              bitwise identical receptive patches give bitwise identical values), the 2x2 pool as an explicit scan in ATen's order
              (0,0) (0,1) (1,0) (1,1) with ATen's rule `v > best or isnan(v)` - the first maximum wins, the last NaN wins;
  replay64    the same network ON A GIVEN BRANCH: the pool winners (2-bit codes) and the ReLU gates are arguments, which leaves a linear map
              that torch autograd differentiates - what tests/branch_replay.py does for the ResNets.

and what a comparison of an fp32 kernel with them needs: bound32 (a derived rounding bound per pre-pool value) and classify (which
windows' winner rounding cannot change, which windows tie exactly, and which are left undecided).

Real MNIST is mostly exact ties: four pixels in five are exactly 0, strokes saturate at exactly 1.  mnist_like draws such images."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 0.3            # the MNIST configs' epsilon: the PGD start is clamp(x + U(-EPS, EPS), 0, 1)
K1, K2 = 25, 800     # products per output value of conv1 / conv2
U32 = 2.0 ** -24     # unit roundoff of fp32
CORNER = 16          # images of kind 0 / 4 keep their top-left CORNER x CORNER pixels flat: the footprint of conv2's window (0, 0)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _rim(mask):
    """the anti-aliased rim of a binary shape: a background pixel with n of its 3x3 neighbours inside takes the grey level round(255 n / 9) / 255"""
    p = np.pad(mask.astype(np.int64), 1)
    n = sum(p[i:i + 28, j:j + 28] for i in range(3) for j in range(3))
    k = np.rint(255.0 * n / 9.0).astype(np.float32)
    img = k / np.float32(255.0)
    img[mask] = np.float32(1.0)
    return img.astype(np.float32)


def _strokes(rng, free_corner):
    """horizontal, vertical and diagonal bars and a filled blob of exactly 1.0 on a background of exactly 0; free_corner: everything
    (rim included) stays out of the top-left CORNER x CORNER pixels"""
    m = np.zeros((28, 28), dtype=bool)
    r, h, c0, n = int(rng.integers(18, 22)), int(rng.integers(2, 4)), int(rng.integers(1, 6)), int(rng.integers(10, 20))
    m[r:r + h, c0:c0 + n] = True                                   # horizontal bar, rows >= 18
    c, w, r0, n = int(rng.integers(18, 24)), int(rng.integers(2, 4)), int(rng.integers(1, 5)), int(rng.integers(12, 22))
    m[r0:r0 + n, c:c + w] = True                                   # vertical bar, columns >= 18
    r0, c0, n = int(rng.integers(17, 19)), int(rng.integers(2, 9)), int(rng.integers(5, 9))
    for t in range(n):
        m[r0 + t, c0 + t:c0 + t + 2] = True                        # diagonal bar, rows >= 17
    cy, cx, rad = int(rng.integers(21, 24)), int(rng.integers(21, 24)), 3.2
    yy, xx = np.mgrid[0:28, 0:28]
    m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad              # blob
    if not free_corner:
        r, c0, n = int(rng.integers(3, 12)), int(rng.integers(2, 8)), int(rng.integers(6, 14))
        m[r:r + 2, c0:c0 + n] = True
        cy, cx = int(rng.integers(5, 12)), int(rng.integers(5, 12))
        m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= 2.3 * 2.3
    img = _rim(m)
    if free_corner:
        assert not img[:CORNER, :CORNER].any()
    return img


def mnist_like(B, seed, start=None):
    """float32 [B,1,28,28].  Image b is of kind b % 6: 0, 4 strokes outside the top-left corner; 1 all zero; 2 all 1.0; 3, 5 strokes anywhere.
    Background exactly 0, strokes exactly 1.0, rims at grey levels k / 255.

    start=EPS applies the PGD start clamp(x + d, 0, 1) in float32 with d in U(-start, start).  On images with b % 3 == 2 d is drawn per
    pixel, as attacks.py draws it.  Per-pixel noise leaves no two 5x5 patches of a window bitwise identical (a flat 6x6 patch survives it
    with probability 2^-36), i.e. NO exact tie for the tests to pin; so on the other images d is drawn once per quadrant (split at row /
    column 16): flat regions stay flat, at 0 where d < 0 and at a level that is no round number where d > 0 - what the later iterates of a
    sign-gradient attack look like over a flat patch (every pixel of it has moved by the same multiple of the step)."""
    rng = np.random.default_rng(seed)
    x = np.zeros((B, 1, 28, 28), dtype=np.float32)
    for b in range(B):
        kind = b % 6
        if kind == 2:
            x[b] = np.float32(1.0)
        elif kind != 1:
            x[b, 0] = _strokes(rng, free_corner=kind in (0, 4))
    if start is not None:
        hi = (np.arange(28) >= CORNER).astype(np.int64)
        for b in range(B):
            if b % 3 == 2:
                d = rng.uniform(-start, start, (28, 28)).astype(np.float32)
            else:
                d = rng.uniform(-start, start, (2, 2)).astype(np.float32)[hi[:, None], hi[None, :]]
            x[b, 0] = np.clip(x[b, 0] + d, np.float32(0.0), np.float32(1.0))
    return x


def net2_params(seed, hard=False):
    """Net_2()'s parameters under torch.manual_seed(seed) (the layers are created in Net_2.__init__'s order: conv1, conv2, fc1, fc2), as a
    dict of float32 tensors named as its state_dict.  hard: conv1.bias and conv2.bias get four channels of exactly 0.0 (a tie at 0 over a
    flat patch of zeros, which the ReLU must block), four positive and four negative ones."""
    torch.manual_seed(seed)
    layers = {"conv1": torch.nn.Conv2d(1, 32, 5), "conv2": torch.nn.Conv2d(32, 64, 5), "fc1": torch.nn.Linear(1024, 1024), "fc2": torch.nn.Linear(1024, 10)}
    p = {"%s.%s" % (n, k): v.detach().clone() for n, m in layers.items() for k, v in m.named_parameters()}
    if hard:
        edit = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.02, 0.05, 0.11, 0.17, -0.02, -0.05, -0.11, -0.17])
        p["conv1.bias"][:12] = edit
        p["conv2.bias"][:12] = edit * 0.2
    return p


def conv_params(p):
    return p["conv1.weight"], p["conv1.bias"], p["conv2.weight"], p["conv2.bias"]


def dropout_draw(B, seed):
    """Dropout2d's Bernoulli(keep = 0.5) draw [B,64] as 0 / 1 float32, at least a third of the (image, channel) pairs dropped"""
    d = (np.random.default_rng(seed).random((B, 64)) < 0.5).astype(np.float32)
    assert (d == 0).mean() >= 1.0 / 3.0
    return d


# ---- the free forward --------------------------------------------------------------------------------------------------------------
def _np64(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float64)


def conv64(inp, w, b):
    """valid 5x5 convolution in float64 as a tap loop: every output pixel is formed by the same sequence of operations"""
    B, Ci, H, W = inp.shape
    OH, OW = H - 4, W - 4
    z = np.zeros((B, w.shape[0], OH, OW))
    for ci in range(Ci):
        for ky in range(5):
            for kx in range(5):
                z += w[None, :, ci, ky, kx, None, None] * inp[:, None, ci, ky:ky + OH, kx:kx + OW]
    return z + b[None, :, None, None]


def windows(z):
    """[B,C,2h,2w] -> [B,C,h,w,4]: the four values of every 2x2 window in ATen's scan order (0,0) (0,1) (1,0) (1,1); code = 2 dy + dx"""
    B, C, H, W = z.shape
    return z.reshape(B, C, H // 2, 2, W // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)


def scan_pool(v4):
    """ATen's max_pool2d scan over the last axis: `v > best or isnan(v)` takes over -> (best, code)"""
    best = np.full(v4.shape[:-1], -np.inf)
    code = np.zeros(v4.shape[:-1], dtype=np.uint8)
    for k in range(4):
        v = v4[..., k]
        take = (v > best) | np.isnan(v)
        best = np.where(take, v, best)
        code = np.where(take, np.uint8(k), code)
    return best, code


def scale64(drop, keep):
    """the factor the kernels apply: the 0 / 1 draw divided by keep in fp32"""
    return None if drop is None else (_np64(drop).astype(np.float32) / np.float32(keep)).astype(np.float64)


def forward64(x, params, drop=None, keep=1.0, a1_in=None):
    """The free forward.  params = (w1, b1, w2, b2); drop: the 0 / 1 draw [B,64] or None.  a1_in: what conv2 reads instead of this
    function's own a1 (the fp32 a1 a kernel produced: the second half is then judged on the input it really had).
    -> dict(v1 [B,32,12,12,4], code1, a1, v2 [B,64,4,4,4], code2, a2): the four pre-pool values per window, the winners, the outputs"""
    w1, b1, w2, b2 = (_np64(t) for t in params)
    with np.errstate(all="ignore"):
        v1 = windows(conv64(_np64(x), w1, b1))
        best1, code1 = scan_pool(v1)
        a1 = np.where(best1 <= 0, 0.0, best1)  # ATen's relu keeps a NaN
        z2 = conv64(a1 if a1_in is None else _np64(a1_in), w2, b2)
        s = scale64(drop, keep)
        if s is not None:
            z2 = z2 * s[:, :, None, None]
        v2 = windows(z2)
        best2, code2 = scan_pool(v2)
        a2 = np.where(best2 <= 0, 0.0, best2)
    return dict(v1=v1, code1=code1, a1=a1, v2=v2, code2=code2, a2=a2)


# ---- the same network on a given branch ---------------------------------------------------------------------------------------------
def _twindows(z):
    B, C, H, W = z.shape
    return z.view(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)


def _t64(t):
    return (t.detach().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.asarray(t))).double()


def _tcpu(t, dtype):
    return (t.detach().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.asarray(t))).to(dtype)


def replay64(x, params, drop, keep, code1, code2, open1, open2, a1_in=None):
    """The network with the pool winners (code = 2 dy + dx per window) and the ReLU gates (boolean: the value passes) GIVEN: float64 torch
    on the CPU, differentiable.  -> dict(x, params (the float64 leaves: x, [w1, b1, w2, b2]), s1 / s2 (the coded pre-pool values before
    the gate), a1, a2).  a1_in: conv2 reads it instead of a1 (values only: the chain to x is cut)."""
    xl = _t64(x).requires_grad_(True)
    w1, b1, w2, b2 = leaves = [_t64(t).requires_grad_(True) for t in params]
    s1 = _twindows(F.conv2d(xl, w1, b1)).gather(-1, _tcpu(code1, torch.int64).unsqueeze(-1)).squeeze(-1)
    a1 = torch.where(_tcpu(open1, torch.bool), s1, torch.zeros_like(s1))
    z2 = F.conv2d(a1 if a1_in is None else _t64(a1_in), w2, b2)
    s = scale64(drop, keep)
    if s is not None:
        z2 = z2 * torch.from_numpy(s)[:, :, None, None]
    s2 = _twindows(z2).gather(-1, _tcpu(code2, torch.int64).unsqueeze(-1)).squeeze(-1)
    a2 = torch.where(_tcpu(open2, torch.bool), s2, torch.zeros_like(s2))
    return dict(x=xl, params=leaves, s1=s1, a1=a1, s2=s2, a2=a2)


def replay_gradients(rep, da2):
    """(dx, da1, dw1, db1, dw2, db2) of <a2, da2> on the replayed branch"""
    w1, b1, w2, b2 = rep["params"]
    dx, da1, dw1, db1, dw2, db2 = torch.autograd.grad(rep["a2"], [rep["x"], rep["a1"], w1, b1, w2, b2], _t64(da2), retain_graph=True)
    return dx, da1, dw1, db1, dw2, db2


# ---- rounding -----------------------------------------------------------------------------------------------------------------------
def bound32(inp, w, b, K, scale=None):
    """A rigorous bound on |fp32 value - exact value| of a pre-pool value computed as a K-term chain of fused multiply-adds (in any order,
    in any number of partial chains) plus a bias add and a scale: (K + 2) u (sum |w x| + |b|) |scale|, u = 2^-24, evaluated in float64
    (each of the at most K + 2 roundings on the way is relative to a partial result no larger than sum |w x| + |b|; second-order terms
    K^2 u^2 are 1e-9 of it and are covered by the two roundings the count is generous by).  -> [B,C,h,w,4], as windows()."""
    with np.errstate(all="ignore"):
        s = conv64(np.abs(_np64(inp)), np.abs(_np64(w)), np.abs(_np64(b)))
        if scale is not None:
            s = s * np.abs(scale)[:, :, None, None]
    return windows((K + 2) * U32 * s)


def patch_equal(inp32):
    """E[k][j] [B,h,w]: the receptive patches ([Ci,5,5] of the fp32 input) of positions k and j of a window are bitwise identical"""
    a = inp32.detach().cpu().numpy() if isinstance(inp32, torch.Tensor) else np.asarray(inp32)
    assert a.dtype == np.float32
    bits = np.ascontiguousarray(a).view(np.uint32)
    win = np.lib.stride_tricks.sliding_window_view(bits, (5, 5), axis=(2, 3))  # [B,Ci,OH,OW,5,5]
    pos = [win[:, :, dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)]
    return [[(pos[k] == pos[j]).all(axis=(1, 4, 5)) for j in range(4)] for k in range(4)]


def classify(v4, b4, inp32, dropped=None):
    """The three classes of windows.  v4: forward64's pre-pool values; b4: bound32 of them; inp32: the fp32 input of the convolution.
    -> (decided, tie, first) [B,C,h,w]: `first` is forward64's winner (the first maximum).
      decided    one position holds the float64 maximum and its margin over every other exceeds twice the (largest) bound: no fp32
                 evaluation within the bound can name another winner;
      tie        several positions hold the float64 maximum, their receptive patches are bitwise identical - a kernel that forms every
                 output pixel by the same instruction sequence produces identical bits there, and ATen's scan keeps the FIRST - and every
                 other position is decided against them.  Also every window of a dropped channel (dropped [B,C]): its four values are
                 (finite) * 0 = +-0 in any arithmetic, all equal, so the first position wins;
      undecided  the rest (windows with a non-finite value among them)."""
    with np.errstate(all="ignore"):
        finite = np.isfinite(v4).all(-1)
        m, first = scan_pool(v4)
        tied = v4 == m[..., None]
        bw = b4.max(-1)
        clear = (tied | (m[..., None] - v4 > 2.0 * bw[..., None])).all(-1)
    E = patch_equal(inp32)
    same = np.ones(v4.shape[:-1], dtype=bool)
    for k in range(4):
        for j in range(4):
            # position j ties with the maximum while `first` is k: its patch must equal k's
            same &= ~((first == k) & tied[..., j]) | E[k][j][:, None]
    n = tied.sum(-1)
    decided = finite & (n == 1) & clear
    tie = finite & (n >= 2) & same & clear
    if dropped is not None:
        d = np.broadcast_to(np.asarray(dropped, dtype=bool)[:, :, None, None], finite.shape)
        tie = tie | (finite & d)
        decided = decided & ~d
    return decided, tie, first


def shares(decided, tie):
    """(share of exact-tie windows, share of undecided windows)"""
    return float(tie.mean()), float(1.0 - (decided | tie).mean())


# ---- the cases the host test and the GPU test share -----------------------------------------------------------------------------------
# one axis at a time around the base case: the batch (11 and 23: two and three groups of ten images in the parameter-gradient kernels, the
# last one partly filled), the PGD start, the weights, the dropout draw
BASE = dict(B=11, start=None, hard=True, drop=True)
CASES = [BASE] + [dict(BASE, B=b) for b in (1, 3, 23)] + [dict(BASE, start=EPS), dict(BASE, hard=False), dict(BASE, drop=False),
                                                           dict(BASE, B=3, start=EPS, hard=False, drop=False)]
KEEP = 0.5


def case_id(c):
    return "B%d-%s-%s-%s" % (c["B"], "start" if c["start"] else "clean", "hard" if c["hard"] else "seeded", "drop" if c["drop"] else "nodrop")


def make_case(c):
    """-> (x [B,1,28,28] float32, (w1, b1, w2, b2) float32 tensors, the 0 / 1 draw [B,64] float32 or None, keep)"""
    x = mnist_like(c["B"], 100 + c["B"], c["start"])
    return x, conv_params(net2_params(7, c["hard"])), (dropout_draw(c["B"], c["B"]) if c["drop"] else None), (KEEP if c["drop"] else 1.0)


def classify_both(x, params, drop, keep, a1_32):
    """forward64 with conv2 reading the fp32 a1_32, and the classes of both layers' windows
    -> (fwd, (decided1, tie1, first1), (decided2, tie2, first2), bound1, bound2)"""
    w1, b1, w2, b2 = params
    fwd = forward64(x, params, drop, keep, a1_in=a1_32)
    bd1 = bound32(x, w1, b1, K1)
    bd2 = bound32(a1_32, w2, b2, K2, scale64(drop, keep))
    c1 = classify(fwd["v1"], bd1, x)
    c2 = classify(fwd["v2"], bd2, a1_32, None if drop is None else np.asarray(drop) == 0)
    return fwd, c1, c2, bd1, bd2
