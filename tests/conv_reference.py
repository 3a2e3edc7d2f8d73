"""Host reference for the convolution kernels (ee_wino.hip, ee_s2.hip, ee_conv.hip, ee_dense.hip, ee_wrw.hip, ee_wprep.hip): plain float64 torch.

A `kind` names one operation of one kernel family; a `case` is a dict {"kind", "shape" = (B, Cin, Cout, H, W) of the convolution's INPUT map, and
the float32 operands the kernel reads}:

    kind          operands      result                                   kernel
    wino_fwd      x, w          conv3x3(x, w), stride 1, padding 1       ee_wino3x3_f32 on wino_f filters (H = 2: ee_dense2x2_f32)
    wino_bwd      dy, w         its input gradient                       ee_wino3x3_f32 on wino_b filters (H = 2: ee_dense2x2_f32, s1t)
    s2_fwd        x, w          conv3x3(x, w), stride 2, padding 1       ee_conv3x3s2_small_fwd_f32
    s2_bwd        dy, w         its input gradient                       ee_conv3x3s2_small_bwd_data_f32
    pair_fwd      x, w, w1      (s2_fwd, conv1x1(x, w1) stride 2)        ee_conv3x3s2_pair_fwd_f32
    pair_bwd      dy, dy1, w, w1  the two input gradients, summed        ee_conv3x3s2_pair_bwd_data_f32
    c1s2_fwd      x, w          conv1x1(x, w), stride 2                  ee_conv1x1s2_fwd_f32
    c1s2_bwd      dy, w         its input gradient                       ee_conv1x1s2_bwd_f32
    stem_fwd      x, w          conv7x7(x, w), stride 2, padding 3       ee_stem7x7s2_fwd_f32 / _fwd_stats_f32
    stem_bwd      dy, w         its input gradient                       ee_stem7x7s2_bwd_data_f32
    wrw3x3        x, dy         weight gradient of wino_fwd              ee_wrw3x3_f32 (Winograd F(3x3, 2x2))
    wrw3x3s2      x, dy[, dy1]  weight gradients of s2_fwd / pair_fwd    ee_wrw3x3s2_f32
    wrw_stem      x, dy         weight gradient of stem_fwd              ee_wrw_stem7x7s2_f32
    wrw1x1        x, dy         weight gradient of conv1x1, stride 1     ee_wrw1x1_f32

Every function returns a TUPLE of tensors, one per result of the kernel (two for pair_fwd and for wrw3x3s2 with dy1).

Two kinds of inputs:
  integer_case    small integers times powers of two, so that EVERY partial sum in ANY order is a float32 number: a kernel must return ref64 bit
                  for bit, and a mismatch is a dropped, duplicated or misplaced term (exactness_margin states the condition);
  relu_like_case  real-valued hard inputs (post-ReLU activations, channel scales 2^-10 .. 2^10, a cancelling result channel), checked element by
                  element against rounding_bound = k * 2^-24 * abs_sum with k COUNTED from the arithmetic (ROUNDINGS below), never fitted.
"""
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24

# (kernel size, stride, padding) of the convolution behind each kind
GEOMETRY = {"wino": (3, 1, 1), "s2": (3, 2, 1), "pair": (3, 2, 1), "c1s2": (1, 2, 0), "stem": (7, 2, 3), "wrw3x3": (3, 1, 1), "wrw3x3s2": (3, 2, 1),
            "wrw_stem": (7, 2, 3), "wrw1x1": (1, 1, 0)}
FWD = ("wino_fwd", "s2_fwd", "pair_fwd", "c1s2_fwd", "stem_fwd")
BWD = ("wino_bwd", "s2_bwd", "pair_bwd", "c1s2_bwd", "stem_bwd")
WRW = ("wrw3x3", "wrw3x3s2", "wrw_stem", "wrw1x1")
KINDS = FWD + BWD + WRW
WINOGRAD = ("wino_fwd", "wino_bwd", "wrw3x3")

# the transform matrices the kernel headers state: ee_wino.hip F(2x2, 3x3) (V = B^T d B, U = G g G^T, Y = A^T M A) and ee_wrw.hip F(3x3, 2x2)
# (dW = sum_t A3^T [ (G2 y G2^T) (.) (B^T d B) ] A3, the same B^T)
BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)
G2 = torch.tensor([[1, 0], [.5, .5], [.5, -.5], [0, 1]], dtype=torch.float64)
AT3 = torch.tensor([[1, 1, 1, 0], [0, 1, -1, 0], [0, 1, 1, -1]], dtype=torch.float64)

# exactness_margin counts in units of this: the smallest step between values a family's arithmetic can produce from integers.  Direct kernels multiply
# and add integers: 1.  Winograd forward / backward-data: B^T d B and A^T M A have entries 0, +-1 only, G g G^T has halves on each side: 1/4.  The
# weight gradient's transforms: B^T d B and A3^T M A3 again 0, +-1 only, G2 y G2^T halves on each side: 1/4 as well.
GRANULARITY = {k: (0.25 if k in WINOGRAD else 1.0) for k in KINDS}


def geometry(kind):
    return GEOMETRY[kind if kind in WRW else kind.rsplit("_", 1)[0]]


def out_hw(kind, H, W):
    k, s, p = geometry(kind)
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


# ---- direct float64 (or any dtype) operations ------------------------------------------------------------------------------------------------
def _fwd(x, w, k, s, p):
    return F.conv2d(x, w, None, s, p)


def _bwd(dy, w, k, s, p, hw):
    return torch.nn.grad.conv2d_input((dy.shape[0], w.shape[1]) + tuple(hw), w, dy, s, p)


def _wrw(x, dy, k, s, p):
    # dW[o][i][kh][kw] = sum_{b,oh,ow} dy[b][o][oh][ow] * x[b][i][s oh + kh - p][s ow + kw - p]
    xp = F.pad(x, (p, p, p, p))
    OH, OW = dy.shape[2], dy.shape[3]
    taps = [torch.einsum("bohw,bihw->oi", dy, xp[:, :, kh:kh + s * (OH - 1) + 1:s, kw:kw + s * (OW - 1) + 1:s]) for kh in range(k) for kw in range(k)]
    return torch.stack(taps, 2).reshape(dy.shape[1], x.shape[1], k, k)


def _direct(kind, ops, dt, mag=False):
    """the operation on `ops` (dict of tensors) in dtype dt; mag: on the operands' magnitudes (the companion sum of absolute terms)"""
    k, s, p = geometry(kind)
    t = {n: (v.to(dt).abs() if mag else v.to(dt)) for n, v in ops.items() if torch.is_tensor(v)}
    H, W = ops["shape"][3], ops["shape"][4]
    if kind in FWD:
        y = _fwd(t["x"], t["w"], k, s, p)
        return (y, _fwd(t["x"], t["w1"], 1, 2, 0)) if kind == "pair_fwd" else (y,)
    if kind in BWD:
        dx = _bwd(t["dy"], t["w"], k, s, p, (H, W))
        if kind == "pair_bwd":
            dx = dx + _bwd(t["dy1"], t["w1"], 1, 2, 0, (H, W))
        return (dx,)
    dw = _wrw(t["x"], t["dy"], k, s, p)
    return (dw, _wrw(t["x"], t["dy1"], 1, 2, 0)) if "dy1" in t else (dw,)


# ---- the Winograd restatements (any dtype; mag: every matrix and operand replaced by its magnitude, the filter transform taken first) -----------
def _patches(x):
    """[B, C, H, H] -> the 4x4 input patches (zero ring) of the (H/2)^2 output tiles: [B, C, T, T, 4, 4]"""
    return F.pad(x, (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)


def wino_f23(x, g, dt, mag=False):
    """conv3x3(x, g), stride 1, padding 1, as F(2x2, 3x3): x [B, K, H, H], g [R, K, 3, 3] -> [B, R, H, H]"""
    bt, gg, at = BT.to(dt), G.to(dt), AT.to(dt)
    u = torch.einsum("ia,rkae,je->rkij", gg, g.to(dt), gg)
    d = _patches(x.to(dt))
    if mag:
        bt, at, u, d = bt.abs(), at.abs(), u.abs(), d.abs()
    v = torch.einsum("ia,bkyxae,je->bkyxij", bt, d, bt)
    m = torch.einsum("rkij,bkyxij->bryxij", u, v)
    y = torch.einsum("pi,bryxij,qj->brypxq", at, m, at)
    B, R, T = y.shape[0], y.shape[1], y.shape[2]
    return y.reshape(B, R, 2 * T, 2 * T)


def wino_f32_wrw(x, dy, dt, mag=False):
    """weight gradient of conv3x3 (stride 1, padding 1) as F(3x3, 2x2): x [B, I, H, H], dy [B, O, H, H] -> [O, I, 3, 3]"""
    bt, gg, at = BT.to(dt), G2.to(dt), AT3.to(dt)
    yh = torch.einsum("ia,boyxae,je->boyxij", gg, dy.to(dt).unfold(2, 2, 2).unfold(3, 2, 2), gg)
    d = _patches(x.to(dt))
    if mag:
        bt, at, yh, d = bt.abs(), at.abs(), yh.abs(), d.abs()
    xh = torch.einsum("ia,bkyxae,je->bkyxij", bt, d, bt)
    m = torch.einsum("boyxij,bkyxij->okij", yh, xh)
    return torch.einsum("pi,okij,qj->okpq", at, m, at)


def _winograd(kind, ops, dt, mag=False):
    if kind == "wino_fwd":
        return (wino_f23(ops["x"], ops["w"], dt, mag),)
    if kind == "wino_bwd":  # the same product on the flipped, transposed filter (what the wino_b set holds)
        return (wino_f23(ops["dy"], ops["w"].transpose(0, 1).flip(2, 3), dt, mag),)
    return (wino_f32_wrw(ops["x"], ops["dy"], dt, mag),)


def wino_filter_sets(w):
    """float64 (U forward [16, Cin, Cout], U backward-data [16, Cout, Cin]) of a [Cout, Cin, 3, 3] filter: what ee_conv_weight_prep_f32 must write"""
    w = w.double()
    co, ci = w.shape[0], w.shape[1]
    uf = torch.einsum("ia,rkae,je->ijkr", G, w, G).reshape(16, ci, co)
    ub = torch.einsum("ia,krae,je->ijkr", G, w.flip(2, 3), G).reshape(16, co, ci)
    return uf, ub


# ---- the reference, its companion sum, the fp32 restatement -----------------------------------------------------------------------------------
def ref64(kind, case):
    """direct float64 convolution / backward-data / weight gradient of the case's float32 operands"""
    return _direct(kind, case, torch.float64)


def abs_sum(kind, case):
    """per result element, the sum of the magnitudes of the terms the family's arithmetic adds up: conv(|x|, |w|) (likewise backward-data and the
    weight gradients) for the direct kernels; for the Winograd ones the transform-domain sum
        F(2x2, 3x3):  |A^T| ( sum_ci |G g G^T| (.) (|B^T| |d| |B|) ) |A|         F(3x3, 2x2):  |A3^T| ( sum_t |G2 y G2^T| (.) (|B^T| |d| |B|) ) |A3|
    (a 2x2 map - the dense product of ee_dense.hip - is a direct kernel)."""
    if kind in WINOGRAD and not (kind != "wrw3x3" and case["shape"][3] == 2):
        return _winograd(kind, case, torch.float64, True)
    return _direct(kind, case, torch.float64, True)


def fp32_restatement(kind, case):
    """the family's arithmetic in plain float32 on the host: F.conv2d and its like for the direct kernels, the transforms for the Winograd ones"""
    if kind in WINOGRAD and not (kind != "wrw3x3" and case["shape"][3] == 2):
        return _winograd(kind, case, torch.float32)
    return _direct(kind, case, torch.float32)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------
def _ints(gen, shape, hi, p_zero):
    """integers in {-hi .. hi} without 0, then a share p_zero of exact zeros, a few of them -0.0"""
    v = torch.randint(1, hi + 1, shape, generator=gen).float() * (torch.randint(0, 2, shape, generator=gen).float() * 2 - 1)
    r = torch.rand(shape, generator=gen)
    v = torch.where(r < p_zero, torch.zeros(()), v)
    return torch.where(r < 0.02 * p_zero, -torch.zeros(()), v)


def _pow2(n, step, off):
    """n exponents cycling through [-20, 20]"""
    return torch.tensor([2.0 ** (((step * i + off) % 41) - 20) for i in range(n)])


def _shapes(kind, shape):
    B, Cin, Cout, H, W = shape
    k = geometry(kind)[0]
    OH, OW = out_hw(kind, H, W)
    return (B, Cin, H, W), (Cout, Cin, k, k), (B, Cout, OH, OW)


def integer_case(kind, shape, seed, pair=True, impulse=False, scaled=True):
    """Operands on which every partial sum, in any order, is a float32 number: activations {-3..3} (half exact zeros), filters {-2..2}, gradients
    {-2..2} (half exact zeros), a few zeros negative; each operand times a power of two that is constant over what one result element sums over -
    forward / backward-data: per image and per RESULT channel of the filter (output channel forward, input channel backward); weight gradients: per
    channel of x and per channel of dy - exponents cycling through [-20, 20].  `case["ints"]` keeps the unscaled integers (exactness_margin).
    impulse: the swept operand (x forward, dy otherwise) is one 1 per image, image b at pixel b (mod the map), in a channel that varies with b;
    pair: wrw3x3s2 with the shortcut's dy1."""
    gen = torch.Generator().manual_seed(seed)
    xs, ws, ys = _shapes(kind, shape)
    B, Cin, Cout = shape[0], shape[1], shape[2]
    ints = {}
    if kind in FWD or kind in WRW:
        ints["x"] = _ints(gen, xs, 3, 0.5)
    if kind in BWD or kind in WRW:
        ints["dy"] = _ints(gen, ys, 2, 0.5)
        if kind == "pair_bwd" or (kind == "wrw3x3s2" and pair):
            ints["dy1"] = _ints(gen, ys, 2, 0.5)
    if kind not in WRW:
        ints["w"] = _ints(gen, ws, 2, 0.2)
        if kind.startswith("pair"):
            ints["w1"] = _ints(gen, (Cout, Cin, 1, 1), 2, 0.2)
    if impulse:
        name = "x" if kind in FWD else "dy"
        t = torch.zeros_like(ints[name])
        n = t.shape[2] * t.shape[3]
        for b in range(B):
            t[b, (5 * b + 3) % t.shape[1], (b % n) // t.shape[3], (b % n) % t.shape[3]] = 1.0
        ints[name] = t
        if "dy1" in ints:
            ints["dy1"] = t.roll(1, 1)
    case = {"kind": kind, "shape": tuple(shape), "ints": ints}
    for n, v in ints.items():
        if not scaled:
            case[n] = v.clone()
        elif kind in WRW:
            c = v.shape[1]
            case[n] = v * (_pow2(c, 7, seed) if n == "x" else _pow2(c, 11, seed + 5)).view(1, c, 1, 1)
        elif n in ("x", "dy", "dy1"):
            case[n] = v * _pow2(B, 13, seed).view(B, 1, 1, 1)
        else:  # filters: per result channel
            case[n] = v * (_pow2(Cout, 11, seed + 5).view(Cout, 1, 1, 1) if kind in FWD else _pow2(Cin, 11, seed + 5).view(1, Cin, 1, 1))
    return case


def exactness_margin(kind, case):
    """max over result elements of abs_sum of the UNSCALED integers, in units of the family's granularity (GRANULARITY).  Every partial sum of every
    summation order is an integer multiple of granularity * 2^e (e the element's constant exponent) and no larger than abs_sum, so it is a float32
    number when this is < 2^24.  A condition on the cases, asserted wherever they are used."""
    ints = dict(case["ints"], shape=case["shape"])
    return max(float(a.max()) for a in abs_sum(kind, ints)) / GRANULARITY[kind]


def relu_like_case(kind, shape, seed, pair=True):
    """Real-valued hard inputs.  x = relu(randn + 1) times a per-channel scale from 2^-10 to 2^10, channel 1 nearly constant (mean 1e3 times its
    spread); filters randn / sqrt(fan_in) with result channel 2 cancelling (each of its filters sums to 0 over its taps - a 1x1 filter over its
    channels - so against activations with a large mean the result is small against its terms); dy randn times a per-channel scale (weight gradients: likewise), for backward-data about half exact zeros as behind
    a ReLU mask, channel 1 nearly constant."""
    gen = torch.Generator().manual_seed(seed)
    xs, ws, ys = _shapes(kind, shape)
    Cin, Cout = shape[1], shape[2]

    def scales(c):
        return torch.tensor([2.0 ** (((7 * i + seed) % 21) - 10) for i in range(c)]).view(1, c, 1, 1)

    def act(s, relu):
        t = torch.randn(s, generator=gen)
        t = torch.relu(t + 1) if relu else t
        if s[1] > 1:
            t[:, 1] = 1.0 + 1e-3 * torch.randn(t[:, 1].shape, generator=gen)
        return t * scales(s[1])

    def filt(s, result_dim):
        w = torch.randn(s, generator=gen) / (s[1] * s[2] * s[3]) ** 0.5
        if s[result_dim] > 2:  # result channel 2: its filters sum to about 0 - over the taps of each filter, for a 1x1 filter over the channels
            idx = [slice(None)] * 4
            idx[result_dim] = 2
            sub = w[tuple(idx)]
            sub -= sub.mean((1, 2), keepdim=True) if s[2] > 1 else sub.mean()
        return w

    case = {"kind": kind, "shape": tuple(shape)}
    if kind in FWD or kind in WRW:
        case["x"] = act(xs, True)
    if kind in BWD or kind in WRW:
        case["dy"] = act(ys, False)
        if kind in BWD:
            case["dy"] = case["dy"] * (torch.rand(ys, generator=gen) < 0.5)
        if kind == "pair_bwd" or (kind == "wrw3x3s2" and pair):
            case["dy1"] = act(ys, False) * ((torch.rand(ys, generator=gen) < 0.5) if kind in BWD else 1.0)
    if kind not in WRW:
        rd = 0 if kind in FWD else 1
        case["w"] = filt(ws, rd)
        if kind.startswith("pair"):
            case["w1"] = filt((Cout, Cin, 1, 1), rd)
    return case


# ---- the rounding bound -----------------------------------------------------------------------------------------------------------------------
def reduction_length(kind, case):
    """per result of the kernel (a tuple like ref64's): the number of products one result element adds up, at most (zero-ring terms are exact zeros:
    adding one does not round)"""
    n = _reduction_length(kind, case)
    if kind == "pair_fwd":
        return (n, case["shape"][1])  # the shortcut's 1x1 output: Cin products
    if kind == "wrw3x3s2" and "dy1" in case:
        return (n, n)  # both weight gradients sum over the same output pixels
    return (n,)


def _reduction_length(kind, case):
    B, Cin, Cout, H, W = case["shape"]
    OH, OW = out_hw(kind, H, W)
    if kind in ("wino_fwd", "wino_bwd"):
        c = Cin if kind == "wino_fwd" else Cout
        return (min(H, 3) ** 2) * c if H == 2 else c  # the dense product of a 2x2 map: 4 pixels x channels; Winograd: channels per transform point
    if kind in ("s2_fwd", "pair_fwd"):
        return 9 * Cin
    if kind in ("s2_bwd", "pair_bwd"):
        return 4 * Cout + (Cout if kind == "pair_bwd" else 0)  # stride 2: at most 2 x 2 taps of the 3 x 3 window reach one input pixel
    if kind == "c1s2_fwd":
        return Cin
    if kind == "c1s2_bwd":
        return Cout
    if kind == "stem_fwd":
        return 49 * Cin
    if kind == "stem_bwd":
        return 16 * Cout  # stride 2: at most 4 x 4 taps of the 7 x 7 window reach one input pixel
    if kind == "wrw3x3":
        return B * (max(H, 2) // 2) ** 2  # tiles
    return B * OH * OW  # wrw3x3s2, wrw_stem, wrw1x1: output pixels


def roundings(kind, case):
    """k per result of the kernel (a tuple like ref64's): the number of float32 roundings on the longest path from the operands to one element
    of that result, whatever the order of the sums.
      direct kernels   n products (1 rounding each, 0 where fused) + n - 1 additions, every path through ONE product and at most n - 1 additions:
                       k = n; + 1 for the second-order term of (1 + u)^n - 1 <= (n + 1) u, which holds while n^2 u < 1 (n < 4096, asserted)
      F(2x2, 3x3)      U = G g G^T: 2 additions per side = 4;  V = B^T d B: 1 per side = 2;  1 product;  KC - 1 additions over the channels;
                       Y = A^T M A: 2 additions per side = 4:  k = KC + 10, + 1 as above
      F(3x3, 2x2)      G2 y G2^T: 1 addition per side = 2;  B^T d B: 2;  1 product;  T - 1 additions over the tiles (the workgroups' partial sums
                       and the fixed-order sum kernel are part of them);  A3^T M A3: 2 per side = 4:  k = T + 8, + 1 as above"""
    ns = reduction_length(kind, case)
    assert max(ns) < 4096
    if kind in ("wino_fwd", "wino_bwd") and case["shape"][3] != 2:
        return tuple(n + 10 + 1 for n in ns)
    if kind == "wrw3x3":
        return tuple(n + 8 + 1 for n in ns)
    return tuple(n + 1 for n in ns)


def rounding_bound(kind, case):
    """k * 2^-24 * abs_sum per result element (a tuple like ref64's)"""
    return tuple(k * U24 * a for k, a in zip(roundings(kind, case), abs_sum(kind, case)))


# ---- reading a mismatch ------------------------------------------------------------------------------------------------------------------------
def describe_mismatch(kind, case, got, ref, part=0, group=1):
    """message for got != ref (float64 tensors): count, first differing index, the image group (`group` images per workgroup), 32-channel block and
    2x2 tile it falls in, and the float64 result there split by tap (weight gradients: by image)"""
    bad = (got != ref) | (torch.isnan(got) != torch.isnan(ref))
    idx = tuple(int(i) for i in bad.nonzero()[0])
    msg = ["%s part %d shape %s: %d of %d elements differ; first at %s: got %r, want %r" % (
        kind, part, case["shape"], int(bad.sum()), bad.numel(), idx, float(got[idx]), float(ref[idx]))]
    k, s, p = (1, 2, 0) if part == 1 else geometry(kind)
    t = {n: v.double() for n, v in case.items() if torch.is_tensor(v)}
    w = t.get("w1" if part == 1 else "w")
    if kind in WRW:
        co, ci, kh, kw = idx
        dy = t["dy1" if part == 1 else "dy"]
        per = _wrw_per_image(t["x"][:, ci:ci + 1], dy[:, co:co + 1], k, s, p)[:, kh, kw]
        msg.append("channel blocks (co %d, ci %d) of 32; per image: %s" % (co // 32, ci // 32, [float(v) for v in per]))
    else:
        b, c, h, x_ = idx
        msg.append("image group %d (image %d of %d in it), channel block %d of 32, tile (%d, %d), pixel (%d, %d) of the tile" % (
            b // group, b % group, group, c // 32, h // 2, x_ // 2, h % 2, x_ % 2))
        taps = torch.zeros(k, k, dtype=torch.float64)
        for kh in range(k):
            for kw in range(k):
                if kind in FWD:
                    ih, iw = s * h + kh - p, s * x_ + kw - p
                    if 0 <= ih < t["x"].shape[2] and 0 <= iw < t["x"].shape[3]:
                        taps[kh, kw] = (t["x"][b, :, ih, iw] * w[c, :, kh, kw]).sum()
                else:
                    dy = t["dy1" if (part == 1 or (kind == "pair_bwd" and k == 1)) else "dy"]
                    oh, ow = h + p - kh, x_ + p - kw
                    if oh % s == 0 and ow % s == 0 and 0 <= oh // s < dy.shape[2] and 0 <= ow // s < dy.shape[3]:
                        taps[kh, kw] = (dy[b, :, oh // s, ow // s] * w[:, c, kh, kw]).sum()
        msg.append("float64 by tap: %s" % taps.tolist())
    return "\n".join(msg)


def _wrw_per_image(x, dy, k, s, p):
    xp = F.pad(x, (p, p, p, p))
    OH, OW = dy.shape[2], dy.shape[3]
    return torch.stack([torch.einsum("bohw,bihw->b", dy, xp[:, :, kh:kh + s * (OH - 1) + 1:s, kw:kw + s * (OW - 1) + 1:s])
                        for kh in range(k) for kw in range(k)], 1).reshape(-1, k, k)


def same_values(got, ref):
    """torch.equal on values: signed zeros compare equal, NaNs do not occur"""
    return got.shape == ref.shape and bool((got == ref).all())


# ---- the cases the GPU tests use (shared with the host test, which asserts their exactness) -------------------------------------------------------
def _c(kind, shape, **kw):
    return (kind, tuple(shape), tuple(sorted(kw.items())))


def gpu_integer_cases():
    """[(kind, shape, options)] of every integer case tests/test_gpu_conv_exact.py runs (impulse sweeps included)"""
    cases = []
    for H, Bs in ((4, (1, 3, 4, 5)), (8, (1, 3)), (16, (1, 2, 3))):  # images per workgroup: 4, 2, 1
        for kind in ("wino_fwd", "wino_bwd"):
            cases += [_c(kind, (B, 32, 32, H, H)) for B in Bs]
            kc = {"wino_fwd": lambda c: (3, c, 32, H, H), "wino_bwd": lambda c: (3, 32, c, H, H)}[kind]
            cases += [_c(kind, kc(c)) for c in (16, 48)]  # reduction channels: an odd number of 16-channel rounds (32: above)
            rc = {"wino_fwd": (3, 32, 96, H, H), "wino_bwd": (3, 96, 32, H, H)}[kind]
            cases.append(_c(kind, rc))  # three result channel blocks against the eight-way numbering
            cases.append(_c(kind, (H * H, 32, 32, H, H), impulse=True))
            if H == 16:  # B H H > 4608 at 96 result channels: xcd_decode's eight-way numbering with three channel blocks (smaller batches keep
                cases.append(_c(kind, (19, 32, 96, H, H) if kind == "wino_fwd" else (19, 96, 32, H, H)))  # the plain block numbering)
        for kind in ("s2_fwd", "s2_bwd", "pair_fwd", "pair_bwd"):
            cases += [_c(kind, (B, 32, 32, H, H)) for B in (1, 3, 9)]
            cases += [_c(kind, (3, 32, 96, H, H)), _c(kind, (3, 96, 32, H, H))]
            if kind in ("s2_fwd", "s2_bwd"):  # 48 reduction channels through ops
                cases.append(_c(kind, (3, 48, 32, H, H) if kind == "s2_fwd" else (3, 32, 48, H, H)))
            n = H * H if kind.endswith("fwd") else (H // 2) ** 2
            cases.append(_c(kind, (n, 32, 32, H, H), impulse=True))
    for shape in C1S2_SHAPES:
        cases += [_c("c1s2_fwd", shape), _c("c1s2_bwd", shape)]
    cases += [_c("c1s2_fwd", (10 * 6, 6, 34, 10, 6), impulse=True), _c("c1s2_bwd", (5 * 3, 6, 34, 10, 6), impulse=True)]
    cases += [_c("stem_fwd", (B, 3, K, H, W)) for B, K, H, W in STEM_FWD_SHAPES]
    cases += [_c("stem_bwd", (B, 3, K, H, W)) for B, K, H, W in STEM_BWD_SHAPES]
    cases += [_c("stem_fwd", (6 * 128, 3, 64, 6, 128), impulse=True), _c("stem_bwd", (35 * 33, 3, 6, 70, 66), impulse=True)]
    for B, Cin, Cout in DENSE_SHAPES:
        cases.append(_c("wino_fwd", (B, Cin, Cout, 2, 2)))
        if Cout % 128 == 0:
            cases.append(_c("wino_bwd", (B, Cin, Cout, 2, 2)))
    cases += [_c("wino_fwd", (4, 128, 128, 2, 2), impulse=True), _c("wino_bwd", (4, 128, 128, 2, 2), impulse=True)]
    for H in (2, 4, 8, 16):
        for B in (1, 5, 37):
            cases.append(_c("wrw3x3", (B, 32, 32, H, H)))
        cases.append(_c("wrw3x3", (5, 96, 32, H, H)))
        cases.append(_c("wrw3x3", (H * H, 32, 32, H, H), impulse=True))
    for H in (4, 8, 16):
        for pair in (True, False):
            cases += [_c("wrw3x3s2", (B, 32, 32, H, H), pair=pair) for B in (1, 5, 37)]
            cases.append(_c("wrw3x3s2", (5, 96, 32, H, H), pair=pair))
        cases.append(_c("wrw3x3s2", ((H // 2) ** 2, 32, 32, H, H), pair=True, impulse=True))
    cases += [_c("wrw_stem", (B, 3, 64, H, W)) for B, H, W in WRW_STEM_SHAPES]
    cases.append(_c("wrw_stem", (16 * 16, 3, 64, 32, 32), impulse=True))
    cases += [_c("wrw1x1", s) for s in WRW1X1_SHAPES]
    cases.append(_c("wrw1x1", (4, 128, 64, 2, 2), impulse=True))
    return cases


C1S2_SHAPES = [(3, 6, 34, 10, 6), (2, 130, 200, 4, 4), (1, 256, 64, 4, 4), (1, 64, 256, 4, 4)]  # the last: the backward's Kdim >= 256 side
STEM_BWD_SHAPES = [(2, 5, 10, 6), (1, 64, 2, 2), (2, 17, 70, 66)]
STEM_FWD_SHAPES = [(1, 64, 2, 64), (3, 128, 10, 64), (2, 64, 6, 128)]
DENSE_SHAPES = [(1, 128, 8), (5, 128, 128), (33, 256, 512)]
WRW_STEM_SHAPES = [(1, 32, 32), (5, 34, 96)]
WRW1X1_SHAPES = [(1, 128, 64, 2, 2), (5, 64, 192, 10, 14)]


def make_integer(kind, shape, opts, seed=None):
    return integer_case(kind, shape, (sum(shape) + len(kind)) if seed is None else seed, **dict(opts))


# ---- the C-ABI argument lists the guard-band harness passes (roles in the order of include/eeadv.h) ----------------------------------------------
# "out" / "out1": result buffers (carved from a guarded buffer), "ws": workspace (likewise), other pointer roles: operands; the rest: integers
ABI_ARGS = {
    "ee_wino3x3_f32": ("x", "u", "out", "B", "KC", "RC", "H", "stream"),
    "ee_dense2x2_f32": ("x", "w2", "out", "B", "Cin", "Cout", "stream"),
    "ee_conv3x3s2_small_fwd_f32": ("x", "w9", "out", "B", "Cin", "Cout", "H", "stream"),
    "ee_conv3x3s2_small_bwd_data_f32": ("dy", "w9", "out", "B", "Cin", "Cout", "H", "stream"),
    "ee_conv3x3s2_pair_fwd_f32": ("x", "w10", "out", "out1", "B", "Cin", "Cout", "H", "stream"),
    "ee_conv3x3s2_pair_bwd_data_f32": ("dy", "dy1", "w10", "out", "B", "Cin", "Cout", "H", "stream"),
    "ee_conv1x1s2_fwd_f32": ("x", "w", "out", "B", "Cin", "Cout", "H", "W", "stream"),
    "ee_conv1x1s2_bwd_f32": ("dy", "w", "out", "B", "Cin", "Cout", "H", "W", "stream"),
    "ee_stem7x7s2_fwd_f32": ("x", "w", "out", "B", "K", "H", "W", "stream"),
    "ee_stem7x7s2_fwd_stats_f32": ("x", "w", "out", "ws", "B", "K", "H", "W", "stream"),
    "ee_stem7x7s2_bwd_data_f32": ("dy", "w", "out", "B", "K", "H", "W", "stream"),
    "ee_wrw3x3_f32": ("x", "dy", "out", "ws", "B", "Cin", "Cout", "H", "stream"),
    "ee_wrw3x3s2_f32": ("x", "dy", "dy1", "out", "ws", "B", "Cin", "Cout", "H", "stream"),
    "ee_wrw_stem7x7s2_f32": ("x", "dy", "out", "ws", "B", "H", "W", "stream"),
    "ee_wrw1x1_f32": ("x", "dy", "out", "ws", "B", "Cin", "Cout", "HW", "stream"),
    "ee_conv_weight_prep_f32": ("kind", "w", "extra", "out", "Cout", "Cin", "stream"),
}


def gpu_relu_cases():
    """[(kind, shape, options)] of every ReLU-like case tests/test_gpu_conv_exact.py runs"""
    cases = []
    for H in (4, 8, 16):
        cases += [_c("wino_fwd", (3, 32, 96, H, H)), _c("wino_bwd", (3, 96, 32, H, H)), _c("wino_fwd", (5, 48, 32, H, H))]
        for kind in ("s2_fwd", "s2_bwd", "pair_fwd", "pair_bwd"):
            cases += [_c(kind, (3, 32, 32, H, H)), _c(kind, (9, 96, 32, H, H))]
        cases += [_c("wrw3x3s2", (5, 96, 32, H, H), pair=True), _c("wrw3x3s2", (37, 32, 32, H, H), pair=False)]
    for H in (2, 4, 8, 16):
        cases += [_c("wrw3x3", (5, 32, 32, H, H)), _c("wrw3x3", (37, 96, 32, H, H))]
    for shape in C1S2_SHAPES:
        cases += [_c("c1s2_fwd", shape), _c("c1s2_bwd", shape)]
    cases += [_c("stem_fwd", (B, 3, K, H, W)) for B, K, H, W in STEM_FWD_SHAPES]
    cases += [_c("stem_bwd", (B, 3, K, H, W)) for B, K, H, W in STEM_BWD_SHAPES]
    for B, Cin, Cout in DENSE_SHAPES:
        cases.append(_c("wino_fwd", (B, Cin, Cout, 2, 2)))
        if Cout % 128 == 0:
            cases.append(_c("wino_bwd", (B, Cin, Cout, 2, 2)))
    cases += [_c("wrw_stem", (B, 3, 64, H, W)) for B, H, W in WRW_STEM_SHAPES]
    cases += [_c("wrw1x1", s) for s in WRW1X1_SHAPES]
    return cases


def make_relu(kind, shape, opts):
    return relu_like_case(kind, shape, sum(shape) + len(kind), **dict(opts))
