"""A float64 bar for BatchNorm and the inputs on which BatchNorm kernels go wrong (tests/test_bn_reference_host.py checks this module on
the CPU, tests/test_gpu_bn_hard_channels.py holds every statistics path of ee_bn.hip / ee_fuse.hpp against it).

hard_input    channels cycle through five kinds (KINDS): a constant channel (variance exactly 0), one whose mean is 128 standard
              deviations from zero, one whose first image is shifted and scaled (partial means differ: the cross term of Chan's update
              dominates the variance), one whose last image is constant, and the distribution the rest of the suite draws.
hard_affine   gamma of both signs and zero, beta of both signs and zero.
bn_ref64      [x + res_in] -> batch_norm -> [+ residual] -> [relu] composed from plain float64 torch operations, train or eval mode, with
              the backward from float64 autograd on a ReLU branch the CALLER fixes (the fp32 kernel's own y > 0, as tests/branch_replay.py
              does for whole networks): one pre-activation within rounding of zero cannot flip a whole gradient sum.
deal, gather_back, rank_param_grads64
              SyncBatchNorm over simulated ranks: the batch dealt to W ranks, the ranks' results put back into whole-batch tensors, and
              each rank's float64 share of dgamma / dbeta.  The bar stays bn_ref64 over the whole batch.
"""
import numpy as np
import torch

KINDS = ("const", "offset", "outlier", "tail", "plain")
CONST = 0.75
GAMMA_CYCLE = (-1.25, 0.0, 0.0, 0.75, -0.5, 1.5)
BETA_CYCLE = (0.3, 0.4, -0.4, -0.2, 0.0, 0.1)
TIE_BAND = 1e-4   # |pre-activation| at or below this: the fp32 mask may legitimately differ from the float64 one
TIE_CAP = 1e-3    # share of such elements (channels with gamma != 0) a seeded case may have
STAT_FLOOR = (1e-5, 1e-6)  # (rtol, atol) on mean / invstd / variance / running statistics: test_bn_act_matches_torch's, see the GPU module


def kinds(C, roll=0):
    """the kind of every channel; `roll` shifts the cycle (the two sides of bn_dual get different kinds per channel)"""
    return [KINDS[(c + roll) % len(KINDS)] for c in range(C)]


def hard_input(B, C, H, W, seed, roll=0):
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(B, C, H, W, generator=g)
    x = torch.empty_like(r)
    for c, k in enumerate(kinds(C, roll)):
        if k == "const":
            x[:, c] = CONST  # every partial sum n * 0.75 is exact in fp32 (n < 2^22): mean == 0.75, M2 == 0
        elif k == "offset":
            x[:, c] = 32.0 + 0.25 * r[:, c]  # |mean| / std = 128
        elif k == "outlier":
            x[:, c] = r[:, c]
            x[0, c] = r[0, c] * 4.0 + 16.0  # one partial with another mean and spread
        elif k == "tail":
            x[:, c] = r[:, c]
            x[B - 1, c] = -3.0  # the last slice / partial is constant
        else:
            x[:, c] = r[:, c] * 2.0 + 0.5
    return x


def hard_affine(C, roll=0):
    gamma = torch.tensor([GAMMA_CYCLE[(c + roll) % len(GAMMA_CYCLE)] for c in range(C)], dtype=torch.float32)
    beta = torch.tensor([BETA_CYCLE[(c + roll) % len(BETA_CYCLE)] for c in range(C)], dtype=torch.float32)
    return gamma, beta


def hard_running(C):
    """running statistics to start from (eval mode reads them): means of both signs, variances in [0.5, 1.25]"""
    c = torch.arange(C, dtype=torch.float32)
    return 0.125 * (c % 3 - 1.0), 0.5 + 0.25 * (c % 4)


def hard_case(shape, seed, roll=0):
    """everything a BatchNorm test feeds, from one seed (fp32, CPU): x, a residual, the incoming gradient, the affine pair and the
    running statistics.  The gradient is the constant 0.5 on `const` channels: with a constant x the masked gradient dz is then constant
    too, its mean equals it exactly, and the train-mode dx = gamma * invstd * ((dz - mean dz) - xhat * mean(dz xhat)) is exactly 0."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed + 7919)
    x = hard_input(B, C, H, W, seed, roll)
    residual = torch.randn(shape, generator=g)
    dy = torch.randn(shape, generator=g)
    for c, k in enumerate(kinds(C, roll)):
        if k == "const":
            dy[:, c] = 0.5
    gamma, beta = hard_affine(C, roll)
    rm, rv = hard_running(C)
    return {"x": x, "residual": residual, "dy": dy, "gamma": gamma, "beta": beta, "rm": rm, "rv": rv, "kinds": kinds(C, roll)}


def split_sum(s, seed):
    """(x, res) with fp32 x + res == s wherever s - res is exact (always on `const` channels: res is a multiple of 0.25 in [-2, 2])"""
    g = torch.Generator().manual_seed(seed + 104729)
    res = torch.round(torch.randn(s.shape, generator=g).clamp(-2, 2) * 4.0) / 4.0
    return s - res, res


def exact_addends(t):
    """(hi, lo) with fp32 hi + lo == t bit for bit: hi keeps the upper half of t's significand, lo = t - hi is the rest (exact)"""
    hi = (t.contiguous().view(torch.int32) & -4096).view(torch.float32)
    return hi, t - hi


def eps32(eps):
    """the eps the kernels see: they take it as a C float"""
    return float(np.float32(eps))


def _bc(v):
    return v.view(1, -1, 1, 1)


def bn_ref64(x, gamma, beta, running_mean, running_var, momentum, eps, training, res_in=None, residual=None, relu=True, dy=None, mask=None):
    """float64 [x + res_in] -> batch_norm -> [+ residual] -> [relu].  Returns a dict: y, pre (y before the ReLU), mean, var (biased), invstd,
    running_mean / running_var after the call (unbiased variance, as nn.BatchNorm2d), and - with dy - dx (also the gradient of res_in),
    dresidual, dgamma, dbeta from autograd through the composition with the ReLU replaced by the fixed 0/1 `mask`."""
    d = lambda t: None if t is None else t.detach().double()
    x, gamma, beta, rm, rv, res_in, residual = d(x), d(gamma), d(beta), d(running_mean), d(running_var), d(res_in), d(residual)
    C = x.shape[1]
    if gamma is None:
        gamma = torch.ones(C, dtype=torch.float64, device=x.device)
    if beta is None:
        beta = torch.zeros(C, dtype=torch.float64, device=x.device)
    eps = eps32(eps)
    momentum = float(np.float32(momentum))
    leaves = [t.requires_grad_(True) for t in (x, gamma, beta)]
    if residual is not None:
        residual.requires_grad_(True)
    s = x if res_in is None else x + res_in
    n = s.numel() // C
    if training:
        mean = s.mean((0, 2, 3))
        var = ((s - _bc(mean)) ** 2).mean((0, 2, 3))
        new_rm = new_rv = None
        if rm is not None:
            new_rm = (1.0 - momentum) * rm + momentum * mean.detach()
            new_rv = (1.0 - momentum) * rv + momentum * var.detach() * (n / (n - 1.0) if n > 1 else 1.0)
    else:
        mean, var, new_rm, new_rv = rm, rv, rm, rv
    invstd = 1.0 / torch.sqrt(var + eps)
    pre = (s - _bc(mean)) * _bc(invstd) * _bc(gamma) + _bc(beta)
    if residual is not None:
        pre = pre + residual
    y = torch.relu(pre) if relu else pre
    out = {"y": y.detach(), "pre": pre.detach(), "mean": mean.detach(), "var": var.detach(), "invstd": invstd.detach(),
           "running_mean": new_rm, "running_var": new_rv}
    if dy is not None:
        if relu:
            if mask is None:
                raise ValueError("bn_ref64: the backward through a ReLU needs the branch to hold fixed (mask)")
            routed = pre * mask.to(pre.device).double()
        else:
            routed = pre
        ins = leaves + ([residual] if residual is not None else [])
        grads = torch.autograd.grad(routed, ins, d(dy))
        out.update(dx=grads[0], dgamma=grads[1], dbeta=grads[2], dresidual=grads[3] if residual is not None else None)
    return out


def tie_share(pre64, gamma, leave_out=()):
    """share of pre-activations within TIE_BAND of zero, over the channels with gamma != 0 that are not in `leave_out`"""
    live = gamma.detach().cpu() != 0
    live[list(leave_out)] = False
    if not bool(live.any()):
        return 0.0
    p = pre64.detach().cpu()[:, live]
    return float((p.abs() <= TIE_BAND).double().mean())


# ---- SyncBatchNorm over simulated ranks: the batch dealt to W ranks, the bar still bn_ref64 over the whole batch ------------------------
def deal(B, sizes=None, stride=None):
    """a partition of range(B), one index list per rank: `sizes` images per rank in order, or `stride` ranks dealt range(r, B, stride)"""
    if stride is not None:
        return [list(range(r, B, stride)) for r in range(stride)]
    assert sum(sizes) == B and min(sizes) > 0
    starts = [sum(sizes[:r]) for r in range(len(sizes))]
    return [list(range(b, b + n)) for b, n in zip(starts, sizes)]


def gather_back(pieces, parts):
    """the whole-batch tensor whose images parts[r] are pieces[r]"""
    B = sum(len(idx) for idx in parts)
    whole = torch.empty((B,) + tuple(pieces[0].shape[1:]), dtype=pieces[0].dtype, device=pieces[0].device)
    for piece, idx in zip(pieces, parts):
        whole[idx] = piece
    return whole


def rank_param_grads64(x, mean, invstd, dy, mask, parts, dy2=None):
    """what each rank adds to the parameter gradients, float64: (dgamma_r, dbeta_r), each [W, C], with dbeta_r = sum over the rank's images
    of dz and dgamma_r = sum of dz * xhat, where dz = (dy [+ dy2]) * mask and xhat = (x - mean) * invstd on the GLOBAL float64 statistics
    (bn_ref64's mean / invstd).  Over the ranks they add up to bn_ref64's dgamma / dbeta on the same mask."""
    d = lambda t: t.detach().double()
    dz = d(dy) if dy2 is None else d(dy) + d(dy2)
    if mask is not None:
        dz = dz * mask.to(dz.device).double()
    prod = dz * ((d(x) - _bc(d(mean))) * _bc(d(invstd)))
    return torch.stack([prod[idx].sum((0, 2, 3)) for idx in parts]), torch.stack([dz[idx].sum((0, 2, 3)) for idx in parts])


# ---- the seeded cases of tests/test_gpu_bn_hard_channels.py (the host test holds every one of them under TIE_CAP) ----------------------
# ee_bn_act_*: name -> (shape, seed); the dispatch branch each reaches is the name
BN_ACT_CASES = {
    "cached<256,2>": ((2, 6, 16, 16), 11),
    "cached<256,7>": ((12, 6, 16, 16), 12),
    "cached<1024,7>": ((40, 6, 16, 16), 13),
    "cached<1024,7>-edge": ((28, 6, 32, 32), 14),
    "split-4-slices": ((33, 6, 30, 30), 15),
    "scalar<256,1>": ((3, 6, 5, 7), 16),
    "scalar<1024,1>": ((68, 6, 15, 17), 17),
}
BN_DUAL_CASE = ((9, 6, 4, 8), 21)  # side b rolls the channel cycle by 2
BN_SUM_CASES = {"cached<256,2>": ((2, 6, 16, 16), 31), "cached<256,7>": ((12, 6, 16, 16), 32), "cached<1024,7>": ((40, 6, 16, 16), 33)}
BN_POOL_CASES = {"one-group": ((3, 6, 8, 12), 41), "two-images-per-group": ((70, 6, 6, 8), 42)}
STEM_CASE = ((3, 3, 10, 64), 64, 51)  # x shape, K, seed
WINO_CASES = {16: 61, 8: 62, 4: 63}   # H -> seed (B = 3)
PAIR_CASES = {16: 71, 8: 72}          # H -> seed (B = 3, 32 -> 64 channels)
# ee_syncbn_*: name -> (shape, seed), train mode, with and without a residual; SYNC_DEALS: name -> {label: images per rank, in rank order}.
# A rank's shard runs in split_slices(B_r * H * W / 4 / 2048) slices (the S of the labels); a slice boundary may lie inside an image.
# [4, 3, 1] and [5, 3, 1] leave the `tail` kind's constant last image alone on a rank; the contiguous deals keep the `outlier` kind's
# shifted first image on rank 0 only, so the cross term of the rank merge carries that channel's variance.
SYNC_CASES = {
    "one-slice": ((8, 6, 4, 4), 81),
    "hw4": ((9, 6, 2, 2), 82),            # H * W == 4: one quad per image and channel
    "two-slices": ((7, 6, 56, 56), 83),
    "four-slices": ((12, 6, 56, 56), 84),
    "channels-70": ((4, 70, 4, 4), 85),   # the per-channel kernels' second 64-thread block, 6 of its threads in use
}
SYNC_DEALS = {
    "one-slice": {"[8]": deal(8, [8]), "[4,4]": deal(8, [4, 4]), "strided-2": deal(8, stride=2), "[2,2,2,2]": deal(8, [2, 2, 2, 2]), "[4,3,1]": deal(8, [4, 3, 1])},
    "hw4": {"[5,3,1]": deal(9, [5, 3, 1])},
    "two-slices": {"[4,3] S=2,2": deal(7, [4, 3]), "[5,2] S=2,1": deal(7, [5, 2])},
    "four-slices": {"[9,3] S=4,2": deal(12, [9, 3])},  # S = 4: slices of 2.25 images
    "channels-70": {"[2,2]": deal(4, [2, 2]), "[3,1]": deal(4, [3, 1])},
}
# channels-70: with 70 channels the kind cycle (5) and the beta cycle (6) meet at channels 10 and 40 - `const` with beta == 0 and gamma
# == -0.5.  Without a residual their 128 pre-activations are exactly 0 in float64, which tie_share counts as ties (4.4e-2 of the case).
# They are none: fp32 gives exactly 0 there as well (x - mean == 0), the mask is closed on both sides, and the GPU test's exact check
# y == relu(beta) covers them.  The tie count of this case therefore leaves `const` channels out, and is then 0 (the host test asserts it).
SYNC_TIES_LEAVE_OUT_CONST = ("channels-70",)


def shaped_conv_operands(x_shape, w_shape, seed, fan_in):
    """operands that shape a convolution's raw output - the BatchNorm input - without setting it: post-ReLU input plus a constant (result
    channels get an offset), image 0 eight times larger (unequal partials), the filters of result channels 0 and 5 zero (constant-0
    channels)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(x_shape, generator=g)) + 0.5
    x[0] *= 8.0
    w = torch.randn(w_shape, generator=g) * (2.0 / fan_in) ** 0.5
    w[0] = 0.0
    w[5] = 0.0
    return x, w


ZERO_FILTER_CHANNELS = (0, 5)
