"""float64 restatements, in plain torch, of what the eval-mode fused convolution kernels compute (ee_wino3x3_bn_eval_*, ee_dense2x2_bn_eval_*,
ee_conv3x3s2_pair_bn_eval_*): the bar of tests/test_gpu_eval_route.py.  tests/test_eval_route_reference_host.py holds this module against
float64 nn.Conv2d / nn.BatchNorm2d(eval) / F.relu autograd on the CPU, so that the bar is right before anything runs on a GPU.

Every ReLU is given from outside: a boolean mask, or the tensor whose sign gives it (the fp32 kernel's own output - `y > 0`), as
tests/branch_replay.py does for whole networks.  Nothing here calls an ee_* kernel.

    forward     pre = (conv2d(x, w) - rm) / sqrt(rv + eps) * g + b [+ res];  y = pre where the mask holds, 0 elsewhere
    backward    dz = (dy [+ dy2]) * mask;  dres = dz;  dx = conv2d_input(dz * g / sqrt(rv + eps)) [+ dx_add]
    pair        the same for the 3x3 / stride 2 / padding 1 and the 1x1 / stride 2 convolution of a down-sampling block, which read the same
                x: (pre3, pre1) forward - only pre3 is followed by a ReLU - and one summed dx backward

eps is the float the kernels take (bn_reference.eps32)."""
import torch
import torch.nn.functional as F

from bn_reference import eps32


def _d(t):
    return None if t is None else t.detach().double()


def _bc(v):
    return v.view(1, -1, 1, 1)


def as_mask(m):
    """a boolean mask as it is; any other tensor stands for `m > 0` (NaN: closed)"""
    return m if m.dtype == torch.bool else m > 0


def bn_scale64(rv, g, eps):
    """g / sqrt(rv + eps) per channel (g None: 1)"""
    s = 1.0 / torch.sqrt(_d(rv) + eps32(eps))
    return s if g is None else s * _d(g)


def bn_eval64(c, rm, rv, g, b, eps):
    """(c - rm) / sqrt(rv + eps) * g + b on a float64 c (g, b None: 1, 0)"""
    z = (c - _bc(_d(rm))) / _bc(torch.sqrt(_d(rv) + eps32(eps)))
    if g is not None:
        z = z * _bc(_d(g))
    return z if b is None else z + _bc(_d(b))


def gate(pre, mask):
    """pre where the mask holds, 0 elsewhere (a NaN under a closed gate stays: 0 * NaN)"""
    return pre * as_mask(mask).to(pre.dtype)


def conv_bn_fwd64(x, w, bn, res=None, stride=1, padding=1):
    """bn = (rm, rv, g, b, eps) -> the pre-activation bn(conv2d(x, w)) [+ res] in float64"""
    rm, rv, g, b, eps = bn
    pre = bn_eval64(F.conv2d(_d(x), _d(w), stride=stride, padding=padding), rm, rv, g, b, eps)
    return pre if res is None else pre + _d(res)


def conv_bn_bwd64(dy, dy2, mask, w, bn, in_shape, dx_add=None, stride=1, padding=1):
    """bn = (rv, g, eps); mask None: no ReLU behind the BatchNorm -> (dx [+ dx_add], dz) in float64; dz is the residual's gradient"""
    rv, g, eps = bn
    dz = _d(dy) if dy2 is None else _d(dy) + _d(dy2)
    if mask is not None:
        dz = dz * as_mask(mask).to(dz.dtype)
    dx = torch.nn.grad.conv2d_input(tuple(in_shape), _d(w), dz * _bc(bn_scale64(rv, g, eps)), stride=stride, padding=padding)
    return (dx if dx_add is None else dx + _d(dx_add)), dz


def pair_fwd64(x, w3, w1, bn3, bn1):
    """(bn3(conv3x3 / stride 2 / padding 1 (x)), bn1(conv1x1 / stride 2 (x))): both pre-activations; the kernel's first output is relu of the first"""
    return conv_bn_fwd64(x, w3, bn3, None, 2, 1), conv_bn_fwd64(x, w1, bn1, None, 2, 0)


def pair_bwd64(dy3, mask3, dy1, w3, w1, bn3, bn1, in_shape):
    """bn = (rv, g, eps) each -> dx = conv3x3s2^T(g3 / sqrt(rv3 + eps) * mask3 * dy3) + conv1x1s2^T(g1 / sqrt(rv1 + eps) * dy1)"""
    dx3, _ = conv_bn_bwd64(dy3, None, mask3, w3, bn3, in_shape, None, 2, 1)
    dx1, _ = conv_bn_bwd64(dy1, None, None, w1, bn1, in_shape, None, 2, 0)
    return dx3 + dx1


def edge_statistics(C, gen, gamma=None, spread=1.5):
    """running statistics (mean, var) for a [C] BatchNorm with three hard channels, placed on the first three channels whose gamma is not 0
    (a zero gamma would hide them): variance 1e-6 (below eps's scale: invstd = 1 / sqrt(1.1e-5)), variance 1e3, and a mean 50 times the
    activations' `spread` from zero (cancellation in c - rm).  The rest as test_gpu_evalfuse._bn draws them."""
    rm = torch.randn(C, generator=gen) * 0.2
    rv = torch.rand(C, generator=gen) + 0.3
    live = [c for c in range(C) if gamma is None or float(gamma[c]) != 0.0][:3]
    assert len(live) == 3
    rv[live[0]], rv[live[1]], rm[live[2]] = 1e-6, 1e3, 50.0 * spread
    return rm, rv, live
