"""The feature-denoising product (ImageNet/models_imagenet/resnet_fd.py:133-148 with embed=False, softmax=False) restated in float64 torch:
both associations of F = s X X^T X and both forms of its input gradient, per sample on [N, C, P] tensors.  Shared by the host and the -m gpu
tests; nothing here touches a device."""
import numpy as np
import torch


def fwd_channel(x, s):
    """(X X^T) X: the reference's association for n_in <= H * W"""
    x = x.double()
    return torch.matmul(torch.matmul(x, x.transpose(1, 2)), x) * s


def fwd_spatial(x, s):
    """X (X^T X): the reference's association for n_in > H * W"""
    x = x.double()
    return torch.matmul(x, torch.matmul(x.transpose(1, 2), x)) * s


def bwd_channel(x, d, s):
    """s [(M + M^T) X + G D], G = X X^T, M = D X^T"""
    x, d = x.double(), d.double()
    g, m = torch.matmul(x, x.transpose(1, 2)), torch.matmul(d, x.transpose(1, 2))
    return (torch.matmul(m + m.transpose(1, 2), x) + torch.matmul(g, d)) * s


def bwd_spatial(x, d, s):
    """s [D A + X (B + B^T)], A = X^T X, B = D^T X"""
    x, d = x.double(), d.double()
    a, b = torch.matmul(x.transpose(1, 2), x), torch.matmul(d.transpose(1, 2), x)
    return (torch.matmul(d, a) + torch.matmul(x, b + b.transpose(1, 2))) * s


def spatial(C, P):
    """the reference's rule (resnet_fd.py:133): the P x P form when n_in > H * W, the C x C form otherwise - the tie included"""
    return C > P


def fwd(x, s):
    return (fwd_spatial if spatial(x.shape[1], x.shape[2]) else fwd_channel)(x, s)


def bwd(x, d, s):
    return (bwd_spatial if spatial(x.shape[1], x.shape[2]) else bwd_channel)(x, d, s)


def fwd_bound(x):
    """|X| |X^T| |X| componentwise, float64: every partial sum of the forward is bounded by it"""
    a = x.double().abs()
    return torch.matmul(torch.matmul(a, a.transpose(1, 2)), a)


def bwd_bound(x, d):
    """the same for the backward: 2 |D| |X^T| |X| bounds (M + M^T) X, |X| |X^T| |D| bounds G D"""
    a, e = x.double().abs(), d.double().abs()
    m = torch.matmul(e, a.transpose(1, 2))
    return torch.matmul(m + m.transpose(1, 2), a) + torch.matmul(torch.matmul(a, a.transpose(1, 2)), e)


def integer_case(N, C, P, seed):
    """x in {-2 .. 2}, df in {-1, 0, 1} as float32 [N, C, P]"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (N, C, P), generator=g).float()
    d = torch.randint(-1, 2, (N, C, P), generator=g).float()
    return x, d


def scale_of(P):
    """fp32(1 / P) as a python float: what the kernels receive"""
    return float(np.float32(1.0 / P))
