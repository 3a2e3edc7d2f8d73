"""tests/eval_route_reference.py against float64 nn.Conv2d / nn.BatchNorm2d(eval) / F.relu autograd on the CPU: the bar of
tests/test_gpu_eval_route.py is right before anything runs on a GPU.  The smallest shapes of that file, bn_reference.hard_affine (gamma of
both signs and zero), the hard running statistics (variance 1e-6 and 1e3, a mean 50 spreads from zero).  Two float64 evaluations of the
same expression in another association: rtol 1e-12 and atol 1e-12 of the largest entry."""
import pytest
import torch
import torch.nn.functional as F

import eval_route_reference as E
from bn_reference import hard_affine

EPS = 1e-5


def _close(a, b, what):
    top = float(b.abs().max())
    torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12 * max(top, 1.0), msg=lambda m: what + ": " + m)


def _modules(w, rm, rv, g, b, stride, padding):
    co, ci, k = w.shape[0], w.shape[1], w.shape[2]
    conv = torch.nn.Conv2d(ci, co, k, stride=stride, padding=padding, bias=False).double()
    bn = torch.nn.BatchNorm2d(co, eps=E.eps32(EPS)).double().eval()
    with torch.no_grad():
        conv.weight.copy_(w.double())
        bn.running_mean.copy_(rm.double()), bn.running_var.copy_(rv.double()), bn.weight.copy_(g.double()), bn.bias.copy_(b.double())
    return conv, bn


def _w(co, ci, k, gen):
    return torch.randn(co, ci, k, k, generator=gen) * (2.0 / (k * k * ci)) ** 0.5


@pytest.mark.parametrize("B,Cin,Cout,H", [(1, 32, 32, 4), (2, 32, 32, 8), (2, 64, 96, 8), (1, 128, 8, 2), (5, 128, 128, 2)])
@pytest.mark.parametrize("pieces,with_res,with_add", [(1, False, False), (2, True, True), (1, True, False), (2, False, True)])
def test_conv_bn_restatement_equals_the_stock_modules(B, Cin, Cout, H, pieces, with_res, with_add):
    gen = torch.Generator().manual_seed(B + Cin + Cout + H)
    x = torch.randn(B, Cin, H, H, generator=gen)
    w = _w(Cout, Cin, 3, gen)
    g, b = hard_affine(Cout)
    rm, rv, live = E.edge_statistics(Cout, gen, g)
    assert float(rv[live[0]]) == pytest.approx(1e-6) and float(rv[live[1]]) == 1e3 and float(rm[live[2]]) == 75.0
    res = torch.randn(B, Cout, H, H, generator=gen) if with_res else None
    dy = torch.randn(B, Cout, H, H, generator=gen)
    dy2 = torch.randn(B, Cout, H, H, generator=gen) if pieces == 2 else None
    dx_add = torch.randn(B, Cin, H, H, generator=gen) if with_add else None
    conv, bn = _modules(w, rm, rv, g, b, 1, 1)
    x64 = x.double().requires_grad_(True)
    r64 = None if res is None else res.double().requires_grad_(True)
    pre_m = bn(conv(x64)) if r64 is None else bn(conv(x64)) + r64
    y_m = F.relu(pre_m)
    pre = E.conv_bn_fwd64(x, w, (rm, rv, g, b, EPS), res)
    _close(pre, pre_m.detach(), "pre-activation")
    mask = pre_m.detach() > 0
    assert 0.2 < float(mask.double().mean()) < 0.8
    _close(E.gate(pre, mask), y_m.detach(), "relu from the mask")
    _close(E.gate(pre, y_m.detach()), y_m.detach(), "relu from the sign of the output")
    dtot = dy.double() if dy2 is None else dy.double() + dy2.double()
    grads = torch.autograd.grad(y_m, [x64] + ([r64] if r64 is not None else []), dtot)
    dx, dz = E.conv_bn_bwd64(dy, dy2, mask, w, (rv, g, EPS), x.shape, dx_add)
    _close(dx, grads[0] if dx_add is None else grads[0] + dx_add.double(), "dx")
    if r64 is not None:
        _close(dz, grads[1], "dres")
    assert torch.equal(dz, dtot * mask.double())
    # without gamma / beta, without the ReLU
    conv1, bn1 = _modules(w, rm, rv, torch.ones(Cout), torch.zeros(Cout), 1, 1)
    x64b = x.double().requires_grad_(True)
    plain = bn1(conv1(x64b))
    _close(E.conv_bn_fwd64(x, w, (rm, rv, None, None, EPS), None), plain.detach(), "no affine parameters, no ReLU")
    (gx,) = torch.autograd.grad(plain, x64b, dy.double())
    _close(E.conv_bn_bwd64(dy, None, None, w, (rv, None, EPS), x.shape)[0], gx, "dx, no affine parameters, no ReLU")


@pytest.mark.parametrize("B,Cin,Cout,H", [(1, 32, 32, 4), (2, 32, 64, 8)])
def test_pair_restatement_equals_the_stock_modules(B, Cin, Cout, H):
    gen = torch.Generator().manual_seed(B + Cin + H)
    x = torch.randn(B, Cin, H, H, generator=gen)
    w3, w1 = _w(Cout, Cin, 3, gen), _w(Cout, Cin, 1, gen)
    (g3, b3), (g1, b1) = hard_affine(Cout), hard_affine(Cout, 3)
    rm3, rv3, _ = E.edge_statistics(Cout, gen, g3)
    rm1, rv1, _ = E.edge_statistics(Cout, gen, g1)
    c3, n3 = _modules(w3, rm3, rv3, g3, b3, 2, 1)
    c1, n1 = _modules(w1, rm1, rv1, g1, b1, 2, 0)
    x64 = x.double().requires_grad_(True)
    p3_m, p1_m = n3(c3(x64)), n1(c1(x64))
    y3_m = F.relu(p3_m)
    p3, p1 = E.pair_fwd64(x, w3, w1, (rm3, rv3, g3, b3, EPS), (rm1, rv1, g1, b1, EPS))
    assert p3.shape == (B, Cout, H // 2, H // 2) == p1.shape
    _close(p3, p3_m.detach(), "bn1(conv3x3s2)"), _close(p1, p1_m.detach(), "bn_ds(conv1x1s2)")
    _close(E.gate(p3, y3_m.detach()), y3_m.detach(), "relu(bn1(conv3x3s2))")
    dy3, dy1 = torch.randn(p3.shape, generator=gen), torch.randn(p3.shape, generator=gen)
    (gx,) = torch.autograd.grad([y3_m, p1_m], x64, [dy3.double(), dy1.double()])
    _close(E.pair_bwd64(dy3, y3_m.detach(), dy1, w3, w1, (rv3, g3, EPS), (rv1, g1, EPS), x.shape), gx, "pair dx")


def test_a_nan_under_a_closed_gate_stays_and_a_nan_mask_is_closed():
    pre = torch.tensor([1.0, float("nan"), -2.0, 3.0], dtype=torch.float64)
    out = E.gate(pre, torch.tensor([1.0, float("nan"), 0.0, 0.0]))
    assert float(out[0]) == 1.0 and bool(torch.isnan(out[1])) and float(out[2]) == 0.0 and float(out[3]) == 0.0
    assert not bool(E.as_mask(torch.tensor([float("nan")]))[0])
