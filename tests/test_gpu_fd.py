"""GPU: the feature-denoising product on ee_fd.hip (ops.fd_fwd / ops.fd_bwd) against the float64 restatement (tests/fd_reference.py) - bit for
bit on integer data, inside the summation-order bound on real data - and resnet18_fd through the model and the attack engine."""
import copy
import functools

import pytest
import torch

import fd_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

REAL = [(2, 64, 3136), (3, 128, 784), (2, 256, 196), (2, 512, 49)]  # the four ResNet-18/34 blocks at 224
# spatial with a ragged P; P = 1; P = 4; the tie C = P (channel form); d at the class limit with one element past the last full split
EDGE = [(3, 64, 35), (2, 512, 1), (2, 512, 4), (2, 64, 64), (1, 256, 257)]
UNSUPPORTED = (1, 320, 300)
U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def integer_reference(shape):
    """(x, df, float32(float64 forward * float64(scale)), the same for the backward, scale), computed once per shape on the host"""
    x, d = R.integer_case(*shape, seed=7 + shape[1] + shape[2])
    s = R.scale_of(shape[2])
    assert R.fwd_bound(x).max() < 2 ** 24 and R.bwd_bound(x, d).max() < 2 ** 24  # any summation order is exact in fp32
    return x, d, R.fwd(x, s).float(), R.bwd(x, d, s).float(), s


def _off_alignment(t):
    """the same values in a contiguous view whose base is one float past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize("shape,unaligned", [(s, False) for s in REAL + EDGE] + [((3, 128, 784), True), ((3, 64, 35), True), (UNSUPPORTED, False)])
def test_integer_data_is_exact_and_reproducible(shape, unaligned):
    from eeadv import ops
    x, d, f64, dx64, s = integer_reference(shape)
    xg, dg = x.to(DEV), d.to(DEV)
    if unaligned:
        xg, dg = _off_alignment(xg), _off_alignment(dg)
    assert ops.fd_supported(shape[1], shape[2]) == (shape != UNSUPPORTED) and ops._fd_on_kernel(xg) == (shape != UNSUPPORTED)
    runs = []
    for _ in range(2):
        f, gram = ops.fd_fwd(xg, s)
        if unaligned:
            gram = _off_alignment(gram)
        runs.append((f, gram, ops.fd_bwd(xg, dg, gram, s)))
    torch.cuda.synchronize()
    f, gram, dx = runs[0]
    wrong = (f.cpu() != f64).sum().item(), (dx.cpu() != dx64).sum().item()
    assert wrong == (0, 0), (wrong, (f.cpu() - f64).abs().max().item(), (dx.cpu() - dx64).abs().max().item())
    xd = x.double()
    want_gram = torch.matmul(xd.transpose(1, 2), xd) if R.spatial(shape[1], shape[2]) else torch.matmul(xd, xd.transpose(1, 2))
    assert torch.equal(gram.cpu().double(), want_gram)
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dist", ["rand", "randn"])
@pytest.mark.parametrize("shape", REAL)
def test_real_data_stays_inside_the_summation_order_bound(shape, dist):
    """|fp32 - float64| <= (C + P + 3) 2^-24 (|X| |X^T| |X|) scale componentwise, and the same factor on the backward's
    2 |D| |X^T| |X| + |X| |X^T| |D|: the first-order bound of two chained inner products of lengths C and P in ANY order, one rounding for the
    symmetrised sum, one for the scale, one for fp32(1 / P) itself.  (The backward runs its two products into one accumulator; read as one
    chain of length 2 min(C, P) its worst case is (2 min(C, P) + max(C, P) + 3) 2^-24 - the test holds the smaller factor.)"""
    from eeadv import ops
    N, C, P = shape
    g = torch.Generator().manual_seed(C + P + len(dist))
    draw = torch.rand if dist == "rand" else torch.randn
    x, d = draw(shape, generator=g), draw(shape, generator=g)
    s = R.scale_of(P)
    xg, dg = x.to(DEV), d.to(DEV)
    assert ops._fd_on_kernel(xg)
    f, gram = ops.fd_fwd(xg, s)
    dx = ops.fd_bwd(xg, dg, gram, s)
    # the matmul composite in the reference's association, fp32 on the same device
    xt = xg.transpose(1, 2)
    if C > P:
        a = torch.matmul(xt, xg)
        b = torch.matmul(dg.transpose(1, 2), xg)
        fc, dxc = torch.matmul(xg, a) * s, (torch.matmul(dg, a) + torch.matmul(xg, b + b.transpose(1, 2))) * s
    else:
        a = torch.matmul(xg, xt)
        m = torch.matmul(dg, xt)
        fc, dxc = torch.matmul(a, xg) * s, (torch.matmul(m + m.transpose(1, 2), xg) + torch.matmul(a, dg)) * s
    f64, dx64 = R.fwd(x, s), R.bwd(x, d, s)
    bf, bb = (C + P + 3) * U * R.fwd_bound(x) * s, (C + P + 3) * U * R.bwd_bound(x, d) * s
    ef, eb = (f.cpu().double() - f64).abs(), (dx.cpu().double() - dx64).abs()
    efc, ebc = (fc.cpu().double() - f64).abs(), (dxc.cpu().double() - dx64).abs()
    print("fd %s %s: forward max|err| %.3e (composite %.3e), max err/bound %.4f (composite %.4f); backward max|err| %.3e (composite %.3e), "
          "max err/bound %.4f (composite %.4f)" % (shape, dist, ef.max(), efc.max(), (ef / bf).max(), (efc / bf).max(), eb.max(), ebc.max(),
                                                   (eb / bb).max(), (ebc / bb).max()))
    assert (ef <= bf).all() and (eb <= bb).all()


def _calibrated_resnet18_fd(seed, x):
    """resnet18_fd for 64 x 64 crops whose BatchNorms carry the statistics of `x` (one train-mode pass with momentum 1 on the host): a freshly
    initialised model overflows in eval mode - four cubic blocks behind BatchNorms that normalise nothing"""
    from eeadv import models
    torch.manual_seed(seed)
    net = models.make_resnet_fd(18, size=64, num_classes=100)
    net.avgpool = torch.nn.AvgPool2d(2, stride=1)
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    for m in bns:
        m.momentum = 1.0
    net.train()
    with torch.no_grad():
        net(x)
    for m in bns:
        m.momentum = 0.1
    return net


def _logits_and_input_gradient(net, x, dl):
    xi = x.clone().requires_grad_(True)
    logits = net(xi)
    (g,) = torch.autograd.grad(logits, xi, dl)
    return logits.detach().double().cpu(), g.double().cpu()


def test_resnet18_fd_eval_is_as_close_to_float64_as_the_composite(monkeypatch):
    from eeadv import models, ops
    gen = torch.Generator().manual_seed(5)
    x, dl = torch.rand(2, 3, 64, 64, generator=gen), torch.randn(2, 100, generator=gen)
    net = _calibrated_resnet18_fd(31, x).eval()
    net64 = copy.deepcopy(net).double()
    net = net.to(DEV)
    calls = []
    fwd = ops.fd_fwd
    monkeypatch.setattr(ops, "fd_fwd", lambda t, s: (calls.append(tuple(t.shape)), fwd(t, s))[1])
    monkeypatch.setattr(models, "_STOCK", frozenset())
    hip = _logits_and_input_gradient(net, x.to(DEV), dl.to(DEV))
    assert calls == [(2, 64, 256), (2, 128, 64), (2, 256, 16), (2, 512, 4)] and all(ops.fd_supported(c, p) for _, c, p in calls)
    monkeypatch.setattr(models, "_STOCK", frozenset(("fd",)))
    stock = _logits_and_input_gradient(net, x.to(DEV), dl.to(DEV))
    assert len(calls) == 4
    ref = _logits_and_input_gradient(net64, x.double(), dl.double())
    assert torch.isfinite(ref[0]).all() and torch.isfinite(ref[1]).all() and ref[1].abs().max() > 0
    for what, h, c, r in zip(("logits", "input gradient"), hip, stock, ref):
        dh, dc = (h - r).norm().item(), (c - r).norm().item()
        print("resnet18_fd eval %s: |hip - f64| %.3e, |composite - f64| %.3e, |f64| %.3e" % (what, dh, dc, r.norm().item()))
        assert dh <= 2 * dc, (what, dh, dc)


def test_three_pgd_iterations_replay_bit_for_bit_and_only_conv3_is_vendor(monkeypatch):
    from eeadv import engine, models, ops
    monkeypatch.setattr(models, "_STOCK", frozenset())
    gen = torch.Generator().manual_seed(9)
    x0 = torch.rand(4, 3, 64, 64, generator=gen).to(DEV)
    y = torch.randint(0, 100, (4,), generator=gen).to(DEV)
    torch.manual_seed(41)
    net = models.make_resnet_fd(18, size=64, num_classes=100)
    net.avgpool = torch.nn.AvgPool2d(2, stride=1)
    nets = [copy.deepcopy(net).to(DEV).train() for _ in range(2)]
    calls = []
    fwd = ops.fd_fwd
    monkeypatch.setattr(ops, "fd_fwd", lambda t, s: (calls.append(tuple(t.shape)), fwd(t, s))[1])
    eps, step = 8 / 255, 2 / 255
    x_init = (x0 + (torch.rand(x0.shape, generator=gen).to(DEV) * 2 - 1) * eps).clamp(0, 1)
    outs = []
    try:
        for m, graph in zip(nets, (False, True)):
            outs.append(engine.pgd_loop(m, x0, x_init.clone(), engine.LossSpec(engine.CE_SUM, y), 3, step, eps, use_graph=graph))
        torch.cuda.synchronize()
    finally:
        engine.clear_graphs()
    assert calls[:4] == [(4, 64, 256), (4, 128, 64), (4, 256, 16), (4, 512, 4)] and len(calls) % 4 == 0
    assert torch.isfinite(outs[0]).all() and (outs[0] != x_init).any()
    assert torch.equal(outs[0], outs[1])
    # the same loop on the plain resnet18: the _fd model adds the four biased 1x1 convolutions to the vendor routes and nothing else
    torch.manual_seed(41)
    plain = models.make_resnet(18, "imagenet", num_classes=100)
    plain.avgpool = torch.nn.AvgPool2d(2, stride=1)
    plain = plain.to(DEV).train()
    engine.pgd_loop(plain, x0, x_init.clone(), engine.LossSpec(engine.CE_SUM, y), 1, step, eps, use_graph=False)
    base, mine = models.fallback_report(plain), models.fallback_report(nets[0])
    assert sorted(set(mine["layers"]) - set(base["layers"])) == ["denoise%d.conv3:miopen" % k for k in (1, 2, 3, 4)]
    assert set(base["layers"]) <= set(mine["layers"]) and mine["of"] == base["of"] + 4 and mine["layers"] == models.fallback_report(nets[1])["layers"]
