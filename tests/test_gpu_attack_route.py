"""The route the headline number is measured on - engine.input_gradient in TRAIN mode inside functional.attack_forward() - pinned to float64.

Only on this route do TrainConvBnConvFn / TrainPairBnConvFn (bn1's batch statistics, and on 16x16 maps its backward, across the kernel
boundary), the one-pass stem with x_argmax and ResNet.head_grad run.  Section 1 compares the whole body with the float64 stock modules on the
ReLU branch the fp32 run took (tests/branch_replay.py); section 2 compares each of the route's kernels with a float64 restatement written in
torch here, never with another ee_* kernel on the reference side.

Bars.  Binding ones are relative to something that is not the code under test: "no further from float64 than twice X is on the same
inputs", X being the all-stock fp32 path (section 1) or the sibling kernel the older tests compare with (section 2), plus a floor of 1e-6
of the gradient's norm / 1e-7 of the reference's largest entry.  Absolute bars next to them are stated in each docstring with what was
measured on MI355X."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

from branch_replay import ALL_STOCK, pool_code_to_index, replayed_attack_gradient, train_pre_mask

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24  # unit roundoff of fp32


@pytest.fixture(scope="module")
def ops():
    from eeadv import ops as _ops
    return _ops


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the whole body on the attack route
# ---------------------------------------------------------------------------------------------------------------------------------------
# absolute bars of section 1: at most 4x the largest value measured on MI355X over the parametrisation and never above 1e-4 of ||g64|| (one
# flipped mask costs 1.5e-3 ... 3.9e-3: the bar separates rounding from a single wrong gate by more than 10x)
ABS_BAR = {16: 8e-6, 100: 6.5e-6}
_STOCK_DISTANCE = {}  # (B, seed, kind) -> the all-stock fp32 path's distance from float64 (does not depend on _TRAINFUSE_MAPS)


def _bn_layers(net):
    return [(n, m) for n, m in net.named_modules() if isinstance(m, torch.nn.BatchNorm2d)]


def _attack_route_case(monkeypatch, B, maps, seed, kind, abs_bar, affine_seed=None):
    from eeadv import engine, functional, models
    monkeypatch.setattr(models, "_TRAINFUSE_MAPS", frozenset(maps))
    assert models._HEAD_CE and functional._POOL_XA and functional._TRAIN_BWD_BOUNDARY
    r = replayed_attack_gradient(monkeypatch, B, seed, kind, affine_seed=affine_seed)
    net, net64, calls = r["net32"], r["net64"], r["calls"]
    # the route under test is the route taken
    fused = [n for n, m in net.named_modules() if isinstance(m, torch.nn.Conv2d) and "(train)" in m.__dict__.get("_ee_route", "")]
    want = 2 if set(maps) == {16} else 6
    assert len(fused) == want, fused
    assert calls == {"train_pre": want, "pool_fwd": 1, "pool_fwd_xa": 1, "ce_head": 1}, calls
    assert r["n_relu"] == 17
    # logits of the same forward, from a second deep copy (the model under test sees one forward)
    with torch.enable_grad(), functional.attack_forward():
        twin2 = copy.deepcopy(r["twin"])
        logits = twin2.head_from_pre(twin2.body_pre(r["x"].clone().requires_grad_(True))).detach()
    e_logit = float((logits.double() - r["logits64"]).abs().max())
    print("attack route B=%d maps=%s seed=%d %s: logits max |d| %.3e" % (B, sorted(maps), seed, kind, e_logit))
    assert e_logit <= 1e-4
    # every BatchNorm's running statistics after the one forward
    bns, bns64 = _bn_layers(net), _bn_layers(net64)
    assert len(bns) == len(bns64) == 20
    worst = [0.0, 0.0]
    for (name, b32), (_, b64) in zip(bns, bns64):
        assert int(b32.num_batches_tracked) == int(b64.num_batches_tracked) == 1, name
        worst[0] = max(worst[0], float(((b32.running_mean.double() - b64.running_mean).abs() / (1e-5 * b64.running_mean.abs() + 1e-6)).max()))
        worst[1] = max(worst[1], float(((b32.running_var.double() - b64.running_var).abs() / (1e-4 * b64.running_var.abs() + 1e-6)).max()))
    print("    running statistics, worst |d| / (rtol |ref| + atol): mean %.3f  var %.3f" % tuple(worst))
    for (name, b32), (_, b64) in zip(bns, bns64):
        torch.testing.assert_close(b32.running_mean.double(), b64.running_mean, rtol=1e-5, atol=1e-6, msg=lambda m: name + ".running_mean: " + m)
        torch.testing.assert_close(b32.running_var.double(), b64.running_var, rtol=1e-4, atol=1e-6, msg=lambda m: name + ".running_var: " + m)
    # the input gradient
    rel = float((r["g32"].double() - r["g64"]).norm() / r["g64"].norm())
    key = (B, seed, kind, affine_seed)
    if key not in _STOCK_DISTANCE:
        s = replayed_attack_gradient(monkeypatch, B, seed, kind, fp32_stock=ALL_STOCK, affine_seed=affine_seed)
        assert s["calls"]["train_pre"] == 0 and s["calls"]["pool_fwd"] == 0 and s["calls"]["ce_head"] == 0
        _STOCK_DISTANCE[key] = float((s["g32"].double() - s["g64"]).norm() / s["g64"].norm())
        del s
    rel_stock = _STOCK_DISTANCE[key]
    print("    input gradient |g32 - g64| / |g64|: this route %.3e, all-stock fp32 %.3e" % (rel, rel_stock))
    assert rel <= 2 * rel_stock + 1e-6, (rel, rel_stock)
    assert rel <= abs_bar, rel
    # the same bits from a fresh deep copy of the model
    monkeypatch.setattr(models, "_STOCK", frozenset())  # (the yardstick run above left the all-stock setting)
    g_again = engine.input_gradient(r["twin"], r["x"].clone(), engine.LossSpec(kind, r["y"])).detach()
    assert torch.equal(g_again, r["g32"])
    for (name, a), (_, b) in zip(_bn_layers(r["twin"]), bns):
        assert torch.equal(a.running_mean, b.running_mean) and torch.equal(a.running_var, b.running_var), name
    return rel, rel_stock


@pytest.mark.parametrize("maps", [(16,), (16, 8, 4)], ids=["maps16", "maps16-8-4"])
@pytest.mark.parametrize("B", [16, 100])
def test_attack_route_input_gradient_equals_float64_on_the_same_branch(monkeypatch, B, maps):
    """make_resnet(18, 'tiny').train(), engine.input_gradient(model, x, LossSpec(CE_SUM, y)) with nothing stocked, against the float64 stock
    modules with all 17 ReLU masks and the stem argmax replayed (branch_replay.replayed_attack_gradient), three inputs each.  maps16 is what the
    headline runs (2 convolutions on the boundary path), maps16-8-4 reaches TrainPairBnConvFn and the boundary forward on 8x8 / 4x4 maps (6).
    Asserted: the route taken (routes, recorder counts, 17 masks, none left over); logits within 1e-4; all 20 BatchNorms' running statistics
    (rtol 1e-5 mean / 1e-4 var, atol 1e-6); ||g32 - g64|| / ||g64|| at most twice the all-stock fp32 path's under the same procedure + 1e-6, and
    at most ABS_BAR; the same bits from a fresh deep copy.
    Measured (MI355X; ||g32 - g64|| / ||g64|| of this route / of the all-stock fp32 path, over the three inputs):
        batch 16,  maps16:      2.03e-6 ... 2.06e-6 / 1.68e-6 ... 1.75e-6        batch 16,  maps16-8-4: 2.02e-6 ... 2.04e-6 / the same
        batch 100, maps16:      1.70e-6 ... 1.71e-6 / 1.59e-6 ... 1.62e-6        batch 100, maps16-8-4: 1.70e-6 ... 1.71e-6 / the same
        (asserted next to the factor-2 rule: ABS_BAR = 8e-6 at batch 16, 6.5e-6 at batch 100 - the parameter-gradient route measured 2.4e-6)
        logits: max |d| 4.6e-6 ... 6.1e-6; running statistics: at most 0.12 of the tolerance (mean, batch 16) / 0.05 (mean, batch 100) / 0.003 (var)."""
    for seed in (0, 1, 2):
        _attack_route_case(monkeypatch, B, maps, seed, "ce_sum", ABS_BAR[B])


def test_attack_route_mean_reduction_equals_float64_on_the_same_branch(monkeypatch):
    """The same at batch 16 with LossSpec(CE_MEAN, y) (ops.ce_pool_linear_bwd's other reduction), every block on the boundary path.
    Measured (MI355X): 2.02e-6 of ||g64||, the all-stock fp32 path 1.75e-6; logits 5.2e-6."""
    _attack_route_case(monkeypatch, 16, (16, 8, 4), 0, "ce_mean", ABS_BAR[16])


def test_attack_route_with_random_batchnorm_weights_and_biases(monkeypatch):
    """The same at batch 16, every block on the boundary path, with every BatchNorm's weight from U(0.5, 1.5) and bias from N(0, 0.2^2): a freshly
    initialised model (weight 1, bias 0) cannot tell `invstd * gamma` from `gamma` inside a ReLU mask, nor see a missing beta.
    Measured (MI355X): 1.93e-6 of ||g64||, the all-stock fp32 path 1.68e-6; logits 5.3e-6; running statistics at most 0.08 of the tolerance."""
    _attack_route_case(monkeypatch, 16, (16, 8, 4), 0, "ce_sum", ABS_BAR[16], affine_seed=5)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. the route's kernels, each against float64
# ---------------------------------------------------------------------------------------------------------------------------------------
def _err(a, ref):
    return float((a.detach().double() - ref).abs().max())


def _twice_the_sibling(got, sibling, ref, what):
    """`got` is no further from the float64 `ref` than twice the sibling kernel is, plus 1e-7 of ref's largest entry"""
    e_g, e_s, top = _err(got, ref), _err(sibling, ref), float(ref.abs().max())
    print("    %-28s kernel %.3e  sibling %.3e  of max |ref| %.3e" % (what, e_g, e_s, top))
    assert e_g <= 2 * e_s + 1e-7 * top, "%s: %.3e from float64, the sibling kernel %.3e (max |ref| %.3e)" % (what, e_g, e_s, top)
    return e_g / top, e_s / top


def _conv_w(co, ci, k, gen):
    return (torch.randn(co, ci, k, k, generator=gen) * (2.0 / (k * k * ci)) ** 0.5).to(DEV)


def _relu_keep_nan(z):
    return torch.where(z > 0, z, torch.where(torch.isnan(z), z, torch.zeros_like(z)))


def _a1_exact(c1, sm, si, gamma, beta):
    """what ee_fuse.hpp's train_bn_apply stages, as fp32 torch operations of the same association, each rounded on its own"""
    sh = (1, -1, 1, 1)
    return _relu_keep_nan((c1 - sm.view(sh)) * (si * gamma).view(sh) + beta.view(sh))


def _merge64(stats, cnt, eps, momentum, rm0, rv0):
    """float64 restatement of ee_fuse.hpp's train_bn_merge on the producer's partials [C, S, 2] = (mean, M2) of cnt values each"""
    st = stats.double()
    S = st.shape[1]
    n = S * cnt
    mean = st[:, :, 0].mean(1)
    m2 = (st[:, :, 1] + cnt * (st[:, :, 0] - mean[:, None]) ** 2).sum(1)
    var = m2 / n
    return mean, 1.0 / torch.sqrt(var + eps), (1 - momentum) * rm0 + momentum * mean, (1 - momentum) * rv0 + momentum * var * (n / (n - 1.0))


def _boundary_forward_checks(ops, c1, stats, cnt, gamma, beta, u2, what):
    """the consumer half (ee_wino3x3_bn_train_pre_f32) on a producer's raw output c1 and its partial moments"""
    C = c1.shape[1]
    eps, mom = 1e-5, 0.1
    rm, rv = torch.full((C,), 0.1, device=DEV), torch.full((C,), 0.9, device=DEV)
    rm_s, rv_s = rm.clone(), rv.clone()
    got, sm, si = ops.wino3x3_bn_train_pre(c1, stats, cnt, gamma, beta, eps, mom, rm, rv, u2)
    _, sm_s, si_s = ops.bn_act_fwd(c1, None, gamma, beta, rm_s, rv_s, mom, eps, True, True)  # the sibling: ee_bn_act_fwd_f32
    # (a) float64 statistics of c1 itself
    x64 = c1.double()
    n = x64.numel() // C
    mean64, var64 = x64.mean((0, 2, 3)), x64.var((0, 2, 3), unbiased=False)
    print("  %s" % what)
    _twice_the_sibling(sm, sm_s, mean64, "save_mean")
    _twice_the_sibling(si, si_s, 1.0 / torch.sqrt(var64 + eps), "save_invstd")
    _twice_the_sibling(rm, rm_s, 0.9 * 0.1 + 0.1 * mean64, "running_mean")
    _twice_the_sibling(rv, rv_s, 0.9 * 0.9 + 0.1 * var64 * (n / (n - 1.0)), "running_var")
    # (b) the merge alone: float64 on the kernel's own partials.  16 lanes add ceil(S / 16) partials each in index order, four butterfly
    # levels follow: the sum carries at most (ceil(S / 16) + 4) roundings; the terms of M2 (a difference, its square, the product with cnt,
    # the sum with M2_s), the division by n, sqrt, the reciprocal and the momentum update (1 - momentum rounded to fp32) at most 12 more.
    assert stats.shape[1] * cnt == n
    mean_m, invstd_m, rm_m, rv_m = _merge64(stats, cnt, eps, mom, 0.1, 0.9)
    bound = (math.ceil(stats.shape[1] / 16) + 16) * U
    for name, a, b in (("save_mean", sm, mean_m), ("save_invstd", si, invstd_m), ("running_mean", rm, rm_m), ("running_var", rv, rv_m)):
        scale = float(stats[:, :, 0].abs().max()) if name == "save_mean" else float(b.abs().max())
        e = _err(a, b)
        print("    merge alone %-16s %.3e of %.3e (allowed %.3e relative)" % (name, e, scale, bound))
        assert e <= bound * scale, "merge of the partials, %s: %.3e of %.3e (allowed %.3e relative)" % (name, e, scale, bound)
    # (c) the output: the Winograd kernel on the staged activation, bit for bit
    want = ops.wino3x3(_a1_exact(c1, sm, si, gamma, beta), u2)
    d = float((got - want).abs().max())
    print("    conv2(relu(bn1 c1)) vs wino3x3(a1 from the fp32 expression): max |d| %.3e, equal %s" % (d, torch.equal(got, want)))
    assert torch.equal(got, want)


@pytest.mark.parametrize("B,C,H", [(100, 64, 16), (5, 64, 16), (7, 128, 8), (2, 128, 8), (9, 256, 4), (4, 256, 4), (3, 32, 16)])
def test_boundary_forward_statistics_against_float64(ops, B, C, H):
    """ee_wino3x3_stats_f32 + ee_wino3x3_bn_train_pre_f32: save_mean / save_invstd / running statistics (momentum 0.1, unbiased n / (n - 1))
    against float64 statistics of c1 itself - no further than twice ee_bn_act_fwd_f32 is, + 1e-7 of the largest entry; against a float64
    restatement of the merge on the kernel's own partials - (ceil(S / 16) + 16) * 2^-24 relative, the roundings counted in
    _boundary_forward_checks; the output torch.equal to ops.wino3x3 on the activation staged by the fp32 torch expression.
    Measured (MI355X; max |d| from float64, kernel / ee_bn_act_fwd_f32, over the seven shapes): save_mean 5.6e-8 ... 1.6e-7 / 7.4e-8 ... 1.2e-7;
    save_invstd 1.2e-7 ... 2.6e-7 / 1.2e-7 ... 2.0e-7; running_mean 9.9e-9 ... 2.3e-8 / 1.1e-8 ... 2.6e-8; running_var 8.3e-8 ... 9.5e-8 / 8.5e-8 ... 9.5e-8
    (largest entries 1.1 ... 1.5, 1.3 ... 1.8, 0.2, 0.9).  The merge alone: at most 1.4e-7 (save_mean), 2.5e-7 (save_invstd), 2.1e-8, 9.4e-8 against
    bounds of 1.0e-6 ... 1.4e-6 relative.  The output: torch.equal on every shape."""
    from eeadv import functional as Fn
    gen = torch.Generator().manual_seed(B + C + H)
    x = torch.relu(torch.randn(B, C, H, H, generator=gen)).to(DEV)
    w1, w2 = _conv_w(C, C, 3, gen), _conv_w(C, C, 3, gen)
    gamma, beta = (torch.rand(C, generator=gen) + 0.5).to(DEV), (torch.randn(C, generator=gen) * 0.2).to(DEV)
    c1, stats = ops.wino3x3_stats(x, Fn.wino_sets(w1)[0])
    _boundary_forward_checks(ops, c1, stats, H * H, gamma, beta, Fn.wino_sets(w2)[0], "wino producer B=%d C=%d H=%d" % (B, C, H))


@pytest.mark.parametrize("B,Cin,Cout,H", [(100, 64, 128, 16), (5, 64, 128, 16), (7, 128, 256, 8), (2, 128, 256, 8)])
def test_boundary_forward_statistics_from_the_stride2_producer_against_float64(ops, B, Cin, Cout, H):
    """The same with ee_conv3x3s2_pair_stats_fwd_f32 as the producer (TrainPairBnConvFn: the first block of layers 2 and 3).
    Measured (MI355X, kernel / sibling): save_mean 8.3e-8 ... 1.5e-7 / 8.7e-8 ... 1.4e-7; save_invstd 1.4e-7 ... 2.0e-7 / 1.5e-7 ... 2.0e-7; running_mean
    1.4e-8 ... 2.6e-8 / 1.5e-8 ... 1.9e-8; running_var 8.9e-8 ... 9.6e-8 / 8.7e-8 ... 9.8e-8; the merge alone at most 2.1e-7 against 1.0e-6 ... 1.7e-6; output torch.equal."""
    from eeadv import functional as Fn
    gen = torch.Generator().manual_seed(B + Cin + H)
    x = torch.relu(torch.randn(B, Cin, H, H, generator=gen)).to(DEV)
    w3, wd, w2 = _conv_w(Cout, Cin, 3, gen), _conv_w(Cout, Cin, 1, gen), _conv_w(Cout, Cout, 3, gen)
    gamma, beta = (torch.rand(Cout, generator=gen) + 0.5).to(DEV), (torch.randn(Cout, generator=gen) * 0.2).to(DEV)
    y3, _, stats, cnt = ops.conv3x3s2_pair_stats_fwd(x, Fn._dense_weight(w3, "s2p_f", wd), Cout)
    _boundary_forward_checks(ops, y3, stats, cnt, gamma, beta, Fn.wino_sets(w2)[0], "stride-2 producer B=%d %d->%d H=%d" % (B, Cin, Cout, H))


def _bn_relu_bwd64(d, c1, mask, sm, si, gamma):
    """gamma * invstd * ((dz - mean(dz)) - xhat * mean(dz * xhat)) in float64: dz = d where `mask`, the batch means over c1 as given"""
    sh = (1, -1, 1, 1)
    dz = torch.where(mask, d.double(), torch.zeros_like(d, dtype=torch.float64))
    xhat = (c1.double() - sm.double().view(sh)) * si.double().view(sh)
    m1, m2 = dz.mean((0, 2, 3), keepdim=True), (dz * xhat).mean((0, 2, 3), keepdim=True)
    return (gamma.double() * si.double()).view(sh) * ((dz - m1) - xhat * m2), dz, xhat


GATE_BAR_DX, GATE_BAR_SUMS = 4e-7, 4.5e-7  # of the largest entry; measured 1.07e-7 and 1.24e-7 (test_relu_gates_agree_at_zero)


def _identity_filter(C):
    w = torch.zeros(C, C, 3, 3, device=DEV)
    w[torch.arange(C), torch.arange(C), 1, 1] = 1.0
    return w


@pytest.mark.parametrize("with_beta", [False, True], ids=["beta0", "beta"])
def test_relu_gates_agree_at_zero(ops, with_beta):
    """The forward prologue, ee_bn_act_bwd2_f32 (mask from x), ee_wino3x3_bwd_sums_f32 and ee_wino3x3_bn_train_bwd_pre_f32 open the same gates.
    `stats` / save_mean / save_invstd come from a random c1 (8 x 64 x 16 x 16) and stay; then 300 entries per channel are overwritten with
    values whose pre-activation (the fp32 expression) is exactly 0 and one / two floats either side of it: beta = 0 - save_mean and
    torch.nextafter around it; beta != 0 - the floats within 64 ulp of save_mean - beta / (invstd * gamma), of which those giving exactly 0, the
    two smallest giving > 0 and the two largest giving < 0 are kept.  Asserted first: >= 100 planted entries per channel on each side of
    zero; an exact zero in every channel for beta = 0, in at least one channel for beta != 0 (whether the product (x - mean) * scale can
    round to -beta exactly depends on the channel's binades; the count is printed).
    Forward: torch.equal to ops.wino3x3 on the staged activation.  Backward: dx of each form against the float64 formula with dz masked by the
    fp32 expression and the batch means over the planted tensor, asserted PER PLANTED ELEMENT: a gate opened differently is an error of
    |dy| * gamma * invstd there.  Bars: ee_bn_act_bwd2_f32 (itself the sibling of the rest of this file) GATE_BAR_DX = 4e-7 of max |dx| and the
    per-image sums of dz and dz * xhat GATE_BAR_SUMS = 4.5e-7 of their largest entry - both under 4x the largest value measured.  The boundary
    consumer is read through conv1^T with an identity filter and held to section 2's rule: no further from the float64 dx than twice the
    unfused sequence ee_bn_act_bwd2_f32 | ee_wino3x3_f32 (the same identity filter) is, + 1e-7 of max |dx| - in the maximum norm and, with
    that same bound, at every planted entry.  More than 99 % of the planted entries carry a |dy| * gamma * invstd above a hundred times
    GATE_BAR_DX, so a wrong gate cannot hide.
    Measured (MI355X): beta = 0 - 140 / 140 planted entries per channel above / below zero, an exact zero in 64 of 64 channels; beta != 0 - 140 / 140 ... 160,
    an exact zero in 27 of 64 channels.  Forward torch.equal.  ee_bn_act_bwd2_f32: 5.6e-7 / 7.4e-7 on the planted entries (9.7e-7 anywhere) of max |dx| 9.1 / 9.8, i.e.
    6.2e-8 / 7.6e-8 relative (1.07e-7 anywhere); the boundary consumer through the identity convolution: 9.0e-7 / 8.7e-7 (1.1e-6 anywhere), 1.3e-7 relative;
    per-image sums: 4.4e-6 / 3.9e-6 of 54 / 50 (dz), 4.6e-6 / 5.2e-6 of 46 / 42 (dz * xhat), i.e. 1.24e-7 relative at most.
    Against the sibling rule: the consumer 1.147e-6 / 1.036e-6 anywhere, the unfused sequence through the same identity filter exactly the same figures
    (allowed: twice that + 9e-7)."""
    from eeadv import functional as Fn
    B, C, H, eps = 8, 64, 16, 1e-5
    gen = torch.Generator().manual_seed(77 + int(with_beta))
    x = torch.relu(torch.randn(B, C, H, H, generator=gen)).to(DEV)
    w1, w2 = _conv_w(C, C, 3, gen), _conv_w(C, C, 3, gen)
    gamma = (torch.rand(C, generator=gen) + 0.5).to(DEV)
    beta = (torch.randn(C, generator=gen) * 0.2).to(DEV) if with_beta else torch.zeros(C, device=DEV)
    dc2 = torch.randn(B, C, H, H, generator=gen).to(DEV)
    c1, stats = ops.wino3x3_stats(x, Fn.wino_sets(w1)[0])
    u2, u2b = Fn.wino_sets(w2)
    _, sm, si = ops.wino3x3_bn_train_pre(c1, stats, H * H, gamma, beta, eps, 0.1, None, None, u2)
    # candidates per channel: 129 consecutive floats around the root of the pre-activation
    root = sm - beta / (si * gamma) if with_beta else sm.clone()
    cand = [root]
    for _ in range(64):
        cand.append(torch.nextafter(cand[-1], torch.full_like(root, float("inf"))))
    lo = root
    for _ in range(64):
        lo = torch.nextafter(lo, torch.full_like(root, float("-inf")))
        cand.insert(0, lo)
    cand = torch.stack(cand, 1)  # [C, 129] ascending
    pre = (cand - sm[:, None]) * (si * gamma)[:, None] + beta[:, None]
    assert bool((pre[:, 1:] >= pre[:, :-1]).all()) and bool((pre[:, 0] < 0).all()) and bool((pre[:, -1] > 0).all())
    n_neg, n_zero = (pre < 0).sum(1), (pre == 0).sum(1)  # ascending: negatives, zeros, positives
    pos = torch.arange(C, device=DEV)
    picks = {"-2": cand[pos, n_neg - 2], "-1": cand[pos, n_neg - 1], "+1": cand[pos, n_neg + n_zero], "+2": cand[pos, n_neg + n_zero + 1]}
    zero_val = cand[pos, torch.clamp(n_neg, max=128)]  # a float whose pre-activation is exactly 0 where the channel has one
    has_zero = n_zero > 0
    c1p = c1.clone().permute(1, 0, 2, 3).reshape(C, -1)
    where = torch.stack([torch.randperm(B * H * H, generator=gen)[:300] for _ in range(C)]).to(DEV)  # [C, 300] distinct positions
    vals = torch.cat([picks["-2"][:, None].expand(C, 70), picks["-1"][:, None].expand(C, 70), picks["+1"][:, None].expand(C, 70),
                      picks["+2"][:, None].expand(C, 70), torch.where(has_zero, zero_val, picks["-1"])[:, None].expand(C, 20)], 1)
    c1p.scatter_(1, where, vals)
    planted = torch.zeros_like(c1p, dtype=torch.bool).scatter_(1, where, True)
    c1p = c1p.view(C, B, H, H).permute(1, 0, 2, 3).contiguous()
    planted = planted.view(C, B, H, H).permute(1, 0, 2, 3).contiguous()
    sh = (1, C, 1, 1)
    pre_p = (c1p - sm.view(sh)) * (si * gamma).view(sh) + beta.view(sh)
    mask = pre_p > 0
    assert torch.equal(mask, train_pre_mask(c1p, sm, si, gamma, beta))
    above, below = (planted & (pre_p > 0)).sum((0, 2, 3)), (planted & (pre_p < 0)).sum((0, 2, 3))
    exact = (planted & (pre_p == 0)).sum((0, 2, 3))
    print("planted per channel: above zero %d..%d, below %d..%d, exactly zero in %d of %d channels (%d entries)"
          % (int(above.min()), int(above.max()), int(below.min()), int(below.max()), int((exact > 0).sum()), C, int(exact.sum())))
    assert int(above.min()) >= 100 and int(below.min()) >= 100
    assert int((exact > 0).sum()) >= (1 if with_beta else C)
    # forward
    got = ops.wino3x3_bn_train_pre(c1p, stats, H * H, gamma, beta, eps, 0.1, None, None, u2)
    assert torch.equal(got[1], sm) and torch.equal(got[2], si)  # the statistics did not move
    assert torch.equal(got[0], ops.wino3x3(_a1_exact(c1p, sm, si, gamma, beta), u2))
    # backward
    d_a1, sums = ops.wino3x3_bwd_sums(dc2, u2b, c1p, sm, si, gamma, beta)
    assert torch.equal(d_a1, ops.wino3x3(dc2, u2b))
    dx64, dz64, xhat64 = _bn_relu_bwd64(d_a1, c1p, mask, sm, si, gamma)
    top = float(dx64.abs().max())
    gate_size = (d_a1.abs() * (gamma * si).view(sh))[planted]
    assert float((gate_size > 100 * GATE_BAR_DX * top).float().mean()) > 0.99
    for name, s, ref in (("sum dz", sums[:, :, 0], dz64.sum((2, 3)).t()), ("sum dz * xhat", sums[:, :, 1], (dz64 * xhat64).sum((2, 3)).t())):
        e, scale = _err(s, ref), float(ref.abs().max())
        print("    per-image %-14s %.3e of %.3e" % (name, e, scale))
        assert e <= GATE_BAR_SUMS * scale, name
    dx_bn = ops.bn_act_bwd(d_a1, None, c1p, gamma, sm, si, None, None, eps, True, True, True, False, False, None, beta)[0]
    d_bn = (dx_bn.double() - dx64).abs()
    print("    ee_bn_act_bwd2_f32: max |d| %.3e on the planted entries, %.3e anywhere, of max |dx| %.3e" % (float(d_bn[planted].max()), float(d_bn.max()), top))
    assert bool((d_bn[planted] <= GATE_BAR_DX * top).all()) and float(d_bn.max()) <= GATE_BAR_DX * top
    u_id = Fn.wino_sets(_identity_filter(C))[1]
    dx_pre = ops.wino3x3_bn_train_bwd_pre(d_a1, c1p, sums, H * H, sm, si, gamma, beta, u_id)
    sibling = ops.wino3x3(dx_bn, u_id)
    _twice_the_sibling(dx_pre, sibling, dx64, "consumer, identity conv1^T")
    d_pre = (dx_pre.double() - dx64).abs()
    print("    ee_wino3x3_bn_train_bwd_pre_f32: max |d| %.3e on the planted entries" % float(d_pre[planted].max()))
    assert bool((d_pre[planted] <= 2 * _err(sibling, dx64) + 1e-7 * top).all())


def test_nan_preactivation_forward_and_backward(ops):
    """One NaN in c1 (statistics from before it was planted).  Forward: relu_keep_nan hands it to conv2, as torch.relu does on the unfused
    path: the output equals ops.wino3x3 on the staged activation, NaN pattern included.  Backward: the kernels CLOSE the gate of a NaN
    pre-activation (`NaN > 0` is false: the image's sum of dz leaves that entry out), ATen's threshold_backward on the unfused path OPENS it
    (`x <= 0 ? 0 : grad`); nothing downstream can tell, because xhat is NaN there: the sum of dz * xhat, with it mean(dz * xhat) and so every
    dx of that channel are NaN either way.  Asserted: both of those statements, and that dx of ee_bn_act_bwd2_f32 and of the boundary consumer
    (before its convolution multiplies the channel into all others) is NaN on exactly that channel - the pattern of ATen's threshold_backward + native_batch_norm_backward given the same saved statistics - and
    within GATE_BAR_DX of max |dx| of the float64 formula (as in test_relu_gates_agree_at_zero) on every other channel (measured 7.7e-8)."""
    from eeadv import functional as Fn
    B, C, H, eps = 5, 64, 16, 1e-5
    gen = torch.Generator().manual_seed(91)
    x = torch.relu(torch.randn(B, C, H, H, generator=gen)).to(DEV)
    w1, w2 = _conv_w(C, C, 3, gen), _conv_w(C, C, 3, gen)
    gamma, beta = (torch.rand(C, generator=gen) + 0.5).to(DEV), (torch.randn(C, generator=gen) * 0.2).to(DEV)
    dc2 = torch.randn(B, C, H, H, generator=gen).to(DEV)
    c1, stats = ops.wino3x3_stats(x, Fn.wino_sets(w1)[0])
    u2, u2b = Fn.wino_sets(w2)
    _, sm, si = ops.wino3x3_bn_train_pre(c1, stats, H * H, gamma, beta, eps, 0.1, None, None, u2)
    d_a1 = ops.wino3x3(dc2, u2b)
    h, w = divmod(int(d_a1[2, 7].abs().argmax()), H)  # where the plane's largest gradient arrives: an open gate there cannot be missed
    c1[2, 7, h, w] = float("nan")
    a1 = _a1_exact(c1, sm, si, gamma, beta)
    assert int(torch.isnan(a1).sum()) == 1 and bool(torch.isnan(torch.relu(c1[2, 7, h, w])))
    got = ops.wino3x3_bn_train_pre(c1, stats, H * H, gamma, beta, eps, 0.1, None, None, u2)[0]
    want = ops.wino3x3(a1, u2)
    assert int(torch.isnan(got).sum()) > 0 and torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(want))
    # backward
    d_a1b, sums = ops.wino3x3_bwd_sums(dc2, u2b, c1, sm, si, gamma, beta)
    assert torch.equal(d_a1b, d_a1)
    mask = train_pre_mask(c1, sm, si, gamma, beta)
    assert not bool(mask[2, 7, h, w])
    closed = torch.where(mask[2, 7], d_a1[2, 7].double(), torch.zeros((), dtype=torch.float64, device=DEV)).sum()
    opened = closed + d_a1[2, 7, h, w].double()
    aten_dz = torch.ops.aten.threshold_backward(d_a1, a1, 0)
    assert float(aten_dz[2, 7, h, w]) == float(d_a1[2, 7, h, w]) != 0.0  # ATen: open
    assert abs(float(sums[7, 2, 0]) - float(closed)) <= 1e-5 * float(d_a1[2, 7].abs().sum()) < abs(float(opened - closed)) / 10  # ours: closed
    assert bool(torch.isnan(sums[7, 2, 1]))
    aten_dx = torch.ops.aten.native_batch_norm_backward(aten_dz, c1, gamma, None, None, sm, si, True, eps, [True, False, False])[0]
    dx_bn = ops.bn_act_bwd(d_a1, None, c1, gamma, sm, si, None, None, eps, True, True, True, False, False, None, beta)[0]
    u_id = Fn.wino_sets(_identity_filter(C))[1]
    dx_pre = ops.wino3x3_bn_train_bwd_pre(d_a1, c1, sums, H * H, sm, si, gamma, beta, u_id)
    nan_channel = torch.zeros(B, C, H, H, dtype=torch.bool, device=DEV)
    nan_channel[:, 7] = True
    assert torch.equal(torch.isnan(aten_dx), nan_channel)
    assert torch.equal(torch.isnan(dx_bn), nan_channel)
    dx64 = _bn_relu_bwd64(d_a1, torch.nan_to_num(c1), mask, sm, si, gamma)[0]
    fine = ~nan_channel
    e_nan = float((dx_bn.double() - dx64)[fine].abs().max())
    print("    ee_bn_act_bwd2_f32 next to a NaN channel: max |d| %.3e of max |dx| %.3e" % (e_nan, float(dx64[fine].abs().max())))
    assert e_nan <= GATE_BAR_DX * float(dx64[fine].abs().max())
    # the consumer half is read through conv1^T: the matrix product multiplies the NaN channel into every result channel (0 * NaN), exactly as
    # ATen's dx does when it is pushed through the same convolution
    assert torch.equal(torch.isnan(dx_pre), torch.isnan(ops.wino3x3(aten_dx, u_id))) and bool(torch.isnan(dx_pre).all())


@pytest.mark.parametrize("C", [64, 32, 128])
@pytest.mark.parametrize("B", [100, 5, 3, 9])
def test_boundary_backward_against_float64(ops, B, C):
    """ee_wino3x3_bwd_sums_f32 + ee_wino3x3_bn_train_bwd_pre_f32 on 16x16 maps against float64 conv1^T(bn_relu_backward(conv2^T dc2)) -
    torch.nn.grad.conv2d_input in float64 both times, the mask from the fp32 expression - no further from it than twice the unfused sequence
    ee_wino3x3_f32 | ee_bn_act_bwd2_f32 | ee_wino3x3_f32 is, + 1e-7 of the largest entry.
    Measured (MI355X; max |d| from float64 of the largest entry 6.1 ... 7.8, kernel / unfused sequence): 1.8e-6 ... 5.1e-6 / 1.8e-6 ... 5.3e-6 over the twelve
    shapes, the two within 7 % of each other on every shape (bit-equal on six)."""
    from eeadv import functional as Fn
    H, eps = 16, 1e-5
    gen = torch.Generator().manual_seed(B + C)
    c1 = torch.randn(B, C, H, H, generator=gen).to(DEV)
    dc2 = torch.randn(B, C, H, H, generator=gen).to(DEV)
    w1, w2 = _conv_w(C, C, 3, gen), _conv_w(C, C, 3, gen)
    gamma, beta = (torch.rand(C, generator=gen) + 0.5).to(DEV), (torch.randn(C, generator=gen) * 0.2).to(DEV)
    sm = c1.mean((0, 2, 3)).contiguous()
    si = (1.0 / torch.sqrt(c1.var((0, 2, 3), unbiased=False) + eps)).contiguous()
    u1b, u2b = Fn.wino_sets(w1)[1], Fn.wino_sets(w2)[1]
    d_a1_64 = torch.nn.grad.conv2d_input(c1.shape, w2.double(), dc2.double(), padding=1)
    d_c1_64 = _bn_relu_bwd64(d_a1_64, c1, train_pre_mask(c1, sm, si, gamma, beta), sm, si, gamma)[0]
    ref = torch.nn.grad.conv2d_input(c1.shape, w1.double(), d_c1_64, padding=1)
    d_a1 = ops.wino3x3(dc2, u2b)
    d_c1 = ops.bn_act_bwd(d_a1, None, c1, gamma, sm, si, None, None, eps, True, True, True, False, False, None, beta)[0]
    sibling = ops.wino3x3(d_c1, u1b)
    d_a1b, sums = ops.wino3x3_bwd_sums(dc2, u2b, c1, sm, si, gamma, beta)
    got = ops.wino3x3_bn_train_bwd_pre(d_a1b, c1, sums, H * H, sm, si, gamma, beta, u1b)
    print("  boundary backward B=%d C=%d" % (B, C))
    _twice_the_sibling(got, sibling, ref, "conv1^T(bn_relu_bwd(conv2^T))")


@pytest.mark.parametrize("B,C,H,W,two", [(100, 64, 32, 32, True), (3, 64, 32, 32, False), (5, 16, 14, 20, True), (2, 8, 7, 12, False)])
def test_stem_backward_from_pooled_sums_against_float64(ops, B, C, H, W, two):
    """ee_bn_relu_pool_bwd_xa_f32 (the batch sums from the pooled gradient and x at every window's argmax): dx, dgamma, dbeta against float64
    autograd of gather(batch_norm(x64), argmax named by `code`) * (y > 0), one and two incoming gradients - no further than twice
    ee_bn_relu_pool_bwd_f32 (which reads the full-resolution map twice) is, + 1e-7 of the largest entry.
    Measured (MI355X; max |d| from float64, kernel / sibling, largest entry): 100x64x32x32 two: dx 3.3e-6 / 3.3e-6 of 17.8, dgamma 1.9e-4 / 1.7e-4 of 1184,
    dbeta 1.4e-4 / 1.2e-4 of 508; 3x64x32x32: 1.5e-6 / 1.5e-6 of 8.6, 8.7e-6 / 1.9e-5 of 118, 5.3e-6 / 8.4e-6 of 83; 5x16x14x20 two: 1.5e-6 / 1.5e-6 of 10.8,
    1.1e-5 / 8.3e-6 of 74, 4.3e-6 / 3.9e-6 of 47; 2x8x7x12: 7.5e-7 / 7.5e-7 of 5.0, 1.6e-6 / 6.9e-7 of 8.4, 1.0e-6 / 1.1e-6 of 9.4."""
    g = torch.Generator(device="cpu").manual_seed(B * C + H)
    x = torch.randn(B, C, H, W, generator=g).to(DEV)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(DEV), torch.randn(C, generator=g).to(DEV)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    y, code, sm, si, xa = ops.bn_relu_pool_fwd(x, gamma, beta, rm.clone(), rv.clone(), 0.1, 1e-5, True, None, True)
    dyp = torch.randn(y.shape, generator=g).to(DEV)
    dyp2 = torch.randn(y.shape, generator=g).to(DEV) if two else None
    x64, g64, b64 = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z64 = F.batch_norm(x64, None, None, g64, b64, True, 0.0, 1e-5)
    out64 = z64.flatten(2).gather(2, pool_code_to_index(code, W).flatten(2)).view(y.shape) * (y > 0).double()
    torch.testing.assert_close(y.double(), out64.detach(), rtol=1e-5, atol=1e-5)  # the reference IS the kernel's forward
    refs = torch.autograd.grad(out64, [x64, g64, b64], dyp.double() if dyp2 is None else dyp.double() + dyp2.double())
    sibling = ops.bn_relu_pool_bwd(dyp, code, x, gamma, beta, sm, si, rm, rv, 1e-5, True, True, True, dyp2)
    got = ops.bn_relu_pool_bwd(dyp, code, x, gamma, beta, sm, si, rm, rv, 1e-5, True, True, True, dyp2, xa)
    print("  stem backward B=%d C=%d %dx%d two=%s" % (B, C, H, W, two))
    for a, s, r, name in zip(got, sibling, refs, ("dx", "dgamma", "dbeta")):
        _twice_the_sibling(a, s, r, name)


@pytest.mark.parametrize("B,C,HW,K,reduction", [(100, 512, 4, 200, "sum"), (3, 2048, 49, 1000, "mean"), (1, 64, 1, 10, "sum"), (7, 300, 4, 33, "mean")])
def test_cross_entropy_head_backward_against_float64(ops, B, C, HW, K, reduction):
    """ee_ce_pool_linear_bwd_f32 against float64 autograd of F.cross_entropy(F.linear(feat64.mean((2, 3)), w64, b64), y, reduction) with respect
    to feat64 - no further than twice ee_ce_f32 followed by ee_pool_linear_bwd_f32 is, + 1e-7 of the largest entry.
    Measured (MI355X; the two are bit-equal, so kernel = sibling): 4.6e-8 of 5.3e-2, 6.5e-10 of 6.8e-4, 3.7e-8 of 0.43, 2.8e-9 of 7.9e-3."""
    g = torch.Generator(device="cpu").manual_seed(B * C + K)
    side = int(HW ** 0.5)
    feat = torch.randn(B, C, side, side, generator=g).to(DEV)
    w = (torch.randn(K, C, generator=g) / C ** 0.5).to(DEV)
    bias = torch.randn(K, generator=g).to(DEV)
    y = torch.randint(0, K, (B,), generator=g).to(DEV)
    f64 = feat.double().requires_grad_(True)
    (ref,) = torch.autograd.grad(F.cross_entropy(F.linear(f64.mean((2, 3)), w.double(), bias.double()), y, reduction=reduction), f64)
    logits, _ = ops.pool_linear_fwd(feat, w, bias)
    sibling = ops.pool_linear_bwd(ops.ce(logits, y, reduction, 0.0, False, True)[1], w, tuple(feat.shape))
    got = ops.ce_pool_linear_bwd(logits, y, w, tuple(feat.shape), reduction)
    print("  head backward B=%d C=%d HW=%d K=%d %s" % (B, C, HW, K, reduction))
    _twice_the_sibling(got, sibling, ref, "d loss / d feat")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. the headline configuration against the oracle, at its own size
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_headline_configuration_replayed_against_the_oracle(monkeypatch):
    """resnet18_EE_square as configs_tinyimagenet/ee_at_bpda3_square.yml builds it, TRAIN mode, batch 100, PGD-10 (epsilon 16/255, step 2/255,
    r 8, thresholds 38 / 76) with an injected start noise and injected Add_Square draws.  The oracle (oracle/ref_path.py, fp32 on the host)
    runs the ten iterations and records every iterate x_k, what its front end hands to the CNN (x_in_k), its logits and its gradients; for
    every k the GPU model is fed the ORACLE's tensors (tests/replay.py: a free-running attack cannot stay on the trajectory):
      front end   front_chain(x_k, draws_k) vs x_in_k: no element off by more than 1e-5;
      logits      of the body on x_in_k: atol 1e-4, argmax equal;
      gradient    of the body at x_in_k against a float64 copy of the body alone (train mode) ON THE BRANCH THE GPU RUN TOOK (branch_replay.Branch):
                  ||g_gpu - g64|| <= ABS_BAR[100] * ||g64||, the bar of section 1, and nothing else.  DEVIATION 1 from the plan of tests/replay.py
                  (a free-running float64 body, ||g_gpu - g64|| <= 2 ||g_ref - g64|| + 1e-6 ||g64||, switch_tol in at most 2 of 10 steps): with
                  a free-running float64 body that budget compares two sets of mask flips, not arithmetic.  Measured that way on MI355X (19 M
                  pre-activations per forward at batch 100, a handful within fp32 rounding of zero in any implementation): GPU 0.8e-3 ... 8.0e-3
                  of ||g64||, the host reference 1.7e-3 ... 4.5e-3, 20 ... 1014 against 76 ... 378 sign disagreements - the GPU nearer than the
                  reference in 2 steps, outside twice its distance in 4.  On the GPU's branch the reference's distance (3.9e-3 ... 7.7e-3, it sits
                  on another branch) says nothing, so the budget is not asserted; the reference's figures are only printed;
      iteration   front_chain | engine._body_input_grad | front_chain_update_ (what engine.attack_step_ runs once chain_ok holds) from x_k:
                  the oracle's x_{k+1} wherever the two moved the pixel in the same direction, in more than 99 % of the pixels (the
                  suite's criterion for this model, test_pgd_on_ee_model_matches_oracle);
      NaN pattern a flat patch the start noise leaves alone has zero edge magnitude and a NaN gradient (0 * inf).  Through autograd
                  (model(x_k, draws_k), the same kernels' backward one by one) isnan(gradient) equals the oracle's exactly.  DEVIATION 2: the
                  chain never materialises d loss / d x_k, so there the pattern is read from the update: no pixel moves where the oracle's
                  gradient is NaN, and a pixel the chain left in place although the oracle moved it must be one where a step AGAINST the
                  oracle's direction is clamped back onto x_k (a sign flip at the edge of the epsilon box or of [0, 1]) - a NaN the chain
                  produced where the oracle's gradient is finite would be a stuck pixel without that excuse;
      statistics  after the ten forwards all 20 BatchNorms' running statistics against the float64 body's (it saw the same ten inputs;
                  rtol 1e-5 mean / 1e-4 var, atol 1e-6, the bars of section 1) and against the oracle's (twice those: two fp32 paths),
                  num_batches_tracked == 10.
    Measured (MI355X, the ten steps): front end 0 elements off; logits 7.5e-6 ... 1.0e-5; body gradient 1.75e-6 ... 1.95e-6 of ||g64|| (the host reference, on its own
    branch, 3.9e-3 ... 7.7e-3), 0 ... 3 sign disagreements of 1 228 800 (the reference 338 ... 886); iterate equal in 99.942 ... 99.987 %
    of the pixels; 2016 NaN gradients in every step, the same set through autograd; 2 ... 38 pixels per step left in place against the oracle's move, every one
    at the edge of its box; running statistics at most 0.09 (mean) / 0.005 (var) of the tolerance against float64."""
    from eeadv import engine, functional
    from oracle import ref_path as R
    from test_gpu_path import _ee_pair
    m, ref = _ee_pair(True)
    m.train(), ref.train()
    aux = _ee_pair(True)[0].train()  # the same weights again (same seed) for the logits and the full iteration: extra forwards, kept away from the statistics under test
    from eeadv import models
    from branch_replay import Branch
    net64 = models.make_resnet(18, "tiny").double().to(DEV).train()
    net64.load_state_dict({k: v for k, v in m.state_dict().items() if k in net64.state_dict()})
    stock = models._STOCK
    assert len(_bn_layers(m)) == len(_bn_layers(net64)) == len(_bn_layers(ref.net)) == 20
    B, K, eps, alpha = 100, 10, 0.062745098039216, 0.007843137254902
    gen = torch.Generator().manual_seed(31)
    x = torch.rand(B, 3, 64, 64, generator=gen)
    x[3, :, 20:44, 12:40] = 0.5
    y = torch.randint(0, 200, (B,), generator=gen)
    noise = (torch.rand(B, 3, 64, 64, generator=gen) * 2 - 1) * eps
    noise[3, :, 20:44, 12:40] = 0.0
    torch.manual_seed(32)  # the oracle's Add_Square draws (host generator)
    # ---- the oracle: ten iterations on the host ----
    xs, steps = [torch.clamp(x + noise, 0, 1)], []
    for k in range(K):
        draws = ref.front.add_square.draw(B)
        xr = xs[k].clone().requires_grad_(True)
        x_in = ref.front(xr, draws)
        logits = ref.net(x_in)
        g, g_in = torch.autograd.grad(F.cross_entropy(logits, y, reduction="sum"), [xr, x_in])
        steps.append(dict(draws=draws, x_in=x_in.detach(), logits=logits.detach(), g=g, g_in=g_in))
        xs.append(R._step(xs[k], g, x, alpha, eps))
    assert int(torch.isnan(steps[0]["g"]).sum()) > 0
    # ---- the replay ----
    spec = engine.LossSpec(engine.CE_SUM, y.to(DEV))
    x0 = x.to(DEV)
    n = steps[0]["g_in"].numel()
    for k, s in enumerate(steps):
        xk = xs[k].to(DEV)
        dd = {"stripe": s["draws"]["stripe"].to(DEV), "sq_pos": s["draws"]["sq_pos"].to(DEV), "sq_sign": s["draws"]["sq_sign"].reshape(1, 3).to(DEV)}
        # front end
        assert aux.chain_ok(xk)
        with torch.no_grad():
            x_in_gpu, ctx = aux.front_chain(xk, dd)
        off = int(((x_in_gpu.cpu() - s["x_in"]).abs() > 1e-5).sum())
        assert off == 0, "step %d: %d front-end outputs differ (an edge bit flipped?)" % (k, off)
        # logits of the body on the oracle's x_in_k
        x_in_ref = s["x_in"].to(DEV)
        with torch.enable_grad(), functional.attack_forward():
            logits = aux.head_from_pre(aux.body_pre(x_in_ref.clone().requires_grad_(True))).detach().cpu()
        e_logit = float((logits - s["logits"]).abs().max())
        assert e_logit <= 1e-4 and torch.equal(logits.argmax(1), s["logits"].argmax(1)), (k, e_logit)
        # body gradient on the oracle's x_in_k: the model under test's ONE forward of this step
        br = Branch(monkeypatch, models)
        br.record()
        g_gpu = engine._body_input_grad(m, x_in_ref.clone().requires_grad_(True), spec, True).detach().double()
        todo = br.replay()
        monkeypatch.setattr(models, "_STOCK", ALL_STOCK)
        x64 = x_in_ref.double().requires_grad_(True)
        (g64,) = torch.autograd.grad(F.cross_entropy(net64(x64), y.to(DEV), reduction="sum"), x64)
        monkeypatch.setattr(models, "_STOCK", stock)
        br.restore()
        assert not todo and len(br.masks) == 17 and br.calls == {"train_pre": 2, "pool_fwd": 1, "pool_fwd_xa": 1, "ce_head": 1}, br.calls
        g_ref = s["g_in"].to(DEV).double()
        e_gpu, e_ref, n64 = float((g_gpu - g64).norm()), float((g_ref - g64).norm()), float(g64.norm())
        f_gpu, f_ref = int((torch.sign(g_gpu) != torch.sign(g64)).sum()), int((torch.sign(g_ref) != torch.sign(g64)).sum())
        assert e_gpu <= ABS_BAR[100] * n64, (k, e_gpu / n64)
        # NaN pattern through autograd: the whole model on the oracle's x_k with its draws
        xa = xk.clone().requires_grad_(True)
        (g_auto,) = torch.autograd.grad(F.cross_entropy(aux(xa, dd), y.to(DEV), reduction="sum"), xa)
        assert torch.equal(torch.isnan(g_auto).cpu(), torch.isnan(s["g"])), "step %d: NaN pattern of the input gradient differs" % k
        # the full iteration from the oracle's x_k
        x_in_gpu.requires_grad_(True)
        g_in = engine._body_input_grad(aux, x_in_gpu, spec, True)
        x_next = xk.clone()
        with torch.no_grad():
            aux.front_chain_update_(x_next, g_in.contiguous(), ctx, x0, alpha, eps, 0.0, 1.0, 1)
        x_next, want = x_next.cpu(), xs[k + 1]
        moved_same = x_next == want
        same_dir = torch.sign(x_next - xs[k]) == torch.sign(want - xs[k])
        agree = float(moved_same.float().mean())
        stuck = (x_next == xs[k]) & (want != xs[k])
        against = R._step(xs[k], -(want - xs[k]), x, alpha, eps)  # a step against the oracle's direction
        print("step %d: logits %.2e  body gradient from float64: GPU %.3e (reference, another branch: %.3e) of |g64|, signs %d / %d of %d; iterate equal in %.3f %%; "
              "NaN gradients %d; left in place against the oracle's move: %d"
              % (k, e_logit, e_gpu / n64, e_ref / n64, f_gpu, f_ref, n, 100 * agree, int(torch.isnan(s["g"]).sum()), int(stuck.sum())))
        assert bool((against == xs[k])[stuck].all()), "step %d: %d pixels left in place that a sign flip cannot explain (NaN?)" % (k, int(((against != xs[k]) & stuck).sum()))
        assert bool((moved_same | ~same_dir).all()), "step %d: same direction but a different iterate" % k
        assert agree > 0.99, (k, agree)
        assert bool((x_next == xs[k])[torch.isnan(s["g"])].all()), "step %d: a NaN-gradient pixel moved" % k
    # running statistics after the ten forwards
    worst = [0.0, 0.0]
    for (name, b), (_, b64), (_, bo) in zip(_bn_layers(m), _bn_layers(net64), _bn_layers(ref.net)):
        assert int(b.num_batches_tracked) == int(bo.num_batches_tracked) == 10, name
        worst[0] = max(worst[0], float(((b.running_mean.double() - b64.running_mean).abs() / (1e-5 * b64.running_mean.abs() + 1e-6)).max()))
        worst[1] = max(worst[1], float(((b.running_var.double() - b64.running_var).abs() / (1e-4 * b64.running_var.abs() + 1e-6)).max()))
        torch.testing.assert_close(b.running_mean.double(), b64.running_mean, rtol=1e-5, atol=1e-6, msg=lambda t: name + ".running_mean vs float64: " + t)
        torch.testing.assert_close(b.running_var.double(), b64.running_var, rtol=1e-4, atol=1e-6, msg=lambda t: name + ".running_var vs float64: " + t)
        torch.testing.assert_close(b.running_mean.cpu(), bo.running_mean, rtol=2e-5, atol=2e-6, msg=lambda t: name + ".running_mean vs oracle: " + t)
        torch.testing.assert_close(b.running_var.cpu(), bo.running_var, rtol=2e-4, atol=2e-6, msg=lambda t: name + ".running_var vs oracle: " + t)
    print("running statistics vs float64, worst |d| / (rtol |ref| + atol): mean %.3f var %.3f" % (worst[0], worst[1]))
