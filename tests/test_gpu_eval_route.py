"""The route every evaluation attack runs on - engine.input_gradient in EVAL mode, where models.eval_block replaces each BasicBlock with
functional.EvalBasicBlockFn / EvalDownBlockFn and all 19 convolutions behind the stem run with the running-statistics BatchNorm, the
residual and the ReLU folded into the convolution kernels - pinned to float64.

tests/test_gpu_evalfuse.py holds these kernels bit-equal to the unfused kernel sequence; since the two share their BatchNorm expressions
that cannot see an error in what they share, nor in how functional.py puts the pieces together (gamma * invstd in the backward, the gate
from the block's output, the residual gradient through dx_add, the two-piece gradient of a forked output, the shortcut's BatchNorm).
Section 1 compares the whole body with the float64 stock modules on the ReLU branch the fp32 run took (tests/branch_replay.py); section 2
compares each fused kernel, and section 3 the two block Functions, with the float64 restatement of tests/eval_route_reference.py - never
with another ee_* kernel on the reference side.

Bars.  Binding ones are relative to something that is not the code under test: "no further from float64 than twice X is on the same
inputs", X being the all-stock fp32 path (section 1) or the unfused kernel sequence test_gpu_evalfuse.py names (sections 2, 3), plus a
floor of 1e-6 of the gradient's norm / 1e-7 of the reference's largest entry.  The absolute bars of section 1 are stated next to what was
measured on MI355X."""
import copy

import pytest
import torch
import torch.nn.functional as F

import eval_route_reference as E
from bn_reference import hard_affine
from branch_replay import ALL_STOCK, replayed_attack_gradient

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
U = 2.0 ** -24  # unit roundoff of fp32


@pytest.fixture(scope="module")
def ops():
    from eeadv import ops as _ops
    return _ops


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the whole body on the eval-mode attack route
# ---------------------------------------------------------------------------------------------------------------------------------------
# Absolute bars: 4x the largest value measured on MI355X over the cases of this section, and never above 1e-4 (logits: max |d|; gradient:
# of ||g64|| - one flipped mask costs 1.5e-3 ... 3.9e-3 of it, tests/branch_replay.py).
# Measured (MI355X, the six cases below): logits max |d| 2.16e-6 ... 2.50e-6 (largest logit 4.4) -> LOGIT_BAR = 1.0e-5; ||g32 - g64|| / ||g64||
# 8.76e-7 ... 9.22e-7 (the all-stock fp32 eval path 6.44e-7 ... 7.38e-7) -> GRAD_BAR = 3.7e-6.
LOGIT_BAR = 1.0e-5
GRAD_BAR = 3.7e-6
_STOCK_DISTANCE = {}  # (B, seed, kind, cotangent) -> the all-stock fp32 eval path's distance from float64 under the same procedure


def _fused_routes(net):
    return [n for n, m in net.named_modules() if isinstance(m, torch.nn.Conv2d) and m.__dict__.get("_ee_route", "").endswith("+bn")]


def _cotangent(B, seed):
    return torch.randn(B, 200, generator=torch.Generator().manual_seed(1000 + seed)).to(DEV)


def _eval_route_case(monkeypatch, B, seed, kind, cotangent=False, fold=False):
    from eeadv import engine, functional, models, ops
    monkeypatch.setattr(functional, "_DENSE_FOLD_BWD", fold)
    folded = [0]
    dense_bwd = ops.dense2x2_bn_eval_bwd

    def counted(*a, **k):
        folded[0] += 1
        return dense_bwd(*a, **k)
    monkeypatch.setattr(ops, "dense2x2_bn_eval_bwd", counted)
    dl = _cotangent(B, seed) if cotangent else None
    r = replayed_attack_gradient(monkeypatch, B, seed, kind, mode="eval", cotangent=dl)
    net, twin, calls = r["net32"], r["twin"], r["calls"]
    # the route under test is the route taken: 16 3x3 + 3 shortcut convolutions folded, nothing on a vendor library; the 13 stride-1
    # convolutions through functional._eval_conv_fwd and the 3 stride-2 pairs make the 16 ReLUs behind the stem's
    assert len(_fused_routes(net)) == 19, _fused_routes(net)
    assert models.fallback_report(net)["count"] == 0, models.fallback_report(net)
    assert calls == {"train_pre": 0, "pool_fwd": 1, "pool_fwd_xa": 0, "ce_head": 0 if cotangent else 1, "eval_conv": 13, "eval_pair": 3}, calls
    assert calls["eval_conv"] + calls["eval_pair"] == 16 and r["n_relu"] == 17  # (none left over: replayed_attack_gradient asserts it)
    assert folded[0] == (3 if fold else 0), folded  # layer 4's three 2x2 convolutions on ee_dense2x2_bn_eval_bwd_f32
    # an eval-mode forward changes no running statistic, no counter (and no parameter)
    before, after = twin.state_dict(), net.state_dict()
    assert len(before) == len(after) == 122 and sum(k.endswith("num_batches_tracked") for k in after) == 20
    for k in after:
        assert torch.equal(before[k], after[k]), k
    # logits of the same forward, from a second deep copy
    with torch.enable_grad(), functional.attack_forward():
        twin2 = copy.deepcopy(twin)
        logits = twin2(r["x"].clone().requires_grad_(True)).detach()
    assert len(_fused_routes(twin2)) == 19
    e_logit = float((logits.double() - r["logits64"]).abs().max())
    what = "cotangent" if cotangent else kind
    print("eval route B=%d seed=%d %s fold=%s: logits max |d| %.3e of max |logit| %.3e" % (B, seed, what, fold, e_logit, float(r["logits64"].abs().max())))
    # the input gradient
    rel = float((r["g32"].double() - r["g64"]).norm() / r["g64"].norm())
    key = (B, seed, kind, cotangent)
    if key not in _STOCK_DISTANCE:
        s = replayed_attack_gradient(monkeypatch, B, seed, kind, fp32_stock=ALL_STOCK, mode="eval", cotangent=dl)
        assert s["calls"] == {"train_pre": 0, "pool_fwd": 0, "pool_fwd_xa": 0, "ce_head": 0, "eval_conv": 0, "eval_pair": 0}, s["calls"]
        assert not _fused_routes(s["net32"])
        _STOCK_DISTANCE[key] = float((s["g32"].double() - s["g64"]).norm() / s["g64"].norm())
        del s
    rel_stock = _STOCK_DISTANCE[key]
    print("    input gradient |g32 - g64| / |g64|: this route %.3e, all-stock fp32 %.3e" % (rel, rel_stock))
    assert rel <= 2 * rel_stock + 1e-6, (rel, rel_stock)
    assert e_logit <= LOGIT_BAR, e_logit
    assert rel <= GRAD_BAR, rel
    assert float(r["g32"].abs().max()) > 0
    # the same bits from a fresh deep copy of the model
    monkeypatch.setattr(models, "_STOCK", frozenset())  # (the yardstick run above left the all-stock setting)
    g_again = engine.input_gradient(twin, r["x"].clone(), r["spec"]).detach()
    assert torch.equal(g_again, r["g32"])
    return rel, rel_stock


@pytest.mark.parametrize("seed", [0, 1])
def test_eval_route_input_gradient_equals_float64_on_the_same_branch(monkeypatch, seed):
    """make_resnet(18, 'tiny').eval() with every BatchNorm moved away from its initial state, engine.input_gradient(model, x, LossSpec(CE_SUM, y))
    at batch 16 with nothing stocked (ResNet.head_grad with ops.ce_pool_linear_bwd), against the float64 stock modules with all 17 ReLU masks
    and the stem argmax replayed (branch_replay.replayed_attack_gradient(mode="eval")).
    Asserted: the route taken (19 convolutions folded, none on a vendor library, 13 _eval_conv_fwd + 3 pair forwards, 17 masks, none left
    over); no running statistic, counter or parameter moved (torch.equal); ||g32 - g64|| / ||g64|| at most twice the all-stock fp32 eval
    path's under the same procedure + 1e-6, and at most GRAD_BAR; logits within LOGIT_BAR; the same bits from a fresh deep copy.
    Measured (MI355X): 8.76e-7 / 9.06e-7 of ||g64|| (seeds 0 / 1), the all-stock fp32 path 7.33e-7 / 7.37e-7; logits 2.39e-6 / 2.50e-6."""
    _eval_route_case(monkeypatch, 16, seed, "ce_sum")


def test_eval_route_mean_reduction_equals_float64_on_the_same_branch(monkeypatch):
    """The same with LossSpec(CE_MEAN, y): ops.ce_pool_linear_bwd's other reduction.
    Measured (MI355X): 8.76e-7 of ||g64||, the all-stock fp32 path 7.38e-7; logits 2.39e-6."""
    _eval_route_case(monkeypatch, 16, 0, "ce_mean")


def test_eval_route_odd_batch_equals_float64_on_the_same_branch(monkeypatch):
    """The same at batch 5: partial image tiles in the Winograd kernels (4 images per workgroup on 4x4 maps, 2 on 8x8) and the stride-2 kernels.
    Measured (MI355X): 8.97e-7 of ||g64||, the all-stock fp32 path 6.44e-7; logits 2.16e-6."""
    _eval_route_case(monkeypatch, 5, 0, "ce_sum")


def test_eval_route_logit_cotangent_equals_float64_on_the_same_branch(monkeypatch):
    """The same at batch 16 with a random cotangent on the logits (branch_replay.LogitCotangent): the branch of engine._body_input_grad that
    APGD's DLR loss and FAB's logit differences take - model(x) under attack_forward(), then PoolLinearFn's backward; ce_pool_linear_bwd does not run.
    Measured (MI355X): 9.22e-7 of ||g64||, the all-stock fp32 path 7.26e-7; logits 2.39e-6."""
    _eval_route_case(monkeypatch, 16, 0, "ce_sum", cotangent=True)


def test_eval_route_with_layer4_backward_folded_equals_float64_on_the_same_branch(monkeypatch):
    """The same at batch 16 with functional._DENSE_FOLD_BWD on: layer 4's three 2x2 backward products run as ee_dense2x2_bn_eval_bwd_f32 (built, not
    the default); asserted that they do.
    Measured (MI355X): 8.84e-7 of ||g64||, the all-stock fp32 path 7.33e-7; logits 2.39e-6."""
    _eval_route_case(monkeypatch, 16, 0, "ce_sum", fold=True)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. each fused kernel against the float64 restatement
# ---------------------------------------------------------------------------------------------------------------------------------------
def _err(a, ref):
    return float((a.detach().double() - ref).abs().max())


def _rule(e_g, e_s, top, what):
    """the kernel is no further from float64 than twice the unfused sequence is, plus 1e-7 of the reference's largest entry"""
    print("    %-34s kernel %.3e  unfused sequence %.3e  of max |ref| %.3e" % (what, e_g, e_s, top))
    assert e_g <= 2 * e_s + 1e-7 * top, "%s: %.3e from float64, the unfused sequence %.3e (max |ref| %.3e)" % (what, e_g, e_s, top)


def _twice_the_sibling(got, sibling, ref, what):
    _rule(_err(got, ref), _err(sibling, ref), float(ref.abs().max()), what)


def _forward_rule(got, sibling, pre64, relu, what):
    """every element compared: with a ReLU `got` against pre64 gated by got's own sign (the sibling by its own); a gate that is wrongly
    CLOSED shows in the second assertion: wherever got == 0 the float64 pre-activation is at most the sibling's distance above zero"""
    top = float(pre64.abs().max())
    e_g = _err(got, E.gate(pre64, got) if relu else pre64)
    e_s = _err(sibling, E.gate(pre64, sibling) if relu else pre64)
    _rule(e_g, e_s, top, what)
    if relu:
        closed = got == 0
        share = float(closed.float().mean())
        assert bool(closed.any()) and not bool(closed.all()) and (got.numel() < 1024 or 0.1 < share < 0.9)  # the ReLU bites
        worst = float(pre64[closed].max())
        print("    %-34s closed gates %.3f of the elements, largest float64 pre-activation under one %.3e" % ("", share, worst))
        assert worst <= 2 * e_s + 1e-7 * top, "%s: a gate is closed over a pre-activation of %.3e" % (what, worst)


def _w(co, ci, k, gen):
    return (torch.randn(co, ci, k, k, generator=gen) * (2.0 / (k * k * ci)) ** 0.5).to(DEV)


def _bn(C, gen, affine, roll=0, edge=True):
    """(gamma, beta, running_mean, running_var) on the device: affine 'rand' as test_gpu_evalfuse._bn draws it, 'hard' = bn_reference.hard_affine
    (gamma of both signs and zero); edge: the running statistics carry eval_route_reference.edge_statistics' three hard channels"""
    g, b = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
    if affine == "hard":
        g, b = hard_affine(C, roll)
    if edge:
        rm, rv, _ = E.edge_statistics(C, gen, g)
    else:
        rm, rv = torch.randn(C, generator=gen) * 0.2, torch.rand(C, generator=gen) + 0.3
    return tuple(t.to(DEV).contiguous() for t in (g, b, rm, rv))


def _mask_tensor(shape, gen):
    """a forward output to take the ReLU mask from: about half exact zeros, 10 % the smallest positive float (torch.nextafter(0, 1): an open
    gate), the rest positive.  The boolean mask is formed on the host."""
    y = torch.relu(torch.randn(shape, generator=gen))
    tiny = torch.nextafter(torch.zeros(()), torch.ones(()))
    planted = torch.rand(shape, generator=gen) < 0.1
    y = torch.where(planted, tiny, y)
    assert float(tiny) > 0 and int((y == tiny).sum()) > 0 and int((y == 0).sum()) > 0
    return y.to(DEV), (y > 0).to(DEV), planted.to(DEV)


def _dres_rule(dres, dz64, planted, what):
    """dz = (dy [+ dy2]) * mask is ONE fp32 addition: within half an ulp of the float64 value at every element, exactly 0 under a closed
    gate - also where the mask tensor holds the smallest positive float (an open gate)"""
    d = (dres.double() - dz64).abs()
    assert bool((d <= U * dz64.abs()).all()), "%s: residual gradient off by %.3e" % (what, float(d.max()))
    assert bool((dres[planted] != 0).any())


WINO_SHAPES = [(1, 32, 32, 4), (2, 32, 32, 8), (3, 32, 32, 16), (5, 64, 64, 16), (3, 128, 128, 8), (7, 256, 256, 4), (2, 64, 96, 8)]
_WINO_IDS = ["%dx%d-%dx%d" % s for s in WINO_SHAPES]


@pytest.mark.parametrize("B,Cin,Cout,H", WINO_SHAPES, ids=_WINO_IDS)
@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("affine", ["rand", "hard"])
def test_wino_bn_eval_forward_against_float64(ops, B, Cin, Cout, H, with_res, affine):
    """ee_wino3x3_bn_eval_fwd_f32 against conv2d -> (c - rm) / sqrt(rv + eps) * g + b -> + res -> ReLU in float64, with and without the
    ReLU and gamma / beta; running variance 1e-6 and 1e3 and a running mean 75 (50 spreads of conv's output) on three live channels.  No
    further than twice ee_wino3x3_f32 | ee_bn_act_fwd_f32 is, + 1e-7 of the largest entry; no gate closed over a positive pre-activation.
    Measured (MI355X): max |d| from float64, of the largest entry (5.6e2 ... 1.9e3: the channel with variance 1e-6), over the 112 comparisons:
    1.3e-7 ... 4.7e-7, the unfused sequence the same figures (bit-equal); closed gates 0.47 ... 0.54 of the elements, the largest float64
    pre-activation under one -9.9e-7."""
    from eeadv import functional as Fn
    gen = torch.Generator().manual_seed(B * 1000 + Cin + Cout + H)
    x = torch.randn(B, Cin, H, H, generator=gen).to(DEV)
    w = _w(Cout, Cin, 3, gen)
    res = torch.randn(B, Cout, H, H, generator=gen).to(DEV) if with_res else None
    g, b, rm, rv = _bn(Cout, gen, affine)
    u = Fn.wino_sets(w)[0]
    print("  wino forward B=%d %d->%d H=%d res=%s %s" % (B, Cin, Cout, H, with_res, affine))
    for relu, gg, bb in ((True, g, b), (False, g, b), (True, None, None), (False, None, None)):
        pre64 = E.conv_bn_fwd64(x, w, (rm, rv, gg, bb, EPS), res)
        sibling = ops.bn_act_fwd(ops.wino3x3(x, u), res, gg, bb, rm, rv, 0.1, EPS, False, relu)[0]
        got = ops.wino3x3_bn_eval_fwd(x, u, (rm, rv, gg, bb, EPS), res, relu)
        _forward_rule(got, sibling, pre64, relu, "relu=%s affine=%s" % (relu, gg is not None))


_BWD_FORMS = [(1, False, False), (2, True, False), (1, True, True), (2, False, True), (2, True, True)]


@pytest.mark.parametrize("B,Cin,Cout,H", WINO_SHAPES, ids=_WINO_IDS)
@pytest.mark.parametrize("pieces,want_dres,with_add", _BWD_FORMS, ids=["%d-%s-%s" % f for f in _BWD_FORMS])
@pytest.mark.parametrize("affine", ["rand", "hard"])
def test_wino_bn_eval_backward_against_float64(ops, B, Cin, Cout, H, pieces, want_dres, with_add, affine):
    """ee_wino3x3_bn_eval_bwd_f32 against dz = (dy [+ dy2]) * (y > 0), dx = conv2d_input(dz * g / sqrt(rv + eps)) [+ dx_add] in float64; y holds
    exact zeros and the smallest positive float.  dx no further than twice ee_bn_act_bwd2_f32 | ee_wino3x3_f32 [+ dx_add] is, + 1e-7 of the
    largest entry; dres within half an ulp of the float64 dz at every element.
    Measured (MI355X): dx 2.1e-7 ... 1.4e-6 of the largest entry (1.0e2 ... 6.1e2) over the 70 cases, the unfused sequence the same figures (bit-equal)."""
    from eeadv import functional as Fn
    gen = torch.Generator().manual_seed(B * 1000 + Cin + Cout + H + pieces)
    y, mask, planted = _mask_tensor((B, Cout, H, H), gen)
    dy = torch.randn(B, Cout, H, H, generator=gen).to(DEV)
    dy2 = torch.randn(B, Cout, H, H, generator=gen).to(DEV) if pieces == 2 else None
    dx_add = torch.randn(B, Cin, H, H, generator=gen).to(DEV) if with_add else None
    w = _w(Cout, Cin, 3, gen)
    g, b, rm, rv = _bn(Cout, gen, affine)
    ub = Fn.wino_sets(w)[1]
    dx64, dz64 = E.conv_bn_bwd64(dy, dy2, mask, w, (rv, g, EPS), (B, Cin, H, H), dx_add)
    dzs, dz_s, _, _ = ops.bn_act_bwd(dy, y, torch.zeros_like(dy), g, None, None, rm, rv, EPS, False, True, True, True, False, dy2)
    sibling = ops.wino3x3(dzs, ub)
    if with_add:
        sibling = sibling + dx_add
    got, dres = ops.wino3x3_bn_eval_bwd(dy, dy2, y, ub, (rv, g, EPS), want_dres, dx_add)
    print("  wino backward B=%d %d->%d H=%d pieces=%d dres=%s add=%s %s" % (B, Cin, Cout, H, pieces, want_dres, with_add, affine))
    _twice_the_sibling(got, sibling, dx64, "dx")
    if want_dres:
        _dres_rule(dres, dz64, planted, "dres")
    else:
        assert dres is None


PAIR_SHAPES = [(1, 32, 32, 4), (2, 32, 64, 8), (3, 32, 32, 16), (5, 64, 128, 16), (9, 256, 512, 4)]


@pytest.mark.parametrize("B,Cin,Cout,H", PAIR_SHAPES, ids=["%dx%d-%dx%d" % s for s in PAIR_SHAPES])
@pytest.mark.parametrize("mt", ["222111", "111222"])
def test_s2_pair_bn_eval_against_float64(ops, B, Cin, Cout, H, mt, monkeypatch):
    """ee_conv3x3s2_pair_bn_eval_fwd_f32 / _bwd_f32 against the float64 pair forms, bn_reference.hard_affine rolled differently for the two
    BatchNorms, both EEADV_S2_MT settings: relu(bn1(conv3x3s2 x)), bn_ds(conv1x1s2 x) and the summed input gradient, each no further than
    twice ee_conv3x3s2_pair_fwd_f32 | ee_bn_act_fwd_f32 resp. ee_bn_act_bwd2_f32 | ee_conv3x3s2_pair_bwd_data_f32 is, + 1e-7 of the largest entry.
    Measured (MI355X): forward 3.9e-8 ... 2.6e-7 of the largest entry (5.3e2 ... 1.7e3), dx 9.7e-8 ... 5.7e-7 of 1.1e2 ... 3.9e2; the unfused sequence the same
    figures (bit-equal)."""
    from eeadv import functional as Fn
    monkeypatch.setenv("EEADV_S2_MT", mt)
    gen = torch.Generator().manual_seed(B + Cin + H)
    x = torch.randn(B, Cin, H, H, generator=gen).to(DEV)
    w3, w1 = _w(Cout, Cin, 3, gen), _w(Cout, Cin, 1, gen)
    g3, b3, rm3, rv3 = _bn(Cout, gen, "hard")
    g1, b1, rm1, rv1 = _bn(Cout, gen, "hard", roll=3)
    w10f, w10b = Fn._dense_weight(w3, "s2p_f", w1), Fn._dense_weight(w3, "s2p_b", w1)
    p3, p1 = E.pair_fwd64(x, w3, w1, (rm3, rv3, g3, b3, EPS), (rm1, rv1, g1, b1, EPS))
    y3, y1 = ops.conv3x3s2_pair_fwd(x, w10f, Cout)
    sib3 = ops.bn_act_fwd(y3, None, g3, b3, rm3, rv3, 0.1, EPS, False, True)[0]
    sib1 = ops.bn_act_fwd(y1, None, g1, b1, rm1, rv1, 0.1, EPS, False, False)[0]
    got3, got1 = ops.conv3x3s2_pair_bn_eval_fwd(x, w10f, Cout, (rm3, rv3, g3, b3, EPS), (rm1, rv1, g1, b1, EPS))
    print("  stride-2 pair B=%d %d->%d H=%d MT=%s" % (B, Cin, Cout, H, mt))
    _forward_rule(got3, sib3, p3, True, "relu(bn1(conv3x3s2))")
    _forward_rule(got1, sib1, p1, False, "bn_ds(conv1x1s2)")
    # backward-data
    OH = H // 2
    out3, mask3, _ = _mask_tensor((B, Cout, OH, OH), gen)
    dy3, dy1 = torch.randn(B, Cout, OH, OH, generator=gen).to(DEV), torch.randn(B, Cout, OH, OH, generator=gen).to(DEV)
    dx64 = E.pair_bwd64(dy3, mask3, dy1, w3, w1, (rv3, g3, EPS), (rv1, g1, EPS), x.shape)
    d3 = ops.bn_act_bwd(dy3, out3, y3, g3, None, None, rm3, rv3, EPS, False, True, True, False, False)[0]
    d1 = ops.bn_act_bwd(dy1, None, y1, g1, None, None, rm1, rv1, EPS, False, False, True, False, False)[0]
    sibling = ops.conv3x3s2_pair_bwd_data(d3, d1, w10b, Cin)
    got = ops.conv3x3s2_pair_bn_eval_bwd(dy3, out3, dy1, w10b, Cin, (rv3, g3, EPS), (rv1, g1, EPS))
    _twice_the_sibling(got, sibling, dx64, "pair dx")


DENSE_SHAPES = [(1, 128, 8), (5, 128, 8), (33, 256, 512), (5, 512, 512), (1, 128, 128), (5, 128, 128)]


@pytest.mark.parametrize("B,Cin,Cout", DENSE_SHAPES, ids=["%dx%d-%d" % s for s in DENSE_SHAPES])
@pytest.mark.parametrize("affine", ["rand", "hard"])
def test_dense2x2_bn_eval_against_float64(ops, B, Cin, Cout, affine):
    """ee_dense2x2_bn_eval_fwd_f32 / _bwd_f32 on 2x2 maps against the float64 restatement: (Cin, Cout) = (128, 8) is the smallest pair
    ops.dense2x2_supported admits; the backward product reduces over 4 Cout and takes Cout a multiple of 128 ((128, 128) is its smallest
    square case): one and two pieces, with and without dx_add, dres checked.  Forward no further than twice ee_dense2x2_f32 | ee_bn_act_fwd_f32
    is, backward than ee_bn_act_bwd2_f32 | ee_dense2x2_f32 on the transposed matrix [+ dx_add], + 1e-7 of the largest entry.
    Measured (MI355X): forward 2.1e-9 ... 6.8e-7 of the largest entry (4.3e2 ... 1.1e3), dx 3.5e-7 ... 1.0e-6 of 78 ... 2.0e2; the unfused sequence the same
    figures (bit-equal)."""
    from eeadv import functional as Fn
    assert ops.dense2x2_supported(128, 8) and not ops.dense2x2_supported(64, 8) and not ops.dense2x2_supported(128, 4)
    gen = torch.Generator().manual_seed(B + Cin + Cout)
    x = torch.randn(B, Cin, 2, 2, generator=gen).to(DEV)
    w = _w(Cout, Cin, 3, gen)
    res = torch.randn(B, Cout, 2, 2, generator=gen).to(DEV)
    g, b, rm, rv = _bn(Cout, gen, affine)
    w2 = Fn._dense_weight(w, "s1")
    print("  dense 2x2 B=%d %d->%d %s" % (B, Cin, Cout, affine))
    c = ops.dense2x2(x, w2)
    for r in (None, res):
        for relu in (True, False):
            pre64 = E.conv_bn_fwd64(x, w, (rm, rv, g, b, EPS), r)
            sibling = ops.bn_act_fwd(c, r, g, b, rm, rv, 0.1, EPS, False, relu)[0]
            got = ops.dense2x2_bn_eval_fwd(x, w2, (rm, rv, g, b, EPS), r, relu)
            _forward_rule(got, sibling, pre64, relu, "forward res=%s relu=%s" % (r is not None, relu))
    if Cout % 128:
        return
    w2t = Fn._dense_weight(w, "s1t")
    y, mask, planted = _mask_tensor((B, Cout, 2, 2), gen)
    dy, dy2 = torch.randn(B, Cout, 2, 2, generator=gen).to(DEV), torch.randn(B, Cout, 2, 2, generator=gen).to(DEV)
    dx_add = torch.randn(B, Cin, 2, 2, generator=gen).to(DEV)
    for pieces, add in ((1, None), (2, dx_add), (1, dx_add), (2, None)):
        d2 = dy2 if pieces == 2 else None
        dx64, dz64 = E.conv_bn_bwd64(dy, d2, mask, w, (rv, g, EPS), x.shape, add)
        dzs = ops.bn_act_bwd(dy, y, torch.zeros_like(dy), g, None, None, rm, rv, EPS, False, True, True, True, False, d2)[0]
        sibling = ops.dense2x2(dzs, w2t)
        if add is not None:
            sibling = sibling + add
        got, dres = ops.dense2x2_bn_eval_bwd(dy, d2, y, w2t, (rv, g, EPS), True, add)
        _twice_the_sibling(got, sibling, dx64, "dx pieces=%d add=%s" % (pieces, add is not None))
        _dres_rule(dres, dz64, planted, "dres")


def _nan_footprint_rule(got, x, w, stride, padding, what):
    """isnan(got) equals the NaN footprint of a direct float64 convolution ON THE HOST (a vendor Winograd spreads a NaN over a whole tile)"""
    want = torch.isnan(F.conv2d(x.double().cpu(), w.double().cpu(), stride=stride, padding=padding))
    n = int(want.sum())
    print("    %-34s %d NaN results expected, %d found" % (what, n, int(torch.isnan(got).sum())))
    assert 0 < n < want.numel() and torch.equal(torch.isnan(got).cpu(), want), what


def test_a_nan_input_has_the_footprint_of_a_direct_convolution(ops):
    """One NaN in x per forward kernel (hard affine: a gamma of 0 does not stop it, (NaN - rm) * 0 is NaN; the ReLU keeps it): the NaN
    pattern of the output is that of a direct float64 convolution on the host - the 3x3 neighbourhood of the input in every result channel of
    that image, nothing else; for the pair the shortcut's 1x1 / stride 2 output has it at the one pixel that reads the input.
    Measured (MI355X): 288 NaN results on each of the 4x4, 8x8 and 16x16 maps (9 positions x 32 channels), 128 / 64 and 64 for the pair, 256 for
    the dense product - the expected sets."""
    from eeadv import functional as Fn
    gen = torch.Generator().manual_seed(5)
    # Winograd, 8x8: the NaN on the seam of two 2x2 output tiles in both directions
    B, C, H = 3, 32, 8
    x = torch.randn(B, C, H, H, generator=gen).to(DEV)
    x[1, 7, 3, 4] = float("nan")
    w = _w(C, C, 3, gen)
    g, b, rm, rv = _bn(C, gen, "hard")
    res = torch.randn(B, C, H, H, generator=gen).to(DEV)
    _nan_footprint_rule(ops.wino3x3_bn_eval_fwd(x, Fn.wino_sets(w)[0], (rm, rv, g, b, EPS), res, True), x, w, 1, 1, "wino3x3_bn_eval_fwd 8x8")
    for H2 in (4, 16):
        x2 = torch.randn(B, C, H2, H2, generator=gen).to(DEV)
        x2[2, 31, 2, 1] = float("nan")
        _nan_footprint_rule(ops.wino3x3_bn_eval_fwd(x2, Fn.wino_sets(w)[0], (rm, rv, g, b, EPS), None, True), x2, w, 1, 1, "wino3x3_bn_eval_fwd %dx%d" % (H2, H2))
    # the stride-2 pair: an even position, read by the 1x1 / stride 2 shortcut as well
    Cout = 64
    w3, w1 = _w(Cout, C, 3, gen), _w(Cout, C, 1, gen)
    g3, b3, rm3, rv3 = _bn(Cout, gen, "hard")
    g1, b1, rm1, rv1 = _bn(Cout, gen, "hard", roll=3)
    got3, got1 = ops.conv3x3s2_pair_bn_eval_fwd(x, Fn._dense_weight(w3, "s2p_f", w1), Cout, (rm3, rv3, g3, b3, EPS), (rm1, rv1, g1, b1, EPS))
    x_even = x.clone()
    x_even[1, 7, 3, 4] = 0.0
    x_even[1, 7, 2, 4] = float("nan")
    e3, e1 = ops.conv3x3s2_pair_bn_eval_fwd(x_even, Fn._dense_weight(w3, "s2p_f", w1), Cout, (rm3, rv3, g3, b3, EPS), (rm1, rv1, g1, b1, EPS))
    _nan_footprint_rule(got3, x, w3, 2, 1, "pair 3x3, odd row")
    assert not bool(torch.isnan(got1).any())  # the shortcut reads even positions only
    _nan_footprint_rule(e3, x_even, w3, 2, 1, "pair 3x3, even position")
    _nan_footprint_rule(e1, x_even, w1, 2, 0, "pair 1x1, even position")
    # the dense product on a 2x2 map: every output of that image, no other image of the 32-row tile
    Bd, Cd, Cod = 5, 128, 64
    xd = torch.randn(Bd, Cd, 2, 2, generator=gen).to(DEV)
    xd[3, 100, 1, 0] = float("nan")
    wd = _w(Cod, Cd, 3, gen)
    gd, bd, rmd, rvd = _bn(Cod, gen, "hard")
    _nan_footprint_rule(ops.dense2x2_bn_eval_fwd(xd, Fn._dense_weight(wd, "s1"), (rmd, rvd, gd, bd, EPS), None, True), xd, wd, 1, 1, "dense2x2_bn_eval_fwd")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. the two block Functions: how functional.py puts the kernels together
# ---------------------------------------------------------------------------------------------------------------------------------------
def _conv(ops, Fn, x, w, back):
    """a 3x3 / stride 1 convolution (back: its backward-data) on the unfused kernels: ee_dense2x2_f32 on 2x2 maps, ee_wino3x3_f32 otherwise"""
    if x.shape[2] == 2:
        return ops.dense2x2(x, Fn._dense_weight(w, "s1t" if back else "s1"))
    return ops.wino3x3(x, Fn.wino_sets(w)[1 if back else 0])


def _block_inputs(B, Cin, Cout, H, OH, gen):
    x = torch.relu(torch.randn(B, Cin, H, H, generator=gen)).to(DEV)
    dy, dy2 = torch.randn(B, Cout, OH, OH, generator=gen).to(DEV), torch.randn(B, Cout, OH, OH, generator=gen).to(DEV)
    return x, dy, dy2


BASIC_CASES = [(3, 32, 16, False), (2, 64, 8, False), (5, 32, 4, False), (5, 128, 2, False), (5, 128, 2, True)]  # (B, C, H, _DENSE_FOLD_BWD: 2x2 maps only)


@pytest.mark.parametrize("B,C,H,fold", BASIC_CASES, ids=["%dx%dx%d%s" % (s[:3] + ("-fold" if s[3] else "",)) for s in BASIC_CASES])
def test_eval_basic_block_against_float64(ops, monkeypatch, B, C, H, fold):
    """functional.EvalBasicBlockFn with a forked output and a gradient on each piece, bn_reference.hard_affine (gamma of both signs: a scale of
    |gamma| in the backward shows here) rolled differently for bn1 and bn2, running statistics as test_gpu_evalfuse._bn draws them (two BatchNorms with a variance of 1e-6 in a row
    would scale dx by 1e5 and bury the residual's share), against the float64 restatement on the masks of its own two
    outputs: out2 and the input gradient - conv1^T of bn1's backward PLUS the residual's dz - no further than twice the unfused kernel
    sequence is, + 1e-7 of the largest entry.  On 2x2 maps (layer 4) the default backward is ee_bn_act_bwd2_f32 and a BLAS product; fold: ee_dense2x2_bn_eval_bwd_f32.
    Measured (MI355X): out2 1.6e-7 ... 2.8e-7 of the largest entry (4.4 ... 14), dx 1.3e-7 ... 2.8e-7 of 5.5 ... 9.6; bit-equal to the unfused sequence but for
    the default backward on 2x2 maps (the BLAS product sums in another order): 1.10 times the unfused sequence's distance."""
    from eeadv import functional as Fn
    monkeypatch.setattr(Fn, "_DENSE_FOLD_BWD", fold)
    gen = torch.Generator().manual_seed(B + C + H)
    x, dy, dy2 = _block_inputs(B, C, C, H, H, gen)
    w1, w2 = _w(C, C, 3, gen), _w(C, C, 3, gen)
    g1, b1, rm1, rv1 = _bn(C, gen, "hard", edge=False)
    g2, b2, rm2, rv2 = _bn(C, gen, "hard", roll=2, edge=False)
    xg = x.clone().requires_grad_(True)
    with torch.enable_grad():
        oa, ob = Fn.EvalBasicBlockFn.apply(xg, xg, w1, w2, g1, b1, rm1, rv1, EPS, g2, b2, rm2, rv2, EPS, True)
    (got_dx,) = torch.autograd.grad([oa, ob], xg, [dy, dy2])
    assert oa.data_ptr() == ob.data_ptr()
    out1 = Fn._eval_conv_fwd(x, w1, (rm1, rv1, g1, b1, EPS), None)  # (the same launch again: the same bits)
    # float64 on the masks of out1 and out2
    a1 = E.gate(E.conv_bn_fwd64(x, w1, (rm1, rv1, g1, b1, EPS)), out1)
    pre2 = E.conv_bn_fwd64(a1, w2, (rm2, rv2, g2, b2, EPS), x)
    d1_64, dres64 = E.conv_bn_bwd64(dy, dy2, oa.detach(), w2, (rv2, g2, EPS), x.shape)
    dx64, _ = E.conv_bn_bwd64(d1_64, None, out1, w1, (rv1, g1, EPS), x.shape, dres64)
    # the unfused kernel sequence
    c1 = _conv(ops, Fn, x, w1, False)
    s1 = ops.bn_act_fwd(c1, None, g1, b1, rm1, rv1, 0.1, EPS, False, True)[0]
    c2 = _conv(ops, Fn, s1, w2, False)
    s2 = ops.bn_act_fwd(c2, x, g2, b2, rm2, rv2, 0.1, EPS, False, True)[0]
    dzs2, dz2, _, _ = ops.bn_act_bwd(dy, s2, c2, g2, None, None, rm2, rv2, EPS, False, True, True, True, False, dy2)
    dzs1 = ops.bn_act_bwd(_conv(ops, Fn, dzs2, w2, True), s1, c1, g1, None, None, rm1, rv1, EPS, False, True, True, False, False)[0]
    sib_dx = _conv(ops, Fn, dzs1, w1, True) + dz2
    print("  basic block B=%d C=%d H=%d fold=%s" % (B, C, H, fold))
    assert float(dres64.abs().max()) > 0.1 * float(dx64.abs().max())  # the residual's share of dx is no rounding matter
    _forward_rule(oa.detach(), s2, pre2, True, "out2")
    _twice_the_sibling(got_dx, sib_dx, dx64, "dx")


DOWN_SHAPES = [(3, 32, 32, 16), (2, 32, 64, 8), (5, 64, 128, 8), (5, 128, 128, 4)]


@pytest.mark.parametrize("B,Cin,Cout,H", DOWN_SHAPES, ids=["%dx%d-%dx%d" % s for s in DOWN_SHAPES])
def test_eval_down_block_against_float64(ops, monkeypatch, B, Cin, Cout, H):
    """functional.EvalDownBlockFn (forked output, a gradient on each piece; hard_affine rolled differently for bn1, the shortcut's BatchNorm
    and bn2, so that one BatchNorm's constants in another's place show) against the float64 restatement on the masks of its own outputs:
    out2 and the input gradient no further than twice the unfused kernel sequence is, + 1e-7 of the largest entry.  H = 4: conv2 on a 2x2 map.
    Measured (MI355X): out2 1.5e-7 ... 3.5e-7 of the largest entry (7.8 ... 9.5), dx 1.3e-7 ... 2.0e-7 of 6.2 ... 9.8; bit-equal to the unfused sequence."""
    from eeadv import functional as Fn
    monkeypatch.setattr(Fn, "_DENSE_FOLD_BWD", False)
    gen = torch.Generator().manual_seed(B + Cin + Cout + H)
    OH = H // 2
    x, dy, dy2 = _block_inputs(B, Cin, Cout, H, OH, gen)
    w3, wd, w2 = _w(Cout, Cin, 3, gen), _w(Cout, Cin, 1, gen), _w(Cout, Cout, 3, gen)
    g1, b1, rm1, rv1 = _bn(Cout, gen, "hard", edge=False)
    gd, bd, rmd, rvd = _bn(Cout, gen, "hard", roll=3, edge=False)
    g2, b2, rm2, rv2 = _bn(Cout, gen, "hard", roll=2, edge=False)
    xg = x.clone().requires_grad_(True)
    with torch.enable_grad():
        oa, ob = Fn.EvalDownBlockFn.apply(xg, xg, w3, wd, w2, g1, b1, rm1, rv1, EPS, gd, bd, rmd, rvd, EPS, g2, b2, rm2, rv2, EPS, True)
    (got_dx,) = torch.autograd.grad([oa, ob], xg, [dy, dy2])
    w10f, w10b = Fn._dense_weight(w3, "s2p_f", wd), Fn._dense_weight(w3, "s2p_b", wd)
    out1 = ops.conv3x3s2_pair_bn_eval_fwd(x, w10f, Cout, (rm1, rv1, g1, b1, EPS), (rmd, rvd, gd, bd, EPS))[0]
    # float64 on the masks of out1 and out2
    p3, p1 = E.pair_fwd64(x, w3, wd, (rm1, rv1, g1, b1, EPS), (rmd, rvd, gd, bd, EPS))
    a1 = E.gate(p3, out1)
    pre2 = E.conv_bn_fwd64(a1, w2, (rm2, rv2, g2, b2, EPS), p1)
    d1_64, dsc64 = E.conv_bn_bwd64(dy, dy2, oa.detach(), w2, (rv2, g2, EPS), a1.shape)
    dx64 = E.pair_bwd64(d1_64, out1, dsc64, w3, wd, (rv1, g1, EPS), (rvd, gd, EPS), x.shape)
    # the unfused kernel sequence
    y3, y1 = ops.conv3x3s2_pair_fwd(x, w10f, Cout)
    s1 = ops.bn_act_fwd(y3, None, g1, b1, rm1, rv1, 0.1, EPS, False, True)[0]
    sc = ops.bn_act_fwd(y1, None, gd, bd, rmd, rvd, 0.1, EPS, False, False)[0]
    c2 = _conv(ops, Fn, s1, w2, False)
    s2 = ops.bn_act_fwd(c2, sc, g2, b2, rm2, rv2, 0.1, EPS, False, True)[0]
    dzs2, dz2, _, _ = ops.bn_act_bwd(dy, s2, c2, g2, None, None, rm2, rv2, EPS, False, True, True, True, False, dy2)
    d3 = ops.bn_act_bwd(_conv(ops, Fn, dzs2, w2, True), s1, y3, g1, None, None, rm1, rv1, EPS, False, True, True, False, False)[0]
    dd = ops.bn_act_bwd(dz2, None, y1, gd, None, None, rmd, rvd, EPS, False, False, True, False, False)[0]
    sib_dx = ops.conv3x3s2_pair_bwd_data(d3, dd, w10b, Cin)
    print("  down block B=%d %d->%d H=%d" % (B, Cin, Cout, H))
    _forward_rule(oa.detach(), s2, pre2, True, "out2")
    _twice_the_sibling(got_dx, sib_dx, dx64, "dx")
