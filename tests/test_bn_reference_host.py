"""tests/bn_reference.py itself, on the CPU: the float64 bar against torch's float64 batch_norm and its autograd, the exactness claims of
the hard input, and the tie cap of every seeded case of tests/test_gpu_bn_hard_channels.py."""
import pytest
import torch
import torch.nn.functional as F

import bn_reference as R


def _rel(a, b):
    """the largest error of any channel in units of that channel's own allowance: F64_TOL of its own largest entry plus F64_ABS"""
    a, b = a.detach().double(), b.detach().double()
    err, scale = (a - b).abs(), b.abs()
    if a.dim() == 4:
        err, scale = err.amax((0, 2, 3)), scale.amax((0, 2, 3))
    return float((err / (scale + F64_ABS / F64_TOL)).max())


# float64 unit roundoff 1.1e-16, amplified by the conditioning of the hard channels (|mean| / std = 128 on `offset`, 1 / sqrt(eps) = 316 on
# `const`) and by sums of up to 3e4 terms accumulated in any order: 1.1e-16 * 316 * 3e4 = 1e-9, relative to the channel's own largest entry
F64_TOL = 1e-9
# a channel whose true value is 0 by cancellation (dx and dgamma on `const`) keeps the rounding of the cancelled terms, which are up to
# |gamma| / sqrt(eps) * |dy| = 1.25 * 316 * 0.5 = 200 each: 1.1e-16 * 200 * sqrt(3e4 terms) = 4e-12, taken as an absolute allowance per channel
F64_ABS = 4e-12


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("relu,res,res_in", [(True, False, False), (True, True, False), (False, True, False), (True, False, True)])
@pytest.mark.parametrize("shape,seed", [((12, 6, 16, 16), 12), ((3, 6, 5, 7), 16), ((9, 11, 4, 8), 21)])
def test_bn_ref64_is_float64_batch_norm_and_its_autograd(shape, seed, relu, res, res_in, training):
    c = R.hard_case(shape, seed)
    x, s_res = (R.split_sum(c["x"], seed) if res_in else (c["x"], None))
    residual = c["residual"] if res else None
    mask = None
    if relu:  # any fixed branch will do here: both sides are given the same one
        mask = torch.rand(shape, generator=torch.Generator().manual_seed(seed)) > 0.4
    got = R.bn_ref64(x, c["gamma"], c["beta"], c["rm"], c["rv"], 0.1, 1e-5, training, res_in=s_res, residual=residual, relu=relu,
                     dy=c["dy"], mask=mask)
    leaves = [t.double().requires_grad_(True) for t in (x, c["gamma"], c["beta"])]
    r64 = None if residual is None else residual.double().requires_grad_(True)
    rm, rv = c["rm"].double().clone(), c["rv"].double().clone()
    s = leaves[0] if s_res is None else leaves[0] + s_res.double()
    pre = F.batch_norm(s, rm, rv, leaves[1], leaves[2], training, float(R.np.float32(0.1)), R.eps32(1e-5))
    if r64 is not None:
        pre = pre + r64
    want_y = torch.relu(pre) if relu else pre
    routed = pre * mask.double() if relu else pre
    grads = torch.autograd.grad(routed, leaves + ([r64] if r64 is not None else []), c["dy"].double())
    assert _rel(got["y"], want_y) <= F64_TOL
    assert _rel(got["running_mean"], rm) <= F64_TOL and _rel(got["running_var"], rv) <= F64_TOL
    for name, g in zip(["dx", "dgamma", "dbeta", "dresidual"], grads):
        assert _rel(got[name], g) <= F64_TOL, name
    if training:
        s64 = s.detach()
        assert _rel(got["mean"], s64.mean((0, 2, 3))) <= F64_TOL and _rel(got["var"], s64.var((0, 2, 3), unbiased=False)) <= F64_TOL
        assert _rel(got["invstd"], 1.0 / torch.sqrt(s64.var((0, 2, 3), unbiased=False) + R.eps32(1e-5))) <= F64_TOL


def _all_bn_inputs():
    """(name, BatchNorm input, gamma) of every seeded GPU case, the convolution producers' raw outputs recomputed here in float64"""
    for name, (shape, seed) in R.BN_ACT_CASES.items():
        yield "bn_act " + name, R.hard_case(shape, seed)
    shape, seed = R.BN_DUAL_CASE
    yield "bn_dual a", R.hard_case(shape, seed)
    yield "bn_dual b", R.hard_case(shape, seed + 1, roll=2)
    for name, (shape, seed) in R.BN_SUM_CASES.items():
        yield "bn_sum_act " + name, R.hard_case(shape, seed)
    for name, (shape, seed) in R.BN_POOL_CASES.items():
        yield "bn_relu_pool " + name, R.hard_case(shape, seed)


def _conv_cases():
    xs, K, seed = R.STEM_CASE
    x, w = R.shaped_conv_operands(xs, (K, 3, 7, 7), seed, 147)
    yield "stem", F.conv2d(x.double(), w.double(), None, 2, 3), K
    for H, seed in R.WINO_CASES.items():
        x, w = R.shaped_conv_operands((3, 32, H, H), (32, 32, 3, 3), seed, 9 * 32)
        yield "wino H=%d" % H, F.conv2d(x.double(), w.double(), None, 1, 1), 32
    for H, seed in R.PAIR_CASES.items():
        x, w = R.shaped_conv_operands((3, 32, H, H), (64, 32, 3, 3), seed, 9 * 32)
        yield "pair H=%d" % H, F.conv2d(x.double(), w.double(), None, 2, 1), 64


def test_hard_input_claims_hold_exactly_in_float64():
    for name, c in _all_bn_inputs():
        x = c["x"]
        assert x.dtype == torch.float32 and bool(torch.isfinite(x).all())
        r = R.bn_ref64(x, c["gamma"], c["beta"], c["rm"], c["rv"], 0.1, 1e-5, True, relu=True)
        const = [i for i, k in enumerate(c["kinds"]) if k == "const"]
        assert const, name
        assert bool((r["mean"][const] == R.CONST).all()) and bool((r["var"][const] == 0).all()), name
        assert bool((r["invstd"][const] == 1.0 / R.eps32(1e-5) ** 0.5).all()), name
        # fp32 partial sums of the constant are exact: in any order, any grouping
        n = x[:, const[0]].numel()
        assert float(x[:, const[0]].sum(dtype=torch.float32)) == R.CONST * n and n < 2 ** 22
        off = [i for i, k in enumerate(c["kinds"]) if k == "offset"][0]
        assert 100 < float(r["mean"][off].abs() * r["invstd"][off]) < 160, name
        out = [i for i, k in enumerate(c["kinds"]) if k == "outlier"][0]
        xo = x[:, out].double()
        cross = float(((xo.mean((1, 2)) - xo.mean()) ** 2).mean() / xo.var(unbiased=False))
        assert cross > 0.5, (name, cross)  # the spread of the per-image means carries most of the variance
        tail = [i for i, k in enumerate(c["kinds"]) if k == "tail"][0]
        assert bool((x[-1, tail] == -3.0).all())
    g, b = R.hard_affine(6)
    assert sorted(g.tolist()) == sorted(R.GAMMA_CYCLE) and {(0.0, 0.4), (0.0, -0.4)} <= {(float(a), round(float(c), 6)) for a, c in zip(g, b)}
    assert float(g[0]) < 0 and R.kinds(6)[0] == "const"


def test_sum_split_is_exact_on_constant_channels():
    for name, (shape, seed) in R.BN_SUM_CASES.items():
        c = R.hard_case(shape, seed)
        x, res = R.split_sum(c["x"], seed)
        const = [i for i, k in enumerate(c["kinds"]) if k == "const"]
        assert bool(((x + res)[:, const] == R.CONST).all()), name


def test_every_seeded_case_keeps_its_ties_under_the_cap():
    """outside the band the GPU tests demand the fp32 ReLU mask equal to the float64 one exactly; inside it they allow a difference - so
    the band may hold only a negligible share of any case.  A condition on the seeds, not a tolerance."""
    worst = {}
    for name, c in _all_bn_inputs():
        roll = 2 if name.endswith(" b") else 0
        for training in (True, False):
            for res in (False, True):
                r = R.bn_ref64(c["x"], c["gamma"], c["beta"], c["rm"], c["rv"], 0.1, 1e-5, training,
                               residual=c["residual"] if res else None, relu=True)
                worst[(name, training, res, roll)] = R.tie_share(r["pre"], c["gamma"])
    shape, seed = R.BN_DUAL_CASE  # the composite relu(bn_a(xa) + bn_b(xb)): every channel is live, side b rides through gamma_a == 0
    a, b = R.hard_case(shape, seed), R.hard_case(shape, seed + 1, roll=2)
    for training in (True, False):
        rb = R.bn_ref64(b["x"], b["gamma"], b["beta"], b["rm"], b["rv"], 0.1, 1e-5, training, relu=False)
        ra = R.bn_ref64(a["x"], a["gamma"], a["beta"], a["rm"], a["rv"], 0.1, 1e-5, training, residual=rb["y"], relu=True)
        worst[("bn_dual", training, True, 0)] = R.tie_share(ra["pre"], torch.ones(shape[1]))
    for name, raw, C in _conv_cases():
        gamma, beta = R.hard_affine(C)
        r = R.bn_ref64(raw, gamma, beta, None, None, 0.1, 1e-5, True, relu=True)
        worst[(name, True, False, 0)] = R.tie_share(r["pre"], gamma)
    for name, (shape, seed) in R.SYNC_CASES.items():  # train mode only: eval mode issues no exchange
        c = R.hard_case(shape, seed)
        const = [i for i, k in enumerate(c["kinds"]) if k == "const"]
        for res in (False, True):
            r = R.bn_ref64(c["x"], c["gamma"], c["beta"], c["rm"], c["rv"], 0.1, 1e-5, True, residual=c["residual"] if res else None, relu=True)
            if name in R.SYNC_TIES_LEAVE_OUT_CONST:  # see the note next to SYNC_CASES: exact zeros on both sides, not ties
                dropped = r["pre"][:, const]
                assert bool((dropped[dropped.abs() <= R.TIE_BAND] == 0).all())
                assert R.tie_share(r["pre"], c["gamma"], leave_out=const) == 0.0, (name, res)
                worst[("syncbn " + name, True, res, 0)] = 0.0
            else:
                worst[("syncbn " + name, True, res, 0)] = R.tie_share(r["pre"], c["gamma"])
    bad = {k: v for k, v in worst.items() if not v < R.TIE_CAP}
    assert not bad, bad


# ---- SyncBatchNorm over simulated ranks: the reference plumbing of the GPU test, and the host restatement of the kernels' merge -----------
SYNC_DEALS = [(name, label) for name in R.SYNC_CASES for label in R.SYNC_DEALS[name]]


def test_every_sync_case_has_its_deals_and_they_are_partitions():
    assert set(R.SYNC_DEALS) == set(R.SYNC_CASES)
    for name, label in SYNC_DEALS:
        B, parts = R.SYNC_CASES[name][0][0], R.SYNC_DEALS[name][label]
        assert sorted(i for idx in parts for i in idx) == list(range(B)) and all(idx for idx in parts), (name, label)
        whole = torch.arange(B * 3.0).view(B, 3)
        assert torch.equal(R.gather_back([whole[idx] for idx in parts], parts), whole), (name, label)
    assert R.deal(8, stride=2) == [[0, 2, 4, 6], [1, 3, 5, 7]] and R.deal(8, [4, 3, 1]) == [[0, 1, 2, 3], [4, 5, 6], [7]]
    # the slice counts the labels promise: ee_bn.hip's split_slices, one slice up to 2048 quads per channel
    slices = lambda name, label: [max(1, -(-(len(idx) * R.SYNC_CASES[name][0][2] * R.SYNC_CASES[name][0][3] // 4) // 2048)) for idx in R.SYNC_DEALS[name][label]]
    assert slices("two-slices", "[4,3] S=2,2") == [2, 2] and slices("two-slices", "[5,2] S=2,1") == [2, 1]
    assert slices("four-slices", "[9,3] S=4,2") == [4, 2] and (9 * 56 * 56 // 4) % 4 == 0 and (9 * 56 * 56 // 4 // 4) % (56 * 56 // 4) != 0
    assert all(s == 1 for name in ("one-slice", "hw4", "channels-70") for label in R.SYNC_DEALS[name] for s in slices(name, label))


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("name,label", SYNC_DEALS)
def test_per_rank_parameter_gradients_add_up_to_the_whole_batch(name, label, res):
    shape, seed = R.SYNC_CASES[name]
    c, parts = R.hard_case(shape, seed), R.SYNC_DEALS[name][label]
    residual = c["residual"] if res else None
    fwd = R.bn_ref64(c["x"], c["gamma"], c["beta"], c["rm"], c["rv"], 0.1, 1e-5, True, residual=residual, relu=True)
    mask = fwd["y"] > 0
    ref = R.bn_ref64(c["x"], c["gamma"], c["beta"], c["rm"], c["rv"], 0.1, 1e-5, True, residual=residual, relu=True, dy=c["dy"], mask=mask)
    dg, db = R.rank_param_grads64(c["x"], ref["mean"], ref["invstd"], c["dy"], mask, parts)
    assert dg.shape == db.shape == (len(parts), shape[1])
    for total, want in ((dg.sum(0), ref["dgamma"]), (db.sum(0), ref["dbeta"])):
        assert bool(((total - want).abs() <= 1e-12 * want.abs()).all()), (total - want).abs().max()
    # the two-addend form of the incoming gradient
    hi, lo = R.exact_addends(c["dy"])
    dg2, db2 = R.rank_param_grads64(c["x"], ref["mean"], ref["invstd"], hi, mask, parts, dy2=lo)
    assert torch.equal(dg2, dg) and torch.equal(db2, db)
    # a rank's images put back where they came from
    assert torch.equal(R.gather_back([c["x"][idx].contiguous() for idx in parts], parts), c["x"])
