"""GPU: the convolution kernels (ee_wino.hip, ee_s2.hip, ee_conv.hip, ee_dense.hip, ee_wrw.hip, ee_wprep.hip) against tests/conv_reference.py.

(a) integer cases: every partial sum in any order is a float32 number (exactness_margin < 2^24, asserted), so the kernel returns float64's result
    BIT FOR BIT; a mismatch is a dropped, duplicated or misplaced term, and the message says where;
(b) impulse sweeps (part of (a)): one 1 per image, image b at pixel b - every pixel of every tile, seams and corners;
(c) ReLU-like cases: |got - ref64| <= k * 2^-24 * abs_sum element by element, k counted from the arithmetic (conv_reference.roundings); the same
    rule is asserted for ATen's float32 result of the same inputs, as a check of the rule;
(d) NaN / inf footprints of the unfused kernels;
guard bands: the C ABI called directly with the wrappers' arguments, result and workspace carved from a buffer filled with one NaN bit pattern.

Measured on MI355X (largest |got - ref64| / (2^-24 abs_sum) per family, against the derived k): see DESIGN.md section 4,
"The convolution kernels against float64, bit for bit".
"""

import pytest
import torch
import torch.nn.functional as F

import conv_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S2_KINDS = ("s2_fwd", "s2_bwd", "pair_fwd", "pair_bwd")
MTS = ("222222", "111111")  # EEADV_S2_MT: 32 / 16 result channels per workgroup, the two settings test_gpu_kernels.py uses
GROUP = {4: 4, 8: 2, 16: 1}  # images per workgroup of ee_wino3x3_f32 (ee_wino.hip: wino3x3_map4_kernel, PcGeo<8>, PcGeo<16>)


@pytest.fixture(scope="module")
def ops():
    from eeadv import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def EF():
    from eeadv import functional as _EF
    return _EF


def _id(c):
    return "%s-%s%s" % (c[0], "x".join(str(v) for v in c[1]), "".join("-%s%d" % (k[0], v) for k, v in c[2]))


def _with_mt(cases):
    out = []
    for c in cases:
        for mt in (MTS if c[0] in S2_KINDS else (None,)):
            out.append(pytest.param(c, mt, id=_id(c) + ("-mt" + mt[0] if mt else "")))
    return out


def _poison(*shapes):
    """fill and free blocks of the sizes the wrapper is about to allocate - two of each, for the kernels with two results of one size: torch.empty
    then hands back NaNs, not an earlier call's right answer"""
    held = [torch.full(tuple(s), float("nan"), device=DEV) for s in shapes for _ in range(2) if all(v > 0 for v in s)]
    del held


def _workspace_floats(kind, case):
    from eeadv import _native as N
    B, Cin, Cout, H, W = case["shape"]
    if kind == "wrw3x3":
        return int(N.lib.ee_wrw3x3_workspace_floats(B, Cin, Cout, H))
    if kind == "wrw3x3s2":
        return int(N.lib.ee_wrw3x3s2_workspace_floats(B, Cin, Cout, H, 1 if "dy1" in case else 0))
    if kind == "wrw_stem":
        return int(N.lib.ee_wrw_stem7x7s2_workspace_floats(B, H, W))
    if kind == "wrw1x1":
        return int(N.lib.ee_wrw1x1_workspace_floats(B, Cin, Cout, H * W))
    if kind == "stem_fwd":
        return int(N.lib.ee_stem7x7s2_fwd_stats_floats(B, Cout, H, W))
    return 0


def _param(t):
    return torch.nn.Parameter(t.to(DEV))


def _wino_u(ops, EF, w, back):
    """the transformed filter set through the weight-prep cache (wino_sets) where the model's channel counts allow it, else one ee_wprep.hip launch"""
    if w.shape[0] % 32 == 0 and w.shape[1] % 32 == 0:
        return EF.wino_sets(w)[1 if back else 0]
    kind = "wino_b" if back else "wino_f"
    u = torch.full(EF._rearranged_shape(w, kind), float("nan"), device=DEV)
    ops.conv_weight_prep(EF._NATIVE_KIND[kind], w.detach(), None, u)
    return u


def run_kernel(ops, EF, kind, case):
    """the case through eeadv.ops and the weight-prep cache -> tuple of float32 device tensors (like conv_reference.ref64)"""
    B, Cin, Cout, H, W = case["shape"]
    t = {n: v.to(DEV) for n, v in case.items() if torch.is_tensor(v)}
    w = _param(case["w"]) if "w" in case else None
    w1 = _param(case["w1"]) if "w1" in case else None
    OH, OW = R.out_hw(kind, H, W)
    _poison((B, Cout, OH, OW), (B, Cin, H, W), (Cout, Cin) + (R.geometry(kind)[0],) * 2, (10 * Cout * Cin,), (9 * Cout * Cin,),
            (max(_workspace_floats(kind, case), 4),))
    if kind in ("wino_fwd", "wino_bwd"):
        back = kind == "wino_bwd"
        a = t["dy"] if back else t["x"]
        if H == 2:
            return (ops.dense2x2(a, EF._dense_weight(w, "s1t" if back else "s1")),)
        return (ops.wino3x3(a, _wino_u(ops, EF, w, back)),)
    if kind == "s2_fwd":
        return (ops.conv3x3s2_small_fwd(t["x"], EF._dense_weight(w, "s2m_f"), Cout),)
    if kind == "s2_bwd":
        return (ops.conv3x3s2_small_bwd_data(t["dy"], EF._dense_weight(w, "s2m_b"), Cin),)
    if kind == "pair_fwd":
        return ops.conv3x3s2_pair_fwd(t["x"], EF._dense_weight(w, "s2p_f", w1), Cout)
    if kind == "pair_bwd":
        return (ops.conv3x3s2_pair_bwd_data(t["dy"], t["dy1"], EF._dense_weight(w, "s2p_b", w1), Cin),)
    if kind == "c1s2_fwd":
        return (ops.conv1x1s2_fwd(t["x"], w.detach()),)
    if kind == "c1s2_bwd":
        return (ops.conv1x1s2_bwd(t["dy"], w.detach(), H, W),)
    if kind == "stem_fwd":
        y = ops.stem7x7s2_fwd(t["x"], w.detach())
        y2, _ = ops.stem7x7s2_fwd(t["x"], w.detach(), True)  # the same kernel with the BatchNorm partials: the y output only
        assert torch.equal(y.view(torch.int32), y2.view(torch.int32)), "stem forward: y differs with want_stats"
        return (y,)
    if kind == "stem_bwd":
        return (ops.stem7x7s2_bwd_data(t["dy"], w.detach(), H, W),)
    if kind == "wrw3x3":
        assert ops.wrw3x3_supported(t["x"], t["dy"])
        return (ops.wrw3x3(t["x"], t["dy"]),)
    if kind == "wrw3x3s2":
        assert ops.wrw3x3s2_supported(t["x"], t["dy"], t.get("dy1"))
        dw3, dw1 = ops.wrw3x3s2(t["x"], t["dy"], t.get("dy1"))
        return (dw3,) if dw1 is None else (dw3, dw1)
    if kind == "wrw_stem":
        assert ops.wrw_stem7x7s2_supported(t["x"], t["dy"])
        return (ops.wrw_stem7x7s2(t["x"], t["dy"]),)
    assert kind == "wrw1x1" and ops.wrw1x1_supported(t["x"], t["dy"])
    return (ops.wrw1x1(t["x"], t["dy"]),)


def aten_f32(kind, case):
    """ATen's float32 result of the same inputs on the device"""
    dev = {n: (v.to(DEV) if torch.is_tensor(v) else v) for n, v in case.items()}
    if kind not in R.WRW:
        return _aten_direct(kind, dev)
    k, st, p = R.geometry(kind)
    B, Cin, Cout, H, W = case["shape"]

    def wrw(dy, k, p):
        return torch.ops.aten.convolution_backward(dy, dev["x"], torch.zeros(Cout, Cin, k, k, device=DEV), None, [st, st], [p, p], [1, 1], False, [0, 0], 1,
                                                   [False, True, False])[1]
    return (wrw(dev["dy"], k, p),) + ((wrw(dev["dy1"], 1, 0),) if "dy1" in dev else ())


def _aten_direct(kind, t):
    k, s, p = R.geometry(kind)
    B, Cin, Cout, H, W = t["shape"]
    if kind in R.FWD:
        y = F.conv2d(t["x"], t["w"], None, s, p)
        return (y, F.conv2d(t["x"], t["w1"], None, 2, 0)) if kind == "pair_fwd" else (y,)
    zx = torch.zeros(B, Cin, H, W, device=DEV)
    dx = torch.ops.aten.convolution_backward(t["dy"], zx, t["w"], None, [s, s], [p, p], [1, 1], False, [0, 0], 1, [True, False, False])[0]
    if kind == "pair_bwd":
        dx = dx + torch.ops.aten.convolution_backward(t["dy1"], zx, t["w1"], None, [2, 2], [0, 0], [1, 1], False, [0, 0], 1, [True, False, False])[0]
    return (dx,)


def assert_exact(kind, case, got, ref):
    for part, (g, r) in enumerate(zip(got, ref)):
        g = g.detach().double().cpu()
        assert g.shape == r.shape, (kind, part, g.shape, r.shape)
        if not R.same_values(g, r):
            pytest.fail(R.describe_mismatch(kind, case, g, r, part, GROUP.get(case["shape"][3], 1)), pytrace=False)


# ---- (a), (b): integer cases and impulse sweeps ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,mt", _with_mt(R.gpu_integer_cases()))
def test_integer_case_equals_float64_bit_for_bit(ops, EF, monkeypatch, c, mt):
    kind, shape, opts = c
    case = R.make_integer(kind, shape, opts)
    assert R.exactness_margin(kind, case) < 2 ** 24
    if mt:
        monkeypatch.setenv("EEADV_S2_MT", mt)
    ref = R.ref64(kind, case)
    got = run_kernel(ops, EF, kind, case)
    assert len(got) == len(ref)
    assert_exact(kind, case, got, ref)


@pytest.mark.parametrize("co,ci", [(64, 32), (32, 96)])
def test_winograd_filter_sets_equal_float64_on_integer_filters(ops, EF, co, ci):
    """ee_conv_weight_prep_f32, kinds wino_f, wino_b, wino_fb, and the cache (wino_sets): G g G^T of integer filters is halves and quarters - exact"""
    w = R.integer_case("wino_fwd", (1, ci, co, 4, 4), co + ci)["w"].to(DEV)
    uf, ub = R.wino_filter_sets(w.cpu())
    for kind, want in (("wino_f", uf), ("wino_b", ub), ("wino_fb", torch.stack([uf.reshape(-1), ub.reshape(-1)]))):
        got = torch.full(EF._rearranged_shape(w, kind), float("nan"), device=DEV)
        ops.conv_weight_prep(EF._NATIVE_KIND[kind], w, None, got)
        assert R.same_values(got.double().cpu(), want), kind
    p = torch.nn.Parameter(w.clone())
    sf, sb = EF.wino_sets(p)
    assert R.same_values(sf.double().cpu(), uf) and R.same_values(sb.double().cpu(), ub)
    with torch.no_grad():
        p.mul_(-4.0)
    sf, sb = EF.wino_sets(p)  # rebuilt in place
    assert R.same_values(sf.double().cpu(), -4.0 * uf) and R.same_values(sb.double().cpu(), -4.0 * ub)


FN_CASES = [("Conv3x3WinoFn", "wino", (3, 32, 64, 8, 8)), ("Conv3x3S2SmallFn", "s2", (3, 32, 64, 8, 8)), ("Conv3x3S2PairFn", "pair", (3, 32, 64, 8, 8)),
            ("Conv1x1S2Fn", "c1s2", (3, 6, 34, 10, 6)), ("StemConvFn", "stem", (3, 3, 64, 10, 64)), ("Conv3x3Map2Fn", "wino", (5, 128, 128, 2, 2))]


@pytest.mark.parametrize("fn,fam,shape", FN_CASES, ids=[f[0] for f in FN_CASES])
def test_autograd_function_output_and_both_gradients_exact(ops, EF, fn, fam, shape):
    """one integer case per family through functional.py's Function: output, input gradient and weight gradient(s) together.  Unscaled integers: the
    three results sum over different things (channels / channels / images), so no power of two is constant over all three reductions."""
    fwd, bwd = fam + "_fwd", fam + "_bwd"
    cf = R.integer_case(fwd, shape, 21, scaled=False)
    cb = R.integer_case(bwd, shape, 22, scaled=False)
    for c in (cf, cb):
        assert R.exactness_margin(c["kind"], c) < 2 ** 24
    x = cf["x"].to(DEV).requires_grad_(True)
    w = _param(cf["w"])
    w1 = _param(cf["w1"]) if "w1" in cf else None
    dys = [cb["dy"].to(DEV)] + ([cb["dy1"].to(DEV)] if "dy1" in cb else [])
    args = (x, w) + ((w1,) if w1 is not None else ())
    out = getattr(EF, fn).apply(*args)
    out = out if isinstance(out, tuple) else (out,)
    grads = torch.autograd.grad(out, args, dys)
    assert_exact(fwd, cf, out, R.ref64(fwd, cf))
    cb2 = dict(cb, w=cf["w"], **({"w1": cf["w1"]} if "w1" in cf else {}))
    assert_exact(bwd, cb2, grads[:1], R.ref64(bwd, cb2))
    k, s, p = R.geometry(fwd)
    dw64 = [R._wrw(cf["x"].double(), cb["dy"].double(), k, s, p)] + ([R._wrw(cf["x"].double(), cb["dy1"].double(), 1, 2, 0)] if "dy1" in cb else [])
    mags = [R._wrw(cf["x"].double().abs(), d.double().abs(), kk, s, pp) for d, kk, pp in zip([cb["dy"]] + ([cb["dy1"]] if "dy1" in cb else []), (k, 1), (p, 0))]
    assert 4 * max(float(m.max()) for m in mags) < 2 ** 24
    for part, (g, r) in enumerate(zip(grads[1:], dw64)):
        g = g.double().cpu()
        assert R.same_values(g, r), "%s weight gradient %d: %d of %d differ, first at %s" % (
            fn, part, int((g != r).sum()), r.numel(), tuple(int(i) for i in (g != r).nonzero()[0]))


# ---- (c): ReLU-like cases against the derived bound -------------------------------------------------------------------------------------------------
# families whose ATen result is NOT held to the rule: filled from what the device shows, each with its reason
ATEN_NOT_HELD = {
    # MI355X: 227.0 against k = 129 at (9, 96, 32, 16, 16) - MIOpen's solver for the stride-2 backward-data is not a direct sum of 4 x Cout terms
    # (every other family's ATen result lies within the direct-kernel rule); ours measures 3.9 there and stays asserted
    "s2_bwd": "MIOpen's stride-2 backward-data solver breaks the direct-kernel bound",
}


def _ratio(g, r, a):
    return float(((g.double().cpu() - r).abs() / (R.U24 * a).clamp_min(1e-300)).max())


@pytest.mark.parametrize("c,mt", _with_mt(R.gpu_relu_cases()))
def test_relu_like_case_within_the_derived_rounding_bound(ops, EF, monkeypatch, c, mt):
    kind, shape, opts = c
    case = R.make_relu(kind, shape, opts)
    if mt:
        monkeypatch.setenv("EEADV_S2_MT", mt)
    ref, mags, ks = R.ref64(kind, case), R.abs_sum(kind, case), R.roundings(kind, case)
    got = run_kernel(ops, EF, kind, case)
    theirs = aten_f32(kind, case)
    fam = kind if shape[3] != 2 or kind == "wrw3x3" else kind.replace("wino", "dense")
    assert len(got) == len(ref) == len(ks) == len(theirs)
    for part, (g, t, r, a, k) in enumerate(zip(got, theirs, ref, mags, ks)):  # every result against ITS count (the pair's shortcut: Cin + 1)
        ours, aten = _ratio(g.detach(), r, a), _ratio(t, r, a)
        print("    %-10s %-22s part %d  k = %4d   ours %8.3f   ATen %8.3f   (units of 2^-24 abs_sum)" % (fam, "x".join(map(str, shape)), part, k, ours, aten))
        bad = (g.detach().double().cpu() - r).abs() > k * R.U24 * a
        assert not bool(bad.any()), "%s part %d: %d elements beyond k = %d roundings, first at %s; largest ratio %.3f" % (
            kind, part, int(bad.sum()), k, tuple(int(i) for i in bad.nonzero()[0]), ours)
        if fam not in ATEN_NOT_HELD:
            assert aten <= k, "ATen's float32 %s part %d breaks the rule: %.3f > k = %d" % (fam, part, aten, k)


# ---- (d): NaN and inf -----------------------------------------------------------------------------------------------------------------------------
def _nan_rule(got, want64, what):
    """test_gpu_eval_route._nan_footprint_rule for any operation: isnan(got) equals the NaN footprint of the direct float64 result on the host"""
    want = torch.isnan(want64)
    n = int(want.sum())
    print("    %-34s %d NaN results expected, %d found" % (what, n, int(torch.isnan(got).sum())))
    assert 0 < n < want.numel() and torch.equal(torch.isnan(got).cpu(), want), what


NAN_CASES = [("wino_fwd", (3, 32, 32, 4, 4)), ("wino_fwd", (3, 32, 32, 8, 8)), ("wino_fwd", (3, 32, 32, 16, 16)), ("wino_bwd", (3, 32, 32, 4, 4)),
             ("wino_bwd", (3, 32, 32, 8, 8)), ("wino_bwd", (3, 32, 32, 16, 16)), ("pair_fwd", (3, 32, 32, 8, 8)), ("pair_bwd", (3, 32, 32, 8, 8)),
             ("s2_fwd", (3, 32, 32, 8, 8)), ("s2_bwd", (3, 32, 32, 8, 8)), ("c1s2_fwd", (3, 6, 34, 10, 6)), ("c1s2_bwd", (3, 6, 34, 10, 6))]


@pytest.mark.parametrize("kind,shape", NAN_CASES, ids=["%s-%d" % (k, s[3]) for k, s in NAN_CASES])
def test_a_nan_has_the_footprint_of_a_direct_convolution(ops, EF, kind, shape):
    """the plain kernels, forward and backward-data: one NaN per run, on tile seams: positions with an odd coordinate (the pair's shortcut output must then stay NaN-free) and an even-even one (the shortcut has it at the one pixel that reads it)"""
    from test_gpu_eval_route import _nan_footprint_rule
    k, s, p = R.geometry(kind)
    if kind == "c1s2_fwd":
        positions = ((2, 2), (4, 0))  # a 1x1 / stride 2 convolution reads even positions only
    else:
        positions = ((1, 2), (2, 1), (2, 2)) if shape[3] > 4 else ((1, 2), (3, 0), (2, 2))  # the last: even-even, read by the pair's shortcut
    for pos in positions:
        case = R.relu_like_case(kind, shape, 5)
        name = "x" if kind in R.FWD else "dy"
        hh, ww = (pos[0] % case[name].shape[2], pos[1] % case[name].shape[3])
        case[name][1, 5, hh, ww] = float("nan")
        if "dy1" in case:
            case["dy1"][1, 3, 0, 0] = float("nan")
        got = run_kernel(ops, EF, kind, case)
        ref = R.ref64(kind, case)
        for part, (g, r) in enumerate(zip(got, ref)):
            what = "%s %dx%d part %d, NaN at %s" % (kind, shape[3], shape[3], part, (hh, ww))
            if part == 1 and not bool(torch.isnan(r).any()):
                assert not bool(torch.isnan(g).any()), what  # the shortcut reads even positions only
            elif kind in R.FWD:
                _nan_footprint_rule(g, case["x"], case["w1" if part == 1 else "w"], 2 if part == 1 else s, 0 if part == 1 else p, what)
            else:
                _nan_rule(g, r, what)


INF_CASES = [("pair_fwd", (3, 32, 32, 8, 8)), ("pair_bwd", (3, 32, 32, 8, 8)), ("s2_fwd", (3, 32, 32, 8, 8)), ("s2_bwd", (3, 32, 32, 8, 8)),
             ("c1s2_fwd", (3, 6, 34, 10, 6)), ("c1s2_bwd", (3, 6, 34, 10, 6))]


@pytest.mark.parametrize("kind,shape", INF_CASES, ids=[k for k, _ in INF_CASES])
def test_an_inf_among_zeros_gives_nan_where_a_direct_convolution_does(ops, EF, kind, shape):
    """One +inf whose neighbours (the whole image) are zeros, integer filters with exact zeros among their taps: 0 * inf = NaN appears exactly where
    the direct float64 convolution has it, +-inf where that has it, 0 elsewhere.  The direct kernels only: F(2x2, 3x3) adds +inf and -inf of one input
    in its output transform (A^T M A), so a Winograd kernel returns NaN where a direct convolution returns inf - by algorithm, as MIOpen's does."""
    case = R.integer_case(kind, shape, 9, scaled=False)
    name = "x" if kind in R.FWD else "dy"
    for n in (name, "dy1"):
        if n in case:
            case[n].zero_()
    # an even position (the 1x1 / stride 2 kernels read it too), the LAST reduction channel: the operand a lane of ee_conv.hip's 1x1 kernel re-reads,
    # clamped, past its last k-step
    last = case[name].shape[1] - 1
    case[name][1, last, 2, 2] = float("inf")
    for wn in ("w", "w1"):  # result channel 0 meets the inf through exact zeros, result channel 1 through ones
        if wn in case and kind in R.FWD:
            case[wn][0, last], case[wn][1, last] = 0.0, 1.0
        elif wn in case:
            case[wn][last, 0], case[wn][last, 1] = 0.0, 1.0
    got = run_kernel(ops, EF, kind, case)
    ref = R.ref64(kind, case)
    assert bool(torch.isnan(ref[0]).any()) and bool(torch.isinf(ref[0]).any())
    for part, (g, r) in enumerate(zip(got, ref)):
        g = g.double().cpu()
        assert torch.equal(torch.isnan(g), torch.isnan(r)), "%s part %d: %d NaN, %d expected" % (kind, part, int(torch.isnan(g).sum()), int(torch.isnan(r).sum()))
        assert torch.equal(torch.nan_to_num(g, nan=7.0), torch.nan_to_num(r, nan=7.0)), "%s part %d: inf / zero pattern" % (kind, part)


# ---- guard bands ----------------------------------------------------------------------------------------------------------------------------------
PATTERN = 0x7FC0BEEF  # one quiet-NaN bit pattern no arithmetic produces
GUARD = 4096


class Guarded:
    """n floats carved from the middle of a buffer filled with PATTERN, GUARD floats on each side"""

    def __init__(self, shape):
        self.shape = tuple(shape)
        n = 1
        for s in self.shape:
            n *= s
        self.n = n
        self.raw = torch.full((2 * GUARD + n,), PATTERN, dtype=torch.int32, device=DEV)
        self.mid = self.raw[GUARD:GUARD + n]

    def ptr(self):
        return self.mid.data_ptr()

    def floats(self):
        return self.mid.view(torch.float32).view(self.shape)

    def check(self, what, written=True):
        lo, hi = self.raw[:GUARD], self.raw[GUARD + self.n:]
        assert bool((lo == PATTERN).all()), "%s: %d floats written BEFORE the buffer" % (what, int((lo != PATTERN).sum()))
        assert bool((hi == PATTERN).all()), "%s: %d floats written PAST the buffer, first at +%d" % (
            what, int((hi != PATTERN).sum()), int((hi != PATTERN).nonzero()[0]))
        if written:
            left = self.mid == PATTERN
            assert not bool(left.any()), "%s: %d of %d result elements never written, first at flat index %d" % (
                what, int(left.sum()), self.n, int(left.nonzero()[0]))


def _abi_plan(ops, EF, N, name, kind, case, extra=None):
    """(role -> value, result shapes, workspace floats, the ops wrapper's result) for one kernel of conv_reference.ABI_ARGS"""
    B, Cin, Cout, H, W = case["shape"]
    t = {n: v.to(DEV) for n, v in case.items() if torch.is_tensor(v)}
    w = _param(case["w"]) if "w" in case else None
    w1 = _param(case["w1"]) if "w1" in case else None
    OH, OW = R.out_hw(kind, H, W)
    v = {"B": B, "Cin": Cin, "Cout": Cout, "H": H, "W": W, "K": Cout, "HW": H * W, "x": t.get("x"), "dy": t.get("dy"), "dy1": t.get("dy1"),
         "w": None if w is None else w.detach()}
    outs, ws = [(B, Cout, OH, OW)], 0
    if name == "ee_wino3x3_f32":
        back = kind == "wino_bwd"
        v.update(x=t["dy"] if back else t["x"], u=_wino_u(ops, EF, w, back), KC=Cout if back else Cin, RC=Cin if back else Cout)
        outs = [(B, v["RC"], H, H)]
    elif name == "ee_dense2x2_f32":
        v.update(w2=EF._dense_weight(w, "s1"))
    elif name.startswith("ee_conv3x3s2_small"):
        v.update(w9=EF._dense_weight(w, "s2m_f" if kind == "s2_fwd" else "s2m_b"))
    elif name.startswith("ee_conv3x3s2_pair"):
        v.update(w10=EF._dense_weight(w, "s2p_f" if kind == "pair_fwd" else "s2p_b", w1))
        if kind == "pair_fwd":
            outs = outs * 2
    elif name == "ee_stem7x7s2_fwd_stats_f32":
        ws = int(N.lib.ee_stem7x7s2_fwd_stats_floats(B, Cout, H, W))
    elif name == "ee_wrw3x3_f32":
        outs, ws = [(Cout, Cin, 3, 3)], int(N.lib.ee_wrw3x3_workspace_floats(B, Cin, Cout, H))
    elif name == "ee_wrw3x3s2_f32":
        outs, ws = [((10 if "dy1" in t else 9) * Cout * Cin,)], int(N.lib.ee_wrw3x3s2_workspace_floats(B, Cin, Cout, H, 1 if "dy1" in t else 0))
    elif name == "ee_wrw_stem7x7s2_f32":
        outs, ws = [(64, 3, 7, 7)], int(N.lib.ee_wrw_stem7x7s2_workspace_floats(B, H, W))
    elif name == "ee_wrw1x1_f32":
        outs, ws = [(Cout, Cin, 1, 1)], int(N.lib.ee_wrw1x1_workspace_floats(B, Cin, Cout, H * W))
    if kind in R.BWD:
        outs = [(B, Cin, H, W)]
    return v, outs, ws


GUARD_CASES = [
    ("ee_wino3x3_f32", "wino_fwd", (3, 32, 96, 4, 4), {}), ("ee_wino3x3_f32", "wino_bwd", (3, 32, 32, 8, 8), {}), ("ee_wino3x3_f32", "wino_fwd", (3, 48, 32, 16, 16), {}),
    ("ee_dense2x2_f32", "wino_fwd", (5, 128, 128, 2, 2), {}),
    ("ee_conv3x3s2_small_fwd_f32", "s2_fwd", (3, 32, 32, 8, 8), {}), ("ee_conv3x3s2_small_bwd_data_f32", "s2_bwd", (9, 32, 32, 4, 4), {}),
    ("ee_conv3x3s2_pair_fwd_f32", "pair_fwd", (9, 32, 32, 4, 4), {}), ("ee_conv3x3s2_pair_bwd_data_f32", "pair_bwd", (3, 32, 32, 16, 16), {}),
    ("ee_conv1x1s2_fwd_f32", "c1s2_fwd", (3, 6, 34, 10, 6), {}), ("ee_conv1x1s2_bwd_f32", "c1s2_bwd", (3, 6, 34, 10, 6), {}),
    ("ee_stem7x7s2_fwd_f32", "stem_fwd", (3, 3, 128, 10, 64), {}), ("ee_stem7x7s2_fwd_stats_f32", "stem_fwd", (3, 3, 128, 10, 64), {}),
    ("ee_stem7x7s2_bwd_data_f32", "stem_bwd", (2, 3, 17, 70, 66), {}),
    ("ee_wrw3x3_f32", "wrw3x3", (5, 32, 32, 4, 4), {}), ("ee_wrw3x3_f32", "wrw3x3", (5, 32, 32, 16, 16), {}), ("ee_wrw3x3s2_f32", "wrw3x3s2", (5, 32, 32, 8, 8), {"pair": True}),
    ("ee_wrw_stem7x7s2_f32", "wrw_stem", (5, 3, 64, 34, 96), {}), ("ee_wrw1x1_f32", "wrw1x1", (5, 64, 192, 10, 14), {}),
]


@pytest.mark.parametrize("name,kind,shape,opts", GUARD_CASES, ids=["%s-%s-%d" % (g[0], g[1], g[2][3]) for g in GUARD_CASES])
def test_guard_bands_hold_and_every_result_element_is_written(ops, EF, name, kind, shape, opts):
    """the C ABI called directly with the pointers and sizes the ops wrapper passes, on a supported partial-group shape: nothing outside the result
    and the workspace is written, every result element is, and the bits are the wrapper's (and, integer inputs, float64's)"""
    from eeadv import _native as N
    case = R.integer_case(kind, shape, sum(shape), **opts)
    assert R.exactness_margin(kind, case) < 2 ** 24
    v, out_shapes, ws_floats = _abi_plan(ops, EF, N, name, kind, case)
    outs = [Guarded(s) for s in out_shapes]
    ws = Guarded((max(ws_floats, 4),)) if "ws" in R.ABI_ARGS[name] else None
    args = []
    for role in R.ABI_ARGS[name]:
        if role == "out":
            args.append(outs[0].ptr())
        elif role == "out1":
            args.append(outs[1].ptr())
        elif role == "ws":
            args.append(ws.ptr())
        elif role == "stream":
            args.append(ops._stream())
        elif torch.is_tensor(v[role]):
            assert v[role].is_contiguous() and v[role].dtype == torch.float32
            args.append(v[role].data_ptr())
        else:
            args.append(v[role])
    N.check(getattr(N.lib, name)(*args), name)
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        o.check("%s result %d" % (name, i))
    if ws is not None:
        ws.check(name + " workspace", written=False)
    want = run_kernel(ops, EF, kind, case)
    got = [o.floats() for o in outs]
    if name == "ee_wrw3x3s2_f32":
        Cout, Cin = shape[2], shape[1]
        got = [got[0][:9 * Cout * Cin].view(Cout, Cin, 3, 3), got[0][9 * Cout * Cin:].view(Cout, Cin, 1, 1)]
    for g, w_ in zip(got, want):
        assert torch.equal(g.view(torch.int32), w_.contiguous().view(torch.int32)), name + ": bits differ from the ops wrapper's"
    assert_exact(kind, case, got, R.ref64(kind, case))


def test_guard_bands_of_the_weight_preparation(ops, EF):
    from eeadv import _native as N
    w = R.integer_case("wino_fwd", (1, 32, 64, 4, 4), 3)["w"].to(DEV)
    uf, ub = R.wino_filter_sets(w.cpu())
    for kind, want in (("wino_f", uf), ("wino_b", ub), ("wino_fb", torch.stack([uf.reshape(-1), ub.reshape(-1)]))):
        out = Guarded(EF._rearranged_shape(w, kind))
        v = {"kind": EF._NATIVE_KIND[kind], "w": w.data_ptr(), "extra": None, "out": out.ptr(), "Cout": 64, "Cin": 32, "stream": ops._stream()}
        N.check(N.lib.ee_conv_weight_prep_f32(*[v[r] for r in R.ABI_ARGS["ee_conv_weight_prep_f32"]]), kind)
        torch.cuda.synchronize()
        out.check("ee_conv_weight_prep_f32 " + kind)
        assert R.same_values(out.floats().double().cpu(), want.reshape(out.shape)), kind
