"""The float64 reference of the edge front end (tests/edge_reference.py) checked on the host: against torch float64 autograd through a plain
restatement of the three filters, against the committed reference fixtures, and - what validates the bound and the classes without a GPU -
the float32 C oracle (host libm) held to exactly the criteria tests/test_gpu_edge_exact.py applies to the kernels.  The conditions the
case generators must meet (shares of undecided / exact-tie / comparable pixels) are asserted on the reference alone.  PARITY UNPINNED as
everywhere: the direction table is the derived one on both sides."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import edge_reference as R
from oracle import ee_oracle as O

check_edge, check_bound, check_grad = R.check_edge, R.check_bound, R.check_grad
WTS = None
CASES = R.cases()
IDS = [c[0] for c in CASES]
_maps = {}


@pytest.fixture(scope="module", autouse=True)
def _weights():
    """the project's float32 filter weights and direction table; imported here so that a missing library fails the tests, not the collection"""
    global WTS
    from eeadv import ops
    WTS = ops.EdgeWeights(1.0)


def maps(cid, x, prm, mode):
    key = (cid, mode)
    if key not in _maps:
        _maps[key] = R.forward(x, WTS, prm["alpha"], prm["low"], prm["high"], mode)
    return _maps[key]


# ---- a plain torch restatement (float64, autograd) ------------------------------------------------------------------------------------------
class _Sign(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v):
        ctx.save_for_backward(v)
        return torch.where(v > 0, torch.ones_like(v), -torch.ones_like(v))

    @staticmethod
    def backward(ctx, g):
        (v,) = ctx.saved_tensors
        return torch.where(v.abs() > R.ONE001, torch.zeros_like(g), g)


class _Cmp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, thr):
        ctx.save_for_backward(v)
        ctx.thr = thr
        return (v > thr).to(v.dtype)

    @staticmethod
    def backward(ctx, g):
        (v,) = ctx.saved_tensors
        return torch.where((v <= ctx.thr) | (v > R.ONE001), torch.zeros_like(g), g), None


class _Eq(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v):
        ctx.save_for_backward(v)
        return (v == 0.5).to(v.dtype)

    @staticmethod
    def backward(ctx, g):
        (v,) = ctx.saved_tensors
        return torch.where(v != 0.5, torch.zeros_like(g), g)


def torch_filter(x, prm, mode):
    g, sx, sy = (torch.from_numpy(w)[None, None] for w in R.weights64(WTS))
    C = x.shape[1]
    alpha, low, high = R.f32(prm["alpha"]), R.f32(prm["low"]), R.f32(prm["high"])
    rp = torch.nn.ReplicationPad2d(1)
    bl = torch.cat([F.conv2d(rp(x[:, c:c + 1]), g) for c in range(C)], 1)
    gx = F.conv2d(rp(bl), sx.repeat(1, C, 1, 1)) / C
    gy = F.conv2d(rp(bl), sy.repeat(1, C, 1, 1)) / C
    mag = (gx ** 2 + gy ** 2) ** 0.5
    if mode != "bpda":
        mag = torch.where(mag < alpha, torch.zeros_like(mag), mag)
    if mode == "step125":
        return _Cmp.apply(mag.clone(), high) * 1
    ori = torch.round((torch.atan(gy / gx) * (360 / np.pi) + 180) / 45) * 45
    wd = torch.zeros(8, 1, 3, 3, dtype=torch.float64)
    for k, (dr, dc) in enumerate(R.dirs_of(WTS)):
        wd[k, 0, 1, 1], wd[k, 0, 1 + dr, 1 + dc] = 1.0, -1.0
    directional = F.conv2d(mag, wd, padding=1)
    pidx = (ori / 45) % 8
    thin = mag.clone()
    for k in range(4):
        oriented = ((pidx == k) * 1 + (pidx == k + 4) * 1)
        is_max = (torch.stack([directional[:, k], directional[:, k + 4]]).min(dim=0)[0] > 0.0).unsqueeze(1)
        rem = (is_max == 0) * 1 * oriented > 0
        if mode == "canny":
            thin[rem] = 0.0
        else:
            thin = thin * ~rem
    wh = torch.full((1, 1, 3, 3), 1.25, dtype=torch.float64)
    if mode == "canny":
        lo_, hi_ = (_Sign.apply(thin - low) + 1) / 2, (_Sign.apply(thin - high) + 1) / 2
        t2 = lo_ * 0.5 + hi_ * 0.5
        return hi_ * 1 + (F.conv2d(t2, wh, padding=1) > 1) * ((t2 == 0.5) * 1) * 1
    lo_, hi_ = _Cmp.apply(thin, low), _Cmp.apply(thin, high)
    t2 = lo_ * 0.5 + hi_ * 0.5
    return hi_ * 1 + _Cmp.apply(F.conv2d(t2, wh, padding=1), 1.0) * _Eq.apply(t2) * 1


@pytest.mark.parametrize("mode", ["step125", "canny", "bpda"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_agrees_with_torch_float64_autograd(case, mode):
    cid, fam, x, prm = case
    m = maps(cid, x, prm, mode)
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    e = torch_filter(xt, prm, mode)
    u = R.upstream(x.shape, 5)
    (e * torch.from_numpy(u.astype(np.float64))).sum().backward()
    ref_e = m["edge125"] if mode == "step125" else m["edge"]
    cls = m["cls125"] if mode == "step125" else m["cls"]
    np.testing.assert_array_equal(e.detach().numpy()[cls != R.UNDECIDED], ref_e[cls != R.UNDECIDED])
    if mode == "step125":
        g, _, comp = R.backward125(m, u, WTS)
    elif mode == "canny":
        g, _, comp = R.backward_canny(m, u, WTS)
    else:
        g, _, comp = R.backward_bpda(m, u, m["thin"], m["t2"], m["removed"], WTS)
    gt = xt.grad.numpy()
    for c in range(x.shape[1]):
        a, b = gt[:, c:c + 1], g
        assert np.array_equal(np.isnan(a)[comp], np.isnan(b)[comp]), "NaN pattern"
        ok = comp & ~np.isnan(b)
        np.testing.assert_allclose(a[ok], b[ok], rtol=1e-10, atol=1e-12)


def test_reference_agrees_with_the_committed_fixtures(golden):
    G = golden("edge125")
    for name in ["rand_tiny", "rand_mnist", "rect_mnist", "rect_rgb", "ramp_thr", "ragged", "two_ch", "one_px", "thin", "big_mag"]:
        x, (alpha, high), u = G[name + "__x"], G[name + "__alpha_high"], G[name + "__u"]
        if x.shape[2] < 2 or x.shape[3] < 2:
            continue
        m = R.forward(x, WTS, float(alpha), 0.0, float(high), "step125")
        dec = m["edge125_dec"]
        assert np.array_equal(G[name + "__edge"][dec], m["edge125"][dec].astype(np.uint8)), name
        g, e, comp = R.backward125(m, u, WTS)
        ref = G[name + "__gx"][:, :1]
        check_grad(ref, g, e + 2e-6, comp, "edge125 fixture " + name)   # the fixture is a float32 torch result: its own rounding on top
    G = golden("canny_full_unpinned")
    for name in ["rand_rgb", "rand_mnist", "rect_rgb"]:
        x, u = G[name + "__x"], G[name + "__u"]
        alpha, low, high = [float(v) for v in G[name + "__alpha_low_high"]]
        for cls, mode in (("CannyFilter", "canny"), ("CannyFilter_BPDA", "bpda")):
            m = R.forward(x, WTS, alpha, low, high, mode)
            check_edge(G[name + "__" + cls + "__edge"].astype(np.float64), m["edge"], m["edge_dec"], "%s %s" % (name, cls))
            if mode == "canny":
                g, e, comp = R.backward_canny(m, u, WTS)
            else:
                g, e, comp = R.backward_bpda(m, u, m["thin"], m["t2"], m["removed"], WTS, own_planes=False)
            check_grad(G[name + "__" + cls + "__gx"][:, :1], g, e + 2e-6, comp, "%s %s gradient" % (name, cls))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_c_oracle_passes_the_criteria_of_the_gpu_test(case):
    """float32 in another operation order than the reference's, host libm atanf: inside every bound, equal at every decided / tie pixel"""
    cid, fam, x, prm = case
    a, lo, hi = prm["alpha"], prm["low"], prm["high"]
    u = R.upstream(x.shape, 11)
    m = maps(cid, x, prm, "canny")
    e, mag, gx, gy = O.edge125_fwd(x, a, hi, want_internals=True)
    check_edge(e, m["edge125"], m["edge125_dec"], "edge125")
    w = {"mag": check_bound(mag, m["mag"], m["e_mag"], m["finite"], "mag"),
         "gx": max(check_bound(gx, m["gx"], m["e_gx"], m["finite"], "gx1"), check_bound(gy, m["gy"], m["e_gy"], m["finite"], "gy1"))}
    g, eb, comp = R.backward125(m, u, WTS)
    w["g125"] = check_grad(O.edge125_bwd(x, u, a, hi), g, eb, comp, "edge125 gradient")
    check_edge(O.canny_fwd(x, a, lo, hi), m["edge"], m["edge_dec"], "canny edge")
    g, eb, comp = R.backward_canny(m, u, WTS)
    w["gcanny"] = check_grad(O.canny_bwd(x, u, a, lo, hi), g, eb, comp, "canny gradient")
    mb = maps(cid, x, prm, "bpda")
    check_edge(O.canny_bpda_fwd(x, lo, hi), mb["edge"], mb["edge_dec"], "bpda edge")
    # the oracle keeps no thin / t2 planes: the replay takes the reference's own, which are the oracle's wherever the pixel is decided
    g, eb, comp = R.backward_bpda(mb, u, mb["thin"], mb["t2"], mb["removed"], WTS, own_planes=False)
    w["gbpda"] = check_grad(O.canny_bpda_bwd(x, u, lo, hi), g, eb, comp, "bpda gradient")
    print("%s worst |oracle - ref64| / bound: %s" % (cid, " ".join("%s %.3f" % kv for kv in sorted(w.items()))))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_generators_meet_their_conditions(case):
    cid, fam, x, prm = case
    assert x.shape[0] >= 2 and x.dtype == np.float32
    for mode in ("canny", "bpda"):
        m = maps(cid, x, prm, mode)
        sh = R.shares(m["cls"])
        assert sh["undecided"] <= (0.05 if fam == "ramp" else 0.01), (mode, sh)
        assert 1.0 - R.comparable(m["cls"]).mean() <= 0.10, (mode, "gradient outputs left out", 1.0 - R.comparable(m["cls"]).mean())
        assert 1.0 - R.comparable(m["cls125"]).mean() <= 0.10
        assert R.shares(m["cls125"])["undecided"] <= (0.05 if fam == "ramp" else 0.01), R.shares(m["cls125"])
        if fam != "ramp":
            assert sh["tie"] >= 0.20, (mode, sh)
        print("%s %s decided %.3f tie %.3f undecided %.4f not comparable %.3f" % (cid, mode, sh["decided"], sh["tie"], sh["undecided"],
                                                                                1.0 - R.comparable(m["cls"]).mean()))
    if fam == "stripes" and x.shape[2] * x.shape[3] >= 500:  # a 9x9 image has 81 pixels and no room for eight oriented regions
        m = maps(cid, x, prm, "canny")
        assert set(m["idx"][m["idx_dec"] & (m["idx"] >= 0)].astype(int).tolist()) == set(range(8))
        assert int((m["rem_tie"] & m["removed"] & (m["magA"] > 0)).sum()) >= 100


def test_ramp_crosses_every_threshold_and_low_zero_is_an_exact_tie():
    for cid, fam, x, prm in CASES:
        if fam != "ramp":
            continue
        m = maps(cid, x, prm, "canny")
        t = m["thin"][m["t_known"]]
        for thr in (prm["alpha"], prm["high"], prm["high"] + 1.001):
            assert (m["mag"] < thr).any() and (m["mag"] > thr).any(), (cid, thr)
        if prm["low"] == 0.0:
            z = m["t_zero_sure"]
            assert z.mean() > 0.2 and (m["t2"][z] == 0).all()   # t = 0 sits exactly on low = 0: strict >, so not weak
            assert (O.canny_fwd(x, prm["alpha"], 0.0, prm["high"])[R._box(z, 1, np.logical_and)] == 0).all()
        assert t.size


def test_specials_nonfinite_footprint_is_the_5x5_support():
    for shape in R.SHAPES[:2]:
        x, prm = R.specials(shape, 3, eval_only=True)
        _, mag, _, _ = O.edge125_fwd(x, prm["alpha"], prm["high"], want_internals=True)
        m = R.forward(x, WTS, prm["alpha"], prm["low"], prm["high"], "canny")
        foot = R.nonfinite_footprint(shape)
        assert np.array_equal(~np.isfinite(mag), foot) and np.array_equal(~np.isfinite(m["mag"]), foot)
        assert (m["cls"][foot] == R.UNDECIDED).all()
        check_edge(O.canny_fwd(x, prm["alpha"], prm["low"], prm["high"]), m["edge"], m["edge_dec"], "canny edge around NaN / inf")


ORACLE = {"mag": lambda x: O.edge125_fwd(x, 0.0, 0.5, want_internals=True)[1], "edge125": O.edge125_fwd, "grad125": O.edge125_bwd,
          "canny": O.canny_fwd, "canny_grad": O.canny_bwd, "bpda_edge": O.canny_bpda_fwd, "bpda_planes": lambda x, lo, hi: None}


def test_oracle_magnitudes_placed_on_alpha_high_and_high_plus_1001():
    """the thresholds are the oracle's own float32 magnitudes at chosen pixels: equality is exact, and the strict rule must hold there"""
    ran = []
    for cid, fam, x, prm in CASES:
        if cid in R.TIE_BASES:
            ran += R.threshold_tie_checks(x, prm, WTS, ORACLE)
    assert ran.count("alpha") >= 4 and ran.count("high125") >= 4 and ran.count("high") >= 4 and ran.count("ste") >= 3, ran
