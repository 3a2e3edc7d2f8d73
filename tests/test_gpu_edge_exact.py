"""The edge front end (ee_edge.hip, ee_canny.hip, ee_stencil.hpp) held to the float64 reference of tests/edge_reference.py on inputs where
exact ties are the rule: k / 255 images, PGD iterates clamped to {0, 1}, bars on an exact 0 background, ramps across the thresholds, +-0.

Per case and per entry point:
  discrete outputs (edge, gate, the stored t2, thin != 0) equal float64 at every decided and exact-tie pixel and hold a legal value elsewhere;
  mag and thin stay inside the derived bound; gradients stay inside theirs at comparable outputs, with float64's NaN pattern;
  the fused variants give the unfused ones' bits (x_in, gate, g_hfs, g_edge), with x_hfs + w * edge placed exactly on 0 and on 1;
  an unaligned view (vec = 0 forced by the pointers) writes every result element and nothing around it.
The same criteria are applied to the float32 C oracle on the host (tests/test_edge_reference_host.py); the figures measured on the MI355X are
in DESIGN.md, "The edge front end against float64".  PARITY UNPINNED: the direction table is the derived one on both sides."""
import ctypes

import numpy as np
import pytest
import torch

import edge_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = R.cases()
IDS = [c[0] for c in CASES]
WEIGHTS = (1.0, 0.75)  # 0.75: w * sum_c g_hfs_c rounds, and -w, 1 - w place x_hfs + w * edge on 0 and 1 through a real product
_cache = {}
check_edge, check_bound, check_grad = R.check_edge, R.check_bound, R.check_grad


@pytest.fixture(scope="module")
def ops():
    from eeadv import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def wts(ops):
    return ops.EdgeWeights(1.0)


def ref(case, wts, mode):
    cid, fam, x, prm = case
    if (cid, mode) not in _cache:
        _cache[(cid, mode)] = R.forward(x, wts, prm["alpha"], prm["low"], prm["high"], mode)
    return _cache[(cid, mode)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def low_pass(x, seed, w=1.0):
    """x_hfs values that put x_hfs + w * edge exactly on 0 and on 1 for either edge bit, inside, and outside [0, 1]"""
    rng = np.random.RandomState(seed)
    pick = np.array([0.0, 1.0, -w, 1.0 - w, 0.5, -0.25, 1.25, 37 / 255], np.float32)
    return pick[rng.randint(0, len(pick), size=x.shape)]


def fused_expect(xh, edge, g_in, W_EDGE=1.0):
    """the front end's combine restated on the device in the documented order: s = x_hfs + w * edge, gate = 0 <= s <= 1, u = w * sum_c g_hfs_c"""
    s = xh + W_EDGE * edge
    gate = ((s >= 0) & (s <= 1)).to(torch.uint8)
    g_hfs = torch.where(gate.bool(), g_in, torch.zeros_like(g_in))
    acc = g_hfs[:, 0:1].clone()
    for c in range(1, g_hfs.shape[1]):
        acc = acc + g_hfs[:, c:c + 1]
    return torch.clamp(s, 0.0, 1.0), gate, g_hfs, (acc * W_EDGE).contiguous()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_step125_and_its_front_end(ops, wts, case):
    cid, fam, x, prm = case
    a, hi = prm["alpha"], prm["high"]
    m = ref(case, wts, "canny")
    xd, u = dev(x), R.upstream(x.shape, 11)
    edge, mag = ops.edge125_fwd(xd, wts, a, hi, want_mag=True)
    check_edge(host(edge), m["edge125"], m["edge125_dec"], "edge125")
    r_mag = check_bound(host(mag), m["mag"], m["e_mag"], m["finite"], "mag")
    g, eb, comp = R.backward125(m, u, wts)
    gd = ops.edge125_bwd(xd, dev(u), wts, a, hi)
    r_g = check_grad(host(gd), g, eb, comp, "edge125 gradient")
    print("%s step125: mag %.3f gradient %.3f of the bound" % (cid, r_mag, r_g))
    # fused: bits of the unfused kernels
    for W_EDGE in WEIGHTS:
        xh, g_in = dev(low_pass(x, 3, W_EDGE)), dev(R.upstream(x.shape, 13, C=x.shape[1]))
        want_in, want_gate, want_hfs, u_f = fused_expect(xh, edge, g_in, W_EDGE)
        want_edge = ops.edge125_bwd(xd, u_f, wts, a, hi)
        x_in, gate, e2 = ops.frontend_fwd(xd, xh, wts, a, hi, W_EDGE, want_edge=True)
        x_in2, gate2, e3, sx, sy = ops.frontend_fwd_save(xd, xh, wts, a, hi, W_EDGE, want_edge=True)
        for got, want, what in ((e2, edge, "edge"), (e3, edge, "edge (save)"), (x_in, want_in, "x_in"), (x_in2, want_in, "x_in (save)"),
                                (gate, want_gate, "gate"), (gate2, want_gate, "gate (save)")):
            assert torch.equal(bits(got), bits(want)), "frontend_fwd %s, w = %g: bits differ from the unfused path" % (what, W_EDGE)
        assert bool(((xh + W_EDGE * edge) == 0).any()) and bool(((xh + W_EDGE * edge) == 1).any())
        check_bound(host(sx), m["gx"], m["e_gx"], m["finite"], "saved gx1")
        check_bound(host(sy), m["gy"], m["e_gy"], m["finite"], "saved gy1")
        for g_hfs, g_edge, what in ((ops.frontend_bwd(g_in, gate, xd, wts, a, hi, W_EDGE)) + ("frontend_bwd",),
                                    (ops.frontend_bwd_saved(g_in, gate, sx, sy, wts, a, hi, W_EDGE)) + ("frontend_bwd_saved",)):
            assert torch.equal(bits(g_hfs), bits(want_hfs)), what + " g_hfs"
            assert torch.equal(bits(g_edge), bits(want_edge)), "%s g_edge, w = %g: bits differ from edge125_bwd" % (what, W_EDGE)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_full_canny_and_its_front_end(ops, wts, case):
    cid, fam, x, prm = case
    a, lo, hi = prm["alpha"], prm["low"], prm["high"]
    m = ref(case, wts, "canny")
    xd, u = dev(x), R.upstream(x.shape, 11)
    edge = ops.canny_fwd(xd, wts, a, lo, hi)
    check_edge(host(edge), m["edge"], m["edge_dec"], "canny edge")
    g, eb, comp = R.backward_canny(m, u, wts)
    r_g = check_grad(host(ops.canny_bwd(xd, dev(u), wts, a, lo, hi)), g, eb, comp, "canny gradient")
    print("%s canny: gradient %.3f of the bound; decided edge pixels %.3f" % (cid, r_g, m["edge_dec"].mean()))
    for W_EDGE in WEIGHTS:
        xh, g_in = dev(low_pass(x, 5, W_EDGE)), dev(R.upstream(x.shape, 17, C=x.shape[1]))
        want_in, want_gate, want_hfs, u_f = fused_expect(xh, edge, g_in, W_EDGE)
        x_in, gate, e2 = ops.canny_frontend_fwd(xd, xh, wts, a, lo, hi, W_EDGE, want_edge=True)
        for got, want, what in ((e2, edge, "edge"), (x_in, want_in, "x_in"), (gate, want_gate, "gate")):
            assert torch.equal(bits(got), bits(want)), "canny_frontend_fwd %s, w = %g: bits differ from the unfused path" % (what, W_EDGE)
        g_hfs, g_edge = ops.canny_frontend_bwd(g_in, gate, xd, wts, a, lo, hi, W_EDGE)
        assert torch.equal(bits(g_hfs), bits(want_hfs)), "canny_frontend_bwd g_hfs"
        assert torch.equal(bits(g_edge), bits(ops.canny_bwd(xd, u_f, wts, a, lo, hi))), "canny_frontend_bwd g_edge, w = %g: bits differ from canny_bwd" % W_EDGE


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bpda_stored_planes_and_replay(ops, wts, case):
    cid, fam, x, prm = case
    lo, hi = prm["low"], prm["high"]
    m = ref(case, wts, "bpda")
    xd, u = dev(x), R.upstream(x.shape, 11)
    edge, thin, t2 = ops.canny_bpda_fwd(xd, wts, lo, hi)
    check_edge(host(edge), m["edge"], m["edge_dec"], "bpda edge")
    th, t2h = host(thin), host(t2)
    bad = m["t2_dec"] & (t2h != m["t2"])
    assert not bad.any(), "stored t2 differs at %d decided pixels, first %s" % (int(bad.sum()), np.argwhere(bad)[0])
    assert np.isin(t2h, (0.0, 0.5, 1.0)).all()
    bad = m["t_known"] & ((th != 0) != (m["thin"] != 0))
    assert not bad.any(), "thin != 0 differs at %d decided pixels, first %s" % (int(bad.sum()), np.argwhere(bad)[0])
    r_t = check_bound(th, m["thin"], m["e_thin"], m["t_known"] & ~m["t_zero_sure"], "thin")
    assert (th[m["t_zero_sure"]] == 0).all()
    loose = ~m["t_known"] & m["finite"]          # undecided suppression: 0 or the magnitude, nothing else
    assert ((th[loose] == 0) | (np.abs(th[loose] - m["mag"][loose]) <= m["e_mag"][loose])).all()
    # backward: float64 replay from the kernel's own planes
    g, eb, comp = R.backward_bpda(m, u, th, t2h, m["removed"], wts)
    r_g = check_grad(host(ops.canny_bpda_bwd(xd, dev(u), thin, t2, wts, lo, hi)), g, eb, comp, "bpda gradient")
    print("%s bpda: thin %.3f gradient %.3f of the bound" % (cid, r_t, r_g))


@pytest.mark.parametrize("shape", R.SHAPES[:3], ids=["%dx%dx%dx%d" % s for s in R.SHAPES[:3]])
def test_eval_paths_around_nan_and_inf(ops, wts, shape):
    """forward only: a NaN or +-inf input reaches its 5x5 neighbourhood and nothing else; every other pixel keeps its class"""
    x, prm = R.specials(shape, 3, eval_only=True)
    m = R.forward(x, wts, prm["alpha"], prm["low"], prm["high"], "canny")
    foot = R.nonfinite_footprint(shape)
    edge, mag = ops.edge125_fwd(dev(x), wts, prm["alpha"], prm["high"], want_mag=True)
    assert np.array_equal(~np.isfinite(host(mag)), foot)
    check_bound(host(mag), m["mag"], m["e_mag"], m["finite"], "mag")
    check_edge(host(edge), m["edge125"], m["edge125_dec"], "edge125")
    ec = ops.canny_fwd(dev(x), wts, prm["alpha"], prm["low"], prm["high"])
    check_edge(host(ec), m["edge"], m["edge_dec"], "canny edge")
    mb = R.forward(x, wts, 0.0, prm["low"], prm["high"], "bpda")
    eb, thin, t2 = ops.canny_bpda_fwd(dev(x), wts, prm["low"], prm["high"])
    check_edge(host(eb), mb["edge"], mb["edge_dec"], "bpda edge")
    assert not (mb["t2_dec"] & (host(t2) != mb["t2"])).any() and np.array_equal(~np.isfinite(host(thin)) & ~foot, np.zeros_like(foot))
    # fused eval forwards: the unfused bits wherever the edge is finite, NaN and a closed gate where it is not
    for w in WEIGHTS:
        xh = dev(low_pass(x, 7, w))
        for (x_in, gate, e2), e1 in ((ops.frontend_fwd(dev(x), xh, wts, prm["alpha"], prm["high"], w, want_edge=True), edge),
                                     (ops.canny_frontend_fwd(dev(x), xh, wts, prm["alpha"], prm["low"], prm["high"], w, want_edge=True), ec)):
            fin = torch.isfinite(e1)
            assert torch.equal(torch.isnan(e2), torch.isnan(e1)) and torch.equal(e2[fin], e1[fin])
            want_in, want_gate, _, _ = fused_expect(xh, e1, torch.zeros_like(xh), w)
            finc = fin.expand_as(xh)
            assert torch.equal(x_in[finc], want_in[finc]) and torch.equal(gate[finc], want_gate[finc])
            assert bool(torch.isnan(x_in[~finc]).all()) and not bool(gate[~finc].any())


@pytest.mark.parametrize("name", ["CannyFilter_step125_1", "CannyFilter", "CannyFilter_BPDA", "ee_front_end", "ee_front_end_step125"])
def test_core_modules_take_the_same_kernels(ops, wts, name):
    """the autograd path of utils.core on every case: the bits of the ops calls above"""
    import utils.core as core
    W_EDGE = 0.75
    for cid, fam, x, prm in CASES:
        a, lo, hi = prm["alpha"], prm["low"], prm["high"]
        xd = dev(x).requires_grad_(True)
        u = dev(R.upstream(x.shape, 11))
        if name.startswith("ee_front_end"):
            full = name == "ee_front_end"
            canny = (core.CannyFilter if full else core.CannyFilter_step125_1)(alpha=a, use_cuda=True).to(DEV)
            xh = dev(low_pass(x, 5, W_EDGE)).requires_grad_(True)
            g_in = dev(R.upstream(x.shape, 17, C=x.shape[1]))
            out = core.ee_front_end(xd, xh, canny, W_EDGE, lo, hi)
            out.backward(g_in)
            if full:
                x_in, gate, _ = ops.canny_frontend_fwd(xd.detach(), xh.detach(), wts, a, lo, hi, W_EDGE)
                g_hfs, g_edge = ops.canny_frontend_bwd(g_in, gate, xd.detach(), wts, a, lo, hi, W_EDGE)
            else:
                x_in, gate, _ = ops.frontend_fwd(xd.detach(), xh.detach(), wts, a, hi, W_EDGE)
                g_hfs, g_edge = ops.frontend_bwd(g_in, gate, xd.detach(), wts, a, hi, W_EDGE)
            assert torch.equal(bits(out.detach()), bits(x_in)) and torch.equal(bits(xh.grad), bits(g_hfs)), cid
            assert torch.equal(bits(xd.grad), bits(g_edge.expand_as(xd).contiguous())), cid
            continue
        mod = getattr(core, name)(alpha=a, use_cuda=True).to(DEV)
        out = mod(xd, low_threshold=lo, high_threshold=hi, hysteresis=True)
        out.backward(u)
        if name == "CannyFilter_step125_1":
            e, g = ops.edge125_fwd(xd.detach(), wts, a, hi), ops.edge125_bwd(xd.detach(), u, wts, a, hi)
        elif name == "CannyFilter":
            e, g = ops.canny_fwd(xd.detach(), wts, a, lo, hi), ops.canny_bwd(xd.detach(), u, wts, a, lo, hi)
        else:
            e, thin, t2 = ops.canny_bpda_fwd(xd.detach(), wts, lo, hi)
            g = ops.canny_bpda_bwd(xd.detach(), u, thin, t2, wts, lo, hi)
        assert torch.equal(bits(out.detach()), bits(e)), "%s forward, %s" % (name, cid)
        assert torch.equal(bits(xd.grad), bits(g.expand_as(xd).contiguous())), "%s backward, %s" % (name, cid)


# ---- float32 magnitudes placed exactly on alpha, on high and 1.001f above high --------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CASES if c[0] in R.TIE_BASES], ids=[c[0] for c in CASES if c[0] in R.TIE_BASES])
def test_kernel_magnitudes_placed_on_the_thresholds(ops, wts, case):
    """the thresholds are the kernel's own float32 magnitudes at chosen pixels (want_mag), so the equality is exact: the strict rules of
    edge_reference.threshold_tie_checks must hold there, in step125, the full filter and BPDA"""
    cid, fam, x, prm = case
    ev = {"mag": lambda x_: host(ops.edge125_fwd(dev(x_), wts, 0.0, 0.5, want_mag=True)[1]),
          "edge125": lambda x_, a, hi: host(ops.edge125_fwd(dev(x_), wts, a, hi)),
          "grad125": lambda x_, u, a, hi: host(ops.edge125_bwd(dev(x_), dev(u), wts, a, hi)),
          "canny": lambda x_, a, lo, hi: host(ops.canny_fwd(dev(x_), wts, a, lo, hi)),
          "canny_grad": lambda x_, u, a, lo, hi: host(ops.canny_bwd(dev(x_), dev(u), wts, a, lo, hi)),
          "bpda_edge": lambda x_, lo, hi: host(ops.canny_bpda_fwd(dev(x_), wts, lo, hi)[0]),
          "bpda_planes": lambda x_, lo, hi: tuple(host(t) for t in ops.canny_bpda_fwd(dev(x_), wts, lo, hi)[1:])}
    ran = R.threshold_tie_checks(x, prm, wts, ev)
    assert {"alpha", "high125", "high"} <= set(ran), ran
    if fam == "stripes":   # the cases with kept magnitudes above 1.1
        assert "ste" in ran, ran


# ---- the unaligned view: vec = 0 forced by the pointers (W % 4 == 0) ----------------------------------------------------------------------------
PATTERN = 0x7FC0BEEF  # one quiet-NaN bit pattern no arithmetic produces
GUARD = 4096


class Guarded:
    """n elements carved one element past a 16-byte boundary out of a buffer filled with PATTERN, a guard band on each side"""

    def __init__(self, shape, dtype=torch.float32):
        self.shape, self.dtype = tuple(shape), dtype
        self.n = int(np.prod(shape))
        if dtype == torch.float32:
            self.raw = torch.full((2 * GUARD + self.n + 1,), PATTERN, dtype=torch.int32, device=DEV)
            self.fill = PATTERN
        else:
            self.raw = torch.full((2 * GUARD + self.n + 1,), 0xA5, dtype=torch.uint8, device=DEV)
            self.fill = 0xA5
        self.mid = self.raw[GUARD + 1:GUARD + 1 + self.n]
        assert self.mid.data_ptr() % 16 != 0

    def ptr(self):
        return ctypes.c_void_p(self.mid.data_ptr())

    def value(self):
        return (self.mid.view(torch.float32) if self.dtype == torch.float32 else self.mid).view(self.shape)

    def load(self, t):
        self.value().copy_(t)
        return self

    def check(self, what, written=True):
        lo, hi = self.raw[:GUARD + 1], self.raw[GUARD + 1 + self.n:]
        assert bool((lo == self.fill).all()) and bool((hi == self.fill).all()), what + ": written outside the result"
        if written and self.dtype == torch.float32:
            assert not bool((self.mid == PATTERN).any()), what + ": result elements never written"


def test_unaligned_views_take_the_scalar_path_and_keep_their_guard_bands(ops, wts):
    from eeadv import _native as N
    cid, fam, x, prm = [c for c in CASES if c[0] == "stripes-2x3x32x32"][0]
    B, C, H, W = x.shape
    a, lo, hi = prm["alpha"], prm["low"], prm["high"]
    W_EDGE = 0.75
    xd, u = dev(x), dev(R.upstream(x.shape, 11))
    xh, g_in = dev(low_pass(x, 5, W_EDGE)), dev(R.upstream(x.shape, 17, C=C))
    st = ops._stream()
    xg, ug, xhg, gig = Guarded(x.shape).load(xd), Guarded(u.shape).load(u), Guarded(x.shape).load(xh), Guarded(x.shape).load(g_in)
    one, full = (B, 1, H, W), (B, C, H, W)

    e, mg = Guarded(one), Guarded(one)
    N.check(N.lib.ee_edge125_fwd_f32(xg.ptr(), B, C, H, W, wts.ptr, a, hi, e.ptr(), mg.ptr(), st), "ee_edge125_fwd_f32")
    want_e, want_m = ops.edge125_fwd(xd, wts, a, hi, want_mag=True)
    g = Guarded(one)
    N.check(N.lib.ee_edge125_bwd_f32(xg.ptr(), ug.ptr(), B, C, H, W, wts.ptr, a, hi, g.ptr(), st), "ee_edge125_bwd_f32")
    ce = Guarded(one)
    N.check(N.lib.ee_canny_fwd_f32(xg.ptr(), None, B, C, H, W, wts.ptr, wts.dirs_ptr, a, lo, hi, 0.0, ce.ptr(), None, None, st), "ee_canny_fwd_f32")
    cg = Guarded(one)
    N.check(N.lib.ee_canny_bwd_f32(xg.ptr(), ug.ptr(), None, None, B, C, H, W, wts.ptr, wts.dirs_ptr, a, lo, hi, 0.0, cg.ptr(), None, st),
            "ee_canny_bwd_f32")
    fx, fg, fe = Guarded(full), Guarded(full, torch.uint8), Guarded(one)
    N.check(N.lib.ee_canny_fwd_f32(xg.ptr(), xhg.ptr(), B, C, H, W, wts.ptr, wts.dirs_ptr, a, lo, hi, W_EDGE, fe.ptr(), fx.ptr(), fg.ptr(), st),
            "ee_canny_fwd_f32 (fused)")
    want_in, want_gate, _ = ops.canny_frontend_fwd(xd, xh, wts, a, lo, hi, W_EDGE)
    bh, bg = Guarded(full), Guarded(one)
    N.check(N.lib.ee_canny_bwd_f32(xg.ptr(), None, gig.ptr(), fg.ptr(), B, C, H, W, wts.ptr, wts.dirs_ptr, a, lo, hi, W_EDGE, bg.ptr(), bh.ptr(), st),
            "ee_canny_bwd_f32 (fused)")
    want_hfs, want_ge = ops.canny_frontend_bwd(g_in, want_gate, xd, wts, a, lo, hi, W_EDGE)
    sx_in, sgate, sgx, sgy = Guarded(full), Guarded(full, torch.uint8), Guarded(one), Guarded(one)
    N.check(N.lib.ee_frontend_fwd_save_f32(xg.ptr(), xhg.ptr(), B, C, H, W, wts.ptr, a, hi, W_EDGE, sx_in.ptr(), sgate.ptr(), None, sgx.ptr(),
                                           sgy.ptr(), st), "ee_frontend_fwd_save_f32")
    w_in, w_gate, _, w_gx, w_gy = ops.frontend_fwd_save(xd, xh, wts, a, hi, W_EDGE)
    sh, sg = Guarded(full), Guarded(one)
    N.check(N.lib.ee_frontend_bwd_saved_f32(gig.ptr(), sgate.ptr(), sgx.ptr(), sgy.ptr(), B, C, H, W, wts.ptr, a, hi, W_EDGE, sh.ptr(), sg.ptr(), st),
            "ee_frontend_bwd_saved_f32")
    w_hfs, w_ge = ops.frontend_bwd_saved(g_in, w_gate, w_gx, w_gy, wts, a, hi, W_EDGE)
    torch.cuda.synchronize()
    for got, want, what in ((e, want_e, "edge125"), (mg, want_m, "mag"), (g, ops.edge125_bwd(xd, u, wts, a, hi), "edge125 gradient"),
                            (ce, ops.canny_fwd(xd, wts, a, lo, hi), "canny edge"), (cg, ops.canny_bwd(xd, u, wts, a, lo, hi), "canny gradient"),
                            (fx, want_in, "x_in"), (fg, want_gate, "gate"), (bh, want_hfs, "g_hfs"), (bg, want_ge, "g_edge"),
                            (sx_in, w_in, "x_in (save)"), (sgate, w_gate, "gate (save)"), (sgx, w_gx, "gx1"), (sgy, w_gy, "gy1"),
                            (sh, w_hfs, "g_hfs (saved)"), (sg, w_ge, "g_edge (saved)")):
        got.check(what)
        assert torch.equal(bits(got.value()), bits(want)), what + ": the scalar path's bits differ from the 16-byte path's"
    for inp, what in ((xg, "x"), (ug, "u"), (xhg, "x_hfs"), (gig, "g_in")):
        inp.check(what, written=False)
