"""GPU: APGD in the L2 threat model - ee_apgd_step_l2_f32 (csrc/ee_apgd_l2.hip) against a numpy restatement, engine.apgd_loop(norm="L2")
eager against graph replay and against tests/apgd_l2_reference.py teacher-forced on the device's gradients, the Linf route left as it was,
and the doors (APGD_T, APGD_Rand, the Tiny-ImageNet driver, Cascade-Rand).

What is bit-exact and what is not.  A norm is (float) sqrt(S) with S summed in double in the kernel's own order; the test's S is the exact sum
(math.fsum) of the same exact squares.  At most 2^18 non-negative terms summed in double carry a relative error below 2^18 * 2^-53 - far
under half an f32 ulp - so the kernel's float is the correctly rounded one or its neighbour: 1 ulp, derived, not measured.  Everything
element-wise is f32 arithmetic rounded once per operation on both sides, so GIVEN the kernel's three norms it is compared bit for bit.

eps = 0.5 (the usual L2 radius at this image size) wherever the ball invariant ||x - x0||_2 <= eps (1 + 4 * 2^-23) is asserted: see
tests/test_apgd_l2_host.py for why the bound, which is relative to eps, belongs to radii of that size."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import apgd_l2_reference as L2
from tiny_models import Args, TinyNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")
F = np.float32
RESIDENT = 12288


@pytest.fixture(scope="module")
def ops():
    from eeadv import ops
    return ops


def _bits(a):
    """The bit patterns, every NaN mapped to one pattern (which NaN an operation returns is the hardware's choice); everything else, signed
    zeros and denormals included, is compared as is."""
    a = np.ascontiguousarray(a)
    bits = a.view(np.uint32).copy()
    bits[np.isnan(a)] = 0x7FC00000
    return bits


# ---- the numpy restatement -------------------------------------------------------------------------------------------------------------
def _tclamp(v):
    r = np.where(v < F(0), F(0), v)
    r = np.where(r > F(1), F(1), r)
    return np.where(np.isnan(v), v, r).astype(F)


def _tmin(a, b):
    return np.where(np.isnan(a) | np.isnan(b), a + b, np.where(a < b, a, b)).astype(F)


def _rescale(eps, n):
    return (_tmin(np.full_like(n, eps), n) / (n + F(1e-12))).astype(F)


def _np_lines(x, xo, g, x0, step, eps, a, norms):
    """The element-wise lines in f32, one rounding per operation, from the three norms given [3, B].  Returns (d1, d2, x_new): the two
    vectors whose norms the kernel takes and the new iterate."""
    a, b1 = F(a), F(1) - F(a)
    ng, n1, n2 = (norms[k][:, None].astype(F) for k in range(3))
    with np.errstate(all="ignore"):
        sg = (step[:, None] / (ng + F(1e-12))).astype(F)
        z = np.where(np.isfinite(ng), x + g * sg, x).astype(F)
        d1 = (z - x0).astype(F)
        z = _tclamp(x0 + d1 * _rescale(F(eps), n1))
        m = ((x + (z - x) * a) + (x - xo) * b1).astype(F)
        d2 = (m - x0).astype(F)
        return d1, d2, _tclamp(x0 + d2 * _rescale(F(eps), n2))


def _exact_norm64(v):
    vals = [float(t) for t in v]
    return math.sqrt(math.fsum(t * t for t in vals))  # the square of a float32 is exact in a double


def _exact_norm(v):
    with np.errstate(over="ignore"):
        return F(_exact_norm64(v))


def _within_one_ulp(got, want):
    if np.isnan(want) or np.isnan(got):
        return bool(np.isnan(want) and np.isnan(got))
    return abs(int(np.array(got, F).view(np.int32)) - int(np.array(want, F).view(np.int32))) <= 1  # both are non-negative


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
KINDS = ("zero gradient", "NaN in the gradient", "inside the ball", "far outside", "generic")


def _inputs(B, P, eps, variant, seed):
    """Sample b of variant v is of kind (v * B + b) % 5, so ceil(5 / B) variants show every kind at every launch shape."""
    rng = np.random.default_rng(seed)
    x0 = rng.random((B, P), dtype=F)
    x0[:, ::7] = 0.0  # on both ends of the box: the clamp cuts there
    x0[:, 3::7] = 1.0
    x = np.clip(x0 + (rng.standard_normal((B, P)) * (0.5 * eps / math.sqrt(P))).astype(F), 0, 1).astype(F)
    xo = np.clip(x0 + (rng.standard_normal((B, P)) * (0.5 * eps / math.sqrt(P))).astype(F), 0, 1).astype(F)
    g = rng.standard_normal((B, P)).astype(F)
    g[:, 1::11] = 0.0
    step = np.array([2 * eps / 2 ** (b % 3) for b in range(B)], dtype=F)
    kinds = [(variant * B + b) % 5 for b in range(B)]
    for b, k in enumerate(kinds):
        if k == 0:
            g[b] = 0.0
            g[b, ::2] = -0.0
        elif k == 1:
            g[b, P // 2] = np.nan
            if P > 2:
                g[b, 0] = np.inf
        elif k == 2:  # a step far smaller than the room left in the ball: n1 < eps
            x[b] = np.clip(x0[b] + (np.clip(rng.standard_normal(P), -2, 2) * (0.1 * eps / math.sqrt(P))).astype(F), 0, 1)
            step[b] = F(eps / 64)
        elif k == 3:  # anywhere in the box, a large step: far outside before the rescale
            x[b] = rng.random(P, dtype=F)
            x[b, ::5] = 1.0 - x0[b, ::5]
            step[b] = F(8 * max(eps, 0.5))
    return x, xo, g, x0, step, kinds


def _launch(ops, x, xo, g, x0, step, it, eps, path, misalign=False):
    def dev(a):
        if not misalign:
            return torch.from_numpy(a).to(DEV)
        pad = torch.zeros(a.size + 1, device=DEV)  # a view one float past a 16-byte boundary
        v = pad[1:].view(a.shape)
        v.copy_(torch.from_numpy(a))
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    xd, od = dev(x), dev(xo)
    norms = ops.apgd_step_l2_(xd, od, dev(g), dev(x0), torch.from_numpy(step).to(DEV), torch.tensor([it], dtype=torch.int32, device=DEV), eps,
                              path=path)
    return xd.cpu().numpy(), od.cpu().numpy(), norms.cpu().numpy()


SHAPES = [(1, 1), (3, 3), (3, 37), (2, 192), (5, 4), (2, 2052), (1, 12288), (1, 12292)]
PATHS = ("auto", "resident", "streaming")


# ---- the kernel against numpy ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,P", SHAPES)
def test_step_kernel_against_numpy(ops, B, P):
    """Every launch shape, counter 0 and 3, every path the size allows, every kind of sample: (1) each norm within 1 ulp of the exactly
    summed one, (2) x and x_old bit for bit from the kernel's own norms, (3) all paths and the unaligned call the same bits."""
    eps = 0.5
    seen = set()
    for variant in range(-(-5 // B)):
        x, xo, g, x0, step, kinds = _inputs(B, P, eps, variant, 1000 * B + P + variant)
        seen.update(kinds)
        for it, a in ((0, 1.0), (3, 0.75)):
            outs = {}
            for path in PATHS:
                if path == "resident" and P > RESIDENT:
                    continue
                outs[path] = _launch(ops, x, xo, g, x0, step, it, eps, path)
            outs["unaligned"] = _launch(ops, x, xo, g, x0, step, it, eps, "auto", misalign=True)
            xn, on, norms = outs["auto"]
            # (3)
            for name, (xa, oa, na) in outs.items():
                assert np.array_equal(_bits(xa), _bits(xn)) and np.array_equal(_bits(oa), _bits(on)) and np.array_equal(_bits(na), _bits(norms)), \
                    (name, it, variant)
            # (2)
            d1, d2, want = _np_lines(x, xo, g, x0, step, eps, a, norms)
            assert np.array_equal(_bits(xn), _bits(want)), (it, variant, kinds)
            assert np.array_equal(_bits(on), _bits(x)), (it, variant)
            # (1): the squares of the restatement, teacher-forced on the kernel's earlier norms
            for b in range(B):
                for k, v in enumerate((g[b], d1[b], d2[b])):
                    want_n = _exact_norm(v)
                    print("B %d P %d it %d sample %d (%s) norm %d: kernel %r exact %r" % (B, P, it, b, KINDS[kinds[b]], k, norms[k, b], want_n))
                    assert _within_one_ulp(norms[k, b], want_n), (it, variant, b, k, norms[k, b], want_n)
            # what the kinds are there for
            for b, kind in enumerate(kinds):
                if kind == 0:
                    assert norms[0, b] == 0 and not np.isnan(xn[b]).any()
                if kind == 1:
                    assert np.isnan(norms[0, b]) and not np.isnan(xn[b]).any()  # no gradient step, and nothing else is NaN
                if kind == 2:
                    assert norms[1, b] < eps
                if kind == 3:
                    assert norms[1, b] > 2 * eps
                assert _exact_norm64(xn[b].astype(np.float64) - x0[b]) <= eps * (1 + 4 * 2.0 ** -23), (b, kind)
            assert xn.min() >= 0 and xn.max() <= 1
    assert seen == set(range(5))
    assert (x0 == 0).any() and ((x0 == 1).any() or P < 4)


def test_step_kernel_eps_zero(ops):
    """eps = 0: min(0, n) / (n + 1e-12) = 0, so every sample returns to x0 - the one with the NaN gradient too - and x_old takes x."""
    x, xo, g, x0, step, kinds = _inputs(5, 37, 0.0, 0, 7)
    x = np.clip(x + F(0.01), 0, 1).astype(F)
    for path in PATHS:
        xn, on, norms = _launch(ops, x, xo, g, x0, np.full(5, 0.25, F), 3, 0.0, path)
        _, _, want = _np_lines(x, xo, g, x0, np.full(5, 0.25, F), 0.0, 0.75, norms)
        assert np.array_equal(_bits(xn), _bits(want)) and np.array_equal(xn, x0) and np.array_equal(on, x)


def test_step_kernel_argument_errors(ops):
    from eeadv import _native as N
    B, P = 2, 8
    t = [torch.rand(B, P, device=DEV) for _ in range(4)]
    keep = [v.clone() for v in t]
    step, counter, norms = torch.full((B,), 0.5, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), torch.full((3, B), -1.0, device=DEV)
    big = torch.zeros(1, RESIDENT + 4, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda v: ctypes.c_void_p(v.data_ptr())  # noqa: E731
    f = N.lib.ee_apgd_step_l2_f32
    base = [p(v) for v in t] + [p(step), p(counter), p(norms)]
    eps = ctypes.c_float(0.5)
    assert f(*base, -1, P, eps, 0, stream) == -2 and f(*base, B, -1, eps, 0, stream) == -2
    assert f(*base, B, P, eps, 3, stream) == -2 and f(*base, B, P, ctypes.c_float(-1.0), 0, stream) == -2
    assert f(*[p(big)] * 4, p(step), p(counter), p(norms), 1, RESIDENT + 4, eps, 1, stream) == -3
    for k in range(7):
        args = list(base)
        args[k] = None
        assert f(*args, B, P, eps, 0, stream) == -1, k
        args[k] = ctypes.c_void_p(base[k].value + 2)
        assert f(*args, B, P, eps, 0, stream) == -4, k
    assert f(*base, 0, P, eps, 0, stream) == 0 and f(*base, B, 0, eps, 0, stream) == 0  # empty: nothing is launched
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(t, keep)) and bool((norms == -1).all()) and int(counter.item()) == 0
    with pytest.raises(N.EEError, match="ee_apgd_step_l2_f32"):
        ops.apgd_step_l2_(big, big.clone(), big.clone(), big.clone(), step[:1].contiguous(), counter, 0.5, path="resident")
    with pytest.raises(ValueError, match="path"):
        ops.apgd_step_l2_(*t, step, counter, 0.5, path="fast")
    n2 = ops.apgd_step_l2_(*t, step, counter, 0.5, norms=norms)
    assert n2 is norms and bool((norms >= 0).all()) and int(counter.item()) == 0  # the step advances nothing


# ---- the engine on TinyNet ----------------------------------------------------------------------------------------------------------------
T_B, T_HW, T_NCLS, T_EPS, T_ITER = 6, 8, 10, 0.5, 10


def _tiny_problem(seed=0):
    torch.manual_seed(seed)
    model = TinyNet(3, T_HW, T_NCLS, seed=seed).eval()
    x0 = torch.rand(T_B, 3, T_HW, T_HW)
    x0[:, :, 0, :2] = 0.0
    x0[:, :, 1, :2] = 1.0
    with torch.no_grad():
        y = model(x0).argmax(1)
    y[0] = (y[0] + 1) % T_NCLS
    x_init = L2.start(x0, T_EPS, torch.randn(T_B, 3, T_HW, T_HW))
    return model, x0, y, x_init


@pytest.fixture(scope="module")
def tiny():
    model, x0, y, x_init = _tiny_problem()
    return model.to(DEV), x0.to(DEV), y.to(DEV), x_init.to(DEV)


@pytest.mark.parametrize("kind,E", [("ce", 1), ("dlr", 1), ("dlr_t", 1), ("ce", 2)], ids=["ce", "dlr", "dlr_t", "ce-eot2"])
def test_engine_eager_equals_replay_and_the_reference(tiny, kind, E):
    """TinyNet, B = 6, 10 iterations.  Eager equals graph replay bit for bit; the eager trace is held step by step against
    tests/apgd_l2_reference.py teacher-forced on the device's gradients, losses, preds and norms: the iterates and x_old bit for bit (f32,
    one rounding per operation on both sides), the reference's own norms within 1 ulp, the flags and the result exactly, as
    tests/test_gpu_apgd.py holds the Linf step, the bookkeeping and the copies; and the result lies in the ball and the box."""
    from eeadv import engine, ops
    m, x0, y, x_init = tiny
    t = torch.fmod(y + 3, T_NCLS) if kind == "dlr_t" else None
    try:
        trace = []
        eager = engine.apgd_loop(m, x0, x_init, y, T_ITER, T_EPS, kind, t, use_graph=False, eot_iter=E, norm="L2", trace=trace)
        plain = engine.apgd_loop(m, x0, x_init, y, T_ITER, T_EPS, kind, t, use_graph=False, eot_iter=E, norm="L2")
        first = engine.apgd_loop(m, x0, x_init, y, T_ITER, T_EPS, kind, t, use_graph=True, eot_iter=E, norm="L2")
        again = engine.apgd_loop(m, x0, x_init, y, T_ITER, T_EPS, kind, t, use_graph=True, eot_iter=E, norm="L2")
    finally:
        engine.clear_graphs()
    for other in (plain, first, again):
        assert all(torch.equal(p, q) for p, q in zip(eager, other))
    steps = [e for e in trace if "step_g" in e]
    evals = [e for e in trace if "draws" in e]
    assert len(steps) == T_ITER and len(evals) == T_ITER + 1 and [e["counter"] for e in steps] == list(range(T_ITER))
    forced = [dict(loss=e["book_loss"].cpu(), g=e["g_mean"].cpu(), pred=e["book_pred"].cpu().bool()) for e in evals]
    for f, s in zip(forced[1:], steps):
        f["norms"] = s["norms"].cpu()
    want_x, want_r, want_l, want = L2.run(None, x0.cpu(), x_init.cpu(), y.cpu(), T_ITER, T_EPS, kind, None, forced)
    for i, (s, e, w) in enumerate(zip(steps, evals[1:], want[1:])):
        assert torch.equal(s["x_in"].cpu(), want[i]["x"]) and torch.equal(s["x_old_in"].cpu(), want[i]["x_old"]), i
        assert torch.equal(s["step_g"].cpu(), want[i]["g"]) and torch.equal(s["step"].cpu(), want[i]["step"]), i
        assert torch.equal(s["x"].cpu(), w["x_new"]) and torch.equal(s["x_old"].cpu(), w["x_old"]), i
        got_n, own_n = s["norms"].cpu().numpy(), w["norms"].numpy()
        assert all(_within_one_ulp(got_n[k, b], own_n[k, b]) for k in range(3) for b in range(T_B)), (i, got_n, own_n)
        flags = e["flags"].cpu()
        assert (flags & ops.APGD_IMPROVED).bool().tolist() == w["improved"] and (flags & ops.APGD_FOOLED).bool().tolist() == w["fooled"], i
        assert (flags & ops.APGD_REDUCED).bool().tolist() == w["reduced"], i
    assert torch.equal(eager[0].cpu(), want_x) and torch.equal(eager[1].cpu(), want_r) and torch.equal(eager[2].cpu(), want_l)
    assert any(any(w["reduced"]) for w in want[1:]) and not bool(eager[1][0])
    xa = eager[0].cpu()
    assert L2.ball_excess(xa, x0.cpu(), T_EPS) <= 4 * 2.0 ** -23 and bool((xa >= 0).all()) and bool((xa <= 1).all())


def test_linf_route_is_unchanged_and_l2_is_one_more_graph(tiny, ops, monkeypatch):
    """norm="Linf" through apgd_loop is the call without `norm`, byte for byte, eager and replayed, on the same captured graph, with no
    `norms` buffer and no L2 launch; the L2 run adds exactly one entry to the capture cache."""
    from eeadv import engine
    m, x0, y, x_init = tiny
    eps = 0.03
    x_lin = torch.clamp(torch.min(torch.max(x_init, x0 - eps), x0 + eps), 0, 1)
    calls = []
    real = ops.apgd_step_l2_
    monkeypatch.setattr(ops, "apgd_step_l2_", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    try:
        for graph in (False, True):
            a = engine.apgd_loop(m, x0, x_lin, y, T_ITER, eps, "ce", use_graph=graph)
            b = engine.apgd_loop(m, x0, x_lin, y, T_ITER, eps, "ce", use_graph=graph, norm="Linf")
            assert all(torch.equal(p, q) for p, q in zip(a, b)) and not calls
        keys = [k for k in engine._GRAPHS if k[0] == "apgd"]
        assert len(keys) == 1 and "Linf" in keys[0] and engine._GRAPHS[keys[0]].run.norms is None
        c = engine.apgd_loop(m, x0, x_lin, y, T_ITER, eps, "ce", use_graph=True, norm="L2")
        keys = [k for k in engine._GRAPHS if k[0] == "apgd"]
        assert len(keys) == 2 and sorted(k[5] for k in keys) == ["L2", "Linf"] and calls
        assert not torch.equal(a[0], c[0])
        assert tuple(engine._GRAPHS[[k for k in keys if "L2" in k][0]].run.norms.shape) == (3, T_B)
        with pytest.raises(ValueError, match="norm"):
            engine.apgd_loop(m, x0, x_lin, y, T_ITER, eps, "ce", norm="L1")
    finally:
        engine.clear_graphs()


# ---- the randomised ResNet ------------------------------------------------------------------------------------------------------------------
def test_resnet18_ee_square_eager_equals_replay(monkeypatch):
    """resnet18_EE_square, B = 4, 3 x 64 x 64 (per-sample size 12288: the resident path), eval mode, 5 iterations, every gradient the mean
    of 2 draws.  With the device draw state rewound before each run, eager and replay give the same bits."""
    import utils.attacks as A
    from eeadv import engine, models, runtime
    torch.manual_seed(5)
    m = models.make_resnet_ee(18, "tiny", True, cize=64, r=8, w=1.0, with_gf=False, low=38.0, high=76.0, alpha=0.0, sigma=1.0,
                              type_canny="CannyFilter_step125_1", epsilon=16 / 255, n_queries=1).to(DEV).eval()
    eps, n_iter, E = 0.5, 5, 2
    g = torch.Generator().manual_seed(1)
    x = torch.rand(4, 3, 64, 64, generator=g).to(DEV)
    noise = torch.randn(4, 3, 64, 64, generator=g).to(DEV)
    runtime.reseed()
    torch.manual_seed(9)
    state = runtime.draw_state(torch.device(DEV))
    with torch.no_grad():
        y = m(x).argmax(1)
    y[0] = (y[0] + 1) % 200
    args = Args(epsilon=eps)

    def attack(graph):
        monkeypatch.setenv("EEADV_GRAPH", "1" if graph else "0")
        state.copy_(state0)
        return A.APGD(m, args, x, y, n_iter, "ce", noise=noise, eot_iter=E, norm="L2")

    try:
        state0 = state.clone()
        attack(True)  # builds the graph (the warm-up passes draw too)
        state0 = state.clone()
        (xe, re_), (xg, rg) = attack(False), attack(True)
    finally:
        engine.clear_graphs()
    assert torch.equal(xe, xg) and torch.equal(re_, rg) and not bool(re_[0])
    assert torch.equal(xe[re_], x[re_]) and bool((xe[~re_] != x[~re_]).flatten(1).any(1).all())
    assert L2.ball_excess(xe.cpu(), x.cpu(), eps) <= 4 * 2.0 ** -23 and bool((xe >= 0).all()) and bool((xe <= 1).all())


# ---- the doors ---------------------------------------------------------------------------------------------------------------------------------
def test_apgd_t_and_apgd_rand_in_l2(tiny, monkeypatch):
    """APGD_T and APGD_Rand hand `norm` to every run: each equals its runs made one by one through APGD(norm="L2"), combined as the Linf
    composites combine them, eager and replayed; the results lie in the L2 ball."""
    import utils.attacks as A
    from eeadv import engine, ops as O
    m, x0, y, _ = tiny
    a = Args(epsilon=T_EPS)
    noise = torch.randn(x0.shape, generator=torch.Generator().manual_seed(4)).to(DEV)
    order = O.topk(m(x0).detach().float().contiguous(), None, 3)[0]
    shape = (-1, 1, 1, 1)
    try:
        for graph in ("0", "1"):
            monkeypatch.setenv("EEADV_GRAPH", graph)
            xt, rt = A.APGD_T(m, a, x0, y, T_ITER, T_NCLS, n_target_classes=2, noise=noise, norm="L2")
            runs = [A.APGD(m, a, x0, y, T_ITER, "dlr_t", order[:, j].contiguous(), noise, norm="L2") for j in (1, 2)]
            want_r = runs[0][1] & runs[1][1]
            want_x = torch.where((runs[0][1] & ~runs[1][1]).view(shape), runs[1][0], runs[0][0])
            assert torch.equal(xt, want_x) and torch.equal(rt, want_r)
            xr, rr = A.APGD_Rand(m, a, x0, y, T_ITER, 2, noise=noise, norm="L2")
            ce = A.APGD(m, a, x0, y, T_ITER, "ce", noise=noise, eot_iter=2, norm="L2")
            dlr = A.APGD(m, a, x0, y, T_ITER, "dlr", noise=noise, eot_iter=2, norm="L2")
            assert torch.equal(rr, ce[1] & dlr[1]) and torch.equal(xr, torch.where((ce[1] & ~dlr[1]).view(shape), dlr[0], ce[0]))
            for xa in (xt, xr):
                assert L2.ball_excess(xa.cpu(), x0.cpu(), T_EPS) <= 4 * 2.0 ** -23 and bool((xa >= 0).all()) and bool((xa <= 1).all())
            lin = A.APGD_T(m, a, x0, y, T_ITER, T_NCLS, n_target_classes=2, noise=noise * 0.1)
            assert not torch.equal(lin[0], xt)
    finally:
        engine.clear_graphs()


def test_tiny_imagenet_driver_evaluates_with_apgd_ce_in_l2(tmp_path):
    cfg = open(os.path.join(PKG, "Tiny_ImageNet", "configs_tinyimagenet", "adversarial_training.yml")).read()
    cfg = re.sub(r"num_steps_(\d): \d+", r"num_steps_\1: 2", cfg).replace("batch_size: 100", "batch_size: 8").replace("print_freq: 50", "print_freq: 1")
    path = tmp_path / "l2.yml"
    path.write_text(cfg)
    r = subprocess.run([sys.executable, "experiments_tinyimagenet.py", "-c", str(path), "--output-root", str(tmp_path), "--data", "synthetic:1:1",
                        "-e", "--attack_method", "APGD-CE", "--norm", "L2"], cwd=os.path.join(PKG, "Tiny_ImageNet"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    logs = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path)) for f in fs if f.startswith("log")]
    text = r.stdout + "".join(open(f).read() for f in logs)
    clean = re.findall(r"^ \* Clean Prec@1 ([\d.]+) Prec@5 ([\d.]+)$", text, flags=re.M)
    adv = re.findall(r"^ \* Adv Prec@1 ([\d.]+) Prec@5 ([\d.]+) \[norm L2\]$", text, flags=re.M)
    assert len(clean) >= 3 and len(clean) == len(adv)
    for (c1, _), (a1, _) in zip(clean, adv):
        assert float(a1) <= float(c1)


def test_cascade_rand_in_l2_device_pools_equal_the_torch_staging():
    """A deterministic TinyNet, a split of 3 batches of 4, rand_stages(norm="L2") with E = 2, eager: what the HIP pools give equals what the
    torch staging gives, bit for bit, and APGD-DLR ran on the survivors of APGD-CE only."""
    from eeadv import cascade, engine
    torch.manual_seed(3)
    m = TinyNet(3, 8, 10, 5).eval()
    xs = torch.rand(12, 3, 8, 8)
    with torch.no_grad():
        ys = m(xs).argmax(1)
    ys[5] = (ys[5] + 1) % 10
    m, xs, ys = m.to(DEV), xs.to(DEV), ys.to(DEV)
    a = Args(epsilon=0.1, eot_iter=2)
    batches = [(xs[i:i + 4], ys[i:i + 4]) for i in (0, 4, 8)]
    runs = {}
    try:
        for mode in ("hip", "torch"):
            torch.manual_seed(100)
            runs[mode] = cascade.evaluate(m, a, batches, 10, compaction=mode, stages=cascade.rand_stages(a, 5, norm="L2"), keep_adv=True)
    finally:
        engine.clear_graphs()
    h, t = runs["hip"], runs["torch"]
    print("rows_attacked %s robust_after %s" % (h.rows_attacked, h.robust_after))
    assert h.stage_names == ["APGD-CE", "APGD-DLR"] and h.n == 12 and h.clean_correct == 11 and int(h.stage[5]) == 0
    assert torch.equal(h.robust, t.robust) and torch.equal(h.stage, t.stage) and torch.equal(h.adv.view(torch.int32), t.adv.view(torch.int32))
    assert h.rows_attacked == t.rows_attacked and h.robust_after == t.robust_after and h.batches_attacked == t.batches_attacked
    assert h.rows_attacked == [h.clean_correct, h.robust_after[0]]
    assert L2.ball_excess(h.adv.cpu(), xs.cpu(), 0.1) <= 4 * 2.0 ** -23 * 5  # eps = 0.1: the absolute rounding term weighs 5 times more than at 0.5
