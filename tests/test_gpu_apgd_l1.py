"""GPU: APGD in the L1 threat model - ee_l1_proj_f32, ee_apgd_step_l1_f32 and ee_apgd_book_l1_f32 through the C ABI against
tests/apgd_l1_reference.py on the same f32 inputs, then the engine (eager trace teacher-forced, graph replay) and the Python door.

What is held: tau, m, j, |A| and the nonzero counts exactly; lambda within 1 ulp of the reference's float64 value rounded to f32 (the
kernel sums in double in a fixed order, the reference exactly: the two quotients round to the same float or to neighbours); given the
kernel's own lambda and tau, every written element bit for bit; resident, streaming and the misaligned element-wise call the same bits."""
import ctypes
import math

import numpy as np
import pytest
import torch

import apgd_l1_reference as L1
from tiny_models import Args, TinyNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
RESIDENT = 12288
PATHS = ("auto", "resident", "streaming")


@pytest.fixture(scope="module")
def ops():
    from eeadv import ops
    return ops


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _within_one_ulp(got, want):
    got, want = F(got), F(want)
    return got == want or got == np.nextafter(want, F(np.inf)) or got == np.nextafter(want, F(-np.inf))


def _dev(a, misalign=False):
    if not misalign:
        return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    pad = torch.zeros(a.size + 1, device=DEV)  # a view one float past a 16-byte boundary
    v = pad[1:].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _step(ops, x, g, x0, step, topk, eps, path, misalign=False):
    xd = _dev(x, misalign)
    scal = ops.apgd_step_l1_(xd, _dev(g, misalign), _dev(x0, misalign), _dev(step), _dev(topk), eps, path=path)
    return xd.cpu().numpy(), scal.cpu().numpy()


def _proj(ops, u, x0, eps, path, misalign=False):
    z, scal = ops.l1_proj(_dev(u, misalign), _dev(x0, misalign), eps, path=path)
    return z.cpu().numpy(), scal.cpu().numpy()


def _all_paths(fn, P):
    outs = {p: fn(p, False) for p in PATHS if not (p == "resident" and P > RESIDENT)}
    outs["unaligned"] = fn("auto", True)
    ref = outs["auto"]
    for name, o in outs.items():
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(o, ref)), name
    return ref


def _inputs(B, P, seed):
    """x0 with both ends of the box, x a point near it, a gradient with exact zeros, per-sample step and topk.  Sample b of variant v is
    'inside' (a short step from a point close to x0: the ball is inactive) when (b + v) is odd, else 'outside'."""
    r = np.random.RandomState(seed)
    x0 = r.rand(B, P).astype(F)
    x0[:, ::5] = 0.0
    x0[:, 1::7] = 1.0
    g = r.randn(B, P).astype(F)
    g[:, ::3] = 0.0 if P > 3 else g[:, ::3]
    topk = (0.05 + 0.5 * r.rand(B)).astype(F)
    return x0, g, topk, r


SIZES = [1, 3, 5, 64, 2052, 12288, 12292]


def _cases(B, P):
    """Two variants of (x, g, x0, step, topk) and eps for a shape, chosen on the CPU: the first seed at which the reference alone shows
    lambda > 0 and lambda = 0 both occurring over the 2 B samples.  No shape is exempt: at P = 1 (x0 = 0) the ball is active when the
    one coordinate has x > 0 and g > 0 and steps by eps."""
    eps = float(F(max(0.5, P / 256.0)))
    for attempt in range(50):
        out, lams = [], []
        for variant in range(2):
            x0, g, topk, r = _inputs(B, P, 1000 * attempt + 100 * P + 10 * B + variant)
            inside = np.array([(b + variant) % 2 == 1 for b in range(B)])
            spread = np.where(inside, 0.05 * eps / P, 2.0 * eps / P).astype(F)
            x = np.clip(x0 + spread[:, None] * r.randn(B, P).astype(F), 0, 1).astype(F)
            x = np.stack([L1.project_row(x[b], x0[b], eps)[0] for b in range(B)])
            step = np.where(inside, eps / 10, eps).astype(F)
            own = [L1.step_row(x[b], g[b], x0[b], step[b], topk[b], eps)[1] for b in range(B)]
            lams += [o["lam"] for o in own]
            out.append((x, g, x0, step, topk, own))
        if any(v > 0 for v in lams) and any(v == 0 for v in lams):
            return eps, out
    raise AssertionError("no seed shows both branches for B %d P %d" % (B, P))


@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("B", [1, 3])
def test_step_kernel_against_the_reference(ops, B, P):
    eps, cases = _cases(B, P)
    for variant, (x, g, x0, step, topk, owns) in enumerate(cases):
        xn, scal = _all_paths(lambda p, mis: _step(ops, x, g, x0, step, topk, eps, p, mis), P)
        for b in range(B):
            own = owns[b]
            print("B %d P %d v %d b %d: lam %r (ref %r) tau %r m %r j %r |A| %r h0 %r dist %r" % (
                B, P, variant, b, scal[0, b], own["lam"], scal[4, b], scal[5, b], scal[6, b], scal[2, b], scal[1, b], scal[3, b]))
            assert _bits(scal[4, b]) == _bits(own["tau"]) and int(scal[5, b]) == own["m"] and int(scal[6, b]) == own["j"], b
            assert int(scal[2, b]) == own["active"], (b, scal[2, b], own["active"])
            assert _within_one_ulp(scal[0, b], own["lam"]), (b, scal[0, b], own["lam"])
            assert (scal[0, b] > 0) == (own["lam"] > 0)
            assert _within_one_ulp(scal[1, b], own["h0"]), (b, scal[1, b], own["h0"])
            want, _ = L1.step_row(x[b], g[b], x0[b], step[b], topk[b], eps, lam=scal[0, b], tau=scal[4, b])
            assert np.array_equal(_bits(xn[b]), _bits(want)), b
            assert xn[b].min() >= 0 and xn[b].max() <= 1
            assert L1.l1_excess(xn[b:b + 1], x0[b:b + 1], eps) <= P * 2.0 ** -23
            assert _within_one_ulp(scal[3, b], math.fsum(np.abs(xn[b].astype(np.float64) - x0[b]).tolist()))


@pytest.mark.parametrize("P", SIZES)
def test_projection_kernel_far_outside_the_box(ops, P):
    """u = x0 + n, n standard normal (the start of a run): most coordinates leave the box.  Ball active (eps small) and inactive."""
    B = 3
    r = np.random.RandomState(P)
    x0 = r.rand(B, P).astype(F)
    x0[:, ::4] = 0.0
    x0[:, 1::4] = 1.0
    u = (x0 + 3 * r.randn(B, P)).astype(F)
    for eps in (float(F(P / 64.0)), float(4 * P)):
        z, scal = _all_paths(lambda p, mis: _proj(ops, u, x0, eps, p, mis), P)
        for b in range(B):
            _, own = L1.project_row(u[b], x0[b], eps)
            assert int(scal[2, b]) == own["active"] and _within_one_ulp(scal[0, b], own["lam"]), (eps, b, scal[:, b], own)
            want, _ = L1.project_row(u[b], x0[b], eps, lam=scal[0, b])
            assert np.array_equal(_bits(z[b]), _bits(want)), (eps, b)
            assert (scal[0, b] > 0) == (own["lam"] > 0)
            assert P < 3 or (own["lam"] > 0) == (eps < P)  # a single coordinate at a box end is held by the box alone
        assert z.min() >= 0 and z.max() <= 1 and L1.l1_excess(z, x0, eps) <= P * 2.0 ** -23
    assert np.array_equal(_bits(scal[4:]), _bits(np.zeros((3, B), F)))  # the projection alone leaves the step's rows


def test_resident_past_its_limit_and_argument_errors(ops):
    from eeadv import _native as N
    B, P = 2, 8
    t = [torch.rand(B, P, device=DEV) for _ in range(3)]
    keep = [v.clone() for v in t]
    step, topk = torch.full((B,), 0.5, device=DEV), torch.full((B,), 0.2, device=DEV)
    scal = torch.full((7, B), -1.0, device=DEV)
    big = torch.zeros(1, RESIDENT + 4, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda v: ctypes.c_void_p(v.data_ptr())  # noqa: E731
    eps = ctypes.c_float(0.5)
    f = N.lib.ee_apgd_step_l1_f32
    base = [p(v) for v in t] + [p(step), p(topk), p(scal)]
    assert f(*base, -1, P, eps, 0, stream) == -2 and f(*base, B, -1, eps, 0, stream) == -2
    assert f(*base, B, P, eps, 3, stream) == -2 and f(*base, B, P, ctypes.c_float(-1.0), 0, stream) == -2
    assert f(*base, B, P, ctypes.c_float(float("nan")), 0, stream) == -2
    assert f(*base, 1, 2 ** 31 - 2048, eps, 2, stream) == -2  # a pass counts per_sample plus its padded slots in an int
    assert f(*[p(big)] * 3, p(step), p(topk), p(scal), 1, RESIDENT + 4, eps, 1, stream) == -3
    for k in range(6):
        args = list(base)
        args[k] = None
        assert f(*args, B, P, eps, 0, stream) == -1, k
        args[k] = ctypes.c_void_p(base[k].value + 2)
        assert f(*args, B, P, eps, 0, stream) == -4, k
    assert f(*base, 0, P, eps, 0, stream) == 0 and f(*base, B, 0, eps, 0, stream) == 0  # empty: nothing is launched
    fp = N.lib.ee_l1_proj_f32
    assert fp(p(t[0]), p(t[1]), p(t[2]), p(scal), 0, P, eps, 0, stream) == 0
    assert fp(p(big), p(big), p(big), p(scal), 1, RESIDENT + 4, eps, 1, stream) == -3
    assert fp(p(t[0]), p(t[1]), p(t[2]), p(scal), B, P, eps, 5, stream) == -2
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(t, keep)) and bool((scal == -1).all())
    with pytest.raises(N.EEError, match="ee_apgd_step_l1_f32"):
        ops.apgd_step_l1_(big, big.clone(), big.clone(), step[:1].contiguous(), topk[:1].contiguous(), 0.5, path="resident")
    with pytest.raises(ValueError, match="path"):
        ops.apgd_step_l1_(*t, step, topk, 0.5, path="fast")
    e = torch.zeros(0, 8, device=DEV)
    z, _ = ops.l1_proj(e, e.clone(), 0.5)
    assert z.shape == (0, 8)


def test_edge_inputs(ops):
    """Sample 0: an all-zero gradient; 1: ties at tau; 2: a NaN; 3: an Inf in the gradient; 4: generic."""
    B, P, eps = 5, 37, 1.0
    x0, g, topk, r = _inputs(B, P, 5)
    x = np.clip(x0 + 0.01 * r.randn(B, P), 0, 1).astype(F)
    g[0] = 0.0
    g[1] = np.sign(r.randn(P)).astype(F) * F(0.25)
    g[2, 4] = np.nan
    g[3, 6] = -np.inf
    step = np.full(B, eps, F)
    xn, scal = _all_paths(lambda p, mis: _step(ops, x, g, x0, step, topk, eps, p, mis), P)
    assert not np.isnan(xn).any() and not np.isnan(scal[[0, 1, 2, 3, 5, 6]]).any()
    assert scal[5, 0] == 0 and np.array_equal(xn[0], x[0])  # nothing moves: x was feasible
    assert scal[5, 1] == P and scal[4, 1] == F(0.25)  # ties are all in
    for b in (2, 3):  # no gradient step; the projection of the feasible x is x
        assert np.array_equal(xn[b], x[b]) and scal[0, b] == 0
    for b in range(B):
        _, own = L1.step_row(x[b], g[b], x0[b], step[b], topk[b], eps)
        assert int(scal[5, b]) == own["m"] and int(scal[6, b]) == own["j"] and _bits(scal[4, b]) == _bits(own["tau"]), b
        want, _ = L1.step_row(x[b], g[b], x0[b], step[b], topk[b], eps, lam=scal[0, b], tau=scal[4, b])
        assert np.array_equal(_bits(xn[b]), _bits(want)), b
        assert (scal[0, b] > 0) == (own["lam"] > 0) and _within_one_ulp(scal[0, b], own["lam"]) and int(scal[2, b]) == own["active"], b
    # eps = 0 returns x0 exactly, from the step and from the projection
    z0, s0 = _all_paths(lambda p, mis: _step(ops, x, g, x0, step, topk, 0.0, p, mis), P)
    assert np.array_equal(_bits(z0), _bits(x0)) and (s0[3] == 0).all()
    u = (x0 + r.randn(B, P)).astype(F)
    z1, _ = _all_paths(lambda p, mis: _proj(ops, u, x0, 0.0, p, mis), P)
    assert np.array_equal(_bits(z1), _bits(x0))
    # a non-finite u is written as x0; the other samples are projected as usual
    u[1, 3] = np.inf
    u[2, 0] = np.nan
    z2, s2 = _all_paths(lambda p, mis: _proj(ops, u, x0, eps, p, mis), P)
    assert np.array_equal(z2[1], x0[1]) and np.array_equal(z2[2], x0[2]) and np.isinf(s2[1, 1]) and not np.isnan(z2).any()
    want, _ = L1.project_row(u[0], x0[0], eps, lam=s2[0, 0])
    assert np.array_equal(_bits(z2[0]), _bits(want))


@pytest.mark.parametrize("P", [5, 2052, 12292])
def test_book_kernel_counts_and_rule(ops, P):
    """A checkpoint iteration and a plain one: the nonzero count of improved ? x : x_best, the rule, the flags."""
    B, eps = 4, 2.0
    r = np.random.RandomState(P)
    x0 = r.rand(B, P).astype(F)
    x, xb = x0.copy(), x0.copy()
    for b in range(B):
        x[b, r.rand(P) < 0.2 + 0.2 * b] += F(0.125)
        xb[b, r.rand(P) < 0.5] -= F(0.125)
    loss = np.array([1.0, 0.0, 2.0, np.nan], F)
    best = np.array([0.5, 0.5, 2.0, 0.0], F)
    pred = np.array([1, 0, 1, 0], np.int32)
    sp_old = np.array([P, max(1, P // 8), 0, P], np.int32)
    step0 = np.array([eps, eps / 3, eps / 9, eps], F)
    for it, k in ((0, 0), (1, 2)):
        fstate = torch.zeros(4, B, device=DEV)
        fstate[ops.APGD_F_STEP] = _dev(step0)
        fstate[ops.APGD_F_LOSS_BEST] = _dev(best)
        istate = torch.zeros(4, B, dtype=torch.int32, device=DEV)
        istate[ops.APGD_I_ROBUST] = 1
        topk = torch.full((B,), 0.2, device=DEV)
        sps = torch.zeros(2, B, dtype=torch.int32, device=DEV)
        sps[0] = _dev(sp_old)
        sched = torch.tensor([0, 2, 0], dtype=torch.int32, device=DEV)
        flags = ops.apgd_book_l1_(_dev(loss), _dev(pred), _dev(x), _dev(xb), _dev(x0), fstate, istate, topk, sps,
                                  torch.tensor([it], dtype=torch.int32, device=DEV), sched, eps).cpu().numpy()
        improved = loss > best
        assert ((flags & ops.APGD_IMPROVED) != 0).tolist() == improved.tolist() and ((flags & ops.APGD_FOOLED) != 0).tolist() == (pred == 0).tolist()
        assert istate[ops.APGD_I_ROBUST].cpu().tolist() == pred.tolist()
        assert np.array_equal(_bits(fstate[ops.APGD_F_LOSS_BEST].cpu().numpy()), _bits(np.where(improved, loss, best)))
        if not k:
            assert not (flags & ops.APGD_REDUCED).any() and sps.cpu().tolist() == [sp_old.tolist(), [0] * B]
            assert np.array_equal(fstate[ops.APGD_F_STEP].cpu().numpy(), step0) and bool((topk == 0.2).all())
            continue
        for b in range(B):
            sp = L1.nonzero(x[b] if improved[b] else xb[b], x0[b])
            red, tk, st = L1.checkpoint(sp, sp_old[b], step0[b], eps, P, F)
            assert sps[:, b].cpu().tolist() == [sp, sp] and bool(flags[b] & ops.APGD_REDUCED) == red, b
            assert _bits(topk[b].cpu().numpy()) == _bits(tk) and _bits(fstate[ops.APGD_F_STEP, b].cpu().numpy()) == _bits(st), b


# ---- the engine on TinyNet (the model and shape of tests/test_gpu_apgd_l2.py) ---------------------------------------------------------
T_B, T_HW, T_NCLS, T_EPS, T_ITER = 6, 8, 10, 6.0, 40  # apgd_l1_schedule(40): checkpoints close iterations 0, 2, 4, ...


def _tiny_problem(seed=0):
    torch.manual_seed(seed)
    model = TinyNet(3, T_HW, T_NCLS, seed=seed).eval()
    x0 = torch.rand(T_B, 3, T_HW, T_HW)
    x0[:, :, 0, :2] = 0.0
    x0[:, :, 1, :2] = 1.0
    with torch.no_grad():
        y = model(x0).argmax(1)
    y[0] = (y[0] + 1) % T_NCLS
    return model, x0, y, x0 + torch.randn(T_B, 3, T_HW, T_HW)


@pytest.fixture(scope="module")
def tiny():
    model, x0, y, x_init = _tiny_problem()
    return model.to(DEV), x0.to(DEV), y.to(DEV), x_init.to(DEV)


N_ENGINE = 8  # two checkpoints and more: apgd_l1_schedule(8) closes every iteration


@pytest.mark.parametrize("kind", ["ce", "dlr_t"])
def test_engine_eager_equals_replay_and_the_reference(tiny, kind):
    from eeadv import engine, ops
    m, x0, y, x_init = tiny
    t = torch.fmod(y + 3, T_NCLS) if kind == "dlr_t" else None
    assert sum(1 for k in engine.apgd_l1_schedule(N_ENGINE) if k) >= 2
    try:
        trace = []
        eager = engine.apgd_l1_loop(m, x0, x_init, y, N_ENGINE, T_EPS, kind, t, use_graph=False, trace=trace)
        stream = engine.apgd_l1_loop(m, x0, x_init, y, N_ENGINE, T_EPS, kind, t, use_graph=False, path="streaming")
        first = engine.apgd_l1_loop(m, x0, x_init, y, N_ENGINE, T_EPS, kind, t, use_graph=True)
        again = engine.apgd_l1_loop(m, x0, x_init, y, N_ENGINE, T_EPS, kind, t, use_graph=True)
    finally:
        engine.clear_graphs()
    for other in (stream, first, again):
        assert all(torch.equal(p, q) for p, q in zip(eager, other))
    assert len(trace) == N_ENGINE + 1 and trace[0]["start"] and [e["counter"] for e in trace[1:]] == list(range(N_ENGINE))
    forced = [dict(loss=e["loss"].cpu().numpy(), g=e["g"].cpu().numpy(), pred=e["pred"].cpu().numpy() != 0,
                   lam=e["scal"][ops.L1_S_LAMBDA].cpu().numpy()) for e in trace]
    for f, e in zip(forced[1:], trace[1:]):
        f["tau"] = e["scal"][ops.L1_S_TAU].cpu().numpy()
    want_x, want_r, want_l, want = L1.run(None, x0.cpu(), x_init.cpu(), y.cpu(), N_ENGINE, T_EPS, kind, None, forced)
    flat = lambda v: v.cpu().numpy().reshape(T_B, -1)  # noqa: E731
    assert np.array_equal(_bits(flat(trace[0]["x"])), _bits(want[0]["x"]))
    reds = []
    for i, (e, w) in enumerate(zip(trace[1:], want[1:])):
        assert np.array_equal(_bits(flat(e["x_in"])), _bits(want[i]["x"])) and np.array_equal(_bits(flat(e["step_g"])), _bits(want[i]["g"])), i
        assert np.array_equal(_bits(flat(e["x"])), _bits(w["x_new"])), i
        for b in range(T_B):
            own = w["infos"][b]
            sc = e["scal"][:, b].cpu().numpy()
            assert int(sc[5]) == own["m"] and int(sc[6]) == own["j"] and int(sc[2]) == own["active"] and _bits(sc[4]) == _bits(own["tau"]), (i, b)
            assert _within_one_ulp(sc[0], own["lam"]), (i, b, sc[0], own["lam"])
        flags = e["flags"].cpu().numpy()
        assert ((flags & ops.APGD_IMPROVED) != 0).tolist() == w["improved"].tolist() and ((flags & ops.APGD_FOOLED) != 0).tolist() == w["fooled"].tolist(), i
        assert ((flags & ops.APGD_REDUCED) != 0).tolist() == w["reduced"].tolist(), i
        assert e["sp"].cpu().tolist() == w["sp"].tolist() and e["sp_old"].cpu().tolist() == w["sp_old"].tolist(), i
        assert np.array_equal(_bits(e["step"].cpu().numpy()), _bits(w["step"])) and np.array_equal(_bits(e["topk"].cpu().numpy()), _bits(w["topk"])), i
        assert np.array_equal(_bits(flat(e["x_out"])), _bits(w["x"])) and np.array_equal(_bits(flat(e["x_best"])), _bits(w["x_best"])), i
        reds.extend(w["reduced"].tolist())
    assert np.array_equal(_bits(eager[0].cpu().numpy()), _bits(want_x)) and eager[1].cpu().tolist() == want_r.tolist()
    assert np.array_equal(_bits(eager[2].cpu().numpy()), _bits(want_l))
    assert any(reds) and not all(reds), "the checkpoints took one branch only"
    xa = eager[0].cpu().numpy()
    assert xa.min() >= 0 and xa.max() <= 1 and L1.l1_excess(xa.reshape(T_B, -1), flat(x0), T_EPS) <= 192 * 2.0 ** -23


def test_apgd_l1_door_on_the_device(tiny):
    import utils.attacks as A
    m, x0, y, x_init = tiny
    noise = x_init - x0
    xa, rb = A.APGD_L1(m, Args(epsilon=T_EPS), x0, y, T_ITER, noise=noise)
    xn, x0n = xa.cpu().numpy().reshape(T_B, -1), x0.cpu().numpy().reshape(T_B, -1)
    assert xn.min() >= 0 and xn.max() <= 1 and L1.l1_excess(xn, x0n, T_EPS) <= 192 * 2.0 ** -23
    with torch.no_grad():
        ok = m(xa).argmax(1) == y
    assert not bool(rb[0]) and torch.equal(ok | rb, rb) and bool((~rb).any())  # a sample reported fooled is misclassified at x_adv
    assert torch.equal(ok[~rb], torch.zeros_like(ok[~rb])) and torch.equal(xa[rb], x0[rb])
    xt, rt = A.APGD_T_L1(m, Args(epsilon=T_EPS), x0, y, 8, T_NCLS, n_target_classes=2, noise=noise)
    assert xt.shape == x0.shape and rt.dtype == torch.bool
    assert L1.l1_excess(xt.cpu().numpy().reshape(T_B, -1), x0n, T_EPS) <= 192 * 2.0 ** -23
    with pytest.raises(ValueError, match="norm"):
        A.APGD(m, Args(epsilon=T_EPS), x0, y, 2, norm="L1")
