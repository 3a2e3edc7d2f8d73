"""GPU: APGD restarts - ee_apgd_start_f32 and ee_apgd_merge_f32 through ops.apgd_start_ / ops.apgd_merge_, and the
restart loop of engine.apgd_loop / apgd_l1_loop.

Bit-exact: the start launch on dyadic inputs against the numpy float32 restatement of its operation order (tests/apgd_start_reference.py),
its four instantiations against each other, the in-kernel uniform draws against eeadv.apgdstart.draw, the merge launch against its numpy
restatement, eager against graph replay, one restart against the call without the argument, a 3-restart run against three runs from the
same starts.  In tolerance: generic L2 noise (the row equals the restatement for n or one of its two float neighbours) and the in-kernel
normal draws (the bound derived at test_in_kernel_normal_draws)."""
import math

import numpy as np
import pytest
import torch

import apgd_start_reference as S
from tiny_models import TinyNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
METRICS = ("Linf", "L2", "L1")
SIZES = (1, 3, 5, 75, 192, 1023, 2049, 4100)  # the last two give a thread more than one group of four
U24 = 2.0 ** -24
EPS_DYADIC = 0.125


@pytest.fixture(scope="module")
def ops():
    from eeadv import ops
    return ops


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _odd(t):
    """The same values at an address 4 bytes past a 16-byte boundary: the kernel then takes its element-wise accesses."""
    pad = torch.zeros(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = pad[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _run_start(ops, x0, eps, metric, noise=None, seed=0, path="auto", odd=False):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    x0d, nd = dev(x0), (None if noise is None else dev(noise))
    x = torch.full(x0.shape, 7.0, device=DEV)  # garbage: every element must be written
    if odd:
        x0d, x = _odd(x0d), _odd(x)
        nd = None if nd is None else _odd(nd)
    ops.apgd_start_(x, x0d, eps, metric, seed=seed, noise=nd, path=path)
    return x.cpu().numpy()


def _dyadic(B, D, seed):
    """Multiples of 2^-8: every double sum of t_i^2 is exact in any order."""
    rng = np.random.default_rng(seed)
    t = (rng.integers(-512, 513, (B, D)) / 256.0).astype(F32)
    x0 = (rng.integers(0, 257, (B, D)) / 256.0).astype(F32)
    if B > 1:
        x0[1] = np.where(rng.random(D) < 0.5, 0.0, 1.0).astype(F32)  # a row on the faces of the box
    if B > 2:
        t[2] = 0.0  # n = 0: s = eps / 1e-12, t * s = 0, the row is x0
    return x0, t


def _generic(B, D, seed=5):
    rng = np.random.default_rng(seed)
    return rng.random((B, D)).astype(F32), rng.standard_normal((B, D)).astype(F32)


# ---- the start launch --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("D", SIZES)
@pytest.mark.parametrize("B", (1, 3, 7))
def test_start_kernel_bit_exact_in_all_instantiations(ops, B, D, metric):
    """Dyadic inputs, eps = 0.125: the float32 restatement in the kernel's order gives the kernel's bits, whichever path runs - resident or
    streaming, 16-byte accesses or (one float past the boundary; D % 4 != 0 is element-wise by itself) element-wise ones."""
    x0, t = _dyadic(B, D, 1000 * D + 10 * B)
    want = S.start_f32(x0, EPS_DYADIC, t, metric)
    got = _run_start(ops, x0, EPS_DYADIC, metric, noise=t)
    assert _same_bits(got, want), np.abs(got - want).max()
    for path in ("resident", "streaming"):
        for odd in (False, True):
            assert _same_bits(_run_start(ops, x0, EPS_DYADIC, metric, noise=t, path=path, odd=odd), want), (path, odd)
    if metric == "L1":
        assert _same_bits(got, x0 + t)
        if D >= 75:
            assert (got < 0).any() and (got > 1).any()  # the L1 output is not clamped: the run's projection follows
    else:
        assert (got >= 0).all() and (got <= 1).all()
    if B > 2 and metric == "L2":
        assert _same_bits(got[2], x0[2])  # a zero draw stays at x0
    if metric == "Linf":
        assert np.abs(got.astype(np.float64) - x0).max() <= EPS_DYADIC * 2  # t in [-2, 2] here; inside the ball scaled by max |t|


@pytest.mark.parametrize("D", SIZES)
@pytest.mark.parametrize("B", (1, 3, 7))
def test_l2_start_on_generic_noise(ops, B, D):
    """Standard normal noise, uniform x0.  The kernel's double sum runs in another order than math.fsum: it differs from the exact sum by
    at most D 2^-53 relative, so once rounded to float32 n is the reference's or one of its two float neighbours, and nothing else in the
    launch depends on an order: the row must equal, bit for bit, the restatement evaluated with one of those three n."""
    x0, t = _generic(B, D, seed=77 * D + B)
    eps = 0.3
    got = _run_start(ops, x0, eps, "L2", noise=t)
    exact = 0
    for b in range(B):
        n = F32(S.l2_norm(t[b].astype(np.float64)))
        cands = [S.start_f32(x0[b:b + 1], eps, t[b:b + 1], "L2", n=np.array([v], F32)) for v in (n, np.nextafter(n, F32(np.inf)), np.nextafter(n, F32(0)))]
        hits = [_same_bits(got[b:b + 1], c) for c in cands]
        assert any(hits), (b, np.abs(got[b] - cands[0][0]).max())
        exact += hits[0]
    assert exact >= (B + 1) // 2  # the neighbours are the exception
    d = np.sqrt(((got.astype(np.float64) - x0) ** 2).sum(axis=1))
    assert (d <= eps * (1 + 4 * U24) + math.sqrt(D) * U24).all()  # inside the ball (the clamp only shortens)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("draw", [False, True], ids=["noise", "philox"])
def test_start_paths_give_the_same_bits(ops, metric, draw):
    """Generic inputs, injected noise and the kernel's own draws: four instantiations, the same bits; past the resident size only the
    streaming path exists."""
    eps, seed = 0.1, 0xABCDEF0123456789
    for D in (75, 192, 4100):
        x0, t = _generic(7, D)
        noise = None if draw else t
        want = _run_start(ops, x0, eps, metric, noise=noise, seed=seed)
        for path in ("resident", "streaming"):
            for odd in (False, True):
                assert _same_bits(_run_start(ops, x0, eps, metric, noise=noise, seed=seed, path=path, odd=odd), want), (D, path, odd)
    x0, t = _generic(2, 12289)
    a = _run_start(ops, x0, eps, metric, noise=None if draw else t, seed=seed)
    b = _run_start(ops, x0, eps, metric, noise=None if draw else t, seed=seed, path="streaming", odd=True)
    assert _same_bits(a, b)
    import eeadv._native as n
    with pytest.raises(n.EEError):
        _run_start(ops, x0, eps, metric, noise=None if draw else t, seed=seed, path="resident")


@pytest.mark.parametrize("D", SIZES)
def test_in_kernel_uniform_draws_are_the_host_draws(ops, D):
    """Linf: t = 2 u - 1 is exact on both sides, so the launch with its own draw equals the launch - and the numpy restatement - fed
    eeadv.apgdstart.draw under the same key, and the float32 host start equals the device start bit for bit."""
    from eeadv import apgdstart
    B, eps, seed = 3, 8 / 255, apgdstart.seed_of(11, 2, 1)
    x0, _ = _generic(B, D, seed=D)
    t = apgdstart.draw(seed, B, D, "Linf")
    got = _run_start(ops, x0, eps, "Linf", seed=seed)
    assert _same_bits(got, S.start_f32(x0, eps, t, "Linf"))
    assert _same_bits(got, _run_start(ops, x0, eps, "Linf", noise=t))
    assert _same_bits(got, apgdstart.start(torch.from_numpy(x0), eps, torch.from_numpy(t), "Linf").numpy())
    # rows do not depend on the batch size, and another key is another draw
    x7, _ = _generic(7, D, seed=D)
    assert _same_bits(_run_start(ops, x7, eps, "Linf", seed=seed)[:3], got)
    if D >= 5:
        assert not _same_bits(_run_start(ops, x0, eps, "Linf", seed=apgdstart.seed_of(11, 2, 2)), got)


@pytest.mark.parametrize("metric", ["L2", "L1"])
@pytest.mark.parametrize("D", SIZES)
def test_in_kernel_normal_draws(ops, D, metric):
    """L2 / L1: the kernel forms t = sqrtf(-2 logf(1 - u_a)) * cosf(a) (or sinf) in float32; the reference (tests/apgd_start_reference.py)
    forms it in float64 from the same words and the same float32 angle a.  With the HIP math library's documented bounds taken as
    logf <= 2 ulp, cosf / sinf <= 2 ulp (each relative to its own result) and a correctly rounded sqrtf, as
    test_gpu_fab_restarts.py::test_in_kernel_normal_draws takes them: the logarithm's 2 x 2^-23 is halved by the root, which adds 2^-24;
    the cosine adds 2 x 2^-23; the product 2^-24:   delta = |t_dev - t| / |t| <= (1 + 2) 2^-23 + 2 x 2^-24 = 4 x 2^-23 = 8 x 2^-24.
    L1, x = fl(x0 + t):  |x_dev - x| <= |t| delta + |x0 + t_dev| 2^-24 <= (|t| delta + |x| 2^-24)(1 + 2^-20), element by element.
    L2: n moves by delta and is rounded once (2^-24); n + 1e-12f is rounded once more; s = fl(eps / .) once more: s moves by
    delta + 3 x 2^-24.  p = fl(t s) moves by delta (t) + delta + 3 x 2^-24 (s) + 2^-24 (its rounding) = 20 x 2^-24, and |p| <= eps
    since |t_i| <= n.  x0 + p < 2 is rounded once, 2^-24 at most, and the clamp does not expand:
        |x_dev - x| <= (20 eps + 1) 2^-24 (1 + 2^-20)   (the last factor covers the second-order terms).
    Both bounds come from the float64 restatement and the library's documented figures; nothing in them was measured on the kernel."""
    B, eps, seed = 3, 0.5, 0x1234ABCD5678EF01
    x0, _ = _generic(B, D, seed=D + 1)
    got = _run_start(ops, x0, eps, metric, seed=seed).astype(np.float64)
    delta = 8 * U24
    for b in range(B):
        t = S.draw_row(seed, b, D, metric)
        want = S.start_row(x0[b].astype(np.float64), float(F32(eps)), t, metric)
        err = np.abs(got[b] - want)
        if metric == "L1":
            bound = (np.abs(t) * delta + np.abs(want) * U24) * (1 + 2.0 ** -20)
        else:
            bound = np.full(D, (20 * eps + 1) * U24 * (1 + 2.0 ** -20))
        print("D=%d %s row %d: max |x_dev - x| / bound = %.3g" % (D, metric, b, (err / bound).max()))
        assert (err <= bound).all(), (b, (err / bound).max())


def test_a_row_that_is_not_finite_is_x0_and_bad_arguments(ops):
    import eeadv._native as n
    x0, t = _generic(4, 75)
    t[1, 3], t[2, 70] = np.inf, np.nan
    for path in ("resident", "streaming"):
        got = _run_start(ops, x0, 0.5, "L2", noise=t, path=path)
        assert _same_bits(got[1], x0[1]) and _same_bits(got[2], x0[2])
        assert not _same_bits(got[0], x0[0]) and not _same_bits(got[3], x0[3])
    x = torch.rand(2, 8, device=DEV)
    with pytest.raises(ValueError, match="two tensors"):
        ops.apgd_start_(x, x, 0.1, "Linf")
    with pytest.raises(n.EEError):
        ops.apgd_start_(x.clone(), x, -0.1, "Linf")
    with pytest.raises(ValueError, match="path"):
        ops.apgd_start_(x.clone(), x, 0.1, "Linf", path="fast")
    e = torch.zeros(0, 8, device=DEV)
    assert ops.apgd_start_(e.clone(), e, 0.1, "L2").shape == (0, 8)


# ---- the merge launch --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("D", [192, 193])
def test_merge_kernel_bit_exact(ops, D, odd):
    """One batch of 7 through three merges (first = 1, then two more): never fooled (rows 0, 6); fooled by the first restart only (1);
    by a later one only (2: the second, 3: the third); fooled twice (4: first and second, 5: second and third) - the first point must
    survive.  Rows hold NaN payloads too: the copy is a copy of bits."""
    rng = np.random.default_rng(D)
    B = 7
    robust_runs = np.array([[1, 0, 1, 1, 0, 1, 1], [1, 1, 0, 1, 0, 0, 1], [1, 1, 1, 0, 1, 0, 1]], np.int32)
    loss_runs = rng.standard_normal((3, B)).astype(F32)
    points = rng.integers(0, 2 ** 32, (3, B, D), dtype=np.uint64).astype(np.uint32)  # any bits, NaNs among them
    adv = rng.integers(0, 2 ** 32, (B, D), dtype=np.uint64).astype(np.uint32)
    rob, loss = np.full(B, 5, np.int32), np.full(B, 9.0, F32)  # what a reused run left behind: first = 1 overwrites it
    dev = lambda a: torch.from_numpy(a.view(F32) if a.dtype == np.uint32 else a).to(DEV)
    adv_d, rob_d, loss_d = dev(adv), dev(rob), dev(loss)
    if odd:
        adv_d = _odd(adv_d)
    untouched = adv.copy()
    for r in range(3):
        adv, rob, loss = S.merge(adv, rob, loss, points[r], robust_runs[r], loss_runs[r], r == 0)
        pts = dev(points[r])
        ops.apgd_merge_(adv_d, rob_d, loss_d, _odd(pts) if odd else pts, dev(robust_runs[r]), dev(loss_runs[r]), r == 0)
        assert _same_bits(adv_d.cpu().numpy().view(np.uint32), adv), r
        assert np.array_equal(rob_d.cpu().numpy(), rob) and _same_bits(loss_d.cpu().numpy(), loss), r
    assert list(rob) == [1, 0, 0, 0, 0, 0, 1]
    assert np.array_equal(adv[[0, 6]], untouched[[0, 6]])  # never fooled: never written
    assert np.array_equal(adv[1], points[0][1]) and np.array_equal(adv[2], points[1][2]) and np.array_equal(adv[3], points[2][3])
    assert np.array_equal(adv[4], points[0][4]) and np.array_equal(adv[5], points[1][5])  # the FIRST fooling point
    assert np.array_equal(loss, loss_runs.max(axis=0))
    with pytest.raises(ValueError, match="two tensors"):
        ops.apgd_merge_(adv_d, rob_d, loss_d, adv_d, rob_d, loss_d, False)


# ---- the loops ---------------------------------------------------------------------------------------------------------------------------
LOOPS = ("linf", "l2", "eot", "l1")
K, B_LOOP, N_ITER, N_RESTARTS = 10, 5, 10, 3
LOOP_EPS = {"linf": 0.03, "l2": 0.3, "eot": 0.03, "l1": 1.5}
LOOP_METRIC = {"linf": "Linf", "l2": "L2", "eot": "Linf", "l1": "L1"}


def _problem(name):
    g = torch.Generator().manual_seed(21)
    m = TinyNet(3, 8, K, 21).eval()
    x0 = 0.1 + 0.8 * torch.rand(B_LOOP, 3, 8, 8, generator=g)
    with torch.no_grad():
        y = m(x0).argmax(dim=1)
    uniform = LOOP_METRIC[name] == "Linf"
    draw = (lambda *s: torch.rand(*s, generator=g) * 2 - 1) if uniform else (lambda *s: torch.randn(*s, generator=g))
    t0, noise = draw(*x0.shape), draw(N_RESTARTS - 1, *x0.shape)
    return m.to(DEV), x0.to(DEV), y.to(DEV), t0.to(DEV), noise.to(DEV)


def _start(ops, name, x0, t):
    return ops.apgd_start_(torch.empty_like(x0), x0, LOOP_EPS[name], LOOP_METRIC[name], noise=t.contiguous())


def _loop(name, m, x0, x_init, y, **kw):
    from eeadv import engine
    eps = LOOP_EPS[name]
    if name == "l1":
        return engine.apgd_l1_loop(m, x0, x_init, y, N_ITER, eps, "ce", **kw)
    if name == "l2":
        return engine.apgd_loop(m, x0, x_init, y, N_ITER, eps, "ce", norm="L2", **kw)
    if name == "eot":
        return engine.apgd_loop(m, x0, x_init, y, N_ITER, eps, "ce", eot_iter=2, **kw)
    return engine.apgd_loop(m, x0, x_init, y, N_ITER, eps, "ce", **kw)


def _launches(ops, fn):
    """(result, launches per timing family) of fn() with the library's own launch recording on."""
    ops.prof_reset()
    ops.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        counts = [ops.prof_read(k)[1] for k in range(30)]
    finally:
        ops.prof_enable(False)
        ops.prof_reset()
    return out, counts


@pytest.mark.parametrize("name", LOOPS)
def test_loops_eager_graph_one_restart_and_the_cache(ops, name):
    """Eager and graph replay give the same bits with 3 restarts; n_restarts = 1 gives the bits and the launches of the call without the
    argument and takes no ticket; a 3-restart run leaves in the graph cache exactly the entries a 1-restart run makes and replays the
    graph that one captured; what restart 0 fooled stays fooled, at its point."""
    from eeadv import engine
    m, x0, y, t0, noise = _problem(name)
    x_init = _start(ops, name, x0, t0)  # the unprojected x0 + n for L1, as apgd_l1_loop takes it
    engine.clear_graphs()
    try:
        today, n_today = _launches(ops, lambda: _loop(name, m, x0, x_init, y, use_graph=False))
        state = torch.cuda.get_rng_state(DEV)
        one, n_one = _launches(ops, lambda: _loop(name, m, x0, x_init, y, use_graph=False, n_restarts=1, seed=None))
        assert torch.equal(torch.cuda.get_rng_state(DEV), state)  # no ticket
        assert all(torch.equal(p, q) for p, q in zip(today, one)) and n_today == n_one
        one_g = _loop(name, m, x0, x_init, y, use_graph=True, n_restarts=1)
        assert all(torch.equal(p, q) for p, q in zip(today, one_g))
        keys1 = set(engine._GRAPHS)
        graphs1 = {k: v.graph for k, v in engine._GRAPHS.items()}
        assert len(keys1) == 1
        assert engine._GRAPHS[next(iter(keys1))].run.adv_all is None  # the cumulative buffers exist only when a call asks for restarts
        three_g = _loop(name, m, x0, x_init, y, use_graph=True, n_restarts=N_RESTARTS, noise=noise)
        assert set(engine._GRAPHS) == keys1 and all(engine._GRAPHS[k].graph is g for k, g in graphs1.items())  # nothing new was captured
        three, n_three = _launches(ops, lambda: _loop(name, m, x0, x_init, y, use_graph=False, n_restarts=N_RESTARTS, noise=noise))
        assert all(torch.equal(p, q) for p, q in zip(three, three_g))
        # the eager launches of 3 restarts: 3 times those of one run, plus 2 starts and 3 merges under EE_K_PGD_STEP
        assert n_three[0] == 3 * n_today[0] + (N_RESTARTS - 1) + N_RESTARTS and n_three[1:] == [3 * c for c in n_today[1:]]
        engine.clear_graphs()
        _loop(name, m, x0, x_init, y, use_graph=True, n_restarts=N_RESTARTS, noise=noise)
        assert set(engine._GRAPHS) == keys1  # captured by a 3-restart run: the same key
        after = _loop(name, m, x0, x_init, y, use_graph=True)
        assert all(torch.equal(p, q) for p, q in zip(today, after))  # and it serves one restart
        assert not bool((three[1] & ~today[1]).any())  # robust never turns from False to True
        fooled = ~today[1]
        assert torch.equal(three[0][fooled], today[0][fooled]) and bool((three[2] >= today[2]).all())
        print("%s: robust after 1 restart %s, after 3 %s" % (name, today[1].tolist(), three[1].tolist()))
        seeded = [_loop(name, m, x0, x_init, y, use_graph=g, n_restarts=2, seed=17) for g in (False, True, True)]
        assert all(torch.equal(p, q) for s in seeded[1:] for p, q in zip(seeded[0], s))  # the kernel's own draws, replayed or not
        with pytest.raises(ValueError, match="n_restarts"):
            _loop(name, m, x0, x_init, y, n_restarts=0)
        with pytest.raises(ValueError, match="noise"):
            _loop(name, m, x0, x_init, y, n_restarts=2, noise=noise)
    finally:
        engine.clear_graphs()


@pytest.mark.parametrize("name", LOOPS)
def test_three_restarts_are_three_runs_combined_by_first_fooling(ops, name):
    """A 3-restart run with injected noise against three separate runs from those starts, combined by utils.attacks._first_fooling: the
    flags and the points bit for bit, the best loss the largest of the three.  (The EOT run's model does not redraw, so its runs are
    repeatable like the others.)"""
    import utils.attacks as A
    m, x0, y, t0, noise = _problem(name)
    x_init = _start(ops, name, x0, t0)
    starts = [x_init] + [_start(ops, name, x0, noise[r]) for r in range(N_RESTARTS - 1)]
    for use_graph in (False, True):
        three = _loop(name, m, x0, x_init, y, use_graph=use_graph, n_restarts=N_RESTARTS, noise=noise)
        runs = [_loop(name, m, x0, s, y, use_graph=use_graph) for s in starts]
        x_adv, robust = A._first_fooling(x0, [(xa, rb) for xa, rb, _ in runs])
        assert torch.equal(three[1], robust) and torch.equal(three[0], x_adv)
        assert torch.equal(three[2], torch.stack([r[2] for r in runs]).max(dim=0)[0])
    from eeadv import engine
    engine.clear_graphs()


def test_public_door_with_restarts_on_the_device(ops):
    """utils.attacks.APGD / APGD_T with n_restarts: one restart is the call it was and takes no ticket; a seed fixes the result; the
    target index keys the draws of APGD_T's classes."""
    import utils.attacks as A
    from tiny_models import Args
    m, x0, y, t0, _ = _problem("linf")
    args = Args(epsilon=0.03)
    un = t0 * 0.03
    one = A.APGD(m, args, x0, y, N_ITER, noise=un)
    state = torch.cuda.get_rng_state(DEV)
    again = A.APGD(m, args, x0, y, N_ITER, noise=un, n_restarts=1, seed=5)
    assert torch.equal(torch.cuda.get_rng_state(DEV), state)
    assert all(torch.equal(p, q) for p, q in zip(one, again))
    three = [A.APGD(m, args, x0, y, N_ITER, noise=un, n_restarts=3, seed=5) for _ in range(2)]
    assert all(torch.equal(p, q) for p, q in zip(*three)) and not bool((three[0][1] & ~one[1]).any())
    t = [A.APGD_T(m, args, x0, y, N_ITER, K, 2, noise=un, n_restarts=2, seed=5) for _ in range(2)]
    assert all(torch.equal(p, q) for p, q in zip(*t))
    from eeadv import engine
    engine.clear_graphs()
