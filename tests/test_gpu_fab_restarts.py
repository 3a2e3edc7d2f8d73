"""GPU: FAB restarts with the random start - ee_fab_start_f32 through ops.fab_start_, and the restart loop of
engine.fab_loop / fab_l1_loop / fab_u_loop / fab_u_l1_loop.

Bit-exact: the start launch on dyadic inputs against a numpy float32 restatement of its operation order, its four instantiations against
each other, the in-kernel uniform draws against eeadv.fabstart.draw, eager against graph replay, one restart against the call without the
argument.  In tolerance: generic noise (the row equals the restatement for n or one of its two float neighbours), the in-kernel normal
draws (the bound derived at test_in_kernel_normal_draws), and every launch of restarts 1 and 2 against the float64 references on the
launch's own inputs, at the tolerances of tests/test_gpu_fab.py and tests/test_gpu_fab_l1.py ::test_teacher_forced_trajectory."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import fab_l1_reference as R1
import fab_reference as R
import fab_start_reference as S
from tiny_models import TinyNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")
F32 = np.float32
INF = float("inf")
METRICS = ("Linf", "L2", "L1")
SIZES = (1, 3, 5, 75, 192, 1023, 2049, 4100)  # the last two give a thread more than one group of four
U23 = 2.0 ** -23


@pytest.fixture(scope="module")
def ops():
    from eeadv import ops
    return ops


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the start launch --------------------------------------------------------------------------------------------------------------------
def _norm32(t, metric):
    """The kernel's n of one row: the sum in float64 (math.fsum: the exactly rounded one), rounded to float32 once."""
    a = np.abs(t.astype(np.float64))
    if np.isnan(a).any():
        return F32(np.nan)
    if metric == "Linf":
        return F32(a.max())
    if metric == "L2":
        return F32(math.sqrt(math.fsum(a * a)))
    return F32(math.fsum(a))


def _start_row32(x0, res, eps, t, n):
    """The operation order of ee_fab_start_f32 in numpy float32: every operation rounded once."""
    if not np.isfinite(n) or n == 0:
        return x0.copy()
    m = min(F32(res), F32(eps))
    return np.clip(x0 + ((m * t) / F32(n)) * F32(0.5), F32(0), F32(1)).astype(F32)


def _start_numpy(x0, res, eps, t, metric):
    return np.stack([_start_row32(x0[b], res[b], eps, t[b], _norm32(t[b], metric)) for b in range(len(x0))])


ROW_CASES = ("res_inf", "res_small", "res_zero", "noise_zero", "faces", "res_large")
EPS_DYADIC = 0.125


def _dyadic_inputs(B, D, shift, seed):
    """Multiples of 2^-8: every double sum of |t_i| or t_i^2 is exact in any order.  Row b is case (b + shift) % 6."""
    rng = np.random.default_rng(seed)
    t = (rng.integers(-64, 65, (B, D)) / 256.0).astype(F32)
    x0 = (rng.integers(0, 257, (B, D)) / 256.0).astype(F32)
    res = np.full(B, 2.0 ** -5, F32)
    names = [ROW_CASES[(b + shift) % len(ROW_CASES)] for b in range(B)]
    for b, name in enumerate(names):
        if name == "res_inf":
            res[b] = np.inf
        if name == "res_zero":
            res[b] = 0.0
        if name == "noise_zero":
            t[b] = 0.0
        if name == "faces":
            x0[b] = np.where(rng.random(D) < 0.5, 0.0, 1.0).astype(F32)
        if name == "res_large":
            res[b] = 4.0
        if name not in ("noise_zero",) and not t[b].any():
            t[b, 0] = F32(0.25)  # D = 1 may have drawn a zero
    return x0, res, t, names


def _run_start(ops, x0, res, eps, metric, noise=None, seed=0, path="auto", odd=False):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    x0d, nd = dev(x0), (None if noise is None else dev(noise))
    x = torch.full(x0.shape, 7.0, device=DEV)  # garbage: every element must be written
    if odd:
        x0d, x = _odd(x0d), _odd(x)
        nd = None if nd is None else _odd(nd)
    ops.fab_start_(x, x0d, dev(res), eps, metric, seed=seed, noise=nd, path=path)
    return x.cpu().numpy()


def _odd(t):
    """The same values at an address 4 bytes past a 16-byte boundary: the kernel then takes its element-wise accesses."""
    pad = torch.zeros(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = pad[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("D", SIZES)
@pytest.mark.parametrize("B", (1, 3, 7))
def test_start_kernel_bit_exact(ops, B, D, metric):
    seen = set()
    for shift in range(len(ROW_CASES)):
        x0, res, t, names = _dyadic_inputs(B, D, shift, 1000 * D + 10 * B + shift)
        want = _start_numpy(x0, res, EPS_DYADIC, t, metric)
        got = _run_start(ops, x0, res, EPS_DYADIC, metric, noise=t)
        assert _same_bits(got, want), (shift, names, np.abs(got - want).max())
        for b, name in enumerate(names):
            if name in ("res_zero", "noise_zero"):
                assert _same_bits(got[b], x0[b]), name  # m = 0 and n = 0 leave the row at x0
            elif D >= 5 and name != "faces":
                assert not _same_bits(got[b], x0[b]), name  # (a short row may sit on the faces its noise pushes it to)
            d = S.dist((got[b].astype(np.float64) - x0[b]), metric)
            slack = {"Linf": 1.0, "L2": D ** 0.5, "L1": float(D)}[metric] * 2.0 ** -24
            assert d <= min(float(res[b]), EPS_DYADIC) / 2 * (1 + 4 * 2.0 ** -24) + slack, (name, d)
        seen |= set(names)
        assert (got >= 0).all() and (got <= 1).all()
    assert seen == set(ROW_CASES)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("D", SIZES)
@pytest.mark.parametrize("B", (1, 3, 7))
def test_start_kernel_generic_inputs(ops, B, D, metric):
    """Standard normal noise, uniform x0, res on either side of eps.  The kernel's double sum runs in another order than math.fsum: it
    differs from the exact sum by at most D 2^-53 relative, so once rounded to float32 n is the reference's or one of its two float
    neighbours, and nothing else in the launch depends on an order: the row must equal, bit for bit, the float32 restatement evaluated
    with one of those three n.  (The operation count - one product, one quotient, one halving, one sum, each rounded once - is the
    restatement's by construction, so no further slack is granted.)"""
    rng = np.random.default_rng(77 * D + B)
    t = rng.standard_normal((B, D)).astype(F32)
    x0 = rng.random((B, D)).astype(F32)
    eps = 0.3
    res = (rng.random(B) * 0.6).astype(F32)
    res[0] = np.inf
    got = _run_start(ops, x0, res, eps, metric, noise=t)
    exact = 0
    for b in range(B):
        n = _norm32(t[b], metric)
        cands = [_start_row32(x0[b], res[b], eps, t[b], v) for v in (n, np.nextafter(n, F32(np.inf)), np.nextafter(n, F32(0)))]
        hits = [_same_bits(got[b], c) for c in cands]
        assert any(hits), (b, np.abs(got[b] - cands[0]).max())
        exact += hits[0]
    assert exact >= (B + 1) // 2  # the neighbours are the exception


def _generic(B, D, seed=5):
    rng = np.random.default_rng(seed)
    return rng.random((B, D)).astype(F32), np.array([np.inf, 0.01, 0.2, 0.0, 0.05, 1.0, 0.03][:B], F32), rng.standard_normal((B, D)).astype(F32)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("draw", [False, True], ids=["noise", "philox"])
def test_start_paths_give_the_same_bits(ops, metric, draw):
    """Resident against streaming, 16-byte against element-wise accesses (the same rows 4 bytes past a 16-byte boundary; D % 4 != 0 is
    element-wise by itself), with injected noise and with the kernel's own draws: four instantiations, the same bits."""
    eps, seed = 0.1, 0xABCDEF0123456789
    for D in (75, 192, 4100):
        x0, res, t = _generic(7, D)
        noise = None if draw else t
        want = _run_start(ops, x0, res, eps, metric, noise=noise, seed=seed)
        for path in ("resident", "streaming"):
            for odd in (False, True):
                got = _run_start(ops, x0, res, eps, metric, noise=noise, seed=seed, path=path, odd=odd)
                assert _same_bits(got, want), (D, path, odd)
    x0, res, t = _generic(2, 12289)  # past the resident size: streaming only
    a = _run_start(ops, x0, res, eps, metric, noise=None if draw else t, seed=seed)
    b = _run_start(ops, x0, res, eps, metric, noise=None if draw else t, seed=seed, path="streaming", odd=True)
    assert _same_bits(a, b)
    import eeadv._native as n
    with pytest.raises(n.EEError):
        _run_start(ops, x0, res, eps, metric, noise=None if draw else t, seed=seed, path="resident")


@pytest.mark.parametrize("D", SIZES)
def test_in_kernel_uniform_draws_are_the_host_draws(ops, D):
    """Linf: t = 2 u - 1 is exact on both sides, so the launch with its own draw equals the launch - and the numpy restatement - fed
    eeadv.fabstart.draw under the same key."""
    from eeadv import fabstart
    B, eps, seed = 3, 8 / 255, fabstart.seed_of(11, 2, 1)
    x0, res, _ = _generic(B, D, seed=D)
    t = fabstart.draw(seed, B, D, "Linf")
    got = _run_start(ops, x0, res, eps, "Linf", seed=seed)
    assert _same_bits(got, _start_numpy(x0, res, eps, t, "Linf"))
    assert _same_bits(got, _run_start(ops, x0, res, eps, "Linf", noise=t))
    host = fabstart.start(torch.from_numpy(x0), torch.from_numpy(res), eps, torch.from_numpy(t), "Linf").numpy()
    assert _same_bits(got, host)  # the float32 host start equals the device start bit for bit


@pytest.mark.parametrize("metric", ["L2", "L1"])
@pytest.mark.parametrize("D", SIZES)
def test_in_kernel_normal_draws(ops, D, metric):
    """L2 / L1: the kernel forms t = sqrtf(-2 logf(1 - u_a)) * cosf(a) (or sinf) in float32; the reference (tests/fab_start_reference.py)
    forms it in float64 from the same words and the same float32 angle a.  With the HIP math library's documented bounds taken as
    logf <= 2 ulp, cosf / sinf <= 2 ulp (each relative to its own result; the table lists 1 to 2 for them) and a correctly rounded sqrtf:
    the logarithm's 2 x 2^-23 is halved by the root, which adds 2^-24; the cosine adds 2 x 2^-23; the product 2^-24:
        delta = |t_dev - t| / |t| <= (1 + 2) 2^-23 + 2 x 2^-24 = 4 x 2^-23.
    n, a norm of t, moves by at most delta relatively and is rounded once (2^-24); q = fl(fl(m t) / n) moves by delta (t) + delta + 2^-24
    (n) and is rounded twice: |q_dev - q| <= |q| (2 delta + 3 x 2^-24), |q| <= m since |t_i| <= n in all three norms.  Halving is exact;
    x0 + q / 2 <= 2 is rounded once on the device (2^-23 at most, before the clamp, which does not expand).  So, against the float64
    start, element by element:  |x_dev - x| <= (m / 2)(8 x 2^-23 + 3 x 2^-24) + 2^-23 = (4.75 m + 1) 2^-23.  The bound is formed from the
    float64 restatement and the library's documented figures; nothing in it was measured on the kernel."""
    B, eps, seed = 3, 0.5, 0x1234ABCD5678EF01
    x0, res, _ = _generic(B, D, seed=D + 1)
    got = _run_start(ops, x0, res, eps, metric, seed=seed).astype(np.float64)
    for b in range(B):
        t = S.draw_row(seed, b, D, metric)
        want = S.start_row(x0[b].astype(np.float64), float(res[b]), float(F32(eps)), t, metric)
        m = min(float(res[b]), float(F32(eps)))
        err = np.abs(got[b] - want).max()
        print("D=%d %s row %d: max |x_dev - x| = %.3g (bound %.3g)" % (D, metric, b, err, (4.75 * m + 1) * U23))
        assert err <= (4.75 * m + 1) * U23, (b, err)
    # and through the host draw: float32 normals within the same delta (plus their own cast) of the float64 ones
    from eeadv import fabstart
    t32 = fabstart.draw(seed, B, D, metric).astype(np.float64)
    t64 = np.stack([S.draw_row(seed, b, D, metric) for b in range(B)])
    assert (np.abs(t32 - t64) <= 2.0 ** -24 * np.abs(t64) * (1 + 2.0 ** -20)).all()


@pytest.mark.parametrize("metric", METRICS)
def test_seeds_rows_and_batch_size(ops, metric):
    """The same seed gives the same bits, another seed other rows, and rows 0..2 of a B = 7 launch are a B = 3 launch: a row's draw
    depends on (seed, b, element) alone."""
    D, eps = 1023, 0.1
    x0, res, _ = _generic(7, D)
    res[:] = np.inf
    a = _run_start(ops, x0, res, eps, metric, seed=41)
    assert _same_bits(a, _run_start(ops, x0, res, eps, metric, seed=41))
    b = _run_start(ops, x0, res, eps, metric, seed=42)
    assert all(not _same_bits(a[r], b[r]) for r in range(7))
    same_x0 = np.repeat(x0[:1], 7, axis=0)
    rows = _run_start(ops, same_x0, res, eps, metric, seed=41)
    assert all(not _same_bits(rows[0], rows[r]) for r in range(1, 7))  # every row has a draw of its own
    c = _run_start(ops, x0[:3], res[:3], eps, metric, seed=41)
    assert _same_bits(a[:3], c)
    big = _run_start(ops, x0, res, eps, metric, seed=41 + 2 ** 63)  # the key's upper half counts
    assert not _same_bits(a, big)


def test_empty_batch_and_bad_arguments(ops):
    import eeadv._native as n
    e = torch.empty(0, 12, device=DEV)
    out = ops.fab_start_(e.clone(), e, torch.empty(0, device=DEV), 0.1, "L2")
    torch.cuda.synchronize()
    assert out.shape == (0, 12)
    x0 = torch.rand(2, 8, device=DEV)
    x, res = torch.zeros_like(x0), torch.ones(2, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    call = lambda metric, path, eps=0.1: n.lib.ee_fab_start_f32(p(x), p(x0), p(res), None, 2, 8, eps, metric, 0, path, None)
    assert call(0, 3) == -2 and call(0, -1) == -2 and call(3, 0) == -2 and call(-1, 0) == -2 and call(0, 0, -1.0) == -2
    assert n.lib.ee_fab_start_f32(p(x), p(x0), p(res), None, 2, 12289, 0.1, 0, 0, 1, None) == -3
    torch.cuda.synchronize()
    assert bool((x == 0).all())  # nothing was launched
    with pytest.raises(ValueError, match="path"):
        ops.fab_start_(x, x0, res, 0.1, "Linf", path="fast")
    with pytest.raises(ValueError, match="metric"):
        ops.fab_start_(x, x0, res, 0.1, "L0")
    with pytest.raises(ValueError, match="two tensors"):
        ops.fab_start_(x0, x0, res, 0.1, "Linf")
    assert call(0, 0) == 0
    torch.cuda.synchronize()
    assert bool((x != 0).any())


# ---- the loops -----------------------------------------------------------------------------------------------------------------------------
LOOPS = ("fab", "fab_l1", "fab_u", "fab_u_l1")
K, B_LOOP, N_ITER, N_RESTARTS = 10, 7, 10, 3
LOOP_EPS = {"fab": 0.05, "fab_u": 0.05, "fab_l1": 3.0, "fab_u_l1": 3.0}
LOOP_METRIC = {"fab": "Linf", "fab_u": "Linf", "fab_l1": "L1", "fab_u_l1": "L1"}


def _problem():
    g = torch.Generator().manual_seed(21)
    m = TinyNet(3, 8, K, 21).eval()
    x0 = 0.1 + 0.8 * torch.rand(B_LOOP, 3, 8, 8, generator=g)
    x0[0, :, :2], x0[0, :, 2:4] = 0.0, 1.0
    with torch.no_grad():
        order = torch.sort(m(x0), dim=1, descending=True, stable=True)[1]
    noise = torch.randn(N_RESTARTS - 1, *x0.shape, generator=torch.Generator().manual_seed(8))
    return m.to(DEV), x0.to(DEV), order[:, 0].contiguous().to(DEV), order[:, 1].contiguous().to(DEV), noise.to(DEV)


def _loop(name, m, x0, y, t, **kw):
    from eeadv import engine
    eps = LOOP_EPS[name]
    if name == "fab":
        return engine.fab_loop(m, x0, y, t, N_ITER, eps, **kw)
    if name == "fab_l1":
        return engine.fab_l1_loop(m, x0, y, t, N_ITER, eps, **kw)
    if name == "fab_u":
        return engine.fab_u_loop(m, x0, y, N_ITER, eps, nclass=K, **kw)
    return engine.fab_u_l1_loop(m, x0, y, N_ITER, eps, nclass=K, **kw)


def _make_run(name, x0, y, t, noise):
    from eeadv import engine
    eps = LOOP_EPS[name]
    seeds = (0,) * (N_RESTARTS - 1)
    if name == "fab":
        run = engine._FabRun(x0, y, N_ITER, eps)
        run.load(x0, y, t, eps, seeds, noise)
    elif name == "fab_l1":
        run = engine._FabL1Run(x0, y, N_ITER, eps)
        run.load(x0, y, t, eps, seeds, noise)
    elif name == "fab_u":
        run = engine._FabURun(x0, y, N_ITER, eps, K)
        run.load(x0, y, eps, seeds, noise)
    else:
        run = engine._FabUL1Run(x0, y, N_ITER, eps, K)
        run.load(x0, y, eps, seeds, noise)
    return run


@pytest.mark.parametrize("name", LOOPS)
def test_loops_eager_graph_one_restart_and_the_cache(name):
    """Eager and graph replay give the same bits with 3 restarts; n_restarts = 1 gives the bits of the call without the argument; a
    3-restart run leaves in the graph cache exactly the entries a 1-restart run makes, and replays the graph that one captured; the
    norm never grows with restarts, and where it did not shrink the adversarial point is the one of the single run."""
    from eeadv import engine
    m, x0, y, t, noise = _problem()
    eps = LOOP_EPS[name]
    engine.clear_graphs()
    try:
        today = _loop(name, m, x0, y, t, use_graph=False)
        one = _loop(name, m, x0, y, t, use_graph=False, n_restarts=1, seed=3)
        assert all(torch.equal(p, q) for p, q in zip(today, one))
        one_g = _loop(name, m, x0, y, t, use_graph=True, n_restarts=1)
        assert all(torch.equal(p, q) for p, q in zip(today, one_g))
        keys1 = set(engine._GRAPHS)
        graphs1 = {k: v.graph for k, v in engine._GRAPHS.items()}
        assert len(keys1) == 1
        three_g = _loop(name, m, x0, y, t, use_graph=True, n_restarts=N_RESTARTS, noise=noise)
        assert set(engine._GRAPHS) == keys1 and all(engine._GRAPHS[k].graph is g for k, g in graphs1.items())  # nothing new was captured
        three = _loop(name, m, x0, y, t, use_graph=False, n_restarts=N_RESTARTS, noise=noise)
        assert all(torch.equal(p, q) for p, q in zip(three, three_g))
        engine.clear_graphs()
        _loop(name, m, x0, y, t, use_graph=True, n_restarts=N_RESTARTS, noise=noise)
        assert set(engine._GRAPHS) == keys1  # captured by a 3-restart run: the same key
        after = _loop(name, m, x0, y, t, use_graph=True)
        assert all(torch.equal(p, q) for p, q in zip(today, after))  # and it serves one restart
        res1, res3 = today[2], three[2]
        assert bool((res3 <= res1).all()) and bool(torch.isfinite(res3).any())
        kept = res3 == res1
        assert torch.equal(three[0][kept], today[0][kept]) and torch.equal(three[1], ~(res3 <= eps))
        print("%s: norm after 1 restart %s, after 3 %s" % (name, res1.tolist(), res3.tolist()))
        seeded = [_loop(name, m, x0, y, t, use_graph=g, n_restarts=2, seed=17) for g in (False, True, True)]
        assert all(torch.equal(p, q) for s in seeded[1:] for p, q in zip(seeded[0], s))  # the kernel's own draws, replayed or not
        with pytest.raises(ValueError, match="n_restarts"):
            _loop(name, m, x0, y, t, n_restarts=0)
        with pytest.raises(ValueError, match="noise"):
            _loop(name, m, x0, y, t, n_restarts=2, noise=noise)
    finally:
        engine.clear_graphs()


def _recorded(name, m, x0, y, t, noise):
    """The eager run of N_RESTARTS restarts with every launch recorded; also checks that the recorded run is the loop's."""
    run = _make_run(name, x0, y, t, noise)
    recs, starts = [], []
    proj, step_, commit_ = run.proj, run.step_, run.commit_

    def rproj(x, o, w, df, path, scal):
        recs.append(dict(x_in=x.clone(), w=w.clone(), df=df.clone()))
        out = proj(x, o, w, df, path, scal)
        recs[-1]["scal"] = scal.clone()
        return out

    def rstep(x, o, w, scal):
        out = step_(x, o, w, scal)
        recs[-1]["x_step"] = x.clone()
        return out

    def rcommit(z, yy, x, o, adv, res, pred, flags, counter):
        recs[-1].update(z2=z.clone(), adv_in=adv.clone(), res_in=res.clone())
        out = commit_(z, yy, x, o, adv, res, pred, flags, counter)
        recs[-1].update(x_out=x.clone(), adv=adv.clone(), res=res.clone(), pred=pred.clone(), flags=flags.clone())
        return out

    run.proj, run.step_, run.commit_ = rproj, rstep, rcommit
    for r in range(N_RESTARTS):
        if r == 0:
            run.start(m)
        else:
            res_in, adv_in = run.res.clone(), run.adv.clone()
            run.restart(m, r)
            assert torch.equal(run.res, res_in) and torch.equal(run.adv, adv_in) and int(run.counter.item()) == 0 and not bool(run.flags.any())
            starts.append(dict(res_in=res_in.cpu(), x=run.x.detach().clone().cpu()))
        for _ in range(N_ITER):
            run.iteration(m)
            recs[-1]["restart"] = torch.tensor(r)
        assert int(run.counter.item()) == N_ITER
    got = run.result()
    plain = _loop(name, m, x0, y, t, use_graph=False, n_restarts=N_RESTARTS, noise=noise)
    assert all(torch.equal(p, q) for p, q in zip(got, plain))
    assert len(recs) == N_RESTARTS * N_ITER
    return [{k: v.cpu() for k, v in e.items()} for e in recs], starts


def _check_linf_launches(e, o, yc, i):
    """tests/test_gpu_fab.py::test_teacher_forced_trajectory, on the launch's own recorded inputs: the signs equal, lambda within
    max(2 E, 4 ulp) with E the float32 restatement's own error on these problems, the stepped point within that bound propagated through
    the step, the commit exact."""
    from test_gpu_fab import _proj_reference, _rel_err
    Bn = o.shape[0]
    x2, w2, df = e["x_in"].flatten(1).numpy(), e["w"].flatten(1).numpy(), e["df"].numpy()
    scal = e["scal"].numpy()
    lam64, sgn, lam32, on = _proj_reference(x2, o, w2, df)
    E = float(_rel_err(lam32, lam64).max())
    tol = max(2 * E, 4 * 2.0 ** -23)
    assert (scal[1][on] == sgn[on]).all() and (scal[:, ~on] == 0).all(), i
    assert (_rel_err(scal[0].astype(np.float64), lam64)[on] <= tol).all(), (i, E)
    xs = e["x_step"].flatten(1).numpy()
    for b in range(Bn):
        if not on[b]:
            assert np.array_equal(xs[b], x2[b]), (i, b)
            continue
        l1, s1, n1, d1 = R.project(x2[b].astype(np.float64), w2[b].astype(np.float64), float(df[b]))
        c2 = float(F32(float(df[b]) + float(np.sum(w2[b].astype(np.float64) * (o[b] - x2[b]).astype(np.float64)))))
        l2, s2, n2, d2 = R.project(o[b].astype(np.float64), w2[b].astype(np.float64), c2)
        a1, a2 = max(n1, 1e-8), max(n2, 1e-8)
        alpha = min(a1 / (a1 + a2), 0.1)
        want = np.clip((x2[b] + 1.05 * d1) * (1 - alpha) + (o[b] + 1.05 * d2) * alpha, 0, 1)
        atol = 1.05 * tol * (n1 + n2) + tol * alpha + 8 * 2.0 ** -24
        assert (np.abs(xs[b].astype(np.float64) - want) <= atol).all(), (i, b, np.abs(xs[b] - want).max())
    x0f, xst = torch.from_numpy(o).view(e["x_step"].shape), e["x_step"]
    n_adv = 0
    for b in range(Bn):
        pred, nan = R.first_class(e["z2"][b])
        is_adv = pred != yc[b] and not nan
        nrm = (xst[b] - x0f[b]).abs().max()
        improved = is_adv and float(nrm) < float(e["res_in"][b])
        assert int(e["pred"][b]) == pred and int(e["flags"][b]) == (1 if is_adv else 0) | (2 if improved else 0), (i, b)
        assert torch.equal(e["res"][b], nrm if improved else e["res_in"][b]), (i, b)
        assert torch.equal(e["adv"][b], xst[b] if improved else e["adv_in"][b]), (i, b)
        assert torch.equal(e["x_out"][b], x0f[b] + 0.9 * (xst[b] - x0f[b]) if is_adv else xst[b]), (i, b)
        n_adv += is_adv
    return n_adv


def _check_l1_launches(e, o, yc, i):
    """tests/test_gpu_fab_l1.py::test_teacher_forced_trajectory, on the launch's own recorded inputs."""
    from test_gpu_fab_l1 import _within_one_ulp
    Bn = o.shape[0]
    xin, wv, dfv = e["x_in"].flatten(1).numpy(), e["w"].flatten(1).numpy(), e["df"].numpy()
    scal = e["scal"].numpy()
    for b in range(Bn):
        sabs = float(np.abs(wv[b]).astype(np.float64).sum())
        if not (np.isfinite(dfv[b]) and dfv[b] != 0 and sabs > 0):
            assert (scal[:, [b, Bn + b]] == 0).all(), (i, b)  # no hyperplane: both problems rest
            continue
        for k, (p, wq, c) in enumerate(R1.problems(dict(x=xin[b], x0=o[b], w=wv[b], df=dfv[b]))):
            q = k * Bn + b
            th, ph, s64, n64, _ = R1.project(p, wq, float(c))
            lo, hi, _ = R1.fill_margin(p, wq, float(c))
            assert scal[1, q] == s64 and scal[0, q] == F32(th), (i, q, scal[:, q], th)
            assert _within_one_ulp(scal[2, q], n64), (i, q, scal[2, q], n64)
            assert abs(float(scal[3, q]) - ph) <= 2.0 ** -24 * ph + (2 * abs(float(c)) - lo) / (lo + hi) * 192 * 2.0 ** -52, (i, q)
    xs = e["x_step"].flatten(1).numpy()
    n_adv = 0
    for b in range(Bn):
        want = R1.step_f32(xin[b], o[b], wv[b], tuple(scal[k, b] for k in range(4)) + tuple(scal[k, Bn + b] for k in range(4)))
        assert np.array_equal(xs[b], want), (i, b)
        pred, nan = R1.first_class(e["z2"][b])
        is_adv = pred != yc[b] and not nan
        nrm = R1.l1(xs[b] - o[b])
        improved = is_adv and nrm < float(e["res_in"][b])
        assert int(e["pred"][b]) == pred and int(e["flags"][b]) == (1 if is_adv else 0) | (2 if improved else 0), (i, b)
        if improved:
            assert _within_one_ulp(e["res"][b], nrm) and np.array_equal(e["adv"][b].flatten().numpy(), xs[b]), (i, b)
        else:
            assert float(e["res"][b]) == float(e["res_in"][b]) and torch.equal(e["adv"][b], e["adv_in"][b]), (i, b)
        assert np.array_equal(e["x_out"][b].flatten().numpy(), R1.shrink_f32(xs[b], o[b]) if is_adv else xs[b]), (i, b)
        n_adv += is_adv
    return n_adv


@pytest.mark.parametrize("name", LOOPS)
def test_trajectory_of_the_restarts(name):
    """The eager run with every launch recorded.  Each restart's start point against the float64 reference evaluated on the run's own res
    (|x_dev - x| <= (m + 1) 2^-23: the float32 roundings of the product, the quotient and n - each 2^-24 of |q| <= m, halved: 0.75 m 2^-23,
    taken as m for the second-order terms - and the one rounding of the sum, whose value is below 2), inside the radius min(res, eps) / 2, with the iterate chain unbroken.  Then every
    launch of restarts 1 and 2, teacher-forced on its own recorded inputs against the float64 references, at the tolerances of the
    metric's own test_teacher_forced_trajectory."""
    metric, eps = LOOP_METRIC[name], LOOP_EPS[name]
    m, x0, y, t, noise = _problem()
    recs, starts = _recorded(name, m, x0, y, t, noise)
    o = x0.cpu().flatten(1).numpy()
    yc = y.cpu().tolist()
    D = o.shape[1]
    for r, st in enumerate(starts, start=1):
        first = recs[r * N_ITER]
        assert torch.equal(first["x_in"], st["x"]) and torch.equal(st["res_in"], recs[r * N_ITER - 1]["res"])
        assert torch.equal(first["res_in"], st["res_in"])  # res is carried into the restart, not reset
        for b in range(B_LOOP):
            m_b = min(float(st["res_in"][b]), float(F32(eps)))
            want = S.start_row(o[b].astype(np.float64), float(st["res_in"][b]), float(F32(eps)), noise[r - 1, b].cpu().flatten().double().numpy(), metric)
            got = st["x"][b].flatten().double().numpy()
            assert np.abs(got - want).max() <= (m_b + 1) * U23, (r, b)
            slack = {"Linf": 1.0, "L1": float(D)}[metric] * 2.0 ** -24
            assert S.dist(got - o[b], metric) <= m_b / 2 * (1 + 4 * 2.0 ** -24) + slack, (r, b)
        assert not torch.equal(st["x"], x0.cpu())
    check = _check_l1_launches if metric == "L1" else _check_linf_launches
    n_adv = 0
    for i in range(N_ITER, N_RESTARTS * N_ITER):
        e = recs[i]
        if i % N_ITER:
            assert torch.equal(e["x_in"], recs[i - 1]["x_out"]), i
        n_adv += check(e, o, yc, i)
    assert n_adv > 0  # the restarts met adversarial points
    res = [recs[r * N_ITER + N_ITER - 1]["res"] for r in range(N_RESTARTS)]
    assert bool((res[1] <= res[0]).all()) and bool((res[2] <= res[1]).all())


# ---- driver --------------------------------------------------------------------------------------------------------------------------
def test_mnist_driver_evaluates_with_fab_t_restarts_from_a_graph(tmp_path):
    env = dict(os.environ, EEADV_GRAPH="1")
    r = subprocess.run([sys.executable, "experiments_mnist.py", "-c", "configs_mnist/adversarial_training.yml", "--data", "synthetic:1:1",
                        "--output-root", str(tmp_path), "-e", "--attack_method", "FAB-T", "--fab_iters", "2", "--fab_restarts", "2"],
                       cwd=os.path.join(PKG, "MNIST"), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    logs = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path)) for f in fs if f.startswith("log")]
    text = r.stdout + "".join(open(f).read() for f in logs)
    assert re.search(r"^ \* FAB-T: FAB-T, 2 iterations per target class, 2 restarts$", text, flags=re.M)
    assert text.index("2 restarts") < text.index("Test_clean")  # before the first batch
    clean = re.findall(r"^ \* Clean Prec@1 ([\d.]+)", text, flags=re.M)
    adv = re.findall(r"^ \* Adv Prec@1 ([\d.]+) Prec@5 ([\d.]+)$", text, flags=re.M)
    assert len(clean) >= 1 and len(clean) == len(adv)
    for c1, (a1, _) in zip(clean, adv):
        assert float(a1) <= float(c1)
