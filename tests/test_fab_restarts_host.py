"""CPU: FAB restarts with the random start.  The host restatement of the kernel's draws (eeadv.fabstart) against the
explicit Philox of tests/fab_start_reference.py, the keys of the starts, the four plain-torch host runs of utils/attacks.py with restarts
against the reference's chain - teacher-forced in float64 at every restart's start point, the tolerances of the existing host FAB tests -
what is kept across restarts, the radius of every start, the ABI of ee_fab_start_f32 and the drivers."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import fab_start_reference as S
from test_fab_u_host import CHECKS, EPS64, METRICS, _mlp_case, _mnist, cpu_plumbing, host_iteration  # noqa: F401  (cpu_plumbing is a fixture)
from tiny_models import Args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = {"Linf": 0.05, "L2": 0.5, "L1": 3.0}
U24 = 2.0 ** -24


# ---- the draws -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 3, 5, 75, 192])
def test_uniform_draw_is_the_reference_bit_for_bit(D):
    from eeadv import fabstart
    for seed, B in ((0, 1), (0x0123456789ABCDEF, 3), (2 ** 64 - 1, 2)):
        t = fabstart.draw(seed, B, D, "Linf")
        assert t.dtype == np.float32 and t.shape == (B, D)
        want = np.stack([S.draw_row(seed, b, D, "Linf") for b in range(B)])
        assert np.array_equal(t.astype(np.float64), want)  # 2 u - 1 is exact in both
        assert (t >= -1).all() and (t < 1).all()


@pytest.mark.parametrize("metric", ["L2", "L1"])
@pytest.mark.parametrize("D", [1, 3, 5, 75, 192])
def test_normal_draw_is_the_reference_to_float32_rounding(D, metric):
    """Both sides form the value in float64 from the same words and the same float32 angle; they differ by the libm of numpy against that
    of math (a few 2^-53) and the one cast to float32: |t - ref| <= 2^-24 |ref| (1 + 2^-20)."""
    from eeadv import fabstart
    seed, B = 0xFEDCBA9876543210, 3
    t = fabstart.draw(seed, B, D, metric).astype(np.float64)
    want = np.stack([S.draw_row(seed, b, D, metric) for b in range(B)])
    assert (np.abs(t - want) <= U24 * np.abs(want) * (1 + 2.0 ** -20)).all()
    assert np.array_equal(fabstart.draw(seed, B, D, "L2"), fabstart.draw(seed, B, D, "L1"))  # one draw, two norms
    if D >= 75:
        assert abs(float(t.mean())) < 0.3 and 0.6 < float(t.std()) < 1.4  # standard normals, loosely: 225 or more of them


def test_a_row_depends_on_seed_row_and_element_only():
    from eeadv import fabstart
    for metric in METRICS:
        a, b = fabstart.draw(5, 7, 75, metric), fabstart.draw(5, 3, 75, metric)
        assert np.array_equal(a[:3], b)  # not on B
        assert np.array_equal(fabstart.draw(5, 2, 192, metric)[:, :75], a[:2])  # not on D
        assert not np.array_equal(a[0], a[1]) and not np.array_equal(a, fabstart.draw(6, 7, 75, metric))
    with pytest.raises(ValueError, match="metric"):
        fabstart.draw(5, 1, 4, "L3")


def test_seed_of_gives_every_target_class_and_restart_its_own_key():
    from eeadv import fabstart
    keys = {(j, r): fabstart.seed_of(1234, j, r) for j in range(0, 12) for r in range(0, 8)}
    assert len(set(keys.values())) == len(keys) and all(0 <= k < 2 ** 64 for k in keys.values())
    assert fabstart.seed_of(1234, 3, 2) == keys[(3, 2)]  # a function: the same key again
    assert fabstart.seed_of(1235, 3, 2) != keys[(3, 2)]
    # the documented formula, restated
    z =(0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03) & (2 ** 64 - 1)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
    assert fabstart.seed_of(0, 0, 1) == z ^ (z >> 31)


# ---- the start -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_every_start_lies_within_half_the_radius(metric, dtype):
    """||start - x0||_p <= min(res, eps) / 2 up to rounding.  With u the unit roundoff of the dtype: d_i = fl(fl(m t_i) / n) / 2 carries two
    roundings and n one (its double sum adds D 2^-53 at most), so |d_i| <= (m |t_i| / n_exact) (1 + 4 u) / 2, whose norm is (m / 2)(1 + 4 u);
    the sum x0_i + d_i is rounded once more, by at most u (its value is at most 1 after the clamp, which never moves a coordinate away
    from x0_i in [0, 1]): u, sqrt(D) u or D u on the norm.  The difference start - x0 is taken in float64, exactly."""
    from eeadv import fabstart
    u = U24 if dtype == torch.float32 else 2.0 ** -53
    B, shape = 6, (3, 5, 5)
    D = 75
    g = torch.Generator().manual_seed(4)
    x0 = torch.rand(B, *shape, generator=g, dtype=torch.float64).to(dtype)
    x0[0, 0], x0[0, 1] = 0.0, 1.0  # rows on the box faces
    eps = EPS[metric]
    res = torch.tensor([float("inf"), eps / 3, 0.0, eps * 4, eps, eps / 7], dtype=dtype)
    t = torch.from_numpy(fabstart.draw(77, B, D, metric)).view(B, *shape)
    t[5] = 0.0  # a draw without a direction: the row stays at x0
    x = fabstart.start(x0, res, eps, t, metric)
    assert x.dtype == dtype and x.shape == x0.shape and bool((x >= 0).all()) and bool((x <= 1).all())
    assert torch.equal(x[2], x0[2]) and torch.equal(x[5], x0[5])  # m = 0, n = 0
    m = torch.minimum(res, torch.full_like(res, eps)).double()
    slack = {"Linf": u, "L2": D ** 0.5 * u, "L1": D * u}[metric]
    for b in range(B):
        d = S.dist((x[b].double() - x0[b].double()).flatten().numpy(), metric)
        assert d <= float(m[b]) / 2 * (1 + 4 * u) + slack, (b, d, float(m[b]))
    moved = [b for b in (1, 3, 4) if S.dist((x[b].double() - x0[b].double()).flatten().numpy(), metric) >= 0.45 * float(m[b])]
    assert moved == [1, 3, 4]  # rows inside the box reach (nearly) the radius: the bound is not vacuous
    # against the one-sample float64 reference
    if dtype == torch.float64:
        for b in range(B):
            want = S.start_row(x0[b].flatten().numpy(), float(res[b]), eps, t[b].double().flatten().numpy(), metric)
            assert np.abs(x[b].flatten().numpy() - want).max() <= (D + 8) * EPS64 * max(1.0, eps)


def test_float32_linf_host_start_from_the_host_draw_is_reproducible_in_numpy():
    """The float32 Linf start, operation by operation in numpy float32: what the kernel is held to on the GPU (tests/test_gpu_fab_restarts.py)
    is what the host path computes."""
    from eeadv import fabstart
    B, D, eps = 4, 75, np.float32(8 / 255)
    t = fabstart.draw(3, B, D, "Linf")
    x0 = np.random.default_rng(0).random((B, D)).astype(np.float32)
    res = np.array([np.inf, 0.01, 0.5, 0.0], np.float32)
    n = np.abs(t).max(axis=1)
    m = np.minimum(res, eps)
    want = np.clip(x0 + ((m[:, None] * t) / n[:, None]) * np.float32(0.5), np.float32(0), np.float32(1)).astype(np.float32)
    got = fabstart.start(torch.from_numpy(x0), torch.from_numpy(res), float(eps), torch.from_numpy(t), "Linf").numpy()
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()


# ---- the four host runs ------------------------------------------------------------------------------------------------------------------
def _host_run(kind, metric, m, x0, y, t, n_iter, **kw):
    import utils.attacks as A
    if kind == "U":
        return A._fab_u_l1_host(m, x0, y, n_iter, **kw) if metric == "L1" else A._fab_u_host(m, x0, y, n_iter, norm=metric, **kw)
    return A._fab_l1_host(m, x0, y, t, n_iter, **kw) if metric == "L1" else A._fab_host(m, x0, y, t, n_iter, norm=metric, **kw)


def _host_iteration(kind, metric, m, x, x0, y, t, adv, res):
    import utils.attacks as A
    if kind == "U":
        return host_iteration(metric, m, x, x0, y, adv, res)
    if metric == "L1":
        return A._fab_l1_host_iteration(m, x, x0, y, t, adv, res)
    return A._fab_host_iteration(m, x, x0, y, t, adv, res, norm=metric)


def _case(kind):
    m, x0, K = _mlp_case()
    with torch.no_grad():
        order = torch.sort(m(x0), dim=1, descending=True, stable=True)[1]
    y, t = order[:, 0].clone(), (order[:, 1].clone() if kind == "T" else None)
    noise = torch.randn(2, *x0.shape, generator=torch.Generator().manual_seed(8), dtype=torch.float64)
    return m, x0, K, y, t, noise


_CHAINS = {}


def _chain(kind, metric):
    """The reference's chain of 3 restarts of 3 iterations, computed once per (kind, metric) and left unchanged."""
    if (kind, metric) not in _CHAINS:
        m, x0, K, y, t, noise = _case(kind)
        _CHAINS[(kind, metric)] = S.chain(m, x0, y, t, 3, 3, EPS[metric], noise, metric)
    return _CHAINS[(kind, metric)]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", ["T", "U"])
def test_one_restart_is_the_call_without_the_argument(kind, metric):
    m, x0, K, y, t, noise = _case(kind)
    a0, r0 = _host_run(kind, metric, m, x0, y, t, 3)
    a1, r1 = _host_run(kind, metric, m, x0, y, t, 3, n_restarts=1)
    assert a0.numpy().tobytes() == a1.numpy().tobytes() and r0.numpy().tobytes() == r1.numpy().tobytes()
    tr0, tr1 = [], []
    _host_run(kind, metric, m, x0, y, t, 3, trace=tr0)
    _host_run(kind, metric, m, x0, y, t, 3, trace=tr1, n_restarts=1, seed=5, eps=EPS[metric])
    assert len(tr0) == len(tr1) == 3 and all(set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a) for a, b in zip(tr0, tr1))
    with pytest.raises(ValueError, match="n_restarts"):
        _host_run(kind, metric, m, x0, y, t, 3, n_restarts=0)
    with pytest.raises(ValueError, match="eps"):
        _host_run(kind, metric, m, x0, y, t, 3, n_restarts=2, seed=1)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", ["T", "U"])
def test_three_restarts_against_the_reference_chain(kind, metric):
    """Restart by restart: the host start from the reference's res equals the reference's start point to (D + 8) 2^-52 (the float64 sum of
    the norm in another order, four roundings); then every host iteration from the reference's recorded state, at the tolerances of
    tests/test_fab_u_host.py (which are those of the metric's own FAB-T host test).  Then the host run itself: its trace links up - every
    restart starts where fabstart.start puts it from the res the run had, res never grows - and its result is no worse than one run's."""
    from eeadv import fabstart
    m, x0, K, y, t, noise = _case(kind)
    eps, n_iter, D = EPS[metric], 3, x0[0].numel()
    bound = (D + K + 8) * EPS64
    adv_ref, res_ref, restarts = _chain(kind, metric)
    assert len(restarts) == 3 and torch.equal(restarts[0]["x_start"], x0) and bool(torch.isinf(restarts[0]["res_in"]).all())
    n_adv = 0
    for r, rs in enumerate(restarts):
        if r:
            got = fabstart.start(x0, rs["res_in"], eps, noise[r - 1], metric)
            assert float((got - rs["x_start"]).abs().max()) <= (D + 8) * EPS64 * max(1.0, eps), r
            radius = torch.minimum(rs["res_in"], torch.full_like(rs["res_in"], eps)) / 2
            for b in range(x0.shape[0]):
                assert S.dist((rs["x_start"][b] - x0[b]).flatten().numpy(), metric) <= float(radius[b]) * (1 + 8 * EPS64) + D * EPS64
            assert not torch.equal(rs["x_start"], x0)
        for i, e in enumerate(rs["trace"]):
            x, adv, res, info = _host_iteration(kind, metric, m, e["x_in"], x0, y, t, e["adv_in"], e["res_in"])
            if kind == "U":
                assert info["best_k"].tolist() == e["best_k"].tolist(), (r, i)
            assert info["pred"].tolist() == e["pred"].tolist() and info["is_adv"].tolist() == e["is_adv"].tolist(), (r, i)
            assert info["improved"].tolist() == e["improved"].tolist() and info["enabled"].tolist() == e["enabled"].tolist(), (r, i)
            assert info["s1"].tolist() == e["s1"].tolist() and info["s2"].tolist() == e["s2"].tolist(), (r, i)
            assert bool(((info["df"] - e["df"]).abs() <= bound * (e["zt"].abs() + e["zy"].abs())).all()), (r, i)
            wmax = e["w"].flatten(1).abs().max(dim=1)[0].view(-1, 1)
            assert bool(((info["w"] - e["w"].flatten(1)).abs() <= bound * wmax).all()), (r, i)
            CHECKS[metric](info, x, adv, res, e, x0, bound, (r, i))
            n_adv += int(e["is_adv"].sum())
    assert n_adv > 0
    # the reference's own chain: res is carried and never grows
    for a, b in zip(restarts[:-1], restarts[1:]):
        assert torch.equal(a["trace"][-1]["res"], b["res_in"]) and bool((b["res_in"] <= a["res_in"]).all())
    # the host run
    trace = []
    adv3, res3 = _host_run(kind, metric, m, x0, y, t, n_iter, n_restarts=3, noise=noise, eps=eps, trace=trace)
    adv1, res1 = _host_run(kind, metric, m, x0, y, t, n_iter)
    marks = [i for i, e in enumerate(trace) if "restart" in e]
    assert marks == [n_iter, 2 * n_iter + 1] and len(trace) == 3 * n_iter + 2
    assert [int(trace[i]["restart"]) for i in marks] == [1, 2]
    for i in marks:
        before, mark, after = trace[i - 1], trace[i], trace[i + 1]
        assert torch.equal(mark["res_in"], before["res"])
        assert torch.equal(mark["x_start"], fabstart.start(x0, before["res"], eps, noise[int(mark["restart"]) - 1], metric))
        assert bool((after["res"] <= mark["res_in"]).all())
    assert torch.equal(trace[n_iter - 1]["res"], res1) and torch.equal(trace[n_iter - 1]["adv"], adv1)  # restart 0 is the run of today
    assert bool((res3 <= res1).all())
    same = res3 == res1
    assert torch.equal(adv3[same], adv1[same])
    assert torch.equal(trace[-1]["res"], res3) and torch.equal(trace[-1]["adv"], adv3)
    # and the reference's result, to the loosest per-iteration tolerance above (free-running: only where the flags agree all the way)
    assert torch.equal(torch.isfinite(res3), torch.isfinite(res_ref))


def test_seeded_host_restarts_use_the_host_draw(cpu_plumbing):
    """seed in place of noise: restart r of target index j starts from fabstart.draw under seed_of(seed, j, r) - float32, Linf."""
    import utils.attacks as A
    from eeadv import fabstart
    m, x0, K, y, t, _ = _case("T")
    m32, x32 = m.float(), x0.float()
    trace = []
    A._fab_host(m32, x32, y, t, 2, trace=trace, n_restarts=2, seed=99, eps=0.05, target_index=4)
    mark = next(e for e in trace if "restart" in e)
    draw = torch.from_numpy(fabstart.draw(fabstart.seed_of(99, 4, 1), x32.shape[0], x32[0].numel(), "Linf")).view(x32.shape)
    assert torch.equal(mark["x_start"], fabstart.start(x32, mark["res_in"], 0.05, draw, "Linf"))
    other = []
    A._fab_host(m32, x32, y, t, 2, trace=other, n_restarts=2, seed=99, eps=0.05, target_index=5)
    assert not torch.equal(next(e for e in other if "restart" in e)["x_start"], mark["x_start"])


def test_public_doors_take_restarts_on_the_host(cpu_plumbing):
    import utils.attacks as A
    m, x0, K, y, _, _ = _case("U")
    m32, x32 = m.float(), x0.float()
    for door, kw in ((A.FAB, {}), (A.FAB_L1, {}), (A.FAB_T, dict(nclass=K)), (A.FAB_T_L1, dict(nclass=K))):
        eps = 3.0 if door in (A.FAB_L1, A.FAB_T_L1) else 0.05
        one = door(m32, Args(epsilon=eps), x32, y, n_iter=3, **kw)
        again = door(m32, Args(epsilon=eps), x32, y, n_iter=3, n_restarts=1, seed=7, **kw)
        assert all(torch.equal(a, b) for a, b in zip(one, again))
        three = door(m32, Args(epsilon=eps), x32, y, n_iter=3, n_restarts=3, seed=7, **kw)
        same = door(m32, Args(epsilon=eps), x32, y, n_iter=3, n_restarts=3, seed=7, **kw)
        assert all(torch.equal(a, b) for a, b in zip(three, same))  # the seed is all that enters the draws
        assert bool((three[2] <= one[2]).all()) and torch.equal(three[1], ~(three[2] <= eps))
        with pytest.raises(ValueError, match="n_restarts"):
            door(m32, Args(epsilon=eps), x32, y, n_iter=3, n_restarts=0, **kw)


def test_cascade_stages_and_the_dispatch_read_fab_restarts(cpu_plumbing, monkeypatch):
    import utils.attacks as A
    from eeadv import cascade, trainer
    seen = []
    monkeypatch.setattr(A, "FAB_T", lambda *a, **kw: seen.append(("T", kw)) or (a[2], torch.ones(len(a[2]), dtype=torch.bool), None))
    monkeypatch.setattr(A, "FAB_T_L1", lambda *a, **kw: seen.append(("T1", kw)) or (a[2], torch.ones(len(a[2]), dtype=torch.bool), None))
    monkeypatch.setattr(A, "FAB", lambda *a, **kw: seen.append(("U", kw)) or (a[2], None, None))
    x, y = torch.rand(2, 1, 4, 4), torch.zeros(2, dtype=torch.int64)
    for restarts, want in ((None, {}), (1, {}), (3, {"n_restarts": 3})):
        args = Args(epsilon=0.1, fab_iters=2)
        if restarts is not None:
            args.fab_restarts = restarts
        del seen[:]
        dict(cascade.default_stages(args, 2, 10))["FAB-T"](None, args, x, y, None)
        dict(cascade.l1_stages(args, 2, 10))["FAB-T-L1"](None, args, x, y, None)
        args.attack_method, args.method_name = "FAB-U", "AT"
        trainer.attack_for_validation(None, args, x, y, "cpu", 2, 0.01, 10)
        assert [k for k, _ in seen] == ["T", "T1", "U"]
        for _, kw in seen:
            assert {k: v for k, v in kw.items() if k == "n_restarts"} == want
    args = Args(epsilon=0.1, fab_restarts=2)
    args.attack_method, args.method_name = "APGD-CE", "AT"
    with pytest.raises(NotImplementedError, match="fab_restarts"):
        trainer.fab_restarts_for(args)
    args.fab_restarts = 0
    with pytest.raises(ValueError, match="fab_restarts"):
        trainer.fab_restarts_for(args)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_start_launch():
    import eeadv._native as n
    from eeadv import ops
    L = n.lib
    assert "ee_fab_start_f32" in n.SIGNATURES and hasattr(L, "ee_fab_start_f32") and hasattr(ops, "fab_start_")
    assert L.ee_prof_read(29, None, None) != -2 and L.ee_prof_read(30, None, None) == -2  # no new timing family: it records under EE_K_FAB_STEP
    p = ctypes.c_void_p(4096)
    names = ("x", "x0", "res", "noise", "B", "D", "eps", "metric", "seed", "path", "stream")
    ok = (p, p, p, None, 2, 8, 0.1, 0, 5, 0, None)

    def call(**kw):
        a = dict(zip(names, ok))
        a.update(kw)
        return L.ee_fab_start_f32(*[a[k] for k in names])

    for name in ("x", "x0", "res"):
        assert call(**{name: None}) == -1, name
    assert call(B=-1) == -2 and call(D=0) == -2 and call(eps=-0.1) == -2 and call(eps=float("nan")) == -2
    assert call(metric=3) == -2 and call(metric=-1) == -2 and call(path=3) == -2 and call(path=-1) == -2
    assert call(D=12289, path=1) == -3  # the resident path ends at 3*64*64
    assert call(B=0, x=None, x0=None, res=None) == 0  # an empty batch launches nothing
    assert call(x=ctypes.c_void_p(4098)) == -4 and call(noise=ctypes.c_void_p(4098)) == -4
    x = torch.rand(2, 8)
    with pytest.raises(n.EEError):
        ops.fab_start_(x.clone(), x, torch.ones(2), 0.1, "Linf")
    with pytest.raises(ValueError, match="metric"):
        ops.fab_start_(x.clone(), x, torch.ones(2), 0.1, "L3")


# ---- drivers ---------------------------------------------------------------------------------------------------------------------------
def test_mnist_driver_runs_untargeted_fab_with_restarts_on_the_host(tmp_path):
    r = _mnist(tmp_path, "--attack_method", "FAB-U", "--fab_iters", "2", "--fab_restarts", "2")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    logs = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path)) for f in fs if f.startswith("log")]
    text = r.stdout + "".join(open(f).read() for f in logs)
    assert re.search(r"^ \* FAB-U: K = 10 classes, 10 backward passes per iteration, 2 iterations, 2 restarts$", text, flags=re.M)
    assert text.index("2 restarts") < text.index("Test_clean")  # before the first batch
    clean = re.findall(r"^ \* Clean Prec@1 ([\d.]+)", text, flags=re.M)
    adv = re.findall(r"^ \* Adv Prec@1 ([\d.]+) Prec@5 ([\d.]+)$", text, flags=re.M)
    assert len(clean) >= 1 and len(clean) == len(adv)
    for c1, (a1, _) in zip(clean, adv):
        assert float(a1) <= float(c1)


def test_mnist_driver_stops_on_restarts_for_a_method_without_fab(tmp_path):
    r = _mnist(tmp_path, "--attack_method", "APGD-CE", "--fab_restarts", "2")
    assert r.returncode != 0 and "NotImplementedError" in r.stderr and "fab_restarts" in r.stderr
    assert "Adv Prec@1" not in r.stdout
