"""CPU: APGD in the L1 threat model - the reference's projection is the Euclidean projection (variational inequality), the plain-torch host
path of utils.attacks equals tests/apgd_l1_reference.py bit for bit in float64, the ball-and-box invariant in float32, both branches of
the checkpoint rule, and the doors.

The invariant: x in [0,1] and ||x - x0||_1 <= eps + D 2^-23, summed exactly.  The projection solves h(lambda) = eps
on the f32 values a_i, lo_i; each written element then carries the rounding of a_i - cut_i and of x0_i + s_i d_i (results in [0,1]: at
most 2^-25 each, D 2^-24 in all), and the rounding of lambda to f32 moves h by |A| ulp(lambda) / 2: under D 2^-24 more for lambda < 1,
and for lambda in [2^k, 2^(k+1)) as long as |A| <= D 2^-k - which the start x0 + n (n standard normal) and every step here meet."""
import math

import numpy as np
import pytest
import torch

import apgd_l1_reference as L1
from tiny_models import Args, TinyNet

SEED, B, HW, NCLS, EPS, N_ITER = 2, 4, 8, 10, 6.0, 12
D = 3 * HW * HW


@pytest.fixture()
def cpu_plumbing():
    from eeadv import runtime
    runtime.allow_cpu_plumbing(True)
    yield
    runtime.allow_cpu_plumbing(False)


def _problem(dtype=torch.float64, seed=SEED):
    torch.manual_seed(seed)
    model = TinyNet(3, HW, NCLS, seed=seed).to(dtype).eval()
    x0 = torch.rand(B, 3, HW, HW, dtype=dtype)
    x0[:, :, 0, :] = 0.0  # elements on both ends of the box
    x0[:, :, 1, :] = 1.0
    with torch.no_grad():
        y = model(x0).argmax(1)
    y[0] = (y[0] + 1) % NCLS  # one sample starts misclassified
    noise = torch.randn(B, 3, HW, HW, dtype=dtype)
    return model, x0, y, noise


@pytest.mark.parametrize("case", ["inactive", "active", "eps0"])
def test_the_reference_projection_is_optimal(case):
    """z* = P(u) is feasible and (u - z*).(z - z*) <= 1e-12 for a few thousand random feasible z."""
    r = np.random.RandomState(7)
    n = 40
    for trial in range(4):
        x0 = r.rand(n)
        x0[::6], x0[1::6] = 0.0, 1.0
        u = x0 + r.randn(n) * (0.02 if case == "inactive" else 1.0)
        eps = {"inactive": 5.0, "active": 0.5 + trial, "eps0": 0.0}[case]
        z, info = L1.project_row(u, x0, eps)
        assert z.min() >= 0 and z.max() <= 1 and math.fsum(np.abs(z - x0).tolist()) <= eps + 1e-12
        assert (info["lam"] > 0) == (case != "inactive")
        if case == "inactive":
            assert np.array_equal(z, np.clip(u, 0, 1))
        if case == "eps0":
            assert np.array_equal(z, x0)
        worst = -np.inf
        for _ in range(3000):
            d = r.randn(n) * r.rand()
            if eps == 0:
                d[:] = 0
            else:
                d *= min(1.0, eps * r.rand() ** 0.2 / np.abs(d).sum())
            zf = np.clip(x0 + d, 0, 1)  # clipping towards x0's box only shrinks |zf - x0|
            assert np.abs(zf - x0).sum() <= eps + 1e-12
            worst = max(worst, float(np.dot(u - z, zf - z)))
        # vertices of the ball that lie in the box as well
        for i in range(n):
            for s in (-1.0, 1.0):
                zf = x0.copy()
                zf[i] = np.clip(x0[i] + s * eps, 0, 1)
                worst = max(worst, float(np.dot(u - z, zf - z)))
        print(case, trial, "largest (u - z*).(z - z*):", worst)
        assert worst <= 1e-12


FLOAT_KEYS = ("x", "g", "loss", "step", "topk", "loss_best", "x_best", "g_best", "x_best_adv")


@pytest.mark.parametrize("kind", ["ce", "dlr_t"])
def test_host_path_equals_the_reference_in_float64(cpu_plumbing, kind):
    import utils.attacks as A
    from eeadv import engine
    assert sum(1 for k in engine.apgd_l1_schedule(N_ITER) if k) >= 2
    assert {i: k for i, k in enumerate(engine.apgd_l1_schedule(100)) if k} == L1.schedule(100) and L1.schedule(100)[3] == 4 and L1.schedule(100)[9] == 6
    model, x0, y, noise = _problem()
    t = torch.fmod(y + 3, NCLS) if kind == "dlr_t" else None
    x_init = x0 + noise
    want_x, want_r, want_l, want = L1.run(model, x0, x_init, y, N_ITER, EPS, kind, t)
    trace = []
    got_x, got_r, got_l = A._apgd_l1_host(model, x0, x_init, y, N_ITER, EPS, kind, t, trace=trace)
    assert len(trace) == len(want) == N_ITER + 1
    for i, (a, b) in enumerate(zip(trace, want)):
        for key in FLOAT_KEYS:
            assert np.array_equal(a[key].numpy().reshape(b[key].shape), b[key]), (i, key)
        assert a["pred"].tolist() == b["pred"].tolist() and a["robust"].tolist() == b["robust"].tolist() and a["sp_old"].tolist() == b["sp_old"].tolist(), i
        lam = [f["lam"] for f in b["infos"]]
        assert a["lam"].tolist() == lam, (i, a["lam"].tolist(), lam)
        if i:
            for key in ("improved", "fooled", "reduced", "sp"):
                assert a[key].tolist() == b[key].tolist(), (i, key)
            assert a["m"].tolist() == [f["m"] for f in b["infos"]] and a["j"].tolist() == [f["j"] for f in b["infos"]], i
            assert a["tau"].tolist() == [float(f["tau"]) for f in b["infos"]], i
            assert np.array_equal(a["x_new"].numpy().reshape(B, -1), b["x_new"]), i
        for name in ("x", "x_best", "x_best_adv"):
            v = a[name].numpy().reshape(B, -1)
            assert v.min() >= 0 and v.max() <= 1 and L1.l1_excess(v, x0.numpy().reshape(B, -1), EPS) <= D * 2.0 ** -52, (i, name)
    assert np.array_equal(got_x.numpy(), want_x) and got_r.tolist() == want_r.tolist() and np.array_equal(got_l.numpy(), want_l)
    # a checkpoint takes both branches
    reds = [r for e in want[1:] if e["k"] for r in e["reduced"].tolist()]
    assert any(reds) and not all(reds)
    assert any(f["lam"] > 0 for e in want for f in e["infos"])
    # through the door: P(x0 + n) from the injected draw, then the same run
    xa, rb = A.APGD_L1(model, Args(epsilon=EPS), x0, y, N_ITER, loss=kind, y_target=t, noise=noise)
    assert torch.equal(xa, got_x) and torch.equal(rb, got_r) and xa.dtype == torch.float64


def test_float32_iterates_stay_in_the_ball_and_the_box(cpu_plumbing):
    import utils.attacks as A
    model, x0, y, noise = _problem(torch.float32)
    trace = []
    xa, _, _ = A._apgd_l1_host(model, x0, x0 + noise, y, N_ITER, EPS, "ce", trace=trace)
    c0 = x0.numpy().reshape(B, -1)
    worst = -np.inf
    for i, e in enumerate(trace):
        for name in ("x", "x_best", "x_best_adv"):
            v = e[name].numpy().reshape(B, -1)
            worst = max(worst, L1.l1_excess(v, c0, EPS))
            assert v.min() >= 0 and v.max() <= 1 and L1.l1_excess(v, c0, EPS) <= D * 2.0 ** -23, (i, name)
    print("largest ||x - x0||_1 - eps over the run:", worst)
    assert xa.dtype == torch.float32 and worst > -1e-3  # some iterate sits on the ball's surface


def test_a_non_finite_gradient_takes_no_gradient_step():
    r = np.random.RandomState(3)
    x0 = r.rand(30).astype(np.float32)
    x = np.clip(x0 + 0.01 * r.randn(30), 0, 1).astype(np.float32)
    for bad in (np.nan, np.inf):
        g = r.randn(30).astype(np.float32)
        g[4] = bad
        z, info = L1.step_row(x, g, x0, np.float32(1.0), np.float32(0.2), 1.0)
        assert not info["finite"] and np.array_equal(info["u"], x) and np.array_equal(z, x) and not np.isnan(z).any()


def test_apgd_t_l1_and_the_old_door(cpu_plumbing):
    import utils.attacks as A
    model, x0, y, noise = _problem(torch.float32)
    a = Args(epsilon=EPS)
    xt, rt = A.APGD_T_L1(model, a, x0, y, 6, NCLS, n_target_classes=2, noise=noise)
    c0 = x0.numpy().reshape(B, -1)
    assert rt.dtype == torch.bool and L1.l1_excess(xt.numpy().reshape(B, -1), c0, EPS) <= D * 2.0 ** -23
    with torch.no_grad():
        ok = model(xt).argmax(1) == y
    assert not bool(ok[~rt].any()) and torch.equal(xt[rt], x0[rt])
    with pytest.raises(ValueError, match="loss"):
        A._apgd_l1_host(model, x0, x0, y, 2, EPS, "mse")


def test_driver_dispatch_reaches_the_l1_doors(cpu_plumbing, monkeypatch):
    import utils.attacks as A
    from eeadv import trainer
    model, x0, y, _ = _problem(torch.float32)
    calls = []
    monkeypatch.setattr(A, "APGD_L1", lambda m, a, x, t, n, loss: (calls.append(("ce", loss, n)), (x + 0, torch.ones(B, dtype=torch.bool)))[1])
    monkeypatch.setattr(A, "APGD_T_L1", lambda m, a, x, t, n, k: (calls.append(("t", k, n)), (x + 0, torch.ones(B, dtype=torch.bool)))[1])
    for method, want in (("APGD-L1-CE", ["ce"]), ("APGD-L1-T", ["t"]), ("APGD-L1", ["ce", "t"])):
        a = Args(epsilon=EPS, method_name="AT", attack_method=method, random=True)
        assert method in trainer.EVAL_METHODS and method in trainer.L1_METHODS and method not in trainer.L2_METHODS
        calls.clear()
        out = trainer.attack_for_validation(model, a, x0, y, "cpu", 5, 0.1, NCLS)
        assert [c[0] for c in calls] == want and all(c[2] == 5 for c in calls) and out.shape == x0.shape
        assert trainer.norm_tag(a) == " [norm L1]" and trainer.eot_iter_for(a) == 1
        for norm in ("L2", "L1"):
            a.norm = norm
            with pytest.raises((ValueError, NotImplementedError), match="norm"):
                trainer.attack_for_validation(model, a, x0, y, "cpu", 5, 0.1, NCLS)
            with pytest.raises((ValueError, NotImplementedError), match="norm"):
                trainer.norm_tag(a)
        a.norm, a.eot_iter = None, 2
        with pytest.raises(NotImplementedError, match="eot_iter"):
            trainer.attack_for_validation(model, a, x0, y, "cpu", 5, 0.1, NCLS)
        a.eot_iter, a.method_name = None, "tar_AT"
        with pytest.raises(NotImplementedError, match="untargeted"):
            trainer.attack_for_validation(model, a, x0, y, "cpu", 5, 0.1, NCLS)
    # every other method's tag stays as it was
    assert trainer.norm_tag(Args(attack_method="APGD-CE")) == "" and trainer.norm_tag(Args(attack_method="APGD-CE", norm="L2")) == " [norm L2]"


def test_the_l1_run_through_the_dispatch(cpu_plumbing):
    from eeadv import trainer
    model, x0, y, _ = _problem(torch.float32)
    a = Args(epsilon=EPS, method_name="AT", attack_method="APGD-L1", random=True)
    torch.manual_seed(0)
    out = trainer.attack_for_validation(model, a, x0, y, "cpu", 4, 0.1, NCLS)
    assert L1.l1_excess(out.numpy().reshape(B, -1), x0.numpy().reshape(B, -1), EPS) <= D * 2.0 ** -23 and out.min() >= 0 and out.max() <= 1
