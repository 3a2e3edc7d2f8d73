"""CPU: APGD's schedule, the ABI of its kernels, the closed-form DLR gradients of the test reference, and the plain-torch host path of
utils.attacks.APGD / APGD_T against tests/apgd_reference.py bit for bit in float64."""
import ctypes

import pytest
import torch

import apgd_reference as R
from tiny_models import Args, TinyNet


def _checkpoints(sched):
    """1-based iterations after which a checkpoint falls, and the window lengths."""
    return [i + 1 for i, k in enumerate(sched) if k], [k for k in sched if k]


def test_schedule():
    from eeadv import engine
    for n, want_at in ((100, [22, 41, 57, 70, 80, 87, 93, 99]), (10, [2, 3, 4, 5, 6, 7, 8, 9, 10])):
        at, _ = _checkpoints(engine.apgd_schedule(n))
        assert at == want_at
        assert sorted(i + 1 for i in R.schedule(n)) == want_at
    assert _checkpoints(engine.apgd_schedule(100))[1] == [22, 19, 16, 13, 10, 7, 6, 6]
    # n = 1: k = max(int(0.22), 1) = 1 -> the only iteration closes a window of 1
    assert engine.apgd_schedule(1) == [1]
    # n = 17: k = int(3.74) = 3, n_min = max(int(1.02), 1) = 1, dec = max(int(0.51), 1) = 1: windows 3, 2, then 1 for ever:
    # checkpoints after 3, 5, 6, 7, ..., 17
    assert engine.apgd_schedule(17) == [0, 0, 3, 0, 2] + [1] * 12
    assert R.schedule(17) == {i: k for i, k in enumerate([0, 0, 3, 0, 2] + [1] * 12) if k}
    with pytest.raises(ValueError):
        engine.apgd_schedule(0)


def test_abi_of_the_apgd_kernels():
    import eeadv._native as n
    L = n.lib
    for name in ("ee_apgd_step_f32", "ee_apgd_loss_f32", "ee_apgd_book_f32", "ee_apgd_select_f32"):
        assert name in n.SIGNATURES and hasattr(L, name)
    p = ctypes.c_void_p(4096)
    assert L.ee_apgd_step_f32(None, p, p, p, p, p, 2, 8, 0.1, None) == -1 and L.ee_apgd_step_f32(p, p, p, p, None, p, 2, 8, 0.1, None) == -1
    assert L.ee_apgd_step_f32(p, p, p, p, p, None, 2, 8, 0.1, None) == -1
    assert L.ee_apgd_step_f32(None, None, None, None, None, None, 0, 8, 0.1, None) == 0  # n = 0
    assert L.ee_apgd_step_f32(p, p, p, p, p, p, -1, 8, 0.1, None) == -2
    assert L.ee_apgd_step_f32(ctypes.c_void_p(4098), p, p, p, p, p, 2, 8, 0.1, None) == -4
    assert L.ee_apgd_loss_f32(None, p, p, 4, 10, 0, p, p, p, None) == -1 and L.ee_apgd_loss_f32(p, p, p, 4, 10, 0, None, p, p, None) == -1
    assert L.ee_apgd_loss_f32(p, p, None, 4, 10, 2, p, p, p, None) == -1  # the targeted loss needs targets
    assert L.ee_apgd_loss_f32(p, p, p, 4, 10, 3, p, p, p, None) == -2 and L.ee_apgd_loss_f32(p, p, p, 4, 0, 0, p, p, p, None) == -2
    assert L.ee_apgd_loss_f32(p, p, p, 4, 2, 1, p, p, p, None) == -3  # dlr: K >= 3
    assert L.ee_apgd_loss_f32(p, p, p, 4, 3, 2, p, p, p, None) == -3  # dlr_t: K >= 4
    assert L.ee_apgd_book_f32(p, p, None, p, p, p, 10, 4, None) == -1 and L.ee_apgd_book_f32(p, p, p, p, p, None, 10, 4, None) == -1
    assert L.ee_apgd_book_f32(p, p, p, p, p, p, 0, 4, None) == -2
    assert L.ee_apgd_select_f32(p, p, p, p, p, None, p, 4, 8, None) == -1 and L.ee_apgd_select_f32(p, p, p, p, p, p, None, 4, 8, None) == -1
    assert L.ee_apgd_select_f32(p, p, p, p, p, p, p, -1, 8, None) == -2


@pytest.mark.parametrize("kind", ["dlr", "dlr_t"])
def test_reference_dlr_against_autograd_on_the_closed_form(kind):
    g = torch.Generator().manual_seed(3)
    for K in (4, 10, 200):
        z = (3 * torch.randn(16, K, generator=g, dtype=torch.float64))
        y = torch.randint(0, K, (16,), generator=g)
        t = torch.fmod(y + torch.randint(1, K, (16,), generator=g), K)
        for b in range(16):
            zb = z[b].clone().requires_grad_()
            s, _ = torch.sort(zb, descending=True)  # no ties in a random row: the sorted VALUES carry the gradient
            if kind == "dlr":
                other = s[1] if int(torch.argmax(zb)) == int(y[b]) else s[0]
                want = -(zb[y[b]] - other) / ((s[0] - s[2]) + R.TINY.double())
            else:
                want = -(zb[y[b]] - zb[t[b]]) / ((s[0] - (s[2] + s[3]) * 0.5) + R.TINY.double())
            (gw,) = torch.autograd.grad(want, [zb])
            loss, grad = R.row_loss_grad(z[b], y[b], kind, t[b])
            assert torch.allclose(loss, want.detach(), rtol=1e-14, atol=0)
            assert torch.allclose(grad, gw, rtol=1e-12, atol=1e-15)
            assert torch.equal(grad != 0, gw != 0)
            zr = z[b].clone().requires_grad_()
            (ga,) = torch.autograd.grad(R.row_loss(zr, y[b], kind, t[b]), [zr])
            assert torch.allclose(ga, gw, rtol=1e-12, atol=1e-15)


def test_tie_rule():
    """Ties go to the lower index: row [2, 5, 5, 5, 1] has the order 1, 2, 3, 0, 4."""
    z = torch.tensor([2.0, 5.0, 5.0, 5.0, 1.0], dtype=torch.float64)
    assert R.order_row(z) == [1, 2, 3, 0, 4]
    assert R.pred_row(z, 1) and not R.pred_row(z, 2) and not R.pred_row(z, 3)
    # dlr with y = 1 (= p1): o = p2 = 2, numerator 0, denominator z_p1 - z_p3 = 0 + 1e-12f
    loss, grad = R.row_loss_grad(z, 1, "dlr")
    assert float(loss) == 0.0 and abs(float(grad[1]) + float(grad[2])) <= 1e-12 * float(grad[2]) and float(grad[2]) == 1.0 / float(R.TINY.double())
    # y = 2: p1 = 1 is another class, so o = 1; the label is not the prediction
    loss, _ = R.row_loss_grad(z, 2, "dlr")
    assert float(loss) == 0.0
    # dlr_t with y = 0, t = 4: -(2 - 1) / (5 - (5 + 2)/2 + 1e-12f); p3 = 3, p4 = 0
    loss, grad = R.row_loss_grad(z, 0, "dlr_t", 4)
    d = 1.5 + float(R.TINY.double())
    assert float(loss) == -1.0 / d
    assert float(grad[1]) == 1.0 / (d * d) and float(grad[2]) == 0.0 and float(grad[3]) == -0.5 / (d * d)
    assert float(grad[0]) == -1.0 / d - 0.5 / (d * d) and float(grad[4]) == 1.0 / d
    import utils.attacks as A
    zb = z.view(1, -1)
    for kind, y, t in (("dlr", 1, None), ("dlr", 2, None), ("dlr_t", 0, 4), ("ce", 3, None)):
        tt = None if t is None else torch.tensor([t])
        assert torch.equal(A._apgd_row_losses(zb, torch.tensor([y]), kind, tt)[0], R.row_loss(z, y, kind, t))


SEED, B, HW, NCLS, EPS, N_ITER = 0, 6, 8, 10, 0.03, 10


def _problem(dtype=torch.float64):
    from eeadv import runtime
    runtime.allow_cpu_plumbing(True)
    torch.manual_seed(SEED)
    model = TinyNet(3, HW, NCLS, seed=SEED).to(dtype).eval()
    x0 = torch.rand(B, 3, HW, HW, dtype=dtype)
    with torch.no_grad():
        y = model(x0).argmax(1)
    y[0] = (y[0] + 1) % NCLS  # one sample starts misclassified
    noise = torch.zeros_like(x0).uniform_(-EPS, EPS)
    return model, x0, y, noise


@pytest.fixture(scope="module")
def host_problem():
    yield _problem()
    from eeadv import runtime
    runtime.allow_cpu_plumbing(False)


def _equal_traces(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        for key in ("x", "x_old", "g", "loss", "pred", "step", "loss_best", "f_prev", "loss_best_last", "inc", "reduced_last", "robust",
                    "x_best", "g_best", "x_best_adv"):
            assert torch.equal(a[key], b[key].to(a[key].dtype)), (i, key)
        if i:
            for key in ("improved", "fooled", "reduced"):
                assert a[key].tolist() == b[key], (i, key)


@pytest.mark.parametrize("kind", ["ce", "dlr", "dlr_t"])
def test_host_path_equals_the_reference_bit_for_bit(host_problem, kind):
    import utils.attacks as A
    model, x0, y, noise = host_problem
    t = torch.fmod(y + 3, NCLS) if kind == "dlr_t" else None
    x_init = A._uniform_start(x0, EPS, noise)
    assert torch.equal(x_init, torch.clamp(x0 + noise, 0, 1))
    want_x, want_r, want_l, want_trace = R.run(model, x0, x_init, y, N_ITER, EPS, kind, t)
    trace = []
    got_x, got_r, got_l = A._apgd_host(model, x0, x_init, y, N_ITER, EPS, kind, t, trace=trace)
    _equal_traces(trace, want_trace)
    assert torch.equal(got_x, want_x) and torch.equal(got_r, want_r) and torch.equal(got_l, want_l)
    xa, rb = A.APGD(model, Args(epsilon=EPS), x0, y, N_ITER, loss=kind, y_target=t, noise=noise)
    assert torch.equal(xa, want_x) and torch.equal(rb, want_r) and xa.dtype == torch.float64
    assert sum(1 for e in want_trace[1:] if e["k"]) == 9
    if kind == "ce":
        # the run must exercise every branch of the bookkeeping (the seed was chosen for it)
        cps = [e for e in want_trace[1:] if e["k"]]
        assert any(o and not n for e in cps for o, n in zip(e["osc"], e["noimp"])), "no sample reduced by osc alone"
        assert any(n and not o for e in cps for o, n in zip(e["osc"], e["noimp"])), "no sample reduced by noimp alone"
        assert any(not r for e in cps for r in e["reduced"]), "no sample left unreduced at a checkpoint"
        assert any(f for e in want_trace[1:] for f in e["fooled"]) and not bool(want_r.all()), "no sample fooled"
        assert bool(want_r.any()), "every sample fooled"


def test_apgd_t_host(host_problem):
    import utils.attacks as A
    model, x0, y, noise = host_problem
    n_t = 3
    xa, rb = A.APGD_T(model, Args(epsilon=EPS), x0, y, N_ITER, NCLS, n_target_classes=n_t, noise=noise)
    x_init = torch.clamp(x0 + noise, 0, 1)
    with torch.no_grad():
        z0 = model(x0)
    want_x, want_r = x0.clone(), torch.ones(B, dtype=torch.bool)
    for j in range(1, n_t + 1):
        t = torch.tensor([R.order_row(z0[b])[j] for b in range(B)])
        xj, rj, _, _ = R.run(model, x0, x_init, y, N_ITER, EPS, "dlr_t", t)
        for b in range(B):
            if want_r[b] and not rj[b]:
                want_x[b] = xj[b]
        want_r &= rj
    assert torch.equal(xa, want_x) and torch.equal(rb, want_r)
    assert not bool(rb[0])  # misclassified from the start
    # the cap: at most nclass - 1 targets
    xa9, rb9 = A.APGD_T(model, Args(epsilon=EPS), x0, y, 2, NCLS, n_target_classes=50, noise=noise)
    xb9, rc9 = A.APGD_T(model, Args(epsilon=EPS), x0, y, 2, NCLS, n_target_classes=NCLS - 1, noise=noise)
    assert torch.equal(xa9, xb9) and torch.equal(rb9, rc9)


def test_validation_dispatch(host_problem):
    from eeadv import trainer
    import utils.attacks as A
    model, x0, y, noise = host_problem
    torch.manual_seed(11)
    a = Args(epsilon=EPS, method_name="AT", attack_method="APGD-CE", random=True)
    xa = trainer.attack_for_validation(model, a, x0, y, "cpu", 4, 0.01, NCLS)
    torch.manual_seed(11)
    want, _ = A.APGD(model, a, x0, y, 4, "ce")
    assert torch.equal(xa, want)
    for method in ("APGD-T", "APGD"):
        a.attack_method = method
        out = trainer.attack_for_validation(model, a, x0, y, "cpu", 2, 0.01, NCLS)
        assert out.shape == x0.shape and float((out - x0).abs().max()) <= EPS + 1e-12
    a.method_name = "tar_AT"
    with pytest.raises(NotImplementedError):
        trainer.attack_for_validation(model, a, x0, y, "cpu", 2, 0.01, NCLS)
    a.method_name, a.attack_method = "AT", "AA"
    with pytest.raises(NotImplementedError):
        trainer.attack_for_validation(model, a, x0, y, "cpu", 2, 0.01, NCLS)


# ---- the engine's shared pieces: schedules, norm checks, cache keys --------------------------------------------------------------------
def _linf_schedule_as_it_was(n_iter):
    n_iter = int(n_iter)
    if n_iter < 1:
        raise ValueError("APGD needs n_iter >= 1")
    k, n_min, dec = max(int(0.22 * n_iter), 1), max(int(0.06 * n_iter), 1), max(int(0.03 * n_iter), 1)
    sched, since = [0] * n_iter, 0
    for i in range(n_iter):
        since += 1
        if since == k:
            sched[i], since, k = k, 0, max(k - dec, n_min)
    return sched


def _l1_schedule_as_it_was(n_iter):
    n_iter = int(n_iter)
    if n_iter < 1:
        raise ValueError("APGD needs n_iter >= 1")
    k, k_next = max(int(0.04 * n_iter), 1), max(int(0.06 * n_iter), 1)
    sched, since = [0] * n_iter, 0
    for i in range(n_iter):
        since += 1
        if since == k:
            sched[i], since, k = k, 0, k_next
    return sched


def test_both_schedules_are_the_literal_loops():
    from eeadv import engine
    for n in range(1, 301):
        assert engine.apgd_schedule(n) == _linf_schedule_as_it_was(n), n
        assert engine.apgd_l1_schedule(n) == _l1_schedule_as_it_was(n), n
    for schedule in (engine.apgd_schedule, engine.apgd_l1_schedule):
        for n in (0, -3):
            with pytest.raises(ValueError, match="APGD needs n_iter >= 1"):
                schedule(n)


def test_norm_messages(host_problem):
    import re
    from eeadv import engine
    import utils.attacks as A
    model, x0, y, noise = host_problem
    a = Args(epsilon=EPS)
    said = {what: re.escape("%s norm must be one of ['Linf', 'L2'], got 'L1'" % what) for what in ("APGD", "Square", "FAB")}
    with pytest.raises(ValueError, match=said["APGD"]):
        engine.apgd_loop(model, x0, x0, y, 2, EPS, "ce", norm="L1")
    with pytest.raises(ValueError, match=said["APGD"]):
        A.APGD(model, a, x0, y, 2, norm="L1")
    with pytest.raises(ValueError, match=said["Square"]):
        engine.square_loop(model, x0, y, 3, EPS, seed=1, norm="L1")
    with pytest.raises(ValueError, match=said["Square"]):
        A.Square(model, a, x0, y, 3, seed=1, norm="L1")
    with pytest.raises(ValueError, match=said["FAB"]):
        engine.fab_loop(model, x0, y, y, 2, EPS, norm="L1")
    with pytest.raises(ValueError, match=said["FAB"]):
        A.FAB_T(model, a, x0, y, NCLS, n_iter=2, norm="L1")


def test_cache_keys_keep_their_layout(host_problem, monkeypatch):
    """The key each captured loop hands to engine._cached, tuple for tuple as the loops built them before they shared a driver: tests and
    scripts read k[0] as the loop's name, k[5] of an "apgd" key as the norm, and look for "Linf" in a key."""
    from eeadv import engine
    model, x0, y, noise = host_problem

    class Seen(Exception):
        pass

    def cached(key, m, build):
        raise Seen(key)

    monkeypatch.setattr(engine, "_cached", cached)
    shape, mid, dev = tuple(x0.shape), id(model), x0.device.index
    calls = [
        (lambda: engine.pgd_loop(model, x0, x0.clone(), engine.LossSpec(engine.CE_SUM, y), 6, 0.01, EPS, use_graph=True),
         ("pgd", mid, model.training, shape, engine.CE_SUM, tuple(y.shape), y.dtype, 0.01, float(EPS), 1, 0.0, 1.0, dev, 6)),
        (lambda: engine.apgd_loop(model, x0, x0, y, 6, EPS, "ce", use_graph=True),
         ("apgd", mid, model.training, shape, "ce", "Linf", 6, float(EPS), dev, 6, 1)),
        (lambda: engine.apgd_loop(model, x0, x0, y, 34, EPS, "dlr", use_graph=True, eot_iter=4, norm="L2"),
         ("apgd", mid, model.training, shape, "dlr", "L2", 34, float(EPS), dev, 2, 4)),
        (lambda: engine.apgd_l1_loop(model, x0, x0, y, 34, 1.5, "ce", use_graph=True, path="streaming"),
         ("apgd_l1", mid, model.training, shape, "ce", 34, 1.5, dev, 2, "streaming")),
        (lambda: engine.square_loop(model, x0, y, 40, EPS, seed=1, use_graph=True),
         ("square", mid, model.training, shape, 40, float(EPS), dev, 16, "Linf", "auto")),
        (lambda: engine.square_loop(model, x0, y, 5, 0.5, seed=1, use_graph=True, norm="L2", path="resident"),
         ("square", mid, model.training, shape, 5, 0.5, dev, 4, "L2", "resident")),
        (lambda: engine.fab_loop(model, x0, y, y, 6, EPS, use_graph=True),
         ("fab", mid, model.training, shape, "auto", dev, 6, "Linf")),
        (lambda: engine.fab_loop(model, x0, y, y, 34, EPS, use_graph=True, path="resident", norm="L2"),
         ("fab", mid, model.training, shape, "resident", dev, 2, "L2")),
    ]
    for call, want in calls:
        with pytest.raises(Seen) as seen:
            call()
        (key,) = seen.value.args
        assert key == want and [type(v) for v in key] == [type(v) for v in want]
