"""CPU: APGD in the L2 threat model - the plain-torch host path of utils.attacks against tests/apgd_l2_reference.py in float64, the ball
and box invariant of every iterate, the L2 start, Linf left as it was, and the --norm handling of the doors and the drivers.

eps = 0.5 throughout (the usual L2 radius for 32 x 32 images).  The invariant ||x - x0||_2 <= eps (1 + 4 u), u = 2^-23 (f32) or 2^-52 (f64),
is relative to eps, while the last operation of the step, x0 + d s2, rounds each element ABSOLUTELY (half an ulp of a value in [0, 1]:
up to u / 4).  The rescale leaves ||d s2|| <= eps (1 + 1.5 u) (n2, the quotient and the product are each rounded once); the D rounding
errors of the sum enter the norm as their projection onto the unit vector d / ||d||, a sum of independent terms of standard deviation
about u / 10 whatever D is, so five deviations are u / 2 absolute = u relative at eps = 0.5: 2.5 u in all, under the 4 u of the bound.  At a
radius of 0.03 the same absolute term would be 17 u relative: the bound is one for L2 radii of the usual size, not for tiny ones."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

import apgd_l2_reference as L2
from tiny_models import Args, TinyNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")

SEED, B, HW, NCLS, EPS, N_ITER = 2, 4, 8, 10, 0.5, 10
D = 3 * HW * HW
# every norm of the host path (torch's float64 sum of rounded squares) is within D 2^-53 relative of the reference's exactly summed one; the
# differences add up over the iterations at most linearly and pass through the classifier's gradient, for whose amplification 2^10 is
# allowed (TinyNet: one 3x3 convolution, a ReLU, a linear layer with weights of order 0.5 and 0.2)
TOL = D * N_ITER * 2.0 ** -53 * 2 ** 10


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


FLOAT_KEYS = ("x", "x_old", "g", "loss", "step", "loss_best", "f_prev", "loss_best_last", "x_best", "g_best", "x_best_adv")
EXACT_KEYS = ("pred", "inc", "reduced_last", "robust")


@pytest.mark.parametrize("kind", ["ce", "dlr", "dlr_t"])
def test_host_path_against_the_reference_in_float64(cpu_plumbing, kind):
    """B = 4, 3x8x8, 10 classes, 10 iterations - apgd_schedule(10) closes a checkpoint after iteration 2 and after every one from 3 on - in
    float64: every recorded quantity of _apgd_host(norm="L2") equals the per-sample restatement to TOL, the discrete ones exactly, and
    every iterate lies in the ball and the box."""
    import utils.attacks as A
    from eeadv import engine
    assert sum(1 for k in engine.apgd_schedule(N_ITER) if k) >= 2
    model, x0, y, noise = _problem()
    t = torch.fmod(y + 3, NCLS) if kind == "dlr_t" else None
    x_init = A._l2_start(x0, EPS, noise)  # the start has a test of its own
    want_x, want_r, want_l, want = L2.run(model, x0, x_init, y, N_ITER, EPS, kind, t)
    trace = []
    got_x, got_r, got_l = A._apgd_host(model, x0, x_init, y, N_ITER, EPS, kind, t, trace=trace, norm="L2")
    assert len(trace) == len(want) == N_ITER + 1 and "norms" not in trace[0]
    for i, (a, b) in enumerate(zip(trace, want)):
        for key in FLOAT_KEYS + (("norms",) if i else ()):
            assert torch.allclose(a[key], b[key].to(a[key].dtype), rtol=TOL, atol=TOL), (i, key, float((a[key] - b[key]).abs().max()))
        for key in EXACT_KEYS:
            assert a[key].tolist() == b[key].tolist(), (i, key)
        if i:
            for key in ("improved", "fooled", "reduced"):
                assert a[key].tolist() == b[key], (i, key)
        for name in ("x", "x_best", "x_best_adv"):
            assert L2.ball_excess(a[name], x0, EPS) <= 4 * 2.0 ** -52, (i, name)
            assert bool((a[name] >= 0).all()) and bool((a[name] <= 1).all()), (i, name)
    assert torch.allclose(got_x, want_x, rtol=TOL, atol=TOL) and torch.equal(got_r, want_r) and torch.allclose(got_l, want_l, rtol=TOL, atol=TOL)
    cps = [e for e in want[1:] if e["k"]]
    assert len(cps) >= 2
    assert any(r for e in cps for r in e["reduced"]), "no checkpoint halved a step"
    # with the initial step 2 eps the gradient step leaves the ball and is pulled back onto it (the step that stays inside: the NaN test)
    assert bool((torch.stack([e["norms"][1] for e in want[1:]]) > EPS).any())
    # through the door: the published start from the injected draw, then the same run
    xa, rb = A.APGD(model, Args(epsilon=EPS), x0, y, N_ITER, loss=kind, y_target=t, noise=noise, norm="L2")
    assert torch.equal(xa, got_x) and torch.equal(rb, got_r) and xa.dtype == torch.float64


def test_float32_iterates_stay_in_the_ball_and_the_box(cpu_plumbing):
    import utils.attacks as A
    model, x0, y, noise = _problem(torch.float32)
    x_init = A._l2_start(x0, EPS, noise)
    trace = []
    xa, _, _ = A._apgd_host(model, x0, x_init, y, N_ITER, EPS, "ce", trace=trace, norm="L2")
    for i, e in enumerate(trace):
        for name in ("x", "x_best", "x_best_adv"):
            assert L2.ball_excess(e[name], x0, EPS) <= 4 * 2.0 ** -23, (i, name)
            assert bool((e[name] >= 0).all()) and bool((e[name] <= 1).all()), (i, name)
    assert L2.ball_excess(xa, x0, EPS) <= 4 * 2.0 ** -23 and xa.dtype == torch.float32
    assert max(L2.ball_excess(e["x"], x0, EPS) for e in trace[1:]) > -1e-3  # some iterate sits on the sphere


def test_a_nan_gradient_takes_no_gradient_step(cpu_plumbing):
    """The reference and the host path agree on the rule: the sample whose gradient holds a NaN keeps z = x, so with a = 1 and x inside
    the ball it does not move, and the other samples step as usual."""
    import utils.attacks as A
    model, x0, y, noise = _problem()
    x = L2.start(x0, 0.5 * EPS, noise)
    g = torch.randn_like(x0)
    g[1, 0, 0, 0] = float("nan")
    g[2] = 0.0
    step = torch.full((B,), 2 * EPS, dtype=x0.dtype)
    x_new, x_old, norms = L2.step(x, x, g, x0, step, EPS, 1.0)
    assert torch.isnan(norms[0, 1]) and not torch.isnan(x_new).any()
    # "does not move" up to the 1e-12 in the two denominators: each rescale multiplies d by n / (n + 1e-12), n about 0.25
    assert torch.allclose(x_new[1], x[1], rtol=0, atol=1e-11) and torch.allclose(x_new[2], x[2], rtol=0, atol=1e-11)
    assert not torch.allclose(x_new[0], x[0]) and torch.equal(x_old, x)

    class Fixed(torch.nn.Module):  # a classifier whose input gradient is g: logits = <g, x> on class 0
        def forward(self, v):
            z = torch.zeros(v.shape[0], NCLS, dtype=v.dtype)
            z[:, 0] = -(torch.nan_to_num(g) * v).flatten(1).sum(1)
            return z + 0 * v.flatten(1)[:, :1] * g.flatten(1)[:, :1]  # the NaN reaches the gradient of sample 1
    trace = []
    A._apgd_host(Fixed(), x0, x, torch.zeros(B, dtype=torch.int64), 1, EPS, "ce", trace=trace, norm="L2")
    assert torch.isnan(trace[1]["norms"][0, 1]) and not torch.isnan(trace[1]["x"]).any()


def test_l2_start(cpu_plumbing):
    import utils.attacks as A
    _, x0, _, noise = _problem()
    for dtype in (torch.float64, torch.float32):
        xs = A._l2_start(x0.to(dtype), EPS, noise.to(dtype))
        want = L2.start(x0.to(dtype), EPS, noise.to(dtype))
        u = 2.0 ** -52 if dtype == torch.float64 else 2.0 ** -23
        assert xs.dtype == dtype and torch.allclose(xs, want, rtol=0, atol=D * u)
        assert L2.ball_excess(xs, x0.to(dtype), EPS) <= 4 * u and bool((xs >= 0).all()) and bool((xs <= 1).all())
    # unclamped, the start lies ON the sphere (up to the 1e-12 next to ||n||, about 14 here); a draw of its own is seeded by torch
    mid = torch.full_like(x0, 0.5)
    assert -1e-12 <= L2.ball_excess(A._l2_start(mid, 0.25, noise), mid, 0.25) <= 4 * 2.0 ** -52
    torch.manual_seed(3)
    a = A._l2_start(mid, 0.25)
    torch.manual_seed(3)
    assert torch.equal(a, A._l2_start(mid, 0.25)) and not torch.equal(a, A._l2_start(mid, 0.25))


def test_linf_is_left_as_it_was(cpu_plumbing):
    """norm="Linf" returns the same bytes as a call without the parameter, through every door."""
    import utils.attacks as A
    from eeadv import cascade
    model, x0, y, _ = _problem(torch.float32)
    noise = torch.zeros_like(x0).uniform_(-0.03, 0.03)
    a = Args(epsilon=0.03)
    x_init = torch.clamp(x0 + noise, 0, 1)
    t1, t2 = [], []
    r1 = A._apgd_host(model, x0, x_init, y, N_ITER, 0.03, "ce", trace=t1)
    r2 = A._apgd_host(model, x0, x_init, y, N_ITER, 0.03, "ce", trace=t2, norm="Linf")
    assert all(torch.equal(p, q) for p, q in zip(r1, r2)) and all("norms" not in e for e in t2)
    assert all(torch.equal(p[k], q[k]) for p, q in zip(t1, t2) for k in p)
    for fn, args in ((A.APGD, (N_ITER, "dlr")), (A.APGD_T, (N_ITER, NCLS, 2)), (A.APGD_Rand, (3, 2))):
        p = fn(model, a, x0, y, *args, noise=noise)
        q = fn(model, a, x0, y, *args, noise=noise, norm="Linf")
        assert torch.equal(p[0], q[0]) and torch.equal(p[1], q[1]), fn.__name__
    # the L2 run is another run
    p = A.APGD(model, a, x0, y, N_ITER, noise=noise)
    q = A.APGD(model, a, x0, y, N_ITER, noise=noise, norm="L2")
    assert not torch.equal(p[0], q[0])
    # the rand stages hand APGD no `norm` unless it is L2
    seen = []
    real = A.APGD
    try:
        A.APGD = lambda *args, **kw: (seen.append(kw), real(*args, **kw))[1]
        for norm, want in ((None, False), ("Linf", False), ("L2", True)):
            stages = cascade.rand_stages(a, 2, 2) if norm is None else cascade.rand_stages(a, 2, 2, norm)
            for _, fn in stages:
                fn(model, a, x0, y, None)
            assert all(("norm" in kw) == want for kw in seen) and len(seen) == 2
            seen.clear()
    finally:
        A.APGD = real


def test_unknown_norm_raises(cpu_plumbing):
    import utils.attacks as A
    from eeadv import cascade, engine, trainer
    model, x0, y, _ = _problem(torch.float32)
    a = Args(epsilon=EPS, method_name="AT", attack_method="APGD-CE", random=True)
    for bad in ("L1", "l2", "linf", 2, None):
        with pytest.raises(ValueError, match="norm"):
            A.APGD(model, a, x0, y, 2, norm=bad)
        with pytest.raises(ValueError, match="norm"):
            A._apgd_host(model, x0, x0, y, 2, EPS, "ce", norm=bad)
        with pytest.raises(ValueError, match="norm"):
            A.APGD_T(model, a, x0, y, 2, NCLS, norm=bad)
        with pytest.raises(ValueError, match="norm"):
            A.APGD_Rand(model, a, x0, y, 2, 2, norm=bad)
        with pytest.raises(ValueError, match="norm"):
            engine.apgd_loop(model, x0, x0, y, 2, EPS, "ce", norm=bad)
        with pytest.raises(ValueError, match="norm"):
            engine._ApgdRun(x0, y, 2, EPS, "ce", norm=bad)
        with pytest.raises(ValueError, match="norm"):
            cascade.rand_stages(a, 2, 2, bad)
    for bad in ("L1", "l2"):
        a.norm = bad
        with pytest.raises(ValueError, match=r"--norm must be Linf or L2, got '%s'; the L2 threat model is built for APGD-CE, APGD-T" % bad):
            trainer.attack_for_validation(model, a, x0, y, "cpu", 2, 0.01, NCLS)


REFUSING = ("Square", "APGD+Square", "FAB-T", "APGD+FAB+Square", "Cascade", "PGD", "FGSM", "CW")
ACCEPTED = ("APGD-CE", "APGD-T", "APGD", "APGD-DLR", "Rand", "Cascade-Rand")


def test_dispatch_under_l2(cpu_plumbing):
    """trainer.attack_for_validation and driver.validate_cascade under --norm L2: the methods that are APGD runs reach the L2 doors, every
    other method stops with the list of those that have L2, AA still stops, and an args object without the key means Linf."""
    import utils.attacks as A
    from eeadv import driver, trainer
    model, x0, y, _ = _problem(torch.float32)
    assert trainer.L2_METHODS == ACCEPTED
    for method in ACCEPTED:
        assert trainer.norm_for(Args(attack_method=method, norm="L2")) == "L2"
        assert trainer.norm_tag(Args(attack_method=method, norm="L2")) == " [norm L2]"
    for method in REFUSING + ACCEPTED + ("AA",):
        assert trainer.norm_for(Args(attack_method=method)) == "Linf" == trainer.norm_for(Args(attack_method=method, norm="Linf"))
        assert trainer.norm_tag(Args(attack_method=method)) == ""
    for method in REFUSING + ("AA",):
        a = Args(epsilon=EPS, method_name="AT", attack_method=method, random=True, norm="L2", square_queries=4, fab_iters=2)
        with pytest.raises(NotImplementedError, match=r"--norm L2 with --attack_method %s: the L2 threat model is built for APGD-CE, APGD-T, APGD, "
                           r"APGD-DLR, Rand and Cascade-Rand only" % re.escape(method)):
            trainer.attack_for_validation(model, a, x0, y, "cpu", 2, 0.01, NCLS)
    a = Args(epsilon=EPS, method_name="AT", attack_method="Cascade", random=True, norm="L2")
    with pytest.raises(NotImplementedError, match="--norm L2 with --attack_method Cascade:"):
        driver.validate_cascade([(x0, y)], model, a, torch.device("cpu"), 2, NCLS, print)
    a = Args(epsilon=EPS, method_name="AT", attack_method="AA", random=True)
    with pytest.raises(NotImplementedError):
        trainer.attack_for_validation(model, a, x0, y, "cpu", 2, 0.01, NCLS)
    # the dispatch reaches the L2 doors with the run's own arguments
    for method, want in (("APGD-CE", lambda: A.APGD(model, a, x0, y, 3, "ce", norm="L2")[0]),
                         ("APGD-T", lambda: A.APGD_T(model, a, x0, y, 3, NCLS, norm="L2")[0]),
                         ("APGD-DLR", lambda: A.APGD(model, a, x0, y, 3, "dlr", norm="L2")[0]),
                         ("Rand", lambda: A.APGD_Rand(model, a, x0, y, 3, 2, NCLS, norm="L2")[0])):
        a = Args(epsilon=EPS, method_name="AT", attack_method=method, random=True, norm="L2", eot_iter=2 if method == "Rand" else None)
        torch.manual_seed(21)
        got = trainer.attack_for_validation(model, a, x0, y, "cpu", 3, 0.01, NCLS)
        torch.manual_seed(21)
        assert torch.equal(got, want()), method
        assert L2.ball_excess(got, x0, EPS) <= 4 * 2.0 ** -23
        a.norm = "Linf"
        torch.manual_seed(21)
        assert not torch.equal(trainer.attack_for_validation(model, a, x0, y, "cpu", 3, 0.01, NCLS), got), method
    lines = []
    a = Args(epsilon=EPS, method_name="AT", attack_method="Cascade-Rand", random=True, norm="L2", eot_iter=2)
    driver.validate_cascade([(x0, y)], model, a, torch.device("cpu"), 2, NCLS, lines.append)
    assert lines[0].startswith(" * Cascade: 4 samples, APGD-CE/APGD-DLR") and lines[0].endswith(" [norm L2]")
    lines.clear()
    a.norm = "Linf"
    driver.validate_cascade([(x0, y)], model, a, torch.device("cpu"), 2, NCLS, lines.append)
    assert re.fullmatch(r" \* Cascade: 4 samples, APGD-CE/APGD-DLR attacked rows per stage \d+/\d+, [\d.]+ s", lines[0])


def test_abi_of_the_l2_step():
    import eeadv._native as n
    from eeadv import ops
    L = n.lib
    assert "ee_apgd_step_l2_f32" in n.SIGNATURES and hasattr(L, "ee_apgd_step_l2_f32")
    p, q, r, s = (ctypes.c_void_p(4096 * k) for k in (1, 2, 3, 4))
    f = L.ee_apgd_step_l2_f32
    eps = ctypes.c_float(0.5)
    assert f(p, q, r, s, p, p, p, -1, 8, eps, 0, None) == -2 and f(p, q, r, s, p, p, p, 2, -8, eps, 0, None) == -2
    assert f(p, q, r, s, p, p, p, 2, 8, eps, 3, None) == -2 and f(p, q, r, s, p, p, p, 2, 8, eps, -1, None) == -2  # no such path
    assert f(p, q, r, s, p, p, p, 2, 8, ctypes.c_float(-0.5), 0, None) == -2 and f(p, q, r, s, p, p, p, 2, 8, ctypes.c_float(float("nan")), 0, None) == -2
    assert f(p, q, r, s, p, p, p, 2, 12292, eps, 1, None) == -3  # the resident path ends at 12288
    assert f(None, None, None, None, None, None, None, 0, 8, eps, 0, None) == 0 and f(None, None, None, None, None, None, None, 3, 0, eps, 0, None) == 0
    for k in range(7):  # every pointer is required, norms included
        ptrs = [p, q, r, s, p, p, p]
        ptrs[k] = None
        assert f(*ptrs, 2, 8, eps, 0, None) == -1, k
        ptrs[k] = ctypes.c_void_p(4098)
        assert f(*ptrs, 2, 8, eps, 0, None) == -4, k
    assert ops.APGD_L2_PATHS == {"auto": 0, "resident": 1, "streaming": 2} and ops.APGD_L2_RESIDENT == 12288
    z = torch.zeros(2, 8)
    with pytest.raises(n.EEError):  # no CPU fallback
        ops.apgd_step_l2_(z, z.clone(), z.clone(), z.clone(), torch.zeros(2), torch.zeros(1, dtype=torch.int32), 0.5)


def _mnist_cfg(tmp_path):
    cfg = open(os.path.join(PKG, "MNIST", "configs_mnist", "adversarial_training.yml")).read()
    cfg = re.sub(r"num_steps_(\d): \d+", r"num_steps_\1: 2", cfg)
    cfg = re.sub(r"batch_size: \d+", "batch_size: 4", cfg)
    path = tmp_path / "l2.yml"
    path.write_text(cfg)
    return str(path)


def _mnist(tmp_path, *extra):
    return subprocess.run([sys.executable, "experiments_mnist.py", "-c", _mnist_cfg(tmp_path), "--no-cuda", "--data", "synthetic:1:1", "--output-root",
                           str(tmp_path), "-e", *extra], cwd=os.path.join(PKG, "MNIST"), capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("method", REFUSING + ("AA",))
def test_mnist_driver_refuses_l2_for(tmp_path, method):
    r = _mnist(tmp_path, "--attack_method", method, "--norm", "L2")
    assert r.returncode != 0
    assert "--norm L2 with --attack_method %s: the L2 threat model is built for APGD-CE, APGD-T, APGD, APGD-DLR, Rand and Cascade-Rand only" % method in r.stderr
    assert "creating model" not in r.stdout  # it stops before any work is done


def test_mnist_driver_refuses_an_unknown_norm(tmp_path):
    r = _mnist(tmp_path, "--attack_method", "APGD-CE", "--norm", "L1")
    assert r.returncode != 0 and "--norm must be Linf or L2, got 'L1'; the L2 threat model is built for APGD-CE" in r.stderr
    assert "creating model" not in r.stdout


@pytest.mark.parametrize("method", ACCEPTED)
def test_mnist_driver_evaluates_in_l2_on_the_host(tmp_path, method):
    r = _mnist(tmp_path, "--attack_method", method, "--norm", "L2", *(("--eot_iter", "2") if method in ("Rand", "Cascade-Rand") else ()))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    logs = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path)) for f in fs if f == "log.txt"]
    assert logs
    for text in (r.stdout, "".join(open(f).read() for f in logs)):
        if method == "Cascade-Rand":
            assert len(re.findall(r"^ \* Cascade: .* \[norm L2\]$", text, flags=re.M)) == 3
        else:
            assert len(re.findall(r"^ \* Adv Prec@1 [\d.]+ Prec@5 [\d.]+ \[norm L2\]$", text, flags=re.M)) == 3
            assert len(re.findall(r"^ \* Clean Prec@1 [\d.]+ Prec@5 [\d.]+$", text, flags=re.M)) == 3


def test_mnist_driver_linf_lines_are_unchanged(tmp_path):
    r = _mnist(tmp_path, "--attack_method", "APGD-CE", "--norm", "Linf")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert len(re.findall(r"^ \* Adv Prec@1 [\d.]+ Prec@5 [\d.]+$", r.stdout, flags=re.M)) == 3 and "norm" not in r.stdout
