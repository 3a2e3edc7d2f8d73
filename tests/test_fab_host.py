"""CPU: the float64 FAB-T reference's own projection (feasible, minimal), the ABI of the ee_fab_* kernels, the plain-torch host path of
utils.attacks.FAB_T against tests/fab_reference.py teacher-forced in float64, the closed form on a linear classifier, the dispatch in
attack_for_validation and one driver run."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import fab_reference as R
from tiny_models import Args, TinyNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")
EPS64 = 2.0 ** -52


def test_abi_of_the_fab_kernels():
    import eeadv._native as n
    L = n.lib
    for name in ("ee_fab_diff_f32", "ee_fab_proj_linf_f32", "ee_fab_step_f32", "ee_fab_commit_f32"):
        assert name in n.SIGNATURES and hasattr(L, name)
    assert (n.K_FAB_DIFF, n.K_FAB_PROJ, n.K_FAB_STEP, n.K_FAB_COMMIT) == (26, 27, 28, 29)
    assert L.ee_prof_read(29, None, None) != -2 and L.ee_prof_read(30, None, None) == -2  # EE_K_COUNT moved with them
    p = ctypes.c_void_p(4096)
    assert L.ee_fab_diff_f32(None, p, p, 4, 10, p, p, p, None) == -1 and L.ee_fab_diff_f32(p, p, None, 4, 10, p, p, p, None) == -1
    assert L.ee_fab_diff_f32(p, p, p, 4, 1, p, p, p, None) == -2 and L.ee_fab_diff_f32(p, p, p, -1, 10, p, p, p, None) == -2
    assert L.ee_fab_diff_f32(None, None, None, 0, 10, None, None, None, None) == 0
    assert L.ee_fab_diff_f32(p, ctypes.c_void_p(4100), p, 4, 10, p, p, p, None) == -4
    assert L.ee_fab_proj_linf_f32(p, p, None, p, 2, 8, 0, p, None) == -1 and L.ee_fab_proj_linf_f32(p, p, p, p, 2, 8, 0, None, None) == -1
    assert L.ee_fab_proj_linf_f32(p, p, p, p, 2, 0, 0, p, None) == -2 and L.ee_fab_proj_linf_f32(p, p, p, p, 2, 8, 3, p, None) == -2
    assert L.ee_fab_proj_linf_f32(p, p, p, p, 2, 12289, 1, p, None) == -3  # the resident path ends at 3*64*64
    assert L.ee_fab_proj_linf_f32(None, None, None, None, 0, 8, 0, None, None) == 0
    assert L.ee_fab_proj_linf_f32(ctypes.c_void_p(4098), p, p, p, 2, 8, 0, p, None) == -4
    assert L.ee_fab_step_f32(p, p, p, None, 2, 8, None) == -1 and L.ee_fab_step_f32(p, p, p, p, -1, 8, None) == -2
    assert L.ee_fab_step_f32(None, None, None, None, 0, 8, None) == 0 and L.ee_fab_step_f32(p, ctypes.c_void_p(4098), p, p, 2, 8, None) == -4
    assert L.ee_fab_commit_f32(p, p, 4, 10, p, p, p, p, p, p, None, 8, None) == -1 and L.ee_fab_commit_f32(p, p, 4, 1, p, p, p, p, p, p, p, 8, None) == -2
    assert L.ee_fab_commit_f32(None, None, 0, 10, None, None, None, None, None, None, None, 8, None) == 0


def test_ops_refuse_cpu_tensors():
    from eeadv import ops
    import eeadv._native as n
    x = torch.rand(2, 8)
    with pytest.raises(n.EEError):
        ops.fab_proj_linf(x, x, x, torch.ones(2))
    with pytest.raises(n.EEError):
        ops.fab_step_(x, x, x, torch.zeros(3, 4))


# ---- the reference's own projection --------------------------------------------------------------------------------------------------
def _problem(D, rng, kind):
    p = rng.random(D)
    w = rng.standard_normal(D)
    if kind == "clipped":
        p[::2] = np.where(rng.random(p[::2].size) < 0.5, 0.02, 0.98)
    if kind == "ends":
        p[::2] = np.where(rng.random(p[::2].size) < 0.5, 0.0, 1.0)
        w[1::3] = 0.0
    sign = 1.0 if rng.random() < 0.5 else -1.0
    a, r = R.rooms(p, w, sign)
    ginf = float(np.sum(a * r))
    frac = {"inactive": 0.02, "clipped": 0.6, "ends": 0.5}[kind]
    return p, w, sign * frac * ginf


@pytest.mark.parametrize("D", [1, 3, 5, 75, 192])
def test_reference_projection_is_feasible_and_minimal(D):
    rng = np.random.default_rng(D)
    seen = 0
    for kind in ("inactive", "clipped", "ends"):
        for _ in range(6):
            p, w, c = _problem(D, rng, kind)
            if c == 0:
                continue
            lam, s, norm, delta = R.project(p, w, c)
            a, r = R.rooms(p, w, s)
            assert np.isfinite(lam) and lam > 0
            # feasible: inside the box, on the hyperplane <w, p + delta> = <w, p> - c to float64 rounding
            q = p + delta
            assert (q >= -1e-16).all() and (q <= 1 + 1e-16).all() and (np.abs(delta) <= r + 1e-16).all()
            scale = float(np.sum(np.abs(w * delta))) + abs(c)
            assert abs(float(np.sum(w * delta)) + c) <= (D + 8) * EPS64 * scale
            assert norm == float(np.max(np.abs(delta)))
            # minimal: a slightly smaller lam leaves the residual's sign, and a brute-force bisection on lam finds nothing closer
            cp = abs(c)
            assert R.g_of(lam * (1 - 1e-6), a, r) < cp
            lo, hi = 0.0, 2.0
            for _ in range(200):
                mid = 0.5 * (lo + hi)
                if R.g_of(mid, a, r) >= cp:
                    hi = mid
                else:
                    lo = mid
            brute = min(hi, float(r[a != 0].max()))
            assert brute >= norm * (1 - (D + 8) * EPS64)
            assert brute <= norm * (1 + 1e-9)  # and the walk is not larger than the brute-force answer either
            seen += 1
    assert seen >= 12


def test_reference_projection_edge_cases():
    p, w = np.array([0.25, 0.5, 1.0]), np.array([1.0, -2.0, -3.0])
    lam, s, norm, delta = R.project(p, w, 0.0)
    assert lam == 0 and s == 1 and norm == 0 and not delta.any()
    lam, s, norm, delta = R.project(p, w, 100.0)  # infeasible: everything to its bound (coordinate 2 has no room)
    assert lam == float("inf") and norm == 0.5 and delta.tolist() == [-0.25, 0.5, 0.0]
    lam, s, norm, delta = R.project(p, w, -0.3)  # the sign flip: v = -w, coordinate 0 moves up, 1 down, 2 down
    assert s == -1 and lam == pytest.approx(0.05) and delta.tolist() == pytest.approx([0.05, -0.05, -0.05])
    lam, s, norm, delta = R.project(p, np.zeros(3), 0.3)
    assert lam == float("inf") and norm == 0 and not delta.any()


# ---- the host path against the reference -----------------------------------------------------------------------------------------------
def _setup(dtype=torch.float64, B=4, K=10, seed=21):
    g = torch.Generator().manual_seed(seed)
    m = TinyNet(3, 8, K, seed).to(dtype)
    x0 = (0.1 + 0.8 * torch.rand(B, 3, 8, 8, generator=g)).to(dtype)
    x0[0, :, :2] = 0.0  # one sample with pixels on both ends of the box
    x0[0, :, 2:4] = 1.0
    with torch.no_grad():
        order = torch.sort(m(x0), dim=1, descending=True, stable=True)[1]
    return m, x0, order[:, 0].clone(), order[:, 1].clone()


def _close(got, want, bound, what):
    """|got - want| <= bound * |want|, element-wise; bound a float or a tensor that broadcasts."""
    got, want = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(want, dtype=torch.float64)
    both_inf = torch.isinf(got) & torch.isinf(want) & (got == want)
    err = torch.where(both_inf, torch.zeros_like(want), (got - want).abs())
    assert bool((err <= bound * want.abs()).all()), (what, float(err.max()))


def test_host_path_teacher_forced_against_the_reference():
    """Every iteration of the host path starts from the reference's recorded state.  Flags and pred equal.  Real quantities: the sums
    (the two logits behind df, the gradient) are held to (D + K + 8) * 2^-52 relative to their own size.  df is the difference of two such
    sums and cancels - a run approaches the decision boundary, |df| falls far below the logits - so its relative error, and that of
    everything proportional to it (lambda, the norms, alpha, the step), is that bound times (|z_t| + |z_y|) / |df|.  Element-wise tensors
    with entries in [0, 1] are compared relative to max(|value|, 1)."""
    import utils.attacks as A
    n_iter, K = 6, 10
    m, x0, y, t = _setup(K=K)
    D = x0[0].numel()
    bound = (D + K + 8) * EPS64
    _, _, trace = R.run(m, x0, y, t, n_iter)
    n_adv = n_imp = 0
    for i, e in enumerate(trace):
        x, adv, res, info = A._fab_host_iteration(m, e["x_in"], x0, y, t, e["adv_in"], e["res_in"])
        assert info["pred"].tolist() == e["pred"].tolist() and info["is_adv"].tolist() == e["is_adv"].tolist(), i
        assert info["improved"].tolist() == e["improved"].tolist() and info["enabled"].tolist() == e["enabled"].tolist(), i
        assert info["s1"].tolist() == e["s1"].tolist() and info["s2"].tolist() == e["s2"].tolist(), i
        assert bool(((info["df"] - e["df"]).abs() <= bound * (e["zt"].abs() + e["zy"].abs())).all()), i
        cond = (e["zt"].abs() + e["zy"].abs()) / e["df"].abs()
        for k in ("lam1", "lam2", "n1", "n2", "alpha", "nrm"):
            _close(info[k], e[k], bound * cond, (k, i))
        _close(res, e["res"], bound * cond, ("res", i))
        wmax = e["w"].flatten(1).abs().max(dim=1)[0].view(-1, 1)
        assert bool(((info["w"] - e["w"].flatten(1)).abs() <= bound * wmax).all()), i
        for got, want in ((info["x_step"], e["x_step"]), (x, e["x"]), (adv, e["adv"])):
            assert bool(((got - want).abs() <= (bound * cond).view(-1, 1, 1, 1) * want.abs().clamp_min(1.0)).all()), i
        n_adv += int(e["is_adv"].sum())
        n_imp += int(e["improved"].sum())
    assert n_adv > 0 and n_imp > 0 and n_adv > n_imp  # the run saw adversarial points that improved and some that did not


def test_host_path_free_running_matches_its_own_iterations():
    import utils.attacks as A
    m, x0, y, t = _setup()
    trace = []
    adv, res = A._fab_host(m, x0, y, t, 5, trace=trace)
    assert len(trace) == 5 and torch.equal(trace[-1]["adv"], adv) and torch.equal(trace[-1]["res"], res)
    found = torch.isfinite(res)
    assert bool(found.any())
    assert torch.equal((adv - x0).flatten(1).abs().max(dim=1)[0][found], res[found])
    assert torch.equal(adv[~found], x0[~found])
    with torch.no_grad():
        assert bool((m(adv).argmax(1) != y)[found].all())


def test_host_path_rests_on_a_sample_without_a_hyperplane():
    """t == y gives df = 0 and w = 0: delta = 0 for both problems, the iterate stays where it is."""
    import utils.attacks as A
    m, x0, y, t = _setup()
    t = t.clone()
    t[1] = y[1]
    x = (x0 * 0.9 + 0.05).clone()
    x_new, adv, res, info = A._fab_host_iteration(m, x, x0, y, t, x0.clone(), torch.full((4,), float("inf"), dtype=torch.float64))
    assert not bool(info["enabled"][1]) and bool(info["enabled"][[0, 2, 3]].all())
    assert torch.equal(info["x_step"][1], x[1]) and float(info["lam1"][1]) == 0 and float(info["s1"][1]) == 0
    ref = R.iterate(m, x[1:2], x0[1:2], int(y[1]), int(t[1]), x0[1:2], float("inf"))
    assert not ref["enabled"] and torch.equal(ref["x_step"], x[1:2])


# ---- the closed form on a linear classifier ------------------------------------------------------------------------------------------
class _Linear(torch.nn.Module):
    def __init__(self, D, seed, dtype):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.fc = torch.nn.Linear(D, 2).to(dtype)
        with torch.no_grad():
            self.fc.weight.copy_(torch.randn(2, D, generator=g, dtype=torch.float64) * 0.08)
            self.fc.bias.copy_(torch.tensor([0.9, -0.9], dtype=torch.float64))

    def forward(self, x):
        return self.fc(x.flatten(1))


def linear_case(dtype, seed=4, B=6, D=192):
    """One Linear(D, 2), x0 in [0.3, 0.7], weights small enough that the box never binds, |df(x0)| >= 0.5 with logits of order 1."""
    g = torch.Generator().manual_seed(seed + 100)
    m = _Linear(D, seed, dtype)
    x0 = (0.3 + 0.4 * torch.rand(B, 3, 8, 8, generator=g, dtype=torch.float64)).to(dtype)
    with torch.no_grad():
        z = m(x0).double()
    y = z.argmax(1)
    t = 1 - y
    df = (z[torch.arange(B), t] - z[torch.arange(B), y])
    w1 = (m.fc.weight[1] - m.fc.weight[0]).double().abs().sum()
    dist = df.abs() / w1
    return m, x0, y, t, df, dist


def test_linear_classifier_bound_in_float64():
    import utils.attacks as A
    D, n_iter = 192, 5
    m, x0, y, t, df, dist = linear_case(torch.float64)
    assert bool((df.abs() >= 0.5).all()) and float(m(x0).detach().abs().max()) < 10
    adv_r, res_r, trace = R.run(m, x0, y, t, n_iter)
    for e in trace:  # the reference run keeps every coordinate strictly inside the box: the closed form dist = |df| / ||w||_1 applies
        assert bool((e["x_step"] > 0).all()) and bool((e["x_step"] < 1).all())
    eps = 2 * float(dist.detach().max())
    margin = (D + 8) * EPS64
    a = Args(epsilon=eps)
    from eeadv import runtime
    runtime.allow_cpu_plumbing(True)
    try:
        x_adv, robust, norm = A.FAB_T(m, a, x0, y, 2, n_iter=n_iter)
    finally:
        runtime.allow_cpu_plumbing(False)
    for nrm in (res_r, norm):
        assert bool((nrm >= dist * (1 - margin)).all()) and bool((nrm <= 1.05 * dist * (1 + margin)).all())
    assert not bool(robust.any())
    with torch.no_grad():
        assert bool((m(x_adv).argmax(1) != y).all())
    assert torch.equal((x_adv - x0).flatten(1).abs().max(dim=1)[0], norm)


# ---- dispatch ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def cpu_plumbing():
    from eeadv import runtime
    runtime.allow_cpu_plumbing(True)
    yield
    runtime.allow_cpu_plumbing(False)


@pytest.mark.parametrize("method", ["FAB-T", "APGD+FAB+Square"])
def test_attack_for_validation_takes_the_fab_methods(cpu_plumbing, method):
    from eeadv import trainer
    torch.manual_seed(0)
    m = TinyNet(3, 8, 10, 5).eval()
    x = torch.rand(4, 3, 8, 8)
    with torch.no_grad():
        y = m(x).argmax(1)
    eps = 16 / 255
    a = Args(epsilon=eps, method_name="AT", attack_method=method, random=True, square_queries=6, fab_iters=3)
    assert method in trainer.FAB_METHODS
    xa = trainer.attack_for_validation(m, a, x, y, torch.device("cpu"), 3, eps / 4, 10)
    e = torch.tensor(eps, dtype=torch.float32)
    assert xa.shape == x.shape and bool((xa >= x - e).all()) and bool((xa <= x + e).all()) and bool((xa >= 0).all()) and bool((xa <= 1).all())
    a.method_name = "tar_AT"
    with pytest.raises(NotImplementedError, match="untargeted"):
        trainer.attack_for_validation(m, a, x, y, torch.device("cpu"), 3, eps / 4, 10)
    a.method_name, a.attack_method = "AT", "AA"
    with pytest.raises(NotImplementedError):
        trainer.attack_for_validation(m, a, x, y, torch.device("cpu"), 3, eps / 4, 10)


def test_fab_t_thresholds_at_eps_and_marks_clean_errors(cpu_plumbing):
    import utils.attacks as A
    m, x0, y, t = _setup(torch.float32)
    y = y.clone()
    y[2] = (y[2] + 1) % 10  # misclassified before any attack: norm 0, the clean point is its own adversarial example
    big, small = Args(epsilon=1.0), Args(epsilon=1e-6)
    xa, robust, norm = A.FAB_T(m, big, x0, y, 10, n_iter=4, n_target_classes=2)
    assert float(norm[2]) == 0 and not bool(robust[2]) and torch.equal(xa[2], x0[2])
    assert torch.equal(robust, ~(norm <= 1.0))
    xs, rs, ns = A.FAB_T(m, small, x0, y, 10, n_iter=4, n_target_classes=2)
    assert torch.equal(ns, norm) and rs.tolist() == [True, True, False, True] and torch.equal(xs, x0)


def test_mnist_driver_evaluates_with_fab_on_the_host(tmp_path):
    r = subprocess.run([sys.executable, "experiments_mnist.py", "-c", "configs_mnist/adversarial_training.yml", "--no-cuda", "--data", "synthetic",
                        "--output-root", str(tmp_path), "-e", "--attack_method", "FAB-T", "--fab_iters", "3"],
                       cwd=os.path.join(PKG, "MNIST"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    logs = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path)) for f in fs if f.startswith("log")]
    text = r.stdout + "".join(open(f).read() for f in logs)
    clean = re.findall(r"^ \* Clean Prec@1 ([\d.]+)", text, flags=re.M)
    adv = re.findall(r"^ \* Adv Prec@1 ([\d.]+)", text, flags=re.M)
    assert len(clean) >= 1 and len(clean) == len(adv)
    for c1, a1 in zip(clean, adv):
        assert float(a1) <= float(c1)
