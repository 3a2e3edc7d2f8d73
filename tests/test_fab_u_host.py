"""CPU: untargeted FAB.  The plain-torch host paths utils.attacks._fab_u_host / _fab_u_l1_host against
tests/fab_u_reference.py teacher-forced in float64 (the tolerances of test_fab_host.py, test_fab_l2_host.py and test_fab_l1_host.py for the
same comparison), the selection rules (tie, NaN gradient, k == y, nothing left), the closed form on a linear classifier - with the case the
attack exists for: the closest boundary belongs to a class FAB_T never targets - the ABI of ee_fab_select_f32, and the drivers."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import fab_u_reference as U
from test_fab_l2_host import _MLP, segment
from tiny_models import Args, TinyNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")
EPS64 = 2.0 ** -52
METRICS = ("Linf", "L2", "L1")


@pytest.fixture()
def cpu_plumbing():
    from eeadv import runtime
    runtime.allow_cpu_plumbing(True)
    yield
    runtime.allow_cpu_plumbing(False)


def host_iteration(metric, m, x, x0, y, adv, res):
    import utils.attacks as A
    if metric == "L1":
        return A._fab_u_l1_host_iteration(m, x, x0, y, adv, res)
    return A._fab_u_host_iteration(m, x, x0, y, adv, res, norm=metric)


def host_run(metric, m, x0, y, n_iter, trace=None):
    import utils.attacks as A
    if metric == "L1":
        return A._fab_u_l1_host(m, x0, y, n_iter, trace=trace)
    return A._fab_u_host(m, x0, y, n_iter, trace=trace, norm=metric)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_select_launch():
    import eeadv._native as n
    L = n.lib
    assert "ee_fab_select_f32" in n.SIGNATURES and hasattr(L, "ee_fab_select_f32")
    assert L.ee_prof_read(29, None, None) != -2 and L.ee_prof_read(30, None, None) == -2  # no new timing family: it records under EE_K_FAB_DIFF
    p = ctypes.c_void_p(4096)
    ok = (p, p, p, 1, 0, 1, 4, 10, 8, p, p, p, p, None)

    def call(**kw):
        names = ("g", "logits", "labels", "k", "metric", "first", "B", "K", "D", "best", "best_k", "w", "df", "stream")
        a = dict(zip(names, ok))
        a.update(kw)
        return L.ee_fab_select_f32(*[a[k] for k in names])

    for name in ("g", "logits", "labels", "best", "best_k", "w", "df"):
        assert call(**{name: None}) == -1, name
    assert call(k=-1) == -2 and call(k=10) == -2 and call(K=1) == -2 and call(D=0) == -2 and call(B=-1) == -2
    assert call(metric=3) == -2 and call(metric=-1) == -2
    assert call(B=0, g=None, logits=None, labels=None, best=None, best_k=None, w=None, df=None) == 0  # an empty batch launches nothing
    assert call(g=ctypes.c_void_p(4098)) == -4 and call(labels=ctypes.c_void_p(4100)) == -4


def test_select_refuses_cpu_tensors_and_unknown_metrics():
    from eeadv import ops
    import eeadv._native as n
    g, z, y = torch.rand(2, 8), torch.rand(2, 4), torch.zeros(2, dtype=torch.int64)
    st = (torch.zeros(2), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 8), torch.zeros(2))
    with pytest.raises(n.EEError):
        ops.fab_select(g, z, y, 1, "Linf", *st)
    with pytest.raises(ValueError, match="metric"):
        ops.fab_select(g, z, y, 1, "L3", *st)
    with pytest.raises(ValueError, match="class"):
        ops.fab_select(g, z, y, 4, "Linf", *st)


# ---- host against reference, teacher-forced ------------------------------------------------------------------------------------------
def _mlp_case():
    g = torch.Generator().manual_seed(3)
    m = _MLP(48, 16, 6, 3)
    x0 = 0.1 + 0.8 * torch.rand(5, 3, 4, 4, generator=g, dtype=torch.float64)
    x0[0, :, :1], x0[0, :, 1:2] = 0.0, 1.0  # one sample with pixels on both ends of the box
    return m, x0, 6


def _conv_case():
    g = torch.Generator().manual_seed(21)
    m = TinyNet(3, 8, 10, 21).double().eval()
    x0 = 0.1 + 0.8 * torch.rand(4, 3, 8, 8, generator=g, dtype=torch.float64)
    x0[0, :, :2], x0[0, :, 2:4] = 0.0, 1.0
    return m, x0, 10


def _check_linf(info, x, adv, res, e, x0, bound, i):
    """test_fab_host.py::test_host_path_teacher_forced_against_the_reference"""
    cond = (e["zt"].abs() + e["zy"].abs()) / e["df"].abs()
    for k in ("lam1", "lam2", "n1", "n2", "alpha", "nrm"):
        _close(info[k], e[k], bound * cond, (k, i))
    _close(res, e["res"], bound * cond, ("res", i))
    for got, want in ((info["x_step"], e["x_step"]), (x, e["x"]), (adv, e["adv"])):
        assert bool(((got - want).abs() <= (bound * cond).view(-1, 1, 1, 1) * want.abs().clamp_min(1.0)).all()), i


def _close(got, want, bound, what):
    got, want = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(want, dtype=torch.float64)
    both_inf = torch.isinf(got) & torch.isinf(want) & (got == want)
    err = torch.where(both_inf, torch.zeros_like(want), (got - want).abs())
    assert bool((err <= bound * want.abs()).all()), (what, float(err.max()))


def _check_l2(info, x, adv, res, e, x0, bound, i):
    """test_fab_l2_host.py::test_host_run_teacher_forced_against_the_reference_run"""
    B = x0.shape[0]
    amp = torch.ones(B, dtype=torch.float64)
    for b in range(B):
        for p, c, mu in ((e["x_in"][b], e["df"][b], e["lam1"][b]), (x0[b], e["c2"][b], e["lam2"][b])):
            S, _ = segment(p.flatten().numpy(), e["w"][b].flatten().numpy(), float(c), float(mu))
            amp[b] = max(float(amp[b]), (abs(float(c)) + S) / (abs(float(c)) - S))
    tol = bound * amp * (e["zt"].abs() + e["zy"].abs()) / e["df"].abs()
    for k in ("lam1", "lam2", "n1", "n2", "alpha", "nrm"):
        assert bool(((info[k] - e[k]).abs() <= tol * e[k].abs()).all()), (k, i)
    assert bool(((res - e["res"]).abs() <= tol * e["res"].abs())[torch.isfinite(e["res"])].all()), i
    assert torch.equal(torch.isfinite(res), torch.isfinite(e["res"]))
    for got, want in ((info["x_step"], e["x_step"]), (x, e["x"]), (adv, e["adv"])):
        assert bool(((got - want).abs() <= tol.view(-1, 1, 1, 1) * want.abs().clamp_min(1.0)).all()), i


def _check_l1(info, x, adv, res, e, x0, bound, i):
    """test_fab_l1_host.py::test_host_iteration_teacher_forced_against_the_reference_iteration"""
    B = x0.shape[0]
    wr = e["w"].flatten(1)
    wmax = wr.abs().max(dim=1)[0]
    dc = bound * (e["zt"].abs() + e["zy"].abs() + (wr * (x0 - e["x_in"]).flatten(1)).abs().sum(dim=1))
    tol_n = torch.zeros(B, dtype=torch.float64)
    for k in ("lam1", "lam2"):
        assert bool(((info[k] - e[k]).abs() <= bound * wmax).all()), (k, i)
        tol_n = torch.maximum(tol_n, dc / e[k])
    for k in ("n1", "n2"):
        assert bool(((info[k] - e[k]).abs() <= tol_n + bound * e[k]).all()), (k, i)
    assert bool(((info["nrm"] - e["nrm"]).abs() <= 1.05 * tol_n + bound * e["nrm"].clamp_min(1.0)).all()), i
    tol_x = (1.05 * tol_n * (1 + (e["n1"] + e["n2"]) / (e["n1"] + e["n2"]).clamp_min(1e-8)) + bound).view(-1, 1, 1, 1)
    for got, want in ((info["x_step"], e["x_step"]), (x, e["x"]), (adv, e["adv"])):
        assert bool(((got - want).abs() <= tol_x).all()), i


CHECKS = {"Linf": _check_linf, "L2": _check_l2, "L1": _check_l1}


@pytest.mark.parametrize("case", [_mlp_case, _conv_case], ids=["mlp", "conv"])
@pytest.mark.parametrize("metric", METRICS)
def test_host_path_teacher_forced_against_the_reference(metric, case):
    """Every host iteration starts from the reference's recorded state.  The chosen class, the flags, pred and the signs are equal; df and
    the gradient are held to (D + K + 8) 2^-52 of their size; everything downstream to the bound the metric's own FAB-T test derives."""
    m, x0, K = case()
    with torch.no_grad():
        y = m(x0).argmax(1)
    n_iter, D = 3, x0[0].numel()
    bound = (D + K + 8) * EPS64
    _, _, trace = U.run(m, x0, y, n_iter, metric)
    n_adv, chosen = 0, set()
    for i, e in enumerate(trace):
        x, adv, res, info = host_iteration(metric, m, e["x_in"], x0, y, e["adv_in"], e["res_in"])
        assert info["best_k"].tolist() == e["best_k"].tolist(), i
        assert bool((e["best_k"] != y).all()) and bool((e["best_k"] >= 0).all())
        _close(info["best"], e["best"], bound * (e["zt"].abs() + e["zy"].abs()) / e["df"].abs(), ("best", i))
        assert info["pred"].tolist() == e["pred"].tolist() and info["is_adv"].tolist() == e["is_adv"].tolist(), i
        assert info["improved"].tolist() == e["improved"].tolist() and info["enabled"].tolist() == e["enabled"].tolist(), i
        assert info["s1"].tolist() == e["s1"].tolist() and info["s2"].tolist() == e["s2"].tolist(), i
        assert bool(((info["df"] - e["df"]).abs() <= bound * (e["zt"].abs() + e["zy"].abs())).all()), i
        wmax = e["w"].flatten(1).abs().max(dim=1)[0].view(-1, 1)
        assert bool(((info["w"] - e["w"].flatten(1)).abs() <= bound * wmax).all()), i
        CHECKS[metric](info, x, adv, res, e, x0, bound, i)
        n_adv += int(e["is_adv"].sum())
        chosen |= set(e["best_k"].tolist())
    assert n_adv > 0 and len(chosen) > 1  # the run saw adversarial points, and more than one class was the closest somewhere
    trace_h = []
    adv, res = host_run(metric, m, x0, y, n_iter, trace=trace_h)
    assert len(trace_h) == n_iter and torch.equal(trace_h[-1]["adv"], adv) and torch.equal(trace_h[-1]["res"], res)
    assert torch.equal(adv[~torch.isfinite(res)], x0[~torch.isfinite(res)])


# ---- the selection rules ---------------------------------------------------------------------------------------------------------------
class _NanGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return torch.where(g != 0, torch.full_like(g, float("nan")), g)  # a zero gradient (another class's pass) stays zero


class _Affine(torch.nn.Module):
    """z = A x + c in float64; nan_class: that logit's value is unchanged and its gradient is NaN."""

    def __init__(self, A, c, nan_class=None):
        super().__init__()
        self.A, self.c, self.nan_class = A.double(), c.double(), nan_class

    def forward(self, x):
        f = x.flatten(1)
        z = f @ self.A.t() + self.c
        if self.nan_class is not None:
            k = self.nan_class
            z = torch.cat([z[:, :k], (_NanGrad.apply(f) @ self.A[k:k + 1].t() + self.c[k:k + 1]), z[:, k + 1:]], dim=1)
        return z


def _rule_case(nan_class=None):
    """D = 4, K = 5, the label is class 2 (zero weights, logit 1).  Classes 1 and 3 are mirror images: the same |df| = 0.5 and gradients e_0 and
    -e_0 - an exact tie in every dual norm; class 0 is farther (|df| = 0.9), class 4 would be by far the closest (|df| = 0.01)."""
    A = torch.zeros(5, 4, dtype=torch.float64)
    A[0, 1], A[1, 0], A[3, 0], A[4, 2] = 1.0, 1.0, -1.0, 1.0
    c = torch.tensor([0.1 - 0.5, 0.5 - 0.5, 1.0, 0.5 + 0.5, 0.99 - 0.5], dtype=torch.float64)
    x = torch.full((1, 1, 2, 2), 0.5, dtype=torch.float64)
    return _Affine(A, c, nan_class), x, torch.tensor([2])


@pytest.mark.parametrize("metric", METRICS)
def test_selection_rules(metric):
    import utils.attacks as A
    dual = {"Linf": A._dual_of_linf, "L2": A._l2_norms, "L1": A._dual_of_l1}[metric]

    def plane(m, x, y):
        return A._fab_closest_plane(m, x.clone().requires_grad_(), y, dual)

    # class 4 is the closest; with its gradient NaN (its logit and df are finite) it is skipped, and the tie of 1 and 3 goes to 1
    m, x, y = _rule_case()
    w, df, k, best = plane(m, x, y)
    assert k.tolist() == [4] and float(df) == pytest.approx(-0.01) and float(best) == pytest.approx(0.01)
    z, J = U.jacobian(m, x)
    assert U.select(z, J, 2, metric)[0] == 4
    m, x, y = _rule_case(nan_class=4)
    w, df, k, best = plane(m, x, y)
    assert k.tolist() == [1] and float(df) == -0.5 and float(best) == 0.5 / (1e-12 + 1.0) and w.flatten().tolist() == [1.0, 0.0, 0.0, 0.0]
    z, J = U.jacobian(m, x)
    ks, bs, dists = U.select(z, J, 2, metric)
    assert ks == 1 and dists[1] == dists[3] == bs and dists[2] is None and dists[4] is None and bool(np.isnan(J[4]).any())
    # k == y is never chosen, although its "distance" would be 0
    assert all(int(plane(m, x, torch.tensor([c]))[2]) != c for c in range(5))
    # every class skipped: zero gradients everywhere - nothing chosen, and the iteration does not move
    flat = _Affine(torch.zeros(5, 4), torch.tensor([0.0, 0.1, 1.0, 0.2, 0.3]))
    w, df, k, best = plane(flat, x, y)
    assert k.tolist() == [-1] and float(df) == 0 and float(best) == float("inf") and not bool(w.any())
    x1 = torch.full((1, 1, 2, 2), 0.25, dtype=torch.float64)
    x_new, adv, res, info = host_iteration(metric, flat, x1, x, y, x.clone(), torch.full((1,), float("inf"), dtype=torch.float64))
    assert torch.equal(x_new, x1) and not bool(info["enabled"].any()) and float(info["s1"]) == 0 and torch.equal(adv, x) and float(res) == float("inf")
    ref = U.iterate(flat, x1, x, 2, x.clone(), float("inf"), metric)
    assert ref["best_k"] == -1 and not ref["enabled"] and torch.equal(ref["x"], x1)


# ---- the closed form on a linear classifier ------------------------------------------------------------------------------------------
def linear_case(dtype, seed=11, B=6, D=48, K=12):
    """z = A x + c, K = 12, x0 = 0.5 +- 0.01, the label is class 0 (zero weights, logit 0.5).  Classes 1 .. 10 are its runners-up by logit
    (0.065 .. 0.2) with weights of 1e-3: their boundaries lie outside the box in every metric.  Class 11 has the LOWEST logit (about 0,
    |df| about 0.5) and weights of 0.25, one of 2 (zero mean, so its logit does not depend on the 0.5): its boundary is by far the closest - and it is
    not among the nine classes FAB_T targets.  Returns (model, x0, y, A, c) with A, c float64."""
    g = torch.Generator().manual_seed(seed)
    A = torch.zeros(K, D, dtype=torch.float64)
    small = 1e-3 * torch.randn(K - 2, D, generator=g, dtype=torch.float64)
    A[1:K - 1] = small - small.mean(dim=1, keepdim=True)
    big = 0.25 * torch.randn(D, generator=g, dtype=torch.float64)
    big[7] = 2.0  # one dominant coordinate: the L1 boundary (|df| / max |a_i|) is then reachable inside the box too
    A[K - 1] = big - big.mean()
    c = torch.zeros(K, dtype=torch.float64)
    c[0] = 0.5
    c[1:K - 1] = 0.05 + 0.015 * torch.arange(1, K - 1, dtype=torch.float64)
    fc = torch.nn.Linear(D, K).to(dtype)
    with torch.no_grad():
        fc.weight.copy_(A)
        fc.bias.copy_(c)
    m = torch.nn.Sequential(torch.nn.Flatten(), fc)
    x0 = (0.5 + 0.02 * (torch.rand(B, 3, 4, 4, generator=g, dtype=torch.float64) - 0.5)).to(dtype)
    return m, x0, torch.zeros(B, dtype=torch.int64), fc.weight.detach().double(), fc.bias.detach().double()


def closest_boundary(x0, y, A, c, metric):
    """(d* [B], k* [B], cond [B]) in float64: d* = min_k |df_k| / ||a_k - a_y||_dual; cond = the size of the two sums behind df_k* over |df_k*|."""
    f = x0.flatten(1).double()
    z = f @ A.t() + c
    B, K = z.shape
    G = A.unsqueeze(0) - A[y].unsqueeze(1)  # [B, K, D]
    n = {"Linf": G.abs().sum(dim=2), "L2": (G ** 2).sum(dim=2).sqrt(), "L1": G.abs().max(dim=2)[0]}[metric]
    df = z - z[torch.arange(B), y].view(-1, 1)
    dist = torch.where(n > 0, df.abs() / n, torch.full_like(n, float("inf")))
    dist[torch.arange(B), y] = float("inf")
    d, k = dist.min(dim=1)
    size = f.abs() @ A.abs().t() + c.abs()
    cond = (size[torch.arange(B), k] + size[torch.arange(B), y]) / df[torch.arange(B), k].abs()
    return d, k, cond, z


@pytest.mark.parametrize("metric", METRICS)
def test_linear_classifier_bound_in_float64(cpu_plumbing, metric):
    """The first step lands at 1.05 d* exactly on the closest boundary when the box is inactive (asserted), and later adversarial iterates
    can only be closer: d* <= norm <= 1.05 d*, up to the slack of the metric's FAB-T test of the same name - (D + 8) 2^-52, for L1 times the
    conditioning of df.  The closest class is none of the nine runners-up: FAB_T cannot reach a boundary inside the box at all."""
    import utils.attacks as A
    n_iter = 5
    m, x0, y, W, c = linear_case(torch.float64)
    D = x0[0].numel()
    dist, kstar, cond, z = closest_boundary(x0, y, W, c, metric)
    order = torch.sort(z, dim=1, descending=True, stable=True)[1]
    assert bool((order[:, 0] == y).all()) and bool((kstar == 11).all()) and bool((order[:, 11] == 11).all())  # class 11: last by logit, first by distance
    assert float(1.05 * dist.max()) < 0.45
    margin = (D + 8) * EPS64 * (cond if metric == "L1" else 1.0)
    trace = []
    adv, res = host_run(metric, m, x0, y, n_iter, trace=trace)
    first = torch.full_like(dist, float("inf"))
    for e in reversed(trace):
        assert bool((e["x_step"] > 0).all()) and bool((e["x_step"] < 1).all())  # the box never binds
        assert bool((e["best_k"] == 11).all())
        first = torch.where(e["is_adv"], e["nrm"], first)
    assert bool((first >= dist * (1 - margin)).all()) and bool((first <= 1.05 * dist * (1 + margin)).all())
    assert bool((res <= first).all()) and bool((res >= dist * (1 - margin)).all())
    _, res_r, _ = U.run(m, x0, y, n_iter, metric)
    assert bool((res_r >= dist * (1 - margin)).all()) and bool((res_r <= 1.05 * dist * (1 + margin)).all())
    args = Args(epsilon=2 * float(dist.max()))
    if metric == "L1":
        x_adv, robust, norm = A.FAB_L1(m, args, x0, y, n_iter=n_iter)
        norm_t = A.FAB_T_L1(m, args, x0, y, 12, n_iter=n_iter)[2]
    else:
        x_adv, robust, norm = A.FAB(m, args, x0, y, n_iter=n_iter, norm=metric)
        norm_t = A.FAB_T(m, args, x0, y, 12, n_iter=n_iter, norm=metric)[2]
    assert torch.equal(norm, res) and not bool(robust.any())
    with torch.no_grad():
        assert bool((m(x_adv).argmax(1) != y).all())
    assert bool((norm_t > norm).all())  # nine runs towards the runners-up miss the closest boundary


def test_public_interface(cpu_plumbing):
    import utils.attacks as A
    from eeadv import engine, trainer
    m, x0, y, _, _ = linear_case(torch.float32)
    with pytest.raises(ValueError, match="norm"):
        A.FAB(m, Args(epsilon=0.1), x0, y, n_iter=2, norm="L1")
    with pytest.raises(ValueError, match="norm"):
        A._fab_u_host(m, x0, y, 2, norm="L1")
    y2 = y.clone()
    y2[1] = 3  # misclassified before any attack: norm 0, the clean point is its own adversarial example
    xa, robust, norm = A.FAB(m, Args(epsilon=1.0), x0, y2, n_iter=2)
    assert float(norm[1]) == 0 and not bool(robust[1]) and torch.equal(xa[1], x0[1]) and torch.equal(robust, ~(norm <= 1.0))
    xs, rs, ns = A.FAB(m, Args(epsilon=1.0), x0, y2, n_iter=2, eps=1e-6)  # eps overrides args.epsilon and only thresholds
    assert torch.equal(ns, norm) and rs.tolist() == [True, False, True, True, True, True] and torch.equal(xs, x0)
    assert trainer.FAB_U_METHODS == ("FAB-U",) and trainer.L1_FAB_U_METHODS == ("FAB-L1-U",)
    assert {"FAB-U", "FAB-L1-U"} <= set(trainer.EVAL_METHODS) and not {"FAB-U", "FAB-L1-U"} & set(trainer.L2_METHODS)
    assert trainer.norm_tag(Args(attack_method="FAB-L1-U")) == " [norm L1]" and trainer.norm_tag(Args(attack_method="FAB-U")) == ""
    for name in ("fab_u_loop", "fab_u_l1_loop", "_FabURun", "_FabUL1Run"):
        assert hasattr(engine, name)
    assert issubclass(engine._FabURun, engine._FabRun) and issubclass(engine._FabUL1Run, engine._FabURun)
    for method, fn in (("FAB-U", "FAB"), ("FAB-L1-U", "FAB_L1")):
        a = Args(epsilon=0.05, method_name="AT", attack_method=method, random=True, fab_iters=2)
        out = trainer.attack_for_validation(m, a, x0, y, torch.device("cpu"), 3, 0.01, 12)
        assert torch.equal(out, getattr(A, fn)(m, a, x0, y, 2)[0])
        a.eot_iter = 2
        with pytest.raises(NotImplementedError, match="eot_iter"):
            trainer.attack_for_validation(m, a, x0, y, torch.device("cpu"), 3, 0.01, 12)
        a.eot_iter, a.norm = None, "L2"
        with pytest.raises(NotImplementedError, match="norm"):
            trainer.attack_for_validation(m, a, x0, y, torch.device("cpu"), 3, 0.01, 12)
        a.norm, a.method_name = None, "tar_AT"
        with pytest.raises(NotImplementedError, match="untargeted"):
            trainer.attack_for_validation(m, a, x0, y, torch.device("cpu"), 3, 0.01, 12)


# ---- drivers ---------------------------------------------------------------------------------------------------------------------------
def _mnist(tmp_path, *extra):
    return subprocess.run([sys.executable, "experiments_mnist.py", "-c", "configs_mnist/adversarial_training.yml", "--no-cuda", "--data", "synthetic:1:1",
                           "--output-root", str(tmp_path), "-e", *extra], cwd=os.path.join(PKG, "MNIST"), capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("method,tag", [("FAB-U", ""), ("FAB-L1-U", " [norm L1]")])
def test_mnist_driver_evaluates_with_untargeted_fab_on_the_host(tmp_path, method, tag):
    r = _mnist(tmp_path, "--attack_method", method, "--fab_iters", "2")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    logs = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path)) for f in fs if f.startswith("log")]
    text = r.stdout + "".join(open(f).read() for f in logs)
    assert re.search(r"^ \* %s: K = 10 classes, 10 backward passes per iteration, 2 iterations$" % re.escape(method), text, flags=re.M)
    clean = re.findall(r"^ \* Clean Prec@1 ([\d.]+)", text, flags=re.M)
    adv = re.findall(r"^ \* Adv Prec@1 ([\d.]+) Prec@5 ([\d.]+)%s$" % re.escape(tag), text, flags=re.M)
    assert len(clean) >= 1 and len(clean) == len(adv)
    for c1, (a1, _) in zip(clean, adv):
        assert float(a1) <= float(c1)
    assert text.index("backward passes per iteration") < text.index("Test_clean")  # before the first batch


@pytest.mark.parametrize("extra,word", [(("--norm", "L2", "--attack_method", "FAB-U"), "norm"), (("--eot_iter", "2", "--attack_method", "FAB-U"), "eot_iter"),
                                        (("--eot_iter", "2", "--attack_method", "FAB-L1-U"), "eot_iter")])
def test_mnist_driver_stops_on_what_untargeted_fab_has_not(tmp_path, extra, word):
    r = _mnist(tmp_path, "--fab_iters", "2", *extra)
    assert r.returncode != 0 and "NotImplementedError" in r.stderr and word in r.stderr
    assert "Adv Prec@1" not in r.stdout
