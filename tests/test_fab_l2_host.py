"""CPU: FAB-T in the L2 threat model - the host projection of utils.attacks against tests/fab_l2_reference.py in
float64, the KKT conditions of the delta it returns, the host run against the reference run, the closed form on a linear classifier, the
`norm` keyword and the ABI of the three L2 launches.  `proj_cases` is shared with tests/test_gpu_fab_l2.py."""
import ctypes
import math

import numpy as np
import pytest
import torch

import fab_l2_reference as R
from tiny_models import Args

EPS64 = 2.0 ** -52
CASES = ("inactive", "clipped", "infeasible", "c_zero", "c_negative", "w_zero", "w_third_zero", "ends", "rooms_equal", "w_nan", "df_inf",
         "ratios_equal", "w_tiny")
NO_HYPERPLANE = ("c_zero", "w_zero", "w_nan", "df_inf")
TINY = {np.float32: 1e-40, np.float64: 1e-310}  # denormal in the dtype: r / |w| overflows to +inf for any room above 1e-2


def _room(v, p):
    one, zero = p.dtype.type(1), p.dtype.type(0)
    return np.maximum(np.where(v > 0, p, np.where(v < 0, one - p, zero)), zero).astype(p.dtype)


def proj_cases(D, reps, seed, dtype):
    """len(CASES) * reps samples (x, x0, w, df, names) in `dtype`: the case list of tests/test_gpu_fab.py (every branch of the projection
    among them) plus `ratios_equal` (half of the coordinates share one breakpoint r_i / |w_i|) and `w_tiny` (every third |w_i| denormal:
    its breakpoint is +inf and it never saturates; never coordinate 0, so D = 1 keeps a solution that fits the dtype)."""
    rng = np.random.default_rng(seed)
    f = dtype
    xs, x0s, ws, dfs, names = [], [], [], [], []
    for rep in range(reps):
        for name in CASES:
            x = rng.random(D).astype(f)
            w = rng.standard_normal(D).astype(f)
            frac, sign = 0.3, 1.0
            if name == "clipped":
                x[::2] = np.where(rng.random(x[::2].size) < 0.5, 0.01, 0.99).astype(f)
                frac = 0.6
            if name == "c_negative":
                sign = -1.0
            if name == "w_zero":
                w[:] = 0
            if name == "w_third_zero":
                w[::3] = 0
                frac = 0.4
            if name == "ends":  # what a clamped iterate looks like: rooms of exactly 0, massive ties
                x[::2] = np.where(rng.random(x[::2].size) < 0.5, 0.0, 1.0).astype(f)
                frac = 0.5
            if name == "rooms_equal":
                x[:] = 0.5
            if name == "ratios_equal":  # rooms 0.5 and |w| = 0.75 on every second coordinate: one quotient, one breakpoint
                x[::2] = 0.5
                w[::2] = np.where(rng.random(w[::2].size) < 0.5, -0.75, 0.75).astype(f)
                frac = (0.2, 0.5, 0.8)[rep % 3]
            if name == "w_tiny":
                w[1::3] = np.where(rng.random(w[1::3].size) < 0.5, -TINY[f], TINY[f]).astype(f)
            x0 = np.clip(x + (rng.random(D).astype(f) - f(0.5)) * f(0.1), 0, 1).astype(f)
            if name == "ends":
                x0[::4] = x[::4]
            a, r = np.abs(w), _room(f(sign) * w, x)
            ginf = float(np.sum(a.astype(np.float64) * r))
            df = sign * frac * ginf
            if name == "inactive":  # mu a_i below every room: mu = c' / sum a^2 <= 0.5 min_i (r_i / a_i)
                t = (r[a != 0] / a[a != 0]).astype(np.float64)
                df = 0.5 * float(t.min()) * float(np.sum(a.astype(np.float64) ** 2)) if t.size else 0.0
            if name == "infeasible":
                df = 2.0 * ginf + 1.0
            if name == "c_zero":
                df = 0.0
            if name == "w_nan":
                w[D // 2] = np.nan
            if name == "df_inf":
                df = np.inf if rep % 2 == 0 else -np.inf
            xs.append(x), x0s.append(x0), ws.append(w), dfs.append(f(df)), names.append(name)
    return np.stack(xs), np.stack(x0s), np.stack(ws), np.array(dfs, dtype=f), names


def problems(x, x0, w, df):
    """The 2N projection problems (point, w, c, enabled) of N samples as every implementation forms them: q < N projects x[q] with c = df,
    q >= N projects x0 with c = df + sum w (x0 - x) rounded to the dtype of the inputs."""
    N = x.shape[0]
    out = [None] * (2 * N)
    for b in range(N):
        sabs = float(np.sum(np.abs(w[b]).astype(np.float64)))
        on = bool(np.isfinite(df[b]) and df[b] != 0 and np.isfinite(sabs) and sabs > 0)
        dot = math.fsum((w[b].astype(np.float64) * (x0[b] - x[b]).astype(np.float64)).tolist()) if on else 0.0
        out[b] = (x[b], w[b], df[b], on)
        out[N + b] = (x0[b], w[b], df.dtype.type(float(df[b]) + dot), on)
    return out


def segment(p, w, c, mu):
    """(S, A) of the segment that holds mu: S = sum of a_i r_i over the saturated coordinates, A = sum of a_i^2 over the others."""
    s = 1.0 if c >= 0 else -1.0
    a, r = R.rooms(np.asarray(p, dtype=np.float64), np.asarray(w, dtype=np.float64), s)
    keep = a != 0
    a, r = a[keep], r[keep]
    sat = r <= mu * a
    return float(np.sum(a[sat] * r[sat])), float(np.sum(a[~sat] ** 2))


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_l2_launches():
    import eeadv._native as n
    L = n.lib
    for name in ("ee_fab_proj_l2_f32", "ee_fab_step_l2_f32", "ee_fab_commit_l2_f32"):
        assert name in n.SIGNATURES and hasattr(L, name)
    assert L.ee_prof_read(29, None, None) != -2 and L.ee_prof_read(30, None, None) == -2  # no new kernel family: EE_K_COUNT stays
    p = ctypes.c_void_p(4096)
    assert L.ee_fab_proj_l2_f32(p, p, None, p, 2, 8, 0, p, None) == -1 and L.ee_fab_proj_l2_f32(p, p, p, p, 2, 8, 0, None, None) == -1
    assert L.ee_fab_proj_l2_f32(p, p, p, p, 2, 0, 0, p, None) == -2 and L.ee_fab_proj_l2_f32(p, p, p, p, 2, 8, 3, p, None) == -2
    assert L.ee_fab_proj_l2_f32(p, p, p, p, 2, 12289, 1, p, None) == -3  # the resident path ends at 3*64*64
    assert L.ee_fab_proj_l2_f32(None, None, None, None, 0, 8, 0, None, None) == 0
    assert L.ee_fab_proj_l2_f32(ctypes.c_void_p(4098), p, p, p, 2, 8, 0, p, None) == -4
    assert L.ee_fab_step_l2_f32(p, p, p, None, 2, 8, None) == -1 and L.ee_fab_step_l2_f32(p, p, p, p, -1, 8, None) == -2
    assert L.ee_fab_step_l2_f32(None, None, None, None, 0, 8, None) == 0 and L.ee_fab_step_l2_f32(p, ctypes.c_void_p(4098), p, p, 2, 8, None) == -4
    assert L.ee_fab_commit_l2_f32(p, p, 4, 10, p, p, p, p, p, p, None, 8, None) == -1
    assert L.ee_fab_commit_l2_f32(p, p, 4, 1, p, p, p, p, p, p, p, 8, None) == -2
    assert L.ee_fab_commit_l2_f32(None, None, 0, 10, None, None, None, None, None, None, None, 8, None) == 0


def test_l2_ops_refuse_cpu_tensors():
    from eeadv import ops
    import eeadv._native as n
    x = torch.rand(2, 8)
    with pytest.raises(n.EEError):
        ops.fab_proj_l2(x, x, x, torch.ones(2))
    with pytest.raises(n.EEError):
        ops.fab_step_l2_(x, x, x, torch.zeros(3, 4))


# ---- the host projection ---------------------------------------------------------------------------------------------------------------
def _host(p, w, c):
    import utils.attacks as A
    tp, tw, tc = torch.from_numpy(p)[None], torch.from_numpy(w)[None], torch.tensor([c], dtype=torch.float64)
    mu, s, n = A._fab_projection_l2(tp, tw, tc)
    return float(mu), float(s), float(n), A._fab_delta_l2(tp, tw, mu, s)[0].numpy()


@pytest.mark.parametrize("D", [1, 2, 3, 75, 192])
def test_host_projection_against_the_reference(D):
    """Every problem with a hyperplane.  mu = (c' - S) / A on the segment that holds it, S and A sums of at most D non-negative terms, each
    side off by at most (D + 8) 2^-52 of them: |mu - mu_ref| <= 2 (D + 8) 2^-52 ((c' + S) / A + mu).  The norm moves with mu by at most
    sqrt(A) per unit (d||delta|| / dmu = mu A' / ||delta|| <= sqrt(A'), A' <= A + the squares at the breakpoint) and carries its own sum."""
    x, x0, w, df, names = proj_cases(D, 2, 11 * D, np.float64)
    N, seen = x.shape[0], set()
    for q, (p, wq, c, on) in enumerate(problems(x, x0, w, df)):
        name = names[q % N]
        assert not (on and name in NO_HYPERPLANE) and (on or name in NO_HYPERPLANE or D < 3), name  # D < 3: a case can run out of coordinates
        if not on:
            continue
        seen.add(name)
        mu_r, s_r, n_r, d_r = R.project(p, wq, float(c))
        mu, s, n, d = _host(p, wq, float(c))
        assert s == s_r and math.isinf(mu) == math.isinf(mu_r), (name, mu, mu_r)
        if name == "infeasible" and q < N:
            assert math.isinf(mu_r)
        if math.isinf(mu_r):
            assert n == pytest.approx(n_r, rel=(D + 8) * EPS64) and np.array_equal(d, d_r)
            continue
        S, A = segment(p, wq, float(c), mu_r)
        tol = 2 * (D + 8) * EPS64 * ((abs(float(c)) + S) / A + mu_r)
        assert abs(mu - mu_r) <= tol, (name, mu, mu_r, tol)
        assert abs(n - n_r) <= tol * math.sqrt(sum(float(v) ** 2 for v in wq)) + (D + 8) * EPS64 * n_r, (name, n, n_r)
        if name == "inactive" and q < N:
            a, r = R.rooms(p, wq, s_r)
            assert (mu * a[a != 0] < r[a != 0]).all()
        if name == "w_tiny" and q < N and D > 1:
            a, r = R.rooms(p, wq, s_r)
            tiny = (a != 0) & (a < 1e-300)
            assert tiny.any() and (np.abs(d[tiny]) < r[tiny]).all()  # a denormal |w_i| never reaches its bound
        seen.add(name)
    assert seen == set(CASES) - set(NO_HYPERPLANE) if D >= 3 else len(seen) >= 6
    # c = 0: the point lies on the hyperplane
    mu, s, n, d = _host(x[0], w[0], 0.0)
    assert mu == 0 and s == 1 and n == 0 and not d.any()


def _grid_closest(p, w, c, n=401):
    """The smallest ||q - p||_2 over a fine grid of the feasible set {q in [0,1]^D : <w, q> = <w, p> - c}, D <= 3: the coordinate of the
    largest |w_i| is solved from the others, which run over the grid; inf when no grid point is feasible."""
    D = p.size
    k = int(np.argmax(np.abs(w)))
    rest = [i for i in range(D) if i != k]
    axes = np.meshgrid(*[np.linspace(0.0, 1.0, n)] * len(rest), indexing="ij") if rest else []
    target = float(np.dot(w, p)) - c
    acc = np.zeros(axes[0].shape if rest else ())
    for ax, i in zip(axes, rest):
        acc = acc + w[i] * ax
    qk = (target - acc) / w[k]
    ok = (qk >= 0) & (qk <= 1)
    d2 = (qk - p[k]) ** 2
    for ax, i in zip(axes, rest):
        d2 = d2 + (ax - p[i]) ** 2
    return float(np.sqrt(np.min(np.where(ok, d2, np.inf))))


@pytest.mark.parametrize("D", [1, 2, 3, 75, 192])
def test_host_delta_satisfies_the_kkt_conditions(D):
    x, x0, w, df, names = proj_cases(D, 2, 13 * D + 1, np.float64)
    N, checked, grids = x.shape[0], 0, 0
    for q, (p, wq, c, on) in enumerate(problems(x, x0, w, df)):
        if not on:
            continue
        c = float(c)
        mu, s, n, d = _host(p, wq, c)
        a, r = R.rooms(p, wq, s)
        point = p + d
        assert (point >= 0).all() and (point <= 1).all(), names[q % N]
        with np.errstate(invalid="ignore"):
            want = np.where(a != 0, -np.sign(s * wq) * np.minimum(mu * a, r), 0.0)
        assert np.array_equal(d, want), names[q % N]
        assert not d[wq == 0].any()
        assert n == pytest.approx(R.l2(d), rel=(D + 8) * EPS64)
        if math.isinf(mu):
            assert np.array_equal(np.abs(d)[a != 0], r[a != 0])  # infeasible: every moving coordinate at its bound
            continue
        scale = float(np.sum(np.abs(wq * d))) + abs(c)
        assert abs(float(np.sum(wq * d)) + c) <= (D + 8) * EPS64 * scale, names[q % N]  # on the hyperplane
        checked += 1
        if D <= 3:
            # the grid's feasible points are exact solutions of the constraint: none may be closer than delta (its norm is off by rounding only)
            assert _grid_closest(p, wq, c) >= n * (1 - 1e-12), names[q % N]
            grids += 1
    assert checked >= 12 and (D > 3 or grids >= 12)


# ---- the host run against the reference run -----------------------------------------------------------------------------------------------
class _MLP(torch.nn.Module):
    def __init__(self, D, H, K, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.a, self.b = torch.nn.Linear(D, H).double(), torch.nn.Linear(H, K).double()
        with torch.no_grad():
            for lin in (self.a, self.b):
                lin.weight.copy_(torch.randn(lin.weight.shape, generator=g, dtype=torch.float64) / math.sqrt(lin.weight.shape[1]))
                lin.bias.copy_(0.1 * torch.randn(lin.bias.shape, generator=g, dtype=torch.float64))

    def forward(self, x):
        return self.b(torch.tanh(self.a(x.flatten(1))))


def _mlp_setup(B=5, K=6, seed=3):
    g = torch.Generator().manual_seed(seed)
    m = _MLP(48, 16, K, seed)
    x0 = 0.1 + 0.8 * torch.rand(B, 3, 4, 4, generator=g, dtype=torch.float64)
    x0[0, :, :1], x0[0, :, 1:2] = 0.0, 1.0  # one sample with pixels on both ends of the box
    with torch.no_grad():
        order = torch.sort(m(x0), dim=1, descending=True, stable=True)[1]
    return m, x0, order[:, 0].clone(), order[:, 1].clone()


def test_host_run_teacher_forced_against_the_reference_run():
    """B = 5, 3 iterations, float64; every host iteration starts from the reference's recorded state, so both sides take the gradient at
    the same point.  Flags, pred and signs equal.  Sums (the logits, the gradient) are held to bound = (D + K + 8) 2^-52 of their size; df
    is a difference of two logits, so everything proportional to it carries bound * cond, cond = (|z_t| + |z_y|) / |df|; mu = (c' - S) / A
    subtracts once more, so the scalars and the points carry bound * cond * amp, amp = the larger (c' + S) / (c' - S) of the two problems."""
    import utils.attacks as A
    n_iter = 3
    m, x0, y, t = _mlp_setup()
    B, K, D = x0.shape[0], 6, x0[0].numel()
    bound = (D + K + 8) * EPS64
    _, _, trace = R.run(m, x0, y, t, n_iter)
    n_adv = 0
    for i, e in enumerate(trace):
        x, adv, res, info = A._fab_host_iteration(m, e["x_in"], x0, y, t, e["adv_in"], e["res_in"], norm="L2")
        assert info["pred"].tolist() == e["pred"].tolist() and info["is_adv"].tolist() == e["is_adv"].tolist(), i
        assert info["improved"].tolist() == e["improved"].tolist() and info["enabled"].tolist() == e["enabled"].tolist(), i
        assert info["s1"].tolist() == e["s1"].tolist() and info["s2"].tolist() == e["s2"].tolist(), i
        assert bool(((info["df"] - e["df"]).abs() <= bound * (e["zt"].abs() + e["zy"].abs())).all()), i
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
        wmax = e["w"].flatten(1).abs().max(dim=1)[0].view(-1, 1)
        assert bool(((info["w"] - e["w"].flatten(1)).abs() <= bound * wmax).all()), i
        for got, want in ((info["x_step"], e["x_step"]), (x, e["x"]), (adv, e["adv"])):
            assert bool(((got - want).abs() <= tol.view(-1, 1, 1, 1) * want.abs().clamp_min(1.0)).all()), i
        n_adv += int(e["is_adv"].sum())
    assert n_adv > 0
    # and the free-running host run is the chain of its own iterations: res is the L2 distance of adv
    trace_h = []
    adv, res = A._fab_host(m, x0, y, t, n_iter, trace=trace_h, norm="L2")
    found = torch.isfinite(res)
    assert len(trace_h) == n_iter and bool(found.any())
    assert torch.equal(A._l2_norms(adv - x0)[found], res[found]) and torch.equal(adv[~found], x0[~found])


def test_host_iteration_rests_on_a_sample_without_a_hyperplane():
    import utils.attacks as A
    m, x0, y, t = _mlp_setup()
    t = t.clone()
    t[1] = y[1]  # df = 0 and w = 0
    x = (x0 * 0.9 + 0.05).clone()
    inf = torch.full((5,), float("inf"), dtype=torch.float64)
    _, _, _, info = A._fab_host_iteration(m, x, x0, y, t, x0.clone(), inf, norm="L2")
    assert not bool(info["enabled"][1]) and bool(info["enabled"][[0, 2, 3, 4]].all())
    assert torch.equal(info["x_step"][1], x[1]) and float(info["lam1"][1]) == 0 and float(info["s1"][1]) == 0 and float(info["n1"][1]) == 0
    ref = R.iterate(m, x[1:2], x0[1:2], int(y[1]), int(t[1]), x0[1:2], float("inf"))
    assert not ref["enabled"] and torch.equal(ref["x_step"], x[1:2])


# ---- the closed form on a linear classifier -------------------------------------------------------------------------------------------
class _Linear(torch.nn.Module):
    def __init__(self, D, seed, dtype):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.fc = torch.nn.Linear(D, 2).to(dtype)
        with torch.no_grad():
            self.fc.weight.copy_(torch.randn(2, D, generator=g, dtype=torch.float64) * 0.08)
            self.fc.bias.copy_(torch.tensor([0.3, -0.3], dtype=torch.float64))

    def forward(self, x):
        return self.fc(x.flatten(1))


def linear_case(dtype, seed=4, B=6, D=192):
    """One Linear(D, 2), x0 in [0.3, 0.7]: the nearest point of the decision boundary in L2 lies at d = |df| / ||w||_2, w = W_t - W_y, and
    moves coordinate i by d |w_i| / ||w||_2 - less than 0.25 here, so the box never binds (asserted by the callers)."""
    g = torch.Generator().manual_seed(seed + 100)
    m = _Linear(D, seed, dtype)
    x0 = (0.3 + 0.4 * torch.rand(B, 3, 8, 8, generator=g, dtype=torch.float64)).to(dtype)
    W, bias = m.fc.weight.detach().double(), m.fc.bias.detach().double()
    z = x0.flatten(1).double() @ W.t() + bias
    y = z.argmax(1)
    t = 1 - y
    rows = torch.arange(B)
    df = z[rows, t] - z[rows, y]
    wd = W[1] - W[0]
    dist = df.abs() / wd.norm()
    assert float((1.05 * dist * wd.abs().max() / wd.norm()).max()) < 0.25 and float(df.abs().min()) > 0.05
    return m, x0, y, t, df, dist


def test_linear_classifier_bound_in_float64():
    """x = x0 at the first iteration, so both projections are the same vector, of length d exactly when the box is inactive, and the step
    goes 1.05 of it: the first adversarial point lies within [d, 1.05 d] of x0 and the final res is at most that."""
    import utils.attacks as A
    from eeadv import runtime
    D, n_iter = 192, 5
    m, x0, y, t, df, dist = linear_case(torch.float64)
    margin = (D + 8) * EPS64
    trace = []
    adv, res = A._fab_host(m, x0, y, t, n_iter, trace=trace, norm="L2")
    first = torch.full_like(dist, float("inf"))
    for e in reversed(trace):
        assert bool((e["x_step"] > 0).all()) and bool((e["x_step"] < 1).all())  # the box never binds
        first = torch.where(e["is_adv"], e["nrm"], first)
    assert bool((first >= dist * (1 - margin)).all()) and bool((first <= 1.05 * dist * (1 + margin)).all())
    assert bool((res <= first).all()) and bool((res >= dist * (1 - margin)).all())
    _, res_r, _ = R.run(m, x0, y, t, n_iter)
    assert bool((res_r >= dist * (1 - margin)).all()) and bool((res_r <= 1.05 * dist * (1 + margin)).all())
    runtime.allow_cpu_plumbing(True)
    try:
        x_adv, robust, norm = A.FAB_T(m, Args(epsilon=2 * float(dist.max())), x0, y, 2, n_iter=n_iter, norm="L2")
    finally:
        runtime.allow_cpu_plumbing(False)
    assert torch.equal(norm, res) and not bool(robust.any()) and torch.equal(A._l2_norms(x_adv - x0), norm)
    with torch.no_grad():
        assert bool((m(x_adv).argmax(1) != y).all())


# ---- the keyword -----------------------------------------------------------------------------------------------------------------------
def test_norm_keyword():
    import utils.attacks as A
    from eeadv import engine, runtime
    from tiny_models import TinyNet
    torch.manual_seed(0)
    m = TinyNet(3, 8, 10, 5).eval()
    x = torch.rand(4, 3, 8, 8)
    with torch.no_grad():
        y = m(x).argmax(1)
    a = Args(epsilon=0.5)
    runtime.allow_cpu_plumbing(True)
    try:
        plain = A.FAB_T(m, a, x, y, 10, n_iter=3, n_target_classes=2)
        linf = A.FAB_T(m, a, x, y, 10, n_iter=3, n_target_classes=2, norm="Linf")
        l2 = A.FAB_T(m, a, x, y, 10, n_iter=3, n_target_classes=2, norm="L2")
        with pytest.raises(ValueError, match="norm"):
            A.FAB_T(m, a, x, y, 10, n_iter=3, n_target_classes=2, norm="L1")
    finally:
        runtime.allow_cpu_plumbing(False)
    assert all(torch.equal(p, q) for p, q in zip(plain, linf))
    found = torch.isfinite(l2[2])
    assert bool(found.any()) and not torch.equal(l2[2], plain[2])
    assert bool((l2[2][found] >= plain[2][found]).all())  # ||.||_2 >= ||.||_inf of the closest points of the two metrics
    with pytest.raises(ValueError, match="norm"):
        A._fab_host(m, x, y, y, 1, norm="L1")
    with pytest.raises(ValueError, match="norm"):
        engine.fab_loop(m, x, y, y, 1, 0.5, norm="L1")
    with pytest.raises(ValueError, match="norm"):
        engine._FabRun(x, y, 1, 0.5, norm="l2")
