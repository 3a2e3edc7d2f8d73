"""GPU: the FAB-T kernels (ee_fab.hip) and engine.fab_loop against tests/fab_reference.py.

Bit-exact: df and its gradient, the step and the commit (fp32 on both sides, the same operations in the same order), the two paths of the
projection against each other, eager against graph replay.  In tolerance: the projection's lambda against the float64 reference on the
same fp32 inputs, held to twice the error of a plain float32 restatement (sort + sequential cumsum) on the same cases, 4 ulp at least."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import fab_reference as R
from tiny_models import Args, TinyNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")
INF = float("inf")


@pytest.fixture(scope="module")
def ops():
    from eeadv import ops
    return ops


# ---- df, its gradient, pred ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K", [(B, K) for B in (1, 5, 130) for K in (2, 3, 10, 200, 1000)])
def test_diff_kernel(ops, B, K):
    g = torch.Generator().manual_seed(1000 * B + K)
    z = 3 * torch.randn(B, K, generator=g)
    y = torch.randint(0, K, (B,), generator=g)
    t = torch.randint(0, K, (B,), generator=g)
    z[0, :] = z[0, 0]  # a row of ties: the lower index wins
    if B > 1:
        z[1, K - 1] = float("nan")  # NaN above everything
        y[1], t[1] = 0, K - 1
    if B > 2:
        z[2, K // 2] = z[2].max() + 1
        z[2, K - 1] = z[2, K // 2]  # a tie at the top, not at index 0
        t[3 % B] = y[3 % B]  # target == label: df = 0, the two entries cancel
    df, d, pred = ops.fab_diff(z.to(DEV), y.to(DEV), t.to(DEV))
    rows = torch.arange(B)
    want_df = z[rows, t] - z[rows, y]
    assert torch.equal(torch.nan_to_num(df.cpu(), nan=-12345.0), torch.nan_to_num(want_df, nan=-12345.0))  # one fp32 difference: the same bits
    want_d = torch.zeros(B, K)
    want_d[rows, t] += 1
    want_d[rows, y] -= 1
    assert torch.equal(d.cpu(), want_d)
    want_pred = [R.first_class(z[b])[0] for b in range(B)]
    assert pred.cpu().tolist() == want_pred
    assert pred[0].item() == 0 and (B < 2 or pred[1].item() == K - 1) and (B < 3 or K < 3 or pred[2].item() == K // 2)


# ---- the projection ------------------------------------------------------------------------------------------------------------------
CASES = ("inactive", "clipped", "infeasible", "c_zero", "c_negative", "w_zero", "w_third_zero", "ends", "rooms_equal", "w_nan", "df_inf")


def _room32(v, p):
    one, zero = np.float32(1), np.float32(0)
    return np.maximum(np.where(v > 0, p, np.where(v < 0, one - p, zero)), zero).astype(np.float32)


def _proj_inputs(D, reps, seed):
    """len(CASES) * reps samples (x, x0, w, df) in float32, every branch of the kernel among them."""
    rng = np.random.default_rng(seed)
    xs, x0s, ws, dfs, names = [], [], [], [], []
    for rep in range(reps):
        for name in CASES:
            x = rng.random(D).astype(np.float32)
            w = rng.standard_normal(D).astype(np.float32)
            frac, sign = 0.3, 1.0
            if name == "clipped":
                x[::2] = np.where(rng.random(x[::2].size) < 0.5, 0.01, 0.99).astype(np.float32)
                frac = 0.6
            if name == "c_negative":
                sign = -1.0
            if name == "w_zero":
                w[:] = 0
            if name == "w_third_zero":
                w[::3] = 0
                frac = 0.4
            if name == "ends":  # what a clamped iterate looks like: rooms of exactly 0, massive ties
                x[::2] = np.where(rng.random(x[::2].size) < 0.5, 0.0, 1.0).astype(np.float32)
                frac = 0.5
            if name == "rooms_equal":
                x[:] = 0.5
            x0 = np.clip(x + (rng.random(D).astype(np.float32) - np.float32(0.5)) * np.float32(0.1), 0, 1).astype(np.float32)
            if name == "ends":
                x0[::4] = x[::4]
            a, r = np.abs(w), _room32(np.float32(sign) * w, x)
            ginf = float(np.sum(a.astype(np.float64) * r))
            df = sign * frac * ginf
            if name == "inactive":  # lambda below every room
                moving = r[a != 0]
                df = 0.5 * float(moving.min()) * float(np.sum(a.astype(np.float64))) if moving.size else 0.0
            if name == "infeasible":
                df = 2.0 * ginf + 1.0
            if name == "c_zero":
                df = 0.0
            if name == "w_nan":
                w[D // 2] = np.nan
            if name == "df_inf":
                df = np.inf if rep % 2 == 0 else -np.inf
            xs.append(x), x0s.append(x0), ws.append(w), dfs.append(np.float32(df)), names.append(name)
    return np.stack(xs), np.stack(x0s), np.stack(ws), np.array(dfs, dtype=np.float32), names


def _proj_reference(x, x0, w, df):
    """Per problem q of 2N (q < N: point x, c = df; else point x0, c = float32(df + sum w (x0 - x))): the float64 reference's (lam, s) on
    the float32 inputs, the float32 restatement's lam, and whether the sample has a hyperplane at all."""
    N = x.shape[0]
    lam64, sgn, lam32, on = np.zeros(2 * N), np.zeros(2 * N), np.zeros(2 * N), np.zeros(2 * N, dtype=bool)
    for b in range(N):
        sabs = float(np.sum(np.abs(w[b]).astype(np.float64)))
        enabled = bool(np.isfinite(df[b]) and df[b] != 0 and np.isfinite(sabs) and sabs > 0)
        if not enabled:
            continue
        dot = float(np.sum(w[b].astype(np.float64) * (x0[b] - x[b]).astype(np.float64)))
        for q, p, c in ((b, x[b], df[b]), (N + b, x0[b], np.float32(float(df[b]) + dot))):
            on[q] = True
            lam, s, _, _ = R.project(p.astype(np.float64), w[b].astype(np.float64), float(c))
            lam64[q], sgn[q] = lam, s
            lam32[q] = 0.0 if c == 0 else R.lambda_f32(p, w[b], c)
    return lam64, sgn, lam32, on


def _rel_err(got, want):
    finite = np.isfinite(want) & (want != 0)
    err = np.zeros_like(want)
    err[finite] = np.abs(got[finite] - want[finite]) / np.abs(want[finite])
    return err


def _step_torch(x, x0, w, scal):
    """ee_fab_step_f32 in torch float32 on the CPU, the kernel's operations in the kernel's order; also returns delta1, delta2."""
    B = x.shape[0]
    l1, l2, s1, s2, n1, n2 = (scal[0, :B], scal[0, B:], scal[1, :B], scal[1, B:], scal[2, :B], scal[2, B:])
    col = lambda v: v.view(-1, 1)

    def room(v, p):
        return torch.where(v > 0, p, torch.where(v < 0, 1 - p, torch.zeros_like(p))).clamp_min(0)

    v1, v2 = col(s1) * w, col(s2) * w
    d1 = -torch.sign(v1) * torch.minimum(col(l1), room(v1, x))
    d2 = -torch.sign(v2) * torch.minimum(col(l2), room(v2, x0))
    a1, a2 = n1.clamp_min(1e-8), n2.clamp_min(1e-8)
    alpha = col(torch.minimum(a1 / (a1 + a2), torch.tensor(0.1, dtype=torch.float32)))
    out = torch.clamp((x + 1.05 * d1) * (1 - alpha) + (x0 + 1.05 * d2) * alpha, 0, 1)
    return torch.where(col(s1) == 0, x, out), d1, d2, room(v1, x), room(v2, x0)


@pytest.mark.parametrize("D,reps", [(D, reps) for D in (1, 3, 5, 75, 1023, 192, 3 * 64 * 64) for reps in (1, 3)])
def test_projection_kernel(ops, D, reps):
    """Both paths on every branch.  The yardstick E is measured here: the largest relative error of the float32 restatement against the
    float64 reference over this test's cases; the kernel may miss the reference by 2 E (another summation order), 4 ulp at least."""
    x, x0, w, df, names = _proj_inputs(D, reps, 7 * D + reps)
    N = x.shape[0]
    lam64, sgn, lam32, on = _proj_reference(x, x0, w, df)
    E = float(_rel_err(lam32, lam64).max())
    print("D = %d, %d problems: float32 restatement error E = %.3e" % (D, 2 * N, E))
    tx, t0, tw, tdf = (torch.from_numpy(a) for a in (x, x0, w, df))
    outs = {}
    for path in ("resident", "streaming"):
        outs[path] = ops.fab_proj_linf(tx.to(DEV), t0.to(DEV), tw.to(DEV), tdf.to(DEV), path).cpu()
    assert torch.equal(outs["resident"], outs["streaming"])  # one summation order on both paths: the same bits
    assert torch.equal(ops.fab_proj_linf(tx.to(DEV), t0.to(DEV), tw.to(DEV), tdf.to(DEV)).cpu(), outs["resident"])
    scal = outs["resident"]
    lam, s, nrm = scal[0].numpy().astype(np.float64), scal[1].numpy(), scal[2].numpy()
    # samples without a hyperplane rest: lambda = 0, s = 0, norm = 0 in both problems
    assert not on[[q for q in range(2 * N) if names[q % N] in ("c_zero", "w_zero", "w_nan", "df_inf")]].any()
    assert (lam[~on] == 0).all() and (s[~on] == 0).all() and (nrm[~on] == 0).all()
    assert (s[on] == sgn[on]).all()
    assert all(lam[q] == INF for q in range(N) if names[q] == "infeasible")
    assert (np.isinf(lam) == np.isinf(lam64)).all() and (lam[np.isinf(lam)] > 0).all()
    assert all(s[q] == -1 for q in range(N) if names[q] == "c_negative")
    for q in range(N):
        if names[q] == "inactive" and on[q]:
            assert lam[q] < _room32(w[q], x[q])[w[q] != 0].min()
    err = _rel_err(lam, lam64)
    tol = np.maximum(2 * E, 4 * np.spacing(np.abs(lam64).astype(np.float32)).astype(np.float64) / np.maximum(np.abs(lam64), 1e-300))
    finite = np.isfinite(lam64) & (lam64 != 0)
    print("kernel error max %.3e (tolerance 2 E = %.3e, 4 ulp = %.3e)" % (err.max(), 2 * E, 4 * 2.0 ** -23))
    assert (err[finite] <= tol[finite]).all(), (err.max(), E)
    assert (lam[lam64 == 0] == 0).all()
    # with the returned scalars: delta_i = -sign(s w_i) min(lambda, r_i), 0 where w_i = 0, inside the rooms, its largest entry the returned norm
    want_x, d1, d2, r1, r2 = _step_torch(tx, t0, tw, scal)
    for d, r, nq in ((d1, r1, scal[2, :N]), (d2, r2, scal[2, N:])):
        assert bool((d[tw == 0] == 0).all()) and bool((d.abs() <= r).all())
        assert torch.equal(d.abs().max(dim=1)[0], nq)
        assert bool((d[~torch.from_numpy(on[:N])] == 0).all())
    xd = tx.to(DEV)
    ops.fab_step_(xd, t0.to(DEV), tw.to(DEV), scal.to(DEV))
    assert torch.equal(xd.cpu(), want_x)


# ---- step and commit -----------------------------------------------------------------------------------------------------------------
def _state(B, P, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, P, generator=g)
    x = torch.clamp(x0 + (torch.rand(B, P, generator=g) - 0.5) * 0.2, 0, 1)
    x[:, ::5] = 0.0
    x[:, 3::5] = 1.0
    w = torch.randn(B, P, generator=g)
    special = torch.tensor([0.0, -0.0, float("nan"), 1e-30, -1e30])
    w.view(-1)[::4] = special[torch.arange(w.view(-1)[::4].numel()) % 5]
    return x, x0, w, g


@pytest.mark.parametrize("P,B", [(P, B) for P in (1, 3, 5, 75, 1023, 192) for B in (1, 3, 7)])
def test_step_kernel_bit_exact(ops, B, P):
    x, x0, w, g = _state(B, P, 100 * B + P)
    for trial in range(3):
        lam = torch.rand(2 * B, generator=g) * (0.05, 0.5, 2.0)[trial]
        lam[trial % (2 * B)] = INF
        sgn = torch.where(torch.rand(2 * B, generator=g) < 0.5, -1.0, 1.0)
        nrm = torch.minimum(lam, torch.rand(2 * B, generator=g))
        nrm[(trial + 1) % (2 * B)] = 0.0  # below the 1e-8 floor
        if B > 1:  # a sample without a hyperplane keeps its x
            lam[1], lam[B + 1], sgn[1], sgn[B + 1], nrm[1], nrm[B + 1] = 0, 0, 0, 0, 0, 0
        scal = torch.stack([lam, sgn, nrm])
        want = _step_torch(x, x0, w, scal)[0]
        xd = x.to(DEV)
        ops.fab_step_(xd, x0.to(DEV), w.to(DEV), scal.to(DEV))
        got = xd.cpu()
        assert torch.equal(got, want), (trial, B, P)
        assert bool((got >= 0).all()) and bool((got <= 1).all())
        if B > 1:
            assert torch.equal(got[1], x[1])
    # a view at an odd offset: the 16-byte path is not taken, the result is the same
    import ctypes
    from eeadv import _native as N
    pad = torch.zeros(3, B * P + 1, device=DEV)
    views = [pad[i, 1:].view(B, P) for i in range(3)]
    for v, src in zip(views, (x, x0, w)):
        v.copy_(src)
    sd = scal.to(DEV)
    rc = N.lib.ee_fab_step_f32(*[ctypes.c_void_p(v.data_ptr()) for v in views], ctypes.c_void_p(sd.data_ptr()), B, P,
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(views[0].cpu(), want)


@pytest.mark.parametrize("P,B", [(P, B) for P in (1, 3, 5, 75, 1023, 192) for B in (1, 3, 7)])
def test_commit_kernel_bit_exact(ops, B, P):
    """Per sample one of: adversarial and closer (adv, res take it), adversarial but not closer, not adversarial, NaN logits (never
    adversarial); `shift` moves the cases over the samples so that every B sees all four.  The counter advances by one per launch."""
    K = 5
    x, x0, _, g = _state(B, P, 300 * B + P)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    for shift in range(4):
        y = torch.randint(0, K, (B,), generator=g)
        z = torch.randn(B, K, generator=g)
        nrm = (x - x0).abs().max(dim=1)[0]
        res = torch.full((B,), INF)
        case = [(b + shift) % 4 for b in range(B)]
        for b, c in enumerate(case):
            z[b, y[b]] = z[b].max() + 1  # the label is on top ...
            if c in (0, 1, 3):
                z[b, (y[b] + 1) % K] = z[b, y[b]] + 1  # ... unless another class is above it
            if c == 2 and y[b] < K - 1:
                z[b, K - 1] = z[b, y[b]]  # a tie with a higher index: the label wins it
            if c == 1:
                res[b] = nrm[b]  # equal is not closer
            if c == 3:
                z[b, (y[b] + 2) % K] = float("nan")
        adv0 = torch.rand(B, P, generator=g)
        xd, advd, resd = x.to(DEV), adv0.to(DEV), res.to(DEV)
        pred = torch.zeros(B, dtype=torch.int32, device=DEV)
        flags = torch.zeros(B, dtype=torch.int32, device=DEV)
        ops.fab_commit_(z.to(DEV), y.to(DEV), xd, x0.to(DEV), advd, resd, pred, flags, counter)
        want_flags = [{0: 3, 1: 1, 2: 0, 3: 0}[c] for c in case]
        assert flags.cpu().tolist() == want_flags, (shift, case)
        assert pred.cpu().tolist() == [R.first_class(z[b])[0] for b in range(B)]
        is_adv = torch.tensor([f & 1 for f in want_flags], dtype=torch.bool).view(-1, 1)
        improved = torch.tensor([f & 2 for f in want_flags], dtype=torch.bool)
        assert torch.equal(xd.cpu(), torch.where(is_adv, x0 + 0.9 * (x - x0), x))
        assert torch.equal(advd.cpu(), torch.where(improved.view(-1, 1), x, adv0))
        assert torch.equal(resd.cpu(), torch.where(improved, nrm, res))
        assert int(counter.item()) == shift + 1


def test_kernels_take_empty_batches(ops):
    e = torch.empty(0, 12, device=DEV)
    assert ops.fab_proj_linf(e, e.clone(), e.clone(), torch.empty(0, device=DEV)).shape == (3, 0)
    ops.fab_step_(e, e.clone(), e.clone(), torch.empty(3, 0, device=DEV))
    torch.cuda.synchronize()


# ---- teacher-forced trajectory ---------------------------------------------------------------------------------------------------------
def test_teacher_forced_trajectory(ops):
    """B = 4, 3x8x8, 6 iterations of the float64 reference; every launch is fed the reference's recorded state rounded to float32 and
    compared with the reference formulas evaluated in float64 ON THOSE ROUNDED INPUTS.  Flags equal; lambda within the bound of
    test_projection_kernel (2 E with E measured on these problems, 4 ulp at least); the stepped point within that bound propagated through
    the step: 1.05 (tol n1 + tol n2) for the two deltas, tol * alpha for the mixing weight, and 8 * 2^-24 for the float32 roundings of the
    six operations on values of at most 1.05."""
    K, n_iter = 10, 6
    g = torch.Generator().manual_seed(21)
    m = TinyNet(3, 8, K, 21).double()
    x0 = 0.1 + 0.8 * torch.rand(4, 3, 8, 8, generator=g, dtype=torch.float64)
    x0[0, :, :2], x0[0, :, 2:4] = 0.0, 1.0
    with torch.no_grad():
        order = torch.sort(m(x0), dim=1, descending=True, stable=True)[1]
    y, t = order[:, 0].clone(), order[:, 1].clone()
    _, _, trace = R.run(m, x0, y, t, n_iter)
    x0f = x0.float()
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    n_adv = 0
    for i, e in enumerate(trace):
        xf, wf, dff = e["x_in"].float(), e["w"].float(), e["df"].float()
        x2, o2, w2 = (a.flatten(1).numpy() for a in (xf, x0f, wf))
        lam64, sgn, lam32, on = _proj_reference(x2, o2, w2, dff.numpy())
        E = float(_rel_err(lam32, lam64).max())
        scal = ops.fab_proj_linf(xf.to(DEV), x0f.to(DEV), wf.to(DEV), dff.to(DEV)).cpu()
        lam = scal[0].numpy().astype(np.float64)
        tol = max(2 * E, 4 * 2.0 ** -23)
        assert (scal[1].numpy() == sgn).all() and on.all(), i
        assert (_rel_err(lam, lam64) <= tol).all(), (i, _rel_err(lam, lam64).max(), E)
        # the step in float64 from the rounded inputs and the reference's own projections
        B = 4
        want = np.zeros_like(x2, dtype=np.float64)
        atol = np.zeros(B)
        for b in range(B):
            l1, s1, n1, d1 = R.project(x2[b].astype(np.float64), w2[b].astype(np.float64), float(dff[b]))
            c2 = float(np.float32(float(dff[b]) + float(np.sum(w2[b].astype(np.float64) * (o2[b] - x2[b]).astype(np.float64)))))
            l2, s2, n2, d2 = R.project(o2[b].astype(np.float64), w2[b].astype(np.float64), c2)
            a1, a2 = max(n1, 1e-8), max(n2, 1e-8)
            alpha = min(a1 / (a1 + a2), 0.1)
            want[b] = np.clip((x2[b] + 1.05 * d1) * (1 - alpha) + (o2[b] + 1.05 * d2) * alpha, 0, 1)
            atol[b] = 1.05 * tol * (n1 + n2) + tol * alpha + 8 * 2.0 ** -24
        xd = xf.to(DEV)
        ops.fab_step_(xd, x0f.to(DEV), wf.to(DEV), scal.to(DEV))
        got = xd.cpu().flatten(1).numpy().astype(np.float64)
        assert (np.abs(got - want) <= atol[:, None]).all(), (i, np.abs(got - want).max())
        # the commit from the reference's stepped point and its second-forward logits
        xs = e["x_step"].float()
        xd, advd, resd = xs.to(DEV), e["adv_in"].float().to(DEV), e["res_in"].float().to(DEV)
        pred = torch.zeros(4, dtype=torch.int32, device=DEV)
        flags = torch.zeros(4, dtype=torch.int32, device=DEV)
        ops.fab_commit_(e["z2"].float().to(DEV), y.to(DEV), xd, x0f.to(DEV), advd, resd, pred, flags, counter)
        assert pred.cpu().tolist() == e["pred"].tolist(), i
        assert [f & 1 for f in flags.cpu().tolist()] == [int(v) for v in e["is_adv"].tolist()], i
        assert [(f >> 1) & 1 for f in flags.cpu().tolist()] == [int(v) for v in e["improved"].tolist()], i
        nrm = (xs - x0f).flatten(1).abs().max(dim=1)[0]
        assert torch.equal(resd.cpu(), torch.where(e["improved"], nrm, e["res_in"].float())), i
        assert torch.equal(advd.cpu(), torch.where(e["improved"].view(-1, 1, 1, 1), xs, e["adv_in"].float())), i
        assert torch.equal(xd.cpu(), torch.where(e["is_adv"].view(-1, 1, 1, 1), x0f + 0.9 * (xs - x0f), xs)), i
        n_adv += int(e["is_adv"].sum())
    assert n_adv > 0 and int(counter.item()) == n_iter


# ---- free-running on the ResNets -----------------------------------------------------------------------------------------------------
def _resnet(ee):
    from eeadv import models
    torch.manual_seed(5)
    if ee:
        m = models.make_resnet_ee(18, "tiny", True, cize=64, r=8, w=1.0, with_gf=False, low=38.0, high=76.0, alpha=0.0, sigma=1.0,
                                  type_canny="CannyFilter_step125_1", epsilon=16 / 255, n_queries=1)
    else:
        m = models.make_resnet(18, "tiny")
    return m.to(DEV).eval()


def _batch(m, seed, B=4):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 3, 64, 64, generator=g).to(DEV)
    with torch.no_grad():
        y = m(x).argmax(1)
    y[0] = (y[0] + 1) % 200  # one sample starts misclassified (for the edge-enhanced model the labels are one draw's predictions)
    return x, y


@pytest.mark.parametrize("ee", [False, True], ids=["resnet18", "resnet18_EE_square"])
def test_free_running_eager_equals_graph(ops, ee, monkeypatch):
    """FAB-T, two targets, 64 x 64, B = 4, eval mode, 4 iterations: eager and graph replay give the same bits, a second replay with new
    inputs equals a fresh eager run, and the results are valid.  The Add_Square draws of the edge-enhanced model are pinned by rewinding
    the device draw state before every run.  `a fresh forward misclassifies every non-robust x_adv` is checked for the plain model: with
    n_queries = 1 every forward of the edge-enhanced model draws a new square per sample and the point kept was adversarial under the draw
    of ITS iteration (the reason tests/test_gpu_apgd.py gives for the same check)."""
    import utils.attacks as A
    from eeadv import engine, runtime
    m = _resnet(ee)
    eps, n_iter = 16 / 255, 4
    args = Args(epsilon=eps)
    runtime.reseed()
    torch.manual_seed(9)
    state = runtime.draw_state(torch.device(DEV))
    batches = [_batch(m, 1), _batch(m, 2)]

    def attack(batch, graph):
        monkeypatch.setenv("EEADV_GRAPH", "1" if graph else "0")
        state.copy_(state0)
        return A.FAB_T(m, args, batch[0], batch[1], 200, n_iter=n_iter, n_target_classes=2)

    state0 = state.clone()
    attack(batches[0], True)  # builds the graph (the warm-up passes draw too)
    state0 = state.clone()
    eager = [attack(b, False) for b in batches]
    graph = [attack(b, True) for b in batches]
    found = 0
    for (xe, re_, ne), (xg, rg, ng), (x, y) in zip(eager, graph, batches):
        assert torch.equal(xe, xg) and torch.equal(re_, rg) and torch.equal(ne, ng)
        assert bool((xe >= 0).all()) and bool((xe <= 1).all())
        assert torch.equal(re_, ~(ne <= eps))
        assert torch.equal((xe - x).flatten(1).abs().max(dim=1)[0][~re_], ne[~re_])  # exactly: both are maxima of the same fp32 differences
        assert torch.equal(xe[re_], x[re_])  # robust rows are the clean inputs
        if not ee:
            with torch.no_grad():
                assert bool((m(xe).argmax(1) != y)[~re_].all())
        found += int((~re_).sum())
        print("non-robust %d of %d, norms %s" % (int((~re_).sum()), len(y), ne.tolist()))
    assert not torch.equal(eager[0][0], eager[1][0])
    # the two projection paths give the same run
    state.copy_(state0)
    x, y = batches[0]
    t = torch.fmod(y + 7, 200)
    a = engine.fab_loop(m, x, y, t, n_iter, 1.0, use_graph=False, path="resident")
    state.copy_(state0)
    b = engine.fab_loop(m, x, y, t, n_iter, 1.0, use_graph=False, path="streaming")
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    found += int((~a[1]).sum())
    assert found > 0
    engine.clear_graphs()


def test_linear_classifier_bound_on_the_device(ops):
    """One Linear(192, 2), the box never binds (checked on the CPU in tests/test_fab_host.py for this seed): dist = |df| / ||w||_1, and
    dist (1 - m) <= norm <= 1.05 dist (1 + m) with m = (D + K + 8) * 2^-23."""
    import utils.attacks as A
    from test_fab_host import linear_case
    D, K, n_iter = 192, 2, 5
    m32, x0, y, t, _, _ = linear_case(torch.float32)
    W = m32.fc.weight.detach().double()
    z = x0.flatten(1).double() @ W.t() + m32.fc.bias.detach().double()
    rows = torch.arange(x0.shape[0])
    df = z[rows, t] - z[rows, y]
    dist = df.abs() / (W[1] - W[0]).abs().sum()
    assert bool((df.abs() >= 0.5).all())
    eps = 2 * float(dist.max())
    x_adv, robust, norm = A.FAB_T(m32.to(DEV), Args(epsilon=eps), x0.to(DEV), y.to(DEV), 2, n_iter=n_iter)
    margin = (D + K + 8) * 2.0 ** -23
    norm = norm.cpu().double()
    print("norm / dist:", (norm / dist).tolist())
    assert bool((norm >= dist * (1 - margin)).all()) and bool((norm <= 1.05 * dist * (1 + margin)).all())
    assert not bool(robust.any())
    with torch.no_grad():
        assert bool((m32(x_adv).argmax(1).cpu() != y).all())


# ---- driver --------------------------------------------------------------------------------------------------------------------------
def test_tiny_imagenet_driver_evaluates_with_fab(tmp_path):
    cfg = open(os.path.join(PKG, "Tiny_ImageNet", "configs_tinyimagenet", "adversarial_training.yml")).read()
    cfg = re.sub(r"num_steps_(\d): \d+", r"num_steps_\1: 2", cfg).replace("batch_size: 100", "batch_size: 8").replace("print_freq: 50", "print_freq: 1")
    path = tmp_path / "fab.yml"
    path.write_text(cfg)
    r = subprocess.run([sys.executable, "experiments_tinyimagenet.py", "-c", str(path), "--output-root", str(tmp_path), "--data", "synthetic:1:1",
                        "-e", "--attack_method", "FAB-T", "--fab_iters", "2"], cwd=os.path.join(PKG, "Tiny_ImageNet"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    logs = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path)) for f in fs if f.startswith("log")]
    text = r.stdout + "".join(open(f).read() for f in logs)
    clean = re.findall(r"^ \* Clean Prec@1 ([\d.]+) Prec@5 ([\d.]+)$", text, flags=re.M)
    adv = re.findall(r"^ \* Adv Prec@1 ([\d.]+) Prec@5 ([\d.]+)$", text, flags=re.M)
    assert len(clean) >= 3 and len(clean) == len(adv)
    for (c1, _), (a1, _) in zip(clean, adv):
        assert float(a1) <= float(c1)
