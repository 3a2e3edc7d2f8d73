"""GPU: untargeted FAB - ee_fab_select_f32, the retained backward passes it rests on, and engine.fab_u_loop /
fab_u_l1_loop against tests/fab_u_reference.py.

Bit-exact: the select launch against a numpy restatement on dyadic inputs (every double sum is then exact in any order), its two access
widths against each other, the k-th backward pass off a retained forward against a fresh forward and backward, eager against graph replay.
In tolerance: the chosen class's distance on generic inputs (1e-6 relative: three float roundings of 2^-24 per side), the trajectory
(the tolerances of tests/test_gpu_fab.py::test_teacher_forced_trajectory), the closed form on a linear classifier."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import fab_reference as R
import fab_u_reference as U
from tiny_models import Args, TinyNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")
INF = float("inf")
METRICS = ("Linf", "L2", "L1")
SIZES = (1, 3, 5, 75, 192, 1023, 2049, 4100)  # the last two give a thread more than one group of four
K = 5


@pytest.fixture(scope="module")
def ops():
    from eeadv import ops
    return ops


# ---- the select launch -----------------------------------------------------------------------------------------------------------------
def _dual32(g, metric):
    """The kernel's n: the sum (or sum of squares) in float64 - exact on the dyadic grid, in any order - rounded to float32 once."""
    a = np.abs(g.astype(np.float64))
    if np.isnan(a).any():
        return np.float32(np.nan)
    if metric == "Linf":
        return np.float32(a.sum())
    if metric == "L2":
        return np.float32(np.sqrt((a * a).sum()))
    return np.float32(a.max())


def _select_numpy(G, z, y, metric, w0):
    """ee_fab_select_f32 over the classes 0 .. K-1 in order, restated: G [K, B, D], z [B, K] float32, y [B].  -> best, best_k, df, w"""
    Kc, B, D = G.shape
    best, best_k, df, w = np.full(B, np.inf, np.float32), np.full(B, -1, np.int32), np.zeros(B, np.float32), w0.copy()
    for k in range(Kc):
        for b in range(B):
            if not 0 <= y[b] < Kc or y[b] == k:
                continue
            d = np.float32(z[b, k] - z[b, y[b]])
            n = _dual32(G[k, b], metric)
            if not (np.isfinite(d) and np.isfinite(n)) or n == 0:
                continue
            dist = np.float32(np.abs(d) / np.float32(np.float32(1e-12) + n))
            if dist < best[b]:
                best[b], best_k[b], df[b], w[b] = dist, k, d, G[k, b]
    return best, best_k, df, w


ROW_CASES = ("generic", "tie", "nan_column", "zero_gradient", "label_outside", "label_negative")


def _dyadic_inputs(B, D, shift, seed):
    """Small integers x 2^-8.  Row b is case (b + shift) % 6: `tie` - classes 1 and 3 mirror each other and are the closest; `nan_column` -
    class 2 would be the closest but one element of its gradient is NaN; `zero_gradient` - class 1 would be, but its gradient is zero;
    the label outside [0, K) on either side.  Every row meets k == y with a non-zero gradient and df = 0: a distance of 0 that must not win."""
    rng = np.random.default_rng(seed)
    G = (rng.integers(-64, 65, (K, B, D)) / 256.0).astype(np.float32)
    z = (rng.integers(-512, 513, (B, K)) / 256.0).astype(np.float32)
    y = rng.integers(0, K, B)
    names = [ROW_CASES[(b + shift) % len(ROW_CASES)] for b in range(B)]
    big = np.where(rng.random(D) < 0.5, -0.25, 0.25).astype(np.float32)
    for b, name in enumerate(names):
        if name in ("tie", "nan_column", "zero_gradient"):
            y[b] = 0
            z[b] = z[b, 0] + (np.arange(K) + 1) * np.float32(0.25)  # every other class at least 64 grid steps away in df
        if name == "tie":
            G[1, b], G[3, b] = big, -big
            z[b, 1], z[b, 3] = z[b, 0] + np.float32(2.0 ** -8), z[b, 0] - np.float32(2.0 ** -8)
        if name == "nan_column":
            G[2, b] = big
            G[2, b, D // 2] = np.nan
            z[b, 2] = z[b, 0] + np.float32(2.0 ** -8)
        if name == "zero_gradient":
            G[1, b] = 0.0
            z[b, 1] = z[b, 0] - np.float32(2.0 ** -8)
        if name == "label_outside":
            y[b] = K
        if name == "label_negative":
            y[b] = -1
    return G, z, y.astype(np.int64), names


def _run_select(ops, G, z, y, metric, w0, garbage=True):
    Kc, B, D = G.shape
    dev = lambda a: torch.from_numpy(a).to(DEV)
    zd, yd = dev(z), dev(y)
    # what the launch of class 0 must not read: a best of 0 would block every class
    best = torch.zeros(B, device=DEV) if garbage else torch.full((B,), INF, device=DEV)
    best_k = torch.full((B,), 77, dtype=torch.int32, device=DEV)
    df = torch.full((B,), 5.0, device=DEV)
    w = dev(w0)
    for k in range(Kc):
        ops.fab_select(dev(np.ascontiguousarray(G[k])), zd, yd, k, metric, best, best_k, w, df)
    return best.cpu().numpy(), best_k.cpu().numpy(), df.cpu().numpy(), w.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("D", SIZES)
@pytest.mark.parametrize("B", (1, 3, 7))
def test_select_kernel_bit_exact(ops, B, D, metric):
    seen = set()
    for shift in range(len(ROW_CASES)):
        G, z, y, names = _dyadic_inputs(B, D, shift, 1000 * D + 10 * B + shift)
        w0 = np.full((B, D), 7.0, np.float32)  # rows that take no class keep it
        want = _select_numpy(G, z, y, metric, w0)
        got = _run_select(ops, G, z, y, metric, w0)
        for g_, w_, what in zip(got, want, ("best", "best_k", "df", "w")):
            assert _same_bits(g_, w_), (what, shift, names, g_, w_)
        best, best_k, df, w = got
        for b, name in enumerate(names):
            assert not 0 <= y[b] < K or best_k[b] != y[b]  # k == y is never chosen
            if name == "tie":
                assert best_k[b] == 1 and df[b] == np.float32(2.0 ** -8)  # classes 1 and 3 are equally close: the lower one
            if name == "nan_column":
                assert best_k[b] not in (-1, 2)
            if name == "zero_gradient":
                assert best_k[b] not in (-1, 1)
            if name in ("label_outside", "label_negative"):
                assert best_k[b] == -1 and best[b] == np.inf and df[b] == 0 and (w[b] == 7.0).all()
        seen |= set(names)
    assert seen == set(ROW_CASES)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("D", SIZES)
@pytest.mark.parametrize("B", (1, 3, 7))
def test_select_kernel_generic_inputs(ops, B, D, metric):
    """Standard normal gradients and logits: the chosen class's float64 distance is within 1e-6 relative of the float64 minimum (the float
    path rounds n, the sum 1e-12 + n and the quotient once each: 3 x 2^-24 per side, about 4e-7 for the two sides).  No case is excluded."""
    rng = np.random.default_rng(77 * D + B)
    G = rng.standard_normal((K, B, D)).astype(np.float32)
    z = rng.standard_normal((B, K)).astype(np.float32)
    y = rng.integers(0, K, B).astype(np.int64)
    best, best_k, df, w = _run_select(ops, G, z, y, metric, np.zeros((B, D), np.float32))
    for b in range(B):
        d64 = {}
        for k in range(K):
            if k != y[b]:
                d64[k] = abs(float(z[b, k]) - float(z[b, y[b]])) / (1e-12 + U.dual_norm(G[k, b], metric))
        k = int(best_k[b])
        assert k in d64
        lo = min(d64.values())
        assert d64[k] <= lo * (1 + 1e-6), (b, k, d64)
        assert abs(float(best[b]) - d64[k]) <= 1e-6 * d64[k]
        assert df[b] == np.float32(z[b, k] - z[b, y[b]]) and _same_bits(w[b], G[k, b])


@pytest.mark.parametrize("metric", METRICS)
def test_select_access_paths_give_the_same_bits(ops, metric):
    """An aligned D with 16-byte aligned rows takes 128-bit accesses; the same rows in views at offset 1 take the element-wise path."""
    B, D = 3, 192
    rng = np.random.default_rng(5)
    G = rng.standard_normal((K, B, D)).astype(np.float32)
    z = rng.standard_normal((B, K)).astype(np.float32)
    y = np.array([0, 2, 4], dtype=np.int64)
    w0 = np.zeros((B, D), np.float32)
    want = _run_select(ops, G, z, y, metric, w0)
    zd, yd = torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV)
    best, best_k, df = torch.zeros(B, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros(B, device=DEV)
    pad_g, pad_w = torch.zeros(B * D + 1, device=DEV), torch.zeros(B * D + 1, device=DEV)
    g, w = pad_g[1:].view(B, D), pad_w[1:].view(B, D)
    assert g.data_ptr() % 16 == 4 and g.is_contiguous()
    for k in range(K):
        g.copy_(torch.from_numpy(G[k]))
        ops.fab_select(g, zd, yd, k, metric, best, best_k, w, df)
    got = (best.cpu().numpy(), best_k.cpu().numpy(), df.cpu().numpy(), w.cpu().numpy())
    assert all(_same_bits(a, b) for a, b in zip(got, want))
    assert float(pad_w[0]) == 0


def test_empty_batches_launch_nothing(ops):
    from eeadv import engine
    e = torch.empty(0, 12, device=DEV)
    st = (torch.empty(0, device=DEV), torch.empty(0, dtype=torch.int32, device=DEV), e.clone(), torch.empty(0, device=DEV))
    ops.fab_select(e, torch.empty(0, 4, device=DEV), torch.empty(0, dtype=torch.int64, device=DEV), 1, "L2", *st)
    torch.cuda.synchronize()
    m = TinyNet(3, 8, 4, 1).to(DEV).eval()
    for out in (engine.fab_u_loop(m, torch.empty(0, 3, 8, 8, device=DEV), torch.empty(0, dtype=torch.int64, device=DEV), 2, 0.1),
                engine.fab_u_l1_loop(m, torch.empty(0, 3, 8, 8, device=DEV), torch.empty(0, dtype=torch.int64, device=DEV), 2, 0.1)):
        assert out[0].shape == (0, 3, 8, 8) and out[1].shape == (0,) and out[2].shape == (0,)


# ---- the retained forward ----------------------------------------------------------------------------------------------------------------
def _model(name):
    from eeadv import models
    torch.manual_seed(5)
    if name == "resnet18":
        return models.make_resnet(18, "tiny").to(DEV).eval(), (2, 3, 64, 64)
    if name == "resnet18_EE":
        return models.make_resnet_ee(18, "tiny", False, cize=64, r=8, w=1.0, with_gf=False, low=38.0, high=76.0, alpha=0.0, sigma=1.0,
                                     type_canny="CannyFilter_step125_1").to(DEV).eval(), (2, 3, 64, 64)
    return models.Net_2().to(DEV).eval(), (2, 1, 28, 28)


@pytest.mark.parametrize("name", ["resnet18", "resnet18_EE", "Net_2"])
def test_retained_backward_equals_a_fresh_one(ops, name):
    """Eval mode, batch 2, the route of the loop (the whole model under attack_forward(), input_grad_only()): the gradient of class k from
    the k-th backward pass over ONE retained forward equals, bit for bit, the one from a forward and backward of its own - no bridge
    consumes or overwrites what it saved.  Classes 0 .. 5 and the last one, in order."""
    from eeadv.functional import attack_forward, input_grad_only
    m, shape = _model(name)
    x = torch.rand(shape, generator=torch.Generator().manual_seed(3)).to(DEV).requires_grad_(True)
    with torch.no_grad():
        y = m(x).argmax(1)
    n_class = m(x.detach()).shape[1]
    classes = list(range(6)) + [n_class - 1]

    def forward():
        with torch.enable_grad(), attack_forward():
            return m(x)

    def backward(logits, k, retain):
        z = logits.detach().float().contiguous()
        d = ops.fab_diff(z, y, torch.full_like(y, k))[1]
        with input_grad_only():
            (g,) = torch.autograd.grad(logits, [x], grad_outputs=d, retain_graph=retain)
        return g.clone()

    kept = forward()
    retained = [backward(kept, k, True) for k in classes]
    again = backward(kept, classes[0], False)  # and the first class once more, after all the others
    for k, g in zip(classes, retained):
        fresh = backward(forward(), k, False)
        assert torch.equal(g, fresh), (name, k)
        assert bool(torch.isfinite(g).all()) and (bool((g != 0).any()) or bool((y == k).all()))
    assert torch.equal(again, retained[0])
    assert not torch.equal(retained[0], retained[1])


# ---- teacher-forced trajectory ---------------------------------------------------------------------------------------------------------
def test_teacher_forced_trajectory(ops):
    """K = 4, 3x8x8, B = 5, 3 iterations of the float64 reference (Linf).  Per iteration: the select launch is fed the reference's Jacobian
    rows and logits rounded to float32 and must pick the reference's class, with df the fp32 difference and w the chosen row; the device
    loop's own hyperplane at the recorded point picks the same class, df within (D + K + 8) 2^-23 of the two logits; then projection, step
    and commit with the tolerances of tests/test_gpu_fab.py::test_teacher_forced_trajectory."""
    from eeadv import engine
    from test_gpu_fab import _proj_reference, _rel_err
    Kc, n_iter, B = 4, 3, 5
    g = torch.Generator().manual_seed(21)
    m = TinyNet(3, 8, Kc, 21).double()
    x0 = 0.1 + 0.8 * torch.rand(B, 3, 8, 8, generator=g, dtype=torch.float64)
    x0[0, :, :2], x0[0, :, 2:4] = 0.0, 1.0
    with torch.no_grad():
        y = m(x0).argmax(1)
    _, _, trace = U.run(m, x0, y, n_iter, "Linf")
    x0f = x0.float()
    D = x0[0].numel()
    m32 = TinyNet(3, 8, Kc, 21).to(DEV)
    run = engine._FabURun(x0f.to(DEV), y.to(DEV), n_iter, 1.0, Kc)
    run.load(x0f.to(DEV), y.to(DEV))
    run.start(m32)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    n_adv = 0
    for i, e in enumerate(trace):
        xf = e["x_in"].float()
        zs, Js = zip(*(U.jacobian(m, e["x_in"][b:b + 1]) for b in range(B)))
        z32 = np.stack(zs).astype(np.float32)
        G = np.stack([[Js[b][k] - Js[b][int(y[b])] for b in range(B)] for k in range(Kc)]).astype(np.float32)
        best, best_k, df, w = _run_select(ops, G, z32, y.numpy(), "Linf", np.zeros((B, D), np.float32))
        assert best_k.tolist() == e["best_k"].tolist(), i
        for b in range(B):
            assert df[b] == np.float32(z32[b, best_k[b]] - z32[b, int(y[b])]) and _same_bits(w[b], G[best_k[b], b])
        # the loop's own hyperplane at the recorded point
        with torch.no_grad():
            run.x.detach().copy_(xf.to(DEV))
        wd, dfd = run.hyperplane(m32)
        assert run.best_k.cpu().tolist() == e["best_k"].tolist(), i
        bound = (D + Kc + 8) * 2.0 ** -23
        assert bool(((dfd.cpu().double() - e["df"]).abs() <= bound * (e["zt"].abs() + e["zy"].abs())).all()), i
        wmax = e["w"].flatten(1).abs().max(dim=1)[0].view(-1, 1)
        assert bool(((wd.cpu().flatten(1).double() - e["w"].flatten(1)).abs() <= bound * wmax).all()), i
        # projection, step and commit from the select launch's (w, df)
        wf, dff = torch.from_numpy(w).view(x0f.shape), torch.from_numpy(df)
        x2, o2, w2 = (a.flatten(1).numpy() for a in (xf, x0f, wf))
        lam64, sgn, lam32, on = _proj_reference(x2, o2, w2, dff.numpy())
        E = float(_rel_err(lam32, lam64).max())
        scal = ops.fab_proj_linf(xf.to(DEV), x0f.to(DEV), wf.to(DEV), dff.to(DEV)).cpu()
        lam = scal[0].numpy().astype(np.float64)
        tol = max(2 * E, 4 * 2.0 ** -23)
        assert (scal[1].numpy() == sgn).all() and on.all(), i
        assert (_rel_err(lam, lam64) <= tol).all(), (i, _rel_err(lam, lam64).max(), E)
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
        xs = e["x_step"].float()
        xd, advd, resd = xs.to(DEV), e["adv_in"].float().to(DEV), e["res_in"].float().to(DEV)
        pred = torch.zeros(B, dtype=torch.int32, device=DEV)
        flags = torch.zeros(B, dtype=torch.int32, device=DEV)
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


# ---- free-running: eager against graph -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_free_running_eager_equals_graph(ops, metric):
    """resnet18 with a head of 10 classes, 64 x 64, B = 3, eval mode, 3 iterations: eager and graph replay (one iteration per graph, three
    replays) give the same bits, a replay with new inputs equals a fresh eager run, the graphs of the three metrics have keys of their own,
    and the result triple is consistent.  Three L1 iterations meet no adversarial point on this untrained network (every norm is +inf,
    the triple is the clean batch), so the run state itself - iterate, chosen classes, w - is compared too, for all three metrics."""
    from eeadv import engine, models
    torch.manual_seed(5)
    m = models.make_resnet(18, "tiny", num_classes=10).to(DEV).eval()
    n_iter, eps = 3, {"Linf": 16 / 255, "L2": 2.0, "L1": 60.0}[metric]
    loop = (lambda x, y, graph: engine.fab_u_l1_loop(m, x, y, n_iter, eps, use_graph=graph)) if metric == "L1" else \
        (lambda x, y, graph: engine.fab_u_loop(m, x, y, n_iter, eps, use_graph=graph, norm=metric))
    dist = {"Linf": lambda v: v.abs().max(dim=1)[0], "L2": None, "L1": None}[metric]
    batches = []
    for seed in (1, 2):
        x = torch.rand(3, 3, 64, 64, generator=torch.Generator().manual_seed(seed)).to(DEV)
        with torch.no_grad():
            batches.append((x, m(x).argmax(1)))
    loop(*batches[0], True)  # builds the graph
    before = set(engine._GRAPHS)
    name = "fab_u_l1" if metric == "L1" else "fab_u"
    assert any(k[0] == name for k in before)
    # the run state itself, whether or not an adversarial point was met: the final iterate, the last chosen classes, the distances
    for x, y in batches:
        run = engine._FabUL1Run(x, y, n_iter, eps, 10) if metric == "L1" else engine._FabURun(x, y, n_iter, eps, 10, "auto", metric)
        run.load(x, y)
        run.start(m)
        run.body(m, n_iter, last=True)
        loop(x, y, True)
        replayed = next(v for k, v in engine._GRAPHS.items() if k[0] == name).run
        assert torch.equal(run.x.detach(), replayed.x.detach()) and torch.equal(run.best_k, replayed.best_k)
        assert torch.equal(run.res, replayed.res) and torch.equal(run.best, replayed.best) and torch.equal(run.w, replayed.w)
        assert int(run.counter.item()) == int(replayed.counter.item()) == n_iter
        assert bool((run.best_k >= 0).all()) and bool((run.best_k.long() != y).all()) and not torch.equal(run.x.detach(), x)
    eager = [loop(x, y, False) for x, y in batches]
    graph = [loop(x, y, True) for x, y in batches]
    assert set(engine._GRAPHS) == before  # the second batch replayed the first one's graph
    found = 0
    for (xe, re_, ne), (xg, rg, ng), (x, y) in zip(eager, graph, batches):
        assert torch.equal(xe, xg) and torch.equal(re_, rg) and torch.equal(ne, ng)
        assert bool((xe >= 0).all()) and bool((xe <= 1).all()) and torch.equal(re_, ~(ne <= eps)) and torch.equal(xe[re_], x[re_])
        if dist is not None:
            assert torch.equal(dist((xe - x).flatten(1))[~re_], ne[~re_])
        with torch.no_grad():
            assert bool((m(xe).argmax(1) != y)[~re_].all())
        found += int((~re_).sum())
        print("%s: non-robust %d of %d, norms %s" % (metric, int((~re_).sum()), len(y), ne.tolist()))
    assert (found > 0 and not torch.equal(eager[0][0], eager[1][0])) or metric == "L1"
    engine.clear_graphs()


# ---- the closed form on a linear classifier ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_linear_classifier_bound_on_the_device(ops, metric):
    """The case of tests/test_fab_u_host.py (the box never binds, checked there on the CPU): d* (1 - m) <= norm <= 1.05 d* (1 + m) with
    m = (D + K + 8) 2^-23, for L1 times the conditioning of df - and FAB_T, whose nine targets do not hold the closest class, reports more."""
    import utils.attacks as A
    from test_fab_u_host import closest_boundary, linear_case
    n_iter = 5
    m32, x0, y, W, c = linear_case(torch.float32)
    D, Kc = x0[0].numel(), 12
    dist, kstar, cond, _ = closest_boundary(x0, y, W, c, metric)
    assert bool((kstar == 11).all())
    args = Args(epsilon=2 * float(dist.max()))
    md, xd, yd = m32.to(DEV), x0.to(DEV), y.to(DEV)
    if metric == "L1":
        x_adv, robust, norm = A.FAB_L1(md, args, xd, yd, n_iter=n_iter)
        norm_t = A.FAB_T_L1(md, args, xd, yd, Kc, n_iter=n_iter)[2]
    else:
        x_adv, robust, norm = A.FAB(md, args, xd, yd, n_iter=n_iter, norm=metric)
        norm_t = A.FAB_T(md, args, xd, yd, Kc, n_iter=n_iter, norm=metric)[2]
    margin = (D + Kc + 8) * 2.0 ** -23 * (cond if metric == "L1" else 1.0)
    norm = norm.cpu().double()
    print("%s: norm / d* = %s" % (metric, (norm / dist).tolist()))
    assert bool((norm >= dist * (1 - margin)).all()) and bool((norm <= 1.05 * dist * (1 + margin)).all())
    assert not bool(robust.any())
    with torch.no_grad():
        assert bool((md(x_adv).argmax(1) != yd).all())
    assert bool((norm_t.cpu().double() > norm).all())


# ---- driver --------------------------------------------------------------------------------------------------------------------------
def test_mnist_driver_evaluates_with_untargeted_fab_from_a_graph(tmp_path):
    env = dict(os.environ, EEADV_GRAPH="1")
    r = subprocess.run([sys.executable, "experiments_mnist.py", "-c", "configs_mnist/adversarial_training.yml", "--data", "synthetic:1:1",
                        "--output-root", str(tmp_path), "-e", "--attack_method", "FAB-U", "--fab_iters", "2"],
                       cwd=os.path.join(PKG, "MNIST"), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    logs = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path)) for f in fs if f.startswith("log")]
    text = r.stdout + "".join(open(f).read() for f in logs)
    assert re.search(r"^ \* FAB-U: K = 10 classes, 10 backward passes per iteration, 2 iterations$", text, flags=re.M)
    clean = re.findall(r"^ \* Clean Prec@1 ([\d.]+)", text, flags=re.M)
    adv = re.findall(r"^ \* Adv Prec@1 ([\d.]+) Prec@5 ([\d.]+)$", text, flags=re.M)
    assert len(clean) >= 1 and len(clean) == len(adv)
    for c1, (a1, _) in zip(clean, adv):
        assert float(a1) <= float(c1)
