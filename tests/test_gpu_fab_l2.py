"""GPU: FAB-T in the L2 threat model - ee_fab_proj_l2_f32, ee_fab_step_l2_f32, ee_fab_commit_l2_f32 and engine.fab_loop(norm="L2") against
tests/fab_l2_reference.py.

Bit-exact: the paths and access widths of the projection against each other, the step and the commit given the kernel's own scalars, eager
against graph replay, the Linf route against itself.  In tolerance: mu and ||delta||_2 against the float64 reference on the same fp32
inputs - the kernel's worst relative error may not exceed that of a plain float32 restatement (numpy sort + sequential cumsum) on the same
cases; the commit's norm within 1 ulp of math.fsum."""
import functools
import math

import numpy as np
import pytest
import torch

import fab_l2_reference as R
import test_fab_l2_host as H
from tiny_models import Args, TinyNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
F32 = np.float32


@pytest.fixture(scope="module")
def ops():
    from eeadv import ops
    return ops


def _odd(t):
    """The same values at an address 4 bytes past a 16-byte boundary: the kernels then take their element-wise accesses."""
    pad = torch.zeros(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = pad[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _within_one_ulp(got, want64):
    """A float32 `got` against a float64 value: at most one float32 spacing (at the value) away."""
    return abs(float(got) - float(want64)) <= float(np.spacing(F32(abs(want64)))) or (math.isinf(want64) and float(got) == want64)


def _nan_equal(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


# ---- the projection ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cases(D, reps):
    """The inputs and, per problem, the float64 reference's (mu, s, norm), the float32 restatement's (mu, norm) and `on` - computed once."""
    x, x0, w, df, names = H.proj_cases(D, reps, 7 * D + reps, F32)
    probs = H.problems(x, x0, w, df)
    n = len(probs)
    ref = dict(mu=np.zeros(n), s=np.zeros(n), nrm=np.zeros(n), mu32=np.zeros(n), nrm32=np.zeros(n), on=np.zeros(n, dtype=bool),
               c=np.array([float(p[2]) for p in probs]))
    for q, (p, wq, c, on) in enumerate(probs):
        ref["on"][q] = on
        if not on:
            continue
        ref["mu"][q], ref["s"][q], ref["nrm"][q], _ = R.project(p.astype(np.float64), wq.astype(np.float64), float(c))
        if c != 0:
            ref["mu32"][q], ref["nrm32"][q] = R.project_f32(p, wq, c)
        else:
            ref["s"][q] = 1.0
    return x, x0, w, df, names, ref


def _rel_err(got, want):
    finite = np.isfinite(want) & (want != 0)
    err = np.zeros_like(want)
    with np.errstate(invalid="ignore"):
        err[finite] = np.abs(got[finite] - want[finite]) / np.abs(want[finite])
    return np.where(np.isnan(err), np.inf, err)


def _room_t(v, p):
    return torch.where(v > 0, p, torch.where(v < 0, 1 - p, torch.zeros_like(p))).clamp_min(0)


def _step_torch(x, x0, w, scal):
    """ee_fab_step_l2_f32 in torch float32 on the CPU, the kernel's operations in the kernel's order; also returns delta1, delta2 and the rooms."""
    B = x.shape[0]
    m1, m2, s1, s2, n1, n2 = (scal[0, :B], scal[0, B:], scal[1, :B], scal[1, B:], scal[2, :B], scal[2, B:])
    col = lambda v: v.view(-1, 1)

    def delta(v, p, mu):
        a = v.abs()
        return torch.where(a != 0, -torch.sign(v) * torch.minimum(col(mu) * a, _room_t(v, p)), torch.zeros_like(p))

    v1, v2 = col(s1) * w, col(s2) * w
    d1, d2 = delta(v1, x, m1), delta(v2, x0, m2)
    a1, a2 = n1.clamp_min(1e-8), n2.clamp_min(1e-8)
    alpha = col(torch.minimum(a1 / (a1 + a2), torch.tensor(0.1, dtype=torch.float32)))
    out = torch.clamp((x + 1.05 * d1) * (1 - alpha) + (x0 + 1.05 * d2) * alpha, 0, 1)
    return torch.where(col(s1) == 0, x, out), d1, d2, _room_t(v1, x), _room_t(v2, x0)


@pytest.mark.parametrize("D,reps", [(D, reps) for D in (1, 3, 5, 75, 1023, 192, 3 * 64 * 64) for reps in (1, 3)])
def test_projection_kernel(ops, D, reps):
    """Every branch on both paths and both access widths: the same bits.  mu and ||delta||_2 against the float64 reference on the same
    float32 inputs: the kernel's worst relative error over the cases may not exceed the worst of the float32 restatement, measured here.
    Infeasible and degenerate problems exactly."""
    x, x0, w, df, names, ref = _cases(D, reps)
    N = x.shape[0]
    dx, d0, dw, ddf = (torch.from_numpy(a).to(DEV) for a in (x, x0, w, df))
    first = ops.fab_proj_l2(dx, d0, dw, ddf, "resident").cpu()
    assert torch.equal(ops.fab_proj_l2(dx, d0, dw, ddf, "streaming").cpu(), first)  # one summation order on both paths: the same bits
    assert torch.equal(ops.fab_proj_l2(dx, d0, dw, ddf).cpu(), first)
    ox, o0, ow = _odd(dx), _odd(d0), _odd(dw)
    for path in ("resident", "streaming"):  # element-wise loads
        assert torch.equal(ops.fab_proj_l2(ox, o0, ow, ddf, path).cpu(), first), path
    scal = first
    assert not bool(torch.isnan(scal).any())
    mu, s, nrm = scal[0].numpy().astype(np.float64), scal[1].numpy(), scal[2].numpy().astype(np.float64)
    on = ref["on"]
    # exactly: samples without a hyperplane rest; c = 0 alone: mu = 0, s = +1; the signs; infeasible is +inf
    rest = [q for q in range(2 * N) if names[q % N] in H.NO_HYPERPLANE]
    assert not on[rest].any()
    assert (mu[~on] == 0).all() and (s[~on] == 0).all() and (nrm[~on] == 0).all()
    assert (s[on] == ref["s"][on]).all()
    zero_c = on & (ref["c"] == 0)
    assert (mu[zero_c] == 0).all() and (nrm[zero_c] == 0).all()
    assert (np.isinf(mu) == np.isinf(ref["mu"])).all() and (mu[np.isinf(mu)] > 0).all()
    assert all(mu[q] == INF for q in range(N) if names[q] == "infeasible" and on[q])
    assert all(s[q] == -1 for q in range(N) if names[q] == "c_negative" and on[q])
    for q in range(N):
        a = np.abs(w[q])
        if names[q] == "inactive" and on[q]:
            assert (mu[q] * a[a != 0] < H._room(F32(s[q]) * w[q], x[q])[a != 0]).all()
    # in tolerance: the yardstick is the float32 restatement on the same cases
    live = on & (ref["c"] != 0)
    e_mu, y_mu = _rel_err(mu, ref["mu"])[live], _rel_err(ref["mu32"], ref["mu"])[live]
    e_n, y_n = _rel_err(nrm, ref["nrm"])[live], _rel_err(ref["nrm32"], ref["nrm"])[live]
    if live.any():
        print("D = %d, %d problems: mu kernel %.3e restatement %.3e; norm kernel %.3e restatement %.3e"
              % (D, int(live.sum()), e_mu.max(), y_mu.max(), e_n.max(), y_n.max()))
        assert e_mu.max() <= y_mu.max(), (e_mu.max(), y_mu.max())
        assert e_n.max() <= y_n.max(), (e_n.max(), y_n.max())
    assert (nrm[live & (ref["nrm"] == 0)] == 0).all()
    # with the returned scalars: delta_i = -sign(s w_i) min(mu |w_i|, r_i), 0 where w_i = 0, inside the rooms; its length is the norm
    # returned up to the roundings of mu and of the products (2^-24 each) and of the norm itself
    tx, t0, tw = (torch.from_numpy(a) for a in (x, x0, w))
    want_x, d1, d2, r1, r2 = _step_torch(tx, t0, tw, scal)
    for d, r, nq in ((d1, r1, scal[2, :N]), (d2, r2, scal[2, N:])):
        d = torch.nan_to_num(d, nan=0.0)  # the w_nan sample: it has s = 0 and is not stepped
        assert bool((d[tw == 0] == 0).all()) and bool((d.abs() <= r).all())
        assert bool((d[~torch.from_numpy(on[:N])] == 0).all())
        dn = d.double().norm(dim=1)
        assert bool(((dn - nq.double()).abs() <= 4 * 2.0 ** -23 * dn).all())
    ops.fab_step_l2_(dx, d0, dw, scal.to(DEV))
    assert _nan_equal(dx.cpu(), want_x)


# ---- step and commit -----------------------------------------------------------------------------------------------------------------
def _state(B, P, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, P, generator=g)
    x = torch.clamp(x0 + (torch.rand(B, P, generator=g) - 0.5) * 0.2, 0, 1)
    x[:, ::5] = 0.0
    x[:, 3::5] = 1.0
    w = torch.randn(B, P, generator=g)
    special = torch.tensor([0.0, -0.0, float("nan"), 1e-30, -1e30, 1e-40])
    w.view(-1)[::4] = special[torch.arange(w.view(-1)[::4].numel()) % 6]
    return x, x0, w, g


@pytest.mark.parametrize("P,B", [(P, B) for P in (1, 3, 5, 75, 1023, 192) for B in (1, 3, 7)])
def test_step_kernel_bit_exact(ops, B, P):
    """Against the torch restatement given the scalars; rows with mu = inf (no inf * 0 where w_i = 0), with a norm below the 1e-8 floor,
    and a sample with s = 0, which keeps its x.  A NaN w_i gives a NaN there on both sides (min propagates it)."""
    x, x0, w, g = _state(B, P, 100 * B + P)
    for trial in range(3):
        mu = torch.rand(2 * B, generator=g) * (0.05, 0.5, 2.0)[trial]
        mu[trial % (2 * B)] = INF
        sgn = torch.where(torch.rand(2 * B, generator=g) < 0.5, -1.0, 1.0)
        nrm = torch.rand(2 * B, generator=g) * 3
        nrm[(trial + 1) % (2 * B)] = 0.0  # below the 1e-8 floor
        if B > 1:  # a sample without a hyperplane keeps its x
            mu[1], mu[B + 1], sgn[1], sgn[B + 1], nrm[1], nrm[B + 1] = 0, 0, 0, 0, 0, 0
        scal = torch.stack([mu, sgn, nrm])
        want = _step_torch(x, x0, w, scal)[0]
        xd = x.to(DEV)
        ops.fab_step_l2_(xd, x0.to(DEV), w.to(DEV), scal.to(DEV))
        got = xd.cpu()
        assert _nan_equal(got, want), (trial, B, P)
        assert bool(torch.isnan(got)[w == 0].logical_not().all())  # mu = inf met no zero
        ok = ~torch.isnan(got)
        assert bool((got[ok] >= 0).all()) and bool((got[ok] <= 1).all())
        if B > 1:
            assert torch.equal(got[1], x[1])
        od = _odd(x.to(DEV))  # element-wise accesses: the same bits
        ops.fab_step_l2_(od, _odd(x0.to(DEV)), _odd(w.to(DEV)), scal.to(DEV))
        assert _nan_equal(od.cpu(), want)


def _l2_f32(d):
    """The correctly rounded float32 of sqrt(sum d_i^2) for float32 differences d [P]."""
    return math.sqrt(math.fsum(float(v) * float(v) for v in d.tolist()))


@pytest.mark.parametrize("P,B", [(P, B) for P in (1, 3, 5, 75, 1023, 192) for B in (1, 3, 7)])
def test_commit_kernel(ops, B, P):
    """Per sample one of: adversarial and closer (adv, res take it), adversarial and exactly as far (equal is not closer), not adversarial,
    NaN logits (never adversarial), a label outside the row (never adversarial); `shift` moves the cases over the samples.  A first launch
    with res = inf shows the kernel's own norm: within 1 ulp of math.fsum, the same bits through element-wise accesses.  Everything else
    bit for bit."""
    K = 5
    x, x0, _, g = _state(B, P, 300 * B + P)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    want_nrm = [_l2_f32((x[b] - x0[b])) for b in range(B)]
    launches = 0
    for shift in range(5):
        y = torch.randint(0, K, (B,), generator=g)
        # the kernel's own norm: every row adversarial, res = inf
        zp = torch.zeros(B, K)
        zp[torch.arange(B), (y + 1) % K] = 1.0
        outs = []
        for view in (lambda t: t, _odd):
            xd, advd, resd = view(x.to(DEV)), view(torch.zeros(B, P, device=DEV)), torch.full((B,), INF, device=DEV)
            pred = torch.zeros(B, dtype=torch.int32, device=DEV)
            flags = torch.zeros(B, dtype=torch.int32, device=DEV)
            ops.fab_commit_l2_(zp.to(DEV), y.to(DEV), xd, view(x0.to(DEV)), advd, resd, pred, flags, counter)
            launches += 1
            assert flags.cpu().tolist() == [3] * B and torch.equal(advd.cpu(), x)
            assert torch.equal(xd.cpu(), x0 + 0.9 * (x - x0))
            outs.append(resd.cpu())
        assert torch.equal(outs[0], outs[1])  # vector and element-wise accesses: the same bits
        nrm = outs[0]
        assert all(_within_one_ulp(nrm[b], want_nrm[b]) for b in range(B)), (nrm.tolist(), want_nrm)
        # the cases
        z = torch.randn(B, K, generator=g)
        res = torch.full((B,), INF)
        case = [(b + shift) % 5 for b in range(B)]
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
            if c == 4:
                z[b, (y[b] + 1) % K] = z[b, y[b]] + 1
                y[b] = K + 2 if b % 2 else -1  # outside the row: never dereferenced, never adversarial
        adv0 = torch.rand(B, P, generator=g)
        xd, advd, resd = x.to(DEV), adv0.to(DEV), res.to(DEV)
        pred = torch.zeros(B, dtype=torch.int32, device=DEV)
        flags = torch.zeros(B, dtype=torch.int32, device=DEV)
        ops.fab_commit_l2_(z.to(DEV), y.to(DEV), xd, x0.to(DEV), advd, resd, pred, flags, counter)
        launches += 1
        want_flags = [{0: 3, 1: 1, 2: 0, 3: 0, 4: 0}[c] for c in case]
        assert flags.cpu().tolist() == want_flags, (shift, case)
        assert pred.cpu().tolist() == [R.first_class(z[b])[0] for b in range(B)]
        is_adv = torch.tensor([f & 1 for f in want_flags], dtype=torch.bool).view(-1, 1)
        improved = torch.tensor([f & 2 for f in want_flags], dtype=torch.bool)
        assert torch.equal(xd.cpu(), torch.where(is_adv, x0 + 0.9 * (x - x0), x))
        assert torch.equal(advd.cpu(), torch.where(improved.view(-1, 1), x, adv0))
        assert torch.equal(resd.cpu(), torch.where(improved, nrm, res))
        assert int(counter.item()) == launches


def test_kernels_take_empty_batches(ops):
    e = torch.empty(0, 12, device=DEV)
    assert ops.fab_proj_l2(e, e.clone(), e.clone(), torch.empty(0, device=DEV)).shape == (3, 0)
    ops.fab_step_l2_(e, e.clone(), e.clone(), torch.empty(3, 0, device=DEV))
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    i32 = torch.empty(0, dtype=torch.int32, device=DEV)
    ops.fab_commit_l2_(torch.empty(0, 5, device=DEV), torch.empty(0, dtype=torch.int64, device=DEV), e, e.clone(), e.clone(),
                       torch.empty(0, device=DEV), i32, i32.clone(), counter)
    torch.cuda.synchronize()
    assert int(counter.item()) == 0  # nothing was launched
    from eeadv import engine
    xa, robust, nrm = engine.fab_loop(TinyNet(3, 8, 10, 1).to(DEV).eval(), torch.empty(0, 3, 8, 8, device=DEV),
                                      torch.empty(0, dtype=torch.int64, device=DEV), torch.empty(0, dtype=torch.int64, device=DEV), 3, 0.5,
                                      norm="L2")
    assert xa.shape == (0, 3, 8, 8) and robust.shape == (0,) and nrm.shape == (0,)


# ---- the engine on a small conv net -------------------------------------------------------------------------------------------------------
def _tiny_problem():
    K = 10
    g = torch.Generator().manual_seed(21)
    m = TinyNet(3, 8, K, 21).eval()
    x0 = 0.1 + 0.8 * torch.rand(4, 3, 8, 8, generator=g)
    x0[0, :, :2], x0[0, :, 2:4] = 0.0, 1.0
    with torch.no_grad():
        order = torch.sort(m(x0), dim=1, descending=True, stable=True)[1]
    return m.to(DEV), x0.to(DEV), order[:, 0].contiguous().to(DEV), order[:, 1].contiguous().to(DEV)


def test_teacher_forced_trajectory():
    """B = 4, 3x8x8, 4 eager iterations of the engine with every launch recorded.  The reference is forced on the device's gradients (w,
    df) and on the scalars the projection launch emitted: its own mu (float64 on the same float32 inputs) lies within 1 ulp of the
    device's and so do its norms, the signs are equal; GIVEN the device's scalars the stepped point is the reference's float32 step bit for
    bit; the commit's pred and flags are the reference's, its norm within 1 ulp of math.fsum, adv / res / the shrunk x bit for bit."""
    from eeadv import engine
    n_iter = 4
    m, x0, y, t = _tiny_problem()
    run = engine._FabRun(x0, y, n_iter, 0.5, norm="L2")
    run.load(x0, y, t)
    run.start(m)
    recs = []
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
    for _ in range(n_iter):
        run.iteration(m)
    got = run.result()
    plain = engine.fab_loop(m, x0, y, t, n_iter, 0.5, use_graph=False, norm="L2")
    assert all(torch.equal(p, q) for p, q in zip(got, plain))  # the recorded run is the engine's run
    assert len(recs) == n_iter and int(run.counter.item()) == n_iter
    B = 4
    o = x0.cpu().flatten(1).numpy()
    yc = y.cpu().tolist()
    n_adv = n_imp = 0
    for i, e in enumerate(recs):
        e = {k: v.cpu() for k, v in e.items()}
        xin, wv, dfv = e["x_in"].flatten(1).numpy(), e["w"].flatten(1).numpy(), e["df"].numpy()
        assert np.array_equal(xin, o if i == 0 else recs[i - 1]["x_out"].cpu().flatten(1).numpy()), i
        scal = e["scal"].numpy()
        probs = H.problems(xin, o, wv, dfv)
        for q, (p, wq, c, on) in enumerate(probs):
            assert on, (i, q)
            mu64, s64, n64, _ = R.project(p.astype(np.float64), wq.astype(np.float64), float(c))
            assert scal[1, q] == s64 and _within_one_ulp(scal[0, q], mu64) and _within_one_ulp(scal[2, q], n64), (i, q, scal[:, q], mu64, n64)
        xs = e["x_step"].flatten(1).numpy()
        for b in range(B):
            want = R.step_f32(xin[b], o[b], wv[b], (scal[0, b], scal[1, b], scal[2, b], scal[0, B + b], scal[1, B + b], scal[2, B + b]))
            assert np.array_equal(xs[b], want), (i, b)
            pred, nan = R.first_class(e["z2"][b])
            is_adv = pred != yc[b] and not nan
            nrm = R.l2((xs[b] - o[b]).astype(np.float64))
            improved = is_adv and nrm < float(e["res_in"][b])
            assert int(e["pred"][b]) == pred and int(e["flags"][b]) == (1 if is_adv else 0) | (2 if improved else 0), (i, b)
            if improved:
                assert _within_one_ulp(e["res"][b], nrm) and np.array_equal(e["adv"][b].flatten().numpy(), xs[b]), (i, b)
            else:
                assert float(e["res"][b]) == float(e["res_in"][b]) and torch.equal(e["adv"][b], e["adv_in"][b]), (i, b)
            assert np.array_equal(e["x_out"][b].flatten().numpy(), R.shrink_f32(xs[b], o[b]) if is_adv else xs[b]), (i, b)
            n_adv += is_adv
            n_imp += improved
    assert n_adv > 0 and n_imp > 0


def test_linf_route_is_unchanged_and_the_two_norms_share_the_cache(ops, monkeypatch):
    """fab_loop(norm="Linf") is fab_loop(), bit for bit, eager and replayed, on one captured graph and without an L2 launch; the L2 run is
    one more graph; Linf, L2, Linf again: the third run has the bits of the first."""
    from eeadv import engine
    m, x0, y, t = _tiny_problem()
    n_iter, eps = 4, 0.5
    calls = []
    real = ops.fab_proj_l2
    monkeypatch.setattr(ops, "fab_proj_l2", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    engine.clear_graphs()
    try:
        for graph in (False, True):
            a = engine.fab_loop(m, x0, y, t, n_iter, eps, use_graph=graph)
            b = engine.fab_loop(m, x0, y, t, n_iter, eps, use_graph=graph, norm="Linf")
            assert all(torch.equal(p, q) for p, q in zip(a, b)) and not calls
        keys = [k for k in engine._GRAPHS if k[0] == "fab"]
        assert len(keys) == 1 and "Linf" in keys[0]
        c_eager = engine.fab_loop(m, x0, y, t, n_iter, eps, use_graph=False, norm="L2")
        c = engine.fab_loop(m, x0, y, t, n_iter, eps, use_graph=True, norm="L2")
        assert calls and all(torch.equal(p, q) for p, q in zip(c, c_eager))
        keys = [k for k in engine._GRAPHS if k[0] == "fab"]
        assert len(keys) == 2 and sorted(k[-1] for k in keys) == ["L2", "Linf"]
        assert not torch.equal(a[2], c[2]) and bool((c[2] >= a[2]).all())  # ||.||_2 >= ||.||_inf
        a2 = engine.fab_loop(m, x0, y, t, n_iter, eps, use_graph=True)
        c2 = engine.fab_loop(m, x0, y, t, n_iter, eps, use_graph=True, norm="L2")
        assert all(torch.equal(p, q) for p, q in zip(a, a2)) and all(torch.equal(p, q) for p, q in zip(c, c2))
        assert len([k for k in engine._GRAPHS if k[0] == "fab"]) == 2
        with pytest.raises(ValueError, match="norm"):
            engine.fab_loop(m, x0, y, t, n_iter, eps, norm="L1")
    finally:
        engine.clear_graphs()


def test_one_cached_graph_thresholds_with_each_callers_eps():
    """eps only thresholds FAB's result and is not in the cache key: the run cached by the first call answers later calls with THEIR eps."""
    from eeadv import engine
    m, x0, y, t = _tiny_problem()
    engine.clear_graphs()
    try:
        got = {}
        for eps in (1.0, 0.0, 1.0):  # inside the box no Linf distance exceeds 1; none but a clean miss is <= 0
            want = engine.fab_loop(m, x0, y, t, 4, eps, use_graph=False)
            got[eps] = engine.fab_loop(m, x0, y, t, 4, eps, use_graph=True)
            assert all(torch.equal(p, q) for p, q in zip(got[eps], want)), eps
        assert len([k for k in engine._GRAPHS if k[0] == "fab"]) == 1
        assert torch.equal(got[1.0][2], got[0.0][2]) and not torch.equal(got[1.0][1], got[0.0][1])  # the same search, other flags
    finally:
        engine.clear_graphs()


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
    y[0] = (y[0] + 1) % 200  # one sample starts misclassified
    return x, y


@pytest.mark.parametrize("ee", [False, True], ids=["resnet18", "resnet18_EE_square"])
def test_free_running_eager_equals_graph(ee, monkeypatch):
    """FAB-T in L2, one target, 64 x 64 (per-sample size 12288: the resident path), B = 4, eval mode, 4 iterations: eager and graph replay
    give the same bits, a second replay with new inputs equals a fresh eager run, and the results are valid.  The Add_Square draws of the
    edge-enhanced model are pinned by rewinding the device draw state before every run, as in tests/test_gpu_fab.py."""
    import utils.attacks as A
    from eeadv import engine, runtime
    m = _resnet(ee)
    eps, n_iter = 8.0, 4  # the radius only thresholds the result: four iterations on these untrained networks end 0.6 - 5 away
    args = Args(epsilon=eps)
    runtime.reseed()
    torch.manual_seed(9)
    state = runtime.draw_state(torch.device(DEV))
    batches = [_batch(m, 1), _batch(m, 2)]

    def attack(batch, graph):
        monkeypatch.setenv("EEADV_GRAPH", "1" if graph else "0")
        state.copy_(state0)
        return A.FAB_T(m, args, batch[0], batch[1], 200, n_iter=n_iter, n_target_classes=1, norm="L2")

    try:
        state0 = state.clone()
        attack(batches[0], True)  # builds the graph (the warm-up passes draw too)
        state0 = state.clone()
        eager = [attack(b, False) for b in batches]
        graph = [attack(b, True) for b in batches]
        found = 0
        for (xe, re_, ne), (xg, rg, ng), (x, y) in zip(eager, graph, batches):
            assert torch.equal(xe, xg) and torch.equal(re_, rg) and torch.equal(ne, ng)
            assert bool((xe >= 0).all()) and bool((xe <= 1).all())
            assert torch.equal(re_, ~(ne <= eps)) and float(ne[0]) == 0 and not bool(re_[0])
            dist = (xe - x).flatten(1).cpu()
            for b in range(len(y)):
                if not bool(re_[b]):
                    assert _within_one_ulp(ne[b].cpu(), _l2_f32(dist[b])), b
            assert torch.equal(xe[re_], x[re_])  # robust rows are the clean inputs
            if not ee:
                with torch.no_grad():
                    assert bool((m(xe).argmax(1) != y)[~re_].all())
            found += int((~re_[1:]).sum())
            print("non-robust %d of %d, norms %s" % (int((~re_).sum()), len(y), ne.tolist()))
        assert found > 0 and not torch.equal(eager[0][0], eager[1][0])
    finally:
        engine.clear_graphs()


def test_linear_classifier_bound_on_the_device():
    """One Linear(192, 2), the box never binds (tests/test_fab_l2_host.py): the first iteration starts at x0, projects onto the boundary at
    d = |df| / ||w||_2 and steps 1.05 of the way - the first adversarial point lies within [d, 1.05 d] of x0, and the final norm is at most
    that and at least d; margin m = (D + K + 8) * 2^-23."""
    import utils.attacks as A
    from eeadv import engine
    D, K = 192, 2
    m32, x0, y, t, _, dist = H.linear_case(torch.float32)
    eps = 2 * float(dist.max())
    margin = (D + K + 8) * 2.0 ** -23
    md, xd, yd, td = m32.to(DEV), x0.to(DEV), y.to(DEV), t.to(DEV)
    _, robust1, first = engine.fab_loop(md, xd, yd, td, 1, eps, use_graph=False, norm="L2")
    first = first.cpu().double()
    assert bool((first >= dist * (1 - margin)).all()) and bool((first <= 1.05 * dist * (1 + margin)).all()) and not bool(robust1.any())
    x_adv, robust, norm = A.FAB_T(md, Args(epsilon=eps), xd, yd, 2, n_iter=5, norm="L2")
    norm = norm.cpu().double()
    print("first / dist:", (first / dist).tolist(), "final / dist:", (norm / dist).tolist())
    assert bool((norm <= first).all()) and bool((norm >= dist * (1 - margin)).all()) and not bool(robust.any())
    with torch.no_grad():
        assert bool((md(x_adv).argmax(1) != yd).all())
