"""GPU: FAB-T in the L1 threat model - ee_fab_proj_l1_f32, ee_fab_step_l1_f32, ee_fab_commit_l1_f32 and engine.fab_l1_loop against
tests/fab_l1_reference.py.

Bit-exact: theta and the sign against the float64 reference on cases built with a margin, the paths and access widths of the projection
against each other, the step and the commit given the kernel's own scalars, eager against graph replay, the Linf and L2 routes against
themselves.  In tolerance: phi within one float rounding of the float64 value plus the conditioning of (c' - S) / P; ||delta||_1 no worse
than a plain float32 restatement (and 2^-24); the commit's norm within one rounding of math.fsum."""
import functools
import math

import numpy as np
import pytest
import torch

import fab_l1_reference as R
import test_fab_l1_host as H
from tiny_models import Args, TinyNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
F32 = np.float32
RESIDENT = 3 * 64 * 64


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


# ---- the projection ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cases(D):
    """The cases of three seeds with the float64 reference's answers (tests/test_fab_l1_host.py computes them once) and, per live problem,
    the float32 restatement's norm."""
    out = [c for seed in range(3) for c in H.cases(D, F32, seed)]
    for case in out:
        case["n32"] = [R.project_f32(p, w, c)[2] if case["on"] and float(c) != 0 else 0.0 for p, w, c in case["problems"]]
    return out


def _variants(D):
    paths = ("resident", "streaming", "auto") if D <= RESIDENT else ("streaming", "auto")
    return [(path, odd) for path in paths for odd in (False, True)]


@pytest.mark.parametrize("D", [1, 3, 5, 75, 192, 1023, 2049, 12288, 12289])
def test_projection_kernel(ops, D):
    """B = 2 per launch (4 problems), every case of three seeds.  All paths and access widths: the same bits.  theta, s, and phi on the
    exact cases equal the reference's; the infeasible, c = 0 and no-hyperplane answers exactly.  phi otherwise: (c' - S) / P in double,
    rounded to float once - relative 2^-24, plus the conditioning term (S + c') / P * D * 2^-52 of the two sums.  ||delta||_1 against the
    float64 reference on the same float32 inputs: its worst relative error may not exceed max(the float32 restatement's, 2^-24).  Then
    the step from the kernel's own scalars, bit for bit against the reference's float32 step."""
    cases = _cases(D)
    if D > RESIDENT:
        e = torch.zeros(2, D, device=DEV)
        with pytest.raises(Exception):
            ops.fab_proj_l1(e, e, e, torch.ones(2, device=DEV), "resident")
    err_n, err_n32, seen = 0.0, 0.0, set()
    for i in range(0, len(cases), 2):
        pair = [cases[i], cases[(i + 1) % len(cases)]]
        x, x0, w = (np.stack([c[k] for c in pair]) for k in ("x", "x0", "w"))
        df = np.array([c["df"] for c in pair], dtype=F32)
        dx, d0, dw, ddf = (torch.from_numpy(a).to(DEV) for a in (x, x0, w, df))
        ox, o0, ow = _odd(dx), _odd(d0), _odd(dw)
        first = None
        for path, odd in _variants(D):
            got = (ops.fab_proj_l1(ox, o0, ow, ddf, path) if odd else ops.fab_proj_l1(dx, d0, dw, ddf, path)).cpu()
            first = got if first is None else first
            assert torch.equal(got, first), (path, odd, pair[0]["name"], pair[1]["name"])
        scal = first.numpy()
        assert scal.shape == (4, 4) and not np.isnan(scal).any()
        for b, case in enumerate(pair):
            name = case["name"]
            for q, ((p, wq, c), ref) in enumerate(zip(case["problems"], case["ref"])):
                theta, s, n, phi = (scal[k, 2 * q + b] for k in range(4))
                c = float(c)
                if not case["on"]:
                    assert (theta, s, n, phi) == (0, 0, 0, 0), name
                    continue
                theta_r, phi_r, s_r, n_r, _ = ref
                if c == 0:
                    assert (theta, s, n, phi) == (INF, 1, 0, 0), name
                    seen.add("c_zero")
                    continue
                if name == "infeasible":
                    assert (theta, s, phi) == (0, s_r, 1) and abs(float(n) - n_r) <= 2.0 ** -24 * n_r, (name, n, n_r)
                    seen.add(name)
                    continue
                lo, hi, total = case["margin"][q]
                if case["f"] is None and min(lo, hi) <= (D + 8) * 2.0 ** -40 * total:
                    continue  # the undesigned problem of c_zero, should it ever sit on a boundary
                assert theta == F32(theta_r) and s == s_r, (name, D, q, theta, theta_r)
                if case["exact"]:
                    assert phi == 1.0, (name, D, q, phi)
                else:
                    tol = 2.0 ** -24 * phi_r + (2 * abs(c) - lo) / (lo + hi) * D * 2.0 ** -52
                    assert abs(float(phi) - phi_r) <= tol, (name, D, q, phi, phi_r, tol)
                err_n = max(err_n, abs(float(n) - n_r) / n_r)
                err_n32 = max(err_n32, abs(case["n32"][q] - n_r) / n_r)
                seen.add(name)
        # the step from these scalars
        sc = first.to(DEV)
        ops.fab_step_l1_(dx, d0, dw, sc)
        ops.fab_step_l1_(ox, o0, ow, sc)
        got = dx.cpu().numpy()
        assert np.array_equal(ox.cpu().numpy(), got)
        for b in range(2):
            want = R.step_f32(x[b], x0[b], w[b], tuple(scal[k, b] for k in range(4)) + tuple(scal[k, 2 + b] for k in range(4)))
            assert np.array_equal(got[b], want), (pair[b]["name"], D)
    print("D = %d: ||delta||_1 worst relative error: kernel %.3e, float32 restatement %.3e" % (D, err_n, err_n32))
    assert err_n <= max(err_n32, 2.0 ** -24), (err_n, err_n32)
    assert seen == set(R.CASES), set(R.CASES) - seen


@pytest.mark.parametrize("D", [5, 192, 2049, 12289])
def test_degenerate_rows_rest(ops, D):
    """df = 0, NaN, +-inf, w all zero, a NaN in w: no hyperplane - theta = 0, s = 0, n = 0, phi = 0 in both problems, and the step keeps x."""
    rng = np.random.default_rng(D)
    kinds = ("df_zero", "df_nan", "df_inf", "df_ninf", "w_zero", "w_nan", "fine")
    N = len(kinds)
    x, x0, w = rng.random((N, D)).astype(F32), rng.random((N, D)).astype(F32), rng.standard_normal((N, D)).astype(F32)
    df = np.full(N, 0.3, dtype=F32)
    df[0], df[1], df[2], df[3] = 0.0, np.nan, np.inf, -np.inf
    w[4] = 0
    w[5, D // 2] = np.nan
    dx, d0, dw, ddf = (torch.from_numpy(a).to(DEV) for a in (x, x0, w, df))
    first = None
    for path, odd in _variants(D):
        got = (ops.fab_proj_l1(_odd(dx), _odd(d0), _odd(dw), ddf, path) if odd else ops.fab_proj_l1(dx, d0, dw, ddf, path)).cpu()
        first = got if first is None else first
        assert torch.equal(got, first), (path, odd)
    scal = first.numpy()
    assert not scal[:, :6].any() and not scal[:, N:N + 6].any() and scal[1, 6] == 1 and scal[0, 6] > 0
    ops.fab_step_l1_(dx, d0, dw, first.to(DEV))
    got = dx.cpu().numpy()
    assert np.array_equal(got[:6], x[:6]) and not np.array_equal(got[6], x[6])


# ---- step and commit -----------------------------------------------------------------------------------------------------------------
def _state(B, P, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, P, generator=g)
    x = torch.clamp(x0 + (torch.rand(B, P, generator=g) - 0.5) * 0.2, 0, 1)
    x[:, ::5] = 0.0
    x[:, 3::5] = 1.0
    w = torch.randn(B, P, generator=g)
    special = torch.tensor([0.0, -0.0, float("nan"), 1e-30, -1e30, 1e-40, 0.75, -0.75])
    w.view(-1)[::3] = special[torch.arange(w.view(-1)[::3].numel()) % 8]
    return x, x0, w, g


@pytest.mark.parametrize("P,B", [(P, B) for P in (1, 3, 5, 75, 1023, 192) for B in (1, 3, 7)])
def test_step_kernel_bit_exact(ops, B, P):
    """Against the reference's float32 step given the scalars: theta at a tied |w_i| = 0.75 (the fraction applies), below every |w_i|,
    theta = 0 with phi = 1 (infeasible: w_i = 0 and NaN stay), theta = inf (nothing moves), a norm below the 1e-8 floor, and a sample with
    s = 0, which keeps its x.  No NaN comes out, whatever w holds."""
    x, x0, w, g = _state(B, P, 100 * B + P)
    for trial in range(3):
        theta = torch.full((2 * B,), 0.75)
        theta[trial % (2 * B)] = (0.0, INF, 1e-35)[trial]
        phi = torch.rand(2 * B, generator=g)
        phi[trial % (2 * B)] = (1.0, 0.0, 0.5)[trial]
        sgn = torch.where(torch.rand(2 * B, generator=g) < 0.5, -1.0, 1.0)
        nrm = torch.rand(2 * B, generator=g) * 30
        nrm[(trial + 1) % (2 * B)] = 0.0  # below the 1e-8 floor
        if B > 1:  # a sample without a hyperplane keeps its x
            for v in (theta, phi, sgn, nrm):
                v[1], v[B + 1] = 0, 0
        scal = torch.stack([theta, sgn, nrm, phi])
        sn = scal.numpy()
        want = np.stack([R.step_f32(x[b].numpy(), x0[b].numpy(), w[b].numpy(), tuple(sn[k, b] for k in range(4)) + tuple(sn[k, B + b] for k in range(4)))
                         for b in range(B)])
        xd = x.to(DEV)
        ops.fab_step_l1_(xd, x0.to(DEV), w.to(DEV), scal.to(DEV))
        got = xd.cpu().numpy()
        assert np.array_equal(got, want), (trial, B, P)
        assert not np.isnan(got).any() and got.min() >= 0 and got.max() <= 1
        if B > 1:
            assert np.array_equal(got[1], x[1].numpy())
        od = _odd(x.to(DEV))  # element-wise accesses: the same bits
        ops.fab_step_l1_(od, _odd(x0.to(DEV)), _odd(w.to(DEV)), scal.to(DEV))
        assert np.array_equal(od.cpu().numpy(), want)


def _l1_f32(d):
    return math.fsum(abs(float(v)) for v in d.tolist())


@pytest.mark.parametrize("P,B", [(P, B) for P in (1, 3, 5, 75, 1023, 192, 2049) for B in (1, 3, 7)])
def test_commit_kernel(ops, B, P):
    """Per sample one of: adversarial and closer (adv, res take it), adversarial and exactly as far (equal is not closer), not adversarial,
    NaN logits (never adversarial), a label outside the row (never adversarial); `shift` moves the cases over the samples.  A first launch
    with res = inf shows the kernel's own norm: (float) fsum |x - x0| within one rounding, the same bits through element-wise accesses.
    Everything else bit for bit."""
    K = 5
    x, x0, _, g = _state(B, P, 300 * B + P)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    want_nrm = [_l1_f32(x[b] - x0[b]) for b in range(B)]
    launches = 0
    for shift in range(5):
        y = torch.randint(0, K, (B,), generator=g)
        zp = torch.zeros(B, K)
        zp[torch.arange(B), (y + 1) % K] = 1.0
        outs = []
        for view in (lambda t: t, _odd):
            xd, advd, resd = view(x.to(DEV)), view(torch.zeros(B, P, device=DEV)), torch.full((B,), INF, device=DEV)
            pred = torch.zeros(B, dtype=torch.int32, device=DEV)
            flags = torch.zeros(B, dtype=torch.int32, device=DEV)
            ops.fab_commit_l1_(zp.to(DEV), y.to(DEV), xd, view(x0.to(DEV)), advd, resd, pred, flags, counter)
            launches += 1
            assert flags.cpu().tolist() == [3] * B and torch.equal(advd.cpu(), x)
            assert torch.equal(xd.cpu(), x0 + 0.9 * (x - x0))
            outs.append(resd.cpu())
        assert torch.equal(outs[0], outs[1])  # vector and element-wise accesses: the same bits
        nrm = outs[0]
        assert all(_within_one_ulp(nrm[b], want_nrm[b]) for b in range(B)), (nrm.tolist(), want_nrm)
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
        ops.fab_commit_l1_(z.to(DEV), y.to(DEV), xd, x0.to(DEV), advd, resd, pred, flags, counter)
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
    assert ops.fab_proj_l1(e, e.clone(), e.clone(), torch.empty(0, device=DEV)).shape == (4, 0)
    ops.fab_step_l1_(e, e.clone(), e.clone(), torch.empty(4, 0, device=DEV))
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    i32 = torch.empty(0, dtype=torch.int32, device=DEV)
    ops.fab_commit_l1_(torch.empty(0, 5, device=DEV), torch.empty(0, dtype=torch.int64, device=DEV), e, e.clone(), e.clone(),
                       torch.empty(0, device=DEV), i32, i32.clone(), counter)
    torch.cuda.synchronize()
    assert int(counter.item()) == 0  # nothing was launched
    from eeadv import engine
    xa, robust, nrm = engine.fab_l1_loop(TinyNet(3, 8, 10, 1).to(DEV).eval(), torch.empty(0, 3, 8, 8, device=DEV),
                                         torch.empty(0, dtype=torch.int64, device=DEV), torch.empty(0, dtype=torch.int64, device=DEV), 3, 0.5)
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


def _recorded_run(n_iter, eps=8.0):
    """n_iter eager iterations of the engine's L1 run with every launch recorded; also checks that the recorded run is the engine's."""
    from eeadv import engine
    m, x0, y, t = _tiny_problem()
    run = engine._FabL1Run(x0, y, n_iter, eps)
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
    plain = engine.fab_l1_loop(m, x0, y, t, n_iter, eps, use_graph=False)
    assert all(torch.equal(p, q) for p, q in zip(got, plain))
    assert len(recs) == n_iter and int(run.counter.item()) == n_iter and tuple(run.scal.shape) == (4, 8)
    return m, x0, y, t, [{k: v.cpu() for k, v in e.items()} for e in recs]


def test_teacher_forced_trajectory():
    """B = 4, 3x8x8, 4 eager iterations.  Given the device's gradients (w, df), theta and the sign of every projection equal the float64
    reference's, ||delta||_1 lies within 1 ulp and phi within its bound; GIVEN the device's scalars the stepped point is the reference's
    float32 step bit for bit; the commit's pred and flags are the reference's, its norm within one rounding of math.fsum, adv / res / the
    shrunk x bit for bit."""
    n_iter, B = 4, 4
    m, x0, y, t, recs = _recorded_run(n_iter)
    o = x0.cpu().flatten(1).numpy()
    yc = y.cpu().tolist()
    n_adv = n_imp = 0
    for i, e in enumerate(recs):
        xin, wv, dfv = e["x_in"].flatten(1).numpy(), e["w"].flatten(1).numpy(), e["df"].numpy()
        assert np.array_equal(xin, o if i == 0 else recs[i - 1]["x_out"].flatten(1).numpy()), i
        scal = e["scal"].numpy()
        for b in range(B):
            probs = R.problems(dict(x=xin[b], x0=o[b], w=wv[b], df=dfv[b]))
            for k, (p, wq, c) in enumerate(probs):
                q = k * B + b
                th, ph, s64, n64, _ = R.project(p, wq, float(c))
                lo, hi, _ = R.fill_margin(p, wq, float(c))
                assert scal[1, q] == s64 and scal[0, q] == F32(th), (i, q, scal[:, q], th)
                assert _within_one_ulp(scal[2, q], n64), (i, q, scal[2, q], n64)
                assert abs(float(scal[3, q]) - ph) <= 2.0 ** -24 * ph + (2 * abs(float(c)) - lo) / (lo + hi) * 192 * 2.0 ** -52, (i, q)
        xs = e["x_step"].flatten(1).numpy()
        for b in range(B):
            want = R.step_f32(xin[b], o[b], wv[b], tuple(scal[k, b] for k in range(4)) + tuple(scal[k, B + b] for k in range(4)))
            assert np.array_equal(xs[b], want), (i, b)
            pred, nan = R.first_class(e["z2"][b])
            is_adv = pred != yc[b] and not nan
            nrm = R.l1(xs[b] - o[b])
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


def test_engine_against_the_host_path_teacher_forced():
    """Every host iteration (float32, on the CPU) starts from the state the device recorded.  pred, the flags and the signs are equal.  The
    two gradients come from different convolutions: each |w_i| - theta is one of them - carries bound = (D + K + 8) 2^-24 of the largest;
    c' carries dc = bound (|df| + sum |w_i (x0_i - x_i)|) plus the forward's bound on the logits, what is left of c' is filled at theta, so
    ||delta||_1 moves by dc / theta, and the points by 1.05 of that."""
    import utils.attacks as A
    n_iter, B, D, K = 4, 4, 192, 10
    m, x0, y, t, recs = _recorded_run(n_iter)
    mc, oc, yc, tc = TinyNet(3, 8, K, 21).eval(), x0.cpu(), y.cpu(), t.cpu()  # the same seeded weights on the CPU
    bound = (D + K + 8) * 2.0 ** -24
    for i, e in enumerate(recs):
        with torch.no_grad():
            zmax = mc(e["x_in"]).abs().max(dim=1)[0]
        x, adv, res, info = A._fab_l1_host_iteration(mc, e["x_in"], oc, yc, tc, e["adv_in"], e["res_in"])
        flags = info["is_adv"].int() + 2 * info["improved"].int()
        assert info["pred"].tolist() == e["pred"].tolist() and flags.tolist() == e["flags"].tolist(), i
        scal = e["scal"]
        assert torch.equal(info["s1"], scal[1, :B]) and torch.equal(info["s2"], scal[1, B:]), i
        wr = e["w"].flatten(1)
        wmax = wr.abs().max(dim=1)[0]
        dc = bound * (2 * zmax + (wr * (oc - e["x_in"]).flatten(1)).abs().sum(dim=1) + wmax * D)
        for k, lam, nn in ((0, "lam1", "n1"), (1, "lam2", "n2")):
            th, nd = scal[0, k * B:(k + 1) * B], scal[2, k * B:(k + 1) * B]
            assert bool(((info[lam] - th).abs() <= bound * wmax).all()), (i, lam)
            assert bool(((info[nn] - nd).abs() <= dc / th + bound * nd).all()), (i, nn, info[nn], nd)
    # and the free-running results agree on who is robust at a radius no norm is close to
    from eeadv import engine
    eps = 8.0
    got = engine.fab_l1_loop(m, x0, y, t, n_iter, eps, use_graph=False)
    adv, res = A._fab_l1_host(mc, oc, yc, tc, n_iter)
    assert torch.equal(got[1].cpu(), ~(res <= eps))


def test_eager_graph_paths_and_the_three_norms_share_the_cache():
    """fab_l1_loop: eager and replayed runs give the same bits, and so do the resident and the streaming path.  A Linf, an L2 and an L1
    graph of one shape coexist; after the L1 runs the Linf and L2 results are the bits they were before them."""
    from eeadv import engine
    m, x0, y, t = _tiny_problem()
    n_iter, eps = 4, 8.0
    engine.clear_graphs()
    try:
        linf = engine.fab_loop(m, x0, y, t, n_iter, 0.5, use_graph=True)
        l2 = engine.fab_loop(m, x0, y, t, n_iter, 0.5, use_graph=True, norm="L2")
        eager = engine.fab_l1_loop(m, x0, y, t, n_iter, eps, use_graph=False)
        graph = engine.fab_l1_loop(m, x0, y, t, n_iter, eps, use_graph=True)
        assert all(torch.equal(p, q) for p, q in zip(eager, graph))
        for path in ("resident", "streaming"):
            for use_graph in (False, True):
                other = engine.fab_l1_loop(m, x0, y, t, n_iter, eps, use_graph=use_graph, path=path)
                assert all(torch.equal(p, q) for p, q in zip(eager, other)), (path, use_graph)
        again = engine.fab_l1_loop(m, x0, y, t, n_iter, eps, use_graph=True)
        assert all(torch.equal(p, q) for p, q in zip(eager, again))
        assert sorted(k[-1] for k in engine._GRAPHS if k[0] == "fab") == ["L2", "Linf"]
        assert len([k for k in engine._GRAPHS if k[0] == "fab_l1"]) == 3  # auto, resident, streaming
        linf2 = engine.fab_loop(m, x0, y, t, n_iter, 0.5, use_graph=True)
        l22 = engine.fab_loop(m, x0, y, t, n_iter, 0.5, use_graph=True, norm="L2")
        assert all(torch.equal(p, q) for p, q in zip(linf, linf2)) and all(torch.equal(p, q) for p, q in zip(l2, l22))
        assert len(engine._GRAPHS) == 5
        found = torch.isfinite(eager[2]) & torch.isfinite(l2[2])
        assert bool(found.any()) and bool((eager[2][found] >= l2[2][found] * (1 - 2.0 ** -20)).all())  # ||.||_1 >= ||.||_2 of the closest points
        with pytest.raises(ValueError, match="norm"):
            engine.fab_loop(m, x0, y, t, n_iter, eps, norm="L1")
    finally:
        engine.clear_graphs()


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def test_linear_classifier_bound_on_the_device():
    """One Linear(192, 2), the box never binds (tests/test_fab_l1_host.py): the first iteration starts at x0, projects onto the boundary at
    d = |df| / ||w||_inf along one coordinate and steps 1.05 of the way - the first adversarial point lies within [d, 1.05 d] of x0 in L1,
    and the final norm is at most that and at least d; margin m = (D + K + 8) * 2^-23 * cond, cond the conditioning of df as a difference
    of two float32 logits (linear_case).  FAB_T_L1 on device tensors agrees with the CPU door
    on `robust` at a radius between the samples' distances."""
    import utils.attacks as A
    from eeadv import engine, runtime
    D, K = 192, 2
    m32, x0, y, t, _, dist, cond = H.linear_case(torch.float32)
    eps = 2 * float(dist.max())
    margin = (D + K + 8) * 2.0 ** -23 * cond
    md, xd, yd, td = m32.to(DEV), x0.to(DEV), y.to(DEV), t.to(DEV)
    _, robust1, first = engine.fab_l1_loop(md, xd, yd, td, 1, eps, use_graph=False)
    first = first.cpu().double()
    print("first / dist:", (first / dist).tolist())
    assert bool((first >= dist * (1 - margin)).all()) and bool((first <= 1.05 * dist * (1 + margin)).all()) and not bool(robust1.any())
    x_adv, robust, norm = A.FAB_T_L1(md, Args(epsilon=eps), xd, yd, 2, n_iter=5)
    norm = norm.cpu().double()
    assert bool((norm <= first).all()) and bool((norm >= dist * (1 - margin)).all()) and not bool(robust.any())
    with torch.no_grad():
        assert bool((md(x_adv).argmax(1) != yd).all())
    mid = float(dist.sort()[0][2:4].mean()) * 1.03  # between two samples' distances, a few percent from either
    assert float(((1.05 * dist - mid).abs() / mid).min()) > 0.005 and float(((dist - mid).abs() / mid).min()) > 0.005
    dev = A.FAB_T_L1(md, Args(epsilon=mid), xd, yd, 2, n_iter=5)
    runtime.allow_cpu_plumbing(True)
    try:
        cpu = A.FAB_T_L1(m32.cpu(), Args(epsilon=mid), x0, y, 2, n_iter=5)
    finally:
        runtime.allow_cpu_plumbing(False)
    assert torch.equal(dev[1].cpu(), cpu[1]) and bool(cpu[1].any()) and not bool(cpu[1].all())
