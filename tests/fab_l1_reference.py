"""An independent float64 restatement of FAB-T in the L1 threat model (Croce & Hein 2020; targeted, eta = 1.05, beta = 0.9, alpha_max = 0.1,
one run from the clean point) for the tests: numpy, math.fsum and torch autograd only, one sample at a time.  Nothing
here is shared with utils/attacks.py, eeadv/engine.py or the other reference files.

    rooms(p, w, s)                    (|v_i|, r_i) of v = s w at the point p
    project(p, w, c)                  the least-L1 projection by explicit stable sort and a walk over the groups of equal |w_i| ->
                                      (theta, phi, s, n, delta); every coordinate of the group the fill ends in takes the fraction phi
    fill_margin(p, w, c)              (c' - S, S + P - c', total): how far c' is from the two neighbouring answers
    project_f32(p, w, c)              the same walk in float32 (numpy sort + sequential cumsum) -> (theta, phi, n): the yardstick
    l1(v)                             fsum(|v_i|)
    step_f32(x, x0, w, scal8)         the step in float32, one rounding per operation, from given projection scalars
    shrink_f32(x, x0)                 x0 + 0.9 (x - x0) in float32
    iterate(model, x, x0, y, t, adv, res, w=None)   one iteration of one sample -> dict (w: a gradient to use instead of autograd's)
    run(model, x0, y, t, n_iter)      the whole run over a batch -> (adv, res, trace)
    proj_cases(D, dtype, rng)         the projection cases, each with a margin around its answer
    problems(case)                    the two projection problems (p, w, c) of a case as every implementation forms them
"""
import math

import numpy as np
import torch

ETA, BETA, ALPHA_MAX = 1.05, 0.9, 0.1


def rooms(p, w, s):
    """(a, r) as float64 arrays.  The room 1 - p_i is a quantity of the inputs' dtype - rounded once there, as every implementation forms
    it - and only then widened."""
    dt = np.asarray(p).dtype.type
    v = dt(s) * np.asarray(w)
    one, zero = dt(1), dt(0)
    r = np.maximum(np.where(v > 0, p, np.where(v < 0, one - p, zero)), zero).astype(dt)
    return np.abs(v).astype(np.float64), r.astype(np.float64)


def l1(v):
    return math.fsum(abs(float(e)) for e in np.asarray(v).reshape(-1))


_GROUPS = {}  # the groups of the last few |w|: a case is walked several times (its builder, project, fill_margin)


def _groups(a, r):
    """The coordinates with a_i != 0 in groups of equal a, by a descending (an explicit stable sort): [(a, [indices])]."""
    key = a.tobytes()
    if key not in _GROUPS:
        if len(_GROUPS) >= 4:
            _GROUPS.clear()
        _GROUPS[key] = _build_groups(a)
    return _GROUPS[key]


def _build_groups(a):
    idx = np.argsort(-a, kind="stable")
    idx = idx[a[idx] != 0]
    av = a[idx]
    bounds = [0] + (np.flatnonzero(av[1:] != av[:-1]) + 1).tolist() + [idx.size]
    il, al = idx.tolist(), av.tolist()
    return [(al[lo], il[lo:hi]) for lo, hi in zip(bounds[:-1], bounds[1:]) if hi > lo]


def _walk(a, r, cp):
    """(theta, phi, S, P, total) of the fill: theta = the largest a with sum_{a_i >= a} a_i r_i >= c', exactly summed; (0, 1, ...) when
    c' exceeds the whole sum."""
    groups = _groups(a, r)
    pr = a * r  # float64 products, each rounded once at most (exact for float32 inputs)
    flat = pr[[i for _, g in groups for i in g]].tolist()  # the products in the order of the walk, cut into the groups
    ends = np.cumsum([len(g) for _, g in groups]).tolist()
    prods = [flat[lo:hi] for lo, hi in zip([0] + ends[:-1], ends)]
    total = math.fsum(flat)
    above, rough = [], 0.0  # rough: a plain running sum (off by D 2^-53 of itself at most) that says when the exact test is worth taking
    for (ag, _), pg in zip(groups, prods):
        P = math.fsum(pg)
        if rough + P >= cp * (1 - 1e-9) and math.fsum(above + pg) >= cp:
            S = math.fsum(above)
            phi = min(max((cp - S) / P, 0.0), 1.0) if P > 0 else 0.0
            return ag, phi, S, P, total
        above += pg
        rough += P
    return 0.0, 1.0, total, 0.0, total


def project(p, w, c):
    """p, w [D] in the dtype of the inputs (the rooms are formed there), c float; everything else in float64.  Returns (theta, phi, s, n,
    delta): delta_i = -sign(s w_i) m_i, m_i = r_i where a_i > theta, phi r_i where a_i == theta, 0 below and where w_i == 0; n = ||delta||_1."""
    p, w = np.asarray(p), np.asarray(w)
    s = 1.0 if c >= 0 else -1.0
    a, r = rooms(p, w, s)
    cp = abs(float(c))
    if cp == 0:
        return math.inf, 0.0, s, 0.0, np.zeros(p.shape)
    theta, phi, _, _, _ = _walk(a, r, cp)
    up, at = (a > theta) & (a != 0), (a == theta) & (a != 0)
    m = np.where(up, r, np.where(at, phi * r, 0.0))
    n = math.fsum(r[up].tolist()) + phi * math.fsum(r[at].tolist())
    return theta, phi, s, n, -np.sign(s * w.astype(np.float64)) * m


def fill_margin(p, w, c):
    """(c' - S, S + P - c', total) of a feasible problem with c != 0: the distance of c' to the answer `one group earlier` and to `one
    group later`, and the size of the sums an implementation adds up."""
    a, r = rooms(p, w, 1.0 if c >= 0 else -1.0)
    _, _, S, P, total = _walk(a, r, abs(float(c)))
    return abs(float(c)) - S, S + P - abs(float(c)), total


def project_f32(p, w, c):
    """The fill in float32 on float32 inputs (c already rounded to float32), every operation rounded to float32: numpy sort, sequential
    cumulative sums.  Returns (theta, phi, n) as floats."""
    f = np.float32
    p, w = np.asarray(p, dtype=f), np.asarray(w, dtype=f)
    s = f(1.0 if c >= 0 else -1.0)
    v = s * w
    a = np.abs(v)
    r = np.maximum(np.where(v > 0, p, np.where(v < 0, f(1) - p, f(0))), f(0)).astype(f)
    cp = abs(f(c))
    keep = a != 0
    a, r = a[keep], r[keep]
    if a.size == 0:
        return 0.0, 1.0, 0.0
    order = np.argsort(-a, kind="stable")
    a, r = a[order], r[order]
    cum = np.cumsum((a * r).astype(f), dtype=f)
    if cp > cum[-1]:
        return 0.0, 1.0, float(np.cumsum(r, dtype=f)[-1])
    k = int(np.argmax(cum >= cp))
    theta = a[k]
    up, at = a > theta, a == theta
    S = np.cumsum((a[up] * r[up]).astype(f), dtype=f)[-1] if up.any() else f(0)
    P = np.cumsum((a[at] * r[at]).astype(f), dtype=f)[-1]
    phi = f(min(max(f(f(cp - S) / P), f(0)), f(1))) if P > 0 else f(0)
    N = np.cumsum(r[up], dtype=f)[-1] if up.any() else f(0)
    R = np.cumsum(r[at], dtype=f)[-1]
    return float(theta), float(phi), float(f(N + f(phi * R)))


def step_f32(x, x0, w, scal):
    """The step of one sample in float32 arithmetic, every operation rounded once, from scal = (theta1, s1, n1, phi1, theta2, s2, n2, phi2)
    as given (the scalars of the code under test): x, x0, w float32 [D] -> the stepped point, float32 [D]."""
    f = np.float32
    th1, s1, n1, ph1, th2, s2, n2, ph2 = (f(v) for v in scal)
    if s1 == 0:
        return x.copy()

    def delta(p, s, theta, phi):
        v = s * w
        a = np.abs(v)
        r = np.maximum(np.where(v > 0, p, np.where(v < 0, f(1) - p, f(0))), f(0))
        with np.errstate(invalid="ignore"):
            m = np.where(a > theta, r, np.where((a == theta) & (a != 0), phi * r, f(0)))
        return (-np.sign(np.nan_to_num(v, nan=0.0)) * m).astype(f)

    a1, a2 = max(n1, f(1e-8)), max(n2, f(1e-8))
    alpha = min(f(a1 / f(a1 + a2)), f(ALPHA_MAX))
    d1, d2 = delta(x, s1, th1, ph1), delta(x0, s2, th2, ph2)
    out = (x + f(ETA) * d1) * f(f(1) - alpha) + (x0 + f(ETA) * d2) * alpha
    assert out.dtype == f
    return np.clip(out, f(0), f(1))


def shrink_f32(x, x0):
    f = np.float32
    out = x0 + f(BETA) * (x - x0)
    assert out.dtype == f
    return out


def first_class(z_row):
    """The first class by value descending, ties to the lower index, NaN above everything; and whether the row holds a NaN."""
    vals = [float(v) for v in z_row]
    nan = any(v != v for v in vals)
    best = 0
    for c in range(1, len(vals)):
        bv, cv = vals[best], vals[c]
        if bv != bv:
            continue
        if cv != cv or cv > bv:
            best = c
    return best, nan


def iterate(model, x, x0, y, t, adv, res, w=None):
    """One iteration of one sample: x, x0, adv float64 tensors [1, ...]; y, t ints; res float.  Returns a dict with every intermediate.
    `w` (a tensor shaped like x) replaces the gradient of autograd - a teacher-forced run hands in the gradient of the code under test."""
    shape = x0.shape
    xc = x.detach().clone().requires_grad_()
    z = model(xc)
    diff = z[0, t] - z[0, y]
    if w is None:
        (w,) = torch.autograd.grad(diff, [xc])
    df = float(diff.detach())
    w_np, x_np, x0_np = w.detach().reshape(-1).numpy().copy(), x.detach().reshape(-1).numpy().copy(), x0.reshape(-1).numpy().copy()
    sabs = float(np.sum(np.abs(w_np)))
    enabled = bool(np.isfinite(df) and df != 0 and np.isfinite(sabs) and sabs > 0)
    out = dict(df=df, zt=float(z[0, t].detach()), zy=float(z[0, y].detach()), w=w.detach().clone(), enabled=enabled)
    if enabled:
        c2 = df + math.fsum(w_np * (x0_np - x_np))
        th1, ph1, s1, n1, d1 = project(x_np, w_np, df)
        th2, ph2, s2, n2, d2 = project(x0_np, w_np, c2)
        a1, a2 = max(n1, 1e-8), max(n2, 1e-8)
        alpha = min(a1 / (a1 + a2), ALPHA_MAX)
        x_step = np.clip((x_np + ETA * d1) * (1 - alpha) + (x0_np + ETA * d2) * alpha, 0.0, 1.0)
    else:
        th1 = ph1 = s1 = n1 = th2 = ph2 = s2 = n2 = alpha = c2 = 0.0
        x_step = x_np.copy()
    x_step_t = torch.from_numpy(x_step).view(shape)
    with torch.no_grad():
        z2 = model(x_step_t)
    pred, nan = first_class(z2[0])
    out["z2"] = z2.detach().clone()
    is_adv = (pred != y) and not nan
    nrm = l1(x_step - x0_np)
    improved = is_adv and nrm < res
    if improved:
        adv, res = x_step_t.clone(), nrm
    x_new = torch.from_numpy(x0_np + BETA * (x_step - x0_np)).view(shape) if is_adv else x_step_t
    out.update(c2=c2, lam1=th1, phi1=ph1, s1=s1, n1=n1, lam2=th2, phi2=ph2, s2=s2, n2=n2, alpha=alpha, x_step=x_step_t, pred=pred,
               is_adv=is_adv, improved=improved, nrm=nrm, x=x_new, adv=adv, res=res)
    return out


def run(model, x0, y, t, n_iter):
    """The whole run, sample by sample.  Returns (adv [B,...], res [B], trace): trace[i] holds, per key, the batch-stacked values of
    iteration i, and 'x_in' / 'adv_in' / 'res_in', the state the iteration started from."""
    B = x0.shape[0]
    xs = [x0[b:b + 1].clone() for b in range(B)]
    advs = [x0[b:b + 1].clone() for b in range(B)]
    ress = [math.inf] * B
    trace = []
    for _ in range(n_iter):
        rows = []
        for b in range(B):
            r = iterate(model, xs[b], x0[b:b + 1], int(y[b]), int(t[b]), advs[b], ress[b])
            r.update(x_in=xs[b], adv_in=advs[b], res_in=ress[b])
            xs[b], advs[b], ress[b] = r["x"], r["adv"], r["res"]
            rows.append(r)
        entry = {}
        for k in rows[0]:
            vals = [r[k] for r in rows]
            if isinstance(vals[0], torch.Tensor):
                entry[k] = torch.cat(vals)
            else:
                entry[k] = torch.tensor(vals, dtype=torch.float64 if isinstance(vals[0], float) else None)
        trace.append(entry)
    return torch.cat(advs), torch.tensor(ress, dtype=torch.float64), trace


# ---- the projection cases -------------------------------------------------------------------------------------------------------------
CASES = ("generic", "c_negative", "half_tied", "all_tied", "w_tiny", "ends", "w_third_zero", "c_zero", "infeasible", "k_first", "k_last",
         "exact_f0", "exact_f1")
TINY = {np.float32: 1e-40, np.float64: 1e-310}  # denormal in the dtype
FRACTIONS = (0.25, 0.5, 0.75)


def problems(case):
    """The two projection problems (p, w, c) of a case: p = x with c = df, and p = x0 with c = df + sum w (x0 - x), the sum taken exactly
    and c rounded to the dtype of the inputs once."""
    x, x0, w, df = case["x"], case["x0"], case["w"], case["df"]
    dot = math.fsum((w.astype(np.float64) * (x0 - x).astype(np.float64)).tolist())
    return [(x, w, df), (x0, w, df.dtype.type(float(df) + dot))]


def proj_cases(D, dtype, rng):
    """One case per name of CASES: dict(name, x, x0, w, df, f, exact, theta, phi) in `dtype` (theta, phi: the designed answer, where f is
    not None).  x0 = x (so both problems of the sample are the designed
    one) except in `c_zero`.  The designed problem fills down to a chosen group k of equal |w_i| and takes the fraction f of it: c' = S + f P
    in float64, rounded to the dtype - the distance to either neighbouring theta is min(f, 1 - f) P, and the builder asserts that at least
    0.2 P of it is left after the rounding of c'.  `exact` cases (f = 0 and f = 1) are dyadic: every sum is exact in every dtype.
      generic       Gaussian w, the fill ends in the middle            c_negative    the same with c < 0
      half_tied     every second |w_i| = 0.75, the fill ends there     all_tied      every |w_i| = 0.75
      w_tiny        every third |w_i| denormal (from index 1)          ends          p at exactly 0 and 1 on half of the coordinates, some
      w_third_zero  every third w_i = 0 (from index 1)                               of them in the tied set the fill ends in
      c_zero        df = -<w, x0 - x> exactly: problem 2 has c = 0     infeasible    c' above the whole sum
      k_first       the fill ends in the largest |w_i|                 k_last        ... in the smallest (|w_i| >= 0.5 there)
      exact_f0      c' = S exactly: the larger a with phi = 1          exact_f1      c' = S + P exactly: phi = 1"""
    f = dtype
    out = []
    for ci, name in enumerate(CASES):
        frac = FRACTIONS[(ci + int(rng.integers(3))) % 3]
        sign = -1.0 if name == "c_negative" else 1.0
        exact = name in ("exact_f0", "exact_f1")
        if exact:
            w = (rng.integers(1, 129, D) * rng.choice([-1, 1], D) / 64.0).astype(f)
            x = (rng.integers(0, 65, D) / 64.0).astype(f)
        else:
            w = rng.standard_normal(D).astype(f)
            x = (0.05 + 0.9 * rng.random(D)).astype(f)
        if name in ("half_tied", "ends"):
            w[::2] = np.where(rng.random(w[::2].size) < 0.5, -0.75, 0.75).astype(f)
        if name == "all_tied":
            w[:] = np.where(rng.random(D) < 0.5, -0.75, 0.75).astype(f)
        if name == "w_tiny":
            w[1::3] = np.where(rng.random(w[1::3].size) < 0.5, -TINY[f], TINY[f]).astype(f)
        if name == "w_third_zero":
            w[1::3] = 0
        if name == "k_last":
            w = (np.where(rng.random(D) < 0.5, -1.0, 1.0) * (0.5 + rng.random(D))).astype(f)
        if name == "ends":  # what a clamped iterate looks like: rooms of exactly 0 and 1, also inside the tied set
            x[::4] = np.where(rng.random(x[::4].size) < 0.5, 0.0, 1.0).astype(f)
            x[1::4] = np.where(rng.random(x[1::4].size) < 0.5, 0.0, 1.0).astype(f)
        a = np.abs(w).astype(np.float64)
        groups = _groups(a, None)
        # the group the fill ends in
        if name in ("half_tied", "all_tied", "ends"):
            k = [g for g, (ag, _) in enumerate(groups) if ag == 0.75][0]
        elif name == "k_first":
            k = 0
        elif name == "k_last":
            k = len(groups) - 1
        elif exact:
            k = min(len(groups) // 2, 4)  # near the top: S + P stays below 2^11, so c' is a float32 whatever D
            if name == "exact_f0" and len(groups) > 1:
                k = max(k, 1)
        else:
            normal = [g for g, (ag, _) in enumerate(groups) if ag > 1e-30]
            k = normal[len(normal) // 2]
        x[groups[k][1][0]] = 0.5  # a room of 0.5 whichever way w pushes: P > 0
        if name == "exact_f0" and k > 0:
            x[groups[k - 1][1][0]] = 0.5  # ... and in the group above, which is the answer when c' = S
        a, r = rooms(x, w, sign)
        pr = a * r
        S, P = math.fsum(pr[[i for _, g in groups[:k] for i in g]].tolist()), math.fsum(pr[groups[k][1]].tolist())
        total = math.fsum(pr.tolist())
        if name == "exact_f0":
            frac = 0.0 if k > 0 and S > 0 else 1.0
        if name == "exact_f1":
            frac = 1.0
        cp = S + frac * P
        x0 = x.copy()
        if name == "infeasible":
            cp, frac = 2.0 * total + 1.0, None
        df = f(sign * cp)
        if name == "c_zero":  # problem 2: c = df + w_j (x0_j - x_j) = 0 exactly; problem 1 is whatever (p = x, c = df) gives
            j = groups[k][1][0]
            w[j], x[j], x0[j] = 1.0, 0.5, 0.75
            df, frac = f(-0.25), None
        # the designed answer: the group's a and the fraction; c' = S exactly belongs to the group above, wholly filled
        theta, phi = (groups[k - 1][0], 1.0) if frac == 0.0 else (groups[k][0], frac)
        case = dict(name=name, x=x, x0=x0, w=w, df=df, f=frac, exact=exact, theta=theta, phi=phi)
        if frac is not None:
            lo, hi, _ = fill_margin(x, w, float(df))
            if exact:
                assert float(df) == sign * cp and (hi == 0 or lo == 0), (name, D)  # c' = S + P, or (f = 0) c' = S
            else:
                assert P > 0 and min(lo, hi) >= 0.2 * P, (name, D, lo, hi, P)
        out.append(case)
    return out
