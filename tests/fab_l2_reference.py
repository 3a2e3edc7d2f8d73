"""An independent float64 restatement of FAB-T in the L2 threat model (Croce & Hein 2020; targeted, eta = 1.05, beta = 0.9, alpha_max = 0.1,
one run from the clean point) for the tests: numpy, math.fsum and torch autograd only, one sample at a time.  Nothing here is shared with
utils/attacks.py, eeadv/engine.py or tests/fab_reference.py.

    rooms(p, w, s)                    (|v_i|, r_i) of v = s w at the point p
    project(p, w, c)                  the box-constrained least-L2 projection by explicit sort and segment walk -> (mu, s, norm, delta)
    g_of(mu, a, r)                    sum_i a_i min(mu a_i, r_i)
    project_f32(p, w, c)              the same walk in float32 (sort + sequential cumsum) -> (mu, norm): the yardstick for a float32 kernel
    l2(v)                             sqrt(fsum(v_i^2))
    step_f32(x, x0, w, scal6)         the step in float32, one rounding per operation, from given projection scalars
    shrink_f32(x, x0)                 x0 + 0.9 (x - x0) in float32
    iterate(model, x, x0, y, t, adv, res, w=None)   one iteration of one sample -> dict (w: a gradient to use instead of autograd's)
    run(model, x0, y, t, n_iter)      the whole run over a batch -> (adv, res, trace)
"""
import math

import numpy as np
import torch

ETA, BETA, ALPHA_MAX = 1.05, 0.9, 0.1


def rooms(p, w, s):
    v = s * w
    a = np.abs(v)
    r = np.where(v > 0, p, np.where(v < 0, 1.0 - p, 0.0))
    return a, np.maximum(r, 0.0)


def g_of(mu, a, r):
    keep = a != 0
    return float(np.sum(a[keep] * np.minimum(mu * a[keep], r[keep])))


def l2(v):
    return math.sqrt(math.fsum(float(e) * float(e) for e in np.asarray(v).reshape(-1)))


def _walk(a, r, cp):
    """mu of the segment walk over the breakpoints t_i = r_i / a_i in ascending order, float64; inf when infeasible.  In segment k the
    coordinates before k sit at their bounds and the others move by mu a_i: mu_k = (c' - sum_{j < k} a_j r_j) / sum_{j >= k} a_j^2, and the
    first segment whose mu_k does not pass its breakpoint holds the solution."""
    keep = a != 0
    a, r = a[keep], r[keep]
    if a.size == 0:
        return math.inf
    with np.errstate(over="ignore"):
        t = r / a
    order = np.argsort(t, kind="stable")
    a, r, t = a[order], r[order], t[order]
    below = np.concatenate((np.zeros(1), np.cumsum(a * r)))  # below[k] = sum_{j < k} a_j r_j
    if cp >= below[-1]:
        return math.inf
    above = np.cumsum((a * a)[::-1])[::-1]  # above[k] = sum_{j >= k} a_j^2, from the top: no term is ever subtracted
    for k in range(a.size):
        if above[k] == 0:  # only coordinates whose square underflows are left: nothing can take the rest of c'
            break
        mu = (cp - below[k]) / above[k]
        if mu <= t[k]:
            return float(mu)
    return math.inf


def project(p, w, c):
    """p, w float64 [D], c float.  Returns (mu, s, norm, delta): delta_i = -sign(s w_i) min(mu a_i, r_i), 0 where w_i == 0."""
    p, w = np.asarray(p, dtype=np.float64), np.asarray(w, dtype=np.float64)
    s = 1.0 if c >= 0 else -1.0
    a, r = rooms(p, w, s)
    cp = abs(float(c))
    mu = 0.0 if cp == 0 else _walk(a, r, cp)
    move = np.zeros_like(p)
    keep = a != 0
    move[keep] = r[keep] if math.isinf(mu) else np.minimum(mu * a[keep], r[keep])
    delta = -np.sign(s * w) * move
    return mu, s, l2(move), delta


def project_f32(p, w, c):
    """The walk in float32 on float32 inputs (c already rounded to float32), every operation rounded to float32: numpy sort, sequential
    cumulative sums.  Returns (mu, norm) as floats."""
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
        return math.inf, 0.0
    with np.errstate(over="ignore"):
        t = (r / a).astype(f)
    order = np.argsort(t, kind="stable")
    a, r, t = a[order], r[order], t[order]
    below = np.cumsum(a * r, dtype=f)
    mu = f(np.inf)
    if cp < below[-1]:
        above = np.cumsum((a * a)[::-1], dtype=f)[::-1]  # sum_{j >= k} a_j^2
        prev = np.concatenate((np.zeros(1, dtype=f), below[:-1]))
        with np.errstate(divide="ignore", invalid="ignore"):  # the squares of denormal |w_i| underflow in float32
            cand = ((cp - prev) / above).astype(f)
        ok = cand <= t
        if ok.any():
            mu = cand[int(np.argmax(ok))]
    move = r if np.isinf(mu) else np.minimum((mu * a).astype(f), r)
    norm = np.sqrt(np.cumsum((move * move).astype(f), dtype=f)[-1], dtype=f)
    return float(mu), float(norm)


def step_f32(x, x0, w, scal):
    """The step of one sample in float32 arithmetic, every operation rounded once, from scal = (mu1, s1, n1, mu2, s2, n2) as given (the
    scalars of the code under test): x, x0, w float32 [D] -> the stepped point, float32 [D]."""
    f = np.float32
    mu1, s1, n1, mu2, s2, n2 = (f(v) for v in scal)
    if s1 == 0:
        return x.copy()

    def delta(p, s, mu):
        v = s * w
        a = np.abs(v)
        r = np.maximum(np.where(v > 0, p, np.where(v < 0, f(1) - p, f(0))), f(0))
        with np.errstate(invalid="ignore"):
            m = np.where(a != 0, np.minimum(mu * a, r), f(0))
        return (-np.sign(v) * m).astype(f)

    a1, a2 = max(n1, f(1e-8)), max(n2, f(1e-8))
    alpha = min(f(a1 / f(a1 + a2)), f(ALPHA_MAX))
    d1, d2 = delta(x, s1, mu1), delta(x0, s2, mu2)
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
        mu1, s1, n1, d1 = project(x_np, w_np, df)
        mu2, s2, n2, d2 = project(x0_np, w_np, c2)
        a1, a2 = max(n1, 1e-8), max(n2, 1e-8)
        alpha = min(a1 / (a1 + a2), ALPHA_MAX)
        x_step = np.clip((x_np + ETA * d1) * (1 - alpha) + (x0_np + ETA * d2) * alpha, 0.0, 1.0)
    else:
        mu1 = s1 = n1 = mu2 = s2 = n2 = alpha = c2 = 0.0
        x_step = x_np.copy()
    x_step_t = torch.from_numpy(x_step).view(shape)
    with torch.no_grad():
        z2 = model(x_step_t)
    pred, nan = first_class(z2[0])
    out["z2"] = z2.detach().clone()
    is_adv = (pred != y) and not nan
    nrm = l2(x_step - x0_np)
    improved = is_adv and nrm < res
    if improved:
        adv, res = x_step_t.clone(), nrm
    x_new = torch.from_numpy(x0_np + BETA * (x_step - x0_np)).view(shape) if is_adv else x_step_t
    out.update(c2=c2, lam1=mu1, s1=s1, n1=n1, lam2=mu2, s2=s2, n2=n2, alpha=alpha, x_step=x_step_t, pred=pred, is_adv=is_adv, improved=improved,
               nrm=nrm, x=x_new, adv=adv, res=res)
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
