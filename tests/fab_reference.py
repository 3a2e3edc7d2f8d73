"""An independent float64 restatement of FAB-T (Croce & Hein 2020; Linf, targeted, eta = 1.05, beta = 0.9, alpha_max = 0.1, one run from the
clean point) for the tests: numpy and torch autograd only, one sample at a time.  Nothing here is shared with utils/attacks.py or
eeadv/engine.py.

    rooms(p, w, s)                    (|v_i|, r_i) of v = s w at the point p
    project(p, w, c)                  the box-constrained Linf projection by explicit sort and segment walk -> (lam, s, norm, delta)
    g_of(lam, a, r)                   sum_i a_i min(lam, r_i)
    lambda_f32(p, w, c)               the same walk in float32 (sort + sequential cumsum): the yardstick for a float32 kernel's error
    iterate(model, x, x0, y, t, adv, res)   one iteration of one sample -> dict
    run(model, x0, y, t, n_iter)      the whole run over a batch -> (adv, res, trace)
"""
import numpy as np
import torch

ETA, BETA, ALPHA_MAX = 1.05, 0.9, 0.1


def rooms(p, w, s):
    v = s * w
    a = np.abs(v)
    r = np.where(v > 0, p, np.where(v < 0, 1.0 - p, 0.0))
    return a, np.maximum(r, 0.0)


def g_of(lam, a, r):
    return float(np.sum(a * np.minimum(lam, r)))


def _walk(a, r, cp, dtype):
    """lam of the segment walk over the sorted breakpoints, all arithmetic in `dtype`; inf when infeasible."""
    keep = a != 0
    a, r = a[keep].astype(dtype), r[keep].astype(dtype)
    cp = dtype(cp)
    if a.size == 0:
        return dtype(np.inf)
    order = np.argsort(r, kind="stable")
    a, r = a[order], r[order]
    below = np.cumsum(a * r, dtype=dtype)  # sum_{j <= k} a_j r_j, sequentially
    if cp >= below[-1]:
        return dtype(np.inf)
    above = np.cumsum(a[::-1], dtype=dtype)[::-1]  # sum_{j >= k} a_j
    # segment k: every coordinate before k sits at its bound, the others move by lam; the first k whose lam does not pass r_k holds the solution
    prev = np.concatenate((np.zeros(1, dtype=dtype), below[:-1]))
    lam = (cp - prev) / above
    ok = lam <= r
    return lam[int(np.argmax(ok))] if ok.any() else dtype(np.inf)


def project(p, w, c):
    """p, w float64 [D], c float.  Returns (lam, s, norm, delta): delta_i = -sign(s w_i) min(lam, r_i)."""
    p, w = np.asarray(p, dtype=np.float64), np.asarray(w, dtype=np.float64)
    s = 1.0 if c >= 0 else -1.0
    a, r = rooms(p, w, s)
    cp = abs(float(c))
    lam = 0.0 if cp == 0 else float(_walk(a, r, cp, np.float64))
    delta = -np.sign(s * w) * np.minimum(lam, r)
    moving = r[a != 0]
    norm = min(lam, float(moving.max())) if moving.size else 0.0
    return lam, s, norm, delta


def lambda_f32(p, w, c):
    """The walk in float32 on float32 inputs (c already rounded to float32)."""
    p, w = np.asarray(p, dtype=np.float32), np.asarray(w, dtype=np.float32)
    s = np.float32(1.0 if c >= 0 else -1.0)
    v = s * w
    a = np.abs(v)
    r = np.maximum(np.where(v > 0, p, np.where(v < 0, np.float32(1) - p, np.float32(0))), np.float32(0))
    return float(_walk(a, r, abs(np.float32(c)), np.float32))


def first_class(z_row):
    """The first class by value descending, ties to the lower index, NaN above everything; and whether the row holds a NaN."""
    vals = [float(v) for v in z_row]
    nan = any(v != v for v in vals)
    order = sorted(range(len(vals)), key=lambda c: (0 if vals[c] != vals[c] else 1, -vals[c] if vals[c] == vals[c] else 0.0, c))
    return order[0], nan


def iterate(model, x, x0, y, t, adv, res):
    """One iteration of one sample: x, x0, adv float64 tensors [1, ...]; y, t ints; res float.  Returns a dict with every intermediate."""
    shape = x0.shape
    xc = x.detach().clone().requires_grad_()
    z = model(xc)
    diff = z[0, t] - z[0, y]
    (w,) = torch.autograd.grad(diff, [xc])
    df = float(diff.detach())
    w_np, x_np, x0_np = w.reshape(-1).numpy().copy(), x.detach().reshape(-1).numpy().copy(), x0.reshape(-1).numpy().copy()
    sabs = float(np.sum(np.abs(w_np)))
    enabled = bool(np.isfinite(df) and df != 0 and np.isfinite(sabs) and sabs > 0)
    out = dict(df=df, zt=float(z[0, t].detach()), zy=float(z[0, y].detach()), w=w.detach().clone(), enabled=enabled)
    if enabled:
        c2 = df + float(np.sum(w_np * (x0_np - x_np)))
        lam1, s1, n1, d1 = project(x_np, w_np, df)
        lam2, s2, n2, d2 = project(x0_np, w_np, c2)
        a1, a2 = max(n1, 1e-8), max(n2, 1e-8)
        alpha = min(a1 / (a1 + a2), ALPHA_MAX)
        x_step = np.clip((x_np + ETA * d1) * (1 - alpha) + (x0_np + ETA * d2) * alpha, 0.0, 1.0)
    else:
        lam1 = s1 = n1 = lam2 = s2 = n2 = alpha = c2 = 0.0
        x_step = x_np.copy()
    x_step_t = torch.from_numpy(x_step).view(shape)
    with torch.no_grad():
        z2 = model(x_step_t)
    pred, nan = first_class(z2[0])
    out["z2"] = z2.detach().clone()
    is_adv = (pred != y) and not nan
    nrm = float(np.max(np.abs(x_step - x0_np)))
    improved = is_adv and nrm < res
    if improved:
        adv, res = x_step_t.clone(), nrm
    x_new = torch.from_numpy(x0_np + BETA * (x_step - x0_np)).view(shape) if is_adv else x_step_t
    out.update(c2=c2, lam1=lam1, s1=s1, n1=n1, lam2=lam2, s2=s2, n2=n2, alpha=alpha, x_step=x_step_t, pred=pred, is_adv=is_adv, improved=improved,
               nrm=nrm, x=x_new, adv=adv, res=res)
    return out


def run(model, x0, y, t, n_iter):
    """The whole run, sample by sample.  Returns (adv [B,...], res [B], trace): trace[i] holds, per key, the batch-stacked values of
    iteration i, and 'x_in' / 'adv_in' / 'res_in', the state the iteration started from."""
    B = x0.shape[0]
    xs = [x0[b:b + 1].clone() for b in range(B)]
    advs = [x0[b:b + 1].clone() for b in range(B)]
    ress = [float("inf")] * B
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
