"""An independent restatement of APGD in the L1 threat model (Croce & Hein 2021, "Mind the box") for the tests, written from DESIGN.md
section 19: one sample at a time in numpy, element-wise arithmetic in the dtype of its inputs (float64 in the host tests, float32 against
the kernels), selection by numpy.sort, the projection's multiplier by a search over the sorted breakpoints with every sum taken exactly
(math.fsum).  Nothing here is shared with utils/attacks.py or eeadv/engine.py.

    project_row(u, x0, eps, lam=None)       P(u) of one sample -> (z, info); info: lam (float64, before its cast), h0, active, bad
    step_row(x, g, x0, step, topk, eps, lam=None, tau=None)   one sample's step -> (x_new, info); info also: tau, m, j, u
    nonzero(v, x0)                          #{i : v_i != x0_i}
    checkpoint(sp, sp_old, step, eps, D, dtype)   the rule -> (red, topk, step)
    schedule(n_iter)                        {iteration (0-based): window length} of the iterations a checkpoint closes
    l1_excess(x, x0, eps)                   max over the batch of ||x - x0||_1 - eps, summed exactly
    run(model, x0, x_init, y, n_iter, eps, kind, t, forced)   the whole attack; forced: the gradient evaluations to use instead of its own
A `lam` / `tau` argument replaces the module's own value in the arithmetic: teacher forcing on somebody else's scalars.
"""
import math

import numpy as np
import torch

F32 = np.float32


def _c(v, dt):
    """The float32 constant v in the dtype dt."""
    return np.dtype(dt).type(F32(v))


def _h(a, lo, lam):
    """h(lam) = sum_i (a_i - min(max(lam, lo_i), a_i)), exactly summed (a, lo float64)."""
    c = np.minimum(np.maximum(lam, lo), a)
    return math.fsum(a.tolist() + (-c).tolist())


def coords(u, x0):
    """(w, a, lo) of one sample in its dtype: w = u - x0, a = |w|, lo = min(max(0, -min(1 - u, u)), a)."""
    dt = u.dtype.type
    w = u - x0
    a = np.abs(w)
    with np.errstate(invalid="ignore"):
        lo = np.minimum(np.maximum(dt(0), -np.minimum(dt(1) - u, u)), a)
    return w, a, lo


def multiplier(a, lo, eps):
    """(lam as a float64 before any cast, h0, |A|) for the breakpoints a, lo (any float dtype; finite)."""
    a64, lo64 = a.astype(np.float64), lo.astype(np.float64)
    h0 = _h(a64, lo64, 0.0)
    if h0 <= eps:
        return 0.0, h0, 0
    bp = np.unique(np.concatenate([lo64, a64, [0.0]]))  # sorted; h(bp[0] = 0) > eps, h(bp[-1]) = 0 <= eps
    lo_i, hi_i = 0, len(bp) - 1
    while hi_i - lo_i > 1:  # the last breakpoint with h > eps
        mid = (lo_i + hi_i) // 2
        if _h(a64, lo64, bp[mid]) > eps:
            lo_i = mid
        else:
            hi_i = mid
    t = bp[lo_i]
    act = (lo64 <= t) & (a64 > t)
    fixed = (lo64 > t) & (a64 > t)
    n = int(act.sum())
    if n == 0:
        return float(bp[hi_i]), h0, 0
    terms = a64[fixed].tolist() + (-lo64[fixed]).tolist() + a64[act].tolist() + [-float(eps)]
    return math.fsum(terms) / n, h0, n


def project_row(u, x0, eps, lam=None):
    """P(u) of one sample (1-D arrays of one dtype).  info["lam"] is the module's own multiplier as a float64; the arithmetic uses `lam`
    when given, else that value cast to the dtype."""
    dt = u.dtype.type
    w, a, lo = coords(u, x0)
    if not np.isfinite(w).all():
        return x0.copy(), dict(lam=0.0, h0=math.inf, active=0, bad=True)
    own, h0, n = multiplier(a, lo, float(eps))
    use = dt(own) if lam is None else dt(lam)
    cut = np.minimum(np.maximum(use, lo), a)
    z = np.clip(x0 + np.sign(w) * (a - cut), dt(0), dt(1))
    return z.astype(u.dtype), dict(lam=own, h0=h0, active=n, bad=False)


def select(g, topk, D):
    """(j, tau, m, finite): the rank, the threshold (ordered by the bit pattern of |g|), the count of moved coordinates."""
    dt = g.dtype.type
    v = np.floor((dt(1) - dt(topk)) * dt(D))
    j = 0 if not v >= 0 else (D - 1 if v >= D else int(v))
    ab = np.abs(g)
    bits = ab.view(np.uint32 if g.dtype == np.float32 else np.uint64)
    tau = ab[np.argsort(bits, kind="stable")[j]]
    tau_bits = tau.view(bits.dtype)
    mask = bits >= tau_bits
    m = int((mask & ((g < 0) | (g > 0))).sum())
    return j, tau, m, bool(np.isfinite(g).all())


def step_row(x, g, x0, step, topk, eps, lam=None, tau=None):
    dt = x.dtype.type
    D = x.size
    j, own_tau, m, finite = select(g, topk, D)
    t = own_tau if tau is None else dt(tau)
    bits = np.abs(g).view(np.uint32 if g.dtype == np.float32 else np.uint64)
    mask = bits >= np.abs(t).view(bits.dtype)
    m_used = int((mask & ((g < 0) | (g > 0))).sum())
    with np.errstate(over="ignore", invalid="ignore"):
        sg = dt(step) / (dt(m_used) + _c(1e-10, x.dtype))
        s = np.sign(np.nan_to_num(g, nan=0.0))
        moved = x + sg * s
    u = np.where(mask & (s != 0), moved, x).astype(x.dtype) if finite else x.copy()
    z, info = project_row(u, x0, eps, lam)
    info.update(j=j, tau=own_tau, m=m, u=u, finite=finite)
    return z, info


def nonzero(v, x0):
    return int((v != x0).sum())


def checkpoint(sp, sp_old, step, eps, D, dtype):
    dt = np.dtype(dtype).type
    with np.errstate(divide="ignore", invalid="ignore"):
        red = bool(dt(sp) / dt(sp_old) < _c(0.95, dtype))
    topk = dt(sp) / dt(D) / _c(1.5, dtype)
    s = dt(eps) if red else dt(step) / _c(1.5, dtype)
    s = min(max(s, dt(eps) / _c(10.0, dtype)), dt(eps))
    return red, topk, s


def schedule(n_iter):
    first, later = max(int(0.04 * n_iter), 1), max(int(0.06 * n_iter), 1)
    out, i, k = {}, -1, first
    while True:
        i += k
        if i >= n_iter:
            return out
        out[i] = k
        k = later


def l1_excess(x, x0, eps):
    x, x0 = np.asarray(x, dtype=np.float64), np.asarray(x0, dtype=np.float64)
    return max(math.fsum(np.abs(x[b] - x0[b]).ravel().tolist()) - eps for b in range(x.shape[0]))


def _row_losses(z, y, kind, t):
    """Row losses of logits [B, K] (torch, any dtype) and pred; classes by value descending, ties to the lower index."""
    rows = torch.arange(z.shape[0])
    zs, order = torch.sort(z, dim=1, descending=True, stable=True)
    pred = order[:, 0] == y
    if kind == "ce":
        return torch.logsumexp(z, dim=1) - z[rows, y], pred
    tiny = torch.tensor(1e-12, dtype=torch.float32).to(z.dtype)
    if kind == "dlr_t":
        return -(z[rows, y] - z[rows, t]) / ((zs[:, 0] - (zs[:, 2] + zs[:, 3]) * 0.5) + tiny), pred
    raise ValueError(kind)


def run(model, x0, x_init, y, n_iter, eps, kind, t=None, forced=None):
    """The whole attack on torch tensors (any float dtype); x_init is the unprojected start x0 + n.  trace[0] is the start point,
    trace[i + 1] the state after iteration i.  forced: n_iter + 1 dicts {"loss", "g", "pred"[, "lam", "tau"]} - the gradient evaluations
    (the start's first) and, when present, the scalars of the step (the start: of the projection) BEFORE that evaluation, used in the
    place of this module's own."""
    npdt = np.float64 if x0.dtype == torch.float64 else np.float32
    dt = npdt
    B = x0.shape[0]
    D = x0[0].numel()
    c0 = x0.detach().numpy().reshape(B, D).astype(npdt)

    def grad_at(xn, k):
        if forced is not None:
            f = forced[k]
            return (np.asarray(f["loss"], dtype=npdt).copy(), np.asarray(f["g"], dtype=npdt).reshape(B, D).copy(),
                    np.asarray(f["pred"]).astype(bool).copy())
        xc = torch.from_numpy(xn.reshape(x0.shape).copy()).requires_grad_()
        z = model(xc)
        rows, pred = _row_losses(z, y, kind, t)
        (g,) = torch.autograd.grad(rows.sum(), [xc])
        return rows.detach().numpy().astype(npdt), g.numpy().reshape(B, D).astype(npdt), pred.numpy()

    def given(k, name, b):
        if forced is None or name not in forced[k]:
            return None
        return np.asarray(forced[k][name]).reshape(-1)[b]

    sched = schedule(n_iter)
    u0 = x_init.detach().numpy().reshape(B, D).astype(npdt)
    rows, infos = zip(*[project_row(u0[b], c0[b], eps, given(0, "lam", b)) for b in range(B)])
    x = np.stack(rows)
    l, g, pred = grad_at(x, 0)
    step = np.full(B, dt(eps), dtype=npdt)
    topk = np.full(B, _c(0.2, npdt), dtype=npdt)
    sp_old = np.full(B, D, dtype=np.int64)
    loss_best, robust = l.copy(), pred.copy()
    x_best, g_best, x_best_adv = x.copy(), g.copy(), x.copy()

    def snap(**kw):
        e = dict(x=x.copy(), g=g.copy(), loss=l.copy(), pred=pred.copy(), step=step.copy(), topk=topk.copy(), sp_old=sp_old.copy(),
                 loss_best=loss_best.copy(), robust=robust.copy(), x_best=x_best.copy(), g_best=g_best.copy(), x_best_adv=x_best_adv.copy())
        e.update(kw)
        return e

    trace = [snap(infos=list(infos))]
    for i in range(n_iter):
        rows, infos = zip(*[step_row(x[b], g[b], c0[b], step[b], topk[b], eps, given(i + 1, "lam", b), given(i + 1, "tau", b))
                            for b in range(B)])
        x = np.stack(rows)
        l, g, pred = grad_at(x, i + 1)
        x_new, g_new = x.copy(), g.copy()
        fooled = ~pred
        robust = robust & pred
        with np.errstate(invalid="ignore"):
            improved = l > loss_best
        loss_best = np.where(improved, l, loss_best)
        x_best_adv[fooled] = x[fooled]
        x_best[improved] = x[improved]
        g_best[improved] = g[improved]
        k = sched.get(i, 0)
        reduced, sp = np.zeros(B, dtype=bool), np.zeros(B, dtype=np.int64)
        if k:
            for b in range(B):
                sp[b] = nonzero(x_best[b], c0[b])
                reduced[b], topk[b], step[b] = checkpoint(sp[b], sp_old[b], step[b], eps, D, npdt)
                sp_old[b] = sp[b]
            x[reduced] = x_best[reduced]
            g[reduced] = g_best[reduced]
        trace.append(snap(x_new=x_new, g_new=g_new, infos=list(infos), improved=improved, fooled=fooled, reduced=reduced, sp=sp, k=k))
    x_adv = np.where(robust[:, None], c0, x_best_adv)
    return x_adv.reshape(tuple(x0.shape)), robust, loss_best, trace
