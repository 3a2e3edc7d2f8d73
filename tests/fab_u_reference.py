"""An independent float64 restatement of untargeted FAB (Croce & Hein 2020; Linf, L2, L1; eta = 1.05, beta = 0.9, alpha_max = 0.1, one run
from the clean point) for the tests: numpy and torch autograd only, one sample at a time.  Nothing here is shared with utils/attacks.py or
eeadv/engine.py.  What makes FAB untargeted is restated here - the explicit Jacobian, the three dual norms, the arg-min over the classes
with its skip and tie rules; from the chosen class on, the iteration is the one of tests/fab_reference.py (Linf), tests/fab_l2_reference.py
and tests/fab_l1_reference.py, called with that class as the target.

    jacobian(model, x)                       (z [K], J [K, D]): row k of J is d z_k / dx, one backward pass per class
    dual_norm(g, metric)                     sum |g| (Linf), sqrt(sum g^2) (L2), max |g| (L1); nan if g holds one
    select(z, J, y, metric)                  (k*, dist*, dists): the class of the closest linearised boundary, -1 if every class is skipped
    iterate(model, x, x0, y, adv, res, metric)   one iteration of one sample -> dict (the metric reference's, plus best_k / best)
    run(model, x0, y, n_iter, metric)        the whole run over a batch -> (adv, res, trace)
"""
import math

import numpy as np
import torch

import fab_l1_reference
import fab_l2_reference
import fab_reference

REFS = {"Linf": fab_reference, "L2": fab_l2_reference, "L1": fab_l1_reference}


def jacobian(model, x):
    """x float64 [1, ...].  One forward, K backward passes: z [K] and J [K, D] as numpy float64."""
    xc = x.detach().clone().requires_grad_()
    z = model(xc)
    K = z.shape[1]
    rows = []
    for k in range(K):
        (gk,) = torch.autograd.grad(z[0, k], [xc], retain_graph=True)
        rows.append(gk.reshape(-1).numpy().copy())
    return z[0].detach().numpy().copy(), np.stack(rows)


def dual_norm(g, metric):
    g = np.asarray(g, dtype=np.float64)
    if np.isnan(g).any():
        return float("nan")
    a = np.abs(g)
    if metric == "Linf":
        return math.fsum(a)
    if metric == "L2":
        return math.sqrt(math.fsum(a * a))
    if metric == "L1":
        return float(a.max())
    raise ValueError(metric)


def select(z, J, y, metric):
    """The class whose linearised boundary z_k - z_y = 0 is closest to the point in the dual norm: dist_k = |z_k - z_y| / (1e-12 + n_k).
    Skipped: k == y, df_k or n_k not finite, n_k == 0.  Ties go to the lower class.  Returns (k*, dist*, [dist_k or None])."""
    best_k, best, dists = -1, math.inf, []
    for k in range(len(z)):
        if k == y:
            dists.append(None)
            continue
        df = float(z[k]) - float(z[y])
        n = dual_norm(J[k] - J[y], metric)
        if not (math.isfinite(df) and math.isfinite(n)) or n == 0:
            dists.append(None)
            continue
        d = abs(df) / (1e-12 + n)
        dists.append(d)
        if d < best:
            best_k, best = k, d
    return best_k, best, dists


def iterate(model, x, x0, y, adv, res, metric):
    """One iteration of one sample.  The chosen class k* is handed to the metric reference's iterate as the target: its df is z_k* - z_y and
    its gradient d(z_k* - z_y)/dx.  No class left: the target is the label itself - df = 0, w = 0, the iteration rests."""
    z, J = jacobian(model, x)
    k, best, dists = select(z, J, y, metric)
    out = REFS[metric].iterate(model, x, x0, y, k if k >= 0 else y, adv, res)
    out.update(best_k=k, best=best, n_live=sum(d is not None for d in dists))
    return out


def run(model, x0, y, n_iter, metric):
    """The whole run, sample by sample.  Returns (adv [B,...], res [B], trace) in the layout of fab_reference.run."""
    B = x0.shape[0]
    xs = [x0[b:b + 1].clone() for b in range(B)]
    advs = [x0[b:b + 1].clone() for b in range(B)]
    ress = [math.inf] * B
    trace = []
    for _ in range(n_iter):
        rows = []
        for b in range(B):
            r = iterate(model, xs[b], x0[b:b + 1], int(y[b]), advs[b], ress[b], metric)
            r.update(x_in=xs[b], adv_in=advs[b], res_in=ress[b])
            xs[b], advs[b], ress[b] = r["x"], r["adv"], r["res"]
            rows.append(r)
        entry = {}
        for key in rows[0]:
            vals = [r[key] for r in rows]
            if isinstance(vals[0], torch.Tensor):
                entry[key] = torch.cat(vals)
            else:
                entry[key] = torch.tensor(vals, dtype=torch.float64 if isinstance(vals[0], float) else None)
        trace.append(entry)
    return torch.cat(advs), torch.tensor(ress, dtype=torch.float64), trace
