"""An independent restatement of APGD in the L2 threat model (Croce & Hein 2020, the L2 branch) for the tests: one sample at a time, torch
ops in the dtype of its inputs (float64 in the host tests), every norm sqrt(math.fsum(squares)) - exact summation.  Nothing here is
shared with utils/attacks.py or eeadv/engine.py; the losses, the bookkeeping and the copies, which do not know the norm, are those of
tests/apgd_reference.py.

    norm(v)                                        ||v||_2 of one sample as a Python float: sqrt of the exactly summed squares
    step_row(x, xo, g, x0, step, eps, a, norms)    one sample's step -> (x_new, [ng, n1, n2]); norms: teacher-forced scalars, else its own
    step(x, xo, g, x0, step, eps, a, norms)        the batch: (x_new, x, norms [3, B]); the second is the new x_old
    start(x0, eps, n)                              clamp(x0 + eps n / (||n|| + 1e-12), 0, 1), per sample
    ball_excess(x, x0, eps)                        max over the batch of ||x - x0||_2 / eps - 1
    run(model, x0, x_init, y, n_iter, eps, kind, t, forced)   the whole attack; forced: the gradient evaluations to use instead of its own
"""
import math

import torch

import apgd_reference as R

TINY = torch.tensor(1e-12, dtype=torch.float32)  # the float32 constant 1e-12f in every dtype


def norm(v):
    vals = [float(t) for t in v.detach().to(torch.float64).flatten()]
    return math.sqrt(math.fsum(t * t for t in vals))  # the square of a float32 is exact in a double


def step_row(x, xo, g, x0, step, eps, a, norms=None):
    """One sample (tensors of one shape and dtype, step a 0-dim tensor).  Returns (x_new, own) with own = [ng, n1, n2] as 0-dim tensors of
    that dtype; `norms` (three 0-dim tensors) replaces them in the arithmetic - teacher forcing on somebody else's norms."""
    dt = x.dtype
    tiny, radius = TINY.to(dt), torch.tensor(eps, dtype=dt)
    own = []

    def take(v):
        own.append(torch.tensor(norm(v), dtype=torch.float64).to(dt))
        return own[-1] if norms is None else norms[len(own) - 1].to(dt)

    ng = take(g)
    z = x + g * (step / (ng + tiny)) if math.isfinite(float(ng)) else x  # a gradient without a finite norm moves nothing
    d = z - x0
    n1 = take(d)
    z = torch.clamp(x0 + d * (torch.minimum(radius, n1) / (n1 + tiny)), 0, 1)
    m = (x + (z - x) * a) + (x - xo) * (1.0 - a)
    d = m - x0
    n2 = take(d)
    return torch.clamp(x0 + d * (torch.minimum(radius, n2) / (n2 + tiny)), 0, 1), own


def step(x, xo, g, x0, step_size, eps, a, norms=None):
    """step_size [B]; norms [3, B] or None.  Returns (x_new, x, own norms [3, B])."""
    rows, own = [], []
    for b in range(x.shape[0]):
        r, o = step_row(x[b], xo[b], g[b], x0[b], step_size[b], eps, a, None if norms is None else [norms[k, b] for k in range(3)])
        rows.append(r)
        own.append(torch.stack(o))
    return torch.stack(rows), x, torch.stack(own, dim=1)


def start(x0, eps, n):
    rows = []
    for b in range(x0.shape[0]):
        nb = torch.tensor(norm(n[b]), dtype=torch.float64).to(x0.dtype)
        rows.append(torch.clamp(x0[b] + n[b] * (torch.tensor(eps, dtype=x0.dtype) / (nb + TINY.to(x0.dtype))), 0, 1))
    return torch.stack(rows)


def ball_excess(x, x0, eps):
    return max(norm(x[b].to(torch.float64) - x0[b].to(torch.float64)) / eps - 1.0 for b in range(x.shape[0]))


def run(model, x0, x_init, y, n_iter, eps, kind, t=None, forced=None):
    """The whole attack, as apgd_reference.run with the L2 step.  trace[0] is the start point, trace[i + 1] the state after iteration i:
    x, x_old, g (after the copies), x_new / g_new (before them), norms [3, B] of the step, loss, pred, the scalars and the flag lists.
    forced: a list of n_iter + 1 dicts {"loss", "g", "pred"[, "norms"]} - the gradient evaluations (the start's first) and, when present,
    the norms of the step BEFORE that evaluation, used in the place of this module's own."""
    def grad_at(xc, k):
        if forced is not None:
            f = forced[k]
            return f["loss"].clone(), f["g"].clone(), f["pred"].clone()
        xc = xc.detach().clone().requires_grad_()
        z = model(xc)
        rows, pred = R.batch_loss(z, y, kind, t)
        (g,) = torch.autograd.grad(rows.sum(), [xc])
        return rows.detach(), g.detach(), pred

    sched = R.schedule(n_iter)
    x = x_init.detach().clone()
    l, g, pred = grad_at(x, 0)
    book = R.Book(l, pred, eps)
    x_old, x_best, x_best_adv, g_best = x.clone(), x.clone(), x.clone(), g.clone()
    trace = [dict(x=x.clone(), x_old=x_old.clone(), g=g.clone(), x_new=x.clone(), g_new=g.clone(), loss=l.clone(), pred=pred.clone(),
                  x_best=x_best.clone(), g_best=g_best.clone(), x_best_adv=x_best_adv.clone(), **book.snapshot())]
    for i in range(n_iter):
        given = None if forced is None else forced[i + 1].get("norms")
        x, x_old, norms = step(x, x_old, g, x0, torch.stack(book.step), eps, 1.0 if i == 0 else 0.75, given)
        l, g, pred = grad_at(x, i + 1)
        x_new, g_new = x.clone(), g.clone()
        improved, fooled, reduced, osc, noimp = book.update(l, pred, sched.get(i, 0))
        x, g, x_best, g_best, x_best_adv = R.apply_flags(x, g, x_best, g_best, x_best_adv, improved, fooled, reduced)
        trace.append(dict(x=x.clone(), x_old=x_old.clone(), g=g.clone(), x_new=x_new, g_new=g_new, norms=norms, loss=l.clone(),
                          pred=pred.clone(), x_best=x_best.clone(), g_best=g_best.clone(), x_best_adv=x_best_adv.clone(), improved=improved,
                          fooled=fooled, reduced=reduced, osc=osc, noimp=noimp, k=sched.get(i, 0), **book.snapshot()))
    robust = torch.tensor(book.robust)
    x_adv = x0.clone()
    for b in range(x0.shape[0]):
        if not book.robust[b]:
            x_adv[b] = x_best_adv[b]
    return x_adv, robust, torch.stack(book.loss_best), trace
