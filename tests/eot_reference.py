"""An independent restatement of the EOT iteration of APGD for the tests (Linf, one run, every gradient the mean over E forwards of a
randomised model): torch ops and autograd for the forwards, then one sample and one draw at a time in plain Python.  Nothing here is shared
with utils/attacks.py or eeadv/engine.py; the step, the bookkeeping and the copies are those of tests/apgd_reference.py.

    ScriptedDraws(net, s, o)                 forward number k computes net(x * s[k % len(s)] + o[k % len(s)]); .calls counts the forwards
    mean_gradient(gs)                        the accumulate kernel's arithmetic on E arrays, in numpy: sequential sum, then * (1 / E)
    mean_loss(ls, dtype)                     the float64 sum of E row losses in draw order, / E, cast to dtype
    eot_chunk(n_iter, E, cap)                iterations per captured graph
    run(model, x0, x_init, y, n_iter, eps, kind, E, t)   the whole attack; returns (x_adv, robust, loss_best, trace)
"""
import numpy as np
import torch

import apgd_reference as R


class ScriptedDraws(torch.nn.Module):
    """A 'randomised' model whose draws are a script: forward number k (counted from 0 over the module's life, reset by setting .calls)
    sees x * s[k % len(s)] + o[k % len(s)]."""

    def __init__(self, net, s, o):
        super().__init__()
        assert len(s) == len(o)
        self.net, self.s, self.o, self.calls = net, [float(v) for v in s], [float(v) for v in o], 0

    def forward(self, x):
        k = self.calls % len(self.s)
        self.calls += 1
        return self.net(x * self.s[k] + self.o[k])


def mean_gradient(gs):
    """numpy float32 (or float64) arrays of one shape, in draw order -> their mean as the accumulate launch forms it: acc = g_0;
    acc = acc + g_k; acc = acc * inv with inv = 1 / E formed in the arrays' dtype."""
    E = len(gs)
    dt = gs[0].dtype.type
    with np.errstate(all="ignore"):
        acc = gs[0].copy()
        for g in gs[1:]:
            acc = acc + g
        inv = dt(1) / dt(E)
        return acc * inv


def mean_loss(ls, dtype=np.float32):
    """E arrays of row losses in draw order -> (float64 sum, its mean cast to dtype)."""
    with np.errstate(all="ignore"):
        acc = ls[0].astype(np.float64)
        for l in ls[1:]:
            acc = acc + l.astype(np.float64)
        return acc, (acc / np.float64(len(ls))).astype(dtype)


def eot_chunk(n_iter, E, cap=16):
    """The largest divisor of n_iter not above max(1, cap // E)."""
    top = max(1, cap // E)
    best = 1
    for c in range(1, n_iter + 1):
        if n_iter % c == 0 and c <= top:
            best = c
    return best


def run(model, x0, x_init, y, n_iter, eps, kind, E, t=None):
    """The whole attack.  trace[0] is the start point, trace[i + 1] the state after iteration i, as apgd_reference.run records them, plus
    draw_loss [E, B], draw_g [E, B, ...] and draw_pred [E, B] of the E draws behind each gradient (E > 1)."""
    B = x0.shape[0]

    def one_draw(xc):
        xc = xc.detach().clone().requires_grad_()
        z = model(xc)
        rows, pred = R.batch_loss(z, y, kind, t)
        (g,) = torch.autograd.grad(rows.sum(), [xc])
        return rows.detach(), g.detach(), pred

    def grad_at(xc):
        draws = [one_draw(xc) for _ in range(E)]
        if E == 1:
            return draws[0] + ({},)
        inv = torch.tensor(1.0, dtype=xc.dtype) / torch.tensor(float(E), dtype=xc.dtype)
        g_mean, l_mean = torch.empty_like(xc), torch.empty(B, dtype=xc.dtype)
        for b in range(B):
            acc, lsum = draws[0][1][b].clone(), float(draws[0][0][b].to(torch.float64))
            for k in range(1, E):
                acc = acc + draws[k][1][b]
                lsum = lsum + float(draws[k][0][b].to(torch.float64))  # Python floats are float64
            g_mean[b] = acc * inv
            l_mean[b] = torch.tensor(lsum / E, dtype=torch.float64).to(xc.dtype)
        extra = dict(draw_loss=torch.stack([d[0] for d in draws]), draw_g=torch.stack([d[1] for d in draws]),
                     draw_pred=torch.stack([d[2] for d in draws]))
        return l_mean, g_mean, draws[-1][2], extra

    sched = R.schedule(n_iter)
    x = x_init.detach().clone()
    l, g, pred, extra = grad_at(x)
    book = R.Book(l, pred, eps)
    x_old, x_best, x_best_adv, g_best = x.clone(), x.clone(), x.clone(), g.clone()
    trace = [dict(x=x.clone(), x_old=x_old.clone(), g=g.clone(), x_new=x.clone(), g_new=g.clone(), loss=l.clone(), pred=pred.clone(),
                  x_best=x_best.clone(), g_best=g_best.clone(), x_best_adv=x_best_adv.clone(), **extra, **book.snapshot())]
    for i in range(n_iter):
        x, x_old = R.step(x, x_old, g, x0, torch.stack(book.step), eps, 1.0 if i == 0 else 0.75)
        l, g, pred, extra = grad_at(x)
        x_new, g_new = x.clone(), g.clone()
        improved, fooled, reduced, osc, noimp = book.update(l, pred, sched.get(i, 0))
        x, g, x_best, g_best, x_best_adv = R.apply_flags(x, g, x_best, g_best, x_best_adv, improved, fooled, reduced)
        trace.append(dict(x=x.clone(), x_old=x_old.clone(), g=g.clone(), x_new=x_new, g_new=g_new, loss=l.clone(), pred=pred.clone(),
                          x_best=x_best.clone(), g_best=g_best.clone(), x_best_adv=x_best_adv.clone(), improved=improved, fooled=fooled,
                          reduced=reduced, osc=osc, noimp=noimp, k=sched.get(i, 0), **extra, **book.snapshot()))
    robust = torch.tensor(book.robust)
    x_adv = x0.clone()
    for b in range(B):
        if not book.robust[b]:
            x_adv[b] = x_best_adv[b]
    return x_adv, robust, torch.stack(book.loss_best), trace
