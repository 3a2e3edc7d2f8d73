"""An independent restatement of APGD (Linf, one run) for the tests: torch ops and autograd only, any float dtype, the bookkeeping one
sample at a time in plain Python.  Nothing here is shared with utils/attacks.py or eeadv/engine.py.

    schedule(n_iter)                         the checkpoints as {iteration (0-based): window length k}
    row_loss(z_row, y, kind, t)              one row's loss as a 0-dim tensor (autograd flows through it)
    row_loss_grad(z_row, y, kind, t)         (loss, d loss / d z_row) from the closed form, no autograd
    pred_row(z_row, y)                       is the first class in the order (value descending, ties to the lower index) the label
    step(x, x_old, g, x0, step, eps, a)      the momentum step -> (x_new, x_old_new)
    Book(l0, pred0, eps)                     the per-sample scalars; .update(l, pred, k) -> per-sample flag lists
    run(model, x0, x_init, y, n_iter, eps, kind, t)   the whole attack; returns (x_adv, robust, loss_best, trace)
"""
import torch

TINY = torch.tensor(1e-12, dtype=torch.float32)  # the DLR denominators add the float32 constant 1e-12f in every dtype


def schedule(n_iter):
    k = max(int(0.22 * n_iter), 1)
    n_min = max(int(0.06 * n_iter), 1)
    dec = max(int(0.03 * n_iter), 1)
    out, count = {}, 0
    for i in range(n_iter):
        count += 1
        if count == k:
            out[i] = k
            count = 0
            k = max(k - dec, n_min)
    return out


def order_row(z_row):
    """Class indices by value descending, ties to the lower index."""
    vals = [float(v) for v in z_row.detach().to(torch.float64)]
    return sorted(range(len(vals)), key=lambda c: (-vals[c], c))


def pred_row(z_row, y):
    return order_row(z_row)[0] == int(y)


def row_loss(z_row, y, kind, t=None):
    y = int(y)
    if kind == "ce":
        return torch.logsumexp(z_row, dim=0) - z_row[y]
    p = order_row(z_row)
    tiny = TINY.to(z_row.dtype)
    if kind == "dlr":
        o = p[1] if p[0] == y else p[0]
        return -(z_row[y] - z_row[o]) / ((z_row[p[0]] - z_row[p[2]]) + tiny)
    if kind == "dlr_t":
        return -(z_row[y] - z_row[int(t)]) / ((z_row[p[0]] - (z_row[p[2]] + z_row[p[3]]) * 0.5) + tiny)
    raise ValueError(kind)


def row_loss_grad(z_row, y, kind, t=None):
    """Loss and gradient of one row from the closed form (contributions summed where indices coincide)."""
    z = z_row.detach()
    y = int(y)
    grad = torch.zeros_like(z)
    if kind == "ce":
        lse = torch.logsumexp(z, dim=0)
        grad = torch.exp(z - lse)
        grad[y] -= 1
        return lse - z[y], grad
    p = order_row(z)
    tiny = TINY.to(z.dtype)
    if kind == "dlr":
        # where the label is p1 or p3 two contributions land on one class and nearly cancel (-1/d + n/d^2 with n ~ d): summed there
        # analytically - d + n and n - d are single differences of logits - so that the reference's own error stays at rounding level
        d = (z[p[0]] - z[p[2]]) + tiny
        if p[0] == y:
            n = z[y] - z[p[1]]
            grad[y] = -((z[p[1]] - z[p[2]]) + tiny) / (d * d)
            grad[p[1]] = 1 / d
            grad[p[2]] = -n / (d * d)
        else:
            n = z[y] - z[p[0]]
            grad[p[0]] = ((z[y] - z[p[2]]) + tiny) / (d * d)
            if p[2] == y:
                grad[y] = -tiny / (d * d)
            else:
                grad[y] = -1 / d
                grad[p[2]] = -n / (d * d)
        return -n / d, grad
    o = int(t)
    d = (z[p[0]] - (z[p[2]] + z[p[3]]) * 0.5) + tiny
    n = z[y] - z[o]
    grad[y] += -1 / d
    grad[o] += 1 / d
    grad[p[0]] += n / (d * d)
    for c in (p[2], p[3]):
        grad[c] += -0.5 * n / (d * d)
    return -n / d, grad


def batch_loss(z, y, kind, t=None):
    """Row losses [B] (autograd flows) and pred [B] bool."""
    rows = [row_loss(z[b], y[b], kind, None if t is None else t[b]) for b in range(z.shape[0])]
    pred = torch.tensor([pred_row(z[b], y[b]) for b in range(z.shape[0])], dtype=torch.bool)
    return torch.stack(rows), pred


def project(v, x0, eps):
    return torch.clamp(torch.min(torch.max(v, x0 - eps), x0 + eps), 0, 1)


def step(x, x_old, g, x0, step_size, eps, a):
    """step_size: [B] tensor of x's dtype.  Returns (x_new, x) - the second is the new x_old."""
    s = step_size.view((-1,) + (1,) * (x.dim() - 1))
    z = project(x + s * torch.sign(g), x0, eps)
    x_new = project((x + (z - x) * a) + (x - x_old) * (1.0 - a), x0, eps)
    return x_new, x


class Book:
    """The per-sample scalars, kept as Python lists of 0-dim tensors / ints / bools."""

    def __init__(self, l0, pred0, eps):
        B = l0.shape[0]
        self.step = [torch.tensor(2.0 * eps, dtype=l0.dtype) for _ in range(B)]
        self.loss_best = [l0[b].clone() for b in range(B)]
        self.f_prev = [l0[b].clone() for b in range(B)]
        self.loss_best_last = [l0[b].clone() for b in range(B)]
        self.reduced_last = [True] * B
        self.inc = [0] * B
        self.robust = [bool(pred0[b]) for b in range(B)]

    def update(self, l, pred, k):
        """One iteration; k = window length when a checkpoint closes it, else 0.  Returns (improved, fooled, reduced, osc, noimp) lists."""
        B = l.shape[0]
        improved, fooled, reduced, oscs, noimps = [False] * B, [False] * B, [False] * B, [None] * B, [None] * B
        for b in range(B):
            if not bool(pred[b]):
                self.robust[b] = False
                fooled[b] = True
            if bool(l[b] > self.f_prev[b]):
                self.inc[b] += 1
            self.f_prev[b] = l[b].clone()
            if bool(l[b] > self.loss_best[b]):
                self.loss_best[b] = l[b].clone()
                improved[b] = True
            if k:
                osc = 4 * self.inc[b] <= 3 * k
                noimp = (not self.reduced_last[b]) and bool(self.loss_best_last[b] >= self.loss_best[b])
                red = osc or noimp
                oscs[b], noimps[b] = osc, noimp
                self.reduced_last[b] = red
                self.loss_best_last[b] = self.loss_best[b].clone()
                self.inc[b] = 0
                if red:
                    self.step[b] = self.step[b] / 2
                    reduced[b] = True
        return improved, fooled, reduced, oscs, noimps

    def snapshot(self):
        return dict(step=torch.stack(self.step), loss_best=torch.stack(self.loss_best), f_prev=torch.stack(self.f_prev),
                    loss_best_last=torch.stack(self.loss_best_last), inc=torch.tensor(self.inc), reduced_last=torch.tensor(self.reduced_last),
                    robust=torch.tensor(self.robust))


def apply_flags(x, g, x_best, g_best, x_best_adv, improved, fooled, reduced):
    """The tensor copies of steps (5), (7), (8), sample by sample, in that order; returns new tensors."""
    x, g, x_best, g_best, x_best_adv = x.clone(), g.clone(), x_best.clone(), g_best.clone(), x_best_adv.clone()
    for b in range(x.shape[0]):
        if fooled[b]:
            x_best_adv[b] = x[b]
        if improved[b]:
            x_best[b] = x[b]
            g_best[b] = g[b]
        if reduced[b]:
            x[b] = x_best[b]
            g[b] = g_best[b]
    return x, g, x_best, g_best, x_best_adv


def run(model, x0, x_init, y, n_iter, eps, kind, t=None):
    """The whole attack.  trace[0] is the start point, trace[i + 1] the state after iteration i; every entry holds x, x_old, g (after the
    copies), x_new / g_new (the iterate and its gradient before them), loss, pred, the scalars, and - for iterations - the flag lists."""
    def grad_at(xc):
        xc = xc.detach().clone().requires_grad_()
        z = model(xc)
        rows, pred = batch_loss(z, y, kind, t)
        (g,) = torch.autograd.grad(rows.sum(), [xc])
        return rows.detach(), g.detach(), pred

    sched = schedule(n_iter)
    x = x_init.detach().clone()
    l, g, pred = grad_at(x)
    book = Book(l, pred, eps)
    x_old, x_best, x_best_adv, g_best = x.clone(), x.clone(), x.clone(), g.clone()
    trace = [dict(x=x.clone(), x_old=x_old.clone(), g=g.clone(), x_new=x.clone(), g_new=g.clone(), loss=l.clone(), pred=pred.clone(),
                  x_best=x_best.clone(), g_best=g_best.clone(), x_best_adv=x_best_adv.clone(), **book.snapshot())]
    for i in range(n_iter):
        x, x_old = step(x, x_old, g, x0, torch.stack(book.step), eps, 1.0 if i == 0 else 0.75)
        l, g, pred = grad_at(x)
        x_new, g_new = x.clone(), g.clone()
        improved, fooled, reduced, osc, noimp = book.update(l, pred, sched.get(i, 0))
        x, g, x_best, g_best, x_best_adv = apply_flags(x, g, x_best, g_best, x_best_adv, improved, fooled, reduced)
        trace.append(dict(x=x.clone(), x_old=x_old.clone(), g=g.clone(), x_new=x_new, g_new=g_new, loss=l.clone(), pred=pred.clone(),
                          x_best=x_best.clone(), g_best=g_best.clone(), x_best_adv=x_best_adv.clone(), improved=improved, fooled=fooled,
                          reduced=reduced, osc=osc, noimp=noimp, k=sched.get(i, 0), **book.snapshot()))
    robust = torch.tensor(book.robust)
    x_adv = x0.clone()
    for b in range(x0.shape[0]):
        if not book.robust[b]:
            x_adv[b] = x_best_adv[b]
    return x_adv, robust, torch.stack(book.loss_best), trace
