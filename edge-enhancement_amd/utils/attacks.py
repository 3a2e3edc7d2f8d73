#!/usr/bin/env python
# -*- encoding: utf-8 -*-
"""Drop-in for the reference's utils/attacks.py: same names, argument order, defaults and side effects,
with the per-step element-wise work and the losses running as HIP kernels (libeeadv.so).

Reference lines are cited per function (paths relative to the reference root).  Differences, all
deliberate and documented in DESIGN.md:
  * `device='cuda'` strings hard-coded in the reference (attacks.py:250,291,311,383,406) follow the input
    tensor's device instead;
  * random starts are drawn on the device (Philox inside the init kernel) unless `noise=` is injected -
    device and host generators differ anyway, parity tests inject the noise;
  * CWLinfAttack(target=None) works (the reference raises TypeError at :152);
  * APGD / APGD_T, Square, FAB_T, FAB and APGD_Rand are additions: the reference runs them through the `autoattack` package (DESIGN.md
    sections 11 - 13 and 15);
  * CPU tensors are refused unless eeadv.runtime.allow_cpu_plumbing(True) was called (--no-cuda drivers).
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from eeadv import _native  # noqa: F401  (fails loudly at import when libeeadv.so is missing)
from eeadv import apgdstart, engine, fabstart, functional as EF, ops, runtime

_INF = float("inf")


# ---------------------------------------------------------------------------------------------------------
# shared pieces
# ---------------------------------------------------------------------------------------------------------
def _uniform_start(x0, eps, noise=None):
    """attacks.py:15-17: clamp(x0 + U(-eps, eps), 0, 1)."""
    if runtime.require_device(x0, "random start"):
        x0c = x0.contiguous()
        if noise is not None:
            return ops.pgd_init(x0c, noise.to(x0c.device, torch.float32).contiguous(), 0.0, 1.0)
        seed, off = runtime.philox_ticket(x0c.device, x0c.numel())
        return ops.pgd_init_rng(x0c, float(eps), 0, seed, off, 0.0, 1.0)
    nz = torch.zeros_like(x0).uniform_(-eps, eps) if noise is None else noise
    return torch.clamp(x0 + nz, 0, 1)


def _l2_norms(v):
    """||v[b]||_2 per sample [B] in v's dtype: the squares summed in float64, the root taken there, then cast."""
    return torch.sqrt((v.reshape(v.shape[0], -1).to(torch.float64) ** 2).sum(dim=1)).to(v.dtype)


def _l2_start(x0, eps, noise=None):
    """The published start of APGD in the L2 threat model: clamp(x0 + eps * n / (||n||_2 + 1e-12), 0, 1) with n a standard normal draw per
    element (`noise=` injects n) and the norm per sample.  Once per attack, in torch ops on whatever device x0 lives on."""
    n = torch.randn_like(x0) if noise is None else noise.to(x0.device, x0.dtype)
    tiny = torch.tensor(1e-12, dtype=torch.float32).to(x0.dtype)  # the constant is a float32 one in every dtype
    scale = (torch.tensor(eps, dtype=x0.dtype) / (_l2_norms(n) + tiny)).view((-1,) + (1,) * (x0.dim() - 1))
    return torch.clamp(x0 + n * scale, 0, 1)


def _randn_start(x0, noise=None, scale=0.001):
    """attacks.py:250 / :406: x_natural + 0.001 * randn (NOT clamped)."""
    if runtime.require_device(x0, "random start"):
        x0c = x0.contiguous()
        if noise is not None:
            nz = (scale * noise.to(x0c.device, torch.float32)).contiguous()
            return ops.pgd_init(x0c, nz, -_INF, _INF)
        seed, off = runtime.philox_ticket(x0c.device, x0c.numel())
        return ops.pgd_init_rng(x0c, scale, 1, seed, off, -_INF, _INF)
    nz = torch.randn(x0.shape, device=x0.device) if noise is None else noise
    return x0 + scale * nz


def _host_loop(model, x0, x, loss_fn, num_steps, step_size, eps, direction):
    """Plumbing path for CPU tensors (opt-in): the reference's own expressions, attacks.py:19-27."""
    for _ in range(num_steps):
        x.requires_grad_()
        with torch.enable_grad():
            loss = loss_fn(model(x))
        grad = torch.autograd.grad(loss, [x])[0]
        x = x.detach() + direction * step_size * torch.sign(grad.detach())
        x = torch.min(torch.max(x, x0 - eps), x0 + eps)
        x = torch.clamp(x, 0, 1)
    return x


def _loop(model, x0, x, spec, host_loss, num_steps, step_size, eps, direction=1):
    if runtime.require_device(x0, "PGD loop"):
        return engine.pgd_loop(model, x0, x, spec, num_steps, float(step_size), float(eps), direction)
    return _host_loop(model, x0, x, host_loss, num_steps, step_size, eps, direction)


def _random_targets(labels, nclass, device, label_offset=None):
    """attacks.py:38-40: target = fmod(y + randint(1, nclass), nclass)."""
    if label_offset is None:
        label_offset = torch.randint(low=1, high=nclass, size=labels.shape).to(device)
    return torch.fmod(labels + label_offset.to(labels.device), nclass)


# ---------------------------------------------------------------------------------------------------------
# Projected Gradient Descent (attacks.py:12-29)
# ---------------------------------------------------------------------------------------------------------
def PGD(model, args, inputs, targets, num_steps, step_size, noise=None):
    x0 = inputs.detach()
    x = _uniform_start(x0, args.epsilon, noise) if args.random else x0.clone()
    return _loop(model, x0, x, engine.LossSpec(engine.CE_SUM, targets),
                 lambda z: F.cross_entropy(z, targets, reduction='sum'), num_steps, step_size, args.epsilon)


# A targeted_PGD white-box attacker with random target label (attacks.py:33-56)
def targeted_PGD(model, args, inputs, labels, num_steps, step_size, nclass, device, noise=None, label_offset=None):
    x0 = inputs.detach()
    target_labels = _random_targets(labels, nclass, device, label_offset)
    x = _uniform_start(x0, args.epsilon, noise) if args.random else x0.clone()
    x = _loop(model, x0, x, engine.LossSpec(engine.CE_SUM, target_labels),
              lambda z: F.cross_entropy(z, target_labels, reduction='sum'), num_steps, step_size, args.epsilon, -1)
    return x, target_labels


def targeted_PGD_trick(model, args, inputs, labels, num_steps, step_size, nclass, device, noise=None, label_offset=None,
                       start_from_noise=None):
    """attacks.py:59-86: one Bernoulli per BATCH decides whether the random start is used (:69-71)."""
    x0 = inputs.detach()
    target_labels = _random_targets(labels, nclass, device, label_offset)
    x = x0.clone()
    if args.random:
        if start_from_noise is None:
            start_from_noise = bool(torch.gt(torch.rand([]), args.prob_start_from_clean))
        # x + 0 * noise then clamp == clamp(x): the clamp at :73 runs either way
        x = _uniform_start(x0, args.epsilon, noise) if start_from_noise else torch.clamp(x0, 0.0, 1.0)
    x = _loop(model, x0, x, engine.LossSpec(engine.CE_SUM, target_labels),
              lambda z: F.cross_entropy(z, target_labels, reduction='sum'), num_steps, step_size, args.epsilon, -1)
    return x, target_labels


# ---------------------------------------------------------------------------------------------------------
# APGD-CE and APGD-T (Croce & Hein 2020): the two gradient attacks of AutoAttack's `standard` version.  Not in the
# reference's utils/attacks.py - its drivers call the `autoattack` package for them.  Square, the black-box member, and FAB-T follow below;
# `eot_iter` averages every gradient over that many forwards (EOT), and APGD_Rand is the `rand` version's order, APGD-CE then APGD-DLR with
# EOT.  `norm="L2"` runs APGD (every loss, EOT included) in the L2 threat model of radius args.epsilon: the published
# L2 step and start, everything else shared.  EOT for APGD-T, Square and FAB-T, the L1 norm
# and restarts are NOT here, so the result is not an AutoAttack number.
# ---------------------------------------------------------------------------------------------------------
def _apgd_row_losses(z, y, loss, t=None):
    """Row losses [B] of logits [B,K] in z's dtype; classes ordered by value descending, ties to the lower index."""
    rows = torch.arange(z.shape[0], device=z.device)
    zy = z[rows, y]
    if loss == 'ce':
        return torch.logsumexp(z, dim=1) - zy
    K = z.shape[1]
    if K < (3 if loss == 'dlr' else 4):
        raise ValueError("the %s loss needs at least %d classes" % (loss, 3 if loss == 'dlr' else 4))
    zs, order = torch.sort(z, dim=1, descending=True, stable=True)
    tiny = torch.tensor(1e-12, dtype=torch.float32).to(z.dtype)  # the constant is a float32 one in every dtype
    if loss == 'dlr':
        o = torch.where(order[:, 0] == y, order[:, 1], order[:, 0])
        return -(zy - z[rows, o]) / ((zs[:, 0] - zs[:, 2]) + tiny)
    if loss == 'dlr_t':
        return -(zy - z[rows, t]) / ((zs[:, 0] - (zs[:, 2] + zs[:, 3]) * 0.5) + tiny)
    raise ValueError("APGD loss must be 'ce', 'dlr' or 'dlr_t', got %r" % (loss,))


def _check_norm(norm):
    return engine._check_norm(norm, engine.APGD_NORMS, "APGD")


def _apgd_grad_once(model, xc, y, loss, t):
    """(row losses, their input gradient, pred == y) of one forward/backward at xc: what both APGD host loops evaluate."""
    xc = xc.detach().requires_grad_()
    with torch.enable_grad():
        z = model(xc)
        rows = _apgd_row_losses(z, y, loss, t)
    g = torch.autograd.grad(rows.sum(), [xc])[0]
    first = torch.sort(z.detach(), dim=1, descending=True, stable=True)[1][:, 0]
    return rows.detach(), g.detach(), first == y


def _apgd_restart_kw(x0, n_restarts, seed):
    """What the APGD doors add to their engine / host calls: nothing for one restart (the calls stay the ones they always were, no ticket
    taken), else n_restarts and the seed - the caller's, or one drawn here, once for all target classes of a targeted attack."""
    n_restarts = int(n_restarts)
    if n_restarts < 1:
        raise ValueError("APGD needs n_restarts >= 1, got %d" % n_restarts)
    if n_restarts == 1:
        return {}
    if seed is None:
        seed = engine._drawn_seed(x0.device) if x0.is_cuda else int(torch.randint(0, 2 ** 62, (1,)).item())
    return dict(n_restarts=n_restarts, seed=int(seed))


def _apgd_host_restarts(run, x0, x, eps, metric, n_restarts, seed, noise, target_index):
    """The chain of both APGD host paths: restart 0 is run(x) - with n_restarts = 1 that is all, and no generator
    is touched - and restart r = 1 .. n_restarts - 1 is run(eeadv.apgdstart.start(x0, eps, t, metric)) on the whole batch, t being
    noise[r - 1] of the injected `noise` [n_restarts - 1, B, ...] or the host restatement of the kernel's draw under
    fabstart.seed_of(seed, target_index, r).  The flags are ANDed, the first fooling point is kept, the best loss is the largest."""
    n_restarts = int(n_restarts)
    if n_restarts < 1:
        raise ValueError("APGD needs n_restarts >= 1, got %d" % n_restarts)
    x_adv, robust, loss_best = run(x)
    if n_restarts == 1:
        return x_adv, robust, loss_best
    if noise is None and seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    B = x0.shape[0]
    shape = (-1,) + (1,) * (x0.dim() - 1)
    for r in range(1, n_restarts):
        if noise is not None:
            t = noise[r - 1]
        else:
            t = torch.from_numpy(apgdstart.draw(apgdstart.seed_of(seed, target_index, r), B, x0[0].numel() if B else 0, metric))
        xa, rb, lb = run(apgdstart.start(x0, eps, t.to(device=x0.device).reshape(x0.shape), metric))
        x_adv = torch.where((robust & ~rb).view(shape), xa, x_adv)
        robust = robust & rb
        loss_best = torch.where(lb > loss_best, lb, loss_best)
    return x_adv, robust, loss_best


def _apgd_host(model, x0, x, y, n_iter, eps, loss, t=None, trace=None, eot_iter=1, norm="Linf", n_restarts=1, seed=None, noise=None,
               target_index=0):
    """_apgd_host_run from x and - n_restarts > 1 - from the starts of the later restarts (_apgd_host_restarts), which share `trace`."""
    _check_norm(norm)
    return _apgd_host_restarts(lambda xs: _apgd_host_run(model, x0, xs, y, n_iter, eps, loss, t, trace, eot_iter, norm), x0, x, eps, norm,
                               n_restarts, seed, noise, target_index)


def _apgd_host_run(model, x0, x, y, n_iter, eps, loss, t=None, trace=None, eot_iter=1, norm="Linf"):
    """Plumbing path for CPU tensors (opt-in), the counterpart of _host_loop: the iteration of engine.apgd_loop in plain torch ops, in the
    input's dtype.  `trace`, a list, receives one dict of clones per iteration (the start point first).  eot_iter = E > 1: every gradient
    is the sum of E draws' gradients in draw order times 1/E (formed in the input's dtype), the loss the mean of their row losses summed
    in float64, pred the last draw's; the trace then also holds draw_loss / draw_g / draw_pred, stacked over the draws.  norm = "L2": the
    step is the one of csrc/ee_apgd_l2.hip in torch ops (each norm the root of the squares summed in float64, cast to the dtype; a sample
    whose gradient norm is not finite takes no gradient step) and the trace also holds norms [3, B]; everything else is shared."""
    E = int(eot_iter)
    if E < 1:
        raise ValueError("APGD needs eot_iter >= 1, got %d" % E)
    _check_norm(norm)
    last = {}

    def grad_at(xc):
        if E == 1:
            return grad_once(xc)
        draws = [grad_once(xc) for _ in range(E)]
        acc, lacc = draws[0][1], draws[0][0].to(torch.float64)
        for l_k, g_k, _ in draws[1:]:
            acc = acc + g_k
            lacc = lacc + l_k.to(torch.float64)
        last.update(draw_loss=torch.stack([d[0] for d in draws]), draw_g=torch.stack([d[1] for d in draws]),
                    draw_pred=torch.stack([d[2] for d in draws]))
        return (lacc / E).to(draws[0][0].dtype), acc * (torch.ones((), dtype=acc.dtype) / E), draws[-1][2]

    def grad_once(xc):
        return _apgd_grad_once(model, xc, y, loss, t)

    def proj(v):
        return torch.clamp(torch.min(torch.max(v, x0 - eps), x0 + eps), 0, 1)

    shape = (-1,) + (1,) * (x0.dim() - 1)

    def step_linf(x, x_old, g, step, a):
        z = proj(x + step.view(shape) * torch.sign(g))
        return proj((x + (z - x) * a) + (x - x_old) * (1.0 - a))

    def step_l2(x, x_old, g, step, a):
        tiny = torch.tensor(1e-12, dtype=torch.float32).to(x.dtype)  # the constant is a float32 one in every dtype
        radius = torch.tensor(eps, dtype=x.dtype)
        ng = _l2_norms(g)
        sg = step / (ng + tiny)
        z = torch.where(torch.isfinite(ng).view(shape), x + g * sg.view(shape), x)
        d = z - x0
        n1 = _l2_norms(d)
        z = torch.clamp(x0 + d * (torch.minimum(radius, n1) / (n1 + tiny)).view(shape), 0, 1)
        m = (x + (z - x) * a) + (x - x_old) * (1.0 - a)
        d = m - x0
        n2 = _l2_norms(d)
        last.update(norms=torch.stack([ng, n1, n2]))
        return torch.clamp(x0 + d * (torch.minimum(radius, n2) / (n2 + tiny)).view(shape), 0, 1)

    step_fn = step_l2 if norm == "L2" else step_linf
    sched = engine.apgd_schedule(n_iter)
    x = x.detach()
    l, g, pred = grad_at(x)
    step = torch.full_like(l, 2.0 * eps)
    loss_best, f_prev, loss_best_last = l.clone(), l.clone(), l.clone()
    x_best, x_best_adv, x_old, g_best = x.clone(), x.clone(), x.clone(), g.clone()
    reduced_last = torch.ones_like(pred)
    inc = torch.zeros_like(y)
    robust = pred.clone()

    def note(**kw):
        if trace is not None:
            kw.update(last)
            kw.update(x=x, x_old=x_old, g=g, loss=l, pred=pred, step=step, loss_best=loss_best, f_prev=f_prev, loss_best_last=loss_best_last,
                      inc=inc, reduced_last=reduced_last, robust=robust, x_best=x_best, g_best=g_best, x_best_adv=x_best_adv)
            trace.append({k: v.clone() for k, v in kw.items()})
    note()
    for i in range(n_iter):
        a = 1.0 if i == 0 else 0.75
        x_new = step_fn(x, x_old, g, step, a)
        x_old, x = x, x_new
        l, g, pred = grad_at(x)
        fooled = ~pred
        robust = robust & pred
        x_best_adv = torch.where(fooled.view(shape), x, x_best_adv)
        inc = inc + (l > f_prev).to(inc.dtype)
        f_prev = l.clone()
        improved = l > loss_best
        loss_best = torch.where(improved, l, loss_best)
        x_best = torch.where(improved.view(shape), x, x_best)
        g_best = torch.where(improved.view(shape), g, g_best)
        reduced = torch.zeros_like(pred)
        k = sched[i]
        if k:
            osc = 4 * inc <= 3 * k
            noimp = ~reduced_last & (loss_best_last >= loss_best)
            reduced = osc | noimp
            reduced_last, loss_best_last, inc = reduced.clone(), loss_best.clone(), torch.zeros_like(inc)
            step = torch.where(reduced, step / 2, step)
            x = torch.where(reduced.view(shape), x_best, x)
            g = torch.where(reduced.view(shape), g_best, g)
        note(improved=improved, fooled=fooled, reduced=reduced)
    return torch.where(robust.view(shape), x0, x_best_adv), robust, loss_best


def APGD(model, args, inputs, targets, num_steps, loss='ce', y_target=None, noise=None, eot_iter=1, norm="Linf", n_restarts=1, seed=None,
         target_index=0):
    """One APGD run (norm 'Linf' or 'L2', radius args.epsilon, num_steps iterations) on loss 'ce', 'dlr' or 'dlr_t' (targeted at `y_target`).  Returns
    (x_adv, robust): the inputs, with every sample that some iterate fooled replaced by such an iterate, and the [B] bool flags of the samples
    that stayed correctly classified throughout.  The start point is the project's uniform start, clamp(x0 + U(-eps, eps), 0, 1) (`noise=`
    injects the draw); the public implementation rescales each sample's draw to the full radius first - that normalisation is deliberately
    left out.  The model runs in the mode the caller left it in.  On the device the targeted DLR denominator is formed as the mean of
    z_p1 - z_p3 and z_p1 - z_p4 (csrc/ee_apgd.hip: no cancellation against a rounded sum); the host path below keeps
    z_p1 - (z_p3 + z_p4)/2, so an fp32 host run and a device run differ in the last bits of the `dlr_t` loss.  eot_iter = E > 1 (for a
    defence that redraws at every forward): every gradient is the mean over E forwards, the loss the run keeps books on is the mean of
    their row losses, and a sample counts as fooled when the last of the E draws of some iterate misclassifies it.
    norm = "L2": the ball is the L2 ball, the step the published L2 step (csrc/ee_apgd_l2.hip; a rescale onto the ball followed by the
    clamp, not the exact projection onto ball and box) and the start the published one, clamp(x0 + eps n / ||n||_2, 0, 1) - `noise=` then
    injects the standard normal draw n.  n_restarts > 1: restart 0 is the run above; every
    later restart runs the same iterations on the whole batch from a fresh draw of the same start distribution, made on the device under
    eeadv.fabstart.seed_of(seed, target_index, r) (seed None draws one); a sample counts as fooled if any restart fooled it and the first
    restart that did supplies its point.  `noise=` injects restart 0's draw only."""
    eot_iter = int(eot_iter)
    if eot_iter < 1:
        raise ValueError("APGD needs eot_iter >= 1, got %d" % eot_iter)
    _check_norm(norm)
    x0 = inputs.detach()
    eps = float(args.epsilon)
    x = _uniform_start(x0, eps, noise) if norm == "Linf" else _l2_start(x0, eps, noise)
    kw = {} if norm == "Linf" else {"norm": norm}  # a Linf run makes exactly the calls made before the parameter existed
    rkw = _apgd_restart_kw(x0, n_restarts, seed)  # and so does a run with one restart
    if rkw:
        kw = dict(kw, target_index=int(target_index), **rkw)
    if runtime.require_device(x0, "APGD"):
        x_adv, robust, _ = engine.apgd_loop(model, x0, x, targets, num_steps, eps, loss, y_target, eot_iter=eot_iter, **kw)
    else:
        x_adv, robust, _ = _apgd_host(model, x0, x, targets, num_steps, eps, loss, y_target, eot_iter=eot_iter, **kw)
    return x_adv, robust


def _first_fooling(x0, runs):
    """Combines attacks of one batch, taken in order from `runs` (an iterable of (x_adv, robust)): the flags ANDed and, per sample, the
    first fooling point."""
    x_adv = x0.clone()
    robust = torch.ones(x0.shape[0], dtype=torch.bool, device=x0.device)
    for xa, rb in runs:
        x_adv = torch.where((robust & ~rb).view((-1,) + (1,) * (x0.dim() - 1)), xa, x_adv)
        robust = robust & rb
    return x_adv, robust


def _restarts_kw(n_restarts, seed=None):
    """The keywords the composites hand on to APGD / APGD_L1: none for one restart, as _norm_kw hands on none for Linf."""
    if int(n_restarts) == 1:
        return {}
    return {"n_restarts": int(n_restarts)} if seed is None else {"n_restarts": int(n_restarts), "seed": seed}


def _norm_kw(norm):
    """The keyword the composites hand on to APGD: none for Linf, so that a Linf call is the call made before the parameter existed."""
    return {} if _check_norm(norm) == "Linf" else {"norm": norm}


def APGD_Rand(model, args, inputs, targets, num_steps, eot_iter=20, nclass=None, noise=None, norm="Linf", n_restarts=1, seed=None):
    """The order of the public ensemble's `rand` version, for defences that redraw at every forward: APGD-CE, then APGD-DLR (the untargeted
    DLR loss), each one run of num_steps iterations with every gradient averaged over eot_iter forwards, each on the whole batch.  Returns
    (x_adv, robust) with the flags ANDed and, per sample, the first fooling point - as APGD_T combines its runs.  The DLR loss reads the three
    largest logits: `nclass` (default: read off one clean forward) must be at least 3.  norm: 'Linf' or 'L2', for both runs.  n_restarts and seed as in
    APGD, for both runs (seed None: each run draws its own)."""
    eot_iter = int(eot_iter)
    if eot_iter < 1:
        raise ValueError("APGD_Rand needs eot_iter >= 1, got %d" % eot_iter)
    kw = dict(_norm_kw(norm), **_restarts_kw(n_restarts, seed))
    x0 = inputs.detach()
    if nclass is None:
        with torch.no_grad():
            nclass = model(x0).shape[1]
    if int(nclass) < 3:
        raise ValueError("APGD_Rand runs APGD-DLR, whose loss is normalised by the spread of the three largest logits: it needs at least 3 "
                         "classes and this model has %d (MNIST's 10 are enough; only the targeted DLR loss of APGD-T needs 4)" % int(nclass))
    return _first_fooling(x0, (APGD(model, args, inputs, targets, num_steps, loss, None, noise, eot_iter, **kw) for loss in ('ce', 'dlr')))


# ---------------------------------------------------------------------------------------------------------
# APGD in the L1 threat model (Croce & Hein 2021, "Mind the box"): doors of their own - APGD(norm="L1") stays refused.  One run, no
# momentum, the sparse sign step, the exact projection onto ball and box, the sparsity / step-size checkpoints.
# The large-radius warm-up, EOT and L1 inside Cascade / Rand are NOT here; restarts: DESIGN.md section 24 (L1 Square: Square_L1 below, section 21).
# ---------------------------------------------------------------------------------------------------------
def _f32c(v, dtype):
    """The float32 constant v in `dtype`: the constants of the L1 run are float32 ones in every dtype."""
    return torch.tensor(v, dtype=torch.float32).to(dtype)


def _l1_multiplier(a, lo, eps):
    """lambda of one sample as a Python float: a, lo 1-D float64 tensors (finite, 0 <= lo <= a).  The segment is located on sorted
    breakpoints with cumulative sums, confirmed with exactly summed h (math.fsum), and solved with an exactly summed numerator."""
    import math

    def h(t):
        return math.fsum(a.tolist() + (-torch.minimum(torch.clamp(lo, min=t), a)).tolist())

    if h(0.0) <= eps:
        return 0.0
    bp = torch.unique(torch.cat([lo, a, a.new_zeros(1)]))  # sorted
    a_s, lo_s = torch.sort(a)[0], torch.sort(lo)[0]
    ca, cl = torch.cat([a.new_zeros(1), torch.cumsum(a_s, 0)]), torch.cat([a.new_zeros(1), torch.cumsum(lo_s, 0)])
    na = torch.searchsorted(a_s, bp, right=True)    # a_i <= t
    nl = torch.searchsorted(lo_s, bp, right=True)   # lo_i <= t
    cut = ca[na] + (cl[-1] - cl[nl]) + bp * (nl - na).to(bp.dtype)
    above = (ca[-1] - cut) > eps
    k = int(above.nonzero().max()) if bool(above.any()) else 0
    while k + 1 < bp.numel() - 1 and h(float(bp[k + 1])) > eps:  # the cumulative sums round: settle the segment exactly
        k += 1
    while k > 0 and not h(float(bp[k])) > eps:
        k -= 1
    t = float(bp[k])
    act, fixed = (lo <= t) & (a > t), (lo > t) & (a > t)
    n = int(act.sum())
    if n == 0:
        return float(bp[k + 1])
    return math.fsum(a[fixed].tolist() + (-lo[fixed]).tolist() + a[act].tolist() + [-float(eps)]) / n


def _l1_project(u, x0, eps):
    """P(u): the Euclidean projection onto {z : ||z - x0||_1 <= eps} n [0,1]^D per sample, in u's dtype, as csrc/ee_apgd_l1.hip states it.
    Returns (z, lam [B]).  A sample whose u - x0 is not finite is returned as x0."""
    B = u.shape[0]
    w = (u - x0).reshape(B, -1)
    uf, cf = u.reshape(B, -1), x0.reshape(B, -1)
    a = w.abs()
    lo = torch.minimum(torch.clamp(-torch.minimum(1 - uf, uf), min=0), a)
    bad = ~torch.isfinite(w).all(dim=1)
    lam = torch.zeros(B, dtype=u.dtype)
    for b in range(B):
        if not bool(bad[b]):
            lam[b] = _l1_multiplier(a[b].to(torch.float64), lo[b].to(torch.float64), float(eps))
    cut = torch.minimum(torch.maximum(lam.view(-1, 1), lo), a)
    z = torch.clamp(cf + torch.sign(w) * (a - cut), 0, 1)
    z = torch.where(bad.view(-1, 1), cf, z)
    return z.reshape(u.shape), lam


def _l1_step(x, g, x0, step, topk, eps):
    """The sparse sign step and the projection of an L1 run in torch ops, in x's dtype.  Returns (x_new, info)."""
    B = x.shape[0]
    D = x[0].numel()
    dt = x.dtype
    gf, xf = g.reshape(B, -1), x.reshape(B, -1)
    v = torch.floor((1 - topk) * D)
    j = torch.where(v >= 0, torch.clamp(v, max=D - 1), torch.zeros_like(v)).to(torch.int64)  # a NaN selects 0
    ab = gf.abs()
    bits = ab.view(torch.int32 if dt == torch.float32 else torch.int64)  # non-negative patterns: the integer order is the kernel's
    tau_bits = torch.sort(bits, dim=1)[0].gather(1, j.view(-1, 1))
    mask = bits >= tau_bits
    s = torch.sign(torch.nan_to_num(gf, nan=0.0))
    m = (mask & (s != 0)).sum(dim=1)
    sg = step / (m.to(dt) + _f32c(1e-10, dt))
    finite = torch.isfinite(gf).all(dim=1)
    u = torch.where(mask & (s != 0) & finite.view(-1, 1), xf + sg.view(-1, 1) * s, xf)
    z, lam = _l1_project(u.reshape(x.shape), x0, eps)
    return z, dict(j=j, tau=tau_bits.view(dt).reshape(B), m=m, lam=lam, u=u.reshape(x.shape))


def _apgd_l1_host(model, x0, x_init, y, n_iter, eps, loss, t=None, trace=None, n_restarts=1, seed=None, noise=None, target_index=0):
    """_apgd_l1_host_run from x_init and - n_restarts > 1 - from the unprojected starts x0 + n of the later restarts
    (_apgd_host_restarts), which share `trace`."""
    return _apgd_host_restarts(lambda xs: _apgd_l1_host_run(model, x0, xs, y, n_iter, eps, loss, t, trace), x0, x_init, eps, "L1",
                               n_restarts, seed, noise, target_index)


def _apgd_l1_host_run(model, x0, x_init, y, n_iter, eps, loss, t=None, trace=None):
    """Plumbing path for CPU tensors (opt-in): the iteration of engine.apgd_l1_loop in plain torch ops, in the input's dtype, with
    sort-based selection and projection.  x_init is the unprojected start x0 + n.  `trace`, a list, receives one dict of clones per
    iteration (the start point first)."""
    if loss not in ops.APGD_KINDS:
        raise ValueError("APGD loss must be one of %s, got %r" % (sorted(ops.APGD_KINDS), loss))
    sched = engine.apgd_l1_schedule(n_iter)
    dt = x0.dtype
    B, D = x0.shape[0], x0[0].numel()
    shape = (-1,) + (1,) * (x0.dim() - 1)

    def grad_at(xc):
        return _apgd_grad_once(model, xc, y, loss, t)

    radius = torch.tensor(eps, dtype=dt)
    x, lam0 = _l1_project(x_init.detach(), x0, eps)
    l, g, pred = grad_at(x)
    step = torch.full_like(l, eps)
    topk = torch.full_like(l, 1.0) * _f32c(0.2, dt)
    sp_old = torch.full((B,), D, dtype=torch.int64)
    loss_best, robust = l.clone(), pred.clone()
    x_best, x_best_adv, g_best = x.clone(), x.clone(), g.clone()

    def note(**kw):
        if trace is not None:
            kw.update(x=x, g=g, loss=l, pred=pred, step=step, topk=topk, sp_old=sp_old, loss_best=loss_best, robust=robust, x_best=x_best,
                      g_best=g_best, x_best_adv=x_best_adv)
            trace.append({k: v.clone() for k, v in kw.items()})
    note(lam=lam0)
    for i in range(n_iter):
        x, info = _l1_step(x, g, x0, step, topk, eps)
        l, g, pred = grad_at(x)
        x_new, g_new = x, g
        fooled = ~pred
        robust = robust & pred
        x_best_adv = torch.where(fooled.view(shape), x, x_best_adv)
        improved = l > loss_best
        loss_best = torch.where(improved, l, loss_best)
        x_best = torch.where(improved.view(shape), x, x_best)
        g_best = torch.where(improved.view(shape), g, g_best)
        reduced = torch.zeros_like(pred)
        sp = torch.zeros_like(sp_old)
        if sched[i]:
            sp = (x_best != x0).reshape(B, -1).sum(dim=1)
            reduced = (sp.to(dt) / sp_old.to(dt)) < _f32c(0.95, dt)
            topk = sp.to(dt) / torch.tensor(D, dtype=dt) / _f32c(1.5, dt)
            step = torch.minimum(torch.maximum(torch.where(reduced, radius, step / _f32c(1.5, dt)), radius / _f32c(10.0, dt)), radius)
            sp_old = sp
            x = torch.where(reduced.view(shape), x_best, x)
            g = torch.where(reduced.view(shape), g_best, g)
        note(improved=improved, fooled=fooled, reduced=reduced, sp=sp, x_new=x_new, g_new=g_new, **info)
    return torch.where(robust.view(shape), x0, x_best_adv), robust, loss_best


def APGD_L1(model, args, inputs, targets, num_steps, loss='ce', y_target=None, noise=None, n_restarts=1, seed=None, target_index=0):
    """One APGD run in the L1 threat model (radius args.epsilon, num_steps iterations) on loss 'ce', 'dlr' or 'dlr_t' (targeted at
    `y_target`).  Returns (x_adv, robust) as APGD does.  The start is P(x0 + n), n a standard normal draw per element (`noise=` injects n)
    and P the exact projection onto the L1 ball intersected with the box; the step is the sparse sign step followed by P; the
    checkpoints adapt a per-sample sparsity and step size.  The public ensemble's large-radius warm-up
    (3 eps -> 2 eps -> eps) and EOT are not built.  n_restarts, seed and target_index as in APGD: restart r >= 1
    starts at P(x0 + n) for a fresh n drawn on the device."""
    x0 = inputs.detach()
    eps = float(args.epsilon)
    n = torch.randn_like(x0) if noise is None else noise.to(x0.device, x0.dtype)
    x_init = x0 + n
    rkw = _apgd_restart_kw(x0, n_restarts, seed)  # empty for one restart: the calls below are then the ones they always were
    if rkw:
        rkw = dict(rkw, target_index=int(target_index))
    if runtime.require_device(x0, "APGD_L1"):
        x_adv, robust, _ = engine.apgd_l1_loop(model, x0, x_init, targets, num_steps, eps, loss, y_target, **rkw)
    else:
        x_adv, robust, _ = _apgd_l1_host(model, x0, x_init, targets, num_steps, eps, loss, y_target, **rkw)
    return x_adv, robust


def APGD_T_L1(model, args, inputs, targets, num_steps, nclass, n_target_classes=9, noise=None, order=None, n_restarts=1, seed=None):
    """Targeted L1-APGD on the DLR loss: one run per target class as APGD_T takes them, each on the whole batch; the flags are ANDed over
    the runs and, per sample, the first fooling point is kept.  n_restarts and seed as in APGD_T."""
    x0 = inputs.detach()
    n_t = min(int(n_target_classes), int(nclass) - 1)
    order = _class_order(model, x0, n_t, "APGD_T_L1", order)
    rkw = _apgd_restart_kw(x0, n_restarts, seed)  # one seed for all target classes; class j keys its draws by target_index = j
    return _first_fooling(x0, (APGD_L1(model, args, inputs, targets, num_steps, 'dlr_t', order[:, j].contiguous(), noise,
                                       **(dict(rkw, target_index=j) if rkw else {})) for j in range(1, n_t + 1)))


def _class_order(model, x0, n_t, what, order=None):
    """The first n_t + 1 classes of the clean logits [B, n_t + 1] int64, by value descending, ties to the lower index; `order`, the same thing
    computed by the caller (the cascade takes it from its own clean forward), is checked and returned without a forward."""
    on_dev = runtime.require_device(x0, what)
    if order is not None:
        if tuple(order.shape) != (x0.shape[0], n_t + 1) or order.dtype != torch.int64:
            raise ValueError("%s: order must be int64 of shape %s, got %s %s" % (what, (x0.shape[0], n_t + 1), order.dtype, tuple(order.shape)))
        return order
    with torch.no_grad():
        z = model(x0)
    if on_dev:
        return ops.topk(z.detach().float().contiguous(), None, n_t + 1)[0]
    return torch.sort(z, dim=1, descending=True, stable=True)[1][:, :n_t + 1]


def APGD_T(model, args, inputs, targets, num_steps, nclass, n_target_classes=9, noise=None, order=None, norm="Linf", n_restarts=1, seed=None):
    """Targeted APGD on the DLR loss: one run per target class, the 2nd ... (n_target_classes + 1)-th class of the clean logits (at most
    nclass - 1 of them), each on the whole batch - samples fooled by an earlier target are carried along, which keeps one shape (one captured
    graph) for all runs.  Returns (x_adv, robust) with the flags ANDed over the runs and, per sample, the first fooling point.  `order`
    [B, n_t + 1]: the class order of the clean logits if the caller has it already - the clean forward is then skipped.  norm: 'Linf' or
    'L2', for every run; the class order does not know the norm.  n_restarts > 1: every target class runs its
    restarts, restart r >= 1 of the j-th class from the draw keyed by eeadv.fabstart.seed_of(seed, j, r); seed None draws one, once."""
    kw = _norm_kw(norm)
    x0 = inputs.detach()
    n_t = min(int(n_target_classes), int(nclass) - 1)
    order = _class_order(model, x0, n_t, "APGD_T", order)
    rkw = _apgd_restart_kw(x0, n_restarts, seed)  # one seed for all target classes; class j keys its draws by target_index = j
    return _first_fooling(x0, (APGD(model, args, inputs, targets, num_steps, 'dlr_t', order[:, j].contiguous(), noise, **kw,
                                    **(dict(rkw, target_index=j) if rkw else {})) for j in range(1, n_t + 1)))


# ---------------------------------------------------------------------------------------------------------
# Square (Andriushchenko et al. 2020, Linf; norm="L2": its L2 form): the black-box member of AutoAttack's `standard` version - score-based random search on the
# margin loss, p_init = 0.8 with the rescaled schedule, one run, no EOT.  Built from the published description;
# every sample draws a window of its own (the paper's form), so a sample's trajectory does not depend on who shares its batch.
# ---------------------------------------------------------------------------------------------------------
def _square_margin(z, y):
    """margin [B] = z_y - max_{j != y} z_j in z's dtype; NaN for a row with a NaN logit or a label outside [0, K)."""
    K = z.shape[1]
    valid = (y >= 0) & (y < K)
    yc = y.clamp(0, K - 1)
    zy = z.gather(1, yc.view(-1, 1)).squeeze(1)
    other = z.masked_fill(F.one_hot(yc, K).bool(), -_INF).max(dim=1)[0]
    bad = torch.isnan(z).any(dim=1) | ~valid
    return torch.where(bad, torch.full_like(zy, float("nan")), zy - other)


def _check_square_norm(norm):
    return engine._check_norm(norm, engine.SQUARE_NORMS, "Square")


def _square_norms(v, planes, power):
    """||v[b]||_power [B] (planes: ||v[b, c]||_power [B, C]), power 1 or 2, in v's dtype for the L1 / L2 Square host paths: the |values| or
    the squares summed in float64 - then the root, for 2 - rounded once.  Those terms of float32 (and narrower) values are exact there and
    torch's sum is then far inside the last bit of the result; float64 values are summed without error (math.fsum) - their squares as
    the products of halves, which are exact - so that a float64 run, what the tests compare bit for bit, has norms rounded once as well."""
    import math
    rows = v.reshape(v.shape[0] * v.shape[1] if planes else v.shape[0], -1).detach().cpu()
    if v.dtype == torch.float64:
        a = rows.numpy()
        terms = np.abs(a)
        if power == 2:
            c = a * 134217729.0  # Veltkamp: hi holds the upper 26 bits
            hi = c - (c - a)
            lo = a - hi
            terms = np.concatenate([hi * hi, 2.0 * hi * lo, lo * lo], axis=1)
        sums = np.array([math.fsum(r) for r in terms.tolist()], dtype=np.float64)
    else:
        rows = rows.to(torch.float64)
        sums = (rows ** 2 if power == 2 else rows.abs()).sum(dim=1).numpy()
    out = torch.from_numpy(np.sqrt(sums) if power == 2 else sums).to(v.dtype).to(v.device)
    return out.view(v.shape[0], v.shape[1]) if planes else out



def _square_tiles(x0, seed, ids):
    """d, the tiled pattern the L2 and L1 starts share: +-eta(s0) per tile and channel, transposed by the tile's coin,
    0 outside the tiling."""
    from eeadv import sqatk
    B, C, H, W = x0.shape
    s0 = sqatk.start_size(H, W)
    nh, nw = H // s0, W // s0
    oh, ow = (H - nh * s0) // 2, (W - nw * s0) // 2
    bits, tr = (torch.from_numpy(a) for a in sqatk.tiles(seed, ids, nh * nw))
    eta0 = torch.from_numpy(sqatk.eta(s0)).to(x0.dtype)
    one = torch.ones((), dtype=x0.dtype)
    cc = torch.arange(C).view(1, C)
    d = torch.zeros(x0.shape, dtype=x0.dtype)
    for a in range(nh):
        for b in range(nw):
            k = a * nw + b
            block = torch.where(tr[:, k].bool().view(B, 1, 1), eta0.t().unsqueeze(0), eta0.unsqueeze(0))
            sign = torch.where(((bits[:, k].view(B, 1) >> cc) & 1).bool(), one, -one)
            d[:, :, oh + a * s0:oh + (a + 1) * s0, ow + b * s0:ow + (b + 1) * s0] = sign.view(B, C, 1, 1) * block.view(B, 1, s0, s0)
    return d.to(x0.device)


def _square_l2_start(x0, eps, seed, ids):
    """The tiled start of an L2 run: (x_best, n0)."""
    B = x0.shape[0]
    d = _square_tiles(x0, seed, ids)
    tiny = torch.tensor(1e-12, dtype=torch.float32).to(x0.dtype)  # the constant is a float32 one in every dtype
    n0 = _square_norms(d, False, 2)
    q = torch.tensor(eps, dtype=x0.dtype) / (n0 + tiny)
    return torch.clamp(x0 + d * q.view(B, 1, 1, 1), 0, 1), n0


def _square_windows(x0, seed, i, ids, s):
    """(in1, in2, signed) of proposal i for every sample, as the L2 and L1 proposals share them: the masks [B,1,H,W] of the two windows and
    +-eta(s) (transposed by the coin, signed per channel) laid on window 1, [B,C,H,W]."""
    from eeadv import sqatk
    B, C, H, W = x0.shape
    dt = x0.dtype
    vh, vw, bits, tr = sqatk.windows_l2(seed, i, ids, H, W, s)
    vh2, vw2 = sqatk.windows2(seed, i, ids, H, W, s)
    eta_s = torch.from_numpy(sqatk.eta(s)).to(dt)
    pattern = torch.zeros((B, H, W), dtype=dt)
    for b in range(B):
        pattern[b, vh[b]:vh[b] + s, vw[b]:vw[b] + s] = eta_s.t() if tr[b] else eta_s
    hh, ww, cc = torch.arange(H).view(1, H), torch.arange(W).view(1, W), torch.arange(C).view(1, C)

    def inside(ah, aw):
        ah, aw = torch.from_numpy(ah).view(B, 1), torch.from_numpy(aw).view(B, 1)
        return (((hh >= ah) & (hh < ah + s)).view(B, 1, H, 1) & ((ww >= aw) & (ww < aw + s)).view(B, 1, 1, W)).to(x0.device)

    one = torch.ones((), dtype=dt)
    sign = torch.where(((torch.from_numpy(bits).view(B, 1) >> cc) & 1).bool(), one, -one).view(B, C, 1, 1).to(x0.device)
    return inside(vh, vw), inside(vh2, vw2), pattern.to(x0.device).view(B, 1, H, W) * sign


def _square_propose(x_best, x0, seed, i, ids, s, power, scale, tail):
    """Proposal i of an L2 or L1 run for every sample (DESIGN.md sections 18 and 21), written once up to the rescaled window 1: the norms
    are _square_norms' of `power`, scale(n_img, n_un) [B] is the threat model's rule, and tail(delta) = (x_new, the rows of norms that
    follow n_img and n_un, whatever else the caller returns) takes the proposed difference to a point.  Returns (x_new, norms [.. + 2C, B])
    and the tail's extras."""
    B, C, H, W = x0.shape
    dt = x0.dtype
    in1, in2, signed = _square_windows(x0, seed, i, ids, s)
    zero = torch.zeros((), dtype=dt)
    tiny = torch.tensor(1e-12, dtype=torch.float32).to(dt)  # the constant is a float32 one in every dtype
    delta = x_best - x0
    n_img = _square_norms(delta, False, power)
    n_un = _square_norms(torch.where(in1 | in2, delta, zero), False, power)
    n_w = _square_norms(torch.where(in1, delta, zero), True, power)
    new = torch.where(in1, signed + delta / (tiny + n_w).view(B, C, 1, 1), zero)
    n_new = _square_norms(new, True, power)
    new = new / (tiny + n_new).view(B, C, 1, 1) * scale(n_img, n_un).view(B, 1, 1, 1)
    delta = torch.where(in1, new, torch.where(in2, zero, delta))
    x_new, head, *more = tail(delta)
    return (x_new, torch.cat([torch.stack([n_img, n_un] + head), n_w.t(), n_new.t()]), *more)


def _square_l2_propose(x_best, x0, eps, seed, i, ids, s):
    """Proposal i of an L2 run for every sample: (x_new, norms [3 + 2C, B])."""
    B, C = x0.shape[:2]
    e = torch.tensor(eps, dtype=x0.dtype)
    tiny = torch.tensor(1e-12, dtype=torch.float32).to(x0.dtype)

    def scale(n_img, n_un):
        room = torch.clamp(e * e - n_img * n_img, min=0) / C + n_un * n_un
        return torch.from_numpy(np.sqrt(room.cpu().numpy())).to(x0.device)  # the root rounded once: torch's vectorised CPU sqrt may miss the last bit

    def tail(delta):  # the whole delta rescaled to the sphere
        n_d = _square_norms(delta, False, 2)
        return torch.clamp(x0 + delta / (tiny + n_d).view(B, 1, 1, 1) * e, 0, 1), [n_d]

    return _square_propose(x_best, x0, seed, i, ids, s, 2, scale, tail)


def _square_l1_propose(x_best, x0, eps, eps_p, seed, i, ids, s):
    """Proposal i of an L1 run for every sample: (x_new, norms [2 + 2C, B], lam [B])."""
    C = x0.shape[1]
    e = torch.tensor(eps, dtype=x0.dtype)

    def scale(n_img, n_un):
        return torch.clamp(e - n_img, min=0) / torch.tensor(C, dtype=x0.dtype) + n_un

    def tail(delta):  # the exact projection onto the eps_p ball and the box
        x_new, lam = _l1_project(x0 + delta, x0, eps_p)
        return x_new, [], lam

    return _square_propose(x_best, x0, seed, i, ids, s, 1, scale, tail)


class _SquareQueries:
    """What a host run keeps between its forwards, whatever the threat model: the smallest accepted margin, the query count and the
    accept rule of ee_sqatk_margin_f32.  `trace`, a list, receives {"margin", "flags"} (and `extra`) of every forward."""

    def __init__(self, model, x0, y, trace=None):
        B = x0.shape[0]
        self.model, self.y, self.trace = model, y, trace
        self.margin_min = torch.full((B,), _INF, dtype=x0.dtype, device=x0.device)
        self.queries = torch.zeros(B, dtype=torch.int32, device=x0.device)

    def active(self):
        return ~(self.margin_min <= 0)

    def query(self, x_new, x_best, extra=None):
        """One forward on x_new: the new x_best."""
        with torch.no_grad():
            m = _square_margin(self.model(x_new), self.y)
        active = self.active()
        accept = active & (m < self.margin_min)
        self.margin_min = torch.where(accept, m, self.margin_min)
        self.queries = self.queries + active.to(torch.int32)
        if self.trace is not None:
            self.trace.append(dict(extra or {}, margin=m.clone(), flags=accept.clone()))
        return torch.where(accept.view(-1, 1, 1, 1), x_new, x_best)

    def run(self, x_start, kept, sizes, propose, early_exit):
        """The host loop of a tiled-start run: the forward on x_start, then proposal i = 0, 1, ... of edge sizes[i] while a sample is active.
        propose(x_best, i, s) = (the proposal of every sample, {name: per-sample rows [.., B]}); the trace keeps x_new and those rows -
        zeros for a sample that made no proposal and kept x_new = x_best - as it keeps `kept` of the start.  Returns x_best."""
        x_best = self.query(x_start, x_start, dict({"x_new": x_start.clone()}, **kept))
        for i, s in enumerate(sizes):
            active = self.active()
            if early_exit and not bool(active.any()):
                break
            prop, rows = propose(x_best, i, s)
            x_new = torch.where(active.view(-1, 1, 1, 1), prop, x_best)
            rows = {k: torch.where(active, v, torch.zeros((), dtype=v.dtype)) for k, v in rows.items()}
            x_best = self.query(x_new, x_best, dict({"x_new": x_new.clone()}, **rows))
        return x_best


def _square_host(model, x0, y, n_queries, eps, seed, trace=None, ids=None, early_exit=True, norm="Linf"):
    """Plumbing path for CPU tensors (opt-in): the iteration of engine.square_loop in plain torch ops, in the input's dtype, with the
    kernels' draws (eeadv.sqatk: the same Philox key, counters and stream ids).  `ids` [B]: the batch index each sample draws under
    (default 0 .. B-1).  Returns (x_best, margin_min, queries); `trace`, a list, receives {"margin", "flags"} of every forward.
    norm = "L2": start and proposals are those of csrc/ee_sqatk_l2.hip in torch ops on the L2 schedule (each norm the root of the squares
    summed in float64, cast to the dtype); the trace entries then also hold "x_new" and "norms" ([1, B] for the start: n0; [3 + 2C, B] for
    a proposal, zeros for a sample that made none).  Everything else is shared."""
    from eeadv import sqatk
    _check_square_norm(norm)
    B, C, H, W = x0.shape
    ids = np.arange(B) if ids is None else np.asarray(ids)
    st = _SquareQueries(model, x0, y, trace)
    if norm == "L2":
        x_best, n0 = _square_l2_start(x0, eps, seed, ids)

        def propose(x_best, i, s):
            prop, norms = _square_l2_propose(x_best, x0, eps, seed, i, ids, s)
            return prop, {"norms": norms}
        x_best = st.run(x_best, {"norms": n0.view(1, B).clone()}, sqatk.square_schedule_l2(n_queries, H, W), propose, early_exit)
        return x_best, st.margin_min, st.queries
    stripe = torch.from_numpy(sqatk.stripes(seed, ids, C, W)).to(x0.dtype).to(x0.device)
    x_best = torch.clamp(x0 + eps * stripe.view(B, C, 1, W), 0, 1)
    x_best = st.query(x_best, x_best)
    hh, ww, cc = torch.arange(H).view(1, H), torch.arange(W).view(1, W), torch.arange(C).view(1, C)
    for i, s in enumerate(engine.square_schedule(n_queries, H, W)):
        active = st.active()
        if early_exit and not bool(active.any()):
            break
        vh, vw, bits = (torch.from_numpy(a).view(B, 1) for a in sqatk.windows(seed, i, ids, H, W, s))
        inside = ((hh >= vh) & (hh < vh + s)).view(B, 1, H, 1) & ((ww >= vw) & (ww < vw + s)).view(B, 1, 1, W)
        up = torch.tensor(2.0 * eps, dtype=x0.dtype)  # a 0-dim tensor of the input's dtype: two Python scalars would make float32 of it
        sign = torch.where(((bits >> cc) & 1).bool(), up, -up).view(B, C, 1, 1)
        delta = torch.where(inside, sign, torch.zeros((), dtype=x0.dtype)).to(x0.device)
        prop = torch.clamp(torch.min(torch.max(x_best + delta, x0 - eps), x0 + eps), 0, 1)
        x_new = torch.where(active.view(-1, 1, 1, 1), prop, x_best)
        x_best = st.query(x_new, x_best)
    return x_best, st.margin_min, st.queries


def Square(model, args, inputs, targets, n_queries=5000, seed=None, norm="Linf"):
    """One Square attack (norm 'Linf' or 'L2', eps = args.epsilon, at most n_queries forwards per sample).  Returns (x_adv, robust, queries): the inputs
    with every fooled sample (margin z_y - max_{j != y} z_j <= 0 at some query) replaced by its fooling point, the [B] bool flags of the
    samples whose margin stayed positive, and the number of forwards each sample was active for.  `seed` keys the counter-based draws;
    None takes it from torch's generator (torch.manual_seed governs it).  The model runs in the mode the caller left it in; a defence that
    redraws at every forward (Add_Square) makes the margins noisy, and a lucky low margin sticks - what the non-EOT version does."""
    kw = {} if _check_square_norm(norm) == "Linf" else {"norm": norm}  # a Linf call is the call made before the parameter existed
    x0 = inputs.detach()
    eps = float(args.epsilon)
    if runtime.require_device(x0, "Square"):
        return engine.square_loop(model, x0, targets, n_queries, eps, seed, **kw)
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    x_best, margin_min, queries = _square_host(model, x0, targets, n_queries, eps, seed, **kw)
    robust = margin_min > 0
    return torch.where(robust.view(-1, 1, 1, 1), x0, x_best), robust, queries


# ---------------------------------------------------------------------------------------------------------
# Square in the L1 threat model (Croce & Hein 2021, "Mind the box"): doors of their own - Square(norm="L1") and
# _square_host(norm="L1") stay refused.  Pattern, windows, schedule and draws are the L2 run's; the window update is its L1 form, and
# every point is the exact projection (_l1_project) of x0 + delta onto the ball of radius eps_p = float32(eps * (1 - 1e-6)) and the box.
# Restarts, EOT and L1 inside Cascade / Rand at the command line are NOT here.
# ---------------------------------------------------------------------------------------------------------
def _square_l1_host(model, x0, y, n_queries, eps, seed, trace=None, ids=None, early_exit=True):
    """Plumbing path for CPU tensors (opt-in): the iteration of engine.square_l1_loop in plain torch ops, in the input's dtype, with the
    kernels' draws (eeadv.sqatk: windows_l2, windows2, tiles).  Each norm is the |values| summed in float64 and rounded once; the
    projection is the host projection of the L1-APGD host path.  A sample that makes no proposal keeps x_new = x_best untouched: no
    projection runs on it.  Returns (x_best, margin_min, queries); `trace`, a list, receives {"margin", "flags", "x_new", "lam"} of
    every forward and, behind a proposal, "norms" [2 + 2C, B] (zeros, like "lam", for a sample that made none)."""
    from eeadv import sqatk
    if not float(eps) >= 0.0:
        raise ValueError("L1 Square needs eps >= 0, got %r" % (eps,))
    B, C, H, W = x0.shape
    ids = np.arange(B) if ids is None else np.asarray(ids)
    eps_p = sqatk.l1_eps_p(eps)
    st = _SquareQueries(model, x0, y, trace)
    x_best, lam = _l1_project(x0 + _square_tiles(x0, seed, ids), x0, eps_p)

    def propose(x_best, i, s):
        prop, norms, lam = _square_l1_propose(x_best, x0, eps, eps_p, seed, i, ids, s)
        return prop, {"norms": norms, "lam": lam}
    x_best = st.run(x_best, {"lam": lam.clone()}, sqatk.square_schedule_l2(n_queries, H, W), propose, early_exit)
    return x_best, st.margin_min, st.queries




def Square_L1(model, args, inputs, targets, n_queries=5000, seed=None):
    """One Square attack in the L1 threat model (args.epsilon is the L1 radius, at most n_queries forwards per sample).  Returns (x_adv,
    robust, queries) as Square does: robust = margin_min > 0 over the points that were actually queried.  Every queried point lies in
    [0,1] and within eps_p + D * 2^-23 of the input in L1 whenever (C + 1) * eps <= D.  `seed` keys the
    counter-based draws; None takes it from torch's generator."""
    x0 = inputs.detach()
    eps = float(args.epsilon)
    if runtime.require_device(x0, "Square_L1"):
        return engine.square_l1_loop(model, x0, targets, n_queries, eps, seed)
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    x_best, margin_min, queries = _square_l1_host(model, x0, targets, n_queries, eps, seed)
    robust = margin_min > 0
    return torch.where(robust.view(-1, 1, 1, 1), x0, x_best), robust, queries


# ---------------------------------------------------------------------------------------------------------
# FAB-T (Croce & Hein 2020, Linf, targeted): the minimum-norm member of AutoAttack's `standard` version - it walks along linearised
# decision boundaries instead of ascending a loss.  Built from the published algorithm with the constants `standard`
# runs it with (eta = 1.05, beta = 0.9, alpha_max = 0.1, 9 target classes, one run from the clean point: deterministic).  norm="L2" is
# the same iteration in the other metric; L1 comes through FAB_T_L1 below (section 20), untargeted FAB through
# FAB / FAB_L1 (section 22), restarts with the random start through n_restarts (section 23).  The final line search and EOT for FAB are
# NOT here.
# ---------------------------------------------------------------------------------------------------------
_FAB_ETA, _FAB_BETA, _FAB_ALPHA_MAX = 1.05, 0.9, 0.1


def _fab_projection(p, w, c):
    """The box-constrained Linf projection of the rows of p [B,D] (in [0,1]) onto <w, .> = const at signed distance c [B]: (lambda, s,
    ||delta||_inf) per row, delta_i = -sign(s w_i) min(lambda, r_i).  Sort, cumulative sums (the sums above a breakpoint taken from the top,
    so nothing cancels) and the closed form on the segment that holds lambda.  c = 0: lambda = 0; c' >= g(inf): lambda = inf."""
    s = torch.where(c >= 0, torch.ones_like(c), -torch.ones_like(c))
    v = s.view(-1, 1) * w
    a = v.abs()
    r = torch.where(v > 0, p, torch.where(v < 0, 1 - p, torch.zeros_like(p))).clamp_min(0)
    cp = c.abs()
    rs, order = torch.sort(r, dim=1)
    a_s = a.gather(1, order)
    below = torch.cumsum(a_s * rs, dim=1)  # sum_{j <= k} a_j r_j
    above = torch.flip(torch.cumsum(torch.flip(a_s, [1]), dim=1), [1]) - a_s  # sum_{j > k} a_j
    g = below + rs * above  # g at breakpoint k
    zero = torch.zeros_like(cp).view(-1, 1)
    k = (g < cp.view(-1, 1)).sum(dim=1, keepdim=True)  # breakpoints strictly below the solution
    S = torch.cat([zero, below], dim=1).gather(1, k).squeeze(1)
    A = torch.cat([a_s.sum(dim=1, keepdim=True), above], dim=1).gather(1, k).squeeze(1)
    lam = (cp - S) / A
    lam = torch.where(cp >= below[:, -1], torch.full_like(lam, _INF), lam)
    lam = torch.where(cp == 0, torch.zeros_like(lam), lam)
    rmax = torch.where(a != 0, r, torch.zeros_like(r)).max(dim=1)[0]
    return lam, s, torch.minimum(lam, rmax)


def _fab_delta(p, w, lam, s):
    v = s.view(-1, 1) * w
    r = torch.where(v > 0, p, torch.where(v < 0, 1 - p, torch.zeros_like(p))).clamp_min(0)
    return -torch.sign(v) * torch.minimum(lam.view(-1, 1), r)


def _fab_projection_l2(p, w, c):
    """_fab_projection for the least-||.||_2 delta: (mu, s, ||delta||_2) per row, delta_i = -sign(s w_i) min(mu |w_i|, r_i), mu the smallest
    value with g(mu) = sum_i |w_i| min(mu |w_i|, r_i) = |c|.  The breakpoints are t_i = r_i / |w_i| (0 where w_i == 0: such a coordinate adds
    zeros on either side); sort by them, cumulative sums (sum_{t_j > t_k} w_j^2 taken from the top, so nothing cancels) and the closed form
    on the segment that holds mu.  c = 0: mu = 0; c' >= g(inf): mu = inf."""
    s = torch.where(c >= 0, torch.ones_like(c), -torch.ones_like(c))
    v = s.view(-1, 1) * w
    a = v.abs()
    r = torch.where(v > 0, p, torch.where(v < 0, 1 - p, torch.zeros_like(p))).clamp_min(0)
    cp = c.abs()
    moving = a != 0
    t = torch.where(moving, r / torch.where(moving, a, torch.ones_like(a)), torch.zeros_like(r))
    ts, order = torch.sort(t, dim=1)
    a_s, r_s = a.gather(1, order), r.gather(1, order)
    aa = a_s * a_s
    below = torch.cumsum(a_s * r_s, dim=1)  # sum_{j <= k} a_j r_j
    top = torch.flip(torch.cumsum(torch.flip(aa, [1]), dim=1), [1])  # sum_{j >= k} a_j^2
    above = torch.cat([top[:, 1:], torch.zeros_like(top[:, :1])], dim=1)  # sum_{j > k} a_j^2
    g = below + torch.where(above > 0, ts * above, torch.zeros_like(above))  # g at breakpoint k (t_k = inf meets no 0)
    zero = torch.zeros_like(cp).view(-1, 1)
    k = (g < cp.view(-1, 1)).sum(dim=1, keepdim=True)  # breakpoints strictly below the solution
    S = torch.cat([zero, below], dim=1).gather(1, k).squeeze(1)
    A = torch.cat([top[:, :1], above], dim=1).gather(1, k).squeeze(1)
    mu = (cp - S) / A
    mu = torch.where(cp >= below[:, -1], torch.full_like(mu, _INF), mu)
    mu = torch.where(cp == 0, torch.zeros_like(mu), mu)
    return mu, s, _l2_norms(_fab_delta_l2(p, w, mu, s))


def _fab_delta_l2(p, w, mu, s):
    v = s.view(-1, 1) * w
    a = v.abs()
    r = torch.where(v > 0, p, torch.where(v < 0, 1 - p, torch.zeros_like(p))).clamp_min(0)
    m = torch.where(a != 0, torch.minimum(mu.view(-1, 1) * a, r), torch.zeros_like(r))  # mu = inf never meets a zero
    return -torch.sign(v) * m


def _check_fab_norm(norm):
    return engine._check_norm(norm, engine.FAB_NORMS, "FAB")


def _linf_norms(v):
    return v.abs().max(dim=1)[0]


def _fab_host_iteration(model, x, x0, y, t, adv, res, norm="Linf"):
    """One FAB-T iteration in plain torch ops, in the input's dtype: (x, adv, res) -> (x, adv, res, info).  `info` holds every
    intermediate quantity (df, w, the projection scalars, alpha, the stepped point, pred, the flags).  norm: 'Linf' or 'L2' - the metric of
    the two projections (lam1 / lam2 then hold mu), of alpha and of nrm / res."""
    if _check_fab_norm(norm) == "L2":
        return _fab_iteration(model, x, x0, y, t, adv, res, _fab_projection_l2, _fab_delta_l2, _l2_norms)
    return _fab_iteration(model, x, x0, y, t, adv, res, _fab_projection, _fab_delta, _linf_norms)


def _fab_iteration(model, x, x0, y, t, adv, res, project, delta, dist, dual=None):
    """The iteration in the metric of (project, delta, dist): project(p, w, c) -> (lambda, s, ||delta||, *more) per row, delta(p, w, lambda,
    s, *more) rebuilds the vector from those scalars (L1 has one more, phi), dist(v) is the row norm that nrm / res are measured in.
    dual (untargeted FAB, t unused): the row norm dual to the metric - the hyperplane is then the closest one among all classes
    (_fab_closest_plane) and `info` also holds best_k and best."""
    B = x0.shape[0]
    rows = torch.arange(B, device=x0.device)
    xc = x.detach().clone().requires_grad_()
    more_info = {}
    if dual is None:
        with torch.enable_grad():
            z = model(xc)
            diff = z[rows, t] - z[rows, y]
        w = torch.autograd.grad(diff.sum(), [xc])[0].detach().reshape(B, -1)
        df = diff.detach()
    else:
        w, df, best_k, best = _fab_closest_plane(model, xc, y, dual)
        more_info = dict(best_k=best_k, best=best)
    xf, x0f = x.detach().reshape(B, -1), x0.reshape(B, -1)
    sabs = w.abs().sum(dim=1)
    on = torch.isfinite(df) & (df != 0) & torch.isfinite(sabs) & (sabs > 0)
    safe_w = torch.where(on.view(-1, 1), w, torch.ones_like(w))  # rows without a hyperplane are computed on stand-ins and masked below
    c1 = torch.where(on, df, torch.ones_like(df))
    c2 = torch.where(on, df + (safe_w * (x0f - xf)).sum(dim=1), torch.ones_like(df))  # a sum of differences: <w, x0> - <w, x> would cancel
    zero = torch.zeros_like(df)
    l1, s1, n1, *more1 = (torch.where(on, q, zero) for q in project(xf, safe_w, c1))
    l2, s2, n2, *more2 = (torch.where(on, q, zero) for q in project(x0f, safe_w, c2))
    d1, d2 = delta(xf, safe_w, l1, s1, *more1), delta(x0f, safe_w, l2, s2, *more2)
    a1, a2 = n1.clamp_min(1e-8), n2.clamp_min(1e-8)
    alpha = torch.minimum(a1 / (a1 + a2), torch.full_like(a1, _FAB_ALPHA_MAX))
    al = alpha.view(-1, 1)
    x_step = torch.clamp((xf + _FAB_ETA * d1) * (1 - al) + (x0f + _FAB_ETA * d2) * al, 0, 1)
    x_step = torch.where(on.view(-1, 1), x_step, xf)
    with torch.no_grad():
        z2 = model(x_step.view(x0.shape))
    pred = torch.sort(z2, dim=1, descending=True, stable=True)[1][:, 0]
    is_adv = (pred != y) & ~torch.isnan(z2).any(dim=1)
    nrm = dist(x_step - x0f)
    improved = is_adv & (nrm < res)
    adv = torch.where(improved.view(-1, 1), x_step, adv.reshape(B, -1)).view(x0.shape)
    res = torch.where(improved, nrm, res)
    x_new = torch.where(is_adv.view(-1, 1), x0f + _FAB_BETA * (x_step - x0f), x_step).view(x0.shape)
    info = dict(df=df, w=w, lam1=l1, s1=s1, n1=n1, lam2=l2, s2=s2, n2=n2, alpha=alpha, x_step=x_step.view(x0.shape), pred=pred, is_adv=is_adv,
                improved=improved, nrm=nrm, enabled=on)
    if more1:
        info.update(phi1=more1[0], phi2=more2[0])
    info.update(more_info)
    return x_new, adv, res, info


def _fab_host(model, x0, y, t, n_iter, trace=None, norm="Linf", n_restarts=1, seed=None, noise=None, eps=None, target_index=0):
    """Plumbing path for CPU tensors (opt-in), the counterpart of _host_loop: the iteration of engine.fab_loop in plain torch ops, in the
    input's dtype.  Returns (adv, res).  `trace`, a list, receives one dict of clones per iteration.  n_restarts, seed, noise, eps and
    target_index: the restarts of _fab_u_run."""
    _check_fab_norm(norm)
    return _fab_u_run(lambda x, adv, res: _fab_host_iteration(model, x, x0, y, t, adv, res, norm), x0, n_iter, trace, norm, n_restarts, seed,
                      noise, eps, target_index)


def _fab_restart_kw(x0, n_restarts, seed):
    """What the FAB doors add to their engine / host calls: nothing for one restart (the calls stay the ones they always were), else
    n_restarts and the seed - the caller's, or one drawn here, once for all target classes (on the device a ticket from torch's generator,
    as Square takes it)."""
    n_restarts = int(n_restarts)
    if n_restarts < 1:
        raise ValueError("FAB needs n_restarts >= 1, got %d" % n_restarts)
    if n_restarts == 1:
        return {}
    if seed is None:
        seed = engine._drawn_seed(x0.device) if x0.is_cuda else int(torch.randint(0, 2 ** 62, (1,)).item())
    return dict(n_restarts=n_restarts, seed=int(seed))


def FAB_T(model, args, inputs, targets, nclass, n_iter=100, n_target_classes=9, order=None, norm="Linf", n_restarts=1, seed=None):
    """Targeted FAB (norm: 'Linf', or 'L2' - every ||.||_inf below is then ||.||_2 and args.epsilon the L2 radius): one run per target class, the 2nd ... (n_target_classes + 1)-th class of the clean logits (at most nclass - 1 of
    them, taken as APGD_T takes them), each on the whole batch from the clean point.  Returns (x_adv, robust, norm): norm [B] is the smallest
    ||adv - x0||_inf over all runs (+inf if no run found an adversarial point, 0 for a sample the clean forward already misclassifies),
    robust = not (norm <= args.epsilon), and x_adv is the inputs with every non-robust sample replaced by the point that attains its norm
    (the first one, among equals).  eps only thresholds the result - the search is not confined to the ball.  Deterministic.  The model runs in
    the mode the caller left it in.  On the device c2 = df + sum w_i (x0_i - x_i) is summed in double (csrc/ee_fab.hip); the host path
    below forms the same sum of differences in the input's dtype - the public code's <w, x0> - (<w, x> - df) cancels in fp32.  `order`
    [B, n_t + 1]: the class order of the clean logits if the caller has it already - the clean forward is then skipped.  n_restarts > 1
    (DESIGN.md section 23): every target class runs its restarts, restart r >= 1 of the j-th class from the random start keyed by
    eeadv.fabstart.seed_of(seed, j, r), on the whole batch, the best norm kept across them; seed None draws one."""
    x0 = inputs.detach()
    eps = float(args.epsilon)
    kw = {} if _check_fab_norm(norm) == "Linf" else {"norm": norm}  # the Linf call is the call it always was
    rkw = _fab_restart_kw(x0, n_restarts, seed)
    return _fab_targets(model, x0, targets, nclass, n_target_classes, order, eps, "FAB_T",
                        lambda t, j: engine.fab_loop(model, x0, targets, t, n_iter, eps, **kw, **_of_class(rkw, j))[::2],
                        lambda t, j: _fab_host(model, x0, targets, t, n_iter, **kw, **_of_class(rkw, j, eps)))


def _of_class(rkw, j, eps=None):
    """The restart arguments of the run towards the j-th target class: its index keys the draws; the host paths also take eps."""
    if not rkw:
        return {}
    return dict(rkw, target_index=j) if eps is None else dict(rkw, target_index=j, eps=eps)


def _fab_targets(model, x0, targets, nclass, n_target_classes, order, eps, what, device_run, host_run):
    """The runs of FAB_T / FAB_T_L1 over the target classes and their combination; device_run(t, j) / host_run(t, j) -> (adv, norm) of the
    run towards the classes t [B], the j-th of the order."""
    n_t = min(int(n_target_classes), int(nclass) - 1)
    on_dev = runtime.require_device(x0, what)
    order = _class_order(model, x0, n_t, what, order)
    shape = (-1,) + (1,) * (x0.dim() - 1)
    x_adv = x0.clone()
    inf = torch.full((x0.shape[0],), _INF, dtype=torch.float32 if on_dev else x0.dtype, device=x0.device)
    norm = torch.where(order[:, 0] != targets, torch.zeros_like(inf), inf)
    for j in range(1, n_t + 1):
        t = order[:, j].contiguous()
        xa, nj = device_run(t, j) if on_dev else host_run(t, j)
        closer = (nj < norm) & (nj <= eps)
        x_adv = torch.where(closer.view(shape), xa, x_adv)
        norm = torch.minimum(norm, nj)
    return x_adv, ~(norm <= eps), norm


# ---------------------------------------------------------------------------------------------------------
# FAB-T in the L1 threat model: doors of their own - FAB_T(norm="L1") and _fab_host(norm="L1") stay refused.  The
# iteration is FAB-T's; the projection is the least-||.||_1 one, a fill by descending |w_i| in which every coordinate tied at the
# threshold takes the same fraction of its room.  The final line search and L1 inside Cascade are NOT here.
# ---------------------------------------------------------------------------------------------------------
def _l1_norms(v):
    """sum_i |v_i| per row, summed in float64 and rounded to v's dtype once (as the commit kernel does)."""
    return v.abs().to(torch.float64).sum(dim=1).to(v.dtype)


def _fab_projection_l1(p, w, c):
    """_fab_projection for a delta of least ||.||_1: (theta, s, ||delta||_1, phi) per row, delta_i = -sign(s w_i) m_i with m_i = r_i where
    a_i = |w_i| > theta, phi r_i where a_i == theta and 0 below.  Sort by a descending, cumulative sums of a_i r_i; theta is the a at which
    they first reach c' = |c|, and the coordinates AT theta share what is left: phi = (c' - sum_{a_i > theta} a_i r_i) / sum_{a_i == theta}
    a_i r_i.  The sums are taken in float64, as csrc/ee_fab.hip takes them, and rounded to p's dtype once.  c = 0: theta = inf (nothing
    moves); c' > sum a_i r_i: theta = 0, phi = 1 (every moving coordinate at its bound)."""
    dt = p.dtype
    s = torch.where(c >= 0, torch.ones_like(c), -torch.ones_like(c))
    v = s.view(-1, 1) * w
    a = v.abs()
    r = torch.where(v > 0, p, torch.where(v < 0, 1 - p, torch.zeros_like(p))).clamp_min(0)
    cp = c.abs().to(torch.float64)
    r64 = r.to(torch.float64)
    prod = a.to(torch.float64) * r64
    a_s, order = torch.sort(a, dim=1, descending=True, stable=True)
    cum = torch.cumsum(prod.gather(1, order), dim=1)
    k = (cum < cp.view(-1, 1)).sum(dim=1, keepdim=True).clamp_max(a.shape[1] - 1)  # the first coordinate at which the fill reaches c'
    theta = a_s.gather(1, k).squeeze(1)
    above, at = a > theta.view(-1, 1), a == theta.view(-1, 1)
    zero = torch.zeros_like(prod)
    S, P = torch.where(above, prod, zero).sum(dim=1), torch.where(at, prod, zero).sum(dim=1)
    N, R = torch.where(above, r64, zero).sum(dim=1), torch.where(at, r64, zero).sum(dim=1)
    phi = torch.where(P > 0, ((cp - S) / torch.where(P > 0, P, torch.ones_like(P))).clamp(0, 1), torch.zeros_like(P))
    n = N + phi * R
    infeasible = cp > cum[:, -1]
    theta = torch.where(infeasible, torch.zeros_like(theta), theta)
    phi = torch.where(infeasible, torch.ones_like(phi), phi)
    n = torch.where(infeasible, torch.where(a != 0, r64, zero).sum(dim=1), n)
    on_plane = cp == 0
    theta = torch.where(on_plane, torch.full_like(theta, _INF), theta)
    phi = torch.where(on_plane, torch.zeros_like(phi), phi)
    n = torch.where(on_plane, torch.zeros_like(n), n)
    return theta, s, n.to(dt), phi.to(dt)


def _fab_delta_l1(p, w, theta, s, phi):
    v = s.view(-1, 1) * w
    a = v.abs()
    r = torch.where(v > 0, p, torch.where(v < 0, 1 - p, torch.zeros_like(p))).clamp_min(0)
    th = theta.view(-1, 1)
    m = torch.where(a > th, r, torch.where((a == th) & (a != 0), phi.view(-1, 1) * r, torch.zeros_like(r)))
    return -torch.sign(v) * m


def _fab_l1_host_iteration(model, x, x0, y, t, adv, res):
    """_fab_host_iteration in the L1 threat model: lam1 / lam2 of `info` hold theta, and phi1 / phi2 the fractions."""
    return _fab_iteration(model, x, x0, y, t, adv, res, _fab_projection_l1, _fab_delta_l1, _l1_norms)


def _fab_l1_host(model, x0, y, t, n_iter, trace=None, n_restarts=1, seed=None, noise=None, eps=None, target_index=0):
    """_fab_host in the L1 threat model: the iteration of engine.fab_l1_loop in plain torch ops, in the input's dtype.  Returns (adv, res)."""
    return _fab_u_run(lambda x, adv, res: _fab_l1_host_iteration(model, x, x0, y, t, adv, res), x0, n_iter, trace, "L1", n_restarts, seed,
                      noise, eps, target_index)


def FAB_T_L1(model, args, inputs, targets, nclass, n_iter=100, n_target_classes=9, order=None, n_restarts=1, seed=None):
    """FAB_T in the L1 threat model (args.epsilon is the L1 radius): one run per target class as FAB_T takes them, each on the whole batch
    from the clean point.  Returns (x_adv, robust, norm): norm [B] is the smallest ||adv - x0||_1 over all runs (+inf if none found an
    adversarial point, 0 for a sample the clean forward already misclassifies), robust = not (norm <= args.epsilon), and x_adv is the
    inputs with every non-robust sample replaced by the point that attains its norm.  Deterministic.  Two departures from the public
    projection_l1: coordinates of equal |w_i| at the threshold all take the same fraction of their room (the public
    code fills them in the order its argsort returns - the L1 length is the same), and a coordinate takes part exactly when w_i != 0.
    n_restarts and seed as in FAB_T."""
    x0 = inputs.detach()
    eps = float(args.epsilon)
    rkw = _fab_restart_kw(x0, n_restarts, seed)
    return _fab_targets(model, x0, targets, nclass, n_target_classes, order, eps, "FAB_T_L1",
                        lambda t, j: engine.fab_l1_loop(model, x0, targets, t, n_iter, eps, **_of_class(rkw, j))[::2],
                        lambda t, j: _fab_l1_host(model, x0, targets, t, n_iter, **_of_class(rkw, j, eps)))


# ---------------------------------------------------------------------------------------------------------
# Untargeted FAB (the `fab` of the public ensemble's `plus` version and of a `custom` ['apgd-ce', 'fab'] run): the
# iteration of FAB-T, its hyperplane the closest one - in the dual norm - among the linearised boundaries z_k - z_y = 0 of ALL classes
# k != y: K backward passes per iteration.  One run from the clean point, deterministic, unless n_restarts asks for more (section 23); the
# final search and EOT are NOT here.
# ---------------------------------------------------------------------------------------------------------
def _dual_of_linf(g):
    """sum_i |g_i| per row, summed in float64 and rounded to g's dtype once (as ee_fab_select_f32 does)."""
    return g.abs().to(torch.float64).sum(dim=1).to(g.dtype)


def _dual_of_l1(g):
    """max_i |g_i| per row; a NaN propagates, so the class is skipped."""
    return g.abs().max(dim=1)[0]


def _fab_closest_plane(model, xc, y, dual):
    """(w [B,D], df [B], best_k [B], best [B]) at xc (a leaf that requires grad): one forward, then per class k in index order g_k =
    d(z_k - z_y)/dx off the retained graph, n_k = dual(g_k), dist_k = |df_k| / (1e-12 + n_k); the class of smallest dist_k wins, strict <
    over ascending k (ties to the lower class).  Skipped: k == y, df_k or n_k not finite, n_k == 0.  Nothing chosen: w = 0, df = 0,
    best_k = -1 - the iteration then rests."""
    with torch.enable_grad():
        z = model(xc)
    B, K = z.shape
    zy = z[torch.arange(B, device=z.device), y]
    w = torch.zeros(B, xc[0].numel(), dtype=xc.dtype, device=xc.device)
    df = torch.zeros(B, dtype=z.dtype, device=z.device)
    best = torch.full_like(df, _INF)
    best_k = torch.full((B,), -1, dtype=torch.int64, device=z.device)
    for k in range(K):
        diff = z[:, k] - zy
        g = torch.autograd.grad(diff.sum(), [xc], retain_graph=True)[0].detach().reshape(B, -1)
        d, n = diff.detach(), dual(g)
        dist = d.abs() / (1e-12 + n)
        take = (y != k) & torch.isfinite(d) & torch.isfinite(n) & (n != 0) & (dist < best)
        best, best_k, df = torch.where(take, dist, best), torch.where(take, torch.full_like(best_k, k), best_k), torch.where(take, d, df)
        w = torch.where(take.view(-1, 1), g, w)
    return w, df, best_k, best


_FAB_U_METRICS = {"Linf": (_fab_projection, _fab_delta, _linf_norms, _dual_of_linf),
                  "L2": (_fab_projection_l2, _fab_delta_l2, _l2_norms, _l2_norms)}
_FAB_U_L1_METRIC = (_fab_projection_l1, _fab_delta_l1, _l1_norms, _dual_of_l1)


def _fab_u_host_iteration(model, x, x0, y, adv, res, norm="Linf"):
    """One untargeted FAB iteration in plain torch ops, in the input's dtype: _fab_host_iteration with the closest hyperplane."""
    return _fab_iteration(model, x, x0, y, None, adv, res, *_FAB_U_METRICS[_check_fab_norm(norm)])


def _fab_u_l1_host_iteration(model, x, x0, y, adv, res):
    return _fab_iteration(model, x, x0, y, None, adv, res, *_FAB_U_L1_METRIC)


def _fab_u_run(iteration, x0, n_iter, trace, metric="Linf", n_restarts=1, seed=None, noise=None, eps=None, target_index=0):
    """The chain of every FAB host path (targeted ones included): restart 0 from the clean point with res = +inf, then - DESIGN.md section
    23 - restart r = 1 .. n_restarts - 1 from eeadv.fabstart.start(x0, res, eps, t, metric), t being noise[r - 1] of the injected `noise`
    [n_restarts - 1, B, ...] or the host restatement of the kernel's draw under fabstart.seed_of(seed, target_index, r); adv and res are
    carried across restarts.  `trace` receives, before the iterations of a restart r >= 1, one entry {"restart", "x_start", "res_in"}."""
    n_restarts = int(n_restarts)
    if n_restarts < 1:
        raise ValueError("FAB needs n_restarts >= 1, got %d" % n_restarts)
    if n_restarts > 1 and eps is None:
        raise ValueError("a FAB restart starts at distance min(norm so far, eps) / 2: eps is needed")
    if n_restarts > 1 and noise is None and seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    B = x0.shape[0]
    x, adv = x0.clone(), x0.clone()
    res = torch.full((B,), _INF, dtype=x0.dtype, device=x0.device)
    for r in range(n_restarts):
        if r:
            if noise is not None:
                t = noise[r - 1]
            else:
                t = torch.from_numpy(fabstart.draw(fabstart.seed_of(seed, target_index, r), B, x0[0].numel() if B else 0, metric))
            x = fabstart.start(x0, res, eps, t.to(device=x0.device).reshape(x0.shape), metric)
            if trace is not None:
                trace.append(dict(restart=torch.tensor(r), x_start=x.clone(), res_in=res.clone()))
        for _ in range(int(n_iter)):
            x, adv, res, info = iteration(x, adv, res)
            if trace is not None:
                info.update(x=x, adv=adv, res=res)
                trace.append({k: v.clone() for k, v in info.items()})
    return adv, res


def _fab_u_host(model, x0, y, n_iter, trace=None, norm="Linf", n_restarts=1, seed=None, noise=None, eps=None):
    """Plumbing path for CPU tensors (opt-in): the iteration of engine.fab_u_loop in plain torch ops, in the input's dtype, the Jacobian
    taken row by row off one retained forward.  Returns (adv, res).  `trace`, a list, receives one dict of clones per iteration."""
    _check_fab_norm(norm)
    return _fab_u_run(lambda x, adv, res: _fab_u_host_iteration(model, x, x0, y, adv, res, norm), x0, n_iter, trace, norm, n_restarts, seed,
                      noise, eps)


def _fab_u_l1_host(model, x0, y, n_iter, trace=None, n_restarts=1, seed=None, noise=None, eps=None):
    """_fab_u_host in the L1 threat model."""
    return _fab_u_run(lambda x, adv, res: _fab_u_l1_host_iteration(model, x, x0, y, adv, res), x0, n_iter, trace, "L1", n_restarts, seed,
                      noise, eps)


def _fab_untargeted(model, x0, targets, eps, what, device_run, host_run):
    """The one run of FAB / FAB_L1 and FAB_T's result convention; device_run(K) / host_run() -> (adv, norm)."""
    on_dev = runtime.require_device(x0, what)
    with torch.no_grad():
        z = model(x0)
    if on_dev:
        first = ops.topk(z.detach().float().contiguous(), None, 1)[0][:, 0]
    else:
        first = torch.sort(z, dim=1, descending=True, stable=True)[1][:, 0]
    inf = torch.full((x0.shape[0],), _INF, dtype=torch.float32 if on_dev else x0.dtype, device=x0.device)
    norm = torch.where(first != targets, torch.zeros_like(inf), inf)
    xa, nj = device_run(z.shape[1]) if on_dev else host_run()
    closer = (nj < norm) & (nj <= eps)
    x_adv = torch.where(closer.view((-1,) + (1,) * (x0.dim() - 1)), xa, x0)
    norm = torch.minimum(norm, nj)
    return x_adv, ~(norm <= eps), norm


def FAB(model, args, inputs, targets, n_iter=100, eps=None, norm="Linf", n_restarts=1, seed=None):
    """Untargeted FAB (norm: 'Linf' or 'L2'; eps, default args.epsilon, is the radius in that metric): one run of n_iter iterations on the
    whole batch from the clean point, every iteration walking towards the closest linearised decision boundary among all classes k != y -
    K backward passes per iteration, K the width of the clean logits.  Returns what FAB_T returns: (x_adv, robust, norm), norm [B] the
    smallest ||adv - x0|| over the adversarial iterates (+inf if there was none, 0 for a sample the clean forward already misclassifies),
    robust = not (norm <= eps), x_adv the inputs with every non-robust sample replaced by the point that attains its norm.  eps only
    thresholds the result.  Deterministic.  The model runs in the mode the caller left it in; on a model that redraws at every forward one
    iteration linearises one draw (no EOT).  n_restarts > 1: restart r >= 1 runs the same iterations from the
    random start keyed by eeadv.fabstart.seed_of(seed, 0, r), on the whole batch, the best norm kept across them; seed None draws one."""
    x0 = inputs.detach()
    eps = float(args.epsilon if eps is None else eps)
    kw = {} if _check_fab_norm(norm) == "Linf" else {"norm": norm}
    rkw = _fab_restart_kw(x0, n_restarts, seed)
    return _fab_untargeted(model, x0, targets, eps, "FAB",
                           lambda K: engine.fab_u_loop(model, x0, targets, n_iter, eps, nclass=K, **kw, **rkw)[::2],
                           lambda: _fab_u_host(model, x0, targets, n_iter, **kw, **(dict(rkw, eps=eps) if rkw else {})))


def FAB_L1(model, args, inputs, targets, n_iter=100, eps=None, n_restarts=1, seed=None):
    """FAB in the L1 threat model (eps, default args.epsilon, is the L1 radius): the projections of FAB_T_L1, the distance to a hyperplane
    measured in max_i |g_i|.  Returns what FAB_T_L1 returns.  n_restarts and seed as in FAB."""
    x0 = inputs.detach()
    eps = float(args.epsilon if eps is None else eps)
    rkw = _fab_restart_kw(x0, n_restarts, seed)
    return _fab_untargeted(model, x0, targets, eps, "FAB_L1",
                           lambda K: engine.fab_u_l1_loop(model, x0, targets, n_iter, eps, nclass=K, **rkw)[::2],
                           lambda: _fab_u_l1_host(model, x0, targets, n_iter, **(dict(rkw, eps=eps) if rkw else {})))


class LabelSmoothLoss(torch.nn.Module):
    """attacks.py:89-99."""

    def __init__(self, smoothing=0.0):
        super(LabelSmoothLoss, self).__init__()
        self.smoothing = smoothing

    def forward(self, input, target):
        if runtime.require_device(input, "LabelSmoothLoss"):
            return EF.cross_entropy(input, target, "mean", float(self.smoothing))
        log_prob = F.log_softmax(input, dim=-1)
        weight = input.new_ones(input.size()) * self.smoothing / (input.size(-1) - 1.)
        weight.scatter_(-1, target.unsqueeze(-1), (1. - self.smoothing))
        return (-weight * log_prob).sum(dim=-1).mean()


# Compute loss for trick model (attacks.py:103-106)
def compute_loss_and_error(logits, label, label_smoothing=0.):
    return LabelSmoothLoss(label_smoothing)(logits, label.long())


# FGSM (attacks.py:110-128)
def FGSM(model, inputs, target, targeted=False, step_size=0.007):
    x = inputs.detach().clone()
    if runtime.require_device(x, "FGSM"):
        g = engine.input_gradient(engine._unwrap(model), x.contiguous(), engine.LossSpec(engine.CE_SUM, target))
        return ops.fgsm_step(x.detach().contiguous(), g.contiguous(), float(step_size), 0.0, 1.0, -1 if targeted else 1)
    x.requires_grad_()
    with torch.enable_grad():
        loss = F.cross_entropy(model(x), target, reduction='sum')
    grad = torch.autograd.grad(loss, [x])[0]
    x = x.detach() + (-step_size if targeted else step_size) * torch.sign(grad.detach())
    return torch.clamp(x, 0.0, 1.0)


def predict_from_logits(logits, dim=1):
    """attacks.py:131-132."""
    if logits.is_cuda and logits.dim() == 2 and dim in (1, -1) and logits.dtype == torch.float32:
        return ops.topk(logits.contiguous(), None, 1)[0][:, 0]
    return logits.max(dim=dim, keepdim=False)[1]


# CW with Linf norm (attacks.py:136-232)
def CWLinfAttack(x, y, model, magnitude, previous_p, max_eps, max_iters=20, target=None, _type='linf', n_class=10,
                 cur_device=None, noise=None):
    """Evaluation-only attack.  Margin loss -sum(relu(correct - wrong + 50)) (:195-206), fixed step 0.00392
    (:212), three projections per iteration (:218-222); only currently-correct samples are attacked (:146-151).
    The update/projection chain runs through the HIP PGD-step kernel twice (box `magnitude`, then box `max_eps`
    around x - previous_p), which is the same min/max/clamp sequence."""
    model.eval()
    device = cur_device if cur_device is not None else x.device
    x, y = x.to(device), y.to(device)
    if target is not None:
        target = target.to(device)
    adv = x.clone()
    with torch.no_grad():
        pred = predict_from_logits(model(x))
    if torch.sum((pred == y)).item() == 0:
        return adv, previous_p
    ind = (pred == y).nonzero().squeeze()
    x, y = x[ind], y[ind]
    x = x if len(x.shape) == 4 else x.unsqueeze(0)
    y = y if len(y.shape) == 1 else y.unsqueeze(0)
    if target is not None:
        target = target[ind]
        target = target if len(target.shape) == 1 else target.unsqueeze(0)
    previous_p_c = None
    if previous_p is not None:
        previous_p = previous_p.to(device)
        previous_p_c = previous_p.clone()
        previous_p = previous_p[ind]
        previous_p = previous_p if len(previous_p.shape) == 4 else previous_p.unsqueeze(0)
    one_hot_y = torch.zeros(y.size(0), n_class, device=device)
    one_hot_y[torch.arange(y.size(0)), y] = 1
    mag = magnitude.item() if isinstance(magnitude, torch.Tensor) else magnitude
    if noise is None:
        rand_perturb = torch.FloatTensor(x.shape).uniform_(-mag, mag).to(device)
    else:
        rand_perturb = noise.to(device)[ind].reshape(x.shape)
    x = x.contiguous()
    centre2 = (x - previous_p).contiguous() if previous_p is not None else x
    on_dev = runtime.require_device(x, "CWLinfAttack")
    adv_imgs = ops.pgd_init(x, rand_perturb.contiguous(), 0.0, 1.0) if on_dev else torch.clamp(x + rand_perturb, 0, 1)
    for _iter in range(int(max_iters)):
        adv_imgs.requires_grad_(True)
        with torch.enable_grad():
            outputs = model(adv_imgs)
            correct_logit = torch.sum(one_hot_y * outputs, dim=1)
            if target is not None:
                wrong = torch.zeros(target.size(0), n_class, device=device)
                wrong[torch.arange(target.size(0)), target] = 1
                wrong_logit = torch.sum(wrong * outputs, dim=1)
            else:
                wrong_logit, _ = torch.max((1 - one_hot_y) * outputs - 1e4 * one_hot_y, dim=1)
            loss = -torch.sum(F.relu(correct_logit - wrong_logit + 50))
        grads = torch.autograd.grad(loss, adv_imgs)[0]
        adv_imgs = adv_imgs.detach()
        if on_dev:
            # :213 + :218 + :220 : step, box `magnitude` around x, clamp  (max/min commute inside one box)
            ops.pgd_step_(adv_imgs, grads.contiguous(), x, 0.00392, float(mag), 0.0, 1.0, 1)
            # :222 : box `max_eps` around x - previous_p, no clamp inside the loop
            ops.pgd_step_(adv_imgs, torch.zeros_like(adv_imgs), centre2, 0.0, float(max_eps), -_INF, _INF, 1)
        else:
            adv_imgs = adv_imgs + 0.00392 * torch.sign(grads)
            adv_imgs = torch.max(torch.min(adv_imgs, x + mag), x - mag).clamp_(0, 1)
            adv_imgs = torch.max(torch.min(adv_imgs, centre2 + max_eps), centre2 - max_eps)
    adv_imgs = adv_imgs.clamp_(0, 1)
    now_p = adv_imgs - x
    adv[ind] = adv_imgs
    if previous_p is not None:
        previous_p_c[ind] = previous_p + now_p
        return adv, previous_p_c
    return adv, now_p


# ALP (attacks.py:236-272)
class ALP:
    def __init__(self, step_size=0.003, epsilon=0.047, perturb_steps=5, beta=1.0):
        self.step_size = step_size
        self.epsilon = epsilon
        self.perturb_steps = perturb_steps
        self.beta = beta

    def reset_steps(self, k):
        self.perturb_steps = k

    def PGD_Linf(self, model, x_natural, y, noise=None):
        model.eval()  # side effect kept (attacks.py:249)
        x0 = x_natural.detach()
        x = _randn_start(x0, noise)
        return _loop(model, x0, x, engine.LossSpec(engine.CE_MEAN, y), lambda z: F.cross_entropy(z, y),
                     self.perturb_steps, self.step_size, self.epsilon)

    def loss(self, model, logits, logits_adv, y, optimizer):
        model.train()  # side effects kept (attacks.py:265-266)
        optimizer.zero_grad()
        if runtime.require_device(logits, "ALP.loss"):
            loss_robust = 0.5 * EF.cross_entropy(logits, y) + 0.5 * EF.cross_entropy(logits_adv, y)
            return loss_robust + self.beta * EF.mse_loss(logits, logits_adv)
        loss_robust = 0.5 * F.cross_entropy(logits, y) + 0.5 * F.cross_entropy(logits_adv, y)
        return loss_robust + self.beta * F.mse_loss(logits, logits_adv)


# Targeted ALP for Tiny ImageNet (attacks.py:276-333)
class targeted_ALP(ALP):
    def __init__(self, step_size=0.003, epsilon=0.047, perturb_steps=5, beta=1.0, n_class=200):
        ALP.__init__(self, step_size, epsilon, perturb_steps, beta)
        self.n_class = n_class

    def tarPGD_Linf(self, model, x_natural, y, device, noise=None, label_offset=None):
        model.eval()
        target_labels = _random_targets(y, self.n_class, device, label_offset)
        x0 = x_natural.detach()
        x = _randn_start(x0, noise)
        return _loop(model, x0, x, engine.LossSpec(engine.CE_MEAN, target_labels),
                     lambda z: F.cross_entropy(z, target_labels), self.perturb_steps, self.step_size, self.epsilon, -1)


# Targeted ALP for ImageNet (attacks.py:337-357)
def tar_alp_imagenet(model, args, inputs, labels, num_steps, step_size, device, noise=None, label_offset=None):
    x0 = inputs.detach()
    target_labels = _random_targets(labels, 1000, device, label_offset)
    x = _randn_start(x0, noise)
    x = _loop(model, x0, x, engine.LossSpec(engine.CE_SUM, target_labels),
              lambda z: F.cross_entropy(z, target_labels, reduction='sum'), num_steps, step_size, args.epsilon, -1)
    return x, target_labels


def squared_l2_norm(x):
    """attacks.py:360-362 (note: MEAN of squares)."""
    flattened = x.view(x.shape[0], -1)
    return (flattened ** 2).mean(1)


def l2_norm(x):
    return squared_l2_norm(x).sqrt()


class _KLBatchMean(nn.Module):
    """Stands in for nn.KLDivLoss(reduction='batchmean') as `Trades.criterion_kl`: called with
    (log_softmax(q_logits), p) it defers to torch; the loops and `loss` call the fused kernel on logits."""

    def __init__(self):
        super().__init__()
        self._torch = nn.KLDivLoss(reduction="batchmean")

    def forward(self, log_q, p):
        return self._torch(log_q, p)


# TRADES (attacks.py:369-429)
class Trades:
    def __init__(self, step_size=0.003, epsilon=0.047, perturb_steps=5, beta=1.0):
        self.step_size = step_size
        self.epsilon = epsilon
        self.perturb_steps = perturb_steps
        self.beta = beta
        self.criterion_kl = _KLBatchMean()

    def reset_steps(self, k):
        self.perturb_steps = k

    def PGD_L2(self, model, x_natural, logits, noise=None):
        """attacks.py:381-401: gradient normalised by its per-sample RMS, step alpha*g, RMS-ball projection, clamp -
        one kernel per iteration (ee_l2_step_f32) behind the KL loss-gradient kernel."""
        model.eval()
        x0 = x_natural.detach()
        if runtime.require_device(x0, "Trades.PGD_L2"):
            x0 = x0.contiguous()
            x = _randn_start(x0, noise)
            spec = engine.LossSpec(engine.KL, logits.detach().contiguous())
            net = engine._unwrap(model)
            for _ in range(self.perturb_steps):
                g = engine.input_gradient(net, x, spec)
                x = ops.l2_step_(x.detach(), g.contiguous(), x0, float(self.step_size), float(self.epsilon), 0.0, 1.0)
            return x.detach()
        nz = torch.randn(x_natural.shape, device=x_natural.device) if noise is None else noise.to(x_natural.device)
        x_adv = x_natural.detach() + 0.001 * nz.detach()
        prob = F.softmax(logits, dim=-1)
        for _ in range(self.perturb_steps):
            with torch.enable_grad():
                x_adv.requires_grad_()
                loss_kl = self.criterion_kl(F.log_softmax(model(x_adv), dim=1), prob)
            grad = torch.autograd.grad(loss_kl, [x_adv])[0].detach()
            grad /= l2_norm(grad).unsqueeze(-1).unsqueeze(-1).unsqueeze(-1) + 1e-8
            x_adv = x_adv.detach() + self.step_size * grad
            delta = x_adv - x_natural
            delta_norm = l2_norm(delta)
            cond = delta_norm > self.epsilon
            delta[cond] *= self.epsilon / delta_norm[cond].unsqueeze(-1).unsqueeze(-1).unsqueeze(-1)
            x_adv = torch.clamp(x_natural + delta, 0.0, 1.0)
        return x_adv

    def PGD_Linf(self, model, x_natural, logits, noise=None):
        model.eval()  # side effect kept (attacks.py:405), never restored here
        x0 = x_natural.detach()
        x = _randn_start(x0, noise)
        nat = logits.detach().contiguous()  # softmax(logits) is a constant w.r.t. x_adv (attacks.py:407)
        prob = F.softmax(nat, dim=-1)
        return _loop(model, x0, x, engine.LossSpec(engine.KL, nat),
                     lambda z: self.criterion_kl(F.log_softmax(z, dim=1), prob), self.perturb_steps, self.step_size,
                     self.epsilon)

    def loss(self, model, logits, x_adv, labels, optimizer):
        model.train()  # side effects kept (attacks.py:422-423)
        optimizer.zero_grad()
        if runtime.require_device(logits, "Trades.loss"):
            loss_natural = EF.cross_entropy(logits, labels)
            self.last_logits_adv = model(x_adv)  # kept for eeadv.trainer.two_branch_backward (one backward per forward pass)
            loss_robust = EF.kl_div_batchmean(self.last_logits_adv, logits)  # gradient flows into both arguments
            return loss_natural + self.beta * loss_robust
        prob = F.softmax(logits, dim=-1)
        loss_natural = F.cross_entropy(logits, labels)
        loss_robust = self.criterion_kl(F.log_softmax(model(x_adv), dim=1), prob)
        return loss_natural + self.beta * loss_robust


# AVmixup (attacks.py:433-518)
class AVmixup:
    def __init__(self, args, gamma, lambda1, lambda2, step_size, num_steps, num_classes=200, device='cuda'):
        self.args = args
        self.gamma = gamma
        self.lambda1 = lambda1
        self.lambda2 = lambda2
        self.step_size = step_size
        self.num_steps = num_steps
        self.num_classes = num_classes
        self.device = device

    def _label_smoothing(self, one_hot, factor):
        return one_hot * factor + (one_hot - 1.) * ((factor - 1) / float(self.num_classes - 1))

    def _vertex_mix(self, inputs, x, targets, beta):
        """attacks.py:469-479.  The mixing weight is numpy float64, so the labels come back float64."""
        x_weight = np.random.beta(1.0, 1.0, [x.shape[0], 1, 1, 1]) if beta is None else beta
        if runtime.require_device(x, "AVmixup"):
            w = torch.from_numpy(np.ascontiguousarray(x_weight, dtype=np.float64).reshape(-1)).to(x.device)
            x_mix = ops.avmix(x.contiguous(), inputs.contiguous(), w, float(self.gamma))
            y_nat = self._label_smoothing(targets, self.lambda1)
            y_vertex = self._label_smoothing(targets, self.lambda2)
            yw = w.view(-1, 1)
            return x_mix, y_nat * yw + y_vertex * (1 - yw)
        perturb = (x - inputs) * self.gamma
        vertex = torch.clamp(inputs + perturb, 0, 1)
        y_nat = self._label_smoothing(targets, self.lambda1)
        y_vertex = self._label_smoothing(targets, self.lambda2)
        xw = torch.from_numpy(x_weight).to(self.device)
        yw = torch.from_numpy(np.reshape(x_weight, [-1, 1])).to(self.device)
        return (inputs * xw + vertex * (1 - xw)).to(torch.float), y_nat * yw + y_vertex * (1 - yw)

    def perturb(self, model, inputs, targets, noise=None, beta=None):
        """Given (inputs, one-hot targets) returns (mixed adversarial-vertex inputs, mixed soft labels)."""
        x0 = inputs.detach()
        x = _uniform_start(x0, self.args.epsilon, noise) if self.args.random else x0.clone()
        soft = targets.detach()
        x = _loop(model, x0, x, engine.LossSpec(engine.SOFTCE, soft.to(torch.float64).contiguous()),
                  lambda z: -torch.sum(F.log_softmax(z, dim=1) * soft), self.num_steps, self.step_size, self.args.epsilon)
        return self._vertex_mix(x0, x, targets, beta)

    def tar_perturb(self, model, inputs, targets, noise=None, beta=None, label_offset=None):
        """attacks.py:481-518.  As in the reference the loss multiplies log-probabilities [B,K] by the integer
        target LABELS `fmod(targets + offset, K)`; `targets` is whatever the driver passes (one-hot there)."""
        x0 = inputs.detach()
        if label_offset is None:
            label_offset = torch.randint(low=1, high=self.num_classes, size=targets.shape).to(self.device)
        target_labels = torch.fmod(targets + label_offset.to(targets.device), self.num_classes)
        x = _uniform_start(x0, self.args.epsilon, noise) if self.args.random else x0.clone()
        tl = target_labels.detach()
        x = _loop(model, x0, x, engine.LossSpec(engine.SOFTCE, tl.to(torch.float64).contiguous()),
                  lambda z: -torch.sum(F.log_softmax(z, dim=1) * tl), self.num_steps, self.step_size, self.args.epsilon, -1)
        return self._vertex_mix(x0, x, targets, beta)
