"""The attack inner loop on the device (the K-step loop of utils/attacks.py:19-27 and its nine copies).

One PGD step = model forward, loss-gradient kernel on the logits, model backward to the input
(torch.autograd.grad with grad_outputs - the scalar loss itself is never formed inside the loop), then
ONE in-place update kernel on persistent buffers (x, x0): zero temporaries, where the reference allocates
six per step.  The K steps may run from a HIP graph captured on the first call for a given (model, shape,
loss, mode) - the loop body is launch-bound at B = 50..100.

Semantics kept from the reference: the model's train/eval mode is NOT touched here (PGD() runs in whatever
mode the caller left, BatchNorm statistics and dropout included); callers are entered under
torch.enable_grad() so an outer no_grad() does not matter; the result is a new detached tensor.

The evaluation attacks (APGD in Linf / L2 / L1, Square, FAB-T, untargeted FAB) each keep their device state in a run object with four methods - load(*inputs),
start(model), body(model, n): n consecutive iterations, result() - and share one driver: `_prepare` (build, capture, cache, load, refresh) and
`_drive` (eager run, or start + replays + result).  apgd_loop, apgd_l1_loop, fab_loop, fab_l1_loop, fab_u_loop and fab_u_l1_loop are argument checks, a cache key and one call of
`_drive`; square_loop takes `_prepare` and keeps its own replay loop (early exit, eager remainder, finish); pgd_loop, with its probed tail,
stands by itself ("The attack loops' driver").
"""
import os
import weakref

import torch

from . import fabstart, ops, runtime, sqatk
from .functional import attack_forward, input_grad_only, refresh_dense_weights

CE_SUM, CE_MEAN, KL, SOFTCE = "ce_sum", "ce_mean", "kl", "softce"
# the input-gradient pass runs on the calling thread: handing it to autograd's device thread puts cross-thread stream
# synchronisation into the captured graph (a 40 us idle gap in front of the first backward kernel of every iteration)
_MT_BACKWARD = False


class LossSpec:
    """Which d(loss)/d(logits) the loop needs.  payload: labels (CE), natural logits (KL), float64 soft
    targets (SOFTCE).  attacks.py:23 (sum CE), :255 (mean CE), :412 (KL batchmean), :462-463 (soft CE)."""

    def __init__(self, kind, payload):
        self.kind, self.payload = kind, payload

    def dlogits(self, logits):
        z = logits.detach()
        if self.kind == CE_SUM:
            return ops.ce(z, self.payload, "sum", 0.0, False, True)[1]
        if self.kind == CE_MEAN:
            return ops.ce(z, self.payload, "mean", 0.0, False, True)[1]
        if self.kind == KL:
            return ops.kl_batchmean(z, self.payload, False, True, False)[1]
        if self.kind == SOFTCE:
            return ops.softce(z, self.payload, 1.0, False, True)[1].to(torch.float32)
        raise ValueError(self.kind)


_FC_HEAD = True  # models that offer head_grad (Net_2) get head + loss + way back as one launch; False: separate launches


def _body_input_grad(model, x_in, spec, through_body):
    """d loss / d x_in through model.body (through_body) or the whole model: logits -> loss gradient -> autograd.  Models that expose
    `body_pre` / `head_grad` / `head_from_pre` and whose head_grad answers (models.Net_2: from fc1's output on) get the rest of the classifier,
    the cross-entropy and the way back as ONE launch (ops.fc_ce_grad) instead of five; the ResNets': the head's forward, then the loss gradient inside the
    head's backward launch (ops.ce_pool_linear_bwd) - two launches instead of three, the same bits."""
    pre = getattr(model, "body_pre", None) if _FC_HEAD and (through_body or not hasattr(model, "front_chain")) else None
    if pre is not None and spec.kind in (CE_SUM, CE_MEAN) and x_in.is_cuda and hasattr(model, "head_grad"):
        with torch.enable_grad(), attack_forward():
            z = pre(x_in)
        dz = model.head_grad(z.detach(), spec.payload, "mean" if spec.kind == CE_MEAN else "sum")
        if dz is not None:
            with input_grad_only(), torch.autograd.set_multithreading_enabled(_MT_BACKWARD):
                (g,) = torch.autograd.grad(z, [x_in], grad_outputs=dz)
            return g
        with torch.enable_grad():
            logits = model.head_from_pre(z)
    else:
        with torch.enable_grad(), attack_forward():
            logits = model.body(x_in) if through_body else model(x_in)
    d = spec.dlogits(logits.contiguous())
    with input_grad_only(), torch.autograd.set_multithreading_enabled(_MT_BACKWARD):
        (g,) = torch.autograd.grad(logits, [x_in], grad_outputs=d)
    return g


def _unwrap(model):
    """DDP / DataParallel wrappers add nothing to an input-gradient step (no parameter gradients are
    produced, so there is nothing to all-reduce): run the wrapped module directly."""
    inner = getattr(model, "module", None)
    return inner if isinstance(inner, torch.nn.Module) and type(model).__name__ in (
        "DistributedDataParallel", "DataParallel") else model


def input_gradient(model, x, spec):
    """g = d loss / d x for the current x (x: leaf ROCm tensor), through autograd end to end."""
    x.requires_grad_(True)
    return _body_input_grad(model, x, spec, False)


def attack_step_(model, x, x0, spec, step_size, eps, direction, lo, hi):
    """One PGD iteration in place on x (attacks.py:20-27).  Edge-enhanced models that expose their front end
    (eeadv.models._EEFrontMixin) run it as explicit kernel calls around an autograd pass over the CNN body only:
    the input gradient then never exists as one tensor - the update kernel adds its two parts in registers."""
    if getattr(model, "chain_ok", None) is not None and model.chain_ok(x):
        # two launches around the CNN body: ee_chain_fwd_f32 (draws, Add_Square, low-pass, edge filter, combine) and
        # ee_chain_bwd_f32 (gate, edge adjoint, low-pass, d Add_Square, update) - nothing of the front end's gradient reaches HBM
        with torch.no_grad():
            x_in, ctx = model.front_chain(x.detach())
        x_in.requires_grad_(True)
        g_in = _body_input_grad(model, x_in, spec, True)
        with torch.no_grad():
            model.front_chain_update_(x.detach(), g_in.contiguous(), ctx, x0, step_size, eps, lo, hi, direction)
        return
    if getattr(model, "manual_ok", None) is not None and model.manual_ok(x):
        with torch.no_grad():
            x_in, ctx = model.front_manual(x.detach())
        x_in.requires_grad_(True)
        g_in = _body_input_grad(model, x_in, spec, True)
        with torch.no_grad():
            g_lp, g_edge = model.front_manual_backward(g_in.contiguous(), ctx)
            ops.pgd_step_bcast_(x.detach(), g_lp, g_edge, x0, step_size, eps, lo, hi, direction)
        return
    g = input_gradient(model, x, spec)
    ops.pgd_step_(x.detach(), g.contiguous(), x0, step_size, eps, lo, hi, direction)


class _Captured:
    """`iters` consecutive iterations of one attack captured into one graph (one replay covers them all: consecutive replays of a
    one-iteration graph leave a ~12 us bubble between them).  `run` holds the static buffers the graph is bound to."""

    def __init__(self, model, device, iters, run=None):
        self.model, self.device, self.iters, self.run, self.graph = weakref.ref(model), device, iters, run, None

    def capture(self, model, body, start=None, warmup=None):
        """Captures body(model).  start() sets the run up first; the state that the two warm-up executions (warmup(model), by default the
        body) advance is rebuilt by the caller's own start / load before the first replay."""
        runtime.draw_state(self.device)  # the device-side draws of a captured iteration (Add_Square, Net_2's dropout) need their state to exist
        if start is not None:
            start()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):  # warm-up outside capture: MIOpen algorithm search, allocator, autograd
                (warmup or body)(model)
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        from .models import deferred_bn_counters
        with torch.cuda.graph(self.graph, capture_error_mode=runtime.capture_mode()):
            with deferred_bn_counters():  # the BatchNorm counters of the captured forwards: one launch at the end of the graph
                body(model)
        return self


def _times(n, step):
    def body(model):
        for _ in range(n):
            step(model)
    return body


class _PgdBuffers:
    """The static buffers of a captured PGD loop and its step on them."""

    def __init__(self, x0, spec, step_size, eps, direction, lo, hi):
        self.x = torch.empty_like(x0).requires_grad_(True)
        self.x0 = torch.empty_like(x0)
        self.payload = torch.empty_like(spec.payload)
        self.spec = LossSpec(spec.kind, self.payload)
        self.cfg = (step_size, eps, direction, lo, hi)

    def step(self, model):
        attack_step_(model, self.x, self.x0, self.spec, *self.cfg)

    def load(self, x_init, x0, payload):
        with torch.no_grad():
            self.x.detach().copy_(x_init)
            self.x0.copy_(x0)
            self.payload.copy_(payload)


_GRAPHS = {}
# PGD iterations per attack that run OUTSIDE the captured graph even in graph mode, so that the library's
# HIP-event hooks (ee_prof_*) can time their kernels live; bench.py sets it (DESIGN.md "Measurement").
PROBE_ITERS = 0
# a replay covers up to this many consecutive iterations (the largest divisor of the iteration count below it): one-step
# graphs leave a ~12 us bubble between replays, very long graphs cost capture time and node memory for nothing
MAX_ITERS_PER_GRAPH = 16


def graphs_enabled():
    return os.environ.get("EEADV_GRAPH", "0") == "1"


def clear_graphs():
    _GRAPHS.clear()


def _chunk(n):
    """Iterations per replay: the largest divisor of n not above MAX_ITERS_PER_GRAPH."""
    return max(c for c in range(1, min(n, MAX_ITERS_PER_GRAPH) + 1) if n % c == 0)


def _eot_chunk(n, eot_iter):
    """Iterations per replay of a loop whose iteration holds eot_iter forward/backward pairs: the largest divisor of n not above
    max(1, MAX_ITERS_PER_GRAPH // eot_iter) - the graph keeps about the node count of MAX_ITERS_PER_GRAPH plain iterations (E = 20: one
    iteration per graph; E = 1: _chunk(n))."""
    cap = max(1, MAX_ITERS_PER_GRAPH // int(eot_iter))
    return max(c for c in range(1, min(n, cap) + 1) if n % c == 0)


def _cached(key, model, build):
    """The captured loop under `key`: the cached one if it was captured on this very model (ids are reused), else build()'s."""
    gs = _GRAPHS.get(key)
    if gs is not None and gs.model() is model:
        return gs
    # what runs before and around a capture (a start point, the two warm-up executions) are extra train-mode forwards: shield the
    # BatchNorm statistics from them.  Restored through .data so that autograd graphs the caller still holds (TRADES / ALP keep
    # `preds = model(x)` alive across the attack) do not see a version bump on the saved running statistics.
    saved = {}
    if model.training:
        saved = {k: v.clone() for k, v in model.state_dict().items() if "running_" in k or "num_batches" in k}
    gs = _GRAPHS[key] = build()
    if saved:
        live = model.state_dict()
        for k, v in saved.items():
            live[k].data.copy_(v)
    return gs


def _adv_where_fooled(robust, x0, x_adv):
    """x0 where the sample is robust, else its adversarial point."""
    return torch.where(robust.view(-1, *([1] * (x0.dim() - 1))), x0, x_adv)


def _empty_result(x0, dtype):
    """What an attack returns for an empty batch: (x_adv, robust, its third result in `dtype`)."""
    return x0.clone(), torch.ones(0, dtype=torch.bool, device=x0.device), torch.zeros(0, dtype=dtype, device=x0.device)


def _check_norm(norm, allowed, what):
    if norm not in allowed:
        raise ValueError("%s norm must be one of %s, got %r" % (what, list(allowed), norm))
    return norm


def _prepare(model, key, make_run, inputs, chunk):
    """The first half of the driver: the captured loop under `key` - on a miss make_run() is loaded and run.body(model, chunk) captured
    behind run.start(model) - with its run loaded with `inputs` and the weight-derived buffers its kernels read (functional.Conv3x3Map2Fn)
    brought up to date.  What is left to the caller: run.start(model), the replays, run.result()."""
    def build():
        run = make_run()
        run.load(*inputs)
        return _Captured(model, run.x0.device, chunk, run).capture(model, lambda m: run.body(m, chunk), start=lambda: run.start(model))

    gs = _cached(key, model, build)
    gs.run.load(*inputs)
    refresh_dense_weights()
    return gs


def _drive(model, key, make_run, inputs, n_iter, chunk, use_graph, n_restarts=1):
    """One attack of n_iter iterations on a run object (load(*inputs), start(model), body(model, n, last=False): n consecutive
    iterations, result()): eager - one body call, told that none follows - or n_iter // chunk replays of the graph cached under `key`.
    load, start and result stay outside the graph ("The attack loops' driver").  n_restarts > 1 (FAB, section 23;
    APGD, section 24): the same iterations once more behind run.restart(model, r) for r = 1 .. n_restarts - 1 - the same graph, whatever the count."""
    if not use_graph:
        run = make_run()
        run.load(*inputs)
        for r in range(n_restarts):
            run.start(model) if r == 0 else run.restart(model, r)
            run.body(model, n_iter, last=r + 1 == n_restarts)
        return run.result()
    gs = _prepare(model, key, make_run, inputs, chunk)
    for r in range(n_restarts):
        gs.run.start(model) if r == 0 else gs.run.restart(model, r)
        for _ in range(n_iter // gs.iters):
            gs.graph.replay()
    return gs.run.result()


def pgd_loop(model, x0, x_init, spec, num_steps, step_size, eps, direction=1, lo=0.0, hi=1.0, use_graph=None):
    """Runs num_steps updates starting from x_init (a fresh tensor the loop may update in place); returns a
    detached tensor.  attacks.py:19-27: x = clamp(min(max(x + dir*alpha*sign(g), x0-eps), x0+eps), 0, 1)."""
    model = _unwrap(model)
    x0 = x0.detach().contiguous()
    if use_graph is None:
        use_graph = graphs_enabled()
    if use_graph and num_steps > min(PROBE_ITERS, num_steps):
        probe = min(PROBE_ITERS, num_steps)
        n_graph = num_steps - probe
        chunk = _chunk(n_graph)
        key = ("pgd", id(model), model.training, tuple(x0.shape), spec.kind, tuple(spec.payload.shape), spec.payload.dtype,
               float(step_size), float(eps), direction, lo, hi, x0.device.index, chunk)

        def build():
            bufs = _PgdBuffers(x0, spec, step_size, eps, direction, lo, hi)
            bufs.load(x_init, x0, spec.payload)
            return _Captured(model, x0.device, chunk, bufs).capture(model, _times(chunk, bufs.step), warmup=bufs.step)

        gs = _cached(key, model, build)
        gs.run.load(x_init.detach().contiguous(), x0, spec.payload)
        refresh_dense_weights()  # weight-derived buffers the captured kernels read (functional.Conv3x3Map2Fn)
        for _ in range(n_graph // gs.iters):
            gs.graph.replay()
        x = gs.run.x.detach().clone()
        if probe:
            # the probed iterations come LAST: their first kernel then follows an iteration's last one, caches as warm as inside the
            # graph (as the attack's first iteration, right behind the parameter update, the front-end kernel read its tables cold and
            # measured 23 ... 45 us from run to run against rocprofv3's 24 over the in-graph launches)
            for _ in range(probe):  # eager passes launch exactly what the graph replays
                attack_step_(model, x, x0, spec, step_size, eps, direction, lo, hi)
                x = x.detach()
        return x

    x = x_init.detach().contiguous()
    for _ in range(num_steps):
        attack_step_(model, x, x0, spec, step_size, eps, direction, lo, hi)
        x = x.detach()
    return x.requires_grad_(False)


# ---------------------------------------------------------------------------------------------------------------------------------------
# APGD (Croce & Hein 2020; Linf or L2, one run): APGD-CE, APGD-DLR and, on the targeted DLR loss, the runs of APGD-T; eot_iter > 1 averages
# every gradient over that many forwards of a randomised defence; norm = "L2" swaps the step launch (section 16)
# ---------------------------------------------------------------------------------------------------------------------------------------
APGD_NORMS = ("Linf", "L2")


def _schedule(n_iter, first, following):
    """sched[i] = the window length k when a checkpoint closes iteration i (0-based), else 0: the first window is `first` iterations
    long, the one after a window of k `following(k)`."""
    sched, since, k = [0] * n_iter, 0, first
    for i in range(n_iter):
        since += 1
        if since == k:
            sched[i], since, k = k, 0, following(k)
    return sched


def _n_iter(n_iter):
    n_iter = int(n_iter)
    if n_iter < 1:
        raise ValueError("APGD needs n_iter >= 1")
    return n_iter


def apgd_schedule(n_iter):
    """The checkpoints of a Linf / L2 run (_schedule).  k starts at max(int(0.22 n), 1) and shrinks by max(int(0.03 n), 1) per checkpoint
    down to max(int(0.06 n), 1): n = 100 puts checkpoints after iterations 22, 41, 57, 70, 80, 87, 93, 99 (counted from 1)."""
    n = _n_iter(n_iter)
    n_min, dec = max(int(0.06 * n), 1), max(int(0.03 * n), 1)
    return _schedule(n, max(int(0.22 * n), 1), lambda k: max(k - dec, n_min))


def _apgd_args(loss, targets, trace, use_graph):
    """The argument checks the APGD loops share; returns use_graph with its default resolved (a trace asks for an eager run)."""
    if loss not in ops.APGD_KINDS:
        raise ValueError("APGD loss must be one of %s, got %r" % (sorted(ops.APGD_KINDS), loss))
    if loss == "dlr_t" and targets is None:
        raise ValueError("the targeted DLR loss needs targets")
    if use_graph is None:
        use_graph = graphs_enabled() and trace is None
    if use_graph and trace is not None:
        raise ValueError("the APGD trace is recorded by eager runs only")
    return use_graph


def _apgd_restarts(x0, n_restarts, seed, noise, target_index):
    """(n_restarts, what the count adds to the run's load arguments): () for one restart - the load call, like every other, is then the
    one made before restarts existed and no ticket is taken - else (seeds, noise) as _fab_restarts forms them."""
    n_restarts, seeds, noise = _fab_restarts(x0, n_restarts, seed, noise, target_index, "APGD")
    return n_restarts, (() if n_restarts == 1 else (seeds, noise))


class _ApgdSpec:
    """The loss-gradient step of `_body_input_grad` for an APGD run: the row losses, their logit gradient and `pred` in one launch, then -
    once the run is past its start point - the run's per-sample bookkeeping (run.book()).  The kind is none of the CE kinds, so the route
    is the generic one (logits -> this -> autograd): the fused head launches produce no row losses."""

    def __init__(self, run):
        self.kind, self.payload, self.run = run.KIND + run.loss, run.y, run

    def dlogits(self, logits):
        r = self.run
        r.loss_rows, d, r.pred = ops.apgd_loss(logits.detach(), r.y, r.loss, r.t)
        if r.started:
            r.book()
        return d


class _ApgdState:
    """What the APGD runs of every threat model share: the buffers (iterate, clean point, the gradient `g` that travels between
    iterations, best point / its gradient / first fooling point, labels, targets, the per-sample float and int state, counter,
    schedule), `load`, `body` and `result`.  A subclass adds the state of its step and its own `start`, `gradient`, `iteration` and
    `book` (the bookkeeping launch that _ApgdSpec makes inside every forward/backward past the start point).  No host read anywhere."""

    def __init__(self, x0, y, n_iter, eps, loss, sched, trace):
        B, dev = x0.shape[0], x0.device
        self.loss, self.eps, self.n_iter, self.trace = loss, float(eps), int(n_iter), trace
        self.x = torch.empty_like(x0).requires_grad_(True)
        self.x0, self.g = torch.empty_like(x0), torch.empty_like(x0)
        self.x_best, self.g_best, self.x_best_adv = torch.empty_like(x0), torch.empty_like(x0), torch.empty_like(x0)
        self.y = torch.empty(B, dtype=torch.int64, device=dev)
        self.t = torch.empty(B, dtype=torch.int64, device=dev) if loss == "dlr_t" else None
        self.fstate = torch.empty((4, B), dtype=torch.float32, device=dev)
        self.istate = torch.empty((4, B), dtype=torch.int32, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.sched = torch.tensor(sched, dtype=torch.int32).to(dev)
        self.loss_rows = self.pred = None
        self.started = False
        self.spec = _ApgdSpec(self)
        self.n_restarts, self.seeds, self.noise = 1, (), None
        self.adv_all = self.robust_all = self.loss_all = None  # the union across restarts: they exist once a call asks for more than one

    def load(self, x_init, x0, y, targets, seeds=(), noise=None):
        """seeds: the Philox keys of restarts 1 .. n_restarts - 1 (their count sets n_restarts); noise [n_restarts - 1, B, ...]: their draws,
        injected in place of the kernel's own.  Neither is seen by the graph."""
        self.seeds, self.noise, self.n_restarts = tuple(seeds), noise, 1 + len(seeds)
        if self.n_restarts > 1 and self.adv_all is None:
            B, dev = self.x0.shape[0], self.x0.device
            self.adv_all = torch.empty_like(self.x0)
            self.robust_all = torch.empty(B, dtype=torch.int32, device=dev)
            self.loss_all = torch.empty(B, dtype=torch.float32, device=dev)
        with torch.no_grad():
            self.x.detach().copy_(x_init)
            self.x0.copy_(x0)
            self.y.copy_(y)
            if self.t is not None:
                self.t.copy_(targets)

    def _merge(self, first):
        ops.apgd_merge_(self.adv_all, self.robust_all, self.loss_all, self.x_best_adv, self.istate[ops.APGD_I_ROBUST],
                        self.fstate[ops.APGD_F_LOSS_BEST], first)

    def restart(self, model, r):
        """Restart r >= 1: the finished restart goes into the union, x <- a fresh draw of the run's own start
        distribution around x0, then `start` - the forward/backward at the new point and the state reset of restart 0, an L1 run's
        projection and an EOT run's E draws included."""
        noise = None if self.noise is None else self.noise[r - 1]
        with torch.no_grad():
            self._merge(r == 1)
            ops.apgd_start_(self.x.detach(), self.x0, self.eps, self.norm, self.seeds[r - 1], noise, self.path)
        self.start(model)

    def body(self, model, n, last=False):
        """n consecutive iterations.  The gradient enters through self.g and - unless this is the last body of the attack - leaves through
        it: one copy per replay of a captured graph, inside which each iteration reads the autograd result of the one before (an EOT run
        sums into self.g itself: no copy)."""
        g = self.g
        for _ in range(n):
            g = self.iteration(model, g)
        if not last and g is not self.g:
            self.g.copy_(g)

    def result(self):
        with torch.no_grad():
            if self.n_restarts > 1:  # the last restart joins the union: fooled by any restart, the point of the first that fooled
                self._merge(False)
                robust = self.robust_all != 0
                return _adv_where_fooled(robust, self.x0, self.adv_all), robust, self.loss_all.clone()
            robust = self.istate[ops.APGD_I_ROBUST] != 0
            return _adv_where_fooled(robust, self.x0, self.x_best_adv), robust, self.fstate[ops.APGD_F_LOSS_BEST].clone()


class _ApgdRun(_ApgdState):
    """The device state of one APGD run (include/eeadv.h, "APGD") and its two pieces: `start` (the forward/backward at the start point and the
    initial state: a handful of small launches, once per attack) and `iteration` (step, forward, loss, bookkeeping, backward, copies: what
    a captured graph replays).  eot_iter = E > 1: every gradient is the mean over E forward/backward pairs, summed
    into `g` by ee_apgd_eot_acc_f32 (so `g` is the one gradient buffer of the run), and the bookkeeping runs once per iterate on the mean
    of the E row losses and the last draw's pred.  norm = "L2": the run owns `norms` [3, B] and `iteration` launches ee_apgd_step_l2_f32 in
    the place of ee_apgd_step_f32 - nothing else knows the norm.  `trace` (a list, eager runs only) receives one dict per gradient
    evaluation."""
    KIND = "apgd_"
    path = "auto"  # of the restarts' start launch

    def __init__(self, x0, y, n_iter, eps, loss, eot_iter=1, norm="Linf", trace=None):
        self.norm, self.eot_iter = _check_norm(norm, APGD_NORMS, "APGD"), int(eot_iter)
        B, dev = x0.shape[0], x0.device
        self.norms = torch.zeros((3, B), dtype=torch.float32, device=dev) if norm == "L2" else None  # its fill stays the run's first launch
        super().__init__(x0, y, n_iter, eps, loss, apgd_schedule(n_iter), trace)
        if self.eot_iter > 1:
            self.loss_acc = torch.empty(B, dtype=torch.float64, device=dev)
            self.loss_mean = torch.empty(B, dtype=torch.float32, device=dev)
        self.x_old = torch.empty_like(x0)
        self.loss0 = torch.empty(B, dtype=torch.float32, device=dev)

    def book(self):
        """Inside a forward/backward: the bookkeeping of a run without EOT.  An EOT run keeps books once per iterate, after the last draw
        (`gradient`)."""
        if self.eot_iter == 1:
            ops.apgd_book_(self.loss_rows, self.pred, self.fstate, self.istate, self.counter, self.sched)

    def gradient(self, model):
        """The gradient of the current iterate and, past the start point, its bookkeeping.  E = 1: one forward/backward, the bookkeeping
        inside it (_ApgdSpec), a fresh tensor.  E > 1: E of them, each followed by the accumulate launch, then the bookkeeping on
        (loss_mean, the last draw's pred); the result is self.g."""
        E = self.eot_iter
        if E == 1:
            # .contiguous() launches nothing for the dense tensor autograd returns here: the start point, which did without it before
            # EOT existed, and the iterations launch what they always launched
            g = input_gradient(model, self.x, self.spec).contiguous()
            if self.trace is not None:
                self._note([dict(loss=self.loss_rows.clone(), pred=self.pred.clone(), g=g.clone())], self.loss_rows, g)
            return g
        draws = []
        for k in range(E):
            g = input_gradient(model, self.x, self.spec).contiguous()
            ops.apgd_eot_acc_(self.g, g, self.loss_acc, self.loss_rows, self.loss_mean, k, E)
            if self.trace is not None:
                draws.append(dict(loss=self.loss_rows.clone(), pred=self.pred.clone(), g=g.clone()))
        if self.started:
            ops.apgd_book_(self.loss_mean, self.pred, self.fstate, self.istate, self.counter, self.sched)
        if self.trace is not None:
            self._note(draws, self.loss_mean, self.g)
        return self.g

    def _note(self, draws, loss, g):
        """One trace entry: the draws, what the bookkeeping received (the start point has none: its flags are None) and the gradient
        before the copies of `select`."""
        self.trace.append(dict(draws=draws, book_loss=loss.clone(), book_pred=self.pred.clone(), g_mean=g.clone(),
                               counter=int(self.counter.item()) if self.started else None,
                               flags=self.istate[ops.APGD_I_FLAGS].clone() if self.started else None))

    def start(self, model):
        self.started = False
        g = self.gradient(model)
        self.started = True
        loss = self.loss_rows if self.eot_iter == 1 else self.loss_mean
        with torch.no_grad():
            x = self.x.detach()
            for t in (self.x_old, self.x_best, self.x_best_adv):
                t.copy_(x)
            if g is not self.g:
                self.g.copy_(g)
            self.g_best.copy_(g)
            self.loss0.copy_(loss)
            self.fstate[ops.APGD_F_STEP].fill_(2.0 * self.eps)
            self.fstate[ops.APGD_F_LOSS_BEST:].copy_(loss.expand(3, -1))
            self.istate.zero_()
            self.istate[ops.APGD_I_REDUCED_LAST].fill_(1)
            self.istate[ops.APGD_I_ROBUST].copy_(self.pred)
            self.counter.zero_()

    def iteration(self, model, g):
        """One iteration from the gradient `g` of the current iterate; returns the gradient of the next one (a fresh tensor, restored in
        place for the samples a checkpoint sent back)."""
        if self.norms is None:
            if self.trace is not None:
                self.trace.append(dict(step_g=g.clone()))
            ops.apgd_step_(self.x.detach(), self.x_old, g, self.x0, self.fstate[ops.APGD_F_STEP], self.counter, self.eps)
        else:
            entry = None
            if self.trace is not None:
                entry = dict(step_g=g.clone(), x_in=self.x.detach().clone(), x_old_in=self.x_old.clone(),
                             step=self.fstate[ops.APGD_F_STEP].clone(), counter=int(self.counter.item()))
                self.trace.append(entry)
            ops.apgd_step_l2_(self.x.detach(), self.x_old, g, self.x0, self.fstate[ops.APGD_F_STEP], self.counter, self.eps, self.norms)
            if entry is not None:
                entry.update(norms=self.norms.clone(), x=self.x.detach().clone(), x_old=self.x_old.clone())
        g_new = self.gradient(model)
        ops.apgd_select_(self.x.detach(), g_new, self.x_best, self.g_best, self.x_best_adv, self.istate[ops.APGD_I_FLAGS], self.counter)
        return g_new


def apgd_loop(model, x0, x_init, y, n_iter, eps, loss, targets=None, use_graph=None, eot_iter=1, trace=None, norm="Linf", n_restarts=1,
              seed=None, noise=None, target_index=0):
    """One APGD run of n_iter iterations from x_init inside the eps-ball around x0, on loss 'ce', 'dlr' or 'dlr_t' (which takes `targets`).
    norm: 'Linf' (the default: exactly what ran before the parameter existed) or 'L2' - the ball is then the L2 ball of radius eps and the
    step ee_apgd_step_l2_f32; start, losses, bookkeeping, copies, EOT, the initial step 2 eps and the schedule are
    shared, and the trace's {"step_g"} entries also hold "x_in", "x_old_in", "step", "counter", "norms" [3, B], "x" and "x_old".
    Returns (x_adv, robust, loss_best): x0 with the rows that were fooled at any point replaced by a fooling point, robust [B] bool,
    the best row loss seen [B].  The model's mode is left as the caller set it.  Eager, or - under EEADV_GRAPH=1 / use_graph - replayed from a
    captured graph of up to MAX_ITERS_PER_GRAPH iterations; both give the same bits.

    eot_iter = E > 1 (expectation over transformation, for a defence that redraws at every forward): every gradient evaluation, the start
    point's included, is E forward/backward pairs whose input gradients are averaged (ee_apgd_eot_acc_f32); the bookkeeping runs once per
    iterate on the mean of the E row losses (summed in double) and on the LAST draw's pred.  A replay then covers _eot_chunk(n_iter, E)
    iterations.  E = 1 launches exactly what the loop launched before EOT existed.  `trace` (a list, eager only) receives, per gradient
    evaluation (the start's first), {"draws": [{"loss", "pred", "g"} per draw], "book_loss", "book_pred", "g_mean", "counter", "flags"}
    (the last two None at the start point) and, before each step, {"step_g"}: the gradient that step reads.

    n_restarts = 1 (the default) is the one run from x_init - the launches, buffers and bits of the loop before restarts existed, no ticket
    taken.  n_restarts > 1: restart 0 is that run; restart r >= 1 runs the same n_iter iterations - the same graph -
    on the WHOLE batch from a fresh draw of the run's own start distribution (ee_apgd_start_f32: Linf clamp(x0 + eps U(-1, 1), 0, 1),
    L2 clamp(x0 + eps n / ||n||_2, 0, 1)), drawn on the device under fabstart.seed_of(seed, target_index, r) (seed None: one ticket from
    torch's generator) or taken from noise[r - 1] (`noise` [n_restarts - 1, B, ...], injected).  robust is then "no restart fooled it",
    x_adv holds the point of the first restart that did (ee_apgd_merge_f32) and loss_best the largest over the restarts."""
    use_graph = _apgd_args(loss, targets, trace, use_graph)
    eot_iter = int(eot_iter)
    if eot_iter < 1:
        raise ValueError("APGD needs eot_iter >= 1, got %d" % eot_iter)
    _check_norm(norm, APGD_NORMS, "APGD")
    model = _unwrap(model)
    x0 = x0.detach().contiguous()
    x_init = x_init.detach().contiguous()
    n_iter = _n_iter(n_iter)
    chunk = _eot_chunk(n_iter, eot_iter)
    key = ("apgd", id(model), model.training, tuple(x0.shape), loss, norm, n_iter, float(eps), x0.device.index, chunk, eot_iter)
    n_restarts, more = _apgd_restarts(x0, n_restarts, seed, noise, target_index)
    return _drive(model, key, lambda: _ApgdRun(x0, y, n_iter, eps, loss, eot_iter, norm, trace), (x_init, x0, y, targets) + more, n_iter,
                  chunk, use_graph, n_restarts)


# ---------------------------------------------------------------------------------------------------------------------------------------
# APGD in the L1 threat model (Croce & Hein 2021; no momentum, no EOT, no large-radius warm-up; restarts: section 24): a door of its own
# next to apgd_loop, which keeps refusing norm = "L1" 
# ---------------------------------------------------------------------------------------------------------------------------------------
def apgd_l1_schedule(n_iter):
    """The checkpoints of an L1 run (_schedule): the first window is max(int(0.04 n), 1) iterations, every later one max(int(0.06 n), 1) -
    n = 100 puts checkpoints after iterations 4, 10, 16, ... (counted from 1)."""
    n = _n_iter(n_iter)
    k_next = max(int(0.06 * n), 1)
    return _schedule(n, max(int(0.04 * n), 1), lambda k: k_next)


class _ApgdL1Run(_ApgdState):
    """The device state of one L1-APGD run (include/eeadv.h, "APGD in the L1 threat model") and its two pieces: `start` (the projection of
    the start point, its forward/backward and the initial state, once per attack) and `iteration` (step, forward, loss, bookkeeping,
    backward, copies: what a captured graph replays).  `trace` (a list, eager runs only) receives one dict for the start and one per
    iteration."""
    KIND = "apgd_l1_"
    norm = "L1"

    def __init__(self, x0, y, n_iter, eps, loss, path="auto", trace=None):
        B, dev = x0.shape[0], x0.device
        self.path, self.per_sample = path, x0.numel() // B if B else 0
        self.topk = torch.empty(B, dtype=torch.float32, device=dev)
        self.spstate = torch.empty((2, B), dtype=torch.int32, device=dev)
        self.scal = torch.zeros((ops.L1_SCAL_ROWS, B), dtype=torch.float32, device=dev)
        self.scal0 = torch.zeros((ops.L1_SCAL_ROWS, B), dtype=torch.float32, device=dev)  # the start projection's
        super().__init__(x0, y, n_iter, eps, loss, apgd_l1_schedule(n_iter), trace)  # after the two fills: they stay the run's first launches

    def book(self):
        ops.apgd_book_l1_(self.loss_rows, self.pred, self.x.detach(), self.x_best, self.x0, self.fstate, self.istate, self.topk, self.spstate,
                          self.counter, self.sched, self.eps)

    def gradient(self, model):
        return input_gradient(model, self.x, self.spec).contiguous()

    def _state(self):
        return dict(step=self.fstate[ops.APGD_F_STEP].clone(), topk=self.topk.clone(), sp_old=self.spstate[0].clone())

    def start(self, model):
        self.started = False
        x = self.x.detach()
        u = x.clone() if self.trace is not None else None
        ops.l1_proj(x, self.x0, self.eps, out=x, scal=self.scal0, path=self.path)  # x = P(x0 + n): the step's projection, by itself
        g = self.gradient(model)
        self.started = True
        with torch.no_grad():
            for t in (self.x_best, self.x_best_adv):
                t.copy_(x)
            self.g.copy_(g)
            self.g_best.copy_(g)
            self.fstate[ops.APGD_F_STEP].fill_(self.eps)
            self.fstate[ops.APGD_F_LOSS_BEST:].copy_(self.loss_rows.expand(3, -1))
            self.istate.zero_()
            self.istate[ops.APGD_I_ROBUST].copy_(self.pred)
            self.topk.fill_(0.2)
            self.spstate[0].fill_(self.per_sample)
            self.spstate[1].zero_()
            self.counter.zero_()
        if self.trace is not None:
            self.trace.append(dict(start=True, u=u, scal=self.scal0.clone(), x=x.clone(), loss=self.loss_rows.clone(), pred=self.pred.clone(),
                                   g=g.clone(), **self._state()))

    def iteration(self, model, g):
        """One iteration from the gradient `g` of the current iterate; returns the gradient of the next one (a fresh tensor, restored in
        place for the samples a checkpoint sent back)."""
        entry = None
        if self.trace is not None:
            entry = dict(step_g=g.clone(), x_in=self.x.detach().clone(), counter=int(self.counter.item()),
                         **{k + "_in": v for k, v in self._state().items()})
        ops.apgd_step_l1_(self.x.detach(), g, self.x0, self.fstate[ops.APGD_F_STEP], self.topk, self.eps, self.scal, self.path)
        if entry is not None:
            entry.update(scal=self.scal.clone(), x=self.x.detach().clone())
        g_new = self.gradient(model)
        if entry is not None:
            entry.update(loss=self.loss_rows.clone(), pred=self.pred.clone(), g=g_new.clone(), flags=self.istate[ops.APGD_I_FLAGS].clone(),
                         sp=self.spstate[1].clone(), loss_best=self.fstate[ops.APGD_F_LOSS_BEST].clone(), **self._state())
        ops.apgd_select_(self.x.detach(), g_new, self.x_best, self.g_best, self.x_best_adv, self.istate[ops.APGD_I_FLAGS], self.counter)
        if entry is not None:
            entry.update(x_out=self.x.detach().clone(), g_out=g_new.clone(), x_best=self.x_best.clone(), x_best_adv=self.x_best_adv.clone())
            self.trace.append(entry)
        return g_new


def apgd_l1_loop(model, x0, x_init, y, n_iter, eps, loss, targets=None, use_graph=None, trace=None, path="auto", n_restarts=1, seed=None,
                 noise=None, target_index=0):
    """One L1-APGD run of n_iter iterations inside {z : ||z - x0||_1 <= eps} n [0,1]^D, on loss 'ce', 'dlr' or 'dlr_t' (which takes
    `targets`).  x_init is the unprojected start x0 + n: the run starts at P(x_init), the exact projection (ee_l1_proj_f32).  An
    iteration is ee_apgd_step_l1_f32 -> forward -> ee_apgd_loss_f32 -> ee_apgd_book_l1_f32 -> backward -> ee_apgd_select_f32 on the
    schedule apgd_l1_schedule(n_iter); step starts at eps, topk at 0.2, sp_old at the per-sample size.  Returns
    (x_adv, robust, loss_best) as apgd_loop does.  The model's mode is left as the caller set it.  Eager, or - under EEADV_GRAPH=1 /
    use_graph - replayed from a captured graph of up to MAX_ITERS_PER_GRAPH iterations; both give the same bits.  `path` picks the
    kernels' path ('auto', 'resident', 'streaming'; the same bits).  `trace` (a list, eager only) receives the start's dict {"start", "u",
    "scal", "x", "loss", "pred", "g", "step", "topk", "sp_old"} and, per iteration, {"step_g", "x_in", "counter", "step_in", "topk_in",
    "sp_old_in", "scal", "x", "loss", "pred", "g", "flags", "sp", "loss_best", "step", "topk", "sp_old", "x_out", "g_out", "x_best",
    "x_best_adv"}: what the step read and wrote, what the bookkeeping decided, and the state after the copies.  n_restarts, seed, noise
    and target_index as in apgd_loop: restart r >= 1 starts at P(x0 + n), n a fresh standard normal draw (the trace then holds one start
    dict per restart)."""
    use_graph = _apgd_args(loss, targets, trace, use_graph)
    ops._sample_path(path, "the L1 kernels'")
    if not float(eps) >= 0.0:
        raise ValueError("L1-APGD needs eps >= 0, got %r" % (eps,))
    model = _unwrap(model)
    x0 = x0.detach().contiguous()
    x_init = x_init.detach().contiguous()
    n_iter = _n_iter(n_iter)
    if x0.shape[0] == 0:
        return _empty_result(x0, torch.float32)
    chunk = _chunk(n_iter)
    key = ("apgd_l1", id(model), model.training, tuple(x0.shape), loss, n_iter, float(eps), x0.device.index, chunk, path)
    n_restarts, more = _apgd_restarts(x0, n_restarts, seed, noise, target_index)
    return _drive(model, key, lambda: _ApgdL1Run(x0, y, n_iter, eps, loss, path, trace), (x_init, x0, y, targets) + more, n_iter, chunk,
                  use_graph, n_restarts)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Square attack (Andriushchenko et al. 2020; Linf or L2, margin loss, p_init = 0.8 with the rescaled schedule, one run, no EOT): DESIGN.md
# sections 12 and 18
# ---------------------------------------------------------------------------------------------------------------------------------------
SQUARE_CHECK_EVERY = 64  # iterations between two host reads of "is any sample still active" (the only host read of the attack)
SQUARE_NORMS = ("Linf", "L2")


def square_schedule(n_queries, H, W):
    """sizes[i] = the window edge of proposal i (0-based; n_queries - 1 proposals, the start being the first query):
    clamp(int(round(sqrt(p(i) * H * W))), 1, min(H, W)) with Add_Square's p table at p_init = 0.8, i rescaled to a run of 10000."""
    return sqatk.square_schedule(n_queries, H, W)


def _signed64(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed - (1 << 64) if seed >= (1 << 63) else seed


# norm -> (init, step - names in `ops`, looked up when a run is made -, rows of `norms` for C channels, and the attributes of the run that
# init and step take behind eps): the norm enters a Square run at these two launches only.  No rows (Linf): the launches take no pattern
# tables either, and the schedule is the Linf one.  L1 has a door of its own (square_l1_loop): a run class names the norms its door accepts
_SQUARE_NORM = {"Linf": ("sqatk_init_", "sqatk_step_", None, (), ()),
                "L2": ("sqatk_init_l2_", "sqatk_step_l2_", lambda C: 3 + 2 * C, ("path",), ("norms", "path")),
                "L1": ("sqatk_init_l1_", "sqatk_step_l1_", lambda C: 2 + 2 * C, ("eps_p", "scal", "path"), ("eps_p", "norms", "scal", "path"))}
_SQUARE_WRITTEN = ("norms", "scal")  # those of the attributes above that a launch writes: what a trace keeps of it


class _SquareRun:
    """The device state of one Square attack (include/eeadv.h, "Square attack") and its pieces: `start` (the start and its forward, once
    per attack), `iteration` (step, eval forward under no_grad, margin: what a captured graph replays) and `finish` (the commit of the
    last accepted proposal).  No host read anywhere.  Init and step are the launches _SQUARE_NORM names for the norm (`path` picks their
    path) - nothing else knows it; an L2 or L1 run owns `norms`, the pattern tables `eta` with `eta_off` and the L2 schedule, an L1 run
    also `scal` [4, B] (the projection's rows) and eps_p, the radius of every projection (sqatk.l1_eps_p: formed once, here)."""

    NORMS = SQUARE_NORMS  # the norms this door accepts; the rest of _SQUARE_NORM is refused here

    def __init__(self, x0, y, n_queries, eps, norm="Linf", path="auto"):
        init, step, rows, self.init_more, self.step_more = _SQUARE_NORM[_check_norm(norm, self.NORMS, "Square")]
        self.init_, self.step_ = getattr(ops, init), getattr(ops, step)
        if rows is not None:
            ops._sample_path(path, "the %s Square kernels'" % norm)
        self._state(x0, n_queries, eps)
        B, C, dev = x0.shape[0], x0.shape[1], x0.device
        self.norm, self.path, self.norms = norm, path, None
        if "scal" in self.step_more:  # the run projects
            self.eps_p = sqatk.l1_eps_p(eps)
            self.scal = torch.zeros((ops.SQATK_L1_SCAL_ROWS, B), dtype=torch.float32, device=dev)
        if rows is not None:
            self._tables(x0, n_queries)
            self.norms = torch.zeros((rows(C), B), dtype=torch.float32, device=dev)
        else:
            self.sizes = torch.tensor(square_schedule(n_queries, x0.shape[2], x0.shape[3]), dtype=torch.int32).to(dev)

    def _state(self, x0, n_queries, eps):
        """What no launch of the norm's own sees: images, margins, flags, counter, query count, seed."""
        if x0.dim() != 4:
            raise ValueError("the Square attack takes image batches [B,C,H,W], got shape %s" % (tuple(x0.shape),))
        B, dev = x0.shape[0], x0.device
        self.eps, self.n_queries = float(eps), int(n_queries)
        self.x0, self.x_best, self.x_new = torch.empty_like(x0), torch.empty_like(x0), torch.empty_like(x0)
        self.y = torch.empty(B, dtype=torch.int64, device=dev)
        self.margin_out = torch.empty(B, dtype=torch.float32, device=dev)
        self.margin_min = torch.empty(B, dtype=torch.float32, device=dev)
        self.queries = torch.zeros(B, dtype=torch.int32, device=dev)
        self.flags = torch.zeros(B, dtype=torch.int32, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.seed = torch.zeros(1, dtype=torch.int64, device=dev)
        self.trace, self.step_entry = None, None

    def _tables(self, x0, n_queries):
        """The L2 schedule and the pattern tables eta with eta_off (the L1 run's too): sizes, eta, eta_off, eta0."""
        dev = x0.device
        H, W = x0.shape[2:]
        sizes = sqatk.square_schedule_l2(n_queries, H, W)
        s0 = sqatk.start_size(H, W)
        eta, eta_off, off0 = sqatk.eta_tables(sizes, s0)
        self.sizes = torch.tensor(sizes, dtype=torch.int32).to(dev)
        self.eta = torch.from_numpy(eta).to(dev)
        self.eta_off = torch.from_numpy(eta_off).to(dev)
        self.eta0 = self.eta[off0:off0 + s0 * s0].view(s0, s0)  # the start's table: a view, nothing of its own

    def load(self, x0, y, seed):
        with torch.no_grad():
            self.x0.copy_(x0)
            self.y.copy_(y)
            self.seed.copy_(torch.tensor([_signed64(seed)], dtype=torch.int64))  # in place: a captured graph holds this tensor's address

    def _query(self, model):
        with torch.no_grad():
            z = model(self.x_new)
        ops.sqatk_margin_(z.detach().float().contiguous(), self.y, self.margin_out, self.margin_min, self.queries, self.flags, self.counter)
        if self.trace is not None:
            entry = {"margin": self.margin_out.clone(), "flags": self.flags.clone()}
            entry.update(self.step_entry or {})  # an L2 run: what the step before this forward read and wrote
            self.step_entry = None
            self.trace.append(entry)

    def start(self, model):
        with torch.no_grad():
            self.margin_min.fill_(float("inf"))
            self.queries.zero_()
            self.flags.zero_()
            self.counter.fill_(-1)  # the start's margin launch brings it to proposal 0
        self._init()
        self._query(model)

    def _init(self):
        tables = () if self.norms is None else (self.eta0,)
        self.init_(self.x_best, self.x_new, self.x0, self.seed, *tables, self.eps, *(getattr(self, name) for name in self.init_more))
        self._record({}, self.init_more)  # an L1 run: the start's forward carries its projection

    def _step(self, sizes):
        entry = None
        if self.trace is not None and self.norms is not None:
            entry = dict(x_best_in=self.x_best.clone(), x_new_in=self.x_new.clone(), counter=int(self.counter.item()))
        tables = () if self.norms is None else (self.eta_off, self.eta)
        self.step_(self.x_best, self.x_new, self.x0, self.flags, self.margin_min, self.counter, sizes, *tables, self.seed, self.eps,
                   *(getattr(self, name) for name in self.step_more))
        self._record(entry, self.step_more)

    def _record(self, entry, more):
        """Under a trace, a launch that wrote some of `more` leaves `entry`, those and x_new for the forward that follows it."""
        written = [name for name in more if name in _SQUARE_WRITTEN]
        if self.trace is not None and written:
            entry.update({name: getattr(self, name).clone() for name in written}, x_new=self.x_new.clone())
            self.step_entry = entry

    def iteration(self, model):
        self._step(self.sizes)
        self._query(model)

    def body(self, model, n, last=False):
        for _ in range(n):
            self.iteration(model)

    def finish(self):
        """The flags of the last margin launch are still to be committed: a step without a table commits and proposes nothing."""
        self._step(None)

    def any_active(self):
        return bool((~(self.margin_min <= 0)).any().item())

    def result(self):
        with torch.no_grad():
            robust = self.margin_min > 0
            return _adv_where_fooled(robust, self.x0, self.x_best), robust, self.queries.clone()


def square_loop(model, x0, y, n_queries, eps, seed=None, use_graph=None, trace=None, early_exit=True, norm="Linf", path="auto"):
    """One Square attack of at most n_queries forwards per sample inside the eps-ball around x0 [B,C,H,W].  Returns (x_adv, robust,
    queries): x0 with the fooled rows (margin_min <= 0) replaced by their fooling point, robust [B] bool (margin_min > 0), and the number
    of forwards each sample was active for (int32 [B]).  `seed` keys the draws (None: a ticket from torch's generator of the device, so
    torch.manual_seed governs it).  The model's mode is left as the caller set it.  Eager, or - under EEADV_GRAPH=1 / use_graph - replayed
    from a captured graph of MAX_ITERS_PER_GRAPH iterations, the remainder running eagerly; both give the same bits.  early_exit: the
    host reads "is any sample still active" once per SQUARE_CHECK_EVERY iterations and stops when none is - fooled samples are frozen, so
    the result is the same bits either way.  `trace` (a list, eager only) receives {"margin", "flags"} of every forward, the start's
    first.  norm: 'Linf' (the default: exactly what ran before the parameter existed) or 'L2' - the ball is then the L2 ball of radius eps,
    start and proposal those of ee_sqatk_l2.hip (`path` picks the kernels' path, the same bits) on the L2 schedule;
    margin, accept rule, counter, query count, early exit and the graph are shared, and the trace entry of a forward that follows a step
    also holds "x_best_in", "x_new_in", "counter", "norms" [3 + 2C, B] and "x_new"."""
    _check_norm(norm, SQUARE_NORMS, "Square")
    model, x0, n_queries, seed, use_graph = _square_args(model, x0, n_queries, seed, use_graph, trace)
    key = ("square", id(model), model.training, tuple(x0.shape), n_queries, float(eps), x0.device.index, min(n_queries - 1, MAX_ITERS_PER_GRAPH),
           norm, path)
    return _square_drive(model, key, lambda: _SquareRun(x0, y, n_queries, eps, norm, path), x0, y, n_queries, seed, use_graph, trace, early_exit)


def _square_drive(model, key, make_run, x0, y, n_queries, seed, use_graph, trace, early_exit):
    """The queries of one Square attack on a run object, whatever its threat model: start, then n_queries - 1 iterations - replays of the
    graph cached under `key` (whose chunk is min(n_queries - 1, MAX_ITERS_PER_GRAPH)) while a whole chunk is left, eager ones for the
    remainder - with the early-exit read, then finish and result."""
    n_prop = n_queries - 1
    chunk = min(n_prop, MAX_ITERS_PER_GRAPH)
    if x0.shape[0] == 0:
        return _empty_result(x0, torch.int32)
    if not use_graph or chunk == 0:
        run, gs = make_run(), None
        run.load(x0, y, seed)
    else:
        gs = _prepare(model, key, make_run, (x0, y, seed), chunk)
        run = gs.run
    run.trace = trace
    run.start(model)
    done = 0
    while done < n_prop:
        if early_exit and done and done % SQUARE_CHECK_EVERY == 0 and not run.any_active():
            break
        if gs is not None and n_prop - done >= gs.iters:
            gs.graph.replay()
            done += gs.iters
        else:
            run.iteration(model)
            done += 1
    run.finish()
    run.trace = None
    return run.result()


def _square_args(model, x0, n_queries, seed, use_graph, trace):
    """(model, x0, n_queries, seed, use_graph) as both Square doors take them."""
    model = _unwrap(model)
    x0 = x0.detach().contiguous()
    n_queries = int(n_queries)
    if n_queries < 1:
        raise ValueError("Square needs n_queries >= 1")
    if use_graph is None:
        use_graph = graphs_enabled() and trace is None
    if use_graph and trace is not None:
        raise ValueError("the Square trace is recorded by eager runs only")
    if seed is None:
        seed = _drawn_seed(x0.device)
    return model, x0, n_queries, seed, use_graph


def _drawn_seed(device):
    """A key from torch's generator of the device, so torch.manual_seed governs it.  The generator's seed is the same for every attack of
    a process, its offset is what the ticket advances: both go into the key."""
    s, off = runtime.philox_ticket(device, 4)
    return (s + (off + 1) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------------------------------
# Square in the L1 threat model (Croce & Hein 2021): a door of its own - square_loop(norm="L1") and
# _SquareRun(norm="L1") stay refused
# ---------------------------------------------------------------------------------------------------------------------------------------
class _SquareL1Run(_SquareRun):
    """_SquareRun with the two launches of ee_sqatk_l1.hip, `norms` [2 + 2C, B], `scal` and eps_p; everything else is _SquareRun's."""
    NORMS = ("L1",)

    def __init__(self, x0, y, n_queries, eps, path="auto"):
        super().__init__(x0, y, n_queries, eps, "L1", path)


def square_l1_loop(model, x0, y, n_queries, eps, seed=None, use_graph=None, trace=None, early_exit=True, path="auto"):
    """square_loop in the L1 threat model: one Square attack of at most n_queries forwards per sample inside {z : ||z - x0||_1 <= eps} n
    [0,1]^D around x0 [B,C,H,W].  Start and proposal are those of ee_sqatk_l1.hip: the L2 run's pattern, windows,
    schedule and draws, the L1 form of the window update, and the exact projection of ee_l1_proj_f32 onto the ball of radius
    eps_p = float32(eps * (1 - 1e-6)) and the box, inside the step's launch.  Returns (x_adv, robust, queries) as square_loop does; margin,
    accept rule, counter, query count, early exit and the graph are shared with it (the capture key shares nothing, so Linf, L2 and L1
    graphs of one shape coexist).  Eager and replayed runs, early_exit or not, and the paths ('auto', 'resident', 'streaming') return the
    same bits.  `trace` (a list, eager only) receives {"margin", "flags"} of every forward, the start's first - with "scal" [4, B] and
    "x_new" of the start; the entry of a forward that follows a step also holds "x_best_in", "x_new_in", "counter", "norms" [2 + 2C, B],
    "scal" [4, B] and "x_new"."""
    ops._sample_path(path, "the L1 Square kernels'")
    if not float(eps) >= 0.0:
        raise ValueError("L1 Square needs eps >= 0, got %r" % (eps,))
    model, x0, n_queries, seed, use_graph = _square_args(model, x0, n_queries, seed, use_graph, trace)
    key = ("square_l1", id(model), model.training, tuple(x0.shape), n_queries, float(eps), x0.device.index,
           min(n_queries - 1, MAX_ITERS_PER_GRAPH), path)
    return _square_drive(model, key, lambda: _SquareL1Run(x0, y, n_queries, eps, path), x0, y, n_queries, seed, use_graph, trace, early_exit)


# ---------------------------------------------------------------------------------------------------------------------------------------
# FAB-T (Croce & Hein 2020; Linf or L2, targeted, eta = 1.05, beta = 0.9, alpha_max = 0.1, one run from x0, no EOT): DESIGN.md sections
# 13 and 17 (L1: fab_l1_loop at the end of this file, section 20)
# ---------------------------------------------------------------------------------------------------------------------------------------
FAB_NORMS = ("Linf", "L2")


# norm -> (projection, step, commit - names in `ops`, looked up when a run is made -, rows of the projection scalars): the metric enters
# FAB at these three launches only.  L1 has doors of its own (fab_l1_loop, fab_u_l1_loop): a run class names the norms its door accepts
_FAB_METRIC = {"Linf": ("fab_proj_linf", "fab_step_", "fab_commit_", 3),
               "L2": ("fab_proj_l2", "fab_step_l2_", "fab_commit_l2_", 3),
               "L1": ("fab_proj_l1", "fab_step_l1_", "fab_commit_l1_", ops.FAB_L1_ROWS)}


def _fab_restarts(x0, n_restarts, seed, noise, target_index=0, what="FAB"):
    """(n_restarts, seeds, noise) as _FabRun.load takes them.  One restart - the default - draws nothing and takes no ticket: the calls
    are the ones made before restarts existed.  Otherwise restart r = 1 .. n_restarts - 1 draws under fabstart.seed_of(seed, target_index,
    r) (seed None: a ticket from torch's generator of the device, as square_loop takes it), or takes noise[r - 1] of the injected
    `noise` [n_restarts - 1, B, ...]."""
    n_restarts = int(n_restarts)
    if n_restarts < 1:
        raise ValueError("%s needs n_restarts >= 1, got %d" % (what, n_restarts))
    if n_restarts == 1:
        return 1, (), None
    if noise is not None:
        noise = noise.detach().to(device=x0.device, dtype=torch.float32).contiguous()
        if tuple(noise.shape) != (n_restarts - 1,) + tuple(x0.shape):
            raise ValueError("noise has shape %s, expected %s" % (tuple(noise.shape), (n_restarts - 1,) + tuple(x0.shape)))
        return n_restarts, (0,) * (n_restarts - 1), noise
    if seed is None:
        seed = _drawn_seed(x0.device)
    return n_restarts, tuple(fabstart.seed_of(seed, target_index, r) for r in range(1, n_restarts)), None


class _FabSpec:
    """The loss-gradient step of `_body_input_grad` for a FAB run: df = z_t - z_y, its logit gradient and `pred` in one launch.  The kind is
    none of the CE kinds, so the route is the generic one (logits -> this -> autograd), through the whole model for edge-enhanced ones."""

    def __init__(self, run):
        self.kind, self.payload, self.run = "fab_t", run.y, run

    def dlogits(self, logits):
        r = self.run
        r.df, d, r.pred_at_x = ops.fab_diff(logits.detach().float().contiguous(), r.y, r.t)
        return d


class _FabRun:
    """The device state of one FAB-T run (include/eeadv.h, "FAB-T") and its two pieces: `start` (the initial state: a few fills, once per
    run) and `iteration` (forward, diff, backward, projection, step, forward, commit: what a captured graph replays).  No host read anywhere.
    `eps` only thresholds `result`: the graph does not know it, so a cached run takes the caller's through `load`."""

    NORMS = FAB_NORMS  # the norms this door accepts; the rest of _FAB_METRIC is refused here

    def __init__(self, x0, y, n_iter, eps, path="auto", norm="Linf"):
        B, dev = x0.shape[0], x0.device
        self.n_iter, self.eps, self.path, self.norm = int(n_iter), float(eps), path, norm
        *launches, rows = _FAB_METRIC[_check_norm(norm, self.NORMS, "FAB")]
        self.proj, self.step_, self.commit_ = (getattr(ops, name) for name in launches)
        self.x = torch.empty_like(x0).requires_grad_(True)
        self.x0, self.adv = torch.empty_like(x0), torch.empty_like(x0)
        self.y = torch.empty(B, dtype=torch.int64, device=dev)
        self.t = torch.empty(B, dtype=torch.int64, device=dev)
        self.res = torch.empty(B, dtype=torch.float32, device=dev)
        self.scal = torch.zeros((rows, 2 * B), dtype=torch.float32, device=dev)
        self.pred = torch.zeros(B, dtype=torch.int32, device=dev)
        self.flags = torch.zeros(B, dtype=torch.int32, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.df = self.pred_at_x = None
        self.spec = _FabSpec(self)
        self.n_restarts, self.seeds, self.noise = 1, (), None

    def load(self, x0, y, targets, eps=None, seeds=(), noise=None):
        """seeds: the Philox keys of restarts 1 .. n_restarts - 1 (their count sets n_restarts); noise [n_restarts - 1, B, ...]: their draws,
        injected in place of the kernel's own.  Neither is seen by the graph."""
        if eps is not None:
            self.eps = float(eps)
        self.seeds, self.noise, self.n_restarts = tuple(seeds), noise, 1 + len(seeds)
        with torch.no_grad():
            self.x0.copy_(x0)
            self.y.copy_(y)
            self.t.copy_(targets)

    def start(self, model):  # the driver's signature; FAB starts at the clean point, without a forward
        with torch.no_grad():
            self.x.detach().copy_(self.x0)
            self.adv.copy_(self.x0)
            self.res.fill_(float("inf"))
            self.flags.zero_()
            self.counter.zero_()

    def restart(self, model, r):
        """Restart r >= 1: x <- the random point at distance min(res, eps) / 2 from x0, from the run's own res on the
        device; flags and counter as in start.  adv and res stay: the commit launch keeps minimising across restarts."""
        noise = None if self.noise is None else self.noise[r - 1]
        with torch.no_grad():
            ops.fab_start_(self.x.detach(), self.x0, self.res, self.eps, self.norm, self.seeds[r - 1], noise, self.path)
            self.flags.zero_()
            self.counter.zero_()

    def iteration(self, model):
        w = input_gradient(model, self.x, self.spec).contiguous()
        self.advance(model, w, self.df)  # the spec has set df by now

    def advance(self, model, w, df):
        """What follows the hyperplane (w, df), however it was found: projection, step, second forward, commit."""
        x = self.x.detach()
        self.proj(x, self.x0, w, df, self.path, self.scal)
        self.step_(x, self.x0, w, self.scal)
        with torch.no_grad():
            z = model(self.x)
        self.commit_(z.detach().float().contiguous(), self.y, x, self.x0, self.adv, self.res, self.pred, self.flags, self.counter)

    def body(self, model, n, last=False):
        for _ in range(n):
            self.iteration(model)

    def result(self):
        with torch.no_grad():
            robust = ~(self.res <= self.eps)
            return _adv_where_fooled(robust, self.x0, self.adv), robust, self.res.clone()


def _fab_drive(model, x0, n_iter, use_graph, path, restarts, name, size_of, make_run, load, chunk=None, norm=None):
    """What fab_loop, fab_l1_loop, fab_u_loop and fab_u_l1_loop share: the argument checks, the empty batch, the graph key, the restarts'
    keys and _drive.  restarts: the arguments of _fab_restarts behind x0.  size_of(model, x0, n_iter): what the key holds behind the
    device and make_run(x0, size) gets - the iterations per graph of a targeted door, K of an untargeted one.  load: the run's load tuple
    between x0 and (seeds, noise).  chunk: the iterations per graph, where they are not `size` - 1 for the untargeted doors: a replay's
    bubble is nothing against K backward passes, and MAX_ITERS_PER_GRAPH iterations of K passes each would be a graph of thousands of
    nodes.  norm: that of a door that takes one (it ends the key)."""
    model = _unwrap(model)
    x0 = x0.detach().contiguous()
    n_iter = int(n_iter)
    if n_iter < 1:
        raise ValueError("FAB needs n_iter >= 1")
    ops._sample_path(path, "FAB projection")
    if norm is not None:
        _check_norm(norm, FAB_NORMS, "FAB")
    if int(restarts[0]) < 1:
        raise ValueError("FAB needs n_restarts >= 1, got %d" % int(restarts[0]))
    if x0.shape[0] == 0:
        return _empty_result(x0, torch.float32)
    if use_graph is None:
        use_graph = graphs_enabled()
    size = size_of(model, x0, n_iter)
    key = (name, id(model), model.training, tuple(x0.shape), path, x0.device.index, size) + (() if norm is None else (norm,))
    n_restarts, seeds, noise = _fab_restarts(x0, *restarts)
    return _drive(model, key, lambda: make_run(x0, size), (x0,) + load + (seeds, noise), n_iter, size if chunk is None else chunk, use_graph,
                  n_restarts)


def fab_loop(model, x0, y, targets, n_iter, eps, use_graph=None, path="auto", norm="Linf", n_restarts=1, seed=None, noise=None, target_index=0):
    """One FAB-T run of n_iter iterations from x0 towards the classes `targets` [B] in the threat model `norm` ('Linf' or 'L2': the metric of
    the projections, of alpha and of the result).  Returns (x_adv, robust, norm): norm [B] is the smallest ||adv - x0|| in that metric
    over the adversarial iterates (+inf if there was none), robust = not (norm <= eps), and x_adv is x0 with the
    non-robust rows replaced by that closest adversarial point.  The search itself is not confined to the eps-ball: FAB looks for the
    minimum norm and eps only thresholds its result.  With n_restarts = 1 (the default) deterministic - no random start, no draws of its
    own.  n_restarts > 1: restart r >= 1 runs the same n_iter iterations from a random point at distance
    min(norm so far, eps) / 2 from x0, drawn under fabstart.seed_of(seed, target_index, r) (seed None: a ticket from torch's generator) or
    taken from noise[r - 1] (`noise` [n_restarts - 1, B, ...], injected); adv and norm are kept across restarts, so norm is the smallest
    over all of them.  The graph does not know the count: one cached graph serves any number of restarts.  The model's mode is left as the
    caller set it.  Eager, or - under EEADV_GRAPH=1 / use_graph - replayed from a captured graph of up to MAX_ITERS_PER_GRAPH iterations; both
    give the same bits.  `path` picks the projection kernel's path ('auto', 'resident', 'streaming'; the same bits)."""
    return _fab_drive(model, x0, n_iter, use_graph, path, (n_restarts, seed, noise, target_index), "fab",
                      lambda m, x, n: _chunk(n), lambda x, _: _FabRun(x, y, n_iter, eps, path, norm), (y, targets, eps), norm=norm)


# ---------------------------------------------------------------------------------------------------------------------------------------
# FAB-T in the L1 threat model: a door of its own - fab_loop(norm="L1") and _FabRun(norm="L1") stay refused
# ---------------------------------------------------------------------------------------------------------------------------------------
class _FabL1Run(_FabRun):
    """_FabRun with the three L1 launches and their [4, 2B] scalars (theta, sign, ||delta||_1, phi); state, start, iteration and result
    are _FabRun's, and `res` holds L1 distances."""
    NORMS = ("L1",)

    def __init__(self, x0, y, n_iter, eps, path="auto"):
        super().__init__(x0, y, n_iter, eps, path, "L1")


def fab_l1_loop(model, x0, y, targets, n_iter, eps, use_graph=None, path="auto", n_restarts=1, seed=None, noise=None, target_index=0):
    """fab_loop in the L1 threat model: one FAB-T run of n_iter iterations from x0 towards the classes `targets` [B], the projections
    the least-||.||_1 ones (ee_fab_proj_l1_f32: a fill by descending |w_i|, ties sharing one fraction), alpha from their L1 lengths.
    Returns (x_adv, robust, norm): norm [B] is the smallest ||adv - x0||_1 over the adversarial iterates (+inf if there was none),
    robust = not (norm <= eps) with eps the L1 radius, x_adv is x0 with the non-robust rows replaced by that closest point.  Eager, or -
    under EEADV_GRAPH=1 / use_graph - replayed from a captured graph of its own (the key shares nothing with fab_loop's, so Linf, L2 and
    L1 graphs of one shape coexist); both give the same bits, and so do the paths ('auto', 'resident', 'streaming').  n_restarts, seed,
    noise and target_index as in fab_loop; the start of a restart lies at L1 distance min(norm so far, eps) / 2."""
    return _fab_drive(model, x0, n_iter, use_graph, path, (n_restarts, seed, noise, target_index), "fab_l1",
                      lambda m, x, n: _chunk(n), lambda x, _: _FabL1Run(x, y, n_iter, eps, path), (y, targets, eps))


# ---------------------------------------------------------------------------------------------------------------------------------------
# Untargeted FAB (Linf, L2 and - through a door of its own - L1): the iteration of FAB-T with w and df taken from the
# CLOSEST linearised boundary among all classes k != y.  One forward, K backward passes off its retained graph, one ee_fab_select_f32 each
# ---------------------------------------------------------------------------------------------------------------------------------------
def _n_classes(model, x0, nclass):
    """K of an untargeted run: `nclass`, or the width of one clean forward's logits."""
    if nclass is None:
        with torch.no_grad():
            nclass = model(x0).shape[1]
    nclass = int(nclass)
    if nclass < 2:
        raise ValueError("untargeted FAB needs at least 2 classes, got %d" % nclass)
    return nclass


class _FabURun(_FabRun):
    """_FabRun whose w and df come from the running arg-min over the classes: `iteration` takes one forward through the generic route (the
    whole model, attack_forward()), then per class k in index order the logit gradient of z_k - z_y (ops.fab_diff with targets filled with
    k), one backward pass off the retained forward and ops.fab_select; projection, step, second forward and commit are _FabRun's.  The
    [B, K, D] Jacobian never exists: a class's gradient is folded into (best, best_k, w, df) before the next is taken."""

    def __init__(self, x0, y, n_iter, eps, nclass, path="auto", norm="Linf"):
        super().__init__(x0, y, n_iter, eps, path, norm)
        B, dev = x0.shape[0], x0.device
        self.K = int(nclass)
        self.classes = torch.arange(self.K, dtype=torch.int64, device=dev).view(-1, 1).expand(self.K, B).contiguous()  # row k: targets = k
        self.w = torch.zeros_like(x0)
        self.df = torch.zeros(B, dtype=torch.float32, device=dev)
        self.best = torch.full((B,), float("inf"), dtype=torch.float32, device=dev)
        self.best_k = torch.full((B,), -1, dtype=torch.int32, device=dev)

    def load(self, x0, y, eps=None, seeds=(), noise=None):
        super().load(x0, y, y, eps, seeds, noise)

    def hyperplane(self, model):
        """(w, df) of the closest linearised boundary at self.x, in the run's buffers."""
        with torch.enable_grad(), attack_forward():
            logits = model(self.x)
        z = logits.detach().float().contiguous()
        if z.shape[1] != self.K:
            raise ValueError("untargeted FAB was set up for %d classes, the model returns %d" % (self.K, z.shape[1]))
        for k in range(self.K):
            d = ops.fab_diff(z, self.y, self.classes[k])[1]
            with input_grad_only(), torch.autograd.set_multithreading_enabled(_MT_BACKWARD):
                (g,) = torch.autograd.grad(logits, [self.x], grad_outputs=d.to(logits.dtype), retain_graph=k + 1 < self.K)
            ops.fab_select(g.contiguous(), z, self.y, k, self.norm, self.best, self.best_k, self.w, self.df, first=k == 0)
        return self.w, self.df

    def iteration(self, model):
        self.advance(model, *self.hyperplane(model))


class _FabUL1Run(_FabURun):
    """_FabURun with the three L1 launches and their [4, 2B] scalars; the arg-min measures in max |g_i|."""
    NORMS = ("L1",)

    def __init__(self, x0, y, n_iter, eps, nclass, path="auto"):
        super().__init__(x0, y, n_iter, eps, nclass, path, "L1")


def fab_u_loop(model, x0, y, n_iter, eps, use_graph=None, path="auto", norm="Linf", nclass=None, n_restarts=1, seed=None, noise=None):
    """One untargeted FAB run of n_iter iterations from x0 in the threat model `norm` ('Linf' or 'L2'): fab_loop's iteration, contract and
    result triple (x_adv, robust, norm), with the hyperplane of every iteration the closest one - in the dual norm - among the linearised
    boundaries z_k - z_y = 0 of all classes k != y (ties to the lower class; a class whose df or gradient norm is not finite, or whose
    gradient is zero, is skipped; a sample with every class skipped stays where it is).  An iteration costs one forward with autograd, K
    backward passes off its retained graph and one more forward; K = nclass, or the width of one clean forward's logits.  Deterministic
    with n_restarts = 1; n_restarts, seed and noise as in fab_loop (the keys are fabstart.seed_of(seed, 0, r)).
    Eager, or - under EEADV_GRAPH=1 / use_graph - replayed from a captured graph of ONE iteration under a key of its own ("fab_u"); both give
    the same bits.  On a model that redraws at every forward, all K hyperplanes of an iteration belong to the one draw of its forward."""
    _check_norm(norm, FAB_NORMS, "FAB")
    return _fab_drive(model, x0, n_iter, use_graph, path, (n_restarts, seed, noise), "fab_u",
                      lambda m, x, n: _n_classes(m, x, nclass), lambda x, K: _FabURun(x, y, n_iter, eps, K, path, norm), (y, eps), 1, norm)


def fab_u_l1_loop(model, x0, y, n_iter, eps, use_graph=None, path="auto", nclass=None, n_restarts=1, seed=None, noise=None):
    """fab_u_loop in the L1 threat model: the projections of fab_l1_loop, the distance to a hyperplane measured in max |g_i|, eps the L1
    radius.  A graph key of its own ("fab_u_l1")."""
    return _fab_drive(model, x0, n_iter, use_graph, path, (n_restarts, seed, noise), "fab_u_l1",
                      lambda m, x, n: _n_classes(m, x, nclass), lambda x, K: _FabUL1Run(x, y, n_iter, eps, K, path), (y, eps), 1)
