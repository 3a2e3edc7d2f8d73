"""Survivor-only attack cascade over a whole validation split: clean -> APGD-CE -> APGD-T -> FAB-T -> Square.

A sample enters a stage only if it is still correctly classified after every stage before it.  The attack loops replay captured graphs of
ONE batch shape, so "only the survivors" is not a boolean index per batch: the survivors of several validation batches are regrouped into
full batches of the captured shape.  Every stage has a pool of rows (image, label, global sample id, clean-logit class order) in HBM;
whenever a pool holds a full batch it is popped, attacked by the stage's unchanged loop (utils.attacks.APGD / APGD_T / FAB_T / Square),
what the stage broke is recorded by sample id and its survivors are appended to the next stage's pool.  After the last incoming batch the
pools are flushed in stage order; a flushed batch is padded with copies of the pool's first row, which never reach the result.  The
classifier runs in eval mode, so a sample's trajectory does not depend on who shares its batch (sections 11, 12) - except through the
random draws, which stay what each attack draws today, per popped batch (nothing is keyed by the global id).

Host reads: the host decides when to pop, so it reads a pool's count once per append - 4 bytes; nothing is added inside the attack loops.

compaction="hip" (the default on a ROCm device) runs the pools as HIP kernels (csrc/ee_cascade.hip); compaction="torch" (the default for
CPU tensors, what --no-cuda takes) states the same staging with index_select, and feeds identical batches to identical loops.
"""
import collections
import types

import torch

import utils.attacks as A

from . import methods, ops, runtime

STAGES = methods.PLANS["Cascade"].members

# A stage description: a member of eeadv.methods and, optionally, the restart count of that stage alone.  A bare
# member name is Stage(name): no count of its own, the stage takes what _restarts(args) gave the whole list.
Stage = collections.namedtuple("Stage", "member restarts", defaults=(None,))


def _stages(members, ctx):
    """[(name, fn)] of `members` (eeadv.methods; names or Stage tuples), the stage named as its member; fn(model, args, x, y, order) ->
    (x_adv, robust) runs it on one full batch with `ctx`, which holds what the builder read from ITS args, plus the batch's `order`.  A
    Stage with a restart count runs with that count in the place of ctx's APGD and FAB counts (one restart: no keyword, as everywhere)."""
    def stage(member, restarts):
        own = vars(ctx)
        if restarts is not None:
            if int(restarts) < 1:
                raise ValueError("stage %s: restarts must be at least 1, got %d" % (member, int(restarts)))
            kw = {} if int(restarts) == 1 else {"n_restarts": int(restarts)}
            own = dict(own, akw=kw, rkw=kw)
        return lambda model, a, x, y, order: methods.MEMBERS[member](model, a, x, y, types.SimpleNamespace(order=order, **own))
    members = [Stage(m) if isinstance(m, str) else Stage(*m) for m in members]
    return [(s.member, stage(s.member, s.restarts)) for s in members]


def _restarts(args):
    """The APGD and FAB restart counts of args (default 1; DESIGN.md sections 24, 23) as the context's keywords: nothing for one restart."""
    return {"akw": methods.restarts_kw(args, "apgd_restarts", "apgd_restarts"), "rkw": methods.restarts_kw(args, "fab_restarts", "fab_restarts")}


def default_stages(args, num_steps, n_class, n_target_classes=9, norm="Linf"):
    """[(name, fn)] of AutoAttack's `standard` order; fn(model, args, x, y, order) -> (x_adv, robust) runs one stage on one full batch, `order`
    being the class order of the clean logits [B, n_t + 1] (the targets of APGD-T and FAB-T: no clean forward of their own).  norm: 'Linf'
    (the default: the calls made before the parameter existed) or 'L2' - every stage then runs in the L2 ball of radius args.epsilon
    (DESIGN.md sections 16 - 18), so evaluate(..., stages=default_stages(..., norm="L2")) is the L2 `standard` cascade."""
    return _stages(STAGES, methods.context(args, num_steps, n_class, nkw=A._norm_kw(norm), n_target_classes=n_target_classes, **_restarts(args)))


def l1_stages(args, num_steps, n_class, n_target_classes=9):
    """[(name, fn)] of the `standard` order in the L1 threat model, radius args.epsilon: APGD-L1-CE, APGD-T-L1, FAB-T-L1, Square-L1 through
    the L1 doors of utils.attacks (DESIGN.md sections 19 to 21), so evaluate(..., stages=l1_stages(...)) is the L1 `standard` cascade.
    default_stages(norm="L1") stays refused."""
    return _stages(methods.PLANS["APGD-L1+FAB+Square"].members,
                   methods.context(args, num_steps, n_class, n_target_classes=n_target_classes, **_restarts(args)))


def rand_stages(args, num_steps, eot_iter=None, norm="Linf"):
    """[(name, fn)] of the public ensemble's `rand` order for randomised defences: APGD-CE, then APGD-DLR on its survivors, every gradient
    averaged over eot_iter forwards (default args.eot_iter, else 20).  norm: 'Linf' or 'L2', for both stages
    (DESIGN.md section 16)."""
    plan = methods.PLANS["Cascade-Rand"]
    kw = A._norm_kw(norm)  # empty for Linf
    E = eot_iter if eot_iter is not None else getattr(args, "eot_iter", None)
    E = plan.eot if E is None else int(E)
    if E < 1:
        raise ValueError("the rand stages need eot_iter >= 1, got %d" % E)
    return _stages(plan.members, methods.context(args, num_steps, None, E, kw, methods.restarts_kw(args, "apgd_restarts", "apgd_restarts")))


# ---- the four versions of the reference's utils/aa.py as stage lists -------------------------------------------------
# version -> norms it exists for.  `plus`: the six attacks of the public ensemble's plus order, the untargeted ones with 5 restarts;
# `custom`: the reference's own setting (attacks_to_run = ['apgd-ce', 'fab'], 2 restarts each), here on the survivors.
AA_VERSIONS = {"standard": ("Linf", "L2", "L1"), "plus": ("Linf", "L2"), "rand": ("Linf", "L2"), "custom": ("Linf", "L2")}
AA_PLUS = (Stage("APGD-CE", 5), Stage("APGD-DLR", 5), Stage("FAB-U", 5), Stage("Square"), Stage("APGD-T", 1), Stage("FAB-T", 1))
AA_CUSTOM = (Stage("APGD-CE", 2), Stage("FAB-U", 2))
AA_DLR_CLASSES = 4  # the class count `plus` and `rand` ask for: the DLR loss reads the third and fourth largest logit


def aa_stages(args, num_steps, n_class, version, norm="Linf"):
    """[(name, fn)] of `version` ('standard', 'plus', 'rand', 'custom') of the reference's utils/aa.py under `norm`, radius args.epsilon:
        standard  default_stages (Linf, L2) / l1_stages (L1), unchanged - args.apgd_restarts / args.fab_restarts as there
        plus      APGD-CE (5 restarts), APGD-DLR (5), FAB-U (5), Square, APGD-T (1), FAB-T (1); Linf, L2
        rand      rand_stages: APGD-CE, APGD-DLR, every gradient over args.eot_iter forwards (default 20); Linf, L2
        custom    APGD-CE (2), FAB-U (2); Linf, L2
    with args.n_target_classes (default 9) targets at most.  A combination outside the table stops with the nearest one that exists; `plus`
    and `rand` stop below four classes."""
    if version not in AA_VERSIONS:
        raise ValueError("version must be one of %s, got %r" % (", ".join(AA_VERSIONS), version))
    if norm not in AA_VERSIONS["standard"]:
        raise ValueError("norm must be one of %s, got %r" % (", ".join(AA_VERSIONS["standard"]), norm))
    if norm not in AA_VERSIONS[version]:
        raise NotImplementedError("version %s exists under %s, not under %s; the nearest supported combination is version standard under %s"
                                  % (version, " and ".join(AA_VERSIONS[version]), norm, norm))
    if version in ("plus", "rand") and int(n_class) < AA_DLR_CLASSES:
        raise ValueError("version %s runs APGD-DLR, whose loss reads the third and fourth largest logit: it needs at least %d classes and this "
                         "model has %d" % (version, AA_DLR_CLASSES, int(n_class)))
    n_t = min(int(getattr(args, "n_target_classes", 9)), int(n_class) - 1)
    if version == "standard":
        return l1_stages(args, num_steps, n_class, n_t) if norm == "L1" else default_stages(args, num_steps, n_class, n_t, norm)
    if version == "rand":
        return rand_stages(args, num_steps, None, norm)
    return _stages(AA_PLUS if version == "plus" else AA_CUSTOM,
                   methods.context(args, num_steps, n_class, nkw=A._norm_kw(norm), n_target_classes=n_t, **_restarts(args)))


def individual(model, args, batches, n_class, stages, device=None, before_member=None):
    """Every stage of `stages` on ALL samples of `batches`, one member after the other (the --individual mode of utils/aa.py): {name:
    (adv [n, ...], robust [n] bool)}, adv being what the member's door returns for each whole batch.  before_member(name), if given, runs
    before a member's first batch (the script reseeds there, so that each entry can be reproduced on its own).  The class order of the
    clean logits is taken once per batch, as the cascade takes it; the model is expected in eval mode."""
    if iter(batches) is batches:
        batches = list(batches)
    K = min(int(getattr(args, "n_target_classes", 9)), int(n_class) - 1) + 1
    rows = []
    for x, y in batches:
        if device is not None:
            x, y = x.to(device), y.to(device)
        x, y = x.detach(), y.contiguous()
        with torch.no_grad():
            z = model(x)
        if runtime.require_device(x, "cascade"):
            order = ops.topk(z.detach().float().contiguous(), None, K)[0]
        else:
            order = torch.sort(z, dim=1, descending=True, stable=True)[1][:, :K].contiguous()
        rows.append((x, y, order))
    if not rows:
        raise ValueError("the evaluation needs at least one sample")
    out = {}
    for name, fn in stages:
        if before_member is not None:
            before_member(name)
        res = [fn(model, args, x, y, order) for x, y, order in rows]
        out[name] = (torch.cat([xa.detach() for xa, _ in res]), torch.cat([rb for _, rb in res]))
    return out


class _Rows:
    """x [n, D], y [n], ids [n], order [n, K]: the fields of n pool rows (a pool's store, or the batch a pop fills)."""

    def __init__(self, n, D, K, dtype, device):
        self.x = torch.zeros((n, D), dtype=dtype, device=device)
        self.y = torch.zeros(n, dtype=torch.int64, device=device)
        self.ids = torch.zeros(n, dtype=torch.int64, device=device)
        self.order = torch.zeros((n, K), dtype=torch.int64, device=device)

    def fields(self):
        return self.x, self.y, self.ids, self.order


class _HipPool:
    """cap = 2 B rows in HBM and their count on the device (csrc/ee_cascade.hip); `count` is the host's copy of it."""

    def __init__(self, B, D, K, dtype, device):
        if dtype != torch.float32:
            raise TypeError("the device pools hold float32 images, got %s" % dtype)
        self.B, self.rows, self.count = B, _Rows(2 * B, D, K, dtype, device), 0
        self.count_dev = torch.zeros(1, dtype=torch.int32, device=device)

    def append(self, x, y, ids, order, keep):
        ops.pool_append_(x, y, ids, order, keep, *self.rows.fields(), self.count_dev)
        self.count = int(self.count_dev.item())  # THE host read of the cascade: 4 bytes per append, to decide when to pop
        return self.count

    def pop(self, batch):
        ops.pool_pop_(*self.rows.fields(), self.count_dev, *batch.fields())
        self.count = max(self.count - self.B, 0)  # what the count launch computes: no read


class _TorchPool:
    """The same pool in torch ops (index_select): the host path, and the statement the device pools are tested against."""

    def __init__(self, B, D, K, dtype, device):
        self.B, self.rows, self.count = B, _Rows(2 * B, D, K, dtype, device), 0

    def append(self, x, y, ids, order, keep):
        idx = torch.nonzero(keep.view(-1).to(torch.bool)).view(-1)
        k = int(idx.numel())  # the same read: the number of kept rows
        for dst, src in zip(self.rows.fields(), (x, y, ids, order)):
            dst[self.count:self.count + k] = src.index_select(0, idx)
        self.count += k
        return self.count

    def pop(self, batch):
        B, c = self.B, self.count
        idx = torch.arange(B, device=self.rows.x.device)
        idx = torch.where(idx < c, idx, torch.zeros_like(idx))  # padding: the pool's row 0
        for dst, src in zip(batch.fields(), self.rows.fields()):
            dst.copy_(src.index_select(0, idx))
            if c > B:
                src[:c - B] = src[B:c].clone()
        self.count = max(c - B, 0)


def _resolve_torch(robust, ids, x_adv, n_valid, stage, robust_out, stage_out, adv_out, keep):
    valid = torch.arange(robust.shape[0], device=robust.device) < n_valid
    broken = ids[valid & ~robust]
    robust_out[broken] = False
    stage_out[broken] = stage
    if adv_out is not None:
        adv_out[broken] = x_adv[valid & ~robust]
    keep.copy_(valid & robust)
    return keep


def _free_bytes(device):
    """Bytes a new tensor on `device` could take: what the driver reports free plus what torch's allocator holds unused.  None on the host."""
    if device.type != "cuda":
        return None
    free, _ = torch.cuda.mem_get_info(device)
    return free + torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)


def _count_samples(batches):
    return sum(int(y.shape[0]) for _, y in batches)


class _Run:
    """One cascade: the pools, the one batch a pop fills, and the result arrays - everything sized by the first batch."""

    def __init__(self, model, args, stages, x, N, K, keep_adv, compaction, batch_size=None):
        self.model, self.args, self.stages = model, args, stages
        self.on_dev = runtime.require_device(x, "cascade")
        mode = compaction or ("hip" if self.on_dev else "torch")
        if mode not in ("hip", "torch"):
            raise ValueError("compaction must be 'hip' or 'torch', got %r" % (compaction,))
        if mode == "hip" and not self.on_dev:
            raise RuntimeError("compaction='hip' needs the batches on a ROCm device; the host path is compaction='torch'")
        B, D, dev, S = int(batch_size or x.shape[0]), x[0].numel(), x.device, len(stages)
        if not 1 <= B <= 4096:
            raise ValueError("the cascade takes batches of 1 .. 4096 samples, got %d" % B)
        if keep_adv:
            free, need = _free_bytes(dev), (N + S * 2 * B + B) * D * x.element_size()
            if free is not None and need > free:
                raise MemoryError("keep_adv needs %.1f GiB on %s for the adversarial points of %d samples of %d values next to the pools, "
                                  "%.1f GiB are free alongside the model: evaluate without keep_adv, or over a smaller split"
                                  % (need / 2 ** 30, dev, N, D, free / 2 ** 30))
        self.B, self.D, self.K, self.N, self.shape, self.dev = B, D, K, N, tuple(x.shape[1:]), dev
        pool_cls = _HipPool if mode == "hip" else _TorchPool
        self.resolve = ops.cascade_resolve_ if mode == "hip" else _resolve_torch
        self.pools = [pool_cls(B, D, K, x.dtype, dev) for _ in range(S)]
        self.batch = _Rows(B, D, K, x.dtype, dev)
        self.robust = torch.ones(N, dtype=torch.bool, device=dev)
        self.stage = torch.full((N,), S + 1, dtype=torch.int32, device=dev)
        self.adv = torch.zeros((N, D), dtype=x.dtype, device=dev) if keep_adv else None
        self.keep = torch.zeros(B, dtype=torch.bool, device=dev)
        self.rows, self.runs, self.seen = [0] * S, [0] * S, 0

    def clean(self, x, y):
        """The clean stage of one incoming batch: one forward, the class order once, the correct rows into the first pool."""
        b = int(x.shape[0])
        if b > self.B or tuple(x.shape[1:]) != self.shape:
            raise ValueError("batch of shape %s after a first batch of %s: the cascade runs one batch shape"
                             % (tuple(x.shape), (self.B,) + self.shape))
        if self.seen + b > self.N:
            raise ValueError("more samples than n = %d" % self.N)
        with torch.no_grad():
            z = self.model(x)
        if self.on_dev:
            order = ops.topk(z.detach().float().contiguous(), None, self.K)[0]
        else:
            order = torch.sort(z, dim=1, descending=True, stable=True)[1][:, :self.K].contiguous()
        y = y.contiguous()
        ids = torch.arange(self.seen, self.seen + b, dtype=torch.int64, device=self.dev)
        x2 = x.reshape(b, self.D).contiguous()
        keep = torch.zeros(b, dtype=torch.bool, device=self.dev)
        self.resolve((order[:, 0] == y).contiguous(), ids, x2, b, 0, self.robust, self.stage, None, keep)
        if self.adv is not None:
            self.adv[self.seen:self.seen + b] = x2
        self.seen += b
        if self.pools:
            self.pools[0].append(x2, y, ids, order, keep)
            self.drain(0)

    def run_stage(self, s):
        pool, batch, B = self.pools[s], self.batch, self.B
        n_valid = min(pool.count, B)
        pool.pop(batch)
        x_adv, robust = self.stages[s][1](self.model, self.args, batch.x.view((B,) + self.shape), batch.y, batch.order)
        self.resolve(robust.contiguous(), batch.ids, x_adv.detach().reshape(B, self.D).contiguous(), n_valid, s + 1, self.robust, self.stage,
                     self.adv, self.keep)
        self.rows[s] += n_valid
        self.runs[s] += 1
        if s + 1 < len(self.pools):
            self.pools[s + 1].append(*batch.fields(), self.keep)  # the CLEAN rows: every stage starts from the sample itself
            self.drain(s + 1)

    def drain(self, s, flush=False):
        while self.pools[s].count >= self.B or (flush and self.pools[s].count > 0):
            self.run_stage(s)


def evaluate(model, args, batches, n_class, keep_adv=False, compaction=None, stages=None, num_steps=None, n=None, device=None, batch_size=None,
             per_stage_adv=False):
    """Runs the cascade over `batches`, a re-iterable of (x [b, ...], y [b] int64) with b <= B = `batch_size` (default: the size of the first
    batch), the one shape the attack loops capture; the model is expected in eval mode.  `n`: the number of samples if known (else the batches are counted
    in a pass of their own); `device`: where the batches are moved to (default: where they are); `num_steps`: APGD's iterations
    (default args.num_steps_1); args.epsilon, args.fab_iters, args.square_queries and args.n_target_classes (default 9) as for the
    attacks.  `stages`, a list of (name, fn) as default_stages gives, replaces the attacks (tests script them).

    Returns a namespace: n, clean_correct, robust [n] bool and stage [n] int32 indexed by global sample id (the position in the
    iteration order; stage 0 = misclassified clean, k = broken by stage k, len(stages) + 1 = survived), stage_names,
    robust_after [per stage: samples still robust after it], rows_attacked [per stage: rows it ran on, padding excluded],
    batches_attacked [per stage] and adv [n, ...] (keep_adv: the clean sample where robust or misclassified clean, else the point that
    broke it; None otherwise).  per_stage_adv (needs keep_adv): also stage_adv, per stage a namespace (name, ids [k] int64 ascending, adv
    [k, ...]) of the samples that stage broke and the points that broke them - rows of adv, which is resolved by sample id already: no launch
    of its own."""
    if per_stage_adv and not keep_adv:
        raise ValueError("per_stage_adv reads the kept points: it needs keep_adv=True")
    if iter(batches) is batches:
        batches = list(batches)
    N = int(n) if n is not None else _count_samples(batches)
    if N < 1:
        raise ValueError("the cascade needs at least one sample")
    n_t = min(int(getattr(args, "n_target_classes", 9)), int(n_class) - 1)
    if stages is None:
        if num_steps is None:
            num_steps = args.num_steps_1
        stages = default_stages(args, int(num_steps), n_class, n_t)
    S = len(stages)
    run = None
    for x, y in batches:
        if device is not None:
            x, y = x.to(device), y.to(device)
        x = x.detach()
        if run is None:
            run = _Run(model, args, stages, x, N, n_t + 1, keep_adv, compaction, batch_size)
        run.clean(x, y)
    if run.seen != N:
        raise ValueError("%d samples came, n = %d" % (run.seen, N))
    for s in range(S):
        run.drain(s, flush=True)

    counts = torch.bincount(run.stage.to(torch.int64), minlength=S + 2).tolist()  # one read at the end
    clean_correct = N - counts[0]
    robust_after, left = [], clean_correct
    for s in range(S):
        left -= counts[s + 1]
        robust_after.append(left)
    res = types.SimpleNamespace(n=N, clean_correct=clean_correct, robust=run.robust, stage=run.stage, stage_names=[name for name, _ in stages],
                                robust_after=robust_after, rows_attacked=run.rows, batches_attacked=run.runs,
                                adv=None if run.adv is None else run.adv.view((N,) + run.shape))
    if per_stage_adv:
        res.stage_adv = []
        for s, (name, _) in enumerate(stages):
            ids = torch.nonzero(run.stage == s + 1).view(-1)
            res.stage_adv.append(types.SimpleNamespace(name=name, ids=ids, adv=res.adv.index_select(0, ids)))
    return res
