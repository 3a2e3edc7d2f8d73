"""Logit rows on which a per-row loss kernel goes wrong, their float64 references and the bar that holds a kernel to them
(tests/test_loss_edges_host.py checks this module on the CPU, tests/test_gpu_loss_edges.py holds ee_loss.hip to it).

logits        FINITE cases, each for every (B, K) of BS x KS from a seeded generator: `tame` (randn * 3, what the rest of the suite draws),
              `wide` (randn * 1e3: expf underflows to exactly 0 for most classes), `offset` (randn * 3 + 1e4: only the max subtraction keeps
              it finite), `constant` (every row one value), `dominant` (one class 200 above the rest), `two_tied_max`.  `side` 0 is the
              row the kernels differentiate (z, zq), side 1 an independent draw of the same case (zp of the KL divergence).
poisoned      `tame` with ONE row (POISON_ROW[B]) poisoned: a single +inf, a single -inf, a row of -inf, a single NaN.
*_ref         float64 torch on the CPU, written from log_softmax.  kl_ref's dp is p * ((logp - logq) - kl), not autograd through F.kl_div:
              autograd is NaN where a target probability underflows, the limit - and what the kernel computes - is 0.
topk_ref      a stable restatement of ee_rows.hpp's order: value descending, ties to the lower index, NaN first.
sib_*         the sibling under the bar: oracle/ee_oracle.c (fp32 row arithmetic on the host) on the same inputs, its results in the
              format the kernel returns them in.  The C oracle has no label smoothing: the smoothed cross-entropy's sibling is its
              soft-target cross-entropy on the weights ee_ce_f32 forms (smooth_weights32).
within_bar    tests/test_gpu_attack_route.py's _twice_the_sibling with its constants: no further from float64 than twice the sibling,
              plus 1e-7 of the reference's largest entry.  Bar is the same over many cases.
"""
import numpy as np
import torch

from oracle import ee_oracle as O

KS = (1, 2, 63, 64, 65, 128, 129, 1000)  # around the 64-lane stride and twice it, and the reference's widest head
BS = (1, 3, 5, 9)                        # one wavefront per row, four rows per workgroup: 3, 5 and 9 leave a workgroup partly filled
FINITE = ("tame", "wide", "offset", "constant", "dominant", "two_tied_max")
POISON = ("pos_inf", "neg_inf", "all_neg_inf", "nan")
POISON_ROW = {1: 0, 3: 1, 5: 4, 9: 5}    # B = 3: inside a partly filled workgroup; B = 5: alone in the second; B = 9: inside a full one
SMOOTHING = float(np.float32(0.1))       # the kernel's argument is a float
UNDERFLOW_LOGP = -110.0                  # expf is exactly 0 below -103.98 (the smallest fp32 denormal), whatever the libm
NO_TOPK_SIBLING = ("nan",)               # orc_topk_i64 compares with `>` only, which never moves a NaN to the front (see the host test)


def _gen(case, B, K, side):
    return torch.Generator().manual_seed(1000003 * (FINITE + POISON).index(case) + 1009 * B + K + 7919 * side)


def logits(case, B, K, side=0):
    g = _gen(case, B, K, side)
    r = torch.randn(B, K, generator=g)
    rows = torch.arange(B)
    if case == "tame":
        z = r * 3
    elif case == "wide":
        z = r * 1e3
    elif case == "offset":
        z = r * 3 + 1e4
    elif case == "constant":
        z = (1.5 * rows - 2.0 + 0.25 * side).view(B, 1).expand(B, K).clone()
    elif case == "dominant":
        z = r * 3
        z[rows, (7 * rows + 3 + 5 * side) % K] = z.max(1).values + 200.0
    elif case == "two_tied_max":
        z = r * 3
        c1 = (3 * rows + 1 + side) % K
        top = z.max(1).values + 1.0
        z[rows, c1] = top
        z[rows, (c1 + max(K // 2, 1)) % K] = top
    else:
        raise KeyError(case)
    return z.float().contiguous()


def labels(B, K):
    return torch.randint(0, K, (B,), generator=torch.Generator().manual_seed(31 * B + K))


def soft_targets(B, K):
    """float64 rows summing to 1; row 0 has exact zeros at every other class (K >= 2)"""
    t = torch.rand(B, K, generator=torch.Generator().manual_seed(77 * B + K), dtype=torch.float64) + 0.05
    t[0, 1::2] = 0.0
    return t / t.sum(1, keepdim=True)


def poisoned(kind, B, K, side=0):
    """(logits, row): the `tame` logits of this shape with row POISON_ROW[B] poisoned"""
    z, row = logits("tame", B, K, side), POISON_ROW[B]
    col = (2 * K) // 3
    if kind == "pos_inf":
        z[row, col] = float("inf")
    elif kind == "neg_inf":
        z[row, col] = float("-inf")
    elif kind == "all_neg_inf":
        z[row] = float("-inf")
    elif kind == "nan":
        z[row, col] = float("nan")
    else:
        raise KeyError(kind)
    return z, row


# ---- float64 references ----------------------------------------------------------------------------------------------------------------
def smooth_weights64(y, K, smoothing):
    w = torch.full((y.numel(), K), smoothing / (K - 1.0) if smoothing else 0.0, dtype=torch.float64)
    w[torch.arange(y.numel()), y] = 1.0 - smoothing
    return w


def smooth_weights32(y, K, smoothing):
    """the weights as ee_ce_f32 forms them: smoothing / (float(K) - 1) and 1 - smoothing, each one fp32 operation"""
    s = np.float32(smoothing)
    w = torch.full((y.numel(), K), float(s / (np.float32(K) - np.float32(1.0))) if smoothing else 0.0, dtype=torch.float32)
    w[torch.arange(y.numel()), y] = float(np.float32(1.0) - s)
    return w


def ce_ref(z, y, reduction="sum", smoothing=0.0):
    """(loss, dlogits, logp), float64"""
    B, K = z.shape
    lp = torch.log_softmax(z.double(), 1)
    w = smooth_weights64(y, K, smoothing)
    if smoothing:
        rows = -(w * lp).sum(1)
    else:
        rows = -lp[torch.arange(B), y]  # not a product with the one-hot row: 0 * -inf is NaN
    gscale = 1.0 / B if reduction == "mean" else 1.0
    return gscale * rows.sum(), gscale * (lp.exp() - w), lp


def kl_ref(zq, zp):
    """KLDivLoss('batchmean')(log_softmax(zq), softmax(zp)): (loss, dq, dp, logp), float64"""
    B = zq.shape[0]
    logq, logp = torch.log_softmax(zq.double(), 1), torch.log_softmax(zp.double(), 1)
    p, q = logp.exp(), logq.exp()
    kl = torch.where(p > 0, p * (logp - logq), torch.zeros_like(p)).sum(1, keepdim=True)
    return kl.sum() / B, (q - p) / B, p * ((logp - logq) - kl) / B, logp


def softce_ref(z, t, scale):
    lp = torch.log_softmax(z.double(), 1)
    return -(lp * t).sum() * scale, scale * (lp.exp() * t.sum(1, keepdim=True) - t), lp


def mse_ref(a, b):
    d = a.double() - b.double()
    return (d * d).mean(), 2.0 * d / d.numel()


def topk_ref(z, y, k):
    """(idx [B, k], correct [k]) in ee_rows.hpp's order"""
    v = z.double().numpy()
    nan = np.isnan(v)
    key = np.where(nan, 0.0, -v)
    idx = np.stack([np.lexsort((np.arange(v.shape[1]), key[b], ~nan[b]))[:k] for b in range(v.shape[0])]).astype(np.int64)
    hit = idx == np.asarray(y).reshape(-1, 1)
    return idx, np.cumsum(hit, 1).astype(bool).sum(0).astype(np.int64)


# ---- the sibling: the fp32 C oracle, results in the kernel's output format ----------------------------------------------------------------
def _f32(v):
    return torch.tensor(float(np.float32(v)), dtype=torch.float64)


def sib_ce(z, y, reduction="sum", smoothing=0.0):
    B, K = z.shape
    if smoothing:
        v, d = O.softce(z.numpy(), smooth_weights32(y, K, smoothing).double().numpy(), 1.0 / B if reduction == "mean" else 1.0)
        return _f32(v), torch.from_numpy(d.astype(np.float32))
    v, d = O.ce(z.numpy(), y.numpy(), mean=reduction == "mean")
    return _f32(v), torch.from_numpy(d)


def sib_kl(zq, zp):
    v, dq, dp = O.kl_batchmean(zq.numpy(), zp.numpy())
    return _f32(v), torch.from_numpy(dq), torch.from_numpy(dp)


def sib_softce(z, t, scale):
    v, d = O.softce(z.numpy(), t.numpy(), scale)
    return torch.tensor(v, dtype=torch.float64), torch.from_numpy(d)


def sib_mse(a, b):
    v, d = O.mse(a.numpy(), b.numpy())
    return _f32(v), torch.from_numpy(d)


def sib_topk(z, y, k):
    return O.topk(z.numpy(), y.numpy(), k)


# ---- the bar ---------------------------------------------------------------------------------------------------------------------------
def _err(a, ref):
    return float((torch.as_tensor(a).detach().cpu().double() - ref).abs().max())


def bar_figures(got, sibling, ref, floor=1e-7):
    """(kernel error, sibling error, max |ref|, allowed)"""
    ref = torch.as_tensor(ref).double()
    e_g, e_s, top = _err(got, ref), _err(sibling, ref), float(ref.abs().max())
    return e_g, e_s, top, 2 * e_s + floor * top


def within_bar(got, sibling, ref, what, floor=1e-7):
    e_g, e_s, top, allowed = bar_figures(got, sibling, ref, floor)
    print("    %-60s kernel %.3e  sibling %.3e  of max |ref| %.3e" % (what, e_g, e_s, top))
    assert e_g <= allowed, "%s: %.3e from float64, the sibling %.3e (max |ref| %.3e)" % (what, e_g, e_s, top)


class Bar:
    """the bar over many cases: check() records, finish() prints per output the case that came closest to its bar and every case beyond
    it, and fails if there is one - so a failure names every (case, K, B) that caused it.  `floors`: {(name, tag): the share of the
    reference's largest entry allowed next to twice the sibling, where it is not 1e-7}"""

    def __init__(self, floors=None):
        self.worst, self.failed, self.floors = {}, [], floors or {}

    def check(self, got, sibling, ref, name, tag):
        e_g, e_s, top, allowed = bar_figures(got, sibling, ref, self.floors.get((name, tag), 1e-7))
        line = "%-24s %-36s kernel %.3e  sibling %.3e  of max |ref| %.3e" % (name, tag, e_g, e_s, top)
        ratio = e_g / allowed if allowed > 0 else (0.0 if e_g == 0 else float("inf"))
        if name not in self.worst or ratio >= self.worst[name][0]:
            self.worst[name] = (ratio, line)
        if not e_g <= allowed:
            self.failed.append(line + "  (allowed %.3e)" % allowed)

    def finish(self):
        print()
        for name in sorted(self.worst):
            print("    " + self.worst[name][1])
        for line in self.failed:
            print("    BEYOND THE BAR: " + line)
        assert not self.failed, "%d beyond the bar, the first: %s" % (len(self.failed), self.failed[0])


# ---- inputs of the mean-squared error ----------------------------------------------------------------------------------------------------
MSE_NS = (1, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 5)  # around the 256-thread stride and the 4096-element chunk of a workgroup
MSE_KINDS = ("randn", "const", "big")


def mse_inputs(kind, n):
    g = torch.Generator().manual_seed(n + 17 * MSE_KINDS.index(kind))
    if kind == "randn":
        return (torch.randn(n, generator=g) * 3).float(), (torch.randn(n, generator=g) * 3).float()
    if kind == "const":  # a - b is the same fp32 number, 1e-3 rounded once, at every element
        return torch.full((n,), 1e-3, dtype=torch.float32), torch.zeros(n, dtype=torch.float32)
    if kind == "big":  # |a - b| up to 1e4
        return ((torch.rand(n, generator=g) - 0.5) * 1e4).float(), ((torch.rand(n, generator=g) - 0.5) * 1e4).float()
    raise KeyError(kind)
