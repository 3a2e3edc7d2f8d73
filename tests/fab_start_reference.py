"""An independent float64 restatement of the FAB restarts for the tests: the random start of a restart, one sample
at a time, with an explicit Philox4x32-10 of its own in Python integers.  Nothing here is shared with eeadv/fabstart.py, eeadv/sqatk.py,
utils/attacks.py or eeadv/engine.py; the iteration between two starts is the one of tests/fab_reference.py, fab_l2_reference.py,
fab_l1_reference.py (targeted) and fab_u_reference.py (untargeted).

    philox(seed, ctr, stream)            the four 32-bit words of one call
    words(seed, b, D)                    the words of row b: call g covers elements 4 g .. 4 g + 3 under the counter (b << 32) | g
    draw_row(seed, b, D, metric)         t [D] float64: uniform on [-1, 1) (Linf), Box-Muller normals (L2, L1)
    norm(t, metric)                      max |t| (Linf), sqrt(sum t^2) (L2), sum |t| (L1), with math.fsum
    start_row(x0, res, eps, t, metric)   clip(x0 + ((m t) / n) / 2, 0, 1), m = min(res, eps); x0 when n is 0 or not finite
    chain(model, x0, y, t, n_iter, n_restarts, eps, noise, metric)   restart 0 from the clean point, then the restarts, res and adv carried
"""
import math

import numpy as np
import torch

import fab_l1_reference
import fab_l2_reference
import fab_reference
import fab_u_reference

REFS = {"Linf": fab_reference, "L2": fab_l2_reference, "L1": fab_l1_reference}
STREAM = 15
M32 = 0xFFFFFFFF
TWO_PI_F32 = float(np.float32(6.28318530717958647692))


def philox(seed, ctr, stream):
    """Philox4x32-10: key = the two halves of seed, counter = (ctr low, ctr high, stream, 0)."""
    k0, k1 = seed & M32, (seed >> 32) & M32
    c = [ctr & M32, (ctr >> 32) & M32, stream & M32, 0]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M32, (p0 >> 32) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c


def words(seed, b, D):
    return [philox(seed, (b << 32) | g, STREAM) for g in range((D + 3) // 4)]


def _u(word):
    return (word >> 8) / 16777216.0  # 24 bits: exact in float32 and float64


def draw_row(seed, b, D, metric):
    """Row b of the draw, float64 [D].  Linf: 2 u - 1 per word.  L2 / L1: per call the pairs (words 0, 1) and (words 2, 3),
    sqrt(-2 log(1 - u_a)) (cos, sin)(a) with a = float32(float32(2 pi) u_b) - the one float32 rounding the kernel's angle has."""
    out = []
    for w in words(seed, b, D):
        if metric == "Linf":
            out += [2.0 * _u(v) - 1.0 for v in w]
        else:
            for wa, wb in ((w[0], w[1]), (w[2], w[3])):
                rad = math.sqrt(-2.0 * math.log(1.0 - _u(wa)))
                ang = float(np.float32(TWO_PI_F32 * _u(wb)))  # the product of two float32 values is exact in float64: one rounding
                out += [rad * math.cos(ang), rad * math.sin(ang)]
    return np.asarray(out[:D], dtype=np.float64)


def norm(t, metric):
    a = [abs(float(v)) for v in t]
    if any(v != v for v in a):
        return float("nan")
    if metric == "Linf":
        return max(a)
    if metric == "L2":
        return math.sqrt(math.fsum(v * v for v in a))
    if metric == "L1":
        return math.fsum(a)
    raise ValueError(metric)


def start_row(x0, res, eps, t, metric):
    """x0, t float64 [D]; res, eps floats.  The start in float64."""
    n = norm(t, metric)
    if not math.isfinite(n) or n == 0.0:
        return np.array(x0, dtype=np.float64)
    m = min(res, eps)
    return np.clip(np.asarray(x0, dtype=np.float64) + ((m * np.asarray(t, dtype=np.float64)) / n) * 0.5, 0.0, 1.0)


def dist(v, metric):
    return norm(v, metric)


def chain(model, x0, y, t, n_iter, n_restarts, eps, noise, metric):
    """The chain of n_restarts runs of n_iter iterations, sample by sample, in float64.  t: the target classes [B] of a targeted run, or None
    for untargeted FAB.  noise float64 [n_restarts - 1, B, ...].  Returns (adv, res, restarts): restarts[r] = dict(x_start [B, ...],
    res_in [B], trace) with trace in the layout of fab_reference.run."""
    B = x0.shape[0]
    advs = [x0[b:b + 1].clone() for b in range(B)]
    ress = [math.inf] * B
    restarts = []
    for r in range(n_restarts):
        res_in = list(ress)
        if r == 0:
            xs = [x0[b:b + 1].clone() for b in range(B)]
        else:
            xs = [torch.from_numpy(start_row(x0[b].reshape(-1).numpy(), ress[b], eps, noise[r - 1, b].reshape(-1).numpy(), metric)).view(x0[b:b + 1].shape)
                  for b in range(B)]
        x_start = torch.cat(xs)
        trace = []
        for _ in range(n_iter):
            rows = []
            for b in range(B):
                if t is None:
                    e = fab_u_reference.iterate(model, xs[b], x0[b:b + 1], int(y[b]), advs[b], ress[b], metric)
                else:
                    e = REFS[metric].iterate(model, xs[b], x0[b:b + 1], int(y[b]), int(t[b]), advs[b], ress[b])
                e.update(x_in=xs[b], adv_in=advs[b], res_in=ress[b])
                xs[b], advs[b], ress[b] = e["x"], e["adv"], e["res"]
                rows.append(e)
            entry = {}
            for key in rows[0]:
                vals = [e[key] for e in rows]
                if isinstance(vals[0], torch.Tensor):
                    entry[key] = torch.cat(vals)
                else:
                    entry[key] = torch.tensor(vals, dtype=torch.float64 if isinstance(vals[0], float) else None)
            trace.append(entry)
        restarts.append(dict(x_start=x_start, res_in=torch.tensor(res_in, dtype=torch.float64), trace=trace))
    return torch.cat(advs), torch.tensor(ress, dtype=torch.float64), restarts
