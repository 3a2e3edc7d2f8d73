"""An independent float64 restatement of the start point of an APGD restart for the tests, one sample at a time,
with an explicit Philox4x32-10 of its own in Python integers.  Nothing here is shared with eeadv/apgdstart.py, eeadv/fabstart.py,
eeadv/sqatk.py, utils/attacks.py or eeadv/engine.py.

    philox(seed, ctr, stream)        the four 32-bit words of one call
    words(seed, b, D)                the words of row b under stream 16: call g covers elements 4 g .. 4 g + 3, counter (b << 32) | g
    draw_row(seed, b, D, metric)     t [D] float64: uniform on [-1, 1) (Linf), Box-Muller normals (L2, L1)
    l2_norm(t)                       sqrt(sum t^2) with math.fsum
    start_row(x0, eps, t, metric)    Linf clip(x0 + eps t, 0, 1);  L2 clip(x0 + t eps / (n + 1e-12), 0, 1), x0 when n is not finite;
                                     L1 x0 + t, not clipped
    merge(...)                       the union across restarts in numpy, row by row
"""
import math

import numpy as np

STREAM = 16
TAKEN = (0, 7, 11, 12, 13, 14, 15)  # the stream ids other draws of the library use
M32 = 0xFFFFFFFF
TWO_PI_F32 = float(np.float32(6.28318530717958647692))
TINY = float(np.float32(1e-12))


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


def l2_norm(t):
    a = [float(v) for v in t]
    if any(v != v for v in a):
        return float("nan")
    return math.sqrt(math.fsum(v * v for v in a))


def start_row(x0, eps, t, metric):
    """x0, t float64 [D]; eps a float.  The start point in float64."""
    x0, t = np.asarray(x0, dtype=np.float64), np.asarray(t, dtype=np.float64)
    if metric == "Linf":
        return np.clip(x0 + eps * t, 0.0, 1.0)
    if metric == "L1":
        return x0 + t
    if metric != "L2":
        raise ValueError(metric)
    n = l2_norm(t)
    if not math.isfinite(n):
        return x0.copy()
    return np.clip(x0 + t * (eps / (n + TINY)), 0.0, 1.0)


def start_f32(x0, eps, t, metric, n=None):
    """The kernel's own order in numpy float32, one rounding per operation: x0, t float32 [B, D].  n [B] float32: the L2 norms to use
    (default: sqrt of the float64 sum of squares, rounded once - exact-order-free on dyadic inputs)."""
    f = np.float32
    x0, t = np.asarray(x0, dtype=f), np.asarray(t, dtype=f)
    if metric == "Linf":
        return np.clip(x0 + f(eps) * t, f(0), f(1))
    if metric == "L1":
        return x0 + t
    if n is None:
        n = np.sqrt((t.astype(np.float64) ** 2).sum(axis=1)).astype(f)
    n = np.asarray(n, dtype=f)
    with np.errstate(all="ignore"):
        s = f(eps) / (n + f(1e-12))
        moved = np.clip(x0 + t * s[:, None], f(0), f(1))
    return np.where(np.isfinite(n)[:, None], moved, x0)


def merge(adv_all, robust_all, loss_all, x_best_adv, robust_run, loss_run, first):
    """The union across restarts on copies of the cumulative arrays; returns (adv_all, robust_all, loss_all).  Rows as uint32 bits."""
    adv_all, robust_all, loss_all = adv_all.copy(), robust_all.copy(), loss_all.copy()
    for b in range(adv_all.shape[0]):
        if first:
            robust_all[b], loss_all[b] = robust_run[b], loss_run[b]
            if robust_run[b] == 0:
                adv_all[b] = x_best_adv[b]
        else:
            if robust_all[b] != 0 and robust_run[b] == 0:
                adv_all[b] = x_best_adv[b]
                robust_all[b] = 0
            if loss_run[b] > loss_all[b]:
                loss_all[b] = loss_run[b]
    return adv_all, robust_all, loss_all
