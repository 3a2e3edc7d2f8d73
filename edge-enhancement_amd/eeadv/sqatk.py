"""Host-side pieces of the Square attack (csrc/ee_sqatk.hip): the p schedule shared with the Add_Square defence, and
a vectorised numpy Philox4x32-10 that makes the kernels' draws - same key, counters and stream ids - for the plain-torch host path."""
import math

import numpy as np

STREAM_WINDOW, STREAM_STRIPE = 11, 12  # kStreamWindow / kStreamStripe of ee_sqatk.hip; 0 and 7 belong to other kernels
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def p_selection(it, p_init, n_queries=None):
    """The piecewise-constant schedule of the fraction p of pixels a proposal changes (utils/core.py Add_Square.p_selection, core.py:607-634):
    p_init halved after iterations 10, 50, 200, 500, 1000, 2000, 4000, 6000, 8000.  With n_queries the iteration is first rescaled to a
    run of 10000 (`rescale_schedule`)."""
    if n_queries is not None:
        it = int(it / n_queries * 10000)
    if 10 < it <= 50:
        p = p_init / 2
    elif 50 < it <= 200:
        p = p_init / 4
    elif 200 < it <= 500:
        p = p_init / 8
    elif 500 < it <= 1000:
        p = p_init / 16
    elif 1000 < it <= 2000:
        p = p_init / 32
    elif 2000 < it <= 4000:
        p = p_init / 64
    elif 4000 < it <= 6000:
        p = p_init / 128
    elif 6000 < it <= 8000:
        p = p_init / 256
    elif 8000 < it:
        p = p_init / 512
    else:
        p = p_init
    return p


def square_schedule(n_queries, H, W, p_init=0.8):
    """Window edge of each of the n_queries - 1 proposals: s_i = clamp(int(round(sqrt(p(i) * H * W))), 1, min(H, W)), p rescaled."""
    n_queries = int(n_queries)
    if n_queries < 1:
        raise ValueError("Square needs n_queries >= 1")
    return [min(max(int(round(math.sqrt(p_selection(i, p_init, n_queries) * H * W))), 1), min(H, W)) for i in range(n_queries - 1)]


def philox4x32(seed, ctr, stream_id):
    """Philox4x32-10 as csrc/ee_common.hpp keys it: key = the two halves of `seed`, counter words (ctr low, ctr high, stream_id, 0).
    ctr: array of uint64; returns uint32 [len(ctr), 4]."""
    ctr = np.atleast_1d(np.asarray(ctr, dtype=np.uint64))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    c0, c1 = ctr & _MASK, ctr >> np.uint64(32)
    c2, c3 = np.full_like(c0, stream_id), np.zeros_like(c0)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _MASK, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _MASK
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def windows(seed, i, ids, H, W, s):
    """(vh, vw, bits) of proposal i for the samples `ids`: int64 arrays; bit c of bits is channel c's sign (set: +2 eps)."""
    ids = np.asarray(ids, dtype=np.uint64)
    r = philox4x32(seed, (np.uint64(i) << np.uint64(32)) | ids, STREAM_WINDOW).astype(np.uint64)
    vh = (r[:, 0] * np.uint64(H - s + 1)) >> np.uint64(32)
    vw = (r[:, 1] * np.uint64(W - s + 1)) >> np.uint64(32)
    return vh.astype(np.int64), vw.astype(np.int64), r[:, 2].astype(np.int64)


def stripes(seed, ids, C, W):
    """The +-1 stripes of the start, float64 [len(ids), C, W]: one Philox call per (b, c, w >> 7), bit w & 127 of its 128 bits."""
    ids = np.asarray(ids, dtype=np.uint64)
    nw = (W + 127) >> 7
    plane = (ids[:, None] * np.uint64(C) + np.arange(C, dtype=np.uint64)[None, :]).reshape(-1)
    ctr = ((plane[:, None] << np.uint64(32)) | np.arange(nw, dtype=np.uint64)[None, :]).reshape(-1)
    r = philox4x32(seed, ctr, STREAM_STRIPE).reshape(len(ids), C, nw, 4)
    w = np.arange(W)
    word = r[:, :, w >> 7, (w >> 5) & 3]
    return np.where((word >> (w & 31).astype(np.uint32)) & np.uint32(1), 1.0, -1.0)
