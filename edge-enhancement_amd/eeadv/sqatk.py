"""Host-side pieces of the Square attack (csrc/ee_sqatk.hip): the p schedule shared with the Add_Square defence, and
a vectorised numpy Philox4x32-10 that makes the kernels' draws - same key, counters and stream ids - for the plain-torch host path.  The
L2 form (csrc/ee_sqatk_l2.hip) adds its pattern tables eta(s), its schedule and the draws of streams 13 and 14; the
L1 form (csrc/ee_sqatk_l1.hip; section 21) takes all of those unchanged and adds the radius of its projections."""
import math

import numpy as np

STREAM_WINDOW, STREAM_STRIPE = 11, 12  # kStreamWindow / kStreamStripe of ee_sqatk.hpp; 0 and 7 belong to other kernels
STREAM_WINDOW2, STREAM_TILE = 13, 14   # kStreamWindow2 / kStreamTile: window 2 of an L2 proposal, the tiles of the L2 start
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


# ---- the L2 form ------------------------------------------------------------------------------------------------
def _rect(a, s):
    """[a, s] float64: sum over k = 0 .. max(a//2, s//2) of 1/(k+1)^2 on the rows and columns within k of the centre (a//2, s//2)."""
    out = np.zeros((a, s), dtype=np.float64)
    ca, cs = a // 2, s // 2
    for k in range(max(ca, cs) + 1):
        out[max(ca - k, 0):min(ca + k, a - 1) + 1, max(cs - k, 0):min(cs + k, s - 1) + 1] += 1.0 / (k + 1) ** 2
    return out


def eta(s):
    """The [s, s] pattern of an L2 proposal, float32: rect(s//2, s) on the top s//2 rows, -rect(s - s//2, s) on the rest, divided by its own
    L2 norm - formed in float64 and rounded once."""
    s = int(s)
    if s < 1:
        raise ValueError("eta needs s >= 1, got %d" % s)
    t = np.concatenate([_rect(s // 2, s), -_rect(s - s // 2, s)], axis=0)
    return (t / math.sqrt(math.fsum((t * t).reshape(-1).tolist()))).astype(np.float32)


def square_schedule_l2(n_queries, H, W, p_init=0.8):
    """Window edge of each of the n_queries - 1 proposals of an L2 run: s_i = max(int(round(sqrt(p(i) * H * W))), 3), plus 1 if even, capped
    at the largest odd number <= min(H, W); p rescaled as in square_schedule."""
    n_queries = int(n_queries)
    if n_queries < 1:
        raise ValueError("Square needs n_queries >= 1")
    if min(H, W) < 3:
        raise ValueError("L2 Square needs images of at least 3 x 3 (its smallest window), got %d x %d" % (H, W))
    cap = min(H, W) if min(H, W) % 2 else min(H, W) - 1
    out = []
    for i in range(n_queries - 1):
        s = max(int(round(math.sqrt(p_selection(i, p_init, n_queries) * H * W))), 3)
        out.append(min(s + 1 if s % 2 == 0 else s, cap))
    return out


def start_size(H, W):
    """s0, the tile edge of the L2 start: max(min(H, W) // 5, 1)."""
    return max(min(H, W) // 5, 1)


def eta_tables(sizes, s0):
    """(eta float32 [sum of s*s], eta_off [len(sizes)], off0): one table per distinct size of `sizes` and s0's, flattened row-major one
    after the other; eta_off[i] is where the table of sizes[i] starts, off0 where s0's does."""
    where, parts, n = {}, [], 0
    for s in sorted(set(sizes) | {s0}):
        where[s] = n
        parts.append(eta(s).reshape(-1))
        n += s * s
    return np.concatenate(parts), np.asarray([where[s] for s in sizes], dtype=np.int32), where[s0]


def windows_l2(seed, i, ids, H, W, s):
    """(vh, vw, bits, transpose) of window 1 of L2 proposal i: the draw of `windows`, with bit 0 of its fourth word as the transpose coin."""
    ids = np.asarray(ids, dtype=np.uint64)
    r = philox4x32(seed, (np.uint64(i) << np.uint64(32)) | ids, STREAM_WINDOW).astype(np.uint64)
    vh = (r[:, 0] * np.uint64(H - s + 1)) >> np.uint64(32)
    vw = (r[:, 1] * np.uint64(W - s + 1)) >> np.uint64(32)
    return vh.astype(np.int64), vw.astype(np.int64), r[:, 2].astype(np.int64), (r[:, 3] & np.uint64(1)).astype(np.int64)


def windows2(seed, i, ids, H, W, s):
    """(vh2, vw2) of window 2 of L2 proposal i for the samples `ids`: the same counter on stream 13."""
    ids = np.asarray(ids, dtype=np.uint64)
    r = philox4x32(seed, (np.uint64(i) << np.uint64(32)) | ids, STREAM_WINDOW2).astype(np.uint64)
    vh = (r[:, 0] * np.uint64(H - s + 1)) >> np.uint64(32)
    vw = (r[:, 1] * np.uint64(W - s + 1)) >> np.uint64(32)
    return vh.astype(np.int64), vw.astype(np.int64)


def tiles(seed, ids, n_tiles):
    """(bits, transpose), int64 [len(ids), n_tiles], of the tiles of the L2 start: stream 14, ctr = (id << 32) | k; bit c of bits is channel
    c's sign (set: +eta), transpose the tile's coin."""
    ids = np.asarray(ids, dtype=np.uint64)
    ctr = ((ids[:, None] << np.uint64(32)) | np.arange(n_tiles, dtype=np.uint64)[None, :]).reshape(-1)
    r = philox4x32(seed, ctr, STREAM_TILE).reshape(len(ids), n_tiles, 4)
    return r[:, :, 0].astype(np.int64), (r[:, :, 1] & np.uint32(1)).astype(np.int64)


# ---- the L1 form: schedule, start size, tables and draws are the L2 form's ----------------------------------------
def l1_eps_p(eps):
    """eps_p, the radius every projection of an L1 run uses: float32(float64(float32(eps)) * (1 - 1e-6)), formed once on the host."""
    return float(np.float32(np.float64(np.float32(eps)) * (1.0 - 1e-6)))
