"""Host-side pieces of the FAB restarts (csrc/ee_fab.hip, ee_fab_start_f32): the draws of the random start restated
with the numpy Philox of eeadv/sqatk.py - same key, counters and stream id as the kernel - the key of one start, and the start itself in
torch ops for the plain-torch host paths of utils/attacks.py."""
import numpy as np
import torch

from .sqatk import philox4x32

STREAM_FAB_START = 15  # kStreamFabStart of ee_common.hpp
METRICS = ("Linf", "L2", "L1")
_MASK64 = 0xFFFFFFFFFFFFFFFF
_TWO_PI_F32 = np.float32(6.28318530717958647692)


def seed_of(seed, target_index, restart):
    """The 64-bit Philox key of one random start: of restart `restart` (>= 1) of the run towards the target class of index `target_index`
    (1 .. n_target_classes as FAB_T counts them; 0 for untargeted FAB).  A fixed function - the splitmix64 finaliser, a bijection of 64-bit
    words, over seed + 0x9E3779B97F4A7C15 (target_index + 1) + 0xD1B54A32D192ED03 restart (mod 2^64) - so every (target class, restart)
    pair of one attack has a key of its own and nothing else enters a draw."""
    z = (int(seed) + 0x9E3779B97F4A7C15 * (int(target_index) + 1) + 0xD1B54A32D192ED03 * int(restart)) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def draw(seed, B, D, metric, stream=STREAM_FAB_START):
    """t, float32 [B, D]: the draw ee_fab_start_f32 makes for rows 0 .. B-1 under the key `seed` - one Philox call per group of four
    elements, counter (b << 32) | (element >> 2), stream 15 (`stream`: the id of another start launch that draws the same way).  'Linf': t = 2 u - 1 with u = (word >> 8) 2^-24, exact, so bit-identical to
    the kernel.  'L2' / 'L1': the Box-Muller pairs (words 0, 1) and (words 2, 3), sqrt(-2 log(1 - u_a)) cos / sin(a) with the angle
    a = float32(2 pi) * u_b rounded to float32 as the kernel rounds it, everything else in float64 and cast once: the kernel's value up to
    the rounding of its float logf, sqrtf, cosf / sinf and product."""
    if metric not in METRICS:
        raise ValueError("FAB metric must be one of %s, got %r" % (list(METRICS), metric))
    B, D = int(B), int(D)
    G = (D + 3) // 4
    ctr = ((np.arange(B, dtype=np.uint64)[:, None] << np.uint64(32)) | np.arange(G, dtype=np.uint64)[None, :]).reshape(-1)
    r = philox4x32(seed, ctr, int(stream)).reshape(B, G, 4)
    u = (r >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)  # exact
    if metric == "Linf":
        t = np.float32(2.0) * u - np.float32(1.0)
    else:
        rad = np.sqrt(-2.0 * np.log((np.float32(1.0) - u[:, :, 0::2]).astype(np.float64)))  # 1 - u is exact in float32, in (0, 1]
        ang = (_TWO_PI_F32 * u[:, :, 1::2]).astype(np.float64)  # the float32 product, then widened
        t = np.empty((B, G, 4), dtype=np.float64)
        t[:, :, 0::2] = rad * np.cos(ang)
        t[:, :, 1::2] = rad * np.sin(ang)
        t = t.astype(np.float32)
    return np.ascontiguousarray(t.reshape(B, G * 4)[:, :D])


def row_norms(t, metric):
    """n of the start, per row of t [B, D] and in t's dtype: max |t_i| (Linf), sqrt(sum t_i^2) (L2), sum |t_i| (L1) - the sums in float64,
    rounded once, as the kernel forms them."""
    a = t.abs()
    if metric == "Linf":
        return a.max(dim=1)[0]
    a64 = a.to(torch.float64)
    n = (a64 * a64).sum(dim=1).sqrt() if metric == "L2" else a64.sum(dim=1)
    return n.to(t.dtype)


def start(x0, res, eps, t, metric):
    """The start of a restart in torch ops, in x0's dtype: clamp(x0 + ((m t) / n) * 0.5, 0, 1), m = min(res, eps), one rounding per
    operation in the kernel's order; rows whose n is 0 or not finite stay at x0.  t has x0's shape."""
    B = x0.shape[0]
    tf, x0f = t.to(x0.dtype).reshape(B, -1), x0.reshape(B, -1)
    n = row_norms(tf, metric)
    m = torch.minimum(res.to(x0.dtype), torch.full_like(n, float(eps)))
    live = torch.isfinite(n) & (n != 0)
    safe_n = torch.where(live, n, torch.ones_like(n))
    moved = torch.clamp(x0f + ((m.view(-1, 1) * tf) / safe_n.view(-1, 1)) * 0.5, 0, 1)
    return torch.where(live.view(-1, 1), moved, x0f).view(x0.shape)
