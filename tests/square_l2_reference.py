"""An independent restatement of the L2 Square attack as this repository builds it, for the tests: the pattern
eta(s) in scalar Python, the L2 schedule, the tile and window draws (on square_reference's scalar Philox), and a per-sample start /
proposal in numpy that runs in the dtype of the images it is given (float64 on the host, float32 against the kernels) with every norm
the root of math.fsum over the exact squares - or a norm the caller forces, so that the elements can be checked bit for bit next to a
norm that is allowed its last bit.

Nothing here imports the package."""
import math
from fractions import Fraction

import numpy as np

from square_reference import margin_of, p_table, philox

STREAM_WINDOW, STREAM_WINDOW2, STREAM_TILE = 11, 13, 14
TINY32 = np.float32(1e-12)


# ---- the pattern -----------------------------------------------------------------------------------------------------------------------
def rect(a, s):
    out = [[0.0] * s for _ in range(a)]
    ca, cs = a // 2, s // 2
    for k in range(max(ca, cs) + 1):
        for r in range(max(ca - k, 0), min(ca + k, a - 1) + 1):
            for c in range(max(cs - k, 0), min(cs + k, s - 1) + 1):
                out[r][c] += 1.0 / (k + 1) ** 2
    return out


def eta(s):
    """[s, s] float32: rect(s//2, s) above, -rect(s - s//2, s) below, over its own L2 norm; float64 throughout, rounded once."""
    rows = rect(s // 2, s) + [[-v for v in row] for row in rect(s - s // 2, s)]
    n = math.sqrt(math.fsum(v * v for row in rows for v in row))
    return np.array([[v / n for v in row] for row in rows], dtype=np.float64).astype(np.float32)


def schedule(n_queries, H, W):
    cap = min(H, W) if min(H, W) % 2 else min(H, W) - 1
    out = []
    for i in range(n_queries - 1):
        s = max(int(round(math.sqrt(p_table(int(i / n_queries * 10000)) * H * W))), 3)
        if s % 2 == 0:
            s += 1
        out.append(min(s, cap))
    return out


def start_size(H, W):
    return max(min(H, W) // 5, 1)


# ---- the draws -------------------------------------------------------------------------------------------------------------------------
def window1(seed, i, b, H, W, s):
    """(vh, vw, sign bits, transpose) of window 1."""
    r = philox(seed, (i << 32) | b, STREAM_WINDOW)
    return (r[0] * (H - s + 1)) >> 32, (r[1] * (W - s + 1)) >> 32, r[2], r[3] & 1


def window2(seed, i, b, H, W, s):
    r = philox(seed, (i << 32) | b, STREAM_WINDOW2)
    return (r[0] * (H - s + 1)) >> 32, (r[1] * (W - s + 1)) >> 32


def tile(seed, b, k):
    """(sign bits, transpose) of tile k of sample b's start."""
    r = philox(seed, (b << 32) | k, STREAM_TILE)
    return r[0], r[1] & 1


# ---- norms -----------------------------------------------------------------------------------------------------------------------------
def exact_norm(v):
    """sqrt of the exact sum of the squares of v's elements, as a float64: every element is an integer times a power of two, so the sum of
    the squares is formed in integers; it is rounded once on its way to a float64, and the root once more."""
    v = np.asarray(v)
    if v.dtype == np.float32:  # the squares are exact in float64, fsum adds them without error
        return math.sqrt(math.fsum((v.reshape(-1).astype(np.float64) ** 2).tolist()))
    flat = [float(x) for x in v.reshape(-1) if x != 0]
    if not flat:
        return 0.0
    parts = []
    for x in flat:
        m, e = math.frexp(x)
        parts.append((int(m * 2.0 ** 53), e - 53))  # x = M * 2^E exactly
    e_min = min(e for _, e in parts)
    total = sum((m * m) << (2 * (e - e_min)) for m, e in parts)
    return math.sqrt(float(Fraction(total) * Fraction(2) ** (2 * e_min)))


def norm(v):
    """||v||_2 in v's dtype."""
    return v.dtype.type(exact_norm(v))


def ulps(a, b):
    """The distance of two finite values of one dtype in units of the last place."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype
    it = np.int32 if a.dtype == np.float32 else np.int64
    ia, ib = a.view(it).astype(object), b.view(it).astype(object)
    return int(abs(int(ia) - int(ib))) if a.ndim == 0 else [abs(int(p) - int(q)) for p, q in zip(ia.reshape(-1), ib.reshape(-1))]


# ---- start and proposal ----------------------------------------------------------------------------------------------------------------
def start_pattern(shape, dtype, b, seed):
    C, H, W = shape
    s0 = start_size(H, W)
    nh, nw = H // s0, W // s0
    oh, ow = (H - nh * s0) // 2, (W - nw * s0) // 2
    e0 = eta(s0).astype(dtype)
    d = np.zeros(shape, dtype=dtype)
    for a in range(nh):
        for t in range(nw):
            bits, tr = tile(seed, b, a * nw + t)
            blk = e0.T if tr else e0
            for c in range(C):
                d[c, oh + a * s0:oh + (a + 1) * s0, ow + t * s0:ow + (t + 1) * s0] = blk if (bits >> c) & 1 else -blk
    return d


def start(x0, b, eps, seed, norms=None):
    """(x_best, [n0]).  The order of the scaling: one quotient eps / (n0 + tiny), then one product per element."""
    t = x0.dtype.type
    d = start_pattern(x0.shape, x0.dtype, b, seed)
    n0 = norm(d) if norms is None else t(norms[0])
    q = t(eps) / (n0 + t(TINY32))
    return np.clip(x0 + d * q, 0, 1), [n0]


def propose(x_best, x0, eps, seed, i, b, s, norms=None):
    """Proposal i of sample b: (x_new, norms) with norms = [n_img, n_un, n_d, n_w[0..C), n_new[0..C)] in x0's dtype; every norm is taken of
    the elements this function holds at that stage.  `norms`, if given, are used in their place (and the computed ones still returned)."""
    t = x0.dtype.type
    C, H, W = x0.shape
    tiny, e = t(TINY32), t(eps)
    vh, vw, bits, tr = window1(seed, i, b, H, W, s)
    vh2, vw2 = window2(seed, i, b, H, W, s)
    et = eta(s).astype(x0.dtype)
    et = et.T if tr else et
    w1 = (slice(None), slice(vh, vh + s), slice(vw, vw + s))
    w2 = (slice(None), slice(vh2, vh2 + s), slice(vw2, vw2 + s))
    delta = x_best - x0
    union = np.zeros((H, W), dtype=bool)
    union[w1[1:]] = True
    union[w2[1:]] = True
    got = {"n_img": norm(delta), "n_un": norm(delta[:, union]), "n_w": [norm(delta[c][w1[1:]]) for c in range(C)]}
    forced = None
    if norms is not None:
        forced = {"n_img": t(norms[0]), "n_un": t(norms[1]), "n_d": t(norms[2]), "n_w": [t(v) for v in norms[3:3 + C]],
                  "n_new": [t(v) for v in norms[3 + C:3 + 2 * C]]}

    def use(k, c=None):
        src = got if forced is None else forced
        return src[k] if c is None else src[k][c]

    new = np.empty((C, s, s), dtype=x0.dtype)
    for c in range(C):
        new[c] = (et if (bits >> c) & 1 else -et) + delta[c][w1[1:]] / (tiny + use("n_w", c))
    got["n_new"] = [norm(new[c]) for c in range(C)]
    n_img, n_un = use("n_img"), use("n_un")
    scale = np.sqrt(max(e * e - n_img * n_img, t(0)) / t(C) + n_un * n_un)
    for c in range(C):
        new[c] = new[c] / (tiny + use("n_new", c)) * scale
    delta = delta.copy()
    delta[w2] = 0
    delta[w1] = new
    got["n_d"] = norm(delta)
    x_new = np.clip(x0 + delta / (tiny + use("n_d")) * e, 0, 1)
    return x_new, [got["n_img"], got["n_un"], got["n_d"]] + got["n_w"] + got["n_new"]


# ---- the run ---------------------------------------------------------------------------------------------------------------------------
class Sample:
    """One sample's attack as a state machine: `observe(margin)` after the forward on x_new, `advance()` to the next proposal.
    forced_start / forced(i): the norms to use in the place of the reference's own (teacher forcing), or None."""

    def __init__(self, x0, b, n_queries, eps, seed, forced_start=None):
        self.x0, self.b, self.eps, self.seed = x0, b, eps, seed
        self.sizes = schedule(n_queries, x0.shape[1], x0.shape[2])
        self.x_best, self.start_norms = start(x0, b, eps, seed, forced_start)
        self.x_new = self.x_best.copy()
        self.margin_min = x0.dtype.type(np.inf)
        self.queries, self.i, self.flag = 0, 0, False
        self.norms = []    # per proposal made: (i, the reference's own norms)
        self.iterates = [self.x_new.copy()]  # x_new before every forward

    @property
    def fooled(self):
        return bool(self.margin_min <= 0)

    def observe(self, m):
        self.flag = False
        if not self.fooled:
            self.queries += 1
            if m < self.margin_min:  # False for NaN
                self.margin_min, self.x_best, self.flag = m, self.x_new.copy(), True
        return self.flag

    def advance(self, forced=None):
        if not self.fooled and self.i < len(self.sizes):
            self.x_new, own = propose(self.x_best, self.x0, self.eps, self.seed, self.i, self.b, self.sizes[self.i], forced)
            self.norms.append((self.i, own))
        else:
            self.x_new = self.x_best.copy()
        self.i += 1
        self.iterates.append(self.x_new.copy())

    @property
    def robust(self):
        return bool(self.margin_min > 0)


def run(x0, y, n_queries, eps, seed, logits=None, margins=None, ids=None, start_norms=None, norms=None):
    """x0 [B,C,H,W] numpy, y [B].  logits: callable [B,C,H,W] -> [B,K]; or margins [n_queries, B], a recorded sequence.  start_norms [1, B]
    and norms [n_queries - 1][3 + 2C, B] (the norms some other implementation used at the start and at proposal i): teacher forcing.
    Returns (samples, flags, seen)."""
    B = x0.shape[0]
    ids = list(range(B)) if ids is None else list(ids)
    samples = [Sample(x0[k], ids[k], n_queries, eps, seed, None if start_norms is None else [start_norms[0][k]]) for k in range(B)]
    flags, seen = [], []
    for q in range(n_queries):
        if margins is not None:
            m = [x0.dtype.type(margins[q][k]) for k in range(B)]
        else:
            z = np.asarray(logits(np.stack([s.x_new for s in samples])))
            m = [margin_of(z[k], int(y[k])) for k in range(B)]
        flags.append([s.observe(m[k]) for k, s in enumerate(samples)])
        seen.append(m)
        if q < n_queries - 1:
            for k, s in enumerate(samples):
                s.advance(None if norms is None else [row[k] for row in norms[q]])
    return samples, flags, seen
