"""An independent restatement of the Square attack as this repository builds it, for the tests: a scalar-Python
Philox4x32-10, the draws made from it, the schedule, and a per-sample loop in numpy that runs in the dtype of the images it is given
(float64 on the host, float32 against the kernels), fed by a logits callable or by a recorded margin sequence.

Nothing here imports the package."""
import math

import numpy as np

STREAM_WINDOW, STREAM_STRIPE = 11, 12
M32 = 0xFFFFFFFF


def philox_raw(counter, key):
    """Philox4x32-10 (Salmon et al. 2011): counter = 4 words, key = 2 words -> 4 words."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def philox(seed, ctr, stream_id):
    """As the kernels key it: key = the halves of the 64-bit seed, counter = (ctr low, ctr high, stream_id, 0)."""
    seed &= 0xFFFFFFFFFFFFFFFF
    return philox_raw((ctr & M32, (ctr >> 32) & M32, stream_id, 0), (seed & M32, seed >> 32))


def p_table(it, p_init=0.8):
    for bound, div in ((8000, 512), (6000, 256), (4000, 128), (2000, 64), (1000, 32), (500, 16), (200, 8), (50, 4), (10, 2)):
        if it > bound:
            return p_init / div
    return p_init


def schedule(n_queries, H, W):
    out = []
    for i in range(n_queries - 1):
        s = int(round(math.sqrt(p_table(int(i / n_queries * 10000)) * H * W)))
        out.append(min(max(s, 1), min(H, W)))
    return out


def window(seed, i, b, H, W, s):
    r = philox(seed, (i << 32) | b, STREAM_WINDOW)
    return (r[0] * (H - s + 1)) >> 32, (r[1] * (W - s + 1)) >> 32, r[2]


def stripe_sign(seed, b, c, w, C):
    r = philox(seed, ((b * C + c) << 32) | (w >> 7), STREAM_STRIPE)
    return 1.0 if (r[(w >> 5) & 3] >> (w & 31)) & 1 else -1.0


def start_point(x0, b, eps, seed):
    C, H, W = x0.shape
    e = x0.dtype.type(eps)
    out = np.empty_like(x0)
    for c in range(C):
        for w in range(W):
            out[c, :, w] = x0[c, :, w] + (e if stripe_sign(seed, b, c, w, C) > 0 else -e)
    return np.clip(out, 0, 1)


def propose(x_best, x0, eps, vh, vw, s, bits):
    e = x0.dtype.type(eps)
    delta = np.zeros_like(x0)
    for c in range(x0.shape[0]):
        delta[c, vh:vh + s, vw:vw + s] = 2 * e if (bits >> c) & 1 else -(2 * e)
    return np.clip(np.minimum(np.maximum(x_best + delta, x0 - e), x0 + e), 0, 1)


def margin_of(z, y):
    """z_y - max_{j != y} z_j in z's dtype; NaN with a NaN logit or a label outside the row."""
    K = len(z)
    if not 0 <= y < K or np.isnan(z).any():
        return z.dtype.type(np.nan)
    with np.errstate(invalid="ignore"):
        return z[y] - max(z[j] for j in range(K) if j != y)


class Sample:
    """One sample's attack as a state machine: `observe(margin)` after the forward on x_new, `advance()` to the next proposal."""

    def __init__(self, x0, b, n_queries, eps, seed):
        self.x0, self.b, self.eps, self.seed = x0, b, eps, seed
        self.sizes = schedule(n_queries, x0.shape[1], x0.shape[2])
        self.x_best = start_point(x0, b, eps, seed)
        self.x_new = self.x_best.copy()
        self.margin_min = x0.dtype.type(np.inf)
        self.queries, self.i, self.flag = 0, 0, False
        self.history = []  # margin_min after every forward

    @property
    def fooled(self):
        return bool(self.margin_min <= 0)

    def observe(self, m):
        self.flag = False
        if not self.fooled:
            self.queries += 1
            if m < self.margin_min:  # False for NaN
                self.margin_min, self.x_best, self.flag = m, self.x_new.copy(), True
        self.history.append(self.margin_min)
        return self.flag

    def advance(self):
        if not self.fooled and self.i < len(self.sizes):
            s = self.sizes[self.i]
            vh, vw, bits = window(self.seed, self.i, self.b, self.x0.shape[1], self.x0.shape[2], s)
            self.x_new = propose(self.x_best, self.x0, self.eps, vh, vw, s, bits)
        else:
            self.x_new = self.x_best.copy()
        self.i += 1

    @property
    def robust(self):
        return bool(self.margin_min > 0)


def run(x0, y, n_queries, eps, seed, logits=None, margins=None, ids=None):
    """x0 [B,C,H,W] numpy, y [B].  logits: callable [B,C,H,W] -> [B,K] (the samples advance in lockstep so that one batched forward serves
    them; each keeps its own state and draws under its id); or margins [n_queries, B], a recorded sequence.  Returns (samples, flags, seen):
    flags [n_queries][B] the accept decisions, seen [n_queries][B] the margins."""
    B = x0.shape[0]
    ids = list(range(B)) if ids is None else list(ids)
    samples = [Sample(x0[k], ids[k], n_queries, eps, seed) for k in range(B)]
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
            for s in samples:
                s.advance()
    return samples, flags, seen
