"""An independent restatement of the L1 Square attack as this repository builds it, for the tests: per sample,
start and proposal in numpy in the dtype of the images it is given (float64 on the host, float32 against the kernels), every L1 norm
math.fsum over the exact |values| - or a norm the caller forces - and every point the exact projection of apgd_l1_reference.project_row,
with its own multiplier or one the caller forces.  Pattern, schedule and draws are square_l2_reference's, unchanged.

Nothing here imports the package."""
import math

import numpy as np

import square_l2_reference as L2
from apgd_l1_reference import l1_excess, project_row  # noqa: F401  (l1_excess: for the tests)
from square_l2_reference import ulps  # noqa: F401

TINY32 = L2.TINY32


def eps_p(eps):
    """The radius of every projection: float32(float64(float32(eps)) * (1 - 1e-6)), as a Python float."""
    return float(np.float32(np.float64(np.float32(eps)) * (1.0 - 1e-6)))


def exact_norm(v):
    """The exactly summed L1 norm of v as a float64 (rounded once)."""
    return math.fsum(np.abs(np.asarray(v, dtype=np.float64)).reshape(-1).tolist())


def norm(v):
    """||v||_1 in v's dtype."""
    return v.dtype.type(exact_norm(v))


def project(u, x0, r, lam=None):
    """P_r(u) of one sample [C,H,W] -> (z, info)."""
    z, info = project_row(u.reshape(-1), x0.reshape(-1), r, lam)
    return z.reshape(x0.shape), info


def start_point(x0, b, seed):
    """u = x0 + d of the start: the L2 start's pattern, not rescaled."""
    return x0 + L2.start_pattern(x0.shape, x0.dtype, b, seed)


def start(x0, b, eps, seed, lam=None):
    """(x_best, info of the projection)."""
    return project(start_point(x0, b, seed), x0, eps_p(eps), lam)


def proposal_point(x_best, x0, eps, seed, i, b, s, norms=None):
    """(u, norms) of proposal i of sample b: u = x0 + delta before the projection, norms = [n_img, n_un, n_w[0..C), n_new[0..C)] in x0's
    dtype, each taken of the elements this function holds at that stage.  `norms`, if given, are used in their place."""
    t = x0.dtype.type
    C, H, W = x0.shape
    tiny, e = t(TINY32), t(eps)
    vh, vw, bits, tr = L2.window1(seed, i, b, H, W, s)
    vh2, vw2 = L2.window2(seed, i, b, H, W, s)
    et = L2.eta(s).astype(x0.dtype)
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
        forced = {"n_img": t(norms[0]), "n_un": t(norms[1]), "n_w": [t(v) for v in norms[2:2 + C]], "n_new": [t(v) for v in norms[2 + C:2 + 2 * C]]}

    def use(k, c=None):
        src = got if forced is None else forced
        return src[k] if c is None else src[k][c]

    new = np.empty((C, s, s), dtype=x0.dtype)
    for c in range(C):
        new[c] = (et if (bits >> c) & 1 else -et) + delta[c][w1[1:]] / (tiny + use("n_w", c))
    got["n_new"] = [norm(new[c]) for c in range(C)]
    scale = max(e - use("n_img"), t(0)) / t(C) + use("n_un")
    for c in range(C):
        new[c] = new[c] / (tiny + use("n_new", c)) * scale
    delta = delta.copy()
    delta[w2] = 0
    delta[w1] = new
    return x0 + delta, [got["n_img"], got["n_un"]] + got["n_w"] + got["n_new"]


def propose(x_best, x0, eps, seed, i, b, s, norms=None, lam=None):
    """(x_new, norms, info of the projection)."""
    u, own = proposal_point(x_best, x0, eps, seed, i, b, s, norms)
    z, info = project(u, x0, eps_p(eps), lam)
    return z, own, info


class Sample:
    """One sample's attack as a state machine, as square_l2_reference.Sample: `observe(margin)` after the forward on x_new, `advance()` to
    the next proposal.  A sample that makes no proposal keeps x_new = x_best untouched (no projection)."""

    def __init__(self, x0, b, n_queries, eps, seed, lam0=None):
        self.x0, self.b, self.eps, self.seed = x0, b, eps, seed
        self.sizes = L2.schedule(n_queries, x0.shape[1], x0.shape[2])
        self.x_best, self.start_info = start(x0, b, eps, seed, lam0)
        self.x_new = self.x_best.copy()
        self.margin_min = x0.dtype.type(np.inf)
        self.queries, self.i, self.flag = 0, 0, False
        self.norms = []    # per proposal made: (i, the reference's own norms, the projection's info)
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

    def advance(self, norms=None, lam=None):
        if not self.fooled and self.i < len(self.sizes):
            self.x_new, own, info = propose(self.x_best, self.x0, self.eps, self.seed, self.i, self.b, self.sizes[self.i], norms, lam)
            self.norms.append((self.i, own, info))
        else:
            self.x_new = self.x_best.copy()
        self.i += 1
        self.iterates.append(self.x_new.copy())

    @property
    def robust(self):
        return bool(self.margin_min > 0)


def run(x0, y, n_queries, eps, seed, logits=None, margins=None, ids=None, lam0=None, norms=None, lam=None):
    """x0 [B,C,H,W] numpy, y [B].  logits: callable [B,C,H,W] -> [B,K]; or margins [n_queries, B], a recorded sequence.  Teacher forcing:
    lam0 [B] (the start's multiplier), norms [n_queries - 1][2 + 2C, B] and lam [n_queries - 1][B] (what some other implementation used at
    proposal i).  Returns (samples, flags, seen)."""
    B = x0.shape[0]
    ids = list(range(B)) if ids is None else list(ids)
    samples = [Sample(x0[k], ids[k], n_queries, eps, seed, None if lam0 is None else lam0[k]) for k in range(B)]
    flags, seen = [], []
    for q in range(n_queries):
        if margins is not None:
            m = [x0.dtype.type(margins[q][k]) for k in range(B)]
        else:
            z = np.asarray(logits(np.stack([s.x_new for s in samples])))
            m = [L2.margin_of(z[k], int(y[k])) for k in range(B)]
        flags.append([s.observe(m[k]) for k, s in enumerate(samples)])
        seen.append(m)
        if q < n_queries - 1:
            for k, s in enumerate(samples):
                s.advance(None if norms is None else [row[k] for row in norms[q]], None if lam is None else lam[q][k])
    return samples, flags, seen
