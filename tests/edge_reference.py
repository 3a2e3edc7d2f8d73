"""Float64 reference of the edge front end (CannyFilter_step125_1, CannyFilter, CannyFilter_BPDA), host only, numpy.

TEST INFRASTRUCTURE ONLY.  Written from the semantics of utils/core.py (:148-326 full filter, :386-505 BPDA, :509-585 step125): replicate
pad + 3x3 correlation per channel, replicate pad of the blurred planes + Sobel over channels, / C, magnitude, alpha mask, orientation in
degrees, rint(ori / 45) mod 8, non-maximum suppression on the derived direction table, double threshold, hysteresis.  Nothing here follows the
operation order of the kernels or of oracle/ee_oracle.c: sums are taken tap by tap over whole planes, the Sobel responses as differences of
the two non-zero columns (rows) first, the adjoints as scatter + fold.

Three things come out per pixel: the float64 value of every map, a DERIVED bound on what any float32 evaluation may differ by, and a class.

Bounds (u = 2^-24; gamma(k) = k u / (1 - k u); every bound has the form gamma(k) * abs_sum, k = roundings on the path):
  blurred plane   9 fmaf                                                      k = 9        abs_sum Ab = |G| * |x|
  channel Sobel   9 C fmaf on values that carry the 9 above                    k = 9 C + 9  abs_sum S = sum_c |S| * Ab_c
  gx1, gy1        + the division by C                                          k = 9 C + 10 abs_sum S / C
  mag             sqrt is 1-Lipschitz in (gx1, gy1); two squares + one add cost 2u relative on s2 = u on mag, sqrtf one more
                                                                               k = 9 C + 12 abs_sum (Sx + Sy) / C
  orientation     the direction of (gx1, gy1) moves by at most asin(e / mag), e = hypot of the two bounds; the quotient's rounding moves
                  atan by u / 2, device atanf by ATAN_ULP ulp of a value below 2 (ASSUMED), the product with the rounded
                  constant 360 / pi and the + 180 by (2 * 180 + 360) u degrees, the / 45 by 8 u:  in units of ori / 45
                  e_q = (8 / pi) (asin(e / mag) + u / 2 + ATAN_ULP 2^-23) + 24 u.   rintf, * 45, / 45, the mod 8 are exact.
  gradients       gg = gm cos(phi) / C: cos moves by at most asin(e / mag), the seven roundings of 1 / sqrtf(s2), the products and / C add
                  7 u: e_gg = |gm| (asin(e / mag) + gamma(7)) / C (+ the bound gm itself carries).  Sobel^T (18 fmaf) + fold (4 adds) and
                  Gauss^T (9 fmaf) + fold (4 adds): k = 35 on abs_sum |pad^T G^T| |pad^T S^T| |gg|, plus the same maps applied to e_gg.
No product here can underflow: a non-zero response is a multiple of the ulp of a tap product (> 2^-45 for k / 255 images), its square > 2^-90.

Classes.  Every comparison a pixel takes part in is DECIDED when its float64 margin exceeds its bound, an EXACT TIE when float64 and any
float32 evaluation provably hold the same value on both sides, UNDECIDED otherwise.  Proofs used (none assumes an operation order):
  zero window     every input value the pixel's responses depend on (the doubly clamped 5x5 support, all channels) is +-0: every product and
                  sum is +-0, so gx = gy = mag = 0, the orientation is NaN, the pixel is never suppressed, its gradient is 0 * inf = NaN.
                  A FLAT NON-ZERO support is NOT such a proof: a float32 chain -b/2 - b - b/2 + b/2 + b + b/2 need not return to 0.
  same window     the pixel and its neighbour along the quantised direction see bit-identical supports (a pattern invariant under that
                  shift): any deterministic evaluation gives both the same magnitude, m - neighbour == 0, !(mn > 0) removes both.
  exact zero      a masked (mag < alpha decided) or suppressed pixel holds t = 0 exactly; against low = 0 the strict `t - low > 0` is false.
"""
import numpy as np

U = 2.0 ** -24
ATAN_ULP = 5.0  # ASSUMED error of device atanf in ulp: OpenCL's full-profile limit, taken (also an assumption) to hold for the device library
ONE001 = float(np.float32(1.001))


def gamma(k):
    return k * U / (1.0 - k * U)


def f32(v):
    """a Python float as the kernels receive it (ctypes c_float), widened exactly"""
    return float(np.float32(v))


def weights64(wts):
    h = np.asarray(wts.host, dtype=np.float32).astype(np.float64)
    return h[:9].reshape(3, 3), h[9:18].reshape(3, 3), h[18:27].reshape(3, 3)


def dirs_of(wts):
    return np.asarray(wts.dirs, dtype=np.int64).reshape(8, 2)


# ---- linear pieces -----------------------------------------------------------------------------------------------------------------------------
def _pad(a):
    return np.pad(a, [(0, 0)] * (a.ndim - 2) + [(1, 1), (1, 1)], mode="edge")


def _corr3(p, w):
    """3x3 correlation of a padded plane stack [..., H+2, W+2]; every tap multiplies (0 * NaN = NaN like a convolution)"""
    H, W = p.shape[-2] - 2, p.shape[-1] - 2
    out = np.zeros(p.shape[:-2] + (H, W))
    for di in range(3):
        for dj in range(3):
            out = out + w[di, dj] * p[..., di:di + H, dj:dj + W]
    return out


def _sobel_pair(pb, sx, sy):
    """Sobel x / y of padded planes, the two non-zero columns (rows) differenced first: a pattern constant along x gives gx = 0 exactly"""
    H, W = pb.shape[-2] - 2, pb.shape[-1] - 2
    gx = np.zeros(pb.shape[:-2] + (H, W))
    gy = np.zeros_like(gx)
    for d in range(3):
        gx = gx + (sx[d, 2] * pb[..., d:d + H, 2:2 + W] + sx[d, 0] * pb[..., d:d + H, 0:W]) + sx[d, 1] * pb[..., d:d + H, 1:1 + W]
        gy = gy + (sy[2, d] * pb[..., 2:2 + H, d:d + W] + sy[0, d] * pb[..., 0:H, d:d + W]) + sy[1, d] * pb[..., 1:1 + H, d:d + W]
    return gx, gy


def _corr3_T(g, w):
    """transposed 3x3 correlation: [..., H, W] -> padded domain [..., H+2, W+2]"""
    H, W = g.shape[-2:]
    gp = np.zeros(g.shape[:-2] + (H + 2, W + 2))
    for di in range(3):
        for dj in range(3):
            gp[..., di:di + H, dj:dj + W] += w[di, dj] * g
    return gp


def _pad_T(gp):
    """adjoint of ReplicationPad2d(1)"""
    out = gp[..., 1:-1, 1:-1].copy()
    out[..., 0, :] += gp[..., 0, 1:-1]
    out[..., -1, :] += gp[..., -1, 1:-1]
    out[..., :, 0] += gp[..., 1:-1, 0]
    out[..., :, -1] += gp[..., 1:-1, -1]
    out[..., 0, 0] += gp[..., 0, 0]
    out[..., 0, -1] += gp[..., 0, -1]
    out[..., -1, 0] += gp[..., -1, 0]
    out[..., -1, -1] += gp[..., -1, -1]
    return out


def _shift0(a, dr, dc, fill=0.0):
    """out(i, j) = a(i + dr, j + dc), `fill` outside the image (conv2d zero padding)"""
    H, W = a.shape[-2:]
    out = np.full(a.shape, fill, dtype=a.dtype)
    i0, i1 = max(0, -dr), min(H, H - dr)
    j0, j1 = max(0, -dc), min(W, W - dc)
    if i0 < i1 and j0 < j1:
        out[..., i0:i1, j0:j1] = a[..., i0 + dr:i1 + dr, j0 + dc:j1 + dc]
    return out


def _box(a, r, op):
    """op over the (2r+1)^2 in-image neighbourhood (booleans)"""
    out = a.copy()
    for dr in range(-r, r + 1):
        for dc in range(-r, r + 1):
            out = op(out, _shift0(a, dr, dc, fill=(op is np.logical_and)))
    return out


def support(x):
    """[B, H, W, C*81]: every input value the responses of a pixel depend on (clamp of the blurred plane, then clamp of the image)"""
    B, C, H, W = x.shape
    ii, jj = np.arange(H), np.arange(W)
    cols = []
    for a in (-1, 0, 1):
        for a2 in (-1, 0, 1):
            r = np.clip(np.clip(ii + a, 0, H - 1) + a2, 0, H - 1)
            for b in (-1, 0, 1):
                for b2 in (-1, 0, 1):
                    s = np.clip(np.clip(jj + b, 0, W - 1) + b2, 0, W - 1)
                    cols.append(x[:, :, r][:, :, :, s])
    return np.stack(cols, -1).transpose(0, 2, 3, 1, 4).reshape(B, H, W, C * 81)


# ---- forward -----------------------------------------------------------------------------------------------------------------------------------
def forward(x, wts, alpha, low, high, mode):
    """mode: 'step125' | 'canny' | 'bpda'.  x [B, C, H, W] float32.  Returns a dict of [B, 1, H, W] maps (float64 / bool)."""
    assert x.dtype == np.float32
    B, C, H, W = x.shape
    g, sx, sy = weights64(wts)
    alpha, low, high = (0.0 if mode == "bpda" else f32(alpha)), f32(low), f32(high)
    x64 = x.astype(np.float64)
    with np.errstate(all="ignore"):
        blur = _corr3(_pad(x64), g)
        Ab = _corr3(_pad(np.abs(x64)), np.abs(g))
        ax, ay = _sobel_pair(_pad(blur), sx, sy)
        ax, ay = ax.sum(1, keepdims=True), ay.sum(1, keepdims=True)
        Sx = _corr3(_pad(Ab), np.abs(sx)).sum(1, keepdims=True) / C
        Sy = _corr3(_pad(Ab), np.abs(sy)).sum(1, keepdims=True) / C
        gx, gy = ax / C, ay / C
        e_gx, e_gy = gamma(9 * C + 10) * Sx, gamma(9 * C + 10) * Sy
        mag = np.sqrt(gx * gx + gy * gy)
        e_mag = gamma(9 * C + 12) * (Sx + Sy)
        q = (np.arctan(gy / gx) * (360.0 / np.pi) + 180.0) / 45.0
        e_vec = np.hypot(e_gx, e_gy)
        ang = np.arcsin(np.minimum(1.0, e_vec / mag))  # NaN where mag = 0 and e = 0
        e_q = (8.0 / np.pi) * (ang + U / 2 + ATAN_ULP * 2.0 ** -23) + 24 * U
    finite = np.isfinite(mag) & np.isfinite(e_mag)
    sup = support(x)
    zero_win = (sup == 0).all(-1)[:, None]
    # is the magnitude exactly zero?  (decides the NaN orientation and the 0 * inf gradient)
    zero_sure, nonzero_sure = zero_win, finite & (mag > e_mag)
    zero_known = zero_sure | nonzero_sure
    # alpha mask: strict <, equality keeps
    masked = mag < alpha
    alpha_dec = finite & ((np.abs(mag - alpha) > e_mag) | zero_sure)
    magA = np.where(masked, 0.0, mag)
    e_magA = np.where(alpha_dec, np.where(masked, 0.0, e_mag), mag + e_mag)
    e_magA = np.where(zero_sure, 0.0, e_magA)
    out = dict(x=x, C=C, mode=mode, alpha=alpha, low=low, high=high, blur=blur, e_blur=gamma(9) * Ab, gx=gx, gy=gy, e_gx=e_gx, e_gy=e_gy,
               mag=mag, e_mag=e_mag, magA=magA, e_magA=e_magA, q=q, e_q=e_q, ang=ang, zero_win=zero_win, zero_known=zero_known,
               zero_sure=zero_sure, alpha_dec=alpha_dec, finite=finite, support=sup)

    # ---- step125: 1[magA > high], gradient gate high < magA <= 1.001 ----
    e125 = np.where(magA > high, 1.0, np.where(magA <= high, 0.0, magA))
    hi_dec = alpha_dec & ((np.abs(magA - high) > e_magA) | (e_magA == 0))
    g1001_dec = alpha_dec & ((np.abs(magA - ONE001) > e_magA) | (e_magA == 0))
    out.update(edge125=e125, edge125_dec=hi_dec & finite, cls125=_classes(hi_dec & g1001_dec & zero_known & finite, zero_sure))
    if mode == "step125":
        return out

    # ---- orientation index, NMS ----
    dirs = dirs_of(wts)
    with np.errstate(all="ignore"):
        qr = np.rint(q)
        idx = np.where(np.isnan(q), -1.0, np.mod(qr, 8.0))
        idx_dec = (zero_sure | (nonzero_sure & (np.abs(q - qr) + e_q < 0.5))) & finite
    kk = np.where(idx < 0, 0, idx).astype(np.int64) & 3
    sup_t = sup.transpose(0, 3, 1, 2).astype(np.float64)
    removed = np.zeros(mag.shape, bool)
    rem_dec = np.zeros(mag.shape, bool)
    rem_tie = np.zeros(mag.shape, bool)
    for k in range(4):
        sel = (idx >= 0) & (kk == k)
        dmin_rm, all_keep, tie = np.zeros(mag.shape, bool), np.ones(mag.shape, bool), np.zeros(mag.shape, bool)
        rm64 = np.zeros(mag.shape, bool)
        for kd in (k, k + 4):
            dr, dc = int(dirs[kd][0]), int(dirs[kd][1])
            nb, e_nb = _shift0(magA, dr, dc), _shift0(e_magA, dr, dc)
            inside = _shift0(np.ones(mag.shape, bool), dr, dc, fill=False)
            d, e_d = magA - nb, e_magA + e_nb
            same = (sup_t == _shift0(sup_t, dr, dc, fill=np.nan)).all(1, keepdims=True)  # identical supports (False outside the image)
            exact0 = (e_d == 0) & (d == 0)           # both sides hold an exact 0 (masked / zero window / outside the image)
            with np.errstate(invalid="ignore"):
                rm64 |= ~(d > 0)
                dmin_rm |= (d < -e_d) | same | exact0
                tie |= same | exact0
                all_keep &= d > e_d
        removed = np.where(sel, rm64, removed)
        rem_dec = np.where(sel, dmin_rm | all_keep, rem_dec)
        rem_tie = np.where(sel, tie & ~all_keep, rem_tie)
    rem_dec = np.where(idx < 0, True, rem_dec) & idx_dec
    # the thinned magnitude: exactly 0 when masked for sure (whatever the suppression says), else it needs the suppression decided
    t_zero_sure = (alpha_dec & (e_magA == 0) & (magA == 0)) | (rem_dec & removed)
    t_known = t_zero_sure | (rem_dec & ~removed & alpha_dec)
    thin = np.where(removed, 0.0, magA)
    e_thin = np.where(t_zero_sure, 0.0, np.where(t_known, e_magA, magA + e_magA))
    thr_tie = t_zero_sure & (low == 0.0)
    lo_dec = t_known & ((np.abs(thin - low) > e_thin) | t_zero_sure)
    hi2_dec = t_known & ((np.abs(thin - high) > e_thin) | t_zero_sure)
    t2 = 0.5 * (thin > low) + 0.5 * (thin > high)
    t2_dec = lo_dec & hi2_dec & finite
    hsum = sum(_shift0(t2, dr, dc) for dr in (-1, 0, 1) for dc in (-1, 0, 1))   # exact in float32 too: multiples of 1/2
    edge = (t2 == 1.0) * 1.0 + ((1.25 * hsum > 1.0) & (t2 == 0.5)) * 1.0
    edge_dec = _box(t2_dec, 1, np.logical_and)
    # straight-through gate |t - high| <= 1.001 (full filter), thr < thin <= 1.001 (BPDA): the float32 difference carries one rounding more
    with np.errstate(invalid="ignore"):
        if mode == "canny":
            v = np.abs(thin - high)
            ste = v <= ONE001
            ste_dec = t_known & ((np.abs(v - ONE001) > e_thin + U * v) | (t_zero_sure & (abs(abs(high) - ONE001) > U * 2)))
        else:
            ste = thin <= ONE001
            ste_dec = t_known & ((np.abs(thin - ONE001) > e_thin) | t_zero_sure)
    decided = alpha_dec & idx_dec & rem_dec & t2_dec & ste_dec & zero_known & finite
    tie = zero_sure | rem_tie | thr_tie
    out.update(idx=idx, idx_dec=idx_dec, removed=removed, rem_dec=rem_dec, rem_tie=rem_tie, thin=thin, e_thin=e_thin, t_known=t_known,
               t_zero_sure=t_zero_sure, t2=t2, t2_dec=t2_dec, hsum=hsum, edge=edge, edge_dec=edge_dec, ste=ste, ste_dec=ste_dec,
               cls=_classes(decided, tie))
    return out


DECIDED, TIE, UNDECIDED = 0, 1, 2


def _classes(decided, tie):
    return np.where(~decided, UNDECIDED, np.where(tie, TIE, DECIDED)).astype(np.int8)


def shares(cls):
    n = float(cls.size)
    return {"decided": float((cls == DECIDED).sum()) / n, "tie": float((cls == TIE).sum()) / n, "undecided": float((cls == UNDECIDED).sum()) / n}


# ---- the criteria both the host test (C oracle) and the GPU test (kernels) apply ---------------------------------------------------------------
def check_edge(got, ref, dec, what):
    """discrete output: equal to float64 wherever decided or an exact tie, one of the legal values elsewhere"""
    bad = dec & (got != ref)
    assert not bad.any(), "%s: %d decided pixels differ, first at %s" % (what, int(bad.sum()), np.argwhere(bad)[0])
    rest = got[~dec]
    assert np.isin(rest[np.isfinite(rest)], (0.0, 1.0)).all(), what + ": an undecided pixel holds an illegal value"


def check_bound(got, ref, bound, mask, what):
    """|got - ref64| <= bound where `mask`; returns the largest ratio"""
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got.astype(np.float64) - ref)
        ratio = np.where(mask & (err > 0), err / bound, 0.0)
    assert not (mask & ~np.isfinite(got) & np.isfinite(ref)).any(), what + ": non-finite where float64 is finite"
    worst = float(np.nanmax(ratio)) if ratio.size else 0.0
    assert worst <= 1.0, "%s: |got - ref64| = %.3f x its derived bound at %s" % (what, worst, np.unravel_index(np.nanargmax(ratio), ratio.shape))
    return worst


def check_grad(got, ref, bound, comp, what):
    """NaN pattern equal and finite values within the bound at comparable outputs"""
    nan_ref, nan_got = np.isnan(ref), np.isnan(got)
    bad = comp & (nan_ref != nan_got)
    assert not bad.any(), "%s: NaN pattern differs at %d comparable outputs, first %s" % (what, int(bad.sum()), np.argwhere(bad)[0])
    return check_bound(got, np.where(nan_ref, 0.0, ref), bound, comp & ~nan_ref, what)


# ---- backward ----------------------------------------------------------------------------------------------------------------------------------
def _tail(m, gm, e_gm, wts):
    """float64 adjoint chain from d loss / d mag-stage (gm, with its bound) to d loss / d image map; returns (g, bound)"""
    C = m["C"]
    g, sx, sy = weights64(wts)
    gx, gy = m["gx"], m["gy"]
    with np.errstate(all="ignore"):
        s2 = gx * gx + gy * gy
        rs = 1.0 / np.sqrt(s2)
        gs = gm * (0.5 * rs)                      # 0 * inf = NaN kept
        ggx, ggy = (gs * (2.0 * gx)) / C, (gs * (2.0 * gy)) / C
        rel = np.where(np.isfinite(m["ang"]), m["ang"], 0.0) + gamma(7)
        e_gg = (np.abs(gm) * rel + e_gm) / C
        out = _pad_T(_corr3_T(_pad_T(_corr3_T(ggx, sx) + _corr3_T(ggy, sy)), g))
        a1 = _pad_T(_corr3_T(np.abs(np.nan_to_num(ggx)), np.abs(sx)) + _corr3_T(np.abs(np.nan_to_num(ggy)), np.abs(sy)))
        a2 = _pad_T(_corr3_T(a1, np.abs(g)))
        e1 = _pad_T(_corr3_T(e_gg, np.abs(sx)) + _corr3_T(e_gg, np.abs(sy)))
        e2 = _pad_T(_corr3_T(e1, np.abs(g)))
    return out, gamma(35) * a2 + (1.0 + gamma(35)) * e2


def comparable(cls):
    """an output pixel is comparable when every pixel of its 5x5 support is decided or an exact tie"""
    return _box(cls != UNDECIDED, 2, np.logical_and)


def backward125(m, u, wts):
    """core.py:350-358, 575: the gradient passes where high < magA <= 1.001 and mag >= alpha"""
    u = u.astype(np.float64)
    with np.errstate(invalid="ignore"):
        gm = np.where((m["magA"] <= m["high"]) | (m["magA"] > ONE001) | (m["mag"] < m["alpha"]), 0.0, u)
    g, e = _tail(m, gm, np.zeros_like(gm), wts)
    return g, e, comparable(m["cls125"])


def g_mag_canny(m, u):
    """g_mag = (u / 2) 1[|t - high| <= 1.001] 1[not suppressed] 1[mag >= alpha]"""
    with np.errstate(invalid="ignore"):
        return np.where(m["ste"] & ~m["removed"] & ~(m["mag"] < m["alpha"]), u.astype(np.float64) / 2.0, 0.0)


def backward_canny(m, u, wts):
    g, e = _tail(m, g_mag_canny(m, u), np.zeros(m["mag"].shape), wts)
    return g, e, comparable(m["cls"])


def bpda_g_thin(u, thin, t2, low, high):
    """float64 replay of core.py:482-504 from GIVEN thin / t2 planes: out = high + To_compare(conv(t2), 1) * To_eq(t2); returns (g, bound).
    The float32 path: a 9-fmaf chain, one product before it, one add, two halvings (exact), one add: k = 12 on the absolute sum."""
    u, thin, t2 = u.astype(np.float64), thin.astype(np.float64), t2.astype(np.float64)
    low, high = f32(low), f32(high)
    w0 = 1.25 * sum(_shift0(t2, dr, dc) for dr in (-1, 0, 1) for dc in (-1, 0, 1))
    weak = (t2 == 0.5) * 1.0
    g_eq = np.where(t2 == 0.5, u * (w0 > 1.0), 0.0)
    gw0 = np.where((w0 > 1.0) & (w0 <= ONE001), u * weak, 0.0)     # To_compare(., 1).backward: 1 < weak_0 <= 1.001
    g_cv = 1.25 * sum(_shift0(gw0, -dr, -dc) for dr in (-1, 0, 1) for dc in (-1, 0, 1))
    a_cv = 1.25 * sum(_shift0(np.abs(gw0), -dr, -dc) for dr in (-1, 0, 1) for dc in (-1, 0, 1))
    g_t2 = g_eq + g_cv
    g_low = np.where((thin <= low) | (thin > ONE001), 0.0, 0.5 * g_t2)
    g_high = np.where((thin <= high) | (thin > ONE001), 0.0, u + 0.5 * g_t2)
    return g_low + g_high, gamma(12) * (np.abs(u) + np.abs(g_eq) + a_cv)


def backward_bpda(m, u, thin, t2, removed, wts, own_planes=True):
    """d loss / d image from the kernel's stored thin / t2 and the suppression flags (thin * ~to_remove, core.py:480).  Given the planes,
    d loss / d thin is a fixed function of them: only the 5x5 support of the adjoint chain has to be decided.  own_planes=False (the C
    oracle keeps no planes, the reference's go in): d loss / d thin also reads t2 on the 3x3 around the pixel, so the support is 7x7."""
    gt, e = bpda_g_thin(u, thin, t2, m["low"], m["high"])
    gm = np.where(removed, gt * 0.0, gt)
    g, eb = _tail(m, gm, np.where(removed, 0.0, e), wts)
    return g, eb, _box(m["cls"] != UNDECIDED, 2 if own_planes else 3, np.logical_and)


# ---- cases -------------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 1, 28, 28), (2, 3, 32, 32), (2, 3, 26, 34), (2, 2, 13, 66), (2, 4, 9, 9), (2, 3, 25, 31)]


def _q(a):
    """k / 255 images as float32"""
    return (np.round(np.clip(a, 0, 1) * 255.0) / 255.0).astype(np.float32)


def mnist_like(shape, seed):
    """k / 255 strokes (1-3 pixels wide, values varying along the stroke) on an exact 0 background"""
    B, C, H, W = shape
    rng = np.random.RandomState(seed)
    x = np.zeros(shape, np.float64)
    for b in range(B):
        for s in range(max(2, (H * W) // 260)):
            i, j = rng.randint(2, max(3, H - 2)), rng.randint(2, max(3, W - 2))
            di, dj = [(0, 1), (1, 0), (1, 1), (1, -1)][rng.randint(4)]
            wd = 1 + rng.randint(3)
            for t in range(rng.randint(4, 4 + min(H, W) // 2)):
                ii, jj = i + t * di, j + t * dj
                if 0 <= ii < H and 0 <= jj < W:
                    v = rng.randint(40, 256) / 255.0
                    x[b, :, ii:ii + (wd if di == 0 else 1), jj:jj + (wd if dj == 0 else 1)] = v
    return _q(x), dict(alpha=0.3, low=25 / 255, high=51 / 255)


def cifar_pgd(shape, seed, eps=8 / 255):
    """k / 255 colour texture on half of every image, exact 0 elsewhere, plus a PGD iterate's perturbation x0 +- eps clamped to [0, 1]: the sign
    is drawn per quadrant on two images in three and per pixel on the third.  Where the background takes - eps the clamp returns it to 0."""
    B, C, H, W = shape
    rng = np.random.RandomState(seed)
    x0 = rng.randint(0, 256, size=shape) / 255.0
    for b in range(B):
        bg = np.zeros((H, W), bool)
        bg[:, :W // 2] = True if b % 2 == 0 else False
        bg[:H // 2, :] |= b % 2 == 1
        x0[b][:, bg] = 0.0
    sign = np.zeros(shape)
    for b in range(B):
        if b % 3 == 2:
            sign[b] = rng.choice([-1.0, 1.0], size=(C, H, W))
        else:
            for qi in range(2):
                for qj in range(2):
                    s = -1.0 if (x0[b][:, qi * H // 2:(qi + 1) * H // 2, qj * W // 2:(qj + 1) * W // 2] == 0).mean() > 0.6 else rng.choice([-1.0, 1.0])
                    sign[b][:, qi * H // 2:(qi + 1) * H // 2, qj * W // 2:(qj + 1) * W // 2] = s
    x = np.clip(x0.astype(np.float32) + np.float32(eps) * sign.astype(np.float32), np.float32(0), np.float32(1)).astype(np.float32)
    return x, dict(alpha=0.0, low=0.1, high=76 / 255)


def stripes(shape, seed):
    """Image 0: a stack of horizontal bands 1, 2 and 3 rows thick, every band one k / 255 level per channel over the full width (both
    polarities, ridges and plateaus).  The pattern is invariant under the horizontal shift, and a horizontal edge (gx = +-0, atan = +-pi/2,
    index 0) is compared with its horizontal neighbours: every pixel is a plateau tie, and !(mn > 0) removes it.  The levels cycle through three disjoint ranges,
    so no row has a vanishing gy.  Image 1: bars 1-3 pixels wide along the eight quantised orientations on an exact 0 background, the level
    drawn per pixel (a constant bar has a vanishing gradient on its axis, which no float32 evaluation has to reproduce)."""
    B, C, H, W = shape
    rng = np.random.RandomState(seed)
    x = np.zeros(shape, np.float64)
    ii, jj = np.mgrid[0:H, 0:W]
    for b in range(B):
        if b % 2 == 0:
            r, k = 0, 0
            while r < H:
                wd = 1 if (r == 0 or r >= H - 3) else 1 + rng.randint(3)  # one-row bands at the top and bottom: the clamp doubles them
                lo, hi = [(0, 60), (200, 255), (100, 160)][k % 3]      # the two neighbours of a band come from the two other ranges:
                x[b, :, r:r + wd, :] = (rng.randint(lo, hi + 1, size=C) / 255.0)[:, None, None]  # gy cannot cancel over the channels
                r, k = r + wd, k + 1
        elif min(H, W) < 12:  # too small for eight oriented regions: vertical bands (index 4, decided suppression) built the same way
            for c in range(C):
                j, k = 0, 0
                while j < W:
                    wd = 1 if (j == 0 or j >= W - 3) else 1 + rng.randint(3)
                    lo, hi = [(0, 60), (200, 255), (100, 160)][k % 3]
                    x[b, c, :, j:j + wd] = rng.randint(lo, hi + 1) / 255.0
                    j, k = j + wd, k + 1
        else:
            n = 0
            for (p, qd) in [(1, 1), (1, -1), (1, 2), (2, 1), (1, -2), (2, -1), (0, 1), (1, 0)]:
                t = p * ii + qd * jj
                off, wd = rng.randint(0, 6), 1 + (n % 3)
                band = ((t + off) % (9 * max(abs(p), abs(qd)))) < wd * max(abs(p), abs(qd))
                reg = (((ii * 3) // H) + 3 * ((jj * 3) // W)) == (n % 9)
                for c in range(C):
                    x[b, c][band & reg] = (rng.randint(60, 256, size=(H, W)) / 255.0)[band & reg]
                n += 1
    return _q(x), dict(alpha=0.05, low=0.2, high=0.6)


def ramp(shape, seed):
    """columns whose slope grows step by step, so the magnitude crosses alpha, low, high and high + 1.001 from left to right (values leave
    [0, 1]: the filter does not clamp), over an exact 0 band at the top; low = 0 puts every exact-zero t on its threshold"""
    B, C, H, W = shape
    rng = np.random.RandomState(seed)
    base = np.array([1, 2, 3, 4, 8, 10, 12, 25, 32, 40, 90, 96, 110, 130]) / 255.0   # the magnitude of a ramp is 4 x its slope
    if W < len(base):  # too narrow for every step: keep one slope on each side of every threshold and a run of the steepest
        base = np.array([1, 3, 10, 32, 96, 130, 130, 130, 130]) / 255.0
    slopes = base[(np.arange(W) * len(base)) // W]
    prof = np.concatenate([[0.0], np.cumsum(slopes)[:-1]])
    x = np.zeros(shape, np.float64)
    x[:, :, 4:, :] = prof[None, None, None, :]
    x[1:] = x[1:] * 0.5
    x = (np.round(x * 255.0) / 255.0).astype(np.float32)
    x[:, :, 4:, :] += (rng.randint(0, 2, size=(B, C, H - 4, W)) / 255.0).astype(np.float32) * (np.arange(W) % 5 == 0)
    return x.astype(np.float32), dict(alpha=12 / 255, low=0.0 if seed % 2 else 40 / 255, high=0.5)


def specials(shape, seed, eval_only=False):
    """+-0 mixtures; image 0 holds a vertical two-pixel bar of 1.0 (gy = +-0), image 1 a horizontal one (gx = +-0: atan(+-inf), index 0 after
    the wrap, horizontal plateau ties).  eval_only adds one NaN and one +-inf pixel each, away from the bars."""
    B, C, H, W = shape
    rng = np.random.RandomState(seed)
    x = np.zeros(shape, np.float32)
    x[rng.rand(*shape) < 0.5] = -0.0
    x[0, :, :, W // 2:W // 2 + 2] = np.float32(1.0)
    x[1, :, H // 2:H // 2 + 2, :] = np.float32(200 / 255)
    if eval_only:
        for b, c, i, j, v in special_pixels(shape):
            x[b, c, i, j] = v
    return x, dict(alpha=0.1, low=0.15, high=0.3)


def special_pixels(shape):
    B, C, H, W = shape
    return [(0, 0, 2, 2, np.nan), (1, C - 1, H - 3, 2, np.inf), (1, 0, 2, W - 3, -np.inf)]


def nonfinite_footprint(shape):
    """the pixels a NaN / inf input reaches: blur (3x3) then Sobel (3x3, zero-weight taps multiply) = its 5x5 neighbourhood in the image"""
    B, C, H, W = shape
    m = np.zeros((B, 1, H, W), bool)
    for b, c, i, j, v in special_pixels(shape):
        m[b, 0, max(0, i - 2):i + 3, max(0, j - 2):j + 3] = True
    return m


FAMILIES = {"mnist_like": mnist_like, "cifar_pgd": cifar_pgd, "stripes": stripes, "ramp": ramp, "specials": specials}


def cases():
    """(id, family, x, params): every family at the shapes its channel count allows; B >= 2 throughout"""
    out = []
    for fam, fn in FAMILIES.items():
        for k, shape in enumerate(SHAPES):
            if fam == "mnist_like" and shape[1] != 1:
                continue
            if fam == "cifar_pgd":
                if shape[1] != 3:
                    continue
                shape = (3,) + shape[1:]
            x, prm = fn(shape, 100 + 7 * k)
            out.append(("%s-%dx%dx%dx%d" % ((fam,) + tuple(shape)), fam, x, prm))
    return out


def upstream(shape, seed, C=None):
    """upstream gradients: small integers / 8, so products with the exact 1/2 stay exact"""
    rng = np.random.RandomState(seed)
    B, _, H, W = shape
    return (rng.randint(-16, 17, size=(B, C or 1, H, W)) / 8.0).astype(np.float32)


# ---- float32 magnitudes placed exactly on a threshold ------------------------------------------------------------------------------------------
# No operation order makes a sum of Gaussian weights exact, so no input puts a float32 magnitude on a NON-ZERO threshold for every evaluation.
# The threshold is therefore taken from the evaluation under test: its own float32 magnitude at a chosen pixel becomes alpha, high, or
# high + 1.001f, and a second run must then apply the STRICT rule there (mag == alpha keeps; mag == high is no edge, t == high is weak;
# |t - high| == 1.001f passes the gradient).  The reference classes such a pixel undecided; the rule at it is asserted by the tests.
def tie_pixel(m0, lo=0.0, hi=np.inf, rank=0.5):
    """a pixel of maps computed WITHOUT alpha mask whose direction and suppression are decided and which is kept: (b, i, j), chosen as the
    `rank` quantile by magnitude among those with lo < mag < hi"""
    ok = m0["rem_dec"] & ~m0["removed"] & m0["idx_dec"] & m0["finite"] & (m0["mag"] > 1e3 * m0["e_mag"]) & (m0["mag"] > lo) & (m0["mag"] < hi)
    ok &= _box(m0["cls"] != UNDECIDED, 2, np.logical_and)
    cand = np.argwhere(ok[:, 0])
    if not len(cand):
        return None
    mag, e = m0["mag"][:, 0], m0["e_mag"][:, 0]
    order = np.argsort(mag[ok[:, 0]])
    start = min(len(cand) - 1, int(rank * len(cand)))
    H, W = mag.shape[-2:]
    for k in list(order[start:]) + list(order[:start][::-1]):
        b, i, j = (int(v) for v in cand[k])
        blk = (slice(max(0, i - 2), i + 3), slice(max(0, j - 2), j + 3))
        near = np.abs(mag[b][blk] - mag[b, i, j]) <= 4 * (e[b][blk] + e[b, i, j])   # no other magnitude of the 5x5 within rounding of this one
        if near.sum() == 1:
            return b, i, j
    return None


def high_for_1001(t32):
    """a float32 `high` with fabsf(t - high) == 1.001f bit for bit in float32, or None"""
    t32, c = np.float32(t32), np.float32(1.001)
    h = np.float32(t32 - c)
    for _ in range(64):
        d = np.float32(np.abs(np.float32(t32 - h)))
        if d == c:
            return float(h)
        h = np.nextafter(h, np.float32(-np.inf) if d < c else np.float32(np.inf))
    return None


def next_up(v):
    return float(np.nextafter(np.float32(v), np.float32(np.inf)))


def next_down(v):
    return float(np.nextafter(np.float32(v), np.float32(-np.inf)))


def force_ste(m, p, value):
    """maps with the straight-through gate at pixel p set by rule, the pixel classed an exact tie (every other decision at p must be decided)"""
    b, i, j = p
    assert m["alpha_dec"][b, 0, i, j] and m["idx_dec"][b, 0, i, j] and m["rem_dec"][b, 0, i, j] and m["t2_dec"][b, 0, i, j] and m["zero_known"][b, 0, i, j]
    out = dict(m)
    out["ste"], out["cls"] = m["ste"].copy(), m["cls"].copy()
    out["ste"][b, 0, i, j], out["cls"][b, 0, i, j] = value, TIE
    return out


def _force_mag(m, p, value):
    """maps for backward125 with the magnitude at p set by rule (within its bound of the float64 one), the pixel classed an exact tie"""
    b, i, j = p
    assert abs(m["mag"][b, 0, i, j] - value) <= m["e_mag"][b, 0, i, j]
    out = dict(m)
    out["mag"], out["magA"], out["cls125"] = m["mag"].copy(), m["magA"].copy(), m["cls125"].copy()
    out["mag"][b, 0, i, j] = out["magA"][b, 0, i, j] = value
    out["cls125"][b, 0, i, j] = TIE
    return out


TIE_BASES = ("mnist_like-2x1x28x28", "cifar_pgd-3x3x32x32", "stripes-2x3x26x34", "stripes-2x2x13x66", "stripes-2x3x25x31")


def threshold_tie_checks(x, prm, wts, ev):
    """Puts the float32 magnitude of the evaluation `ev` itself on alpha, on high and 1.001f above high, and holds `ev` to the strict rule there.
    ev: callables on numpy arrays - mag(x), edge125(x, a, hi), grad125(x, u, a, hi), canny(x, a, lo, hi), canny_grad(x, u, a, lo, hi),
    bpda_edge(x, lo, hi), and bpda_planes(x, lo, hi) -> (thin, t2) or None.  Returns the names of the checks that ran."""
    ran = []
    m0 = forward(x, wts, 0.0, prm["low"], prm["high"], "canny")
    mag32 = ev["mag"](x)
    u = upstream(x.shape, 23)
    p = tie_pixel(m0, lo=0.05, hi=0.9, rank=0.5)
    if p is not None:
        b, i, j = p
        q = (b, 0, i, j)
        u[q] = 2.0
        v = float(mag32[q])
        # ---- mag == alpha: `mag < alpha` is false, the pixel is kept (core.py:264, :575) ----
        a, lo, hi = v, v / 4, v / 2
        e = ev["edge125"](x, a, hi)
        assert e[q] == 1.0, "step125: mag == alpha must keep the pixel (strict <)"
        assert ev["edge125"](x, next_up(a), hi)[q] == 0.0, "step125: one ulp above, alpha masks the pixel"
        m = forward(x, wts, a, lo, hi, "canny")
        check_edge(e, m["edge125"], m["edge125_dec"], "edge125 at mag == alpha")
        mf = _force_mag(m, p, max(v, m["mag"][q]))
        g, eb, comp = backward125(mf, u, wts)
        assert comp[q]
        check_grad(ev["grad125"](x, u, a, hi), g, eb, comp, "step125 gradient at mag == alpha")
        ec = ev["canny"](x, a, lo, hi)
        assert ec[q] == 1.0 and ev["canny"](x, next_up(a), lo, hi)[q] == 0.0, "canny: mag == alpha must keep the pixel"
        check_edge(ec, m["edge"], m["edge_dec"], "canny edge at mag == alpha")
        ran.append("alpha")
        # ---- mag == high: `magA > high` is false, no edge and no gradient (To_compare, core.py:343-357) ----
        e = ev["edge125"](x, 0.0, v)
        assert e[q] == 0.0, "step125: mag == high is not an edge (strict >)"
        assert ev["edge125"](x, 0.0, next_down(v))[q] == 1.0, "step125: one ulp below, the pixel is an edge"
        m = forward(x, wts, 0.0, v / 2, v, "canny")
        check_edge(e, m["edge125"], m["edge125_dec"], "edge125 at mag == high")
        g, eb, comp = backward125(_force_mag(m, p, min(v, m["mag"][q])), u, wts)
        g_on = backward125(_force_mag(m, p, float(np.nextafter(max(v, m["mag"][q]), np.inf))), u, wts)[0]
        assert comp[q] and (np.abs(np.nan_to_num(g - g_on)) > 4 * eb)[comp].any(), "the gate at mag == high must show in the gradient"
        check_grad(ev["grad125"](x, u, 0.0, v), g, eb, comp, "step125 gradient at mag == high")
        ran.append("high125")
        # ---- t == high: `t - high > 0` is false, the pixel is weak (t2 = 0.5), exactly as with high one ulp up ----
        for name, f in (("canny", lambda h: ev["canny"](x, 0.0, v / 2, h)), ("bpda", lambda h: ev["bpda_edge"](x, v / 2, h))):
            ee = f(v)
            assert np.array_equal(ee, f(next_up(v))), name + ": t == high must behave as t < high"
            check_edge(ee, m["edge"], m["edge_dec"], name + " edge at t == high")
            t2f = m["t2"].copy()
            t2f[q] = 0.5
            nb = m["t2_dec"].copy()
            nb[q] = True
            if _box(nb, 1, np.logical_and)[q]:
                hs = sum(_shift0(t2f, dr, dc) for dr in (-1, 0, 1) for dc in (-1, 0, 1))
                assert ee[q] == float(1.25 * hs[q] > 1.0), name + ": a weak pixel at t == high is an edge only through hysteresis"
        planes = ev["bpda_planes"](x, v / 2, v)
        if planes is not None:
            thin, t2 = planes
            assert thin[q] == mag32[q] and t2[q] == 0.5, "stored planes at t == high: thin = mag, t2 = 0.5"
            assert ev["bpda_planes"](x, v / 2, next_down(v))[1][q] == 1.0
        ran.append("high")
    # ---- |t - high| == 1.001f: `fabsf(t - high) > 1.001f` is false, the gradient passes (core.py:138-145) ----
    p = tie_pixel(m0, lo=1.1, rank=0.5)
    if p is not None:
        b, i, j = p
        q = (b, 0, i, j)
        h = high_for_1001(mag32[q])
        assert h is not None
        u = upstream(x.shape, 29)
        u[q] = 2.0
        m = forward(x, wts, prm["alpha"], prm["low"], h, "canny")
        g, eb, comp = backward_canny(force_ste(m, p, True), u, wts)
        g_off = backward_canny(force_ste(m, p, False), u, wts)[0]
        assert comp[q] and (np.abs(np.nan_to_num(g - g_off)) > 4 * eb)[comp].any(), "the gate must show in the gradient"
        check_grad(ev["canny_grad"](x, u, prm["alpha"], prm["low"], h), g, eb, comp, "canny gradient at |t - high| == 1.001f")
        ran.append("ste")
    return ran
