"""Tensor-level wrappers over the C ABI (include/eeadv.h).

Every function takes ROCm tensors, checks device / dtype / contiguity / shape on the host (a wrong shape
must never reach a kernel), and enqueues ONE library call on torch's current HIP stream.  Nothing here
computes on the CPU and nothing falls back to torch ops: a CPU tensor raises.
"""
import ctypes

import numpy as np
import torch

from . import _native as N

_INF = float("inf")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t, dtype, name, shape=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a tensor" % name)
    if not t.is_cuda:
        raise N.EEError("%s is on %s: the eeadv kernels only run on a ROCm device (no CPU fallback)" % (name, t.device))
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("%s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
    return ctypes.c_void_p(t.data_ptr())


def _opt(t, dtype, name, shape=None):
    return None if t is None else _chk(t, dtype, name, shape)


# ---- fixed 3x3 weights (utils/core.py:58-84, restated in numpy float64 then cast like core.py:164,177,180) ----
def gaussian_kernel_np(k=3, mu=0, sigma=1, normalize=True):
    g1 = np.linspace(-1, 1, k)
    x, y = np.meshgrid(g1, g1)
    d = (x ** 2 + y ** 2) ** 0.5
    g2 = np.exp(-(d - mu) ** 2 / (2 * sigma ** 2))
    g2 = g2 / (2 * np.pi * sigma ** 2)
    if normalize:
        g2 = g2 / np.sum(g2)
    return g2


def sobel_kernel_np(k=3):
    rng = np.linspace(-(k // 2), k // 2, k)
    x, y = np.meshgrid(rng, rng)
    den = x ** 2 + y ** 2
    den[:, k // 2] = 1
    return x / den


# k*45 degrees -> (drow, dcol) of the -1 tap of the directional kernel relative to its centre (core.py:87-112).
# DERIVED (the reference rotates [0,0,1,-1,-1] with cv2, which is unavailable): parity unpinned.
CANNY_DIRS = np.array([(0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1)], dtype=np.int32)


class EdgeWeights:
    """The 27 host floats every edge kernel takes (Gaussian, Sobel-x, Sobel-y) + the full filter's direction table."""

    def __init__(self, sigma=1.0, mu=0.0):
        self.dirs = np.ascontiguousarray(CANNY_DIRS.reshape(-1), dtype=np.int32)
        self.dirs_ptr = self.dirs.ctypes.data_as(ctypes.c_void_p)
        g = gaussian_kernel_np(3, mu, sigma).astype(np.float32).reshape(9)
        s = sobel_kernel_np(3)
        self.host = np.concatenate([g, s.astype(np.float32).reshape(9), s.T.astype(np.float32).reshape(9)])
        self.host = np.ascontiguousarray(self.host, dtype=np.float32)
        self.ptr = self.host.ctypes.data_as(ctypes.c_void_p)


# ---- PGD family ------------------------------------------------------------------------------------------
def pgd_init(x0, noise, lo=0.0, hi=1.0, out=None):
    p0 = _chk(x0, torch.float32, "x0")
    pn = _chk(noise, torch.float32, "noise", x0.shape)
    out = torch.empty_like(x0) if out is None else out
    po = _chk(out, torch.float32, "out", x0.shape)
    N.check(N.lib.ee_pgd_init_f32(po, p0, pn, x0.numel(), lo, hi, _stream()), "ee_pgd_init_f32")
    return out


def pgd_init_rng(x0, scale, dist, seed, offset, lo=0.0, hi=1.0, out=None):
    p0 = _chk(x0, torch.float32, "x0")
    out = torch.empty_like(x0) if out is None else out
    po = _chk(out, torch.float32, "out", x0.shape)
    N.check(N.lib.ee_pgd_init_rng_f32(po, p0, x0.numel(), scale, dist, seed, offset, lo, hi, _stream()),
            "ee_pgd_init_rng_f32")
    return out


def pgd_step_(x, g, x0, alpha, eps, lo=0.0, hi=1.0, direction=1):
    """In place on x (attacks.py:25-27)."""
    px = _chk(x, torch.float32, "x")
    pg = _chk(g, torch.float32, "g", x.shape)
    p0 = _chk(x0, torch.float32, "x0", x.shape)
    N.check(N.lib.ee_pgd_step_f32(px, pg, p0, x.numel(), alpha, eps, lo, hi, direction, _stream()), "ee_pgd_step_f32")
    return x


def pgd_step_bcast_(x, g_lp, g_edge, x0, alpha, eps, lo=0.0, hi=1.0, direction=1):
    B, C, H, W = x.shape
    px = _chk(x, torch.float32, "x")
    pl = _chk(g_lp, torch.float32, "g_lp", x.shape)
    pe = _chk(g_edge, torch.float32, "g_edge", (B, 1, H, W))
    p0 = _chk(x0, torch.float32, "x0", x.shape)
    N.check(N.lib.ee_pgd_step_bcast_f32(px, pl, pe, p0, B, C, H * W, alpha, eps, lo, hi, direction, _stream()),
            "ee_pgd_step_bcast_f32")
    return x


def l2_step_(x, g, x0, step, eps, lo=0.0, hi=1.0):
    """In place on x [B, ...]: the TRADES L2 update (attacks.py:389-400)."""
    B = x.shape[0]
    px = _chk(x, torch.float32, "x")
    pg = _chk(g, torch.float32, "g", x.shape)
    p0 = _chk(x0, torch.float32, "x0", x.shape)
    if B:
        N.check(N.lib.ee_l2_step_f32(px, pg, p0, B, x.numel() // B, step, eps, lo, hi, _stream()), "ee_l2_step_f32")
    return x


def fgsm_step(x, g, alpha, lo=0.0, hi=1.0, direction=1):
    px = _chk(x, torch.float32, "x")
    pg = _chk(g, torch.float32, "g", x.shape)
    out = torch.empty_like(x)
    N.check(N.lib.ee_fgsm_step_f32(_chk(out, torch.float32, "out"), px, pg, x.numel(), alpha, lo, hi, direction, _stream()),
            "ee_fgsm_step_f32")
    return out


def add_clamp(x, delta, lo=0.0, hi=1.0):
    px = _chk(x, torch.float32, "x")
    pd = _chk(delta, torch.float32, "delta", x.shape)
    out = torch.empty_like(x)
    N.check(N.lib.ee_add_clamp_f32(_chk(out, torch.float32, "out"), px, pd, x.numel(), lo, hi, _stream()), "ee_add_clamp_f32")
    return out


def freeat_update_(delta, g, alpha, eps):
    """delta[:n] updated in place, n = g.numel() (the live rows of the persistent noise buffer)."""
    pd = _chk(delta, torch.float32, "delta")
    pg = _chk(g, torch.float32, "g")
    if g.numel() > delta.numel():
        raise ValueError("gradient has more elements than the noise buffer")
    N.check(N.lib.ee_freeat_update_f32(pd, pg, g.numel(), alpha, eps, _stream()), "ee_freeat_update_f32")
    return delta


def freeat_update_masked_(delta, g_in1, x, alpha, eps):
    """delta[:n] += alpha*sign(g_in1 * 1[0 <= x + delta <= 1]); clamp(+-eps); n = x.numel()."""
    pd = _chk(delta, torch.float32, "delta")
    pg = _chk(g_in1, torch.float32, "g_in1", x.shape)
    px = _chk(x, torch.float32, "x")
    if x.numel() > delta.numel():
        raise ValueError("batch has more elements than the noise buffer")
    N.check(N.lib.ee_freeat_update_masked_f32(pd, pg, px, x.numel(), alpha, eps, _stream()), "ee_freeat_update_masked_f32")
    return delta


# ---- fast adversarial training (ee_fastat.hip) --------------------------------------------------
def _host_plumbing(what, *tensors):
    """True when every tensor is on the CPU and the caller opted into the host plumbing (eeadv.runtime.allow_cpu_plumbing, what --no-cuda
    does); a CPU tensor without the opt-in raises, a mix of devices falls through to _chk, which refuses it."""
    from . import runtime
    live = [t for t in tensors if t is not None]
    return bool(live) and not any(t.is_cuda for t in live) and not runtime.require_device(live[0], what)


def fastat_draw_host(n, eps, seed, step):
    """The U(-eps, eps) draw of ee_fastat_start_f32 for elements 0 .. n-1 in numpy float32, bit for bit: one Philox call (stream 0) per
    group of four elements at counter (step << 32) + (i >> 2), u = (word >> 8) 2^-24, then u * (eps - (-eps)) + (-eps), 0 + that, and
    the clamp to [-eps, eps], each rounded to float32 once."""
    from .sqatk import philox4x32
    n, e = int(n), np.float32(eps)
    ctr = (np.uint64((int(step) << 32) & 0xFFFFFFFFFFFFFFFF) + np.arange((n + 3) // 4, dtype=np.uint64))
    u = (philox4x32(seed, ctr, 0) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    z = np.float32(0.0) + (u * (e - (-e)) + (-e))
    return np.ascontiguousarray(np.clip(z, -e, e).reshape(-1)[:n], dtype=np.float32)


def fastat_start_(delta, in1, x, eps, seed=0, step=None, noise=None):
    """The start of a fast-AT batch (main_fast.py:224-225, 233-235), n = x.numel(): delta[:n] = noise (as bits) or, with noise None, the
    U(-eps, eps) draw keyed by (seed, step[0]) - `step` a device int64 [1] tensor read as the uint64 counter, which this launch never
    writes; in1 = clamp(x + delta[:n], 0, 1).  delta is the flat persistent buffer (>= n elements), in1 has x's shape.  CPU tensors under
    the host plumbing: the same bits from fastat_draw_host and torch ops."""
    n = x.numel()
    if delta.numel() < n:
        raise ValueError("batch has more elements than the noise buffer")
    if noise is None and step is None:
        raise ValueError("fastat_start_ draws its noise from (seed, step): give the step counter, or the noise")
    if not float(eps) >= 0.0:
        raise ValueError("eps must be >= 0, got %r" % (eps,))
    if _host_plumbing("fastat_start_", delta, in1, x, noise, step):
        d = delta.view(-1)[:n]
        if noise is not None:
            d.copy_(noise.reshape(-1))
        else:
            d.copy_(torch.from_numpy(fastat_draw_host(n, eps, seed, int(step.view(-1)[0]))))
        in1.copy_(torch.clamp(x + d.view(x.shape), 0.0, 1.0))
        return in1
    px = _chk(x, torch.float32, "x")
    pd = _chk(delta, torch.float32, "delta")
    pi = _chk(in1, torch.float32, "in1", x.shape)
    N.check(N.lib.ee_fastat_start_f32(pd, pi, px, _opt(noise, torch.float32, "noise", x.shape), n, eps, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                      None if noise is not None else _chk(step, torch.int64, "step", (1,)), _stream()), "ee_fastat_start_f32")
    return in1


def fastat_ascend_(delta, in1, g, x, alpha, eps, step=None):
    """The noise update and the descend pass's input in one launch (main_fast.py:246-253): freeat_update_masked_(delta, g, x, alpha, eps)
    then in1 = add_clamp(x, delta[:n]), bit for bit; afterwards step[0] += 1 (`step`: device int64 [1] or None).  in1 may be g."""
    n = x.numel()
    if delta.numel() < n:
        raise ValueError("batch has more elements than the noise buffer")
    if _host_plumbing("fastat_ascend_", delta, in1, g, x, step):
        d = delta.view(-1)[:n].view(x.shape)
        s = x + d
        gd = torch.where((s >= 0) & (s <= 1), g, torch.zeros_like(g))
        d.copy_(torch.clamp(d + alpha * torch.sign(gd), -eps, eps))
        in1.copy_(torch.clamp(x + d, 0.0, 1.0))
        if step is not None:
            step += 1
        return in1
    px = _chk(x, torch.float32, "x")
    pd = _chk(delta, torch.float32, "delta")
    pi = _chk(in1, torch.float32, "in1", x.shape)
    pg = _chk(g, torch.float32, "g", x.shape)
    N.check(N.lib.ee_fastat_ascend_f32(pd, pi, pg, px, n, alpha, eps, _opt(step, torch.int64, "step", (1,)), _stream()), "ee_fastat_ascend_f32")
    return in1


def fastat_keep_(final, x, logits=None, labels=None, first=False):
    """The union across PGD restarts (lib/validation.py:51-57), in place on final [B, ...]: `first` copies every row of x; otherwise the rows
    whose arg-max logit (torch.max(1)[1]'s: lowest index among equal maxima, the first NaN of a row that holds one) differs from the label."""
    B = final.shape[0]
    if tuple(x.shape) != tuple(final.shape):
        raise ValueError("x has shape %s, expected %s" % (tuple(x.shape), tuple(final.shape)))
    if B and final.data_ptr() == x.data_ptr():
        raise ValueError("fastat_keep_ writes final while it reads x: they must be two tensors")
    if not first and (logits is None or labels is None):
        raise ValueError("fastat_keep_ needs logits and labels unless first")
    if _host_plumbing("fastat_keep_", final, x, logits, labels):
        if first:
            final.copy_(x)
        else:
            I = logits.max(1)[1] != labels
            final[I] = x[I]
        return final
    pf = _chk(final, torch.float32, "final")
    px = _chk(x, torch.float32, "x")
    K = 1
    if not first:
        if logits.dim() != 2 or logits.shape[0] != B:
            raise ValueError("logits has shape %s, expected [%d, K]" % (tuple(logits.shape), B))
        K = logits.shape[1]
    N.check(N.lib.ee_fastat_keep_f32(pf, px, None if first else _chk(logits, torch.float32, "logits"),
                                     None if first else _chk(labels, torch.int64, "labels", (B,)), B, K, final.numel() // B if B else 1,
                                     1 if first else 0, _stream()), "ee_fastat_keep_f32")
    return final


def avmix(x, x0, wgt, gamma):
    B = x.shape[0]
    px = _chk(x, torch.float32, "x")
    p0 = _chk(x0, torch.float32, "x0", x.shape)
    pw = _chk(wgt, torch.float64, "wgt", (B,))
    out = torch.empty_like(x)
    N.check(N.lib.ee_avmix_f32(_chk(out, torch.float32, "out"), px, p0, pw, B, x.numel() // max(B, 1), gamma, _stream()),
            "ee_avmix_f32")
    return out


def avmix_labels(labels, wgt, K, lambda1, lambda2):
    B = labels.shape[0]
    pl = _chk(labels, torch.int64, "labels", (B,))
    pw = _chk(wgt, torch.float64, "wgt", (B,))
    out = torch.empty((B, K), dtype=torch.float64, device=labels.device)
    N.check(N.lib.ee_avmix_labels_f64(_chk(out, torch.float64, "out"), pl, pw, B, K, lambda1, lambda2, _stream()),
            "ee_avmix_labels_f64")
    return out


# ---- edge filter / front end ---------------------------------------------------------------------------------
def edge125_fwd(x, wts, alpha, high, want_mag=False):
    B, C, H, W = x.shape
    px = _chk(x, torch.float32, "x")
    edge = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device)
    mag = torch.empty_like(edge) if want_mag else None
    N.check(N.lib.ee_edge125_fwd_f32(px, B, C, H, W, wts.ptr, alpha, high, _chk(edge, torch.float32, "edge"),
                                     _opt(mag, torch.float32, "mag"), _stream()), "ee_edge125_fwd_f32")
    return (edge, mag) if want_mag else edge


def edge125_bwd(x, u, wts, alpha, high):
    B, C, H, W = x.shape
    px = _chk(x, torch.float32, "x")
    pu = _chk(u, torch.float32, "u", (B, 1, H, W))
    g = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device)
    N.check(N.lib.ee_edge125_bwd_f32(px, pu, B, C, H, W, wts.ptr, alpha, high, _chk(g, torch.float32, "g"), _stream()),
            "ee_edge125_bwd_f32")
    return g


def frontend_fwd(x, x_hfs, wts, alpha, high, w, want_edge=False):
    B, C, H, W = x.shape
    px = _chk(x, torch.float32, "x")
    ph = _chk(x_hfs, torch.float32, "x_hfs", x.shape)
    x_in = torch.empty_like(x)
    gate = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    edge = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device) if want_edge else None
    N.check(N.lib.ee_frontend_fwd_f32(px, ph, B, C, H, W, wts.ptr, alpha, high, w, _chk(x_in, torch.float32, "x_in"),
                                      _chk(gate, torch.uint8, "gate"), _opt(edge, torch.float32, "edge"), _stream()),
            "ee_frontend_fwd_f32")
    return x_in, gate, edge


def frontend_bwd(g_in, gate, x, wts, alpha, high, w):
    B, C, H, W = x.shape
    pg = _chk(g_in, torch.float32, "g_in", x.shape)
    pt = _chk(gate, torch.uint8, "gate", x.shape)
    px = _chk(x, torch.float32, "x")
    g_hfs = torch.empty_like(x)
    g_edge = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device)
    N.check(N.lib.ee_frontend_bwd_f32(pg, pt, px, B, C, H, W, wts.ptr, alpha, high, w, _chk(g_hfs, torch.float32, "g_hfs"),
                                      _chk(g_edge, torch.float32, "g_edge"), _stream()), "ee_frontend_bwd_f32")
    return g_hfs, g_edge


def frontend_fwd_save(x, x_hfs, wts, alpha, high, w, want_edge=False):
    """frontend_fwd that also keeps the Sobel responses for frontend_bwd_saved: returns (x_in, gate, edge, gx, gy)."""
    B, C, H, W = x.shape
    px = _chk(x, torch.float32, "x")
    ph = _chk(x_hfs, torch.float32, "x_hfs", x.shape)
    x_in = torch.empty_like(x)
    gate = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    edge = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device) if want_edge else None
    gx = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device)
    gy = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device)
    N.check(N.lib.ee_frontend_fwd_save_f32(px, ph, B, C, H, W, wts.ptr, alpha, high, w, _chk(x_in, torch.float32, "x_in"),
                                           _chk(gate, torch.uint8, "gate"), _opt(edge, torch.float32, "edge"), gx.data_ptr(), gy.data_ptr(),
                                           _stream()), "ee_frontend_fwd_save_f32")
    return x_in, gate, edge, gx, gy


def frontend_bwd_saved(g_in, gate, gx, gy, wts, alpha, high, w):
    """Backward of the front end from the saved Sobel responses (no x, no recomputation): (g_hfs, g_edge), bit-identical to
    frontend_bwd."""
    B, C, H, W = g_in.shape
    pg = _chk(g_in, torch.float32, "g_in")
    pt = _chk(gate, torch.uint8, "gate", g_in.shape)
    g_hfs = torch.empty_like(g_in)
    g_edge = torch.empty((B, 1, H, W), dtype=torch.float32, device=g_in.device)
    N.check(N.lib.ee_frontend_bwd_saved_f32(pg, pt, _chk(gx, torch.float32, "gx", (B, 1, H, W)), _chk(gy, torch.float32, "gy", (B, 1, H, W)),
                                            B, C, H, W, wts.ptr, alpha, high, w, g_hfs.data_ptr(), g_edge.data_ptr(), _stream()),
            "ee_frontend_bwd_saved_f32")
    return g_hfs, g_edge


def canny_fwd(x, wts, alpha, low, high):
    B, C, H, W = x.shape
    edge = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device)
    N.check(N.lib.ee_canny_fwd_f32(_chk(x, torch.float32, "x"), None, B, C, H, W, wts.ptr, wts.dirs_ptr, alpha, low, high, 0.0,
                                   _chk(edge, torch.float32, "edge"), None, None, _stream()), "ee_canny_fwd_f32")
    return edge


def canny_bwd(x, u, wts, alpha, low, high):
    B, C, H, W = x.shape
    g = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device)
    N.check(N.lib.ee_canny_bwd_f32(_chk(x, torch.float32, "x"), _chk(u, torch.float32, "u", (B, 1, H, W)), None, None, B, C, H, W, wts.ptr,
                                   wts.dirs_ptr, alpha, low, high, 0.0, _chk(g, torch.float32, "g"), None, _stream()), "ee_canny_bwd_f32")
    return g


def canny_bpda_fwd(x, wts, low, high):
    """CannyFilter_BPDA forward (core.py:426-505) -> (edge, thin, t2); thin / t2 are the backward's saved state."""
    B, C, H, W = x.shape
    edge, thin, t2 = (torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device) for _ in range(3))
    N.check(N.lib.ee_canny_bpda_fwd_f32(_chk(x, torch.float32, "x"), B, C, H, W, wts.ptr, wts.dirs_ptr, low, high, edge.data_ptr(),
                                        thin.data_ptr(), t2.data_ptr(), _stream()), "ee_canny_bpda_fwd_f32")
    return edge, thin, t2


def canny_bpda_bwd(x, u, thin, t2, wts, low, high):
    B, C, H, W = x.shape
    g = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device)
    scratch = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device)
    N.check(N.lib.ee_canny_bpda_bwd_f32(_chk(x, torch.float32, "x"), _chk(u, torch.float32, "u", (B, 1, H, W)),
                                        _chk(thin, torch.float32, "thin", (B, 1, H, W)), _chk(t2, torch.float32, "t2", (B, 1, H, W)), B, C, H,
                                        W, wts.ptr, wts.dirs_ptr, low, high, scratch.data_ptr(), g.data_ptr(), _stream()),
            "ee_canny_bpda_bwd_f32")
    return g


def canny_frontend_fwd(x, x_hfs, wts, alpha, low, high, w, want_edge=False):
    B, C, H, W = x.shape
    x_in = torch.empty_like(x)
    gate = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    edge = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device) if want_edge else None
    N.check(N.lib.ee_canny_fwd_f32(_chk(x, torch.float32, "x"), _chk(x_hfs, torch.float32, "x_hfs", x.shape), B, C, H, W, wts.ptr,
                                   wts.dirs_ptr, alpha, low, high, w, _opt(edge, torch.float32, "edge"), _chk(x_in, torch.float32, "x_in"),
                                   _chk(gate, torch.uint8, "gate"), _stream()), "ee_canny_fwd_f32")
    return x_in, gate, edge


def canny_frontend_bwd(g_in, gate, x, wts, alpha, low, high, w):
    B, C, H, W = x.shape
    g_hfs = torch.empty_like(x)
    g_edge = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device)
    N.check(N.lib.ee_canny_bwd_f32(_chk(x, torch.float32, "x"), None, _chk(g_in, torch.float32, "g_in", x.shape),
                                   _chk(gate, torch.uint8, "gate", x.shape), B, C, H, W, wts.ptr, wts.dirs_ptr, alpha, low, high, w,
                                   _chk(g_edge, torch.float32, "g_edge"), _chk(g_hfs, torch.float32, "g_hfs"), _stream()),
            "ee_canny_bwd_f32")
    return g_hfs, g_edge


# ---- losses ------------------------------------------------------------------------------------------------------
def _inv(n):
    """1/n with torch's semantics for an empty reduction: the mean of nothing is NaN (0 * NaN in the reduce kernel)."""
    return 1.0 / n if n else float("nan")


def _reduce_rows(rows, scale):
    out = torch.empty(1, dtype=torch.float64, device=rows.device)
    N.check(N.lib.ee_reduce_rows_f64(_chk(rows, torch.float64, "rows"), rows.numel(), scale, _chk(out, torch.float64, "out"),
                                     _stream()), "ee_reduce_rows_f64")
    return out


def ce(logits, labels, reduction="mean", smoothing=0.0, want_loss=True, want_grad=True):
    """Returns (loss: 0-dim fp32 tensor or None, dlogits or None)."""
    B, K = logits.shape
    pz = _chk(logits, torch.float32, "logits")
    py = _chk(labels, torch.int64, "labels", (B,))
    gscale = _inv(B) if reduction == "mean" else 1.0
    rows = torch.empty(B, dtype=torch.float64, device=logits.device) if want_loss else None
    d = torch.empty_like(logits) if want_grad else None
    N.check(N.lib.ee_ce_f32(pz, py, B, K, smoothing, gscale, _opt(rows, torch.float64, "rows"), _opt(d, torch.float32, "d"),
                            _stream()), "ee_ce_f32")
    loss = _reduce_rows(rows, gscale)[0].to(torch.float32) if want_loss else None
    return loss, d


def fc_ce_grad_supported(z1, w2):
    return z1.dim() == 2 and w2.dim() == 2 and w2.shape[1] == z1.shape[1] and w2.shape[0] <= 64 and z1.shape[1] <= 8192


def fc_ce_grad(z1, w2, b2, labels, reduction="sum", want_logits=False):
    """d CrossEntropyLoss(fc2(relu(z1)), labels) / d z1 in one launch (ee_loss.hip: fc_ce_grad_kernel): z1 [B,Hd], w2 [K,Hd], b2 [K] or None.
    Returns dz1, or (dz1, logits)."""
    B, Hd = z1.shape
    K = w2.shape[0]
    dz = torch.empty_like(z1)
    lg = torch.empty((B, K), dtype=torch.float32, device=z1.device) if want_logits else None
    N.check(N.lib.ee_fc_ce_grad_f32(_chk(z1, torch.float32, "z1"), _chk(w2, torch.float32, "w2", (K, Hd)), _opt(b2, torch.float32, "b2"),
                                    _chk(labels, torch.int64, "labels", (B,)), dz.data_ptr(), _opt(lg, torch.float32, "logits"), B, Hd, K,
                                    _inv(B) if reduction == "mean" else 1.0, _stream()), "ee_fc_ce_grad_f32")
    return (dz, lg) if want_logits else dz


def kl_batchmean(zq, zp, want_loss=True, want_dq=True, want_dp=False):
    B, K = zq.shape
    pq = _chk(zq, torch.float32, "zq")
    pp = _chk(zp, torch.float32, "zp", zq.shape)
    rows = torch.empty(B, dtype=torch.float64, device=zq.device) if want_loss else None
    dq = torch.empty_like(zq) if want_dq else None
    dp = torch.empty_like(zq) if want_dp else None
    N.check(N.lib.ee_kl_f32(pq, pp, B, K, _inv(B), _opt(rows, torch.float64, "rows"), _opt(dq, torch.float32, "dq"),
                            _opt(dp, torch.float32, "dp"), _stream()), "ee_kl_f32")
    loss = _reduce_rows(rows, _inv(B))[0].to(torch.float32) if want_loss else None
    return loss, dq, dp


def softce(z, t, scale, want_loss=True, want_grad=True):
    """-sum(log_softmax(z) * t) * scale with float64 targets; loss and gradient are float64."""
    B, K = z.shape
    pz = _chk(z, torch.float32, "z")
    pt = _chk(t, torch.float64, "t", z.shape)
    rows = torch.empty(B, dtype=torch.float64, device=z.device) if want_loss else None
    dz = torch.empty((B, K), dtype=torch.float64, device=z.device) if want_grad else None
    N.check(N.lib.ee_softce_f64(pz, pt, B, K, scale, _opt(rows, torch.float64, "rows"), _opt(dz, torch.float64, "dz"),
                                _stream()), "ee_softce_f64")
    loss = _reduce_rows(rows, scale)[0] if want_loss else None
    return loss, dz


def mse(a, b, want_loss=True, want_grad=True):
    pa = _chk(a, torch.float32, "a")
    pb = _chk(b, torch.float32, "b", a.shape)
    n = a.numel()
    nb = N.lib.ee_mse_num_partials(n)
    part = torch.empty(nb, dtype=torch.float64, device=a.device) if want_loss else None
    da = torch.empty_like(a) if want_grad else None
    N.check(N.lib.ee_mse_f32(pa, pb, n, 2.0 * _inv(n), _opt(part, torch.float64, "part"), _opt(da, torch.float32, "da"), _stream()),
            "ee_mse_f32")
    loss = _reduce_rows(part, _inv(n))[0].to(torch.float32) if want_loss else None
    return loss, da


def topk(logits, labels, k):
    """(idx [B,k] int64, correct [k] int64 or None)."""
    B, K = logits.shape
    pz = _chk(logits, torch.float32, "logits")
    idx = torch.empty((B, k), dtype=torch.int64, device=logits.device)
    correct = torch.empty(k, dtype=torch.int64, device=logits.device) if labels is not None else None
    N.check(N.lib.ee_topk_i64(pz, _opt(labels, torch.int64, "labels", (B,)), B, K, k, _chk(idx, torch.int64, "idx"),
                              _opt(correct, torch.int64, "correct"), _stream()), "ee_topk_i64")
    return idx, correct


# ---- APGD (ee_apgd.hip) ----------------------------------------------------------------------------------------------
APGD_KINDS = {"ce": 0, "dlr": 1, "dlr_t": 2}  # EE_APGD_CE / _DLR / _DLR_T
APGD_F_STEP, APGD_F_LOSS_BEST, APGD_F_PREV, APGD_F_LOSS_BEST_LAST = range(4)  # rows of fstate
APGD_I_INC, APGD_I_REDUCED_LAST, APGD_I_ROBUST, APGD_I_FLAGS = range(4)  # rows of istate
APGD_IMPROVED, APGD_FOOLED, APGD_REDUCED = 1, 2, 4  # bits of the flags row


def apgd_step_(x, x_old, g, x0, step, counter, eps):
    """The momentum step in place on x and x_old [B, ...]; step [B] float32, counter [1] int32 (0: the first iteration, a = 1)."""
    B = x.shape[0]
    px = _chk(x, torch.float32, "x")
    po = _chk(x_old, torch.float32, "x_old", x.shape)
    pg = _chk(g, torch.float32, "g", x.shape)
    p0 = _chk(x0, torch.float32, "x0", x.shape)
    ps = _chk(step, torch.float32, "step", (B,))
    pc = _chk(counter, torch.int32, "counter", (1,))
    N.check(N.lib.ee_apgd_step_f32(px, po, pg, p0, ps, pc, B, x.numel() // B if B else 0, eps, _stream()), "ee_apgd_step_f32")
    return x


# ---- `path` of the kernels that give a sample one workgroup (csrc/ee_sample.hpp) ---------------------------------------
SAMPLE_PATHS = {"auto": 0, "resident": 1, "streaming": 2}  # EE_PATH_*
SAMPLE_RESIDENT = 12288  # per-sample size up to which the resident path exists
APGD_L2_PATHS = APGD_L1_PATHS = SQATK_L2_PATHS = FAB_PATHS = SAMPLE_PATHS
APGD_L2_RESIDENT = APGD_L1_RESIDENT = SQATK_L2_RESIDENT = SAMPLE_RESIDENT


def _sample_path(path, what):
    """EE_PATH_* of `path`; `what` names the kernels in the error."""
    if path not in SAMPLE_PATHS:
        raise ValueError("%s path must be one of %s, got %r" % (what, sorted(SAMPLE_PATHS), path))
    return SAMPLE_PATHS[path]


def apgd_step_l2_(x, x_old, g, x0, step, counter, eps, norms=None, path="auto"):
    """The step of an L2 run (ee_apgd_l2.hip) in place on x and x_old [B, ...]; step [B] float32, counter [1] int32.  Returns norms [3, B]
    (||g||, ||z - x0|| after the gradient step, ||m - x0|| after the momentum mix), written into `norms` when given.  path: 'auto',
    'resident' (per-sample size <= 12288) or 'streaming'; the same bits."""
    B = x.shape[0]
    px = _chk(x, torch.float32, "x")
    po = _chk(x_old, torch.float32, "x_old", x.shape)
    pg = _chk(g, torch.float32, "g", x.shape)
    p0 = _chk(x0, torch.float32, "x0", x.shape)
    ps = _chk(step, torch.float32, "step", (B,))
    pc = _chk(counter, torch.int32, "counter", (1,))
    path = _sample_path(path, "the L2 step's")
    norms = torch.empty((3, B), dtype=torch.float32, device=x.device) if norms is None else norms
    pn = _chk(norms, torch.float32, "norms", (3, B))
    N.check(N.lib.ee_apgd_step_l2_f32(px, po, pg, p0, ps, pc, pn, B, x.numel() // B if B else 0, eps, path, _stream()),
            "ee_apgd_step_l2_f32")
    return norms


def apgd_loss(logits, labels, kind, targets=None):
    """(row losses [B] float32, dlogits [B,K] of their sum, pred [B] int32) for kind 'ce', 'dlr' or 'dlr_t' (which reads targets)."""
    B, K = logits.shape
    pz = _chk(logits, torch.float32, "logits")
    py = _chk(labels, torch.int64, "labels", (B,))
    if kind == "dlr_t" and targets is None:
        raise ValueError("the targeted DLR loss needs targets")
    pt = _chk(targets, torch.int64, "targets", (B,)) if kind == "dlr_t" else None
    loss = torch.empty(B, dtype=torch.float32, device=logits.device)
    d = torch.empty_like(logits)
    pred = torch.empty(B, dtype=torch.int32, device=logits.device)
    N.check(N.lib.ee_apgd_loss_f32(pz, py, pt, B, K, APGD_KINDS[kind], _chk(loss, torch.float32, "loss"), _chk(d, torch.float32, "d"),
                                   _chk(pred, torch.int32, "pred"), _stream()), "ee_apgd_loss_f32")
    return loss, d, pred


def apgd_book_(loss, pred, fstate, istate, counter, sched):
    """One iteration's per-sample bookkeeping in place on fstate [4,B] float32 / istate [4,B] int32 (its flags row is the result)."""
    B = loss.shape[0]
    N.check(N.lib.ee_apgd_book_f32(_chk(loss, torch.float32, "loss", (B,)), _chk(pred, torch.int32, "pred", (B,)),
                                   _chk(fstate, torch.float32, "fstate", (4, B)), _chk(istate, torch.int32, "istate", (4, B)),
                                   _chk(counter, torch.int32, "counter", (1,)), _chk(sched, torch.int32, "sched"), sched.numel(), B, _stream()),
            "ee_apgd_book_f32")
    return istate[APGD_I_FLAGS]


def apgd_select_(x, g, x_best, g_best, x_best_adv, flags, counter):
    """The copies the flags [B] ask for, in place, then counter += 1."""
    B = x.shape[0]
    px = _chk(x, torch.float32, "x")
    ptrs = [_chk(t, torch.float32, n, x.shape) for t, n in ((g, "g"), (x_best, "x_best"), (g_best, "g_best"), (x_best_adv, "x_best_adv"))]
    N.check(N.lib.ee_apgd_select_f32(px, *ptrs, _chk(flags, torch.int32, "flags", (B,)), _chk(counter, torch.int32, "counter", (1,)), B,
                                     x.numel() // B if B else 0, _stream()), "ee_apgd_select_f32")
    return x


def apgd_start_(x, x0, eps, metric, seed=0, noise=None, path="auto"):
    """The start point of an APGD restart, written into x [B, ...]: 'Linf' clamp(x0 + eps t, 0, 1) with t uniform
    on [-1, 1); 'L2' clamp(x0 + t * (eps / (||t||_2 + 1e-12)), 0, 1) with t standard normal (a row whose norm is not finite is x0); 'L1'
    x0 + t, unclamped - the run's own projection follows.  t is the row of `noise` [B, ...] or, with noise None, the draw of
    csrc/ee_apgd_start.hip keyed by `seed` (eeadv.fabstart.draw with stream STREAM_APGD_START restates it)."""
    B = x.shape[0]
    if metric not in FAB_METRICS:
        raise ValueError("APGD metric must be one of %s, got %r" % (sorted(FAB_METRICS), metric))
    px = _chk(x, torch.float32, "x")
    p0 = _chk(x0, torch.float32, "x0", x.shape)
    if B and x.data_ptr() == x0.data_ptr():
        raise ValueError("apgd_start_ writes x while it reads x0: they must be two tensors")
    N.check(N.lib.ee_apgd_start_f32(px, p0, _opt(noise, torch.float32, "noise", x.shape), B, x.numel() // B if B else 1, eps,
                                    FAB_METRICS[metric], int(seed) & 0xFFFFFFFFFFFFFFFF, _sample_path(path, "the APGD start's"), _stream()),
            "ee_apgd_start_f32")
    return x


def apgd_merge_(adv_all, robust_all, loss_all, x_best_adv, robust_run, loss_best_run, first):
    """The union across restarts, in place on adv_all [B, ...] float32, robust_all [B] int32 and loss_all [B]
    float32, from the finished run's x_best_adv, robust row [B] int32 and best losses [B]: a sample this run fooled and no earlier one had
    takes this run's point and loses its flag, loss_all keeps the larger loss; `first` (restart 0) overwrites flags and losses instead."""
    B = adv_all.shape[0]
    pa = _chk(adv_all, torch.float32, "adv_all")
    pb = _chk(x_best_adv, torch.float32, "x_best_adv", adv_all.shape)
    if B and adv_all.data_ptr() == x_best_adv.data_ptr():
        raise ValueError("apgd_merge_ writes adv_all while it reads x_best_adv: they must be two tensors")
    N.check(N.lib.ee_apgd_merge_f32(pa, _chk(robust_all, torch.int32, "robust_all", (B,)), _chk(loss_all, torch.float32, "loss_all", (B,)), pb,
                                    _chk(robust_run, torch.int32, "robust_run", (B,)), _chk(loss_best_run, torch.float32, "loss_best_run", (B,)),
                                    B, adv_all.numel() // B if B else 1, 1 if first else 0, _stream()), "ee_apgd_merge_f32")
    return adv_all


# ---- the perturbation check of an evaluation (ee_pert.hip) ---------------------------------------
def _pert_check_host(x_adv, x0):
    """ee_pert_check_f32 restated in numpy float64 for [B, ...] arrays or CPU tensors: (norms [B, 3] float32, range [B, 2] float32,
    n_nan [B] int32).  d = x_adv - x0 is formed in float32, as the kernel forms it; the sums are numpy's float64 ones (pairwise: not the
    kernel's order, the same value to within the last bit of the float32 result).  A NaN in d makes the row's three norms NaN; NaN
    entries of x_adv are skipped by the range, (+inf, -inf) for a row of NaN entries only."""
    a = np.ascontiguousarray(x_adv.detach().cpu().numpy() if isinstance(x_adv, torch.Tensor) else x_adv, dtype=np.float32)
    o = np.ascontiguousarray(x0.detach().cpu().numpy() if isinstance(x0, torch.Tensor) else x0, dtype=np.float32)
    if a.shape != o.shape:
        raise ValueError("x0 has shape %s, expected %s" % (o.shape, a.shape))
    B = a.shape[0]
    a, o = a.reshape(B, -1), o.reshape(B, -1)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs((a - o).astype(np.float32)).astype(np.float64)
        bad = np.isnan(d).any(axis=1)
        norms = np.stack([d.max(axis=1, initial=0.0), np.sqrt((d * d).sum(axis=1)), d.sum(axis=1)], axis=1).astype(np.float32)
    norms[bad] = np.nan
    nan = np.isnan(a)
    rng = np.stack([np.where(nan, np.inf, a).min(axis=1, initial=np.inf), np.where(nan, -np.inf, a).max(axis=1, initial=-np.inf)],
                   axis=1).astype(np.float32)
    return norms, rng, nan.sum(axis=1).astype(np.int32)


def pert_check(x_adv, x0, path="auto"):
    """(norms [B, 3], range [B, 2], n_nan [B]) of the points x_adv [B, ...] around the clean samples x0: per sample
    the Linf, L2 and L1 norm of x_adv - x0 (all NaN if the difference holds a NaN), the minimum and maximum of x_adv over its entries that
    are no NaN, and the number of those that are.  Device tensors: one launch of ee_pert_check_f32, float32 / float32 / int32 tensors, no
    host read; path: 'auto', 'resident' (per-sample size <= 12288) or 'streaming', the same bits.  CPU tensors are refused, as everywhere,
    unless the caller opted into the host plumbing (eeadv.runtime.allow_cpu_plumbing, what --no-cuda does): then _pert_check_host, the same
    three as tensors."""
    from . import runtime
    if tuple(x_adv.shape) != tuple(x0.shape):
        raise ValueError("x0 has shape %s, expected %s" % (tuple(x0.shape), tuple(x_adv.shape)))
    if not x_adv.is_cuda and not x0.is_cuda and not runtime.require_device(x_adv, "pert_check"):
        _sample_path(path, "the perturbation check's")
        return tuple(torch.from_numpy(v) for v in _pert_check_host(x_adv, x0))
    B = x_adv.shape[0]
    pa = _chk(x_adv, torch.float32, "x_adv")
    p0 = _chk(x0, torch.float32, "x0", x_adv.shape)
    norms = torch.empty((B, 3), dtype=torch.float32, device=x_adv.device)
    rng = torch.empty((B, 2), dtype=torch.float32, device=x_adv.device)
    n_nan = torch.empty(B, dtype=torch.int32, device=x_adv.device)
    N.check(N.lib.ee_pert_check_f32(pa, p0, B, x_adv.numel() // B if B else 1, _chk(norms, torch.float32, "norms"), _chk(rng, torch.float32, "range"),
                                    _chk(n_nan, torch.int32, "n_nan"), _sample_path(path, "the perturbation check's"), _stream()),
            "ee_pert_check_f32")
    return norms, rng, n_nan


# ---- APGD in the L1 threat model (ee_apgd_l1.hip) --------------------------------------------------------------------
L1_S_LAMBDA, L1_S_H0, L1_S_ACTIVE, L1_S_DIST, L1_S_TAU, L1_S_M, L1_S_J = range(7)  # rows of scal
L1_SCAL_ROWS = 7


def _l1_scal(scal, x):
    B = x.shape[0]
    scal = torch.zeros((L1_SCAL_ROWS, B), dtype=torch.float32, device=x.device) if scal is None else scal
    return scal, _chk(scal, torch.float32, "scal", (L1_SCAL_ROWS, B))


def l1_proj(u, x0, eps, out=None, scal=None, path="auto"):
    """P(u): the Euclidean projection of u [B, ...] onto the L1 ball of radius eps around x0 intersected with [0,1]^D, per sample.
    Returns (z, scal): z is `out` when given (it may be u itself), scal [7, B] has rows L1_S_LAMBDA, _H0, _ACTIVE, _DIST written."""
    B = u.shape[0]
    out = torch.empty_like(u) if out is None else out
    pu = _chk(u, torch.float32, "u")
    pz = _chk(out, torch.float32, "out", u.shape)
    p0 = _chk(x0, torch.float32, "x0", u.shape)
    scal, ps = _l1_scal(scal, u)
    path = _sample_path(path, "the L1 kernels'")
    N.check(N.lib.ee_l1_proj_f32(pz, pu, p0, ps, B, u.numel() // B if B else 0, eps, path, _stream()), "ee_l1_proj_f32")
    return out, scal


def apgd_step_l1_(x, g, x0, step, topk, eps, scal=None, path="auto"):
    """The step of an L1 run in place on x [B, ...]: selection, sparse sign step, projection; step, topk [B] float32.  Returns scal
    [7, B] (rows L1_S_*), written into `scal` when given.  path: 'auto', 'resident' (per-sample size <= 12288) or 'streaming'."""
    B = x.shape[0]
    px = _chk(x, torch.float32, "x")
    pg = _chk(g, torch.float32, "g", x.shape)
    p0 = _chk(x0, torch.float32, "x0", x.shape)
    pst = _chk(step, torch.float32, "step", (B,))
    pt = _chk(topk, torch.float32, "topk", (B,))
    scal, ps = _l1_scal(scal, x)
    path = _sample_path(path, "the L1 kernels'")
    N.check(N.lib.ee_apgd_step_l1_f32(px, pg, p0, pst, pt, ps, B, x.numel() // B if B else 0, eps, path, _stream()),
            "ee_apgd_step_l1_f32")
    return scal


def apgd_book_l1_(loss, pred, x, x_best, x0, fstate, istate, topk, spstate, counter, sched, eps):
    """One iteration's bookkeeping of an L1 run in place on fstate [4,B] / istate [4,B] (the APGD run's), topk [B] float32 and spstate
    [2,B] int32 (sp_old, the last count); the flags row of istate is the result."""
    B = loss.shape[0]
    px = _chk(x, torch.float32, "x")
    N.check(N.lib.ee_apgd_book_l1_f32(_chk(loss, torch.float32, "loss", (B,)), _chk(pred, torch.int32, "pred", (B,)), px,
                                      _chk(x_best, torch.float32, "x_best", x.shape), _chk(x0, torch.float32, "x0", x.shape),
                                      _chk(fstate, torch.float32, "fstate", (4, B)), _chk(istate, torch.int32, "istate", (4, B)),
                                      _chk(topk, torch.float32, "topk", (B,)), _chk(spstate, torch.int32, "spstate", (2, B)),
                                      _chk(counter, torch.int32, "counter", (1,)), _chk(sched, torch.int32, "sched"), sched.numel(), B,
                                      x.numel() // B if B else 0, eps, _stream()), "ee_apgd_book_l1_f32")
    return istate[APGD_I_FLAGS]


# ---- EOT for APGD (ee_eot.hip) ---------------------------------------------------------------------------------------
def apgd_eot_acc_(g_acc, g, loss_acc, loss, loss_mean, k, E):
    """Draw k of E in place: g_acc [B, ...] takes g (k == 0) or g_acc + g, and * (1/E) after the last draw; loss_acc [B] float64 takes the
    row losses [B] the same way, and loss_mean [B] = loss_acc / E after the last draw."""
    B = g_acc.shape[0]
    pa = _chk(g_acc, torch.float32, "g_acc")
    pg = _chk(g, torch.float32, "g", g_acc.shape)
    N.check(N.lib.ee_apgd_eot_acc_f32(pa, pg, _chk(loss_acc, torch.float64, "loss_acc", (B,)), _chk(loss, torch.float32, "loss", (B,)),
                                      _chk(loss_mean, torch.float32, "loss_mean", (B,)), int(k), int(E), B, g_acc.numel() // B if B else 0,
                                      _stream()), "ee_apgd_eot_acc_f32")
    return g_acc


# ---- Square attack (ee_sqatk.hip) ------------------------------------------------------------------------------------
def _sqatk_images(x_best, x_new, x0):
    if x_best.dim() != 4:
        raise ValueError("the Square attack takes image batches [B,C,H,W], got shape %s" % (tuple(x_best.shape),))
    return (_chk(x_best, torch.float32, "x_best"), _chk(x_new, torch.float32, "x_new", x_best.shape), _chk(x0, torch.float32, "x0", x_best.shape))


def sqatk_init_(x_best, x_new, x0, seed, eps):
    """The striped start into x_best and x_new [B,C,H,W]; seed int64 [1] on the device."""
    B, C, H, W = x_best.shape
    pb, pn, p0 = _sqatk_images(x_best, x_new, x0)
    N.check(N.lib.ee_sqatk_init_f32(pb, pn, p0, _chk(seed, torch.int64, "seed", (1,)), B, C, H, W, eps, _stream()), "ee_sqatk_init_f32")
    return x_best


def sqatk_margin_(logits, labels, margin_out, margin_min, queries, flags, counter):
    """margin_out <- z_y - max_{j != y} z_j of logits [B,K]; margin_min, queries [B] updated in place, flags [B] <- accept; counter += 1."""
    B, K = logits.shape
    N.check(N.lib.ee_sqatk_margin_f32(_chk(logits, torch.float32, "logits"), _chk(labels, torch.int64, "labels", (B,)), B, K,
                                      _chk(margin_out, torch.float32, "margin_out", (B,)), _chk(margin_min, torch.float32, "margin_min", (B,)),
                                      _chk(queries, torch.int32, "queries", (B,)), _chk(flags, torch.int32, "flags", (B,)),
                                      _chk(counter, torch.int32, "counter", (1,)), _stream()), "ee_sqatk_margin_f32")
    return flags


def sqatk_step_(x_best, x_new, x0, flags, margin_min, counter, sizes, seed, eps):
    """Commit under flags [B], then proposal counter[0] with the window edge sizes[counter[0]] (sizes None or empty: commit only)."""
    B, C, H, W = x_best.shape
    pb, pn, p0 = _sqatk_images(x_best, x_new, x0)
    n_sizes = 0 if sizes is None else int(sizes.numel())
    ps = _chk(sizes, torch.int32, "sizes", (n_sizes,)) if n_sizes else None
    N.check(N.lib.ee_sqatk_step_f32(pb, pn, p0, _chk(flags, torch.int32, "flags", (B,)), _chk(margin_min, torch.float32, "margin_min", (B,)),
                                    _chk(counter, torch.int32, "counter", (1,)), ps, n_sizes, _chk(seed, torch.int64, "seed", (1,)), B, C, H, W,
                                    eps, _stream()), "ee_sqatk_step_f32")
    return x_new


# ---- Square attack in the L2 and L1 threat models (ee_sqatk_l2.hip, ee_sqatk_l1.hip) ----------------------------------
SQATK_L1_SCAL_ROWS = 4  # rows L1_S_LAMBDA .. L1_S_DIST of the launch's projection


def _sqatk_eta0(eta0):
    """The side s0 of the start's table."""
    if eta0.dim() != 2 or eta0.shape[0] != eta0.shape[1]:
        raise ValueError("eta0 must be a square table [s0, s0], got shape %s" % (tuple(eta0.shape),))
    return int(eta0.shape[0])


def _sqatk_tables(sizes, eta_off, eta):
    """(sizes, eta_off, eta, n_sizes) as a step launch takes them: sizes None or empty is a commit-only launch, which reads none of them."""
    n_sizes = 0 if sizes is None else int(sizes.numel())
    if not n_sizes:
        return None, None, None, 0
    return _chk(sizes, torch.int32, "sizes", (n_sizes,)), _chk(eta_off, torch.int32, "eta_off", (n_sizes,)), _chk(eta, torch.float32, "eta"), n_sizes


def _sqatk_l1_scal(scal, x_best):
    B = x_best.shape[0]
    scal = torch.zeros((SQATK_L1_SCAL_ROWS, B), dtype=torch.float32, device=x_best.device) if scal is None else scal
    return scal, _chk(scal, torch.float32, "scal", (SQATK_L1_SCAL_ROWS, B))


def sqatk_init_l2_(x_best, x_new, x0, seed, eta0, eps, path="auto"):
    """The tiled start of an L2 run into x_best and x_new [B,C,H,W]; eta0 float32 [s0, s0] on the device (eeadv.sqatk.eta), seed int64 [1]."""
    B, C, H, W = x_best.shape
    pb, pn, p0 = _sqatk_images(x_best, x_new, x0)
    s0 = _sqatk_eta0(eta0)
    path = _sample_path(path, "the L2 Square kernels'")
    N.check(N.lib.ee_sqatk_init_l2_f32(pb, pn, p0, _chk(seed, torch.int64, "seed", (1,)), _chk(eta0, torch.float32, "eta0"), s0,
                                       B, C, H, W, eps, path, _stream()), "ee_sqatk_init_l2_f32")
    return x_best


def sqatk_step_l2_(x_best, x_new, x0, flags, margin_min, counter, sizes, eta_off, eta, seed, eps, norms=None, path="auto"):
    """Commit under flags [B], then L2 proposal counter[0]: window edge sizes[counter[0]], pattern table eta[eta_off[counter[0]]:] (sizes
    None or empty: commit only; eta_off and eta are then not read).  Returns norms [3 + 2C, B] (n_img, n_un, n_d, n_w[c], n_new[c]; zeros
    for a sample that made no proposal), written into `norms` when given.  path: 'auto', 'resident' (C*H*W <= 12288) or 'streaming'; the
    same bits."""
    B, C, H, W = x_best.shape
    pb, pn, p0 = _sqatk_images(x_best, x_new, x0)
    ps, po, pe, n_sizes = _sqatk_tables(sizes, eta_off, eta)
    norms = torch.zeros((3 + 2 * C, B), dtype=torch.float32, device=x_best.device) if norms is None else norms
    path = _sample_path(path, "the L2 Square kernels'")
    N.check(N.lib.ee_sqatk_step_l2_f32(pb, pn, p0, _chk(flags, torch.int32, "flags", (B,)), _chk(margin_min, torch.float32, "margin_min", (B,)),
                                       _chk(counter, torch.int32, "counter", (1,)), ps, po, pe, n_sizes, _chk(seed, torch.int64, "seed", (1,)),
                                       _chk(norms, torch.float32, "norms", (3 + 2 * C, B)), B, C, H, W, eps, path, _stream()),
            "ee_sqatk_step_l2_f32")
    return norms


def sqatk_init_l1_(x_best, x_new, x0, seed, eta0, eps, eps_p, scal=None, path="auto"):
    """The start of an L1 run into x_best and x_new [B,C,H,W]: P_{eps_p}(x0 + d), d the tiled pattern of the L2 start; eta0 float32
    [s0, s0] on the device (eeadv.sqatk.eta), seed int64 [1].  Returns scal [4, B] (rows L1_S_LAMBDA .. _DIST), written into `scal` when
    given."""
    B, C, H, W = x_best.shape
    pb, pn, p0 = _sqatk_images(x_best, x_new, x0)
    s0 = _sqatk_eta0(eta0)
    scal, ps = _sqatk_l1_scal(scal, x_best)
    path = _sample_path(path, "the L1 Square kernels'")
    N.check(N.lib.ee_sqatk_init_l1_f32(pb, pn, p0, _chk(seed, torch.int64, "seed", (1,)), _chk(eta0, torch.float32, "eta0"), s0,
                                       ps, B, C, H, W, eps, eps_p, path, _stream()), "ee_sqatk_init_l1_f32")
    return scal


def sqatk_step_l1_(x_best, x_new, x0, flags, margin_min, counter, sizes, eta_off, eta, seed, eps, eps_p, norms=None, scal=None, path="auto"):
    """Commit under flags [B], then L1 proposal counter[0] and its projection onto the eps_p ball and the box, in one launch: window edge
    sizes[counter[0]], pattern table eta[eta_off[counter[0]]:] (sizes None or empty: commit only; eta_off and eta are then not read).
    Returns (norms [2 + 2C, B]: n_img, n_un, n_w[c], n_new[c]; scal [4, B]: rows L1_S_LAMBDA .. _DIST) - zeros for a sample that made no
    proposal - written into `norms` / `scal` when given.  path: 'auto', 'resident' (C*H*W <= 12288) or 'streaming'; the same bits."""
    B, C, H, W = x_best.shape
    pb, pn, p0 = _sqatk_images(x_best, x_new, x0)
    ps, po, pe, n_sizes = _sqatk_tables(sizes, eta_off, eta)
    norms = torch.zeros((2 + 2 * C, B), dtype=torch.float32, device=x_best.device) if norms is None else norms
    scal, pscal = _sqatk_l1_scal(scal, x_best)
    path = _sample_path(path, "the L1 Square kernels'")
    N.check(N.lib.ee_sqatk_step_l1_f32(pb, pn, p0, _chk(flags, torch.int32, "flags", (B,)), _chk(margin_min, torch.float32, "margin_min", (B,)),
                                       _chk(counter, torch.int32, "counter", (1,)), ps, po, pe, n_sizes, _chk(seed, torch.int64, "seed", (1,)),
                                       _chk(norms, torch.float32, "norms", (2 + 2 * C, B)), pscal, B, C, H, W, eps, eps_p, path, _stream()),
            "ee_sqatk_step_l1_f32")
    return norms, scal


# ---- FAB-T (ee_fab.hip) ----------------------------------------------------------------------------------------------
FAB_ADV, FAB_IMPROVED = 1, 2  # bits of the flags of fab_commit_ (EE_FAB_*)
FAB_LAMBDA, FAB_SIGN, FAB_NORM = range(3)  # rows of the projection scalars [3, 2B] (row 0 is mu in L2)
FAB_THETA, FAB_PHI, FAB_L1_ROWS = 0, 3, 4  # L1: the scalars are [4, 2B], row 0 is theta and row 3 the fraction phi taken at theta


def fab_diff(logits, labels, targets):
    """(df [B] = z_t - z_y, dlogits [B,K] of its batch sum, pred [B] int32: the first class in the order of topk)."""
    B, K = logits.shape
    df = torch.empty(B, dtype=torch.float32, device=logits.device)
    d = torch.empty_like(logits)
    pred = torch.empty(B, dtype=torch.int32, device=logits.device)
    N.check(N.lib.ee_fab_diff_f32(_chk(logits, torch.float32, "logits"), _chk(labels, torch.int64, "labels", (B,)),
                                  _chk(targets, torch.int64, "targets", (B,)), B, K, _chk(df, torch.float32, "df"), _chk(d, torch.float32, "d"),
                                  _chk(pred, torch.int32, "pred"), _stream()), "ee_fab_diff_f32")
    return df, d, pred


FAB_METRICS = {"Linf": 0, "L2": 1, "L1": 2}  # EE_FAB_METRIC_*: the threat model; fab_select measures in its dual norm


def fab_select(g, logits, labels, k, metric, best, best_k, w, df, first=None):
    """One class of untargeted FAB's running arg-min, in place on best [B] float32, best_k [B] int32, w [B, ...] and df [B]: where class k's
    linearised boundary (gradient g [B, ...], logits [B, K]) is strictly closer in the dual norm of `metric` ('Linf', 'L2', 'L1') than
    best, the sample takes (dist, k, z_k - z_y, g[b]).  first (default: k == 0) stands in for the reset of best / best_k / df."""
    B, K = logits.shape
    if metric not in FAB_METRICS:
        raise ValueError("FAB metric must be one of %s, got %r" % (sorted(FAB_METRICS), metric))
    if not 0 <= int(k) < K:
        raise ValueError("class %r outside [0, %d)" % (k, K))
    pg = _chk(g, torch.float32, "g")
    if g.shape[0] != B:
        raise ValueError("g has %d rows, logits %d" % (g.shape[0], B))
    N.check(N.lib.ee_fab_select_f32(pg, _chk(logits, torch.float32, "logits"), _chk(labels, torch.int64, "labels", (B,)), int(k),
                                    FAB_METRICS[metric], int(k == 0 if first is None else first), B, K, g.numel() // B if B else 1,
                                    _chk(best, torch.float32, "best", (B,)), _chk(best_k, torch.int32, "best_k", (B,)),
                                    _chk(w, torch.float32, "w", g.shape), _chk(df, torch.float32, "df", (B,)), _stream()), "ee_fab_select_f32")
    return best_k


def fab_start_(x, x0, res, eps, metric, seed=0, noise=None, path="auto"):
    """The random start of a FAB restart, written into x [B, ...]: x = clamp(x0 + ((m t) / n) / 2, 0, 1) with
    m = min(res[b], eps), t the row of `noise` [B, ...] - or, with noise None, the draw of csrc/ee_fab.hip keyed by `seed` (eeadv.fabstart.draw
    restates it) - and n its norm in `metric` ('Linf', 'L2', 'L1').  res [B] is read on the device; a row whose n is 0 or not finite is x0."""
    B = x.shape[0]
    if metric not in FAB_METRICS:
        raise ValueError("FAB metric must be one of %s, got %r" % (sorted(FAB_METRICS), metric))
    px = _chk(x, torch.float32, "x")
    p0 = _chk(x0, torch.float32, "x0", x.shape)
    if B and x.data_ptr() == x0.data_ptr():
        raise ValueError("fab_start_ writes x while it reads x0: they must be two tensors")
    N.check(N.lib.ee_fab_start_f32(px, p0, _chk(res, torch.float32, "res", (B,)), _opt(noise, torch.float32, "noise", x.shape), B,
                                   x.numel() // B if B else 1, eps, FAB_METRICS[metric], int(seed) & 0xFFFFFFFFFFFFFFFF,
                                   _sample_path(path, "the FAB start's"), _stream()), "ee_fab_start_f32")
    return x


def _fab_proj(fn, name, x, x0, w, df, path, out, rows=3):
    B = x.shape[0]
    px = _chk(x, torch.float32, "x")
    p0 = _chk(x0, torch.float32, "x0", x.shape)
    pw = _chk(w, torch.float32, "w", x.shape)
    pd = _chk(df, torch.float32, "df", (B,))
    out = torch.empty((rows, 2 * B), dtype=torch.float32, device=x.device) if out is None else out
    po = _chk(out, torch.float32, "out", (rows, 2 * B))
    if B:
        N.check(fn(px, p0, pw, pd, B, x.numel() // B, _sample_path(path, "FAB projection"), po, _stream()), name)
    return out


def fab_proj_linf(x, x0, w, df, path="auto", out=None):
    """The scalars [3, 2B] (rows lambda, sign, ||delta||_inf) of the two projections of every sample: column b projects x[b] with c = df[b],
    column B + b projects x0[b] with c = df[b] + <w[b], x0[b] - x[b]>.  path: 'auto', 'resident' (per-sample size <= 12288) or 'streaming'."""
    return _fab_proj(N.lib.ee_fab_proj_linf_f32, "ee_fab_proj_linf_f32", x, x0, w, df, path, out)


def fab_proj_l2(x, x0, w, df, path="auto", out=None):
    """fab_proj_linf for the least-L2 projections: rows mu, sign, ||delta||_2 (delta_i = -sign(s w_i) min(mu |w_i|, r_i))."""
    return _fab_proj(N.lib.ee_fab_proj_l2_f32, "ee_fab_proj_l2_f32", x, x0, w, df, path, out)


def _fab_step(fn, name, x, x0, w, scal, rows=3):
    B = x.shape[0]
    px = _chk(x, torch.float32, "x")
    N.check(fn(px, _chk(x0, torch.float32, "x0", x.shape), _chk(w, torch.float32, "w", x.shape),
               _chk(scal, torch.float32, "scal", (rows, 2 * B)), B, x.numel() // B if B else 0, _stream()), name)
    return x


def fab_proj_l1(x, x0, w, df, path="auto", out=None):
    """fab_proj_linf for the least-L1 projections: the scalars [4, 2B], rows theta, sign, ||delta||_1, phi (delta_i = -sign(s w_i) m_i,
    m_i = r_i where |w_i| > theta, phi r_i where |w_i| == theta, 0 below)."""
    return _fab_proj(N.lib.ee_fab_proj_l1_f32, "ee_fab_proj_l1_f32", x, x0, w, df, path, out, FAB_L1_ROWS)


def fab_step_(x, x0, w, scal):
    """The FAB step in place on x [B, ...] from the projection scalars [3, 2B]."""
    return _fab_step(N.lib.ee_fab_step_f32, "ee_fab_step_f32", x, x0, w, scal)


def fab_step_l2_(x, x0, w, scal):
    """The FAB step in place on x [B, ...] from the scalars [3, 2B] of fab_proj_l2."""
    return _fab_step(N.lib.ee_fab_step_l2_f32, "ee_fab_step_l2_f32", x, x0, w, scal)


def fab_step_l1_(x, x0, w, scal):
    """The FAB step in place on x [B, ...] from the scalars [4, 2B] of fab_proj_l1."""
    return _fab_step(N.lib.ee_fab_step_l1_f32, "ee_fab_step_l1_f32", x, x0, w, scal, FAB_L1_ROWS)


def _fab_commit(fn, name, logits, labels, x, x0, adv, res, pred, flags, counter):
    B, K = logits.shape
    N.check(fn(_chk(logits, torch.float32, "logits", (x.shape[0], K)), _chk(labels, torch.int64, "labels", (B,)), B, K,
               _chk(x, torch.float32, "x"), _chk(x0, torch.float32, "x0", x.shape), _chk(adv, torch.float32, "adv", x.shape),
               _chk(res, torch.float32, "res", (B,)), _chk(pred, torch.int32, "pred", (B,)),
               _chk(flags, torch.int32, "flags", (B,)), _chk(counter, torch.int32, "counter", (1,)),
               x.numel() // B if B else 0, _stream()), name)
    return flags


def fab_commit_(logits, labels, x, x0, adv, res, pred, flags, counter):
    """The check after the second forward, in place on x, adv [B, ...], res [B]; pred, flags [B] int32 are written; counter += 1."""
    return _fab_commit(N.lib.ee_fab_commit_f32, "ee_fab_commit_f32", logits, labels, x, x0, adv, res, pred, flags, counter)


def fab_commit_l2_(logits, labels, x, x0, adv, res, pred, flags, counter):
    """fab_commit_ with res [B] holding L2 distances."""
    return _fab_commit(N.lib.ee_fab_commit_l2_f32, "ee_fab_commit_l2_f32", logits, labels, x, x0, adv, res, pred, flags, counter)


def fab_commit_l1_(logits, labels, x, x0, adv, res, pred, flags, counter):
    """fab_commit_ with res [B] holding L1 distances."""
    return _fab_commit(N.lib.ee_fab_commit_l1_f32, "ee_fab_commit_l1_f32", logits, labels, x, x0, adv, res, pred, flags, counter)


# ---- sample pools of the attack cascade (ee_cascade.hip) -------------------------------------------------------------
def _u8(t, name, shape):
    """A bool or uint8 flag vector as the uint8 pointer the kernels read (the same bytes: a view, no copy)."""
    if isinstance(t, torch.Tensor) and t.dtype == torch.bool:
        t = t.view(torch.uint8)
    return _chk(t, torch.uint8, name, shape)


def _pool_ptrs(pool_x, pool_y, pool_id, pool_order, count):
    cap, D = pool_x.shape
    K = pool_order.shape[1]
    ptrs = (_chk(pool_x, torch.float32, "pool_x"), _chk(pool_y, torch.int64, "pool_y", (cap,)), _chk(pool_id, torch.int64, "pool_id", (cap,)),
            _chk(pool_order, torch.int64, "pool_order", (cap, K)), _chk(count, torch.int32, "count", (1,)))
    return ptrs, cap, D, K


def pool_append_(x, y, ids, order, keep, pool_x, pool_y, pool_id, pool_order, count):
    """The rows of the batch (x [B,D] f32, y, ids [B] i64, order [B,K] i64) with keep [B] (bool / uint8) set go behind the count [1] int32
    rows already in the pool (pool_x [cap,D], pool_y, pool_id [cap], pool_order [cap,K]), in source order; then count += kept.  The caller
    keeps count + kept <= cap."""
    ptrs, cap, D, K = _pool_ptrs(pool_x, pool_y, pool_id, pool_order, count)
    B = x.shape[0]
    N.check(N.lib.ee_pool_append_f32(_chk(x, torch.float32, "x", (B, D)), _chk(y, torch.int64, "y", (B,)), _chk(ids, torch.int64, "ids", (B,)),
                                     _chk(order, torch.int64, "order", (B, K)), _u8(keep, "keep", (B,)), B, D, K, *ptrs, cap, _stream()),
            "ee_pool_append_f32")
    return count


def pool_pop_(pool_x, pool_y, pool_id, pool_order, count, x, y, ids, order):
    """The first B pool rows into the batch buffers (x [B,D], y, ids [B], order [B,K]; a pool with fewer than B rows pads with its row 0), the
    remaining rows to the front, count = max(count - B, 0).  The caller pops at count < 2 B <= cap."""
    ptrs, cap, D, K = _pool_ptrs(pool_x, pool_y, pool_id, pool_order, count)
    B = x.shape[0]
    N.check(N.lib.ee_pool_pop_f32(*ptrs, cap, B, D, K, _chk(x, torch.float32, "x", (B, D)), _chk(y, torch.int64, "y", (B,)),
                                  _chk(ids, torch.int64, "ids", (B,)), _chk(order, torch.int64, "order", (B, K)), _stream()), "ee_pool_pop_f32")
    return x


def cascade_resolve_(robust, ids, x_adv, n_valid, stage, robust_out, stage_out, adv_out, keep):
    """Rows b < n_valid of a stage's batch: keep[b] = robust[b]; a broken one writes robust_out[ids[b]] = 0, stage_out[ids[b]] = stage and
    - adv_out [N,D] given - adv_out[ids[b]] = x_adv[b].  Every other row: keep[b] = 0.  robust, keep [B] and robust_out [N] are bool / uint8,
    stage_out [N] int32."""
    B = robust.shape[0]
    n = robust_out.shape[0]
    D = x_adv.numel() // B
    N.check(N.lib.ee_cascade_resolve_f32(_u8(robust, "robust", (B,)), _chk(ids, torch.int64, "ids", (B,)), _chk(x_adv, torch.float32, "x_adv"), B,
                                         int(n_valid), D, int(stage), n, _u8(robust_out, "robust_out", (n,)),
                                         _chk(stage_out, torch.int32, "stage_out", (n,)), _opt(adv_out, torch.float32, "adv_out", (n, D)),
                                         _u8(keep, "keep", (B,)), _stream()), "ee_cascade_resolve_f32")
    return keep


# ---- Add_Square ------------------------------------------------------------------------------------------------------
def _square_ptrs(sq_mode, x, sq_x, stripe, sq_sign, sq_pos, sq_size):
    """The Add_Square arguments of a native call, checked against x [B,C,H,W]: (stripe, sq_sign, sq_pos, sq_size, sq_x, nq).
    All empty at sq_mode 0; sq_x only at sq_mode 2."""
    if not sq_mode:
        return None, None, None, None, None, 0
    B, C, H, W = x.shape
    nq = int(sq_size.numel())
    ps = _chk(stripe, torch.float32, "stripe", (B, C, 1, W))
    pg = _chk(sq_sign, torch.float32, "sq_sign", (nq, C))
    pp = _chk(sq_pos, torch.int64, "sq_pos", (nq,))
    pz = _chk(sq_size, torch.int32, "sq_size", (nq,))
    pxo = _chk(sq_x, torch.float32, "sq_x", x.shape) if sq_mode == 2 else None
    return ps, pg, pp, pz, pxo, nq


def add_square_fwd(x, eps, stripe, sq_sign, sq_pos, sq_size):
    B, C, H, W = x.shape
    out = torch.empty_like(x)
    px = _chk(x, torch.float32, "x")
    ps, pg, pp, pz, _, nq = _square_ptrs(1, x, None, stripe, sq_sign, sq_pos, sq_size)
    N.check(N.lib.ee_add_square_fwd_f32(px, B, C, H, W, eps, ps, pg, pp, pz, nq, _chk(out, torch.float32, "out"), _stream()),
            "ee_add_square_fwd_f32")
    return out


def add_square_bwd(g_out, x, eps, stripe, sq_sign, sq_pos, sq_size):
    B, C, H, W = x.shape
    g_x = torch.empty_like(x)
    pgo, px = _chk(g_out, torch.float32, "g_out", x.shape), _chk(x, torch.float32, "x")
    ps, pg, pp, pz, _, nq = _square_ptrs(1, x, None, stripe, sq_sign, sq_pos, sq_size)
    N.check(N.lib.ee_add_square_bwd_f32(pgo, px, B, C, H, W, eps, ps, pg, pp, pz, nq, _chk(g_x, torch.float32, "g_x"), _stream()),
            "ee_add_square_bwd_f32")
    return g_x


# ---- HighFreqSuppress -----------------------------------------------------------------------------------------------
def square_draw(batch, C, h, sq_size, state):
    """The random draws of one Add_Square forward in one launch (core.py:637, :645, :648): returns stripe [B,C,1,h] fp32,
    sq_pos [nq] int64, sq_sign [nq,C] fp32.  state: int64[2] device tensor {seed, offset}, advanced by the kernel."""
    dev = sq_size.device
    nq = int(sq_size.numel())
    stripe = torch.empty((batch, C, 1, h), dtype=torch.float32, device=dev)
    sq_pos = torch.empty((nq,), dtype=torch.int64, device=dev)
    sq_sign = torch.empty((nq, C), dtype=torch.float32, device=dev)
    N.check(N.lib.ee_square_draw_f32(stripe.data_ptr(), stripe.numel(), sq_pos.data_ptr(), sq_sign.data_ptr(),
                                     _chk(sq_size, torch.int32, "sq_size"), nq, C, h, _chk(state, torch.int64, "state", (4,)), _stream()),
            "ee_square_draw_f32")
    return stripe, sq_pos, sq_sign


def _hfs(entry, need, lead, x, tables, sq_mode, sq_x, eps, stripe, sq_sign, sq_pos, sq_size):
    """The shared body of the three low-pass wrappers: `entry` is the native function, `need` its table-size query's answer for
    x's plane, `lead` the arguments between the table and sq_mode."""
    B, C, H, W = x.shape
    px = _chk(x, torch.float32, "x")
    pt = _chk(tables, torch.float32, "tables", (need,))
    out = torch.empty_like(x)
    ps, pg, pp, pz, pxo, nq = _square_ptrs(sq_mode, x, sq_x, stripe, sq_sign, sq_pos, sq_size)
    N.check(getattr(N.lib, entry)(px, _chk(out, torch.float32, "out"), B, C, H, W, pt, *lead, sq_mode, pxo, eps, ps, pg, pp, pz, nq, _stream()),
            entry)
    return out


def hfs(x, tables, NU, NV, sq_mode=0, sq_x=None, eps=0.0, stripe=None, sq_sign=None, sq_pos=None, sq_size=None):
    """y = F(x) (sq_mode 0), F(add_square(x)) (1) or F(x) * d add_square/dx at sq_x (2); F = the low-pass operator."""
    H, W = x.shape[2:]
    return _hfs("ee_hfs_f32", N.lib.ee_hfs_table_floats(H, W, NU, NV), (NU, NV, 1.0 / H), x, tables, sq_mode, sq_x, eps, stripe, sq_sign,
                sq_pos, sq_size)


def hfs_mfma(x, tables, nu_pad, sq_mode=0, sq_x=None, eps=0.0, stripe=None, sq_sign=None, sq_pos=None, sq_size=None):
    """The same operator as `hfs` for planes up to 256 x 256, on the matrix cores (ee_hfs_mfma.hip)."""
    H, W = x.shape[2:]
    return _hfs("ee_hfs_mfma_f32", N.lib.ee_hfs_mfma_table_floats(H, W, nu_pad), (nu_pad,), x, tables, sq_mode, sq_x, eps, stripe, sq_sign,
                sq_pos, sq_size)


def hfs_wide(x, tables, nu_pad, nv_pad, sq_mode=0, sq_x=None, eps=0.0, stripe=None, sq_sign=None, sq_pos=None, sq_size=None):
    """The same operator for planes up to 320 x 320 with up to 48 kept row and 32 kept column frequencies (ee_hfs_wide_f32)."""
    H, W = x.shape[2:]
    return _hfs("ee_hfs_wide_f32", N.lib.ee_hfs_wide_table_floats(H, W, nu_pad, nv_pad), (nu_pad, nv_pad), x, tables, sq_mode, sq_x, eps,
                stripe, sq_sign, sq_pos, sq_size)


# ---- the fused front end of one PGD iteration (ee_chain.hip) ------------------------------------------------------------------------
def chain_supported(C, H, W):
    return bool(N.lib.ee_chain_supported(int(C), int(H), int(W)))


def chain_fwd(x, tables, wts, alpha, high, w, square=False, eps=0.0, sq_size=0, state=None, draws=None, want_edge=False):
    """x [B,C,H,W] -> (x_in, gate, gx, gy, edge): clamp(hfs(add_square(x)) + w * edge125(x), 0, 1) in ONE launch.  `draws`
    (dict stripe [B,C,1,W], sq_pos [1], sq_sign [1,C]) injects the Add_Square draws; otherwise they come from the Philox `state`
    (int64[4] device tensor {seed, offset, ticket, -}, advanced by the kernel)."""
    B, C, H, W = x.shape
    px = _chk(x, torch.float32, "x")
    pt = _chk(tables, torch.float32, "tables", (N.lib.ee_chain_table_floats(H, W),))
    x_in = torch.empty_like(x)
    gate = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    gx = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device)
    gy = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device)
    edge = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device) if want_edge else None
    ps = pp = pg = pst = None
    if square:
        if draws is not None:
            ps = _chk(draws["stripe"], torch.float32, "stripe", (B, C, 1, W))
            pp = _chk(draws["sq_pos"], torch.int64, "sq_pos", (1,))
            pg = _chk(draws["sq_sign"], torch.float32, "sq_sign", (1, C))
        else:
            pst = _chk(state, torch.int64, "state", (4,))
    N.check(N.lib.ee_chain_fwd_f32(px, B, C, H, W, pt, wts.ptr, alpha, high, w, 1 if square else 0, eps, int(sq_size), pst, ps, pp, pg,
                                   x_in.data_ptr(), gate.data_ptr(), gx.data_ptr(), gy.data_ptr(), _opt(edge, torch.float32, "edge"), _stream()),
            "ee_chain_fwd_f32")
    return x_in, gate, gx, gy, edge


def chain_bwd_(x, g_in, gate, gx, gy, x0, tables, wts, alpha, high, w, step, eps, lo=0.0, hi=1.0, direction=1):
    """In place on x: the front end's backward (edge adjoint from gx / gy, low-pass of gate * g_in times d add_square) and the PGD
    update (attacks.py:25-27) in ONE launch."""
    B, C, H, W = x.shape
    px = _chk(x, torch.float32, "x")
    pg = _chk(g_in, torch.float32, "g_in", x.shape)
    pt = _chk(gate, torch.uint8, "gate", x.shape)
    p0 = _chk(x0, torch.float32, "x0", x.shape)
    N.check(N.lib.ee_chain_bwd_f32(pg, pt, _chk(gx, torch.float32, "gx", (B, 1, H, W)), _chk(gy, torch.float32, "gy", (B, 1, H, W)), px, p0, B, C, H, W,
                                   _chk(tables, torch.float32, "tables", (N.lib.ee_chain_table_floats(H, W),)), wts.ptr, alpha, high, w, step, eps, lo,
                                   hi, direction, _stream()), "ee_chain_bwd_f32")
    return x


# ---- BatchNorm2d (+ residual) (+ ReLU) ----------------------------------------------------------------------------------
def _bn_workspace(x, B, C, HW):
    n = N.lib.ee_bn_workspace_floats(B, C, HW)
    return torch.empty(n, dtype=torch.float32, device=x.device).data_ptr() if n else None


def bn_act_fwd(x, residual, gamma, beta, running_mean, running_var, momentum, eps, training, relu):
    """y = [relu]( bn(x) [+ residual] ), one launch; returns (y, save_mean, save_invstd) (the saves are None in eval mode).
    Updates running_mean / running_var in place in training mode, as nn.BatchNorm2d does (resnet.py:44-59)."""
    B, C = x.shape[0], x.shape[1]
    HW = x[0, 0].numel() if B else 1
    px = _chk(x, torch.float32, "x")
    pr = None if residual is None else _chk(residual, torch.float32, "residual", x.shape)
    pg = None if gamma is None else _chk(gamma, torch.float32, "gamma", (C,))
    pb = None if beta is None else _chk(beta, torch.float32, "beta", (C,))
    prm = None if running_mean is None else _chk(running_mean, torch.float32, "running_mean", (C,))
    prv = None if running_var is None else _chk(running_var, torch.float32, "running_var", (C,))
    y = torch.empty_like(x)
    sm = si = psm = psi = None
    if training:
        sm = torch.empty(C, dtype=torch.float32, device=x.device)
        si = torch.empty(C, dtype=torch.float32, device=x.device)
        psm, psi = sm.data_ptr(), si.data_ptr()
    N.check(N.lib.ee_bn_act_fwd_f32(px, pr, pg, pb, prm, prv, float(momentum), float(eps), 1 if training else 0, 1 if relu else 0,
                                    _chk(y, torch.float32, "y"), psm, psi, _bn_workspace(x, B, C, HW), B, C, HW, _stream()),
            "ee_bn_act_fwd_f32")
    return y, sm, si


def bn_act_bwd(dy, y, x, gamma, save_mean, save_invstd, running_mean, running_var, eps, training, relu, want_dx=True,
               want_dres=False, want_dparams=True, dy2=None, beta=None):
    """Backward of bn_act_fwd: returns (dx, dresidual, dgamma, dbeta), None where not wanted.  `dy2`: a second piece of the incoming
    gradient (the output fed two consumers), added to dy on load.  y=None with relu (forward without residual only): the ReLU mask is
    recomputed from x, gamma and `beta`."""
    B, C = x.shape[0], x.shape[1]
    HW = x[0, 0].numel() if B else 1
    pdy = _chk(dy, torch.float32, "dy", x.shape)
    py = None if y is None else _chk(y, torch.float32, "y", x.shape)
    px = _chk(x, torch.float32, "x")
    pg = None if gamma is None else _chk(gamma, torch.float32, "gamma", (C,))
    dx = torch.empty_like(x) if want_dx else None
    dres = torch.empty_like(x) if want_dres else None
    dg = torch.empty(C, dtype=torch.float32, device=x.device) if want_dparams else None
    db = torch.empty(C, dtype=torch.float32, device=x.device) if want_dparams else None
    ptr = lambda t: None if t is None else t.data_ptr()
    pdy2 = None if dy2 is None else _chk(dy2, torch.float32, "dy2", x.shape)
    N.check(N.lib.ee_bn_act_bwd2_f32(pdy, pdy2, py, px, pg, ptr(beta), ptr(save_mean), ptr(save_invstd), ptr(running_mean), ptr(running_var), float(eps),
                                     1 if training else 0, 1 if relu else 0, ptr(dx), ptr(dres), ptr(dg), ptr(db),
                                     _bn_workspace(x, B, C, HW), B, C, HW, _stream()),
            "ee_bn_act_bwd2_f32")
    return dx, dres, dg, db


# ---- the block boundary of a pre-activation ResNet: [relu](bn(x + res)), the sum kept for the identity branch ------------------------
def bn_sum_act_supported(x):
    """1 for the shapes ee_bn_sum_act_*_f32 take: the register-cached kernels hold a channel (ee_bn.hip cached_variant: B*H*W <= 7 * 1024
    float4s, H*W % 4 == 0); the caller adds and calls bn_act_fwd otherwise."""
    if x.dim() != 4 or x.shape[0] < 1:
        return False
    HW = x.shape[2] * x.shape[3]
    return HW % 4 == 0 and x.shape[0] * (HW // 4) <= 7 * 1024 and x.numel() // 4 <= 0xffffffff


def bn_sum_act_fwd(x, res, gamma, beta, running_mean, running_var, momentum, eps, training, relu, want_sum=True):
    """s = x + res; y = [relu](bn(s)), one launch; returns (y, s, save_mean, save_invstd) (s None unless asked for, the saves None in
    eval mode).  Running statistics as bn_act_fwd."""
    B, C = x.shape[0], x.shape[1]
    HW = x[0, 0].numel() if B else 1
    px = _chk(x, torch.float32, "x")
    pr = _chk(res, torch.float32, "res", x.shape)
    ptr = lambda t, name: None if t is None else _chk(t, torch.float32, name, (C,))
    y = torch.empty_like(x)
    s = torch.empty_like(x) if want_sum else None
    sm = si = None
    if training:
        sm = torch.empty(C, dtype=torch.float32, device=x.device)
        si = torch.empty(C, dtype=torch.float32, device=x.device)
    N.check(N.lib.ee_bn_sum_act_fwd_f32(px, pr, ptr(gamma, "gamma"), ptr(beta, "beta"), ptr(running_mean, "running_mean"),
                                        ptr(running_var, "running_var"), float(momentum), float(eps), 1 if training else 0, 1 if relu else 0,
                                        None if s is None else s.data_ptr(), y.data_ptr(), None if sm is None else sm.data_ptr(),
                                        None if si is None else si.data_ptr(), B, C, HW, _stream()), "ee_bn_sum_act_fwd_f32")
    return y, s, sm, si


def bn_sum_act_bwd(dy, dy2, y, s, gamma, beta, save_mean, save_invstd, running_mean, running_var, eps, training, relu, ds_add=None,
                   want_dparams=True):
    """Backward of bn_sum_act_fwd: (ds, dgamma, dbeta) - ds is the gradient of both x and res, with ds_add (the sum's other consumer) added
    on store; dy2 a second piece of y's gradient; y=None with relu: the mask is recomputed from s, gamma and `beta`."""
    B, C = s.shape[0], s.shape[1]
    HW = s[0, 0].numel() if B else 1
    pdy = _chk(dy, torch.float32, "dy", s.shape)
    pdy2 = _opt(dy2, torch.float32, "dy2", s.shape)
    py = _opt(y, torch.float32, "y", s.shape)
    ps = _chk(s, torch.float32, "s")
    pad = _opt(ds_add, torch.float32, "ds_add", s.shape)
    ptr = lambda t: None if t is None else t.data_ptr()
    ds = torch.empty_like(s)
    dg = torch.empty(C, dtype=torch.float32, device=s.device) if want_dparams else None
    db = torch.empty(C, dtype=torch.float32, device=s.device) if want_dparams else None
    N.check(N.lib.ee_bn_sum_act_bwd_f32(pdy, pdy2, py, ps, ptr(gamma), ptr(beta), ptr(save_mean), ptr(save_invstd), ptr(running_mean),
                                        ptr(running_var), float(eps), 1 if training else 0, 1 if relu else 0, pad, ds.data_ptr(), ptr(dg),
                                        ptr(db), B, C, HW, _stream()), "ee_bn_sum_act_bwd_f32")
    return ds, dg, db


# ---- SyncBatchNorm: the local halves around the two exchanges (ee_bn.hip; the collectives live in eeadv/syncbn.py) --------------------
def syncbn_supported(x):
    """the ee_syncbn_* kernels read float4: a dense fp32 tensor whose H*W is a multiple of 4 and whose storage starts on a 16-byte boundary
    (a contiguous view may start anywhere in its storage; the entry points answer EE_ERR_ALIGN to one that does not)"""
    return x.dim() >= 3 and x.shape[0] > 0 and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.data_ptr() % 16 == 0 and (
        N.lib.ee_syncbn_workspace_floats(x.shape[0], x.shape[1], x[0, 0].numel()) > 0)


def _syncbn_workspace(x, B, C, HW):
    return torch.empty(N.lib.ee_syncbn_workspace_floats(B, C, HW), dtype=torch.float32, device=x.device)


def syncbn_stats(x):
    """this rank's (mean, M2, count) per channel: [C, 3]"""
    B, C = x.shape[0], x.shape[1]
    HW = x[0, 0].numel()
    moments = torch.empty((C, 3), dtype=torch.float32, device=x.device)
    ws = _syncbn_workspace(x, B, C, HW)
    N.check(N.lib.ee_syncbn_stats_f32(_chk(x, torch.float32, "x"), ws.data_ptr(), moments.data_ptr(), B, C, HW, _stream()), "ee_syncbn_stats_f32")
    return moments


def syncbn_apply(x, residual, gamma, beta, all_moments, running_mean, running_var, momentum, eps, relu):
    """all_moments [W, C, 3] (rank order) -> (y, save_mean, save_invstd) of the global batch; running statistics updated in place"""
    B, C = x.shape[0], x.shape[1]
    HW = x[0, 0].numel()
    W = all_moments.shape[0]
    pm = _chk(all_moments, torch.float32, "all_moments", (W, C, 3))
    ptr = lambda t: None if t is None else t.data_ptr()
    y = torch.empty_like(x)
    sm = torch.empty(C, dtype=torch.float32, device=x.device)
    si = torch.empty(C, dtype=torch.float32, device=x.device)
    pr = None if residual is None else _chk(residual, torch.float32, "residual", x.shape)
    N.check(N.lib.ee_syncbn_apply_f32(_chk(x, torch.float32, "x"), pr, ptr(gamma), ptr(beta), pm, W, ptr(running_mean), ptr(running_var), float(momentum),
                                      float(eps), 1 if relu else 0, y.data_ptr(), sm.data_ptr(), si.data_ptr(), B, C, HW, _stream()), "ee_syncbn_apply_f32")
    return y, sm, si


def syncbn_bwd_sums(dy, dy2, y, x, gamma, beta, save_mean, save_invstd, relu):
    """this rank's (sum dz, sum dz * xhat) per channel: [C, 2]"""
    B, C = x.shape[0], x.shape[1]
    HW = x[0, 0].numel()
    ptr = lambda t: None if t is None else t.data_ptr()
    sums = torch.empty((C, 2), dtype=torch.float32, device=x.device)
    ws = _syncbn_workspace(x, B, C, HW)
    N.check(N.lib.ee_syncbn_bwd_sums_f32(_chk(dy, torch.float32, "dy", x.shape), None if dy2 is None else _chk(dy2, torch.float32, "dy2", x.shape),
                                         None if y is None else _chk(y, torch.float32, "y", x.shape), _chk(x, torch.float32, "x"), ptr(gamma), ptr(beta),
                                         save_mean.data_ptr(), save_invstd.data_ptr(), 1 if relu else 0, ws.data_ptr(), sums.data_ptr(), B, C, HW, _stream()),
            "ee_syncbn_bwd_sums_f32")
    return sums


def syncbn_bwd_apply(dy, dy2, y, x, gamma, beta, save_mean, save_invstd, global_sums, n_global, relu, want_dx=True, want_dres=False):
    B, C = x.shape[0], x.shape[1]
    HW = x[0, 0].numel()
    ptr = lambda t: None if t is None else t.data_ptr()
    dx = torch.empty_like(x) if want_dx else None
    dres = torch.empty_like(x) if want_dres else None
    N.check(N.lib.ee_syncbn_bwd_apply_f32(_chk(dy, torch.float32, "dy", x.shape), None if dy2 is None else _chk(dy2, torch.float32, "dy2", x.shape),
                                          None if y is None else _chk(y, torch.float32, "y", x.shape), _chk(x, torch.float32, "x"), ptr(gamma), ptr(beta),
                                          save_mean.data_ptr(), save_invstd.data_ptr(), _chk(global_sums, torch.float32, "global_sums", (C, 2)),
                                          float(n_global), 1 if relu else 0, ptr(dx), ptr(dres), B, C, HW, _stream()), "ee_syncbn_bwd_apply_f32")
    return dx, dres


def bn_dual_supported(x):
    return x.dim() == 4 and x.shape[0] > 0 and N.lib.ee_bn_dual_supported(x.shape[0], x.shape[1], x[0, 0].numel()) == 1


def bn_dual_fwd(xa, xb, bna, bnb, training):
    """y = relu(bn_a(xa) + bn_b(xb)) in one launch (the end of a residual block with a down-sampling shortcut, resnet.py:54-59).
    bna / bnb = (gamma, beta, running_mean, running_var, momentum, eps).  Returns (y, (sm_a, si_a, sm_b, si_b)) - Nones in eval mode."""
    B, C = xa.shape[0], xa.shape[1]
    HW = xa[0, 0].numel()
    y = torch.empty_like(xa)
    saves = [None] * 4
    if training:
        saves = [torch.empty(C, dtype=torch.float32, device=xa.device) for _ in range(4)]
    ptr = lambda t: None if t is None else t.data_ptr()
    ga, ba, rma, rva, ma, ea = bna
    gb, bb, rmb, rvb, mb, eb = bnb
    N.check(N.lib.ee_bn_dual_fwd_f32(_chk(xa, torch.float32, "xa"), _chk(xb, torch.float32, "xb", xa.shape), ptr(ga), ptr(ba), ptr(rma), ptr(rva),
                                     float(ma), float(ea), ptr(saves[0]), ptr(saves[1]), ptr(gb), ptr(bb), ptr(rmb), ptr(rvb), float(mb), float(eb),
                                     ptr(saves[2]), ptr(saves[3]), 1 if training else 0, y.data_ptr(), B, C, HW, _stream()), "ee_bn_dual_fwd_f32")
    return y, tuple(saves)


def bn_dual_bwd(dy, dy2, y, xa, xb, ga, gb, saves, rma, rva, rmb, rvb, ea, eb, training, want_dxa=True, want_dxb=True, want_dparams=True):
    """Backward of bn_dual_fwd: (dxa, dxb, dgamma_a, dbeta_a, dgamma_b, dbeta_b), None where not wanted."""
    B, C = xa.shape[0], xa.shape[1]
    HW = xa[0, 0].numel()
    dxa = torch.empty_like(xa) if want_dxa else None
    dxb = torch.empty_like(xb) if want_dxb else None
    dp = [torch.empty(C, dtype=torch.float32, device=xa.device) if want_dparams else None for _ in range(4)]
    ptr = lambda t: None if t is None else t.data_ptr()
    N.check(N.lib.ee_bn_dual_bwd_f32(_chk(dy, torch.float32, "dy", xa.shape), None if dy2 is None else _chk(dy2, torch.float32, "dy2", xa.shape),
                                     _chk(y, torch.float32, "y", xa.shape), _chk(xa, torch.float32, "xa"), _chk(xb, torch.float32, "xb"), ptr(ga),
                                     ptr(saves[0]), ptr(saves[1]), ptr(rma), ptr(rva), float(ea), ptr(gb), ptr(saves[2]), ptr(saves[3]), ptr(rmb),
                                     ptr(rvb), float(eb), 1 if training else 0, ptr(dxa), ptr(dxb), ptr(dp[0]), ptr(dp[1]), ptr(dp[2]), ptr(dp[3]),
                                     B, C, HW, _stream()), "ee_bn_dual_bwd_f32")
    return (dxa, dxb) + tuple(dp)


def bn_relu_pool_supported(x):
    """relu(bn(x)) -> MaxPool2d(3, 2, 1) as one pass each way (the ResNet stem): shapes ee_bn_relu_pool_*_f32 take."""
    return x.dim() == 4 and x.shape[0] > 0 and N.lib.ee_bn_relu_pool_workspace_floats(x.shape[0], x.shape[1], x.shape[2], x.shape[3]) > 0


def _pool_workspace(x):
    n = N.lib.ee_bn_relu_pool_workspace_floats(x.shape[0], x.shape[1], x.shape[2], x.shape[3])
    return torch.empty(n, dtype=torch.float32, device=x.device)


def bn_relu_pool_fwd(x, gamma, beta, running_mean, running_var, momentum, eps, training, conv_stats=None, want_x_argmax=False):
    """maxpool3s2(relu(bn(x))) -> (y_pool, code uint8, save_mean, save_invstd) (resnet.py:113-117); the saves are None in eval mode.
    conv_stats [C,S,3]: the producing convolution's per-workgroup moments of x (stem7x7s2_fwd(want_stats=True)): no statistics pass over x.
    want_x_argmax: a fifth result, x at every window's argmax [B,C,OH,OW] - bn_relu_pool_bwd(x_argmax=...) then needs one pass over x less."""
    B, C, H, W = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((B, C, OH, OW), dtype=torch.float32, device=x.device)
    code = torch.empty((B, C, OH, OW), dtype=torch.uint8, device=x.device)
    sm = si = None
    if training:
        sm = torch.empty(C, dtype=torch.float32, device=x.device)
        si = torch.empty(C, dtype=torch.float32, device=x.device)
    ptr = lambda t: None if t is None else t.data_ptr()
    ws = _pool_workspace(x)
    cs = None if conv_stats is None else _chk(conv_stats, torch.float32, "conv_stats")
    ncs = 0 if conv_stats is None else conv_stats.shape[1]
    if want_x_argmax:
        xa = torch.empty((B, C, OH, OW), dtype=torch.float32, device=x.device)
        N.check(N.lib.ee_bn_relu_pool_fwd_xa_f32(_chk(x, torch.float32, "x"), ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), float(momentum),
                                                 float(eps), 1 if training else 0, y.data_ptr(), code.data_ptr(), xa.data_ptr(), ptr(sm), ptr(si),
                                                 ws.data_ptr(), cs, ncs, B, C, H, W, _stream()), "ee_bn_relu_pool_fwd_xa_f32")
        return y, code, sm, si, xa
    N.check(N.lib.ee_bn_relu_pool_fwd_f32(_chk(x, torch.float32, "x"), ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), float(momentum),
                                          float(eps), 1 if training else 0, y.data_ptr(), code.data_ptr(), ptr(sm), ptr(si), ws.data_ptr(),
                                          cs, ncs, B, C, H, W, _stream()), "ee_bn_relu_pool_fwd_f32")
    return y, code, sm, si


def bn_relu_pool_bwd(dy_pool, code, x, gamma, beta, save_mean, save_invstd, running_mean, running_var, eps, training, want_dx=True,
                     want_dparams=True, dy_pool2=None, x_argmax=None):
    """Backward of bn_relu_pool_fwd: (dx, dgamma, dbeta), None where not wanted; `dy_pool2` = a second piece of the gradient;
    `x_argmax` (bn_relu_pool_fwd(want_x_argmax=True)): training mode then takes its batch sums from the pooled tensors."""
    B, C, H, W = x.shape
    dx = torch.empty_like(x) if want_dx else None
    dg = torch.empty(C, dtype=torch.float32, device=x.device) if want_dparams else None
    db = torch.empty(C, dtype=torch.float32, device=x.device) if want_dparams else None
    ptr = lambda t: None if t is None else t.data_ptr()
    ws = _pool_workspace(x)
    p2 = None if dy_pool2 is None else _chk(dy_pool2, torch.float32, "dy_pool2", code.shape)
    if x_argmax is not None:
        N.check(N.lib.ee_bn_relu_pool_bwd_xa_f32(_chk(dy_pool, torch.float32, "dy_pool", code.shape), p2, _chk(code, torch.uint8, "code"),
                                                 _chk(x, torch.float32, "x"), _chk(x_argmax, torch.float32, "x_argmax", code.shape), ptr(gamma), ptr(beta),
                                                 ptr(save_mean), ptr(save_invstd), ptr(running_mean), ptr(running_var), float(eps), 1 if training else 0,
                                                 ptr(dx), ptr(dg), ptr(db), ws.data_ptr(), B, C, H, W, _stream()), "ee_bn_relu_pool_bwd_xa_f32")
        return dx, dg, db
    N.check(N.lib.ee_bn_relu_pool_bwd_f32(_chk(dy_pool, torch.float32, "dy_pool", code.shape), p2, _chk(code, torch.uint8, "code"),
                                          _chk(x, torch.float32, "x"), ptr(gamma), ptr(beta), ptr(save_mean), ptr(save_invstd), ptr(running_mean),
                                          ptr(running_var), float(eps), 1 if training else 0, ptr(dx), ptr(dg), ptr(db), ws.data_ptr(),
                                          B, C, H, W, _stream()), "ee_bn_relu_pool_bwd_f32")
    return dx, dg, db


# ---- stem max-pool and classifier head -----------------------------------------------------------------------------------
def maxpool3s2_fwd(x):
    """MaxPool2d(3, 2, 1) of x [B,C,H,W] -> (y, code uint8) (resnet.py:117)."""
    B, C, H, W = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((B, C, OH, OW), dtype=torch.float32, device=x.device)
    code = torch.empty((B, C, OH, OW), dtype=torch.uint8, device=x.device)
    N.check(N.lib.ee_maxpool3s2_fwd_f32(_chk(x, torch.float32, "x"), _chk(y, torch.float32, "y"), _chk(code, torch.uint8, "code"), B * C, H, W,
                                        _stream()), "ee_maxpool3s2_fwd_f32")
    return y, code


def maxpool3s2_bwd(dy, code, H, W):
    B, C, OH, OW = dy.shape
    if (OH, OW) != ((H - 1) // 2 + 1, (W - 1) // 2 + 1):
        raise ValueError("maxpool3s2_bwd: dy %s does not belong to a %dx%d input" % (tuple(dy.shape), H, W))
    dx = torch.empty((B, C, H, W), dtype=torch.float32, device=dy.device)
    N.check(N.lib.ee_maxpool3s2_bwd_f32(_chk(dy, torch.float32, "dy"), _chk(code, torch.uint8, "code", dy.shape), _chk(dx, torch.float32, "dx"),
                                        B * C, H, W, _stream()), "ee_maxpool3s2_bwd_f32")
    return dx


def conv1x1s2_fwd(x, weight):
    """Conv2d(Cin, Cout, 1, stride=2, bias=False) (resnet.py:137-142): x [B,Cin,H,W], weight [Cout,Cin,1,1]."""
    B, Cin, H, W = x.shape
    Cout = weight.shape[0]
    y = torch.empty((B, Cout, H // 2, W // 2), dtype=torch.float32, device=x.device)
    N.check(N.lib.ee_conv1x1s2_fwd_f32(_chk(x, torch.float32, "x"), _chk(weight, torch.float32, "weight", (Cout, Cin, 1, 1)), y.data_ptr(), B,
                                       Cin, Cout, H, W, _stream()), "ee_conv1x1s2_fwd_f32")
    return y


def conv1x1s2_bwd(dy, weight, H, W):
    B, Cout = dy.shape[0], dy.shape[1]
    Cin = weight.shape[1]
    dx = torch.empty((B, Cin, H, W), dtype=torch.float32, device=dy.device)
    N.check(N.lib.ee_conv1x1s2_bwd_f32(_chk(dy, torch.float32, "dy", (B, Cout, H // 2, W // 2)),
                                       _chk(weight, torch.float32, "weight", (Cout, Cin, 1, 1)), dx.data_ptr(), B, Cin, Cout, H, W, _stream()),
            "ee_conv1x1s2_bwd_f32")
    return dx


def wino3x3_supported(x, cin, cout):
    return x.dim() == 4 and x.shape[2] == x.shape[3] and x.shape[2] in (4, 8, 16) and cin % 32 == 0 and cout % 32 == 0


def wino3x3(x, u):
    """3x3 / stride 1 / padding 1 convolution of 4x4, 8x8 or 16x16 maps, filters in the Winograd domain: x [B,KC,H,H], u [16,KC,RC] -> [B,RC,H,H]."""
    B, KC, H = x.shape[0], x.shape[1], x.shape[2]
    RC = u.shape[2]
    y = torch.empty((B, RC, H, H), dtype=torch.float32, device=x.device)
    N.check(N.lib.ee_wino3x3_f32(_chk(x, torch.float32, "x", (B, KC, H, H)), _chk(u, torch.float32, "u", (16, KC, RC)), y.data_ptr(), B, KC, RC, H,
                                 _stream()), "ee_wino3x3_f32")
    return y


def _optf(t, name, shape=None):
    return None if t is None else _chk(t, torch.float32, name, shape)


def wino3x3_bn_eval_fwd(x, u, bn, res, relu):
    """[relu]( bn(conv3x3(x)) [+ res] ) with bn in eval mode (running statistics) in ONE launch: bn = (mean, var, gamma, beta, eps)"""
    B, KC, H = x.shape[0], x.shape[1], x.shape[2]
    RC = u.shape[2]
    mean, var, gamma, beta, eps = bn
    y = torch.empty((B, RC, H, H), dtype=torch.float32, device=x.device)
    N.check(N.lib.ee_wino3x3_bn_eval_fwd_f32(_chk(x, torch.float32, "x", (B, KC, H, H)), _chk(u, torch.float32, "u", (16, KC, RC)),
                                             _chk(mean, torch.float32, "running_mean", (RC,)), _chk(var, torch.float32, "running_var", (RC,)),
                                             _optf(gamma, "gamma", (RC,)), _optf(beta, "beta", (RC,)), float(eps), _optf(res, "res", (B, RC, H, H)),
                                             1 if relu else 0, y.data_ptr(), B, KC, RC, H, _stream()), "ee_wino3x3_bn_eval_fwd_f32")
    return y


def wino3x3_bn_eval_bwd(dy, dy2, y, u_b, bn, want_dres, dx_add=None):
    """dz = (y > 0) * (dy [+ dy2]); dx = conv3x3^T(gamma / sqrt(var + eps) * dz) [+ dx_add] in ONE launch -> (dx, dz or None).
    bn = (var, gamma, eps) of the BatchNorm behind the convolution; u_b [16, Cout, Cin]."""
    B, Cout, H = dy.shape[0], dy.shape[1], dy.shape[2]
    Cin = u_b.shape[2]
    var, gamma, eps = bn
    dx = torch.empty((B, Cin, H, H), dtype=torch.float32, device=dy.device)
    dres = torch.empty_like(dy) if want_dres else None
    N.check(N.lib.ee_wino3x3_bn_eval_bwd_f32(_chk(dy, torch.float32, "dy", (B, Cout, H, H)), _optf(dy2, "dy2", (B, Cout, H, H)),
                                             _chk(y, torch.float32, "y", (B, Cout, H, H)), _chk(u_b, torch.float32, "u_b", (16, Cout, Cin)),
                                             _chk(var, torch.float32, "running_var", (Cout,)), _optf(gamma, "gamma", (Cout,)), float(eps),
                                             None if dres is None else dres.data_ptr(), _optf(dx_add, "dx_add", (B, Cin, H, H)), dx.data_ptr(),
                                             B, Cin, Cout, H, _stream()), "ee_wino3x3_bn_eval_bwd_f32")
    return dx, dres


def conv3x3s2_pair_bn_eval_fwd(x, w10, cout, bn3, bn1):
    """(relu(bn3(conv3x3s2(x))), bn1(conv1x1s2(x))) with both BatchNorms in eval mode, ONE launch: bn = (mean, var, gamma, beta, eps)"""
    B, Cin, H = x.shape[0], x.shape[1], x.shape[2]
    y3 = torch.empty((B, cout, H // 2, H // 2), dtype=torch.float32, device=x.device)
    y1 = torch.empty_like(y3)
    N.check(N.lib.ee_conv3x3s2_pair_bn_eval_fwd_f32(
        _chk(x, torch.float32, "x", (B, Cin, H, H)), _chk(w10, torch.float32, "w10", (cout // 32, Cin // 16, 10, 4, 2, 16, 4)),
        _chk(bn3[0], torch.float32, "mean3", (cout,)), _chk(bn3[1], torch.float32, "var3", (cout,)), _optf(bn3[2], "gamma3", (cout,)), _optf(bn3[3], "beta3", (cout,)), float(bn3[4]),
        _chk(bn1[0], torch.float32, "mean1", (cout,)), _chk(bn1[1], torch.float32, "var1", (cout,)), _optf(bn1[2], "gamma1", (cout,)), _optf(bn1[3], "beta1", (cout,)), float(bn1[4]),
        y3.data_ptr(), y1.data_ptr(), B, Cin, cout, H, _stream()), "ee_conv3x3s2_pair_bn_eval_fwd_f32")
    return y3, y1


def conv3x3s2_pair_bn_eval_bwd(dy3, y3, dy1, w10, cin, bn3, bn1):
    """dx = conv3x3s2^T(gamma3 / sqrt(var3 + eps3) * (y3 > 0) * dy3) + conv1x1s2^T(gamma1 / sqrt(var1 + eps1) * dy1); bn = (var, gamma, eps)"""
    B, Cout, OH = dy3.shape[0], dy3.shape[1], dy3.shape[2]
    dx = torch.empty((B, cin, 2 * OH, 2 * OH), dtype=torch.float32, device=dy3.device)
    N.check(N.lib.ee_conv3x3s2_pair_bn_eval_bwd_f32(
        _chk(dy3, torch.float32, "dy3", (B, Cout, OH, OH)), _chk(y3, torch.float32, "y3", (B, Cout, OH, OH)), _chk(dy1, torch.float32, "dy1", (B, Cout, OH, OH)),
        _chk(w10, torch.float32, "w10", (cin // 32, Cout // 16, 10, 4, 2, 16, 4)), _chk(bn3[0], torch.float32, "var3", (Cout,)), _optf(bn3[1], "gamma3", (Cout,)),
        float(bn3[2]), _chk(bn1[0], torch.float32, "var1", (Cout,)), _optf(bn1[1], "gamma1", (Cout,)), float(bn1[2]), dx.data_ptr(), B, cin, Cout, 2 * OH,
        _stream()), "ee_conv3x3s2_pair_bn_eval_bwd_f32")
    return dx


def wino3x3_stats(x, u):
    """conv3x3(x) and, per (result channel, image), the plane's (mean, M2): (y, stats [RC, B, 2]) - the producer half of a train-mode
    BatchNorm exchanged across the kernel boundary (ee_wino3x3_stats_f32)"""
    B, KC, H = x.shape[0], x.shape[1], x.shape[2]
    RC = u.shape[2]
    y = torch.empty((B, RC, H, H), dtype=torch.float32, device=x.device)
    stats = torch.empty((RC, B, 2), dtype=torch.float32, device=x.device)
    N.check(N.lib.ee_wino3x3_stats_f32(_chk(x, torch.float32, "x", (B, KC, H, H)), _chk(u, torch.float32, "u", (16, KC, RC)), y.data_ptr(), stats.data_ptr(),
                                       B, KC, RC, H, _stream()), "ee_wino3x3_stats_f32")
    return y, stats


def wino3x3_bn_train_pre(x, stats, cnt, gamma, beta, eps, momentum, running_mean, running_var, u):
    """conv3x3(relu(batch_norm(x))) in TRAIN mode, the batch statistics merged from `stats` [KC, S, 2] (S partials of `cnt` values each):
    (y, save_mean, save_invstd); running_mean / running_var (or None) move by `momentum` (ee_wino3x3_bn_train_pre_f32)"""
    B, KC, H = x.shape[0], x.shape[1], x.shape[2]
    RC = u.shape[2]
    S = stats.shape[1]
    y = torch.empty((B, RC, H, H), dtype=torch.float32, device=x.device)
    sm = torch.empty(KC, dtype=torch.float32, device=x.device)
    si = torch.empty(KC, dtype=torch.float32, device=x.device)
    N.check(N.lib.ee_wino3x3_bn_train_pre_f32(_chk(x, torch.float32, "x", (B, KC, H, H)), _chk(stats, torch.float32, "stats", (KC, S, 2)), S, int(cnt),
                                              _optf(gamma, "gamma", (KC,)), _optf(beta, "beta", (KC,)), float(eps), float(momentum),
                                              _optf(running_mean, "running_mean", (KC,)), _optf(running_var, "running_var", (KC,)), sm.data_ptr(), si.data_ptr(),
                                              _chk(u, torch.float32, "u", (16, KC, RC)), y.data_ptr(), B, KC, RC, H, _stream()), "ee_wino3x3_bn_train_pre_f32")
    return y, sm, si


def wino3x3_bwd_sums(dc, u_b, x, save_mean, save_invstd, gamma, beta):
    """dy = conv3x3^T(dc) (the backward-data of the layer behind a train-mode BatchNorm) plus, per (channel, image), (sum dz, sum dz * xhat) with
    dz = (bn(x) > 0) * dy: (dy, sums [Cin, B, 2]) - the producer half of the BatchNorm backward across the kernel boundary (16x16 maps)"""
    B, Cout, H = dc.shape[0], dc.shape[1], dc.shape[2]
    Cin = u_b.shape[2]
    dy = torch.empty((B, Cin, H, H), dtype=torch.float32, device=dc.device)
    sums = torch.empty((Cin, B, 2), dtype=torch.float32, device=dc.device)
    N.check(N.lib.ee_wino3x3_bwd_sums_f32(_chk(dc, torch.float32, "dc", (B, Cout, H, H)), _chk(u_b, torch.float32, "u_b", (16, Cout, Cin)),
                                          _chk(x, torch.float32, "x", (B, Cin, H, H)), _chk(save_mean, torch.float32, "save_mean", (Cin,)),
                                          _chk(save_invstd, torch.float32, "save_invstd", (Cin,)), _optf(gamma, "gamma", (Cin,)), _optf(beta, "beta", (Cin,)),
                                          dy.data_ptr(), sums.data_ptr(), B, Cin, Cout, H, _stream()), "ee_wino3x3_bwd_sums_f32")
    return dy, sums


def wino3x3_bn_train_bwd_pre(dy, x, sums, cnt, save_mean, save_invstd, gamma, beta, u_b):
    """dx = conv3x3^T(batch_norm_relu_backward(dy; x)) in TRAIN mode, the batch means of dz and dz * xhat merged from `sums` [Cout, S, 2]"""
    B, Cout, H = dy.shape[0], dy.shape[1], dy.shape[2]
    Cin = u_b.shape[2]
    dx = torch.empty((B, Cin, H, H), dtype=torch.float32, device=dy.device)
    N.check(N.lib.ee_wino3x3_bn_train_bwd_pre_f32(_chk(dy, torch.float32, "dy", (B, Cout, H, H)), _chk(x, torch.float32, "x", (B, Cout, H, H)),
                                                  _chk(sums, torch.float32, "sums", (Cout, sums.shape[1], 2)), sums.shape[1], int(cnt),
                                                  _chk(save_mean, torch.float32, "save_mean", (Cout,)), _chk(save_invstd, torch.float32, "save_invstd", (Cout,)),
                                                  _optf(gamma, "gamma", (Cout,)), _optf(beta, "beta", (Cout,)), _chk(u_b, torch.float32, "u_b", (16, Cout, Cin)),
                                                  dx.data_ptr(), B, Cin, Cout, H, _stream()), "ee_wino3x3_bn_train_bwd_pre_f32")
    return dx


def conv3x3s2_pair_stats_fwd(x, w10, cout):
    """conv3x3s2_pair_fwd plus the statistics of y3 for the train-mode BatchNorm behind it: (y3, y1, stats [Cout, S, 2], cnt)"""
    B, Cin, H = x.shape[0], x.shape[1], x.shape[2]
    y3 = torch.empty((B, cout, H // 2, H // 2), dtype=torch.float32, device=x.device)
    y1 = torch.empty_like(y3)
    S, cnt = (2 * B, 32) if H == 16 else (B, 16)
    stats = torch.empty((cout, S, 2), dtype=torch.float32, device=x.device)
    N.check(N.lib.ee_conv3x3s2_pair_stats_fwd_f32(_chk(x, torch.float32, "x", (B, Cin, H, H)), _chk(w10, torch.float32, "w10", (cout // 32, Cin // 16, 10, 4, 2, 16, 4)),
                                                  y3.data_ptr(), y1.data_ptr(), stats.data_ptr(), B, Cin, cout, H, _stream()), "ee_conv3x3s2_pair_stats_fwd_f32")
    return y3, y1, stats, cnt


def dense2x2_supported(cin, cout):
    return cin % 128 == 0 and cout % 8 == 0


def dense2x2(x, w2):
    """conv3x3 on a 2x2 map as one dense product (ee_dense.hip): x [B, Cin, 2, 2], w2 [4 Cin, 4 Cout] -> [B, Cout, 2, 2]"""
    B, Cin = x.shape[0], x.shape[1]
    Cout = w2.shape[1] // 4
    y = torch.empty((B, Cout, 2, 2), dtype=torch.float32, device=x.device)
    N.check(N.lib.ee_dense2x2_f32(_chk(x, torch.float32, "x", (B, Cin, 2, 2)), _chk(w2, torch.float32, "w2", (4 * Cin, 4 * Cout)), y.data_ptr(), B, Cin, Cout,
                                  _stream()), "ee_dense2x2_f32")
    return y


def dense2x2_bn_eval_fwd(x, w2, bn, res, relu):
    """[relu]( bn(conv3x3(x)) [+ res] ) on a 2x2 map with bn in eval mode, ONE launch: bn = (mean, var, gamma, beta, eps)"""
    B, Cin = x.shape[0], x.shape[1]
    Cout = w2.shape[1] // 4
    mean, var, gamma, beta, eps = bn
    y = torch.empty((B, Cout, 2, 2), dtype=torch.float32, device=x.device)
    N.check(N.lib.ee_dense2x2_bn_eval_fwd_f32(_chk(x, torch.float32, "x", (B, Cin, 2, 2)), _chk(w2, torch.float32, "w2", (4 * Cin, 4 * Cout)),
                                              _chk(mean, torch.float32, "running_mean", (Cout,)), _chk(var, torch.float32, "running_var", (Cout,)),
                                              _optf(gamma, "gamma", (Cout,)), _optf(beta, "beta", (Cout,)), float(eps), _optf(res, "res", (B, Cout, 2, 2)),
                                              1 if relu else 0, y.data_ptr(), B, Cin, Cout, _stream()), "ee_dense2x2_bn_eval_fwd_f32")
    return y


def dense2x2_bn_eval_bwd(dy, dy2, y, w2t, bn, want_dres, dx_add=None):
    """dz = (y > 0) * (dy [+ dy2]); dx = (gamma / sqrt(var + eps) * dz) . w2t [+ dx_add] -> (dx, dz or None); w2t [4 Cout, 4 Cin]; bn = (var, gamma, eps)"""
    B, Cout = dy.shape[0], dy.shape[1]
    Cin = w2t.shape[1] // 4
    var, gamma, eps = bn
    dx = torch.empty((B, Cin, 2, 2), dtype=torch.float32, device=dy.device)
    dres = torch.empty_like(dy) if want_dres else None
    N.check(N.lib.ee_dense2x2_bn_eval_bwd_f32(_chk(dy, torch.float32, "dy", (B, Cout, 2, 2)), _optf(dy2, "dy2", (B, Cout, 2, 2)),
                                              _chk(y, torch.float32, "y", (B, Cout, 2, 2)), _chk(w2t, torch.float32, "w2t", (4 * Cout, 4 * Cin)),
                                              _chk(var, torch.float32, "running_var", (Cout,)), _optf(gamma, "gamma", (Cout,)), float(eps),
                                              None if dres is None else dres.data_ptr(), _optf(dx_add, "dx_add", (B, Cin, 2, 2)), dx.data_ptr(),
                                              B, Cin, Cout, _stream()), "ee_dense2x2_bn_eval_bwd_f32")
    return dx, dres


def fd_supported(C, P):
    """ee_fd.hip takes the map: C % 64 == 0, C <= 2048, 1 <= P <= 4096, min(C, P) <= 256"""
    return bool(N.lib.ee_fd_supported(int(C), int(P)))


def _fd_on_kernel(x):
    return x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.shape[0] <= 65535 and fd_supported(x.shape[1], x.shape[2])


def _fd_check(x, name):
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or not x.is_floating_point():
        raise ValueError("%s must be a floating-point [N, C, P] tensor" % name)


def fd_fwd(x, scale):
    """The feature-denoising product per sample (resnet_fd.py:133-148 with embed=False, softmax=False): x [N, C, P] -> (f, gram) with
    f = scale * X X^T X and gram [N, d, d], d = min(C, P), the unscaled X X^T (C <= P) or X^T X (C > P) that fd_bwd reuses.  Dense fp32 ROCm
    tensors of a supported shape (fd_supported) run on ee_fd.hip; CPU tensors, other dtypes and other shapes take plain matmuls in the
    reference's association (the host fallback: the block exists at every size, the kernel only where it was built)."""
    _fd_check(x, "x")
    n, C, P = x.shape
    if not _fd_on_kernel(x):
        xt = x.transpose(1, 2)
        if C > P:
            gram = torch.matmul(xt, x)
            return torch.matmul(x, gram) * scale, gram
        gram = torch.matmul(x, xt)
        return torch.matmul(gram, x) * scale, gram
    d = min(C, P)
    f = torch.empty_like(x)
    gram = torch.empty((n, d, d), dtype=torch.float32, device=x.device)
    ws = torch.empty(max(int(N.lib.ee_fd_scratch_floats(n, C, P)), 4), dtype=torch.float32, device=x.device)
    N.check(N.lib.ee_fd_fwd_f32(_chk(x, torch.float32, "x"), f.data_ptr(), gram.data_ptr(), ws.data_ptr(), n, C, P, float(scale), _stream()), "ee_fd_fwd_f32")
    return f, gram


def fd_bwd(x, df, gram, scale):
    """d fd_fwd / d x for the upstream gradient df [N, C, P]: scale * [(M + M^T) X + G D], M = D X^T (C <= P) or scale * [D A + X (B + B^T)],
    B = D^T X (C > P), with G / A = fd_fwd's gram; the same routing as fd_fwd."""
    _fd_check(x, "x")
    n, C, P = x.shape
    d = min(C, P)
    if tuple(df.shape) != (n, C, P) or tuple(gram.shape) != (n, d, d):
        raise ValueError("df %s / gram %s do not match x %s" % (tuple(df.shape), tuple(gram.shape), tuple(x.shape)))
    if not _fd_on_kernel(x):
        if C > P:
            b = torch.matmul(df.transpose(1, 2), x)
            return (torch.matmul(df, gram) + torch.matmul(x, b + b.transpose(1, 2))) * scale
        m = torch.matmul(df, x.transpose(1, 2))
        return (torch.matmul(m + m.transpose(1, 2), x) + torch.matmul(gram, df)) * scale
    dx = torch.empty_like(x)
    ws = torch.empty(max(int(N.lib.ee_fd_scratch_floats(n, C, P)), 4), dtype=torch.float32, device=x.device)
    N.check(N.lib.ee_fd_bwd_f32(_chk(x, torch.float32, "x"), _chk(df, torch.float32, "df"), _chk(gram, torch.float32, "gram"), dx.data_ptr(), ws.data_ptr(),
                                n, C, P, float(scale), _stream()), "ee_fd_bwd_f32")
    return dx


def wrw3x3_supported(x, dy):
    """ee_wrw.hip: weight gradient of a 3x3 / stride 1 / padding 1 convolution on 2x2, 4x4, 8x8 or 16x16 maps"""
    return (x.dim() == 4 and dy.dim() == 4 and x.shape[2] == x.shape[3] and x.shape[2] in (2, 4, 8, 16) and x.shape[2:] == dy.shape[2:]
            and x.shape[0] == dy.shape[0] and x.shape[1] % 32 == 0 and dy.shape[1] % 32 == 0 and x.is_cuda and x.dtype == torch.float32
            and dy.dtype == torch.float32 and x.is_contiguous() and dy.is_contiguous())


def wrw3x3(x, dy):
    """d loss / d weight [Cout,Cin,3,3] of conv3x3(x, weight) (stride 1, padding 1) from its input x [B,Cin,H,H] and output gradient dy [B,Cout,H,H]:
    Winograd F(3x3, 2x2) on the matrix cores, partial sums added in a fixed order (bit-reproducible)."""
    B, Cin, H = x.shape[0], x.shape[1], x.shape[2]
    Cout = dy.shape[1]
    dw = torch.empty((Cout, Cin, 3, 3), dtype=torch.float32, device=x.device)
    n = int(N.lib.ee_wrw3x3_workspace_floats(B, Cin, Cout, H))
    ws = torch.empty(max(n, 4), dtype=torch.float32, device=x.device)
    N.check(N.lib.ee_wrw3x3_f32(_chk(x, torch.float32, "x", (B, Cin, H, H)), _chk(dy, torch.float32, "dy", (B, Cout, H, H)), dw.data_ptr(), ws.data_ptr(),
                                B, Cin, Cout, H, _stream()), "ee_wrw3x3_f32")
    return dw


def wrw3x3s2_supported(x, dy3, dy1=None):
    """ee_wrw.hip: weight gradient of a 3x3 / stride 2 / padding 1 convolution from a 16x16, 8x8 or 4x4 map (and of the 1x1 / stride 2 shortcut)"""
    ok = (x.dim() == 4 and dy3.dim() == 4 and x.shape[2] == x.shape[3] and x.shape[2] in (4, 8, 16) and dy3.shape[2] == dy3.shape[3] == x.shape[2] // 2
          and x.shape[0] == dy3.shape[0] and x.shape[1] % 32 == 0 and dy3.shape[1] % 32 == 0 and x.is_cuda and x.dtype == torch.float32
          and dy3.dtype == torch.float32 and x.is_contiguous() and dy3.is_contiguous())
    return ok and (dy1 is None or (dy1.shape == dy3.shape and dy1.dtype == torch.float32 and dy1.is_contiguous()))


def wrw3x3s2(x, dy3, dy1=None):
    """(dw3 [Cout,Cin,3,3], dw1 [Cout,Cin,1,1] or None): weight gradients of conv3x3(x) (stride 2, padding 1) and, with dy1, of the 1x1 / stride 2
    shortcut of the same x, in one launch + the fixed-order sum (two views of one buffer)"""
    B, Cin, H = x.shape[0], x.shape[1], x.shape[2]
    Cout = dy3.shape[1]
    taps = 9 if dy1 is None else 10
    dw = torch.empty(taps * Cout * Cin, dtype=torch.float32, device=x.device)
    n = int(N.lib.ee_wrw3x3s2_workspace_floats(B, Cin, Cout, H, 0 if dy1 is None else 1))
    ws = torch.empty(max(n, 4), dtype=torch.float32, device=x.device)
    N.check(N.lib.ee_wrw3x3s2_f32(_chk(x, torch.float32, "x", (B, Cin, H, H)), _chk(dy3, torch.float32, "dy3", (B, Cout, H // 2, H // 2)),
                                  None if dy1 is None else _chk(dy1, torch.float32, "dy1", (B, Cout, H // 2, H // 2)), dw.data_ptr(), ws.data_ptr(),
                                  B, Cin, Cout, H, _stream()), "ee_wrw3x3s2_f32")
    dw3 = dw[:9 * Cout * Cin].view(Cout, Cin, 3, 3)
    return dw3, (None if dy1 is None else dw[9 * Cout * Cin:].view(Cout, Cin, 1, 1))


def wrw_stem7x7s2_supported(x, dy):
    """ee_wrw.hip: weight gradient of the stem Conv2d(3, 64, 7, stride 2, padding 3)"""
    return (x.dim() == 4 and dy.dim() == 4 and x.shape[1] == 3 and dy.shape[1] == 64 and x.shape[2] % 2 == 0 and x.shape[3] % 32 == 0
            and tuple(dy.shape[2:]) == (x.shape[2] // 2, x.shape[3] // 2) and x.shape[0] == dy.shape[0] and x.is_cuda and x.dtype == torch.float32
            and dy.dtype == torch.float32 and x.is_contiguous() and dy.is_contiguous())


def wrw_stem7x7s2(x, dy):
    """d loss / d weight [64,3,7,7] of the stem convolution from its input x [B,3,H,W] and output gradient dy [B,64,H/2,W/2] (bit-reproducible)"""
    B, H, W = x.shape[0], x.shape[2], x.shape[3]
    dw = torch.empty((64, 3, 7, 7), dtype=torch.float32, device=x.device)
    n = int(N.lib.ee_wrw_stem7x7s2_workspace_floats(B, H, W))
    ws = torch.empty(max(n, 4), dtype=torch.float32, device=x.device)
    N.check(N.lib.ee_wrw_stem7x7s2_f32(_chk(x, torch.float32, "x", (B, 3, H, W)), _chk(dy, torch.float32, "dy", (B, 64, H // 2, W // 2)), dw.data_ptr(),
                                       ws.data_ptr(), B, H, W, _stream()), "ee_wrw_stem7x7s2_f32")
    return dw


def wrw1x1_supported(x, dy):
    """ee_wrw.hip: weight gradient of a 1x1 / stride 1 convolution, NCHW operands"""
    return (x.dim() == 4 and dy.dim() == 4 and x.shape[0] == dy.shape[0] and x.shape[2:] == dy.shape[2:] and x.shape[1] % 64 == 0 and dy.shape[1] % 64 == 0
            and (x.shape[2] * x.shape[3]) % 4 == 0 and x.is_cuda and x.dtype == torch.float32 and dy.dtype == torch.float32 and x.is_contiguous()
            and dy.is_contiguous())


def wrw1x1(x, dy):
    """d loss / d weight [Cout,Cin,1,1] of conv1x1(x, weight) (stride 1) from its input x [B,Cin,H,W] and output gradient dy [B,Cout,H,W] (bit-reproducible)"""
    B, Cin, HW = x.shape[0], x.shape[1], x.shape[2] * x.shape[3]
    Cout = dy.shape[1]
    dw = torch.empty((Cout, Cin, 1, 1), dtype=torch.float32, device=x.device)
    n = int(N.lib.ee_wrw1x1_workspace_floats(B, Cin, Cout, HW))
    ws = torch.empty(max(n, 4), dtype=torch.float32, device=x.device)
    N.check(N.lib.ee_wrw1x1_f32(_chk(x, torch.float32, "x"), _chk(dy, torch.float32, "dy"), dw.data_ptr(), ws.data_ptr(), B, Cin, Cout, HW, _stream()),
            "ee_wrw1x1_f32")
    return dw


def conv3x3s2_small_supported(x, cin, cout):
    """ee_s2.hip: 3x3 / stride 2 / padding 1 from a 16x16, 8x8 or 4x4 map"""
    return x.dim() == 4 and x.shape[2] == x.shape[3] and x.shape[2] in (4, 8, 16) and cin % 32 == 0 and cout % 32 == 0


def conv3x3s2_small_fwd(x, w9, cout):
    """x [B,Cin,H,H] (H = 16, 8 or 4), w9 = the filters rearranged (functional._rearranged kind "s2m_f") -> [B,Cout,H/2,H/2]"""
    B, Cin, H = x.shape[0], x.shape[1], x.shape[2]
    y = torch.empty((B, cout, H // 2, H // 2), dtype=torch.float32, device=x.device)
    N.check(N.lib.ee_conv3x3s2_small_fwd_f32(_chk(x, torch.float32, "x", (B, Cin, H, H)), _chk(w9, torch.float32, "w9", (cout // 32, Cin // 16, 9, 4, 2, 16, 4)),
                                             y.data_ptr(), B, Cin, cout, H, _stream()), "ee_conv3x3s2_small_fwd_f32")
    return y


def conv3x3s2_small_bwd_data(dy, w9, cin):
    """dy [B,Cout,H/2,H/2], w9 = the filters rearranged (kind "s2m_b") -> dx [B,Cin,H,H] (H = 16, 8 or 4)"""
    B, Cout, OH = dy.shape[0], dy.shape[1], dy.shape[2]
    dx = torch.empty((B, cin, 2 * OH, 2 * OH), dtype=torch.float32, device=dy.device)
    N.check(N.lib.ee_conv3x3s2_small_bwd_data_f32(_chk(dy, torch.float32, "dy", (B, Cout, OH, OH)),
                                                  _chk(w9, torch.float32, "w9", (cin // 32, Cout // 16, 9, 4, 2, 16, 4)), dx.data_ptr(), B, cin, Cout, 2 * OH,
                                                  _stream()), "ee_conv3x3s2_small_bwd_data_f32")
    return dx


def conv_weight_prep(kind, weight, extra, out):
    """ee_wprep.hip: the filters of one convolution in the order its kernel reads them (kind = EE_WPREP_* of eeadv.h), written into `out`
    in one launch; `extra` = the shortcut's 1x1 weight for the paired stride-2 kinds."""
    co, ci = weight.shape[0], weight.shape[1]
    N.check(N.lib.ee_conv_weight_prep_f32(kind, _chk(weight, torch.float32, "weight", (co, ci, 3, 3)),
                                          None if extra is None else _chk(extra, torch.float32, "extra", (co, ci, 1, 1)),
                                          _chk(out, torch.float32, "out"), co, ci, _stream()), "ee_conv_weight_prep_f32")
    return out


def conv_weight_prep_batch(items):
    """ee_wprep.hip: `items` = [(kind, weight, extra or None, out)] - every rearranged copy in ONE launch per 64 items (ee_conv_weight_prep_batch_f32)"""
    n = len(items)
    if not n:
        return
    kinds = (ctypes.c_int * n)(*[int(k) for k, _, _, _ in items])
    cout = (ctypes.c_int * n)(*[w.shape[0] for _, w, _, _ in items])
    cin = (ctypes.c_int * n)(*[w.shape[1] for _, w, _, _ in items])
    pw = (ctypes.c_void_p * n)(*[_chk(w, torch.float32, "weight", (w.shape[0], w.shape[1], 3, 3)).value for _, w, _, _ in items])
    pe = (ctypes.c_void_p * n)(*[None if e is None else _chk(e, torch.float32, "extra", (w.shape[0], w.shape[1], 1, 1)).value for _, w, e, _ in items])
    po = (ctypes.c_void_p * n)(*[_chk(o, torch.float32, "out").value for _, _, _, o in items])
    N.check(N.lib.ee_conv_weight_prep_batch_f32(n, kinds, pw, pe, po, cout, cin, _stream()), "ee_conv_weight_prep_batch_f32")


def conv3x3s2_pair_fwd(x, w10, cout):
    """conv3x3 / stride 2 / padding 1 AND conv1x1 / stride 2 of the same x in one launch (a down-sampling BasicBlock's conv1 and shortcut):
    x [B,Cin,H,H], w10 = both filter sets rearranged (functional._rearranged kind "s2p_f") -> (y3, y1), each [B,Cout,H/2,H/2]"""
    B, Cin, H = x.shape[0], x.shape[1], x.shape[2]
    y3 = torch.empty((B, cout, H // 2, H // 2), dtype=torch.float32, device=x.device)
    y1 = torch.empty_like(y3)
    N.check(N.lib.ee_conv3x3s2_pair_fwd_f32(_chk(x, torch.float32, "x", (B, Cin, H, H)), _chk(w10, torch.float32, "w10", (cout // 32, Cin // 16, 10, 4, 2, 16, 4)),
                                            y3.data_ptr(), y1.data_ptr(), B, Cin, cout, H, _stream()), "ee_conv3x3s2_pair_fwd_f32")
    return y3, y1


def conv3x3s2_pair_bwd_data(dy3, dy1, w10, cin):
    """dx = conv3x3s2^T(dy3) + conv1x1s2^T(dy1): dy3, dy1 [B,Cout,H/2,H/2], w10 (kind "s2p_b") -> dx [B,Cin,H,H]"""
    B, Cout, OH = dy3.shape[0], dy3.shape[1], dy3.shape[2]
    dx = torch.empty((B, cin, 2 * OH, 2 * OH), dtype=torch.float32, device=dy3.device)
    N.check(N.lib.ee_conv3x3s2_pair_bwd_data_f32(_chk(dy3, torch.float32, "dy3", (B, Cout, OH, OH)), _chk(dy1, torch.float32, "dy1", (B, Cout, OH, OH)),
                                                 _chk(w10, torch.float32, "w10", (cin // 32, Cout // 16, 10, 4, 2, 16, 4)), dx.data_ptr(), B, cin, Cout, 2 * OH,
                                                 _stream()), "ee_conv3x3s2_pair_bwd_data_f32")
    return dx


def stem7x7s2_bwd_data(dy, weight, H, W):
    """d loss / d image through Conv2d(3, K, 7, stride 2, padding 3) (resnet.py:112): dy [B,K,H/2,W/2] -> [B,3,H,W]."""
    B, K = dy.shape[0], dy.shape[1]
    dx = torch.empty((B, 3, H, W), dtype=torch.float32, device=dy.device)
    N.check(N.lib.ee_stem7x7s2_bwd_data_f32(_chk(dy, torch.float32, "dy", (B, K, H // 2, W // 2)),
                                            _chk(weight, torch.float32, "weight", (K, 3, 7, 7)), dx.data_ptr(), B, K, H, W, _stream()),
            "ee_stem7x7s2_bwd_data_f32")
    return dx


def stem7x7s2_fwd_supported(x, weight):
    return (x.dim() == 4 and x.shape[1] == 3 and x.shape[2] % 2 == 0 and x.shape[3] % 64 == 0 and weight.shape[0] % 64 == 0
            and tuple(weight.shape[1:]) == (3, 7, 7) and weight.data_ptr() % 16 == 0)


def stem7x7s2_fwd(x, weight, want_stats=False):
    """Conv2d(3, K, 7, stride 2, padding 3) forward (resnet.py:112): x [B,3,H,W] -> [B,K,H/2,W/2] on the f32 matrix cores.
    want_stats: also (y, stats [K,S,3]) - per channel and workgroup (sum, M2, count) of y for the BatchNorm that follows."""
    B, _, H, W = x.shape
    K = weight.shape[0]
    y = torch.empty((B, K, H // 2, W // 2), dtype=torch.float32, device=x.device)
    stats = None
    if want_stats:
        n = N.lib.ee_stem7x7s2_fwd_stats_floats(B, K, H, W)
        stats = torch.empty((K, n // (3 * K), 3), dtype=torch.float32, device=x.device)
    N.check(N.lib.ee_stem7x7s2_fwd_stats_f32(_chk(x, torch.float32, "x", (B, 3, H, W)), _chk(weight, torch.float32, "weight", (K, 3, 7, 7)),
                                             y.data_ptr(), None if stats is None else stats.data_ptr(), B, K, H, W, _stream()),
            "ee_stem7x7s2_fwd_stats_f32")
    return (y, stats) if want_stats else y


def pool_linear_fwd(feat, weight, bias):
    """logits = fc(global_avgpool(feat)) (resnet.py:157-160) -> (logits [B,K], pooled [B,C])."""
    B, C = feat.shape[0], feat.shape[1]
    HW = feat[0, 0].numel() if B else 1
    K = weight.shape[0]
    pooled = torch.empty((B, C), dtype=torch.float32, device=feat.device)
    logits = torch.empty((B, K), dtype=torch.float32, device=feat.device)
    pb = None if bias is None else _chk(bias, torch.float32, "bias", (K,))
    N.check(N.lib.ee_pool_linear_fwd_f32(_chk(feat, torch.float32, "feat"), _chk(weight, torch.float32, "weight", (K, C)), pb,
                                         _chk(pooled, torch.float32, "pooled"), _chk(logits, torch.float32, "logits"), B, C, HW, K, _stream()),
            "ee_pool_linear_fwd_f32")
    return logits, pooled


def pool_linear_bwd(dlogits, weight, feat_shape):
    B, C = feat_shape[0], feat_shape[1]
    HW = 1
    for d in feat_shape[2:]:
        HW *= d
    K = weight.shape[0]
    dfeat = torch.empty(feat_shape, dtype=torch.float32, device=dlogits.device)
    N.check(N.lib.ee_pool_linear_bwd_f32(_chk(dlogits, torch.float32, "dlogits", (B, K)), _chk(weight, torch.float32, "weight", (K, C)),
                                         _chk(dfeat, torch.float32, "dfeat"), B, C, HW, K, _stream()), "ee_pool_linear_bwd_f32")
    return dfeat


def ce_pool_linear_bwd(logits, labels, weight, feat_shape, reduction="sum"):
    """d CrossEntropyLoss(logits, labels) / d feat for logits = fc(global_avgpool(feat)): the loss gradient is formed inside the head's backward
    launch (ee_head.hip) - the bits of ce(...) followed by pool_linear_bwd(...), one launch less"""
    B, C = feat_shape[0], feat_shape[1]
    HW = 1
    for d in feat_shape[2:]:
        HW *= d
    K = weight.shape[0]
    dfeat = torch.empty(feat_shape, dtype=torch.float32, device=logits.device)
    N.check(N.lib.ee_ce_pool_linear_bwd_f32(_chk(logits, torch.float32, "logits", (B, K)), _chk(labels, torch.int64, "labels", (B,)),
                                            _inv(B) if reduction == "mean" else 1.0, _chk(weight, torch.float32, "weight", (K, C)),
                                            _chk(dfeat, torch.float32, "dfeat"), B, C, HW, K, _stream()), "ee_ce_pool_linear_bwd_f32")
    return dfeat


# ---- Net_2's convolutional half (MNIST) -------------------------------------------------------------------------------------------
def net2_conv_supported(x, w1, w2):
    return (x.dim() == 4 and tuple(x.shape[1:]) == (1, 28, 28) and tuple(w1.shape) == (32, 1, 5, 5) and tuple(w2.shape) == (64, 32, 5, 5)
            and x.data_ptr() % 16 == 0)


def net2_conv_fwd(x, w1, b1, w2, b2, drop=None, keep=1.0, draw_state=None):
    """a2 = relu(max_pool2d(drop * conv2(relu(max_pool2d(conv1(x), 2))), 2)) (MNIST/models_mnist/Net2.py:13-14), two launches.
    Returns (a2 [B,64,4,4], saved, drop) - `saved` = (a1, code1, code2) for net2_conv_bwd.  drop: Dropout2d's [B,64] Bernoulli(keep) draw (0 / 1) or None;
    the kernels scale by drop / keep (what noise.div_(1 - p) does).  drop None + draw_state (runtime.draw_state): the kernel draws the mask itself and
    the returned `drop` is what it drew."""
    B = x.shape[0]
    dev = x.device
    a1 = torch.empty((B, 32, 12, 12), dtype=torch.float32, device=dev)
    c1 = torch.empty((B, 32, 12, 12), dtype=torch.uint8, device=dev)
    a2 = torch.empty((B, 64, 4, 4), dtype=torch.float32, device=dev)
    c2 = torch.empty((B, 64, 4, 4), dtype=torch.uint8, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    rng = drop is None and draw_state is not None
    drop_out = torch.empty((B, 64), dtype=torch.float32, device=dev) if rng else None
    N.check(N.lib.ee_net2_conv_fwd_f32(_chk(x, torch.float32, "x", (B, 1, 28, 28)), _chk(w1, torch.float32, "w1", (32, 1, 5, 5)),
                                       None if b1 is None else _chk(b1, torch.float32, "b1", (32,)), _chk(w2, torch.float32, "w2", (64, 32, 5, 5)),
                                       None if b2 is None else _chk(b2, torch.float32, "b2", (64,)),
                                       None if drop is None else _chk(drop, torch.float32, "drop", (B, 64)), float(keep),
                                       _chk(draw_state, torch.int64, "draw_state", (4,)) if rng else None, ptr(drop_out), ptr(a1), ptr(c1), ptr(a2),
                                       ptr(c2), B, _stream()), "ee_net2_conv_fwd_f32")
    return a2, (a1, c1, c2), (drop_out if rng else drop)


def net2_conv_bwd(da2, a2, saved, w1, w2, drop=None, keep=1.0, da1_out=None, need_dx=True):
    """d loss / d x [B,1,28,28] of net2_conv_fwd (input gradient only), two launches; da1_out: keeps the gradient of a1 for net2_conv_wrw."""
    a1, c1, c2 = saved
    B = a2.shape[0]
    da1 = torch.empty_like(a1) if da1_out is None else da1_out
    dx = torch.empty((B, 1, 28, 28), dtype=torch.float32, device=a2.device) if need_dx else None
    N.check(N.lib.ee_net2_conv_bwd_f32(_chk(da2, torch.float32, "da2", (B, 64, 4, 4)), _chk(a2, torch.float32, "a2"), _chk(c2, torch.uint8, "code2"),
                                       None if drop is None else _chk(drop, torch.float32, "drop", (B, 64)), float(keep), _chk(w2, torch.float32, "w2"),
                                       _chk(a1, torch.float32, "a1"), _chk(c1, torch.uint8, "code1"), _chk(w1, torch.float32, "w1"),
                                       da1.data_ptr(), None if dx is None else dx.data_ptr(), B, _stream()), "ee_net2_conv_bwd_f32")
    return dx


def net2_conv_wrw(x, da2, a2, saved, da1, drop=None, keep=1.0):
    """(dw1 [32,1,5,5], db1 [32], dw2 [64,32,5,5], db2 [64]) of net2_conv_fwd - views of one buffer: two launches + the fixed-order sum over the
    groups of ten images (bit-reproducible).  da1 = the gradient of a1 (net2_conv_bwd's da1_out)."""
    a1, c1, c2 = saved
    B = a2.shape[0]
    out = torch.empty(64 * 32 * 25 + 32 * 25 + 64 + 32, dtype=torch.float32, device=a2.device)
    n = int(N.lib.ee_net2_conv_wrw_workspace_floats(B))
    ws = torch.empty(max(n, 4), dtype=torch.float32, device=a2.device)
    N.check(N.lib.ee_net2_conv_wrw_f32(_chk(x, torch.float32, "x", (B, 1, 28, 28)), _chk(a1, torch.float32, "a1", (B, 32, 12, 12)), _chk(c1, torch.uint8, "code1"),
                                       _chk(da1, torch.float32, "da1", (B, 32, 12, 12)), _chk(a2, torch.float32, "a2", (B, 64, 4, 4)), _chk(c2, torch.uint8, "code2"),
                                       _chk(da2, torch.float32, "da2", (B, 64, 4, 4)), None if drop is None else _chk(drop, torch.float32, "drop", (B, 64)),
                                       float(keep), out.data_ptr(), ws.data_ptr(), B, _stream()), "ee_net2_conv_wrw_f32")
    n2, n1 = 64 * 32 * 25, 32 * 25
    return out[n2:n2 + n1].view(32, 1, 5, 5), out[n2 + n1 + 64:], out[:n2].view(64, 32, 5, 5), out[n2 + n1:n2 + n1 + 64]


# ---- batch assembly from a device-resident dataset split (eeadv.data) -----------------------------------------------------
def batch_u8(data, labels, idx, flip, lut):
    """data [N,H,W,C] u8, labels [N] i64, idx [B] i32 sample ids, flip [N] u8 or None, lut [256] f32 ->
    (x [B,C,H,W] f32 = lut[data[idx]] mirrored where flip[idx], HWC -> NCHW;  y [B] i64 = labels[idx]).  One launch."""
    if data.dim() != 4:
        raise ValueError("data must be [N,H,W,C], got shape %s" % (tuple(data.shape),))
    n, H, W, C = data.shape
    B = idx.shape[0]
    pd = _chk(data, torch.uint8, "data")
    pl = _chk(labels, torch.int64, "labels", (n,))
    pi = _chk(idx, torch.int32, "idx", (B,))
    pf = _opt(flip, torch.uint8, "flip", (n,))
    pt = _chk(lut, torch.float32, "lut", (256,))
    out = torch.empty((B, C, H, W), dtype=torch.float32, device=data.device)
    y = torch.empty((B,), dtype=torch.int64, device=data.device)
    N.check(N.lib.ee_batch_u8_f32(pd, pl, pi, pf, pt, n, B, C, H, W, _chk(out, torch.float32, "out"), _chk(y, torch.int64, "labels_out"),
                                  _stream()), "ee_batch_u8_f32")
    return out, y


def batch_rrc(pixels, offsets, sizes, labels, idx, boxes, flip, lut, S):
    """pixels [bytes] u8 (images HWC, C = 3, back to back), offsets [N] i64, sizes [N,2] i32 = (H, W), labels [N] i64, idx [B] i32
    sample ids, boxes [N,4] i32 = (top, left, h, w), flip [N] u8 or None, lut [256] f32 ->
    (x [B,3,S,S] f32 = lut[PIL-BILINEAR resize of each sample's crop to S x S] mirrored where flip[idx];  y [B] i64).  One launch."""
    n, B, S = offsets.shape[0], idx.shape[0], int(S)
    if pixels.dim() != 1:
        raise ValueError("pixels must be one flat buffer, got shape %s" % (tuple(pixels.shape),))
    pp = _chk(pixels, torch.uint8, "pixels")
    po = _chk(offsets, torch.int64, "offsets", (n,))
    ps = _chk(sizes, torch.int32, "sizes", (n, 2))
    pl = _chk(labels, torch.int64, "labels", (n,))
    pi = _chk(idx, torch.int32, "idx", (B,))
    pb = _chk(boxes, torch.int32, "boxes", (n, 4))
    pf = _opt(flip, torch.uint8, "flip", (n,))
    pt = _chk(lut, torch.float32, "lut", (256,))
    out = torch.empty((B, 3, S, S), dtype=torch.float32, device=pixels.device)
    y = torch.empty((B,), dtype=torch.int64, device=pixels.device)
    N.check(N.lib.ee_batch_rrc_u8_f32(pp, pixels.numel(), po, ps, pl, pi, pb, pf, pt, n, B, S, _chk(out, torch.float32, "out"),
                                      _chk(y, torch.int64, "labels_out"), _stream()), "ee_batch_rrc_u8_f32")
    return out, y


def batch_aug(data, labels, idx, offs, flip, coef, lut, idx_host, offs_host, pad):
    """data [N,H,W,C] u8, labels [N] i64, lut [256] f32; per batch position idx [B] i32 sample ids, offs [B,2] i32 = (top, left) of the
    crop in the image zero-padded by `pad`, flip [B] u8 or None, coef [B,6] i32 (eeadv.data.aug_coeffs); idx_host / offs_host = the
    HOST tensors idx and offs were uploaded from, which the library checks before it launches ->
    (x [B,C,H,W] f32 = lut[rotate(flip(crop(pad(data[idx]))))], HWC -> NCHW;  y [B] i64 = labels[idx]).  One launch."""
    if data.dim() != 4:
        raise ValueError("data must be [N,H,W,C], got shape %s" % (tuple(data.shape),))
    n, H, W, C = data.shape
    B = idx.shape[0]
    pd = _chk(data, torch.uint8, "data")
    pl = _chk(labels, torch.int64, "labels", (n,))
    pi = _chk(idx, torch.int32, "idx", (B,))
    po = _chk(offs, torch.int32, "offs", (B, 2))
    pf = _opt(flip, torch.uint8, "flip", (B,))
    pc = _chk(coef, torch.int32, "coef", (B, 6))
    pt = _chk(lut, torch.float32, "lut", (256,))
    for t, name, shape in ((idx_host, "idx_host", (B,)), (offs_host, "offs_host", (B, 2))):
        if not isinstance(t, torch.Tensor) or t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous() or tuple(t.shape) != shape:
            raise ValueError("%s must be a contiguous int32 host tensor of shape %s" % (name, shape))
    out = torch.empty((B, C, H, W), dtype=torch.float32, device=data.device)
    y = torch.empty((B,), dtype=torch.int64, device=data.device)
    N.check(N.lib.ee_batch_aug_u8_f32(pd, pl, pi, po, pf, pc, pt, ctypes.c_void_p(idx_host.data_ptr()), ctypes.c_void_p(offs_host.data_ptr()),
                                      n, B, C, H, W, int(pad), _chk(out, torch.float32, "out"), _chk(y, torch.int64, "labels_out"), _stream()),
            "ee_batch_aug_u8_f32")
    return out, y


# ---- timing hooks ------------------------------------------------------------------------------------------------------
def prof_enable(on=True):
    N.check(N.lib.ee_prof_enable(1 if on else 0), "ee_prof_enable")


def prof_mark_empty():
    N.check(N.lib.ee_prof_mark_empty(_stream()), "ee_prof_mark_empty")


def prof_reset():
    N.check(N.lib.ee_prof_reset(), "ee_prof_reset")


def prof_read(kernel_id):
    ms, cnt = ctypes.c_double(0.0), ctypes.c_int64(0)
    N.check(N.lib.ee_prof_read(kernel_id, ctypes.byref(ms), ctypes.byref(cnt)), "ee_prof_read")
    return ms.value, cnt.value


def prof_read_work(kernel_id):
    """Floating-point operations the timed launches of a matrix-core family declared (0 for the HBM-bound families)."""
    w = ctypes.c_double(0.0)
    N.check(N.lib.ee_prof_read_work(kernel_id, ctypes.byref(w)), "ee_prof_read_work")
    return w.value
