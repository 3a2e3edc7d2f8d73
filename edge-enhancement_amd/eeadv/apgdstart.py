"""Host-side pieces of the APGD restarts (csrc/ee_apgd_start.hip, ee_apgd_start_f32), on top of eeadv/fabstart.py:
the draws of a restart's start point restated with the numpy Philox - same key, counters and stream id as the kernel - and the start point
itself in torch ops for the plain-torch host paths of utils/attacks.py.  The key of one start is fabstart.seed_of(seed, target_index,
restart); the stream id keeps APGD's draws apart from FAB's under the same key."""
import torch

from . import fabstart
from .fabstart import METRICS, seed_of  # noqa: F401  (one key function for both attacks)

STREAM_APGD_START = 16  # kStreamApgdStart of ee_common.hpp


def draw(seed, B, D, metric):
    """t, float32 [B, D]: the draw ee_apgd_start_f32 makes for rows 0 .. B-1 under the key `seed` - fabstart.draw on stream 16.  'Linf':
    uniform on [-1, 1), bit-identical to the kernel; 'L2' / 'L1': standard normals, the kernel's up to the rounding of its float math."""
    return fabstart.draw(seed, B, D, metric, STREAM_APGD_START)


def start(x0, eps, t, metric):
    """The start point of a restart in torch ops, in x0's dtype, one rounding per operation in the kernel's order; t has x0's shape.
    'Linf': clamp(x0 + eps t, 0, 1).  'L2': clamp(x0 + t * (eps / (n + 1e-12)), 0, 1), n the root of the squares summed in float64, cast
    once (utils.attacks._l2_start's order; 1e-12 a float32 constant in every dtype); a row whose n is not finite stays at x0.  'L1':
    x0 + t, unclamped - the run projects it."""
    if metric not in METRICS:
        raise ValueError("APGD metric must be one of %s, got %r" % (list(METRICS), metric))
    t = t.to(device=x0.device, dtype=x0.dtype)
    if metric == "Linf":
        return torch.clamp(x0 + torch.tensor(eps, dtype=x0.dtype) * t, 0, 1)
    if metric == "L1":
        return x0 + t
    shape = (-1,) + (1,) * (x0.dim() - 1)
    n = fabstart.row_norms(t.reshape(t.shape[0], -1), "L2")
    tiny = torch.tensor(1e-12, dtype=torch.float32).to(x0.dtype)
    s = torch.tensor(eps, dtype=x0.dtype) / (n + tiny)
    return torch.where(torch.isfinite(n).view(shape), torch.clamp(x0 + t * s.view(shape), 0, 1), x0)
