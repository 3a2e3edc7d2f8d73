#!/usr/bin/env python3
"""Records what the two matrix-core low-pass entry points (ee_hfs_mfma_f32, ee_hfs_wide_f32) return on fixed inputs, on a ROCm device:

    python tests/golden/make_hfs_band_golden.py [ROOT] [OUT] [COMMIT]

ROOT: the checkout whose package is imported (default: this one); OUT: the .npz (default tests/golden/hfs_band_parent.npz next to this
file); COMMIT: the hash of ROOT's commit, kept in the record as `commit` (default: asked of git in ROOT, empty if that fails).
tests/golden/hfs_band_parent.npz was recorded on the commit before the two kernels of csrc/ee_hfs_mfma.hip were folded into one;
tests/test_gpu_hfs_band_parent.py holds the same calls of the current code to it bit for bit.

The inputs and the Add_Square draws are integer formulas (images and gradients on the k / 255 grid), so the record does not hold them.
B = 2, C = 1.  The planes go to ops.hfs_mfma / ops.hfs_wide directly, with tables from band_tables / wide_tables, so that small planes
reach the wide class; per shape the plain operator, sq_mode 1 and sq_mode 2, each also with the input one float past a 16-byte
boundary (the element-wise loads)."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
B, C, EPS = 2, 1, 16.0 / 255.0
# (class, H, W, r, pads): the smallest planes at which each path of the kernel differs
CASES = (("narrow", 7, 9, 2, (16,)),        # one band, one partial strip, MT2 = 2, W % 4 != 0
         ("narrow", 50, 70, 6, (16,)),      # four bands, two strips with a partial second one, MT2 = 2
         ("narrow", 48, 40, 12, (32,)),     # NU = 24: MT2 = 4
         ("narrow", 256, 20, 4, (16,)),     # sixteen wavefronts: the launch bound
         ("wide", 260, 40, 3, (16, 16)),    # 17 bands, the last wavefront owns one; MT2 = 2, NT = 2
         ("wide", 40, 48, 18, (48, 32)))    # NU = 36, NV = 18: MT2 = 6, NT = 4; three bands on two wavefronts
MODES = (0, 1, 2)


def key(case, mode):
    return "%s_%dx%d_r%d_sq%d" % (case[:4] + (mode,))


def inputs(H, W):
    """(x, g): an image and a gradient, [B, C, H, W] float32 on the k / 255 grid."""
    b, h, w = np.arange(B, dtype=np.int64)[:, None, None, None], np.arange(H, dtype=np.int64)[:, None], np.arange(W, dtype=np.int64)[None, :]
    x = ((h * 37 + w * 101 + b * 53 + 60) % 256 + np.zeros((B, C, 1, 1), np.int64)).astype(F32) / F32(255)
    g = ((h * 91 + w * 29 + b * 7 + 3) % 256 - 128 + np.zeros((B, C, 1, 1), np.int64)).astype(F32) / F32(255)
    return x, g


def draws(H, W):
    """Add_Square's draws for three queries (one more than the kernel keeps in registers): stripe [B,C,1,W], sq_sign [3,C], sq_pos [3]
    int64, sq_size [3] int32."""
    b, w = np.arange(B, dtype=np.int64)[:, None, None, None], np.arange(W, dtype=np.int64)
    stripe = np.where((3 * w + b) % 5 < 2, F32(1), F32(-1)).astype(F32) + np.zeros((B, C, 1, 1), F32)
    sq_sign = np.array([[1.0], [-1.0], [1.0]], dtype=F32)
    sq_pos = np.array([1, 0, 2], dtype=np.int64)
    sq_size = np.array([min(H, W) // 2 + 1, 3, 1], dtype=np.int32)
    return stripe, sq_sign, sq_pos, sq_size


def tables(HF, case):
    """The case's table and pads from the tree under test; the pads are what CASES says they are."""
    cls, H, W, r, pads = case
    got = HF.band_tables(H, W, r) if cls == "narrow" else HF.wide_tables(H, W, r)
    assert tuple(got[1:]) == pads, (case, got[1:])
    return got


def odd(torch, t):
    """The same values 4 bytes past a 16-byte boundary."""
    pad = torch.zeros(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = pad[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def run(torch, ops, HF, case, mode, offset):
    """One launch; the result as int32 [B, C, H, W]."""
    cls, H, W, r, pads = case
    dev = "cuda:0"
    flat = tables(HF, case)[0]
    x, g = (torch.from_numpy(a).to(dev) for a in inputs(H, W))
    src = g if mode == 2 else x
    src = odd(torch, src) if offset else src
    sq = () if mode == 0 else (mode, x if mode == 2 else None, EPS) + tuple(torch.from_numpy(a).to(dev) for a in draws(H, W))
    fn = ops.hfs_mfma if cls == "narrow" else ops.hfs_wide
    return fn(src, torch.from_numpy(flat).to(dev), *pads, *sq).cpu().numpy().view(np.int32)


def main():
    root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(HERE))
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "hfs_band_parent.npz")
    sys.path[:0] = [os.path.join(root, "edge-enhancement_amd")]
    import torch
    from eeadv import hfs as HF, ops
    if len(sys.argv) > 3:
        commit = sys.argv[3]
    else:
        got = subprocess.run(["git", "-C", root, "rev-parse", "HEAD"], capture_output=True, text=True)
        commit = got.stdout.strip() if got.returncode == 0 else ""
    arrays = {"commit": np.array(commit)}
    for case in CASES:
        for mode in MODES:
            y = run(torch, ops, HF, case, mode, False)
            assert np.array_equal(y, run(torch, ops, HF, case, mode, True)), (case, mode)  # the access widths agree on the recorded commit
            assert np.isfinite(y.view(F32)).all() and np.abs(y.view(F32)).max() > 0
            arrays[key(case, mode)] = y
            print(key(case, mode), y.shape, float(np.abs(y.view(F32)).max()), flush=True)
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
