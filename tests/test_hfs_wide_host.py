"""CPU: the wide low-pass kernel's host side (ee_hfs_wide_f32, planes past the band kernel's 256 x 256 up to 320 x 320) - the
fragment-ordered tables against the dense operator in float64 through the lane-level emulation (scripts/chain_emulate.py), their
size against the C query, the limits of the shape class and the order of the entry point's argument checks (nothing is launched)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SHAPES = [(288, 288, 18), (260, 40, 3), (33, 262, 5), (289, 291, 18), (272, 304, 20), (320, 320, 24)]  # (H, W, r)


@pytest.fixture(scope="module")
def native():
    import eeadv._native as n
    return n


@pytest.mark.parametrize("H,W,r", SHAPES)
def test_wide_table_layout_against_the_dense_operator_in_float64(H, W, r):
    """wide_apply emulates hfs_wide_kernel lane by lane (two bands per wavefront, the reduction in wavefront order); the bar is
    chain_emulate's own."""
    import chain_emulate as E
    from eeadv import hfs as HF
    x = np.random.RandomState(H + W + r).rand(H, W)
    Ar, Ai, B1, B2 = HF.hfs_matrices(H, W, r)
    want = Ar @ x @ B1 + Ai @ x @ B2
    T = E.wide_tables(H, W, r)
    assert np.abs(E.wide_apply(x, T) - want).max() < 1e-11
    # eeadv.hfs.wide_tables is that table, flattened and cast
    flat, nu_pad, nv_pad = HF.wide_tables(H, W, r)
    assert (2 * nu_pad // 16, 2 * nv_pad // 16) == (T["MT2"], T["NT"])
    spec = np.concatenate([T[k].reshape(-1) for k in ("t1", "t2", "t3", "t4")]).astype(np.float32)
    assert flat.dtype == np.float32 and np.array_equal(flat, spec)


@pytest.mark.parametrize("H,W,r", SHAPES)
def test_wide_table_size_matches_the_c_query(native, H, W, r):
    from eeadv import hfs as HF
    flat, nu_pad, nv_pad = HF.wide_tables(H, W, r)
    assert len(flat) == native.lib.ee_hfs_wide_table_floats(H, W, nu_pad, nv_pad)


def test_wide_pads_at_the_required_shape():
    from eeadv import hfs as HF
    _, nu_pad, nv_pad = HF.wide_tables(288, 288, 18)  # 36 kept row, 18 kept column frequencies
    assert (nu_pad, nv_pad) == (48, 32)
    assert HF.wide_tables(260, 40, 3)[1:] == (16, 16) and HF.wide_tables(320, 320, 24)[1:] == (48, 32)


def test_wide_tables_limits():
    from eeadv import hfs as HF
    def counts(H, W, r):
        return len(HF.keep_set(H, r)), len([v for v in HF.keep_set(W, r) if v <= W // 2])
    assert counts(320, 320, 24) == (48, 24)
    HF.wide_tables(320, 320, 24)           # the class limit on both sizes and on NU
    with pytest.raises(ValueError):
        HF.wide_tables(321, 320, 16)
    with pytest.raises(ValueError):
        HF.wide_tables(320, 321, 16)
    assert counts(319, 64, 24) == (49, 24)  # odd H keeps -24 .. 24
    with pytest.raises(ValueError):
        HF.wide_tables(319, 64, 24)
    assert counts(16, 320, 32) == (16, 32)  # a 16-row plane keeps every row frequency; even W keeps 0 .. 31
    assert HF.wide_tables(16, 320, 32)[1:] == (16, 32)
    assert counts(16, 319, 32) == (16, 33)  # odd W keeps 0 .. 32
    with pytest.raises(ValueError):
        HF.wide_tables(16, 319, 32)


def test_band_tables_class_is_untouched():
    from eeadv import hfs as HF
    with pytest.raises(ValueError):
        HF.band_tables(288, 288, 18)
    flat, nu_pad = HF.band_tables(224, 224, 16)
    assert nu_pad == 32


def test_wide_entry_points_are_bound(native):
    assert "ee_hfs_wide_table_floats" in native.SIGNATURES and "ee_hfs_wide_f32" in native.SIGNATURES


def test_wide_argument_checks_happen_before_any_launch(native):
    L = native.lib
    q, t = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    OK, NULL, SHAPE, UNSUPPORTED, ALIGN = 0, -1, -2, -3, -4

    def call(in_=q, out=q, B=2, C=3, H=288, W=288, tables=t, nu_pad=48, nv_pad=32, sq_mode=0, sq_x=None, stripe=None, sign=None, pos=None,
             size=None, nq=0):
        return L.ee_hfs_wide_f32(in_, out, B, C, H, W, tables, nu_pad, nv_pad, sq_mode, sq_x, 0.1, stripe, sign, pos, size, nq, None)
    # EE_ERR_SHAPE: non-positive sizes, a pad outside its set, a mode outside 0 .. 2
    assert call(B=-1) == SHAPE and call(C=0) == SHAPE and call(H=0) == SHAPE and call(W=-3) == SHAPE
    assert call(nu_pad=64) == SHAPE and call(nu_pad=0) == SHAPE and call(nv_pad=48) == SHAPE and call(nv_pad=8) == SHAPE
    assert call(sq_mode=3) == SHAPE and call(nq=-1) == SHAPE
    assert call(H=321, nu_pad=20) == SHAPE           # the pad is checked before the size limit
    # EE_ERR_UNSUPPORTED past 320
    assert call(H=321) == UNSUPPORTED and call(W=321) == UNSUPPORTED and call(H=321, in_=None) == UNSUPPORTED
    # an empty batch is fine, before any pointer check
    assert call(B=0, in_=None, out=None, tables=None) == OK
    assert call(B=0, H=321) == UNSUPPORTED
    # EE_ERR_NULL
    assert call(in_=None) == NULL and call(out=None) == NULL and call(tables=None) == NULL
    assert call(sq_mode=1) == NULL and call(sq_mode=1, stripe=q, nq=1) == NULL
    assert call(sq_mode=2, stripe=q, sign=q, pos=q, size=q, nq=1) == NULL   # sq_x
    assert call(tables=None, H=0) == SHAPE
    # EE_ERR_ALIGN: the table is read as float4
    assert call(tables=ctypes.c_void_p(8196)) == ALIGN and call(tables=ctypes.c_void_p(8200)) == ALIGN
    assert call(tables=ctypes.c_void_p(8196), in_=None) == NULL  # pointers before alignment
    # the size query follows the same order
    assert L.ee_hfs_wide_table_floats(0, 288, 48, 32) == SHAPE and L.ee_hfs_wide_table_floats(288, 288, 40, 32) == SHAPE
    assert L.ee_hfs_wide_table_floats(288, 288, 48, 24) == SHAPE and L.ee_hfs_wide_table_floats(321, 288, 48, 32) == UNSUPPORTED
    hp = wp = 288
    assert L.ee_hfs_wide_table_floats(288, 288, 48, 32) == (wp // 4 * 4 + 2 * (hp // 16) * 6 * 4 + (wp // 16) * 4 * 4) * 64
    # the band kernel's entry point keeps its contract
    assert L.ee_hfs_mfma_f32(q, q, 2, 3, 288, 288, t, 32, 0, None, 0.1, None, None, None, None, 0, None) == UNSUPPORTED
    assert L.ee_hfs_mfma_table_floats(288, 288, 32) == SHAPE
    assert L.ee_hfs_mfma_table_floats(224, 224, 32) == (224 // 4 * 2 + 2 * 14 * 4 * 4 + 14 * 8) * 64
