"""GPU: the two matrix-core low-pass entry points (ee_hfs_mfma_f32, ee_hfs_wide_f32) against what they returned on the commit before
the two kernels of csrc/ee_hfs_mfma.hip were folded into one - tests/golden/hfs_band_parent.npz, recorded there by
tests/golden/make_hfs_band_golden.py, whose inputs and calls this test repeats.

Bit for bit, as int32.  B = 2; per shape the plain operator, sq_mode 1 and sq_mode 2 (three Add_Square queries), each also with the
input one float into its storage.  The shapes are the smallest at which each path differs: one band with a partial strip and
W % 4 != 0; four bands and a partial second strip; MT2 = 4; sixteen wavefronts; and, on the wide entry point, 17 bands with a
wavefront that owns one, and MT2 = 6 with NT = 4."""
import functools
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def _recorded():
    spec = importlib.util.spec_from_file_location("make_hfs_band_golden", os.path.join(HERE, "golden", "make_hfs_band_golden.py"))
    make = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make)
    want = dict(np.load(os.path.join(HERE, "golden", "hfs_band_parent.npz")))
    assert str(want["commit"]).startswith("ebe16fb")  # the record names the commit it was taken on: the parent of the fold
    return make, want


def test_record_and_pads():
    """No device needed: the record holds every case in every mode, and today's table builders give the pads the cases name."""
    from eeadv import hfs as HF
    make, want = _recorded()
    assert [c[:4] for c in make.CASES] == [("narrow", 7, 9, 2), ("narrow", 50, 70, 6), ("narrow", 48, 40, 12), ("narrow", 256, 20, 4),
                                           ("wide", 260, 40, 3), ("wide", 40, 48, 18)]
    assert [c[4] for c in make.CASES] == [(16,), (16,), (32,), (16,), (16, 16), (48, 32)]
    for case in make.CASES:
        make.tables(HF, case)  # asserts the pads
        for mode in make.MODES:
            y = want[make.key(case, mode)]
            assert y.dtype == np.int32 and y.shape == (make.B, make.C) + case[1:3]


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(6))
def test_band_kernel_equals_the_parent(case):
    import torch
    from eeadv import hfs as HF, ops

    make, want = _recorded()
    case = make.CASES[case]
    for mode in make.MODES:
        for offset in (False, True):
            got = make.run(torch, ops, HF, case, mode, offset)
            assert np.array_equal(got, want[make.key(case, mode)]), (case, mode, offset)
