"""GPU: every entry point of the edge front end (csrc/ee_edge.hip, csrc/ee_canny.hip) against what it returned on the commit before its
kernels were folded onto the shared helpers of csrc/ee_stencil.hpp - tests/golden/edge_parent.npz, recorded there by
tests/golden/make_edge_parent_golden.py, whose inputs and calls this test repeats.

Bit for bit, float outputs as int32 and gates as uint8 (arrays of more than 2048 elements by their SHA-256): the twelve ops wrappers over
the ten entry points, at one shape per tile edge - 32- and 64-wide tiles on the vector and on the scalar path, partial last tiles down
and across, C = 1 .. 4, one-row and one-pixel images, and 16x32 with every tensor one element into its storage (W % 4 == 0 without the
16-byte accesses).  (176, 2, 40, 68) is the one shape on the backward's 16-row route (1056 workgroups): SHA-256 against the record, and
its first two images against the same two run as a batch of 2 on the 11-row route - the tile height changes no bit, on the recorded
commit either (`big_rows_equal`)."""
import functools
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def _make():
    spec = importlib.util.spec_from_file_location("make_edge_parent_golden", os.path.join(HERE, "golden", "make_edge_parent_golden.py"))
    make = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make)
    return make


@functools.lru_cache(maxsize=None)
def _recorded():
    make = _make()
    want = dict(np.load(os.path.join(HERE, "golden", "edge_parent.npz")))
    assert str(want["commit"]).startswith("df24c3b")  # the record names the commit it was taken on: the parent of the fold
    return make, want


def test_fixture_reaches_what_it_should():
    """No device needed.  What the record itself shows per shape: both edge values and both gate values; s = x_hfs + w * edge exactly on 0
    and exactly on 1; in every g_img at least one NaN (the flat 7x7 block) and one finite non-zero.  The 7x7 block needs a 9x9 image to
    leave anything finite, so the gradient counts are asked of those; the one-row and one-pixel images are there for the fold rows.
    The counts are the recorder's (`reach_*`); here they are recomputed only where the record holds the arrays raw, and the GPU test below
    recomputes them from its own outputs for every shape."""
    make, want = _recorded()
    assert bool(want["big_rows_equal"])
    for shape, offset in make.CASES:
        k = make.key(shape, offset)
        got = dict(zip(make.REACH, want["reach_" + k].tolist()))
        if shape[2] >= 9 and shape[3] >= 9:
            assert all(v > 0 for v in got.values()), (k, got)
        # the counts are those of the arrays the record holds raw
        raw = {n: want[k + "/" + n] for n in ("frontend_fwd.gate", "frontend_fwd.x_in") + make.G_IMG}
        if all(a.ndim == 4 for a in raw.values()):
            gate, x_in = raw["frontend_fwd.gate"], raw["frontend_fwd.x_in"].view(np.float32)
            assert ((gate == 1) & (x_in == 0)).sum() == got["s_is_0"] and ((gate == 1) & (x_in == 1)).sum() == got["s_is_1"]
            assert (gate == 0).sum() == got["gate0"] and (gate == 1).sum() == got["gate1"]
            for n in make.G_IMG:
                assert np.isnan(raw[n].view(np.float32)).sum() == got[n + ":nan"]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,offset", [pytest.param(s, o, id=_make().key(s, o)) for s, o in _make().CASES])  # the recorder's own list
def test_every_entry_point_equals_the_parent(shape, offset):
    import torch
    from eeadv import ops

    make, want = _recorded()
    got = make.run(torch, ops, shape, offset)  # integer formulas: the same floats as on the day of the record
    k = make.key(shape, offset)
    assert sorted(k + "/" + n for n in got) == sorted(n for n in want if n.startswith(k + "/"))
    for n, a in got.items():
        assert np.array_equal(make.pack(a), want[k + "/" + n]), (k, n)
    assert np.array_equal(make.reach(got), want["reach_" + k])


@pytest.mark.gpu
def test_sixteen_row_backward_equals_the_parent_and_the_eleven_row_route():
    import torch
    from eeadv import ops

    make, want = _recorded()
    B, _, H, W = make.BIG
    assert B * ((H + 15) // 16) * ((W + 63) // 64) >= 1024 > 2 * ((H + 15) // 16) * ((W + 63) // 64)  # plan()'s switch lies between the two
    big, two = make.run_big(torch, ops), make.run_big(torch, ops, 2)
    for n, a in big.items():
        assert np.array_equal(make.sha(a), want["big/" + n]), n
        assert np.array_equal(a[:2], two[n]), n  # the tile height changes no bit
