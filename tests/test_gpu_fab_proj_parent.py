"""GPU: the three FAB projection entry points against what they returned on the commit before their kernels were folded onto one
scaffold - tests/golden/fab_proj_parent.npz, recorded there by tests/golden/make_fab_proj_golden.py, whose inputs and calls this test
repeats.

Bit for bit: the projection scalars as int32, then x, adv (by their SHA-256), res, flags and pred after the step and the commit that the
scalars feed.  B = 2; per-sample sizes 1, 3, 12288 (the last resident one), 12289 and 12292 (streaming, without and with vectors); both
paths where both exist; every size also with x, x0 and w one float into their storage (the element-wise instantiation).  The five
launches of a size reach each early exit (df 0, NaN, +inf; an all-zero w row; x0 on the hyperplane), the infeasible answer (df huge),
a tiny df, x == x0, and L1's ties (|w| has two values) with phi inside (0, 1); one |w_i| is denormal for L2's breakpoint."""
import functools
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def _recorded():
    spec = importlib.util.spec_from_file_location("make_fab_proj_golden", os.path.join(HERE, "golden", "make_fab_proj_golden.py"))
    make = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make)
    want = dict(np.load(os.path.join(HERE, "golden", "fab_proj_parent.npz")))
    assert str(want["commit"]).startswith("817f53f")  # the record names the commit it was taken on: the parent of the fold
    return make, want


def test_fixture_reaches_every_exit():
    """No device needed.  What the record itself shows, per metric and size: a resting sample (sign 0), a point on the hyperplane (sign 1 and norm 0: lambda
    = 0, theta = +inf), an infeasible problem (lambda = +inf, theta = 0 with phi = 1), and an L1 fraction strictly inside (0, 1)."""
    make, want = _recorded()
    for metric in make.METRICS:
        scal = want["scal_" + metric].view(np.float32)  # [size, batch, rows, 2B]
        head, sign, norm = scal[:, :, 0], scal[:, :, 1], scal[:, :, 2]
        assert (sign == 0).any(axis=(1, 2)).all() and not np.isnan(scal).any()
        on_plane = (sign == 1) & (norm == 0) & (np.isinf(head) if metric == "L1" else head == 0)
        infeasible = (sign != 0) & ((head == 0) & (scal[:, :, 3] == 1) if metric == "L1" else np.isinf(head))
        assert on_plane.any(axis=(1, 2)).all() and infeasible.any(axis=(1, 2)).all()
        if metric == "L1":
            phi = scal[:, :, 3]
            assert ((phi > 0) & (phi < 1)).any(axis=(1, 2))[2:].all()  # from 12288 elements on: a tier of equal |w_i| shares what is left


@pytest.mark.gpu
@pytest.mark.parametrize("metric", ["Linf", "L2", "L1"])
@pytest.mark.parametrize("D", [1, 3, 12288, 12289, 12292])
def test_projection_step_commit_equal_the_parent(D, metric):
    import torch
    from eeadv import ops

    make, want = _recorded()
    i = make.SIZES.index(D)
    x, x0, w = make.inputs(D)  # integer formulas: the same floats as on the day of the record
    for k, (name, bx, b0, bw, df) in enumerate(make.batches(D, x, x0, w)):
        assert np.array_equal(df, want["df"][i, k], equal_nan=True)
        for path, offset in make.variants(D):
            got = make.run(torch, ops, metric, k, bx, b0, bw, df, path, offset)
            for f in make.FIELDS:
                assert np.array_equal(got[f], want["%s_%s" % (f, metric)][i, k]), (name, path, offset, f, got[f], want["%s_%s" % (f, metric)][i, k])
