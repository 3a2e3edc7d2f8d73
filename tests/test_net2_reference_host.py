"""tests/net2_reference.py checked on its own (CPU): the float64 reference that tests/test_gpu_net2.py holds ee_net2.hip's kernels to.

  free forward   forward64 against F.conv2d / F.max_pool2d(return_indices=True) / F.relu in float64: values to 1e-12, indices EQUAL,
                 exact ties, NaN and inf included - which pins "the first maximum wins, a NaN always wins" to ATen's CPU kernel;
  replay         replay64 fed forward64's own branch against autograd through the stock float64 sequence, at 1e-12;
  shares         how many windows the GPU test may leave out of its code assertion, on every case it runs (the caps are conditions)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import net2_reference as R


def _unwindows(v4):
    B, C, h, w, _ = v4.shape
    return v4.reshape(B, C, h, w, 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, C, 2 * h, 2 * w)


def _code_of_index(idx, W):
    """ATen's flat index h * W + w of the winner -> the window code 2 dy + dx"""
    return (2 * ((idx // W) % 2) + (idx % W) % 2).astype(np.uint8)


def _inputs(name):
    c = dict(R.BASE, B=3, start=R.EPS if name == "start" else None)
    x, params, drop, keep = R.make_case(c)
    if name == "poisoned":
        x = x.copy()
        x[0, 0, 9, 4], x[0, 0, 9, 22], x[2, 0, 15, 10] = np.nan, np.inf, -np.inf
    return x, params, drop, keep


@pytest.mark.parametrize("name", ["clean", "start", "poisoned"])
def test_forward64_is_atens_cpu_sequence(name):
    """Values within 1e-12 of F.conv2d's (relative to the largest), the same NaN / inf footprint; on forward64's OWN pre-pool maps
    F.max_pool2d returns the same winners in every window - the flat patches' four-way ties, the ties at +-0 of dropped channels and
    the NaN / +inf windows included - and F.relu the same output."""
    x, params, drop, keep = _inputs(name)
    f = R.forward64(x, params, drop, keep)
    w1, b1, w2, b2 = (t.double() for t in params)
    z1 = F.conv2d(torch.from_numpy(x).double(), w1, b1)
    mine1 = _unwindows(f["v1"])
    fin = np.isfinite(mine1)
    assert np.array_equal(np.isnan(mine1), np.isnan(z1.numpy())) and np.array_equal(fin, np.isfinite(z1.numpy()))
    assert np.array_equal(mine1[~fin & ~np.isnan(mine1)], z1.numpy()[~fin & ~np.isnan(mine1)])
    assert np.abs(mine1[fin] - z1.numpy()[fin]).max() <= 1e-12 * np.abs(mine1[fin]).max()
    for v4, code, a, Wd in ((f["v1"], f["code1"], f["a1"], 24), (f["v2"], f["code2"], f["a2"], 8)):
        z = torch.from_numpy(_unwindows(v4))
        best, idx = F.max_pool2d(z, 2, return_indices=True)
        assert np.array_equal(_code_of_index(idx.numpy(), Wd), code)
        assert np.array_equal(F.relu(best).numpy(), a, equal_nan=True)
    ties1 = (f["v1"] == f["v1"].max(-1, keepdims=True)).sum(-1)
    assert (ties1 == 4).mean() > 0.2 or name != "clean"
    if name == "poisoned":
        assert np.isnan(f["v1"]).any() and np.isposinf(f["v1"]).any() and np.isnan(f["a2"]).any()
    # conv2 on the float64 a1, against the stock sequence end to end (finite inputs: the winners of both pools agree as well)
    if name != "poisoned":
        s = R.scale64(drop, keep)
        z2 = F.conv2d(F.relu(F.max_pool2d(z1, 2)), w2, b2) * torch.from_numpy(s)[:, :, None, None]
        mine2 = _unwindows(f["v2"])
        assert np.abs(mine2 - z2.numpy()).max() <= 1e-12 * np.abs(mine2).max()


@pytest.mark.parametrize("name", ["clean", "start"])
def test_replay64_on_forward64s_branch_is_autograd_through_the_stock_sequence(name):
    """replay64 with forward64's codes and gates (the value passes unless it is <= 0): outputs and the six gradients of <a2, da2> within
    1e-12 (relative to each tensor's largest entry) of autograd through F.conv2d / F.max_pool2d / F.relu in float64."""
    x, params, drop, keep = _inputs(name)
    f = R.forward64(x, params, drop, keep)
    rep = R.replay64(x, params, drop, keep, f["code1"], f["code2"], ~(f["a1"] <= 0), ~(f["a2"] <= 0))
    da2 = torch.randn(3, 64, 4, 4, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    mine = R.replay_gradients(rep, da2)
    xs = torch.from_numpy(x).double().requires_grad_(True)
    ps = [t.double().requires_grad_(True) for t in params]
    a1 = F.relu(F.max_pool2d(F.conv2d(xs, ps[0], ps[1]), 2))
    a2 = F.relu(F.max_pool2d(F.conv2d(a1, ps[2], ps[3]) * torch.from_numpy(R.scale64(drop, keep))[:, :, None, None], 2))
    ref = torch.autograd.grad(a2, [xs, a1] + ps, da2)
    assert float((rep["a2"] - a2).detach().abs().max()) <= 1e-12 * float(a2.detach().abs().max())
    assert np.abs(f["a2"] - a2.detach().numpy()).max() <= 1e-12 * float(a2.detach().abs().max())
    for name_, m, r in zip(("dx", "da1", "dw1", "db1", "dw2", "db2"), mine, ref):
        assert float(r.abs().max()) > 0 and float((m - r).abs().max()) <= 1e-12 * float(r.abs().max()), name_


def test_bound32_covers_an_fp32_evaluation():
    """the derived bound against one fp32 evaluation of the same chains (torch CPU float32): every pre-pool value inside it - a sanity
    check of the formula, not where it comes from"""
    x, params, drop, keep = _inputs("start")
    f = R.forward64(x, params, drop, keep)
    w1, b1, w2, b2 = params
    z1 = R.windows(F.conv2d(torch.from_numpy(x), w1, b1).numpy().astype(np.float64))
    assert (np.abs(z1 - f["v1"]) <= R.bound32(x, w1, b1, R.K1)).all()
    a1 = f["a1"].astype(np.float32)
    f2 = R.forward64(x, params, drop, keep, a1_in=a1)
    s = R.scale64(drop, keep)
    z2 = R.windows((F.conv2d(torch.from_numpy(a1), w2, b2) * torch.from_numpy(s.astype(np.float32))[:, :, None, None]).numpy().astype(np.float64))
    assert (np.abs(z2 - f2["v2"]) <= R.bound32(a1, w2, b2, R.K2, s)).all()


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_excluded_share_stays_under_the_cap(case):
    """The GPU test asserts the kernels' pool winners on decided and exact-tie windows only.  With the float64 forward rounded to float32
    standing in for the kernel, every case it runs must have at least 25 % exact-tie windows in conv1, at least 2 % in conv2, and at most
    2 % undecided windows in either layer (conditions, not measurements: a case that misses them gets another generator or seed).
    Measured (exact-tie share / undecided share; conv2's exact ties include the windows of dropped channels):
                                   conv1               conv2
        B11-clean-hard-drop        62.36 % / 0.00 %    67.52 % / 0.12 %
        B1-clean-hard-drop         53.93 % / 0.00 %    58.98 % / 0.00 %
        B3-clean-hard-drop         84.06 % / 0.00 %    85.87 % / 0.07 %
        B23-clean-hard-drop        60.77 % / 0.00 %    68.68 % / 0.19 %
        B11-start-hard-drop        39.66 % / 0.01 %    53.60 % / 0.65 %
        B11-clean-seeded-drop      62.36 % / 0.00 %    67.52 % / 0.10 %
        B11-clean-hard-nodrop      62.36 % / 0.00 %    40.55 % / 0.28 %
        B3-start-seeded-nodrop     49.12 % / 0.00 %    18.62 % / 1.24 %
    With the start drawn per pixel on every image, as attacks.py draws it, conv1 has no exact tie at all (mnist_like says why it draws
    it per quadrant on two images in three)."""
    x, params, drop, keep = R.make_case(case)
    a1 = R.forward64(x, params, drop, keep)["a1"].astype(np.float32)
    _, (d1, t1, _), (d2, t2, _), _, _ = R.classify_both(x, params, drop, keep, a1)
    (tie1, und1), (tie2, und2) = R.shares(d1, t1), R.shares(d2, t2)
    print("%s: conv1 tie %.4f undecided %.4f, conv2 tie %.4f undecided %.4f" % (R.case_id(case), tie1, und1, tie2, und2))
    assert not (d1 & t1).any() and not (d2 & t2).any()
    assert tie1 >= 0.25 and tie2 >= 0.02, (tie1, tie2)
    assert und1 <= 0.02 and und2 <= 0.02, (und1, und2)
    if drop is not None:
        assert (np.asarray(drop) == 0).mean() >= 1.0 / 3.0


def test_mnist_like_is_mnist_like():
    """exact 0 background, exact 1.0 strokes, grey levels k / 255 in between, one all-zero and one all-one image; the start keeps every
    pixel in [0, 1] and within EPS of the clean image, and is drawn per pixel on every third image"""
    x = R.mnist_like(6, 3)
    assert x.dtype == np.float32 and x.shape == (6, 1, 28, 28)
    assert not x[1].any() and (x[2] == 1).all()
    k = x * np.float32(255.0)
    assert np.array_equal(np.rint(k) / np.float32(255.0), x)
    for b in (0, 3, 4, 5):
        assert (x[b] == 0).mean() > 0.5 and (x[b] == 1).mean() > 0.05 and ((x[b] > 0) & (x[b] < 1)).mean() > 0.03
    assert not x[0, 0, :16, :16].any() and x[3, 0, :16, :16].any()
    xs = R.mnist_like(6, 3, R.EPS)
    assert xs.min() >= 0 and xs.max() <= 1 and np.abs(xs - x).max() <= np.float32(R.EPS)
    assert len(np.unique(xs[1])) <= 4 and len(np.unique(xs[2])) > 300
    assert np.array_equal(R.mnist_like(6, 3, R.EPS), xs)
    hard = R.net2_params(7, True)
    for name in ("conv1.bias", "conv2.bias"):
        b = hard[name]
        assert int((b == 0).sum()) >= 4 and int((b > 0).sum()) >= 4 and int((b < 0).sum()) >= 4
