"""CPU: the L2 Square attack's pattern, schedule and draws, the ABI of its two kernels, the `norm` keyword at every layer, and the
plain-torch host path of utils.attacks.Square(norm="L2") against tests/square_l2_reference.py bit for bit in float64."""
import ctypes
import math

import numpy as np
import pytest
import torch

import square_l2_reference as R
from tiny_models import Args, TinyNet

EPS, NQ, SEED = 0.5, 40, 99
BALL = EPS * (1 + 4 * 2.0 ** -23)


# ---- pattern, schedule, draws ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 44, 57])
def test_eta(s):
    from eeadv import sqatk
    e = sqatk.eta(s)
    assert e.dtype == np.float32 and e.shape == (s, s) and np.array_equal(e, R.eta(s))
    assert R.ulps(np.float32(R.exact_norm(e)), np.float32(1.0)) <= 1
    if s >= 2:
        assert (e[:s // 2] > 0).all() and (e[s // 2:] < 0).all()
    with pytest.raises(ValueError):
        sqatk.eta(0)


def test_schedule():
    from eeadv import sqatk
    for n, H, W in ((5000, 64, 64), (5000, 28, 28), (5000, 32, 32), (40, 9, 9), (40, 16, 20), (100, 9, 130), (2, 3, 7), (300, 224, 224), (60, 8, 8)):
        s = sqatk.square_schedule_l2(n, H, W)
        assert len(s) == n - 1 and s == R.schedule(n, H, W)
        assert all(v % 2 == 1 and 3 <= v <= min(H, W) for v in s)
        assert all(a >= b for a, b in zip(s, s[1:])), "sizes must not increase"
    s = sqatk.square_schedule_l2(5000, 64, 64)
    assert (s[0], s[-1]) == (57, 3)
    assert sqatk.square_schedule_l2(40, 9, 9)[0] == 9  # sqrt(0.8 * 81) rounds to 8: made odd, the window is the image
    assert sqatk.square_schedule_l2(1, 8, 8) == []
    for bad in ((0, 8, 8), (10, 2, 8), (10, 8, 2)):
        with pytest.raises(ValueError):
            sqatk.square_schedule_l2(*bad)
    assert [sqatk.start_size(h, w) for h, w in ((28, 28), (32, 32), (64, 64), (224, 224), (9, 9), (16, 20), (3, 3))] == [5, 6, 12, 44, 1, 3, 1]
    sizes = sqatk.square_schedule_l2(5000, 64, 64)
    eta, off, off0 = sqatk.eta_tables(sizes, 12)
    assert eta.dtype == np.float32 and off.dtype == np.int32 and len(off) == len(sizes) and len(set(sizes) | {12}) <= 12
    for i in (0, 100, 4998):
        assert np.array_equal(eta[off[i]:off[i] + sizes[i] ** 2].reshape(sizes[i], sizes[i]), R.eta(sizes[i]))
    assert np.array_equal(eta[off0:off0 + 144].reshape(12, 12), R.eta(12)) and eta.size == sum(v * v for v in set(sizes) | {12})


def test_draws():
    from eeadv import sqatk
    assert (sqatk.STREAM_WINDOW, sqatk.STREAM_WINDOW2, sqatk.STREAM_TILE) == (R.STREAM_WINDOW, R.STREAM_WINDOW2, R.STREAM_TILE) == (11, 13, 14)
    assert len({0, 7, sqatk.STREAM_WINDOW, sqatk.STREAM_STRIPE, sqatk.STREAM_WINDOW2, sqatk.STREAM_TILE}) == 6
    H, W, s = 9, 13, 5
    coins = set()
    for i in range(40):
        vh, vw, bits, tr = sqatk.windows_l2(77, i, np.arange(6), H, W, s)
        vh2, vw2 = sqatk.windows2(77, i, np.arange(6), H, W, s)
        first = sqatk.windows(77, i, np.arange(6), H, W, s)
        assert all(np.array_equal(a, b) for a, b in zip((vh, vw, bits), first)), "window 1 is the Linf window draw"
        for b in range(6):
            assert (int(vh[b]), int(vw[b]), int(bits[b]), int(tr[b])) == R.window1(77, i, b, H, W, s)
            assert (int(vh2[b]), int(vw2[b])) == R.window2(77, i, b, H, W, s)
            assert 0 <= vh2[b] <= H - s and 0 <= vw2[b] <= W - s
        coins.update(tr.tolist())
    assert coins == {0, 1}
    bits, tr = sqatk.tiles(5, [0, 3, 2 ** 31 + 1], 25)
    assert bits.shape == tr.shape == (3, 25) and set(np.unique(tr)) == {0, 1}
    for k, b in enumerate((0, 3, 2 ** 31 + 1)):
        for t in (0, 1, 24):
            assert (int(bits[k, t]), int(tr[k, t])) == R.tile(5, b, t)


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_l2_square_kernels():
    import eeadv._native as n
    from eeadv import ops
    L = n.lib
    for name in ("ee_sqatk_init_l2_f32", "ee_sqatk_step_l2_f32"):
        assert name in n.SIGNATURES and hasattr(L, name)
    assert (n.K_SQATK_INIT, n.K_SQATK_MARGIN, n.K_SQATK_STEP) == (23, 24, 25)  # the L2 launches record under the Linf ids
    assert ops.SQATK_L2_PATHS == {"auto": 0, "resident": 1, "streaming": 2} and ops.SQATK_L2_RESIDENT == 12288
    p = ctypes.c_void_p(4096)
    eps, nan, odd = ctypes.c_float(0.5), ctypes.c_float(float("nan")), ctypes.c_void_p(4098)
    # init: x_best, x_new, x0, seed, eta, s0, B, C, H, W, eps, path, stream
    f = L.ee_sqatk_init_l2_f32
    assert f(p, p, p, p, p, 1, -1, 3, 8, 8, eps, 0, None) == -2 and f(p, p, p, p, p, 1, 2, 3, 0, 8, eps, 0, None) == -2
    assert f(p, p, p, p, p, 1, 2, 3, 8, 8, ctypes.c_float(-0.5), 0, None) == -2 and f(p, p, p, p, p, 1, 2, 3, 8, 8, nan, 0, None) == -2
    assert f(p, p, p, p, p, 1, 2, 3, 8, 8, eps, 3, None) == -2 and f(p, p, p, p, p, 1, 2, 3, 8, 8, eps, -1, None) == -2  # no such path
    assert f(p, p, p, p, p, 0, 2, 3, 8, 8, eps, 0, None) == -2 and f(p, p, p, p, p, 9, 2, 3, 8, 8, eps, 0, None) == -2  # s0 outside the image
    assert f(p, p, p, p, p, 1, 2, 33, 8, 8, eps, 0, None) == -3
    assert f(p, p, p, p, p, 12, 2, 3, 64, 68, eps, 1, None) == -3 and f(p, p, p, p, p, 12, 2, 3, 64, 68, eps, 3, None) == -2
    assert f(None, None, None, None, None, 1, 0, 3, 8, 8, eps, 0, None) == 0
    for k in range(5):  # every pointer is required
        ptrs = [p] * 5
        ptrs[k] = None
        assert f(*ptrs, 1, 2, 3, 8, 8, eps, 0, None) == -1, k
        ptrs[k] = odd
        assert f(*ptrs, 1, 2, 3, 8, 8, eps, 0, None) == -4, k
    # step: x_best, x_new, x0, flags, margin_min, counter, sizes, eta_off, eta, n_sizes, seed, norms, B, C, H, W, eps, path, stream
    g = L.ee_sqatk_step_l2_f32
    nine = [p] * 9
    assert g(*nine, 5, p, p, -2, 3, 8, 8, eps, 0, None) == -2 and g(*nine, -1, p, p, 2, 3, 8, 8, eps, 0, None) == -2
    assert g(*nine, 5, p, p, 2, 3, 8, -8, eps, 0, None) == -2 and g(*nine, 5, p, p, 2, 3, 8, 8, nan, 0, None) == -2
    assert g(*nine, 5, p, p, 2, 3, 8, 8, eps, 3, None) == -2 and g(*nine, 5, p, p, 2, 3, 8, 8, ctypes.c_float(-1.0), 0, None) == -2
    assert g(*nine, 5, p, p, 2, 33, 8, 8, eps, 0, None) == -3
    assert g(*nine, 5, p, p, 2, 3, 64, 68, eps, 1, None) == -3  # the resident path ends at 12288
    assert g(*([None] * 9), 0, None, None, 0, 3, 8, 8, eps, 0, None) == 0
    for k in range(11):  # every pointer is required (positions 9 and 10 of the pointer list: seed, norms)
        ptrs = [p] * 11
        ptrs[k] = None
        assert g(*ptrs[:9], 5, *ptrs[9:], 2, 3, 8, 8, eps, 0, None) == -1, k
        ptrs[k] = odd
        assert g(*ptrs[:9], 5, *ptrs[9:], 2, 3, 8, 8, eps, 0, None) == -4, k
    # without a table, sizes, eta_off and eta may be NULL: the check goes on to the next pointer
    assert g(p, p, p, p, p, p, None, None, None, 0, None, p, 2, 3, 8, 8, eps, 0, None) == -1
    assert g(p, p, p, p, p, p, None, None, None, 0, odd, p, 2, 3, 8, 8, eps, 0, None) == -4
    z = torch.zeros(2, 3, 8, 8)
    with pytest.raises(n.EEError):  # no CPU fallback
        ops.sqatk_init_l2_(z, z.clone(), z.clone(), torch.zeros(1, dtype=torch.int64), torch.zeros(1, 1), 0.5)
    with pytest.raises(n.EEError):
        ops.sqatk_step_l2_(z, z.clone(), z.clone(), torch.zeros(2, dtype=torch.int32), torch.zeros(2), torch.zeros(1, dtype=torch.int32), None, None,
                           None, torch.zeros(1, dtype=torch.int64), 0.5)


# ---- host path -------------------------------------------------------------------------------------------------------------------------
class _Linear(torch.nn.Module):
    def __init__(self, D, K=10, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.w = torch.nn.Parameter(torch.randn(K, D, generator=g, dtype=torch.float64) * 0.3)

    def forward(self, x):  # a product and a sum per (sample, class): a sample's logits do not depend on who shares its batch
        return (x.flatten(1).unsqueeze(1) * self.w.unsqueeze(0)).sum(dim=2)


@pytest.fixture(scope="module")
def cpu_plumbing():
    from eeadv import runtime
    runtime.allow_cpu_plumbing(True)
    yield
    runtime.allow_cpu_plumbing(False)


@pytest.fixture(scope="module", params=[(3, 9, 9), (3, 16, 20)], ids=["3x9x9", "3x16x20"])
def host_run(request, cpu_plumbing):
    """One traced float64 host run per shape and the reference teacher-forced on its margins and norms, shared by the tests below."""
    import utils.attacks as A
    C, H, W = request.param
    B = 4
    g = torch.Generator().manual_seed(0)
    x0 = torch.rand(B, C, H, W, generator=g, dtype=torch.float64)
    x0[:, :, 0, :] = 0.0  # exact ends of [0, 1]: the clamp binds there
    x0[:, :, 1, :] = 1.0
    model = _Linear(C * H * W).eval()
    with torch.no_grad():
        y = model(x0).argmax(1)
    y[0] = (y[0] + 1) % 10  # one sample starts misclassified
    trace = []
    out = A._square_host(model, x0, y, NQ, EPS, SEED, trace=trace, early_exit=False, norm="L2")
    margins = [t["margin"].numpy() for t in trace]
    ref = R.run(x0.numpy(), y.numpy(), NQ, EPS, SEED, margins=margins, start_norms=trace[0]["norms"].numpy(),
                norms=[t["norms"].numpy() for t in trace[1:]])
    return model, x0, y, trace, out, ref


def test_host_path_equals_the_reference_bit_for_bit(host_run):
    model, x0, y, trace, (x_best, margin_min, queries), (samples, flags, _) = host_run
    assert x_best.dtype == torch.float64 and len(trace) == NQ
    assert torch.stack([t["flags"] for t in trace]).tolist() == flags
    assert sum(sum(f) for f in flags[1:]) >= 1, "no proposal accepted: the run shows nothing"
    for b, s in enumerate(samples):
        for q in range(NQ):
            assert np.array_equal(trace[q]["x_new"][b].numpy(), s.iterates[q]), (b, q)
        assert np.array_equal(x_best[b].numpy(), s.x_best) and float(margin_min[b]) == float(s.margin_min) and int(queries[b]) == s.queries
        # each host norm within one ulp of the reference's own at that stage
        assert R.ulps(np.float64(trace[0]["norms"][0, b]), s.start_norms[0]) <= 1
        for i, own in s.norms:
            assert max(R.ulps(trace[i + 1]["norms"][:, b].numpy(), np.array(own))) <= 1, (b, i)


def test_ball_and_box_on_every_proposal(host_run):
    model, x0, y, trace, _, _ = host_run
    for q, t in enumerate(trace):
        xn = t["x_new"].numpy()
        assert xn.min() >= 0 and xn.max() <= 1
        for b in range(x0.shape[0]):
            assert R.exact_norm(xn[b] - x0[b].numpy()) <= BALL, (q, b)


def test_fooled_samples_are_frozen_and_the_public_function_wraps_the_run(host_run):
    import utils.attacks as A
    model, x0, y, trace, (x_best, margin_min, queries), (samples, _, _) = host_run
    assert int(queries[0]) == 1 and not samples[0].robust  # misclassified at the start: one forward, then frozen
    for t in trace[1:]:
        assert torch.equal(t["x_new"][0], trace[0]["x_new"][0]) and not bool(t["flags"][0]) and not bool(t["norms"][:, 0].any())
    assert torch.equal(x_best[0], trace[0]["x_new"][0])
    # the early exit changes nothing, and Square(norm="L2") is the same run
    again = A._square_host(model, x0, y, NQ, EPS, SEED, norm="L2")
    assert all(torch.equal(a, b) for a, b in zip(again, (x_best, margin_min, queries)))
    xa, robust, qs = A.Square(model, Args(epsilon=EPS), x0, y, n_queries=NQ, seed=SEED, norm="L2")
    assert torch.equal(robust, margin_min > 0) and torch.equal(qs, queries)
    assert torch.equal(xa, torch.where(robust.view(-1, 1, 1, 1), x0, x_best))
    # the Linf call is untouched by the keyword
    a = A._square_host(model, x0, y, 12, 0.05, SEED)
    b = A._square_host(model, x0, y, 12, 0.05, SEED, norm="Linf")
    assert all(torch.equal(p, q) for p, q in zip(a, b)) and not torch.equal(a[0], again[0])


def test_a_trajectory_does_not_depend_on_the_batch(host_run):
    import utils.attacks as A
    model, x0, y, trace, (x_best, margin_min, queries), _ = host_run
    pick = [2, 1]
    xb, mm, q = A._square_host(model, x0[pick], y[pick], NQ, EPS, SEED, ids=pick, early_exit=False, norm="L2")
    assert torch.equal(xb, x_best[pick]) and torch.equal(mm, margin_min[pick]) and torch.equal(q, queries[pick])
    other = A._square_host(model, x0[pick], y[pick], NQ, EPS, SEED, early_exit=False, norm="L2")[0]  # drawn under ids 0, 1
    assert not torch.equal(other, xb)


def test_eps_zero_is_the_clean_image(cpu_plumbing):
    import utils.attacks as A
    x0 = torch.rand(2, 3, 9, 9, dtype=torch.float64)
    model = _Linear(243).eval()
    y = model(x0).argmax(1)
    trace = []
    A._square_host(model, x0, y, 5, 0.0, SEED, trace=trace, early_exit=False, norm="L2")
    assert all(torch.equal(t["x_new"], x0) for t in trace)


# ---- the keyword -----------------------------------------------------------------------------------------------------------------------
def test_a_bad_norm_is_a_value_error_at_every_layer(cpu_plumbing):
    import utils.attacks as A
    from eeadv import cascade, engine
    x0 = torch.rand(2, 3, 9, 9)
    y = torch.zeros(2, dtype=torch.int64)
    model = _Linear(243).float().eval()
    args = Args(epsilon=EPS)
    for call in (lambda: A.Square(model, args, x0, y, 5, seed=1, norm="L1"),
                 lambda: A._square_host(model, x0, y, 5, EPS, 1, norm="l2"),
                 lambda: engine.square_loop(model, x0, y, 5, EPS, seed=1, norm="L1"),
                 lambda: engine._SquareRun(x0, y, 5, EPS, norm=2),
                 lambda: cascade.default_stages(args, 5, 10, norm="L1")):
        with pytest.raises(ValueError, match="norm"):
            call()
    assert engine.SQUARE_NORMS == ("Linf", "L2")


def test_default_stages_in_l2_on_the_host(cpu_plumbing):
    from eeadv import cascade
    torch.manual_seed(0)
    model = TinyNet(3, 8, 10, seed=0).eval()
    x = torch.rand(4, 3, 8, 8)
    with torch.no_grad():
        z = model(x)
    y = z.argmax(1)
    order = torch.sort(z, dim=1, descending=True, stable=True)[1][:, :3].contiguous()
    args = Args(epsilon=EPS, fab_iters=5, square_queries=12)
    stages = cascade.default_stages(args, 5, 10, n_target_classes=2, norm="L2")
    assert [name for name, _ in stages] == list(cascade.STAGES)
    assert [name for name, _ in cascade.default_stages(args, 5, 10)] == list(cascade.STAGES)
    for name, fn in stages:
        x_adv, robust = fn(model, args, x, y, order)
        assert x_adv.shape == x.shape and robust.shape == (4,) and robust.dtype == torch.bool, name
        norms = (x_adv - x).flatten(1).double().norm(dim=1)
        assert float(norms.max()) <= EPS * (1 + 1e-5), (name, norms)  # float32 points: the ball to a few ulps of eps
        assert float(x_adv.min()) >= 0 and float(x_adv.max()) <= 1, name
        assert torch.equal(x_adv[robust], x[robust]), name
