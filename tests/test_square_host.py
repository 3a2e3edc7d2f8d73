"""CPU: the Square attack's schedule and draws, the ABI of its kernels, and the plain-torch host path of utils.attacks.Square against
tests/square_reference.py bit for bit in float64."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import square_reference as R
from tiny_models import Args, TinyNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")


def test_philox_known_answer():
    """Random123's kat_vectors: philox4x32-10, counter 0, key 0."""
    assert R.philox_raw((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert R.philox(0, 0, 0) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)


def test_schedule():
    from eeadv import engine
    for n, H, W in ((5000, 64, 64), (5000, 28, 28), (49, 64, 64), (60, 8, 8), (100, 9, 130), (2, 5, 7)):
        s = engine.square_schedule(n, H, W)
        assert len(s) == n - 1 and s == R.schedule(n, H, W)
        assert all(a >= b for a, b in zip(s, s[1:])), "sizes must not increase"
        assert all(1 <= v <= min(H, W) for v in s)
    assert engine.square_schedule(5000, 64, 64)[0] == round(math.sqrt(0.8 * 4096)) == 57
    assert engine.square_schedule(1, 8, 8) == []
    assert engine.square_schedule(5000, 64, 64)[-1] == max(int(round(math.sqrt(0.8 / 512 * 4096))), 1)
    with pytest.raises(ValueError):
        engine.square_schedule(0, 8, 8)


def _old_p_selection(it, p_init, n_queries, rescale):
    """Add_Square.p_selection as it stood before the table moved to a free function."""
    if rescale:
        it = int(it / n_queries * 10000)
    if 10 < it <= 50:
        return p_init / 2
    elif 50 < it <= 200:
        return p_init / 4
    elif 200 < it <= 500:
        return p_init / 8
    elif 500 < it <= 1000:
        return p_init / 16
    elif 1000 < it <= 2000:
        return p_init / 32
    elif 2000 < it <= 4000:
        return p_init / 64
    elif 4000 < it <= 6000:
        return p_init / 128
    elif 6000 < it <= 8000:
        return p_init / 256
    elif 8000 < it:
        return p_init / 512
    return p_init


@pytest.mark.parametrize("c,h,p_init,nq,rescale", [(3, 64, 0.8, 5000, False), (3, 64, 0.8, 300, True), (1, 28, 0.3, 9000, False), (3, 224, 0.8, 1, False),
                                                   (3, 32, 0.05, 10000, True)])
def test_add_square_sizes_unchanged(c, h, p_init, nq, rescale):
    import utils.core as C
    m = C.Add_Square(c, h, 0.05, p_init=p_init, n_queries=nq, rescale_schedule=rescale)
    want = [max(int(round(math.sqrt(_old_p_selection(i, p_init, nq, rescale) * (c * h * h) / c))), 1) for i in range(nq)]
    assert m.square_sizes("cpu")[0] == want
    for it in (0, 10, 11, 50, 51, 200, 201, 500, 501, 1000, 1001, 2000, 2001, 4000, 4001, 6000, 6001, 8000, 8001, 20000):
        assert m.p_selection(it) == _old_p_selection(it, p_init, nq, rescale)


def test_numpy_philox_equals_the_scalar_one():
    from eeadv import sqatk
    assert (sqatk.STREAM_WINDOW, sqatk.STREAM_STRIPE) == (R.STREAM_WINDOW, R.STREAM_STRIPE)
    assert len({0, 7, sqatk.STREAM_WINDOW, sqatk.STREAM_STRIPE}) == 4
    rng = np.random.default_rng(0)
    ctrs = [0, 1, 2 ** 32 - 1, 2 ** 32, (4998 << 32) | 129, 2 ** 64 - 1] + [int(v) for v in rng.integers(0, 2 ** 63, 94, dtype=np.uint64)]
    for seed in (0, 1, 0x123456789ABCDEF0, 2 ** 64 - 1, -5):
        for sid in (sqatk.STREAM_WINDOW, sqatk.STREAM_STRIPE):
            got = sqatk.philox4x32(seed, np.array(ctrs, dtype=np.uint64), sid)
            assert got.shape == (100, 4)
            for k, c in enumerate(ctrs):
                assert tuple(int(v) for v in got[k]) == R.philox(seed, c, sid), (seed, sid, c)


def test_window_draws():
    from eeadv import sqatk
    H = W = 8
    seen_h, seen_w = set(), set()
    for i in range(200):  # 200 proposals x 10 samples = 2000 draws
        vh, vw, bits = sqatk.windows(77, i, np.arange(10), H, W, 7)
        for b in range(10):
            assert (int(vh[b]), int(vw[b]), int(bits[b])) == R.window(77, i, b, H, W, 7)
        seen_h.update(vh.tolist())
        seen_w.update(vw.tolist())
    assert seen_h == {0, 1} and seen_w == {0, 1}  # [0, H - s], both ends hit
    vh, vw, _ = sqatk.windows(77, 3, np.arange(50), H, W, 8)
    assert not vh.any() and not vw.any()  # s = H: the origin is 0
    vh, vw, _ = sqatk.windows(5, 9, np.arange(500), 9, 130, 3)
    assert vh.min() >= 0 and vh.max() <= 6 and vw.min() >= 0 and vw.max() <= 127
    st = sqatk.stripes(9, [0, 3], 3, 130)
    assert st.shape == (2, 3, 130) and set(np.unique(st)) == {-1.0, 1.0}
    for k, b in enumerate((0, 3)):
        for c in range(3):
            for w in (0, 1, 31, 32, 127, 128, 129):
                assert st[k, c, w] == R.stripe_sign(9, b, c, w, 3)


def test_abi_of_the_square_attack_kernels():
    import eeadv._native as n
    L = n.lib
    for name in ("ee_sqatk_init_f32", "ee_sqatk_margin_f32", "ee_sqatk_step_f32"):
        assert name in n.SIGNATURES and hasattr(L, name)
    assert (n.K_SQATK_INIT, n.K_SQATK_MARGIN, n.K_SQATK_STEP) == (23, 24, 25)
    p = ctypes.c_void_p(4096)
    # init: x_best, x_new, x0, seed, B, C, H, W, eps, stream
    assert L.ee_sqatk_init_f32(None, p, p, p, 2, 3, 8, 8, 0.1, None) == -1 and L.ee_sqatk_init_f32(p, p, p, None, 2, 3, 8, 8, 0.1, None) == -1
    assert L.ee_sqatk_init_f32(p, p, p, p, -1, 3, 8, 8, 0.1, None) == -2 and L.ee_sqatk_init_f32(p, p, p, p, 2, 3, 0, 8, 0.1, None) == -2
    assert L.ee_sqatk_init_f32(p, p, p, p, 2, 33, 8, 8, 0.1, None) == -3
    assert L.ee_sqatk_init_f32(None, None, None, None, 0, 3, 8, 8, 0.1, None) == 0
    assert L.ee_sqatk_init_f32(ctypes.c_void_p(4098), p, p, p, 2, 3, 8, 8, 0.1, None) == -4
    # margin: logits, labels, B, K, margin_out, margin_min, queries, flags, counter, stream
    assert L.ee_sqatk_margin_f32(p, p, 4, 1, p, p, p, p, p, None) == -2  # K = 1: no other class
    assert L.ee_sqatk_margin_f32(p, p, -1, 10, p, p, p, p, p, None) == -2
    assert L.ee_sqatk_margin_f32(None, p, 4, 10, p, p, p, p, p, None) == -1 and L.ee_sqatk_margin_f32(p, p, 4, 10, p, p, p, p, None, None) == -1
    assert L.ee_sqatk_margin_f32(p, None, 4, 10, p, p, p, p, p, None) == -1 and L.ee_sqatk_margin_f32(p, p, 4, 10, p, None, p, p, p, None) == -1
    assert L.ee_sqatk_margin_f32(None, None, 0, 10, None, None, None, None, None, None) == 0
    # step: x_best, x_new, x0, flags, margin_min, counter, sizes, n_sizes, seed, B, C, H, W, eps, stream
    assert L.ee_sqatk_step_f32(p, p, p, p, p, p, p, 5, p, 2, 33, 8, 8, 0.1, None) == -3
    assert L.ee_sqatk_step_f32(p, p, p, p, p, p, p, 5, p, -2, 3, 8, 8, 0.1, None) == -2 and L.ee_sqatk_step_f32(p, p, p, p, p, p, p, -1, p, 2, 3, 8, 8, 0.1, None) == -2
    assert L.ee_sqatk_step_f32(p, p, p, p, p, p, p, 5, p, 2, 3, 8, -8, 0.1, None) == -2
    assert L.ee_sqatk_step_f32(p, None, p, p, p, p, p, 5, p, 2, 3, 8, 8, 0.1, None) == -1 and L.ee_sqatk_step_f32(p, p, p, None, p, p, p, 5, p, 2, 3, 8, 8, 0.1, None) == -1
    assert L.ee_sqatk_step_f32(p, p, p, p, p, p, None, 5, p, 2, 3, 8, 8, 0.1, None) == -1  # a table of 5 entries must exist
    assert L.ee_sqatk_step_f32(p, p, p, p, p, p, p, 5, None, 2, 3, 8, 8, 0.1, None) == -1
    assert L.ee_sqatk_step_f32(None, None, None, None, None, None, None, 0, None, 0, 3, 8, 8, 0.1, None) == 0
    assert L.ee_sqatk_step_f32(p, p, ctypes.c_void_p(4098), p, p, p, p, 5, p, 2, 3, 8, 8, 0.1, None) == -4


# ---- host path -------------------------------------------------------------------------------------------------------------------------
B, HW, NCLS, NQ, SEED = 5, 8, 10, 60, 1234


@pytest.fixture(scope="module")
def host_problem():
    from eeadv import runtime
    runtime.allow_cpu_plumbing(True)
    torch.manual_seed(0)
    model = TinyNet(3, HW, NCLS, seed=0).double().eval()
    x0 = torch.rand(B, 3, HW, HW, dtype=torch.float64)
    x0[:, :, 0, :] = 0.0  # exact ends of [0, 1]: the clamp binds there
    x0[:, :, 1, :] = 1.0
    with torch.no_grad():
        y = model(x0).argmax(1)
    y[0] = (y[0] + 1) % NCLS  # one sample starts misclassified
    yield model, x0, y
    runtime.allow_cpu_plumbing(False)


def _logits_fn(model):
    def f(x):
        with torch.no_grad():
            return model(torch.from_numpy(x)).numpy()
    return f


@pytest.fixture(scope="module")
def reference_runs(host_problem):
    """The reference trajectories, computed once per eps and shared."""
    model, x0, y = host_problem
    return {eps: R.run(x0.numpy(), y.numpy(), NQ, eps, SEED, logits=_logits_fn(model)) for eps in (0.03, 0.6)}


@pytest.mark.parametrize("eps", [0.03, 0.6], ids=["eps0.03", "eps0.6-ball-and-clamp-bind"])
def test_host_path_equals_the_reference_bit_for_bit(host_problem, reference_runs, eps):
    import utils.attacks as A
    model, x0, y = host_problem
    samples, flags, seen = reference_runs[eps]
    trace = []
    x_best, margin_min, queries = A._square_host(model, x0, y, NQ, eps, SEED, trace=trace, early_exit=False)
    assert x_best.dtype == torch.float64 and len(trace) == NQ
    for b, s in enumerate(samples):
        assert np.array_equal(x_best[b].numpy(), s.x_best), b
        assert float(margin_min[b]) == float(s.margin_min) and int(queries[b]) == s.queries, b
    for q in range(NQ):
        assert trace[q]["flags"].tolist() == flags[q], q
        assert np.array_equal(trace[q]["margin"].numpy(), np.array(seen[q]), equal_nan=True), q
    # the early exit changes nothing (it can only trigger once every sample is frozen), and the public function wraps the same run
    xb2, mm2, q2 = A._square_host(model, x0, y, NQ, eps, SEED)
    assert torch.equal(xb2, x_best) and torch.equal(mm2, margin_min) and torch.equal(q2, queries)
    xa, robust, qs = A.Square(model, Args(epsilon=eps), x0, y, n_queries=NQ, seed=SEED)
    assert torch.equal(robust, margin_min > 0) and torch.equal(qs, queries)
    assert torch.equal(xa, torch.where(robust.view(-1, 1, 1, 1), x0, x_best))
    # the ball as the projection forms it: between the rounded x0 - eps and x0 + eps ((x0 + eps) - x0 itself may round above eps)
    assert bool((xa >= x0 - eps).all()) and bool((xa <= x0 + eps).all()) and float(xa.min()) >= 0 and float(xa.max()) <= 1
    # the run exercises what it is meant to
    assert not samples[0].robust and samples[0].queries == 1  # fooled by the start: one forward, frozen
    assert any(any(f) for f in flags[1:]) and any(not all(f) for f in flags[1:]), "accepts and rejects"
    if eps == 0.6:
        xb, x0n = x_best.numpy(), x0.numpy()
        assert ((xb == x0n + eps) | (xb == x0n - eps)).any(), "the ball binds"
        inner = (x0n > 0) & (x0n < 1)
        assert ((xb == 0) & inner).any() and ((xb == 1) & inner).any(), "the [0, 1] clamp binds"


class _RowWise(torch.nn.Module):
    """The classifier applied to one sample at a time: a CPU convolution's last bits depend on the batch it is given, and this test is
    about the attack's draws and decisions, not about that."""

    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, x):
        return torch.cat([self.model(x[b:b + 1]) for b in range(x.shape[0])])


def test_batch_independence(host_problem):
    import utils.attacks as A
    model, x0, y = host_problem
    model = _RowWise(model)
    eps = 0.03
    samples, flags, seen = R.run(x0.numpy(), y.numpy(), NQ, eps, SEED, logits=_logits_fn(model))
    assert any(f[2] for f in flags[1:]) and samples[2].queries > 1
    # the reference: sample 2 alone, under its id, fed the margins it saw inside the batch and - separately - the model itself
    alone, f1, _ = R.run(x0.numpy()[2:3], y.numpy()[2:3], NQ, eps, SEED, margins=[[row[2]] for row in seen], ids=[2])
    assert np.array_equal(alone[0].x_best, samples[2].x_best) and [f[0] for f in f1] == [f[2] for f in flags]
    alone, f2, s2 = R.run(x0.numpy()[2:3], y.numpy()[2:3], NQ, eps, SEED, logits=_logits_fn(model), ids=[2])
    assert np.array_equal(alone[0].x_best, samples[2].x_best) and alone[0].queries == samples[2].queries
    assert [f[0] for f in f2] == [f[2] for f in flags] and [m[0] for m in s2] == [m[2] for m in seen]
    # under another id the draws, and so the trajectory, differ
    other, _, _ = R.run(x0.numpy()[2:3], y.numpy()[2:3], NQ, eps, SEED, logits=_logits_fn(model), ids=[0])
    assert not np.array_equal(other[0].x_best, samples[2].x_best)
    # the host path (TinyNet has no BatchNorm): alone under its id, and with other companions
    full = A._square_host(model, x0, y, NQ, eps, SEED, early_exit=False)
    assert np.array_equal(full[0][2].numpy(), samples[2].x_best)
    solo = A._square_host(model, x0[2:3], y[2:3], NQ, eps, SEED, ids=[2], early_exit=False)
    for a, b in zip(full, solo):
        assert torch.equal(a[2:3], b)
    g = torch.Generator().manual_seed(5)
    x_mixed = torch.rand(B, 3, HW, HW, dtype=torch.float64, generator=g)
    x_mixed[2] = x0[2]
    mixed = A._square_host(model, x_mixed, y, NQ, eps, SEED, early_exit=False)
    for a, b in zip(full, mixed):
        assert torch.equal(a[2], b[2])


def test_nan_and_bad_label_rows_are_never_accepted():
    import utils.attacks as A
    z = torch.tensor([[1.0, 2.0, 0.5], [float("nan"), 2.0, 0.5], [1.0, 2.0, 0.5], [float("inf"), float("inf"), 0.0], [3.0, 3.0, 1.0]], dtype=torch.float64)
    y = torch.tensor([1, 1, 3, 0, 0])
    m = A._square_margin(z, y)
    assert float(m[0]) == 1.0 and math.isnan(float(m[1])) and math.isnan(float(m[2])) and math.isnan(float(m[3])) and float(m[4]) == 0.0
    for b in range(5):
        r = R.margin_of(z[b].numpy(), int(y[b]))
        assert (math.isnan(float(r)) and math.isnan(float(m[b]))) or float(r) == float(m[b])
    # a sample whose margin is always NaN: never accepted, never fooled (margin_min stays +inf, so `robust = margin_min > 0` holds),
    # active for every forward, x_best stays the start
    x0 = np.full((1, 1, 4, 4), 0.5)
    s, flags, _ = R.run(x0, [0], 6, 0.1, 3, margins=[[float("nan")]] * 6)
    assert not any(f[0] for f in flags) and s[0].queries == 6 and s[0].robust and not s[0].fooled
    assert np.array_equal(s[0].x_best, R.start_point(x0[0], 0, 0.1, 3))


# ---- dispatch --------------------------------------------------------------------------------------------------------------------------
def test_validation_dispatch(host_problem):
    from eeadv import trainer
    import utils.attacks as A
    model, x0, y = host_problem
    eps = 0.03
    assert trainer.SQUARE_METHODS == ("Square", "APGD+Square")
    a = Args(epsilon=eps, method_name="AT", attack_method="Square", random=True, square_queries=12)
    torch.manual_seed(11)
    xa = trainer.attack_for_validation(model, a, x0, y, "cpu", 4, 0.01, NCLS)
    torch.manual_seed(11)
    want, _, queries = A.Square(model, a, x0, y, n_queries=12)
    assert torch.equal(xa, want) and int(queries.max()) <= 12
    a.attack_method = "APGD+Square"
    torch.manual_seed(11)
    out = trainer.attack_for_validation(model, a, x0, y, "cpu", 3, 0.01, NCLS)
    assert out.shape == x0.shape and bool((out >= x0 - eps).all()) and bool((out <= x0 + eps).all())
    torch.manual_seed(11)
    xc, rc = A.APGD(model, a, x0, y, 3, "ce")
    xt, rt = A.APGD_T(model, a, x0, y, 3, NCLS)
    xs, rs, _ = A.Square(model, a, x0, y, n_queries=12)
    want = torch.where((rc & ~rt).view(-1, 1, 1, 1), xt, xc)
    want = torch.where((rc & rt & ~rs).view(-1, 1, 1, 1), xs, want)
    assert torch.equal(out, want)
    for method in ("Square", "APGD+Square"):
        a.attack_method, a.method_name = method, "tar_AT"
        with pytest.raises(NotImplementedError):
            trainer.attack_for_validation(model, a, x0, y, "cpu", 2, 0.01, NCLS)
    a.method_name, a.attack_method = "AT", "AA"
    with pytest.raises(NotImplementedError):
        trainer.attack_for_validation(model, a, x0, y, "cpu", 2, 0.01, NCLS)


def test_device_path_refuses_cpu_tensors_without_the_opt_in():
    from eeadv import runtime
    import utils.attacks as A
    was = runtime.cpu_plumbing_allowed()
    runtime.allow_cpu_plumbing(False)
    try:
        with pytest.raises(RuntimeError, match="ROCm device"):
            A.Square(TinyNet(3, 8, 10, seed=0).eval(), Args(epsilon=0.03), torch.rand(2, 3, 8, 8), torch.tensor([0, 1]), n_queries=3)
    finally:
        runtime.allow_cpu_plumbing(was)


def test_mnist_driver_evaluates_with_square_on_the_host(tmp_path):
    r = subprocess.run([sys.executable, "experiments_mnist.py", "-c", "configs_mnist/adversarial_training.yml", "--no-cuda", "--data", "synthetic:1:1",
                        "--output-root", str(tmp_path), "-e", "--attack_method", "Square", "--square_queries", "12"],
                       cwd=os.path.join(PKG, "MNIST"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    logs = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path)) for f in fs if f.startswith("log")]
    text = r.stdout + "".join(open(f).read() for f in logs)
    clean = re.findall(r"^ \* Clean Prec@1 ([\d.]+)", text, flags=re.M)
    adv = re.findall(r"^ \* Adv Prec@1 ([\d.]+)", text, flags=re.M)
    assert len(clean) >= 1 and len(clean) == len(adv)
    for c1, a1 in zip(clean, adv):
        assert float(a1) <= float(c1)
