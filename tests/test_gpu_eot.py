"""GPU: EOT for APGD - the accumulate kernel (ee_eot.hip) against numpy bit for bit, engine.apgd_loop(eot_iter=E) on a deterministic model
(EOT is the identity there), on a model whose draws are scripted (what enters the bookkeeping and the step), on the randomised
resnet18_EE_square (eager against graph replay, every draw a fresh one), the unchanged default, the driver and Cascade-Rand."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import eot_reference as ER
from tiny_models import Args, TinyNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")


@pytest.fixture(scope="module")
def ops():
    from eeadv import ops
    return ops


# ---- 1. the accumulate kernel ------------------------------------------------------------------------------------------------------------
def _bits(a):
    """The bit patterns, every NaN mapped to one pattern: which NaN an addition returns (sign, payload) is the hardware's choice - x86 and
    gfx950 differ for inf - inf - and IEEE 754 leaves it open; everything else, signed zeros and denormals included, is compared as is."""
    a = np.ascontiguousarray(a)
    bits = a.view(np.uint32 if a.dtype == np.float32 else np.uint64).copy()
    bits[np.isnan(a)] = 0x7FC00000 if a.dtype == np.float32 else 0x7FF8000000000000
    return bits


SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.1754942e-38, -5.877472e-39, 3.0e-39, 1.0, -1.0, 3.4028235e38,
                    -3.4028235e38, 1.17549435e-38], dtype=np.float32)


def _draw_values(rng, shape, k):
    n = int(np.prod(shape))
    g = rng.standard_normal(n).astype(np.float32)
    g[rng.integers(0, n, max(1, n // 3))] = SPECIAL[rng.integers(0, len(SPECIAL), max(1, n // 3))]
    g[k % n] = SPECIAL[k % len(SPECIAL)]  # every draw has a special value, wherever the random positions fell
    if n > 4:
        g[4] = [3.0e-39, 2.0e-39, -4.0e-39, 1.0e-39, 5.0e-39][k % 5]  # a denormal in every draw at one element: a denormal sum
    return g.reshape(shape)


@pytest.mark.parametrize("E", [1, 2, 3, 5])
@pytest.mark.parametrize("B,P", [(3, 37), (2, 192), (1, 1), (5, 4)])
def test_accumulate_kernel_bit_exact(ops, B, P, E):
    """g_acc and loss_mean after the E launches k = 0 .. E-1 against numpy: the f32 sequential sum followed by * (1 / E) with 1 / E formed
    in f32, the losses summed in float64 - bit for bit (NaNs as NaNs), also after every launch before the last.  The accumulators start as
    NaN / garbage: k == 0 overwrites them.  Inputs: normals, +-0, +-inf, NaN, denormals and the largest finite values."""
    rng = np.random.default_rng(1000 * B + 10 * P + E)
    gs = [_draw_values(rng, (B, P), k) for k in range(E)]
    ls = [_draw_values(rng, (B,), k + 1) for k in range(E)]
    g_acc = torch.full((B, P), float("nan"), device=DEV)
    g_acc.view(-1)[::2] = 1e30
    loss_acc = torch.full((B,), float("nan"), dtype=torch.float64, device=DEV)
    loss_mean = torch.full((B,), -7.0, device=DEV)
    for k in range(E):
        ops.apgd_eot_acc_(g_acc, torch.from_numpy(gs[k]).to(DEV), loss_acc, torch.from_numpy(ls[k]).to(DEV), loss_mean, k, E)
        if k < E - 1:  # the running sums
            with np.errstate(all="ignore"):
                want = gs[0].copy()
                for g in gs[1:k + 1]:
                    want = want + g
            np.testing.assert_array_equal(_bits(g_acc.cpu().numpy()), _bits(want))
            np.testing.assert_array_equal(_bits(loss_acc.cpu().numpy()), _bits(ER.mean_loss(ls[:k + 1])[0]))
            assert bool((loss_mean == -7.0).all())  # written by the last draw only
    want_acc, want_mean = ER.mean_loss(ls)
    np.testing.assert_array_equal(_bits(g_acc.cpu().numpy()), _bits(ER.mean_gradient(gs)))
    np.testing.assert_array_equal(_bits(loss_acc.cpu().numpy()), _bits(want_acc))
    np.testing.assert_array_equal(_bits(loss_mean.cpu().numpy()), _bits(want_mean))
    # E equal losses give that loss back
    same = torch.from_numpy(ls[0]).to(DEV)
    for k in range(E):
        ops.apgd_eot_acc_(g_acc, torch.from_numpy(gs[k]).to(DEV), loss_acc, same, loss_mean, k, E)
    np.testing.assert_array_equal(_bits(loss_mean.cpu().numpy()), _bits(ls[0]))


def test_accumulate_kernel_unaligned_view_empty_and_errors(ops):
    import ctypes
    from eeadv import _native as N
    B, P, E = 3, 37, 3
    rng = np.random.default_rng(5)
    gs = [_draw_values(rng, (B, P), k) for k in range(E)]
    ls = [rng.standard_normal(B).astype(np.float32) for _ in range(E)]
    pad = torch.zeros(2, B * P + 1, device=DEV)  # views at an odd offset: the 16-byte path is not taken, the result is the same
    acc, g = pad[0, 1:].view(B, P), pad[1, 1:].view(B, P)
    loss_acc, loss_mean = torch.zeros(B, dtype=torch.float64, device=DEV), torch.zeros(B, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for k in range(E):
        g.copy_(torch.from_numpy(gs[k]))
        loss = torch.from_numpy(ls[k]).to(DEV)
        assert N.lib.ee_apgd_eot_acc_f32(ptr(acc), ptr(g), ptr(loss_acc), ptr(loss), ptr(loss_mean), k, E, B, P, stream) == 0
    np.testing.assert_array_equal(_bits(acc.cpu().numpy()), _bits(ER.mean_gradient(gs)))
    np.testing.assert_array_equal(_bits(loss_mean.cpu().numpy()), _bits(ER.mean_loss(ls)[1]))
    # an empty batch launches nothing and leaves nothing behind; bad k or E are errors
    e, e64 = torch.empty(0, 12, device=DEV), torch.empty(0, dtype=torch.float64, device=DEV)
    ops.apgd_eot_acc_(e, e.clone(), e64, torch.empty(0, device=DEV), torch.empty(0, device=DEV), 0, 2)
    z = torch.empty(3, 0, device=DEV)
    la, lm = torch.full((3,), 5.0, dtype=torch.float64, device=DEV), torch.full((3,), 6.0, device=DEV)
    ops.apgd_eot_acc_(z, z.clone(), la, torch.ones(3, device=DEV), lm, 1, 2)
    torch.cuda.synchronize()
    assert bool((la == 5.0).all()) and bool((lm == 6.0).all())
    acc2, g2 = torch.zeros(B, P, device=DEV), torch.ones(B, P, device=DEV)
    for k, bad_E in ((0, 0), (-1, 2), (2, 2), (5, 3), (0, -1)):
        with pytest.raises(N.EEError, match="ee_apgd_eot_acc_f32"):
            ops.apgd_eot_acc_(acc2, g2, loss_acc, loss_mean.clone(), loss_mean, k, bad_E)
    with pytest.raises(N.EEError):
        ops.apgd_eot_acc_(acc2, acc2, loss_acc, loss_mean.clone(), loss_mean, 0, 2)
    torch.cuda.synchronize()
    assert bool((acc2 == 0).all())
    with pytest.raises(TypeError):
        ops.apgd_eot_acc_(acc2, g2, loss_acc.float(), loss_mean.clone(), loss_mean, 0, 2)
    with pytest.raises(ValueError):
        ops.apgd_eot_acc_(acc2, g2[:, :5].contiguous(), loss_acc, loss_mean.clone(), loss_mean, 0, 2)


# ---- 2. a deterministic model makes EOT the identity -------------------------------------------------------------------------------------
T_SEED, T_B, T_HW, T_NCLS, T_EPS, T_ITER = 0, 6, 8, 10, 0.03, 10


def _tiny_problem(dtype=torch.float32):
    torch.manual_seed(T_SEED)
    model = TinyNet(3, T_HW, T_NCLS, seed=T_SEED).to(dtype).eval()
    x0 = torch.rand(T_B, 3, T_HW, T_HW, dtype=dtype)
    with torch.no_grad():
        y = model(x0).argmax(1)
    y[0] = (y[0] + 1) % T_NCLS
    noise = torch.zeros_like(x0).uniform_(-T_EPS, T_EPS)
    return model, x0, y, torch.clamp(x0 + noise, 0, 1)


@pytest.mark.parametrize("kind", ["ce", "dlr"])
def test_deterministic_model_makes_eot_the_identity(kind):
    """TinyNet draws nothing, so the E gradients of an iterate are one gradient g: E = 2 gives (g + g) * 0.5 = g and E = 3 gives
    (g + g + g) * fl(1/3), which differs from g in magnitude only; the step reads only its sign, and the double mean of E equal losses is
    that loss.  So x_adv, robust and loss_best equal the E = 1 run's bit for bit, eager and under graph replay.  The sign argument fails
    only if a non-zero gradient element underflows to zero under * 1/3 (or the sum overflows): the fp32 host run of this very problem
    (seed 0) is checked below to keep every non-zero gradient element between 1e-30 and 1e30 in magnitude, ten binary orders and more away
    from either."""
    import utils.attacks as A
    from eeadv import engine, runtime
    model, x0, y, x_init = _tiny_problem()
    runtime.allow_cpu_plumbing(True)
    try:
        trace = []
        A._apgd_host(model, x0, x_init, y, T_ITER, T_EPS, kind, trace=trace)
    finally:
        runtime.allow_cpu_plumbing(False)
    mags = torch.cat([e["g"].abs().flatten() for e in trace])
    mags = mags[mags != 0]
    assert bool(torch.isfinite(mags).all()) and float(mags.min()) > 1e-30 and float(mags.max()) < 1e30
    m, x0d, yd, xi = model.to(DEV), x0.to(DEV), y.to(DEV), x_init.to(DEV)
    try:
        for graph in (False, True):
            base = engine.apgd_loop(m, x0d, xi, yd, T_ITER, T_EPS, kind, use_graph=graph, eot_iter=1)
            assert not bool(base[1][0]) and not torch.equal(base[0], x0d)  # the attack moved something
            for E in (2, 3):
                got = engine.apgd_loop(m, x0d, xi, yd, T_ITER, T_EPS, kind, use_graph=graph, eot_iter=E)
                for name, a, b in zip(("x_adv", "robust", "loss_best"), got, base):
                    assert torch.equal(a, b), (graph, E, name)
    finally:
        engine.clear_graphs()


# ---- 3. semantics with scripted draws ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ce", "dlr"])
def test_scripted_draws_what_enters_book_and_step(ops, kind, monkeypatch):
    """E = 4, n_iter = 5 (a checkpoint closes every iteration), eager with trace=: the averaged gradient of every iterate is the numpy
    restatement of the accumulate kernel on the 4 recorded draw gradients, the bookkeeping received the double mean of the 4 recorded
    losses and the LAST draw's pred, it ran once per iterate, and the gradient that entered the next step is that average after the copies
    the flags ask for (the average itself, or - for a sample a checkpoint sent back - the average that went with its best loss)."""
    from eeadv import engine
    E, n_iter = 4, 5
    model, x0, y, x_init = _tiny_problem()
    net = ER.ScriptedDraws(model.to(DEV), (1.0, 0.8, 1.2, 0.9, 1.1, 0.7, 1.3), (0.0, 0.05, -0.05, 0.02, -0.02, 0.08, -0.08)).eval()
    book_calls = []
    real_book = ops.apgd_book_
    monkeypatch.setattr(ops, "apgd_book_", lambda *a: (book_calls.append(1), real_book(*a))[1])
    trace = []
    x_adv, robust, loss_best = engine.apgd_loop(net, x0.to(DEV), x_init.to(DEV), y.to(DEV), n_iter, T_EPS, kind, use_graph=False, eot_iter=E,
                                                trace=trace)
    assert net.calls == (n_iter + 1) * E and len(book_calls) == n_iter
    evals, steps = [e for e in trace if "draws" in e], [e for e in trace if "step_g" in e]
    assert len(evals) == n_iter + 1 and len(steps) == n_iter and "draws" in trace[0] and "step_g" in trace[1]
    cur = g_best = None
    restored = differing = 0
    for j, ev in enumerate(evals):
        assert len(ev["draws"]) == E
        gs = [d["g"].cpu().numpy() for d in ev["draws"]]
        ls = [d["loss"].cpu().numpy() for d in ev["draws"]]
        differing += int(not np.array_equal(gs[0], gs[1]))
        g_mean = ev["g_mean"].cpu().numpy()
        np.testing.assert_array_equal(_bits(g_mean), _bits(ER.mean_gradient(gs)))
        np.testing.assert_array_equal(_bits(ev["book_loss"].cpu().numpy()), _bits(ER.mean_loss(ls)[1]))
        assert torch.equal(ev["book_pred"], ev["draws"][-1]["pred"])
        if j == 0:
            assert ev["counter"] is None and ev["flags"] is None  # the start point: no bookkeeping
            cur, g_best = g_mean.copy(), g_mean.copy()
        else:
            assert ev["counter"] == j - 1  # one bookkeeping launch and one `select` per iterate
            f = ev["flags"].cpu().numpy()
            for b in range(T_B):
                cur[b] = g_mean[b]
                if f[b] & ops.APGD_IMPROVED:
                    g_best[b] = g_mean[b]
                elif f[b] & ops.APGD_REDUCED:
                    cur[b] = g_best[b]
                    restored += 1
        if j < n_iter:
            np.testing.assert_array_equal(_bits(steps[j]["step_g"].cpu().numpy()), _bits(cur))
    assert differing == n_iter + 1 and restored >= 1
    assert robust.dtype == torch.bool and not bool(robust[0])


# ---- 4. the randomised model: eager equals graph, every draw a fresh one -----------------------------------------------------------------
def _resnet_ee():
    from eeadv import models
    torch.manual_seed(5)
    m = models.make_resnet_ee(18, "tiny", True, cize=64, r=8, w=1.0, with_gf=False, low=38.0, high=76.0, alpha=0.0, sigma=1.0,
                              type_canny="CannyFilter_step125_1", epsilon=16 / 255, n_queries=1)
    return m.to(DEV).eval()


def _batch(m, seed, B=4):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 3, 64, 64, generator=g).to(DEV)
    with torch.no_grad():
        y = m(x).argmax(1)
    y[0] = (y[0] + 1) % 200  # one sample starts misclassified
    noise = (torch.rand(B, 3, 64, 64, generator=g) * 2 - 1) * (16 / 255)
    return x, y, noise.to(DEV)


def _valid(xa, x0, eps):
    e = torch.tensor(eps, dtype=torch.float32)
    assert bool((xa >= x0 - e).all()) and bool((xa <= x0 + e).all()) and bool((xa >= 0).all()) and bool((xa <= 1).all())


@pytest.mark.parametrize("kind,n_iter,E", [("ce", 4, 3), ("dlr", 4, 3), ("ce", 2, 20)], ids=["ce-4x3", "dlr-4x3", "ce-2x20"])
def test_randomised_model_eager_equals_graph(kind, n_iter, E, monkeypatch):
    """resnet18_EE_square, B = 4, 64 x 64, eval mode; (2, 20) is the one-iteration-per-graph shape.  With the device draw state rewound
    before every run, eager and replay give the same bits, a second replay with a new batch equals a fresh eager run, the results are
    valid, and every run - eager or replayed - advanced the draw state's offset by exactly (n_iter + 1) * E times what one forward
    advances it by: every draw inside a replayed graph is a fresh one."""
    import utils.attacks as A
    from eeadv import engine, runtime
    m = _resnet_ee()
    eps = 16 / 255
    args = Args(epsilon=eps)
    runtime.reseed()
    torch.manual_seed(9)
    state = runtime.draw_state(torch.device(DEV))
    batches = [_batch(m, 1), _batch(m, 2)]
    assert engine._eot_chunk(n_iter, E) == (4 if E == 3 else 1)

    def attack(batch, graph):
        monkeypatch.setenv("EEADV_GRAPH", "1" if graph else "0")
        x, y, noise = batch
        state.copy_(state0)
        out = A.APGD(m, args, x, y, n_iter, kind, noise=noise, eot_iter=E)
        return out, int(state[1].item()) - int(state0[1].item())

    try:
        state0 = state.clone()
        attack(batches[0], True)  # builds the graph (the warm-up passes draw too)
        state0 = state.clone()
        with torch.no_grad():
            m(batches[0][0])
        one = int(state[1].item()) - int(state0[1].item())
        assert one > 0
        eager = [attack(b, False) for b in batches]
        graph = [attack(b, True) for b in batches]
        for ((xe, re_), adv_e), ((xg, rg), adv_g), (x, y, _) in zip(eager, graph, batches):
            assert adv_e == (n_iter + 1) * E * one and adv_g == (n_iter + 1) * E * one
            assert torch.equal(xe, xg) and torch.equal(re_, rg)
            _valid(xe.cpu(), x.cpu(), eps)
            assert not bool(re_[0])
            assert torch.equal(xe[re_], x[re_])  # robust rows are the clean inputs
            assert bool((xe[~re_] != x[~re_]).flatten(1).any(1).all())
        assert not torch.equal(eager[0][0][0], eager[1][0][0])
    finally:
        engine.clear_graphs()


# ---- 5. the unchanged default ------------------------------------------------------------------------------------------------------------
def test_default_is_the_run_without_eot(ops, monkeypatch):
    """A.APGD without eot_iter is apgd_loop(eot_iter=1): the same bits, no accumulate launch; E = 1 and E = 2 are two graphs."""
    import utils.attacks as A
    from eeadv import engine
    model, x0, y, x_init = _tiny_problem()
    m, x0d, yd = model.to(DEV), x0.to(DEV), y.to(DEV)
    noise = (x_init - x0).to(DEV)
    acc_calls = []
    real_acc = ops.apgd_eot_acc_
    monkeypatch.setattr(ops, "apgd_eot_acc_", lambda *a: (acc_calls.append(1), real_acc(*a))[1])
    try:
        for graph in (False, True):
            monkeypatch.setenv("EEADV_GRAPH", "1" if graph else "0")
            xa, rb = A.APGD(m, Args(epsilon=T_EPS), x0d, yd, T_ITER, "ce", noise=noise)
            start = ops.pgd_init(x0d, noise)
            xb, rc, _ = engine.apgd_loop(m, x0d, start, yd, T_ITER, T_EPS, "ce", use_graph=graph, eot_iter=1)
            assert torch.equal(xa, xb) and torch.equal(rb, rc) and not acc_calls
        keys = [k for k in engine._GRAPHS if k[0] == "apgd"]
        assert len(keys) == 1 and keys[0][-1] == 1
        engine.apgd_loop(m, x0d, start, yd, T_ITER, T_EPS, "ce", use_graph=True, eot_iter=2)
        keys = [k for k in engine._GRAPHS if k[0] == "apgd"]
        assert len(keys) == 2 and sorted(k[-1] for k in keys) == [1, 2] and acc_calls
        assert engine._GRAPHS[keys[0]] is not engine._GRAPHS[keys[1]]
    finally:
        engine.clear_graphs()


# ---- 6. driver -----------------------------------------------------------------------------------------------------------------------------
def test_tiny_imagenet_driver_evaluates_with_rand(tmp_path):
    cfg = open(os.path.join(PKG, "Tiny_ImageNet", "configs_tinyimagenet", "adversarial_training.yml")).read()
    cfg = re.sub(r"num_steps_(\d): \d+", r"num_steps_\1: 2", cfg).replace("batch_size: 100", "batch_size: 8").replace("print_freq: 50", "print_freq: 1")
    path = tmp_path / "rand.yml"
    path.write_text(cfg)
    r = subprocess.run([sys.executable, "experiments_tinyimagenet.py", "-c", str(path), "--output-root", str(tmp_path), "--data", "synthetic:1:1",
                        "-e", "--attack_method", "Rand", "--eot_iter", "2"], cwd=os.path.join(PKG, "Tiny_ImageNet"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    logs = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path)) for f in fs if f.startswith("log")]
    text = r.stdout + "".join(open(f).read() for f in logs)
    clean = re.findall(r"^ \* Clean Prec@1 ([\d.]+) Prec@5 ([\d.]+)$", text, flags=re.M)
    adv = re.findall(r"^ \* Adv Prec@1 ([\d.]+) Prec@5 ([\d.]+)$", text, flags=re.M)
    assert len(clean) >= 3 and len(clean) == len(adv)
    for (c1, _), (a1, _) in zip(clean, adv):
        assert float(a1) <= float(c1)


# ---- 7. Cascade-Rand: the device pools against the torch compaction ----------------------------------------------------------------------
def test_cascade_rand_device_pools_equal_the_torch_compaction():
    """A deterministic TinyNet, 3 batches of 4, rand_stages with E = 2, eager: robust and stage from the HIP pools equal those of the
    torch compaction bit for bit, and APGD-DLR ran on the survivors of APGD-CE only."""
    from eeadv import cascade, engine
    torch.manual_seed(3)
    m = TinyNet(3, 8, 10, 5).eval()
    xs = torch.rand(12, 3, 8, 8)
    with torch.no_grad():
        ys = m(xs).argmax(1)
    ys[5] = (ys[5] + 1) % 10
    m, xs, ys = m.to(DEV), xs.to(DEV), ys.to(DEV)
    a = Args(epsilon=2 / 255, eot_iter=2)
    batches = [(xs[i:i + 4], ys[i:i + 4]) for i in (0, 4, 8)]
    runs = {}
    try:
        for mode in ("hip", "torch"):
            torch.manual_seed(100)
            runs[mode] = cascade.evaluate(m, a, batches, 10, compaction=mode, stages=cascade.rand_stages(a, 5))
    finally:
        engine.clear_graphs()
    h, t = runs["hip"], runs["torch"]
    print("rows_attacked %s robust_after %s" % (h.rows_attacked, h.robust_after))
    assert h.stage_names == ["APGD-CE", "APGD-DLR"] and h.n == 12 and h.clean_correct == 11 and int(h.stage[5]) == 0
    assert torch.equal(h.robust, t.robust) and torch.equal(h.stage, t.stage)
    assert h.rows_attacked == t.rows_attacked and h.robust_after == t.robust_after and h.batches_attacked == t.batches_attacked
    assert h.rows_attacked == [h.clean_correct, h.robust_after[0]]
    assert 1 <= h.rows_attacked[1] < h.rows_attacked[0] and h.robust_after[1] >= 1  # APGD-CE broke some rows, not all; some survive both
