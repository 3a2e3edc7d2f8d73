"""GPU: fast adversarial training - the three ee_fastat launches against the launches and torch expressions they
restate, bit for bit; the captured step against the eager one and both against float64; PGD with restarts; the driver."""
import ctypes
import math
import os
import re
import subprocess
import sys

import pytest
import torch

import fastat_reference as FR
from tiny_models import TinyModuleNet

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_DIR = os.path.join(ROOT, "edge-enhancement_amd", "ImageNet", "fgsm_imagenet")
DEV = "cuda:0"
NS = [1, 3, 4, 5, 4099]
EPS, ALPHA = 4 / 255, 5 / 255


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def buf(n, off, fill=None):
    """n floats starting `off` elements into a 16-byte aligned allocation: off = 1 takes the word-wise path"""
    t = torch.empty(n + 4, device=DEV)[off:off + n]
    return t.fill_(fill) if fill is not None else t


def put(v, off):
    return buf(v.numel(), off).copy_(v.to(DEV))


def hard_inputs(n, seed):
    """x with entries at exactly 0 and 1, delta with entries at +-eps and rows that put x + delta on and outside the box, g with
    +-0, NaN, +-inf and +-the smallest subnormal"""
    g0 = torch.Generator().manual_seed(seed)
    x = torch.rand(n, generator=g0)
    d = (torch.rand(n, generator=g0) * 2 - 1) * EPS
    g = torch.randn(n, generator=g0)
    xs = torch.tensor([0.0, 1.0, 0.0, 1.0, 0.5, 0.0, 1.0, EPS, 1.0 - EPS])
    ds = torch.tensor([0.0, 0.0, -EPS, EPS, EPS, EPS, -EPS, -EPS, EPS])  # x + d: 0, 1, below, above, inside, inside, inside, exactly 0, ~1
    gs = torch.tensor([0.0, -0.0, float("nan"), float("inf"), -float("inf"), 1e-45, -1e-45, 1.0, -1.0])
    k = min(n, 9)
    x[:k], d[:k], g[:k] = xs[:k], ds[:k], gs[:k]
    if n > 40:  # every special gradient once more on a plain interior pixel, and big gradients on pixels outside the box
        g[20:27] = gs[:7]
        x[30:34], d[30:34], g[30:34] = torch.tensor([0.0, 1.0, 0.0, 1.0]), torch.tensor([-EPS, EPS, -EPS, EPS]), torch.tensor([5.0, -5.0, -5.0, 5.0])
    return x, d, g


# ---- start -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", NS)
def test_start_injected_noise(n, off):
    from eeadv import ops
    x, d, _ = hard_inputs(n, n)
    X, NZ = put(x, off), put(d, off)
    delta, in1 = buf(n + 8, off, 7.0), buf(n, off)
    ops.fastat_start_(delta, in1, X, EPS, noise=NZ)
    torch.cuda.synchronize()
    assert torch.equal(bits(delta[:n]), bits(NZ)) and bool((delta[n:] == 7.0).all())  # the noise as bits; rows beyond n untouched
    assert torch.equal(bits(in1), bits(ops.add_clamp(X.clone(), NZ.clone(), 0.0, 1.0)))  # ee_add_clamp_f32's bits
    assert torch.equal(bits(in1), bits((X + NZ).clamp(0, 1.0)))  # main_fast.py:234-235


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", NS)
def test_start_drawn_noise(n, off):
    from eeadv import ops
    x, _, _ = hard_inputs(n, n)
    X = put(x, off)
    seed, draws = 0x1234567890ABCDEF, []
    for step in (0, 3):
        ctr = torch.full((1,), step, dtype=torch.int64, device=DEV)
        delta, in1 = buf(n + 8, off, 7.0), buf(n, off)
        ops.fastat_start_(delta, in1, X, EPS, seed=seed, step=ctr)
        want = ops.pgd_init_rng(torch.zeros(n, device=DEV), EPS, 0, seed, step << 32, -EPS, EPS)
        torch.cuda.synchronize()
        assert int(ctr) == step  # read, never written
        assert torch.equal(bits(delta[:n]), bits(want)) and bool((delta[n:] == 7.0).all())
        assert float(delta[:n].abs().max()) <= torch.tensor(EPS, dtype=torch.float32).item()
        assert torch.equal(bits(in1), bits(ops.add_clamp(X.clone(), delta[:n].clone(), 0.0, 1.0)))
        assert torch.equal(delta[:n].cpu(), torch.from_numpy(ops.fastat_draw_host(n, EPS, seed, step)))  # the host restatement
        draws.append(delta[:n].clone())
    assert not torch.equal(draws[0], draws[1])


def test_start_and_ascend_error_codes():
    from eeadv import _native as N
    L, p, q = N.lib, ctypes.c_void_p(4096), ctypes.c_void_p(4098)
    st = torch.zeros(1, dtype=torch.int64, device=DEV)
    s = ctypes.c_void_p(st.data_ptr())
    assert L.ee_fastat_start_f32(p, p, p, None, -1, 0.1, 0, s, None) == -2
    assert L.ee_fastat_start_f32(p, p, p, None, 4 << 32, 0.1, 0, s, None) == -2  # n / 4 >= 2^32
    assert L.ee_fastat_start_f32(p, p, p, None, 16, -0.1, 0, s, None) == -2
    assert L.ee_fastat_start_f32(p, p, p, None, 16, float("nan"), 0, s, None) == -2
    assert L.ee_fastat_start_f32(None, None, None, None, 0, 0.1, 0, None, None) == 0  # n == 0 launches nothing
    assert L.ee_fastat_start_f32(p, None, p, None, 16, 0.1, 0, s, None) == -1
    assert L.ee_fastat_start_f32(p, p, p, None, 16, 0.1, 0, None, None) == -1  # a draw needs the counter
    assert L.ee_fastat_start_f32(q, p, p, p, 16, 0.1, 0, None, None) == -4
    assert L.ee_fastat_start_f32(p, p, p, None, 16, 0.1, 0, ctypes.c_void_p(st.data_ptr() + 4), None) == -4
    assert L.ee_fastat_ascend_f32(p, p, p, p, -1, 0.1, 0.1, None, None) == -2
    assert L.ee_fastat_ascend_f32(None, None, None, None, 0, 0.1, 0.1, None, None) == 0
    assert L.ee_fastat_ascend_f32(p, p, None, p, 16, 0.1, 0.1, None, None) == -1
    assert L.ee_fastat_ascend_f32(p, q, p, p, 16, 0.1, 0.1, None, None) == -4
    assert L.ee_fastat_keep_f32(p, ctypes.c_void_p(8192), p, p, 2, 0, 4, 0, None) == -2  # K < 1 without `first`
    assert L.ee_fastat_keep_f32(p, p, p, p, 2, 3, 4, 1, None) == -2  # final == x
    assert L.ee_fastat_keep_f32(p, ctypes.c_void_p(8192), None, None, 2, 3, 4, 0, None) == -1
    assert L.ee_fastat_keep_f32(p, ctypes.c_void_p(8192), p, ctypes.c_void_p(4100), 2, 3, 4, 0, None) == -4
    assert L.ee_fastat_keep_f32(None, None, None, None, 0, 3, 4, 0, None) == 0


# ---- ascend ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", NS)
def test_ascend_is_the_two_launches_in_one(n, off):
    from eeadv import ops
    x, d, g = hard_inputs(n, 100 + n)
    X, G = put(x, off), put(g, off)
    delta, in1 = buf(n + 8, off, 7.0), buf(n, off)
    delta[:n].copy_(d)
    ctr = torch.full((1,), 41, dtype=torch.int64, device=DEV)
    want_d = buf(n, off).copy_(d)
    ops.freeat_update_masked_(want_d, G, X, ALPHA, EPS)
    want_in = ops.add_clamp(X, want_d, 0.0, 1.0)
    ops.fastat_ascend_(delta, in1, G, X, ALPHA, EPS, ctr)
    torch.cuda.synchronize()
    assert torch.equal(bits(delta[:n]), bits(want_d)) and bool((delta[n:] == 7.0).all())
    assert torch.equal(bits(in1), bits(want_in)) and int(ctr) == 42
    # in1 may be the gradient's buffer, and the counter may be absent
    d2, g2 = buf(n, off).copy_(d), G.clone() if off == 0 else put(g, off)
    ops.fastat_ascend_(d2, g2, g2, X, ALPHA, EPS, None)
    torch.cuda.synchronize()
    assert torch.equal(bits(d2), bits(want_d)) and torch.equal(bits(g2), bits(want_in)) and int(ctr) == 42
    # the rows written by hand: a masked or zero / NaN gradient leaves delta, +-inf and the subnormals move it by alpha
    if n >= 9:
        got = delta[:9].cpu()
        a, e = torch.tensor(ALPHA), torch.tensor(EPS)
        assert got[0] == 0 and got[1] == 0 and got[2] == -e and got[3] == e  # g = 0, -0; x + d outside the box
        assert got[4] == torch.clamp(e - a, -e, e) and got[7] == torch.clamp(-e + a, -e, e)  # -inf; x + d exactly 0 passes the gradient


# ---- keep ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("per", [1, 5, 12288, 12289])
@pytest.mark.parametrize("K", [1, 5, 1000])
@pytest.mark.parametrize("B", [1, 3])
def test_keep_against_torch_indexing(B, K, per, first):
    from eeadv import ops
    g0 = torch.Generator().manual_seed(B * 7 + K)
    x, final = torch.rand(B, per, generator=g0).to(DEV), torch.rand(B, per, generator=g0).to(DEV)
    x[0, 0] = float("nan")  # rows are copied as bits
    logits = torch.randn(B, K, generator=g0)
    labels = torch.randint(0, K, (B,), generator=g0)
    if K >= 5:
        logits[0, 1] = logits[0, K - 1] = 50.0  # a tie: the lowest index, 1
        labels[0] = 1
    if B >= 3:
        labels[2] = K  # out of range: never equal
        if K >= 5:
            logits[1, 3] = logits[1, 2] = float("nan")  # the first NaN, 2
            logits[1, 0] = float("inf")
            labels[1] = 2
    logits, labels = logits.to(DEV), labels.to(DEV)
    want = final.clone()
    if first:
        want = x.clone()
    else:
        I = logits.max(1)[1] != labels  # lib/validation.py:56-57 on the same device
        want[I] = x[I]
        if K >= 5:
            assert not bool(I[0]) and (B < 3 or (not bool(I[1]) and bool(I[2])))
    got = ops.fastat_keep_(final.clone(), x, None if first else logits, None if first else labels, first=bool(first))
    torch.cuda.synchronize()
    assert torch.equal(bits(got), bits(want))
    if per == 12288:  # the same rows one word off 16 bytes: the word-wise copy
        f2, x2 = put(final.view(-1), 1).view(B, per), put(x.view(-1), 1).view(B, per)
        ops.fastat_keep_(f2, x2, None if first else logits, None if first else labels, first=bool(first))
        assert torch.equal(bits(f2), bits(want))


# ---- the step --------------------------------------------------------------------------------------------------------------------------
# five steps: trainer.EAGER_UPDATES_BEFORE_CAPTURE = 2 of them run eagerly, the third is captured and replayed, the fourth and fifth are
# replays of that graph under learning rates (and, where the noise is drawn, counter values) it was not captured with
LRS = (0.1, 0.25, 0.02, 0.3, 0.05)
G_FLOOR = 1e-9


def _setup(dtype):
    g0 = torch.Generator().manual_seed(11)
    m = TinyModuleNet(3, 32, 10, seed=4).to(DEV).to(dtype).train()
    xs = [torch.rand(4, 3, 32, 32, generator=g0).to(DEV).to(dtype) for _ in LRS]
    ys = [torch.randint(0, 10, (4,), generator=g0).to(DEV) for _ in LRS]
    nz = [((torch.rand(4, 3, 32, 32, generator=g0) * 2 - 1) * EPS).to(DEV).to(dtype) for _ in LRS]
    return m, xs, ys, nz


def _state(m, opt, noise, loss):
    out = {"param." + k: v.detach().clone() for k, v in m.named_parameters()}
    out.update({"buffer." + k: v.detach().clone() for k, v in m.named_buffers() if v.dtype.is_floating_point})
    for i, p in enumerate(p for g in opt.param_groups for p in g["params"]):
        out["momentum.%d" % i] = opt.state[p]["momentum_buffer"].detach().clone()
    out["delta"], out["loss"] = noise.detach().clone(), loss.detach().clone().reshape(1)
    return out


def _run_stock(dtype):
    m, xs, ys, nz = _setup(dtype)
    opt = FR.make_sgd(m, 0.1, 0.9, 1e-4)
    noise, gs = torch.zeros(4, 3, 32, 32, device=DEV, dtype=dtype), []
    for lr, x, y, z in zip(LRS, xs, ys, nz):
        FR.set_lr(opt, lr)
        loss, _, g = FR.fast_step(m, opt, x, y, noise, ALPHA, EPS, True, z)
        gs.append(g)
    return _state(m, opt, noise, loss), gs


def _run_ours(graph, monkeypatch, setup=None, inject=True, lr_scale=1.0):
    """the state after EVERY step, and the number of captures"""
    from eeadv import trainer
    monkeypatch.setenv("EEADV_GRAPH", "1" if graph else "0")
    m, xs, ys, nz = (setup or _setup)(torch.float32)
    opt = trainer.make_fast_sgd(m, 0.1, momentum=0.9, weight_decay=1e-4)
    noise = torch.zeros_like(xs[0])
    step = trainer.FastAtStep(m, trainer.Criterion(), opt, noise, ALPHA, EPS, random_init=True, seed=77)
    states = []
    for lr, x, y, z in zip(LRS, xs, ys, nz):
        step.set_lr(lr * lr_scale)
        loss, _ = step(x, y, injected_noise=z if inject else None)
        states.append(_state(m, opt, noise, loss))
    torch.cuda.synchronize()
    assert int(step.step_ctr) == len(LRS)
    return states, step.captures


def _ulp32(v):
    return 2.0 ** (math.floor(math.log2(v)) - 23) if v > 0 else 2.0 ** -149


def _same_after_every_step(eager, graph):
    assert len(eager) == len(graph) == len(LRS)
    for i, (e, g) in enumerate(zip(eager, graph)):
        assert e.keys() == g.keys()
        differ = {k: float((e[k] - g[k]).abs().max()) for k in e if not torch.equal(bits(e[k]), bits(g[k]))}
        assert not differ, ("step %d" % (i + 1), differ)


def test_step_graph_against_eager_and_both_against_float64(monkeypatch):
    """Five steps of TinyModuleNet (convolution, BatchNorm2d, ReLU, pooling, linear) at 3 x 32 x 32, B = 4, injected noise, learning rates
    0.1 / 0.25 / 0.02 / 0.3 / 0.05: steps 4 and 5 replay the graph captured at step 3 under other learning rates.  After EVERY step the
    captured run equals the eager one bit for bit - a learning rate frozen into the graph would show at step 4 - with exactly one
    capture.  Against the float64 restatement every quantity may be 4 x as far as the fp32 stock-torch restatement on the same device,
    plus one fp32 ulp of the quantity's largest magnitude.  delta is compared where the float64 |g| of the last step exceeds
    G_FLOOR = 1e-9, an element counting as disagreeing when the two deltas are more than half a step (alpha / 2) apart: on the CPU the
    stock fp32 run disagrees with float64 on 0 of the 12196 elements above the floor (0.00 %; the smallest non-zero |g| is 1.6e-9, the
    other 92 elements have a gradient of exactly zero in both and move in neither; the largest delta difference is 1.6e-9)."""
    # the model's layers are stock ones: MIOpen must not pick its atomic-add weight gradients, whose sums depend on arrival order
    torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = False, True
    eager, c0 = _run_ours(False, monkeypatch)
    graph, c1 = _run_ours(True, monkeypatch)
    assert c0 == 0 and c1 == 1
    _same_after_every_step(eager, graph)
    assert not torch.equal(graph[3]["param.fc.weight"], graph[4]["param.fc.weight"])  # the replays moved the weights
    graph = graph[-1]
    stock, _ = _run_stock(torch.float32)
    f64, g64 = _run_stock(torch.float64)
    live = g64[-1].abs() > G_FLOOR
    share = float((((stock["delta"].double() - f64["delta"]).abs() > ALPHA / 2) & live).sum()) / max(int(live.sum()), 1)
    print("delta: stock fp32 differs from float64 on %.4f %% of the %d elements above the floor" % (100 * share, int(live.sum())))
    assert share <= 0.01
    for k in f64:
        ref = f64[k]
        a, b = graph[k].double(), stock[k].double()
        if k == "delta":
            a, b, ref = a[live], b[live], ref[live]
        d_ours, d_stock = float((a - ref).abs().max()), float((b - ref).abs().max())
        bound = 4 * d_stock + _ulp32(float(ref.abs().max()))
        print("%-28s ours %.3e stock %.3e bound %.3e" % (k, d_ours, d_stock, bound))
        assert d_ours <= bound, (k, d_ours, d_stock, bound)


def test_step_drawn_noise_replays_draw_on(monkeypatch):
    """The same five steps with the noise DRAWN by ee_fastat_start_f32: under the graph the start launch of a replay reads the counter the
    ascend launch of the replay before advanced.  Bit-identical to the eager run after every step, one capture, and no two steps share
    their noise - a counter frozen into the graph would repeat step 3's draw at steps 4 and 5."""
    torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = False, True
    eager, c0 = _run_ours(False, monkeypatch, inject=False)
    graph, c1 = _run_ours(True, monkeypatch, inject=False)
    assert c0 == 0 and c1 == 1
    _same_after_every_step(eager, graph)
    for i in range(1, len(LRS)):
        # alpha > eps, so most elements end a step clamped at +-eps whatever was drawn; an element inside the ball is its draw moved by 0 or
        # +-alpha: from one draw, two steps would agree on about half of those, from two draws on none
        a, b = graph[i]["delta"], graph[i - 1]["delta"]
        inside = (a.abs() < a.abs().max()) & (b.abs() < b.abs().max())
        same = float((a == b)[inside].float().mean())
        print("steps %d and %d: %d elements inside the ball in both, %.4f %% of them equal" % (i, i + 1, int(inside.sum()), 100 * same))
        assert int(inside.sum()) > 500 and same < 0.01, (i, int(inside.sum()), same)
        assert float(graph[i]["delta"].abs().max()) <= torch.tensor(EPS).item()


def _setup_resnet(dtype):
    """models_imagenet.resnet50 as the driver builds it, at 3 x 32 x 32 (8 x 8, 4 x 4, 2 x 2 and 1 x 1 maps: the Winograd, stride-2, dense
    2 x 2, weight-gradient and fused BatchNorm kernels and their weight-derived filter buffers all take part), batch 8, 10 classes"""
    from eeadv.models import make_resnet
    torch.manual_seed(21)
    m = make_resnet(50, "imagenet", num_classes=10)  # what models_imagenet.resnet50 builds
    m.avgpool = torch.nn.AdaptiveAvgPool2d(1)
    m = m.to(DEV).to(dtype).train()
    g0 = torch.Generator().manual_seed(12)
    xs = [torch.rand(8, 3, 32, 32, generator=g0).to(DEV) for _ in LRS]
    ys = [torch.randint(0, 10, (8,), generator=g0).to(DEV) for _ in LRS]
    return m, xs, ys, [None] * len(LRS)


def test_step_graph_against_eager_on_the_resnet(monkeypatch):
    """The bit-identity part on a ResNet of the package: what the captured step must get right there and a stock model never asks for is
    the rebuild of the weight-derived filter buffers inside the graph (functional.rebuild_dense_weights) against _FusedSGD's
    invalidation in the eager run - a replay that convolved with the filters of the step before would differ from step 4 on.  Drawn
    noise, five learning rates (a tenth of LRS: batch 8 on a fresh ResNet-50), compared after every step, one capture."""
    from eeadv import functional as EF
    torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = False, True
    eager, c0 = _run_ours(False, monkeypatch, setup=_setup_resnet, inject=False, lr_scale=0.1)
    graph, c1 = _run_ours(True, monkeypatch, setup=_setup_resnet, inject=False, lr_scale=0.1)
    assert c0 == 0 and c1 == 1
    assert len(EF._DENSE_W) > 0  # the model does keep weight-derived buffers: the comparison covers their rebuild
    _same_after_every_step(eager, graph)
    assert all(bool(torch.isfinite(s["loss"]).all()) for s in graph)


# ---- PGD with restarts -----------------------------------------------------------------------------------------------------------------
def test_pgd_restarts_graph_against_eager_and_the_restatement(monkeypatch):
    from eeadv import engine, trainer
    g0 = torch.Generator().manual_seed(5)
    m = TinyModuleNet(3, 32, 10, seed=6).to(DEV).eval()
    x, y = torch.rand(8, 3, 32, 32, generator=g0).to(DEV), torch.randint(0, 10, (8,), generator=g0).to(DEV)
    eps, step = 8 / 255, 2 / 255
    noises = [((torch.rand(8, 3, 32, 32, generator=g0) * 2 - 1) * eps).to(DEV) for _ in range(3)]
    monkeypatch.setenv("EEADV_GRAPH", "0")
    fe, oe = trainer.pgd_restarts(m, x, y, eps, 3, step, 3, seed=0, noises=noises)
    monkeypatch.setenv("EEADV_GRAPH", "1")
    engine.clear_graphs()
    fg, og = trainer.pgd_restarts(m, x, y, eps, 3, step, 3, seed=0, noises=noises)
    torch.cuda.synchronize()
    assert torch.equal(bits(fe), bits(fg)) and torch.equal(bits(oe), bits(og))
    lo, hi = torch.clamp(x - eps, 0, 1), torch.clamp(x + eps, 0, 1)  # fp32, as the step forms them
    assert bool((fg >= lo).all()) and bool((fg <= hi).all()) and float(fg.min()) >= 0 and float(fg.max()) <= 1
    fr, orr = FR.validate_pgd_batch(m, x, y, eps, 3, step, noises)
    assert torch.equal(og.max(1)[1] == y, orr.max(1)[1] == y)  # top-1
    fd, _ = trainer.pgd_restarts(m, x, y, eps, 3, step, 2, seed=9)  # drawn starts
    assert bool((fd >= lo).all()) and bool((fd <= hi).all())


# ---- the driver ------------------------------------------------------------------------------------------------------------------------
_CFG = """
TRAIN: {arch: 'resnet50', lr: 0.1, momentum: 0.9, weight_decay: 0.0001, print_freq: 1, start_epoch: 0, epochs: 2,
        lr_epochs: [0, 1, 2], lr_values: [0, 0.4, 0.04], half: true, random_init: true}
ADV: {clip_eps: 4.0, fgsm_step: 5.0, n_repeats: 1, pgd_attack: [[2, 0.00392156862], [3, 0.00392156862]]}
DATA: {workers: 1, max_color_value: 255.0, img_size: 0, batch_size: 8, crop_size: 32}
"""


def test_driver_trains_resumes_and_evaluates(tmp_path):
    (tmp_path / "c.yml").write_text(_CFG)
    main = os.path.join(DRIVER_DIR, "main_fast.py")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "edge-enhancement_amd"), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, main, "synthetic:4:1", "-c", "c.yml", "--output_prefix", "g"], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    name = "g_step5_eps4_repeat1"
    ck = tmp_path / "trained_models" / name / "checkpoint_epoch2.pth.tar"
    assert ck.is_file() and (tmp_path / "trained_models" / name / "checkpoint_epoch1.pth.tar").is_file()
    # utils.py:100-101 copies model_best only when the clean top-1 rose above 0, which 8 random images of 1000 classes need not do
    state = torch.load(ck, map_location="cpu", weights_only=True)
    assert state["epoch"] == 2 and all(k.startswith("module.") for k in state["state_dict"])
    assert (tmp_path / "trained_models" / name / "model_best.pth.tar").is_file() == (state["best_prec1"] > 0)
    log = (tmp_path / "output" / name / "log.txt").read_text().splitlines()
    assert any("TRAIN.half is set: this run is fp32" in ln for ln in log)
    last = [ln for ln in log if ln.startswith("Train Epoch: [1][3/4]")]
    assert len(last) == 1 and last[0].endswith("LR 0.040") and re.search(r"Loss \d+\.\d{4} \(\d+\.\d{4}\)", last[0])
    assert re.match(r"^ Final Prec@1 \d+\.\d{3} Prec@5 \d+\.\d{3}$", log[-1])
    r = subprocess.run([sys.executable, main, "synthetic:4:1", "-c", "c.yml", "--output_prefix", "g", "--resume", str(ck), "--evaluate",
                        "--restarts", "2"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ev = (tmp_path / "output" / name / "eval.txt").read_text().splitlines()
    assert any(ln.endswith("(epoch 2)") for ln in ev) and sum(" PGD eps: " in ln and "restarts: 2" in ln for ln in ev) == 2
    assert [bool(re.match(r"^ PGD Final Prec@1 \d+\.\d{3} Prec@5 \d+\.\d{3}$", ln)) for ln in ev].count(True) == 2
    assert re.match(r"^ Final Prec@1 \d+\.\d{3} Prec@5 \d+\.\d{3}$", ev[-1])
