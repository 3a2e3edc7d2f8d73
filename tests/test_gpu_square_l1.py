"""GPU: the L1 Square kernels (ee_sqatk_l1.hip), engine.square_l1_loop and the two L1 Square drivers against tests/square_l1_reference.py.

Given the norms and the multiplier a kernel emitted, every element it wrote must equal the reference bit for bit; every emitted norm must
be within one unit in the last place of the exactly summed norm of the reference's elements at that stage; lambda, h0, |A| and dist are
held to the rule tests/test_gpu_apgd_l1.py applies to ee_l1_proj_f32; and ee_l1_proj_f32 itself, given the reference's u, must return the
step's x_new and scal rows bit for bit: one definition of the projection.  eps = D / 256 per shape, so (C + 1) eps <= D."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch import nn

import square_l1_reference as R
from tiny_models import Args, TinyNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
SEED = 20261
RESIDENT = 12288
NQ_TABLE = 40
SHAPES = [(3, 3, 9, 9), (2, 1, 28, 28), (3, 3, 16, 20), (2, 3, 64, 64), (2, 3, 64, 68)]
_ids = lambda s: "x".join(map(str, s))
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "edge-enhancement_amd")


def _eps(shape):
    C, H, W = shape[1:]
    D = C * H * W
    eps = D / 256.0
    assert float(F(eps)) == eps and (C + 1) * eps <= D
    return eps


def _images(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(*shape, generator=g)
    x0.view(-1)[::5] = 0.0  # images at exactly 0 and 1: the box binds
    x0.view(-1)[2::5] = 1.0
    return x0.numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _within_one_ulp(got, want):
    got, want = F(got), F(want)
    return got == want or got == np.nextafter(want, F(np.inf)) or got == np.nextafter(want, F(-np.inf))


def _dev(a, misalign=False):
    if not misalign:
        return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    pad = torch.zeros(a.size + 1, device=DEV)  # a view one float past a 16-byte boundary
    v = pad[1:].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _tables(H, W):
    from eeadv import sqatk
    sizes = sqatk.square_schedule_l2(NQ_TABLE, H, W)
    assert sizes == R.L2.schedule(NQ_TABLE, H, W)
    s0 = sqatk.start_size(H, W)
    eta, off, off0 = sqatk.eta_tables(sizes, s0)
    return sizes, s0, torch.tensor(sizes, dtype=torch.int32, device=DEV), torch.from_numpy(eta).to(DEV), torch.from_numpy(off).to(DEV), off0


def _script(B, n_sizes):
    """(counter, flags [B], fooled [B]) per step launch: within one batch samples are accepted, rejected and fooled; one launch is past the
    table.  Sample B - 1 is fooled from the second launch on (its accepted proposal is committed there, then it is frozen)."""
    last = B - 1
    steps = []
    for k, it in enumerate((0, 1, 2, n_sizes - 1, n_sizes, 3)):
        flags = [(b + k) % 2 for b in range(B)]
        fooled = [b == last and k >= 1 for b in range(B)]
        if k == 1:
            flags[last] = 1
        elif k > 1:
            flags[last] = 0
        steps.append((it, flags, fooled))
    return steps


def _run_kernels(ops, shape, x0, eps, path, misalign, steps):
    """The start and the script on the device: [(x_best, x_new, norms, scal)] after the start (norms None) and after every launch."""
    from eeadv import sqatk
    B, C, H, W = shape
    sizes, s0, dsizes, eta, off, off0 = _tables(H, W)
    eps_p = sqatk.l1_eps_p(eps)
    xb, xn, c = _dev(np.zeros_like(x0), misalign), _dev(np.zeros_like(x0), misalign), _dev(x0, misalign)
    seed = torch.tensor([SEED], dtype=torch.int64, device=DEV)
    scal = ops.sqatk_init_l1_(xb, xn, c, seed, eta[off0:off0 + s0 * s0].view(s0, s0), eps, eps_p, path=path)
    out = [(xb.cpu().numpy(), xn.cpu().numpy(), None, scal.cpu().numpy())]
    for it, flags, fooled in steps:
        f = torch.tensor(flags, dtype=torch.int32, device=DEV)
        mm = torch.tensor([-1.0 if z else 1.0 for z in fooled], dtype=torch.float32, device=DEV)
        cnt = torch.tensor([it], dtype=torch.int32, device=DEV)
        norms, scal = ops.sqatk_step_l1_(xb, xn, c, f, mm, cnt, dsizes, off, eta, seed, eps, eps_p, path=path)
        out.append((xb.cpu().numpy(), xn.cpu().numpy(), norms.cpu().numpy(), scal.cpu().numpy()))
    return out


def _check_scal(scal, b, info, z, x0):
    """The rule of tests/test_gpu_apgd_l1.py for ee_l1_proj_f32's rows."""
    assert int(scal[2, b]) == info["active"], (b, scal[:, b], info)
    assert _within_one_ulp(scal[0, b], info["lam"]) and (scal[0, b] > 0) == (info["lam"] > 0), (b, scal[:, b], info)
    assert _within_one_ulp(scal[1, b], info["h0"]), (b, scal[:, b], info)
    assert _within_one_ulp(scal[3, b], math.fsum(np.abs(z.astype(np.float64) - x0).reshape(-1).tolist())), b


@pytest.fixture(scope="module")
def ops():
    from eeadv import ops
    return ops


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_kernels_against_the_reference_on_every_path(ops, shape):
    B, C, H, W = shape
    D, eps = C * H * W, _eps(shape)
    eps_p = R.eps_p(eps)
    x0 = _images(shape, 7)
    sizes = R.L2.schedule(NQ_TABLE, H, W)
    steps = _script(B, len(sizes))
    # on the CPU, with the reference alone: the invariant holds for these inputs (start and every scripted proposal)
    xb = [R.start(x0[b], b, eps, SEED)[0] for b in range(B)]
    for b in range(B):
        assert xb[b].min() >= 0 and xb[b].max() <= 1 and R.l1_excess(xb[b].reshape(1, -1), x0[b].reshape(1, -1), eps_p) <= D * 2.0 ** -23
        for i in sorted({it for it, _, _ in steps if it < len(sizes)}):
            z, _, _ = R.propose(xb[b], x0[b], eps, SEED, i, b, sizes[i])
            assert z.min() >= 0 and z.max() <= 1 and R.l1_excess(z.reshape(1, -1), x0[b].reshape(1, -1), eps_p) <= D * 2.0 ** -23

    runs = {p: _run_kernels(ops, shape, x0, eps, p, False, steps) for p in ("auto", "resident", "streaming") if not (p == "resident" and D > RESIDENT)}
    runs["unaligned"] = _run_kernels(ops, shape, x0, eps, "auto", True, steps)
    got = runs["auto"]
    for name, r in runs.items():  # paths and alignments: the same bits
        for k, (a, ref) in enumerate(zip(r, got)):
            assert all(p is None and q is None or np.array_equal(_bits(p), _bits(q)) for p, q in zip(a, ref)), (name, k)

    # the start
    x_best, x_new, _, scal = got[0]
    ud = np.stack([R.start_point(x0[b], b, SEED) for b in range(B)])
    for b in range(B):
        z, info = R.project(ud[b], x0[b], eps_p, lam=scal[0, b])
        assert np.array_equal(_bits(x_new[b]), _bits(z)) and np.array_equal(_bits(x_best[b]), _bits(z)), b
        _check_scal(scal, b, info, x_new[b], x0[b])
    zp, sp = ops.l1_proj(_dev(ud), _dev(x0), eps_p)
    assert np.array_equal(_bits(zp.cpu().numpy()), _bits(x_new)) and np.array_equal(_bits(sp[:4].cpu().numpy()), _bits(scal))
    assert np.isfinite(x_new).all() and x_new.min() >= 0 and x_new.max() <= 1

    # the script
    rb, rn = [x_new[b].copy() for b in range(B)], [x_new[b].copy() for b in range(B)]
    proposed = 0
    for k, (it, flags, fooled) in enumerate(steps):
        x_best, x_new, norms, scal = got[k + 1]
        us, who = [], []
        for b in range(B):
            if flags[b]:
                rb[b] = rn[b].copy()
            if fooled[b] or it >= len(sizes):  # no proposal: x_new is untouched, the rows are zero
                assert not norms[:, b].any() and not scal[:, b].any(), (k, b)
            else:
                u, own = R.proposal_point(rb[b], x0[b], eps, SEED, it, b, sizes[it], norms=norms[:, b])
                rn[b], info = R.project(u, x0[b], eps_p, lam=scal[0, b])
                assert max(R.ulps(norms[:, b], np.array(own, dtype=F))) <= 1, (k, b, norms[:, b], own)
                _check_scal(scal, b, info, x_new[b], x0[b])
                us.append(u)
                who.append(b)
                proposed += 1
            assert np.array_equal(_bits(x_best[b]), _bits(rb[b])), (k, b)
            assert np.array_equal(_bits(x_new[b]), _bits(rn[b])), (k, b)
            assert R.l1_excess(x_new[b].reshape(1, -1), x0[b].reshape(1, -1), eps_p) <= D * 2.0 ** -23, (k, b)
        assert np.isfinite(x_new).all() and x_new.min() >= 0 and x_new.max() <= 1
        if who:  # one definition, through the ABI: ee_l1_proj_f32 of the reference's u is the step's x_new and scal, bit for bit
            zp, sp = ops.l1_proj(_dev(np.stack(us)), _dev(x0[who]), eps_p)
            assert np.array_equal(_bits(zp.cpu().numpy()), _bits(x_new[who])), k
            assert np.array_equal(_bits(sp[:4].cpu().numpy()), _bits(scal[:, who])), k
    assert proposed >= 2 * (B - 1) and any(s[0, :].max() > 0 for _, _, _, s in got), "the ball must bind somewhere"
    # the frozen sample: bit-unchanged from its commit on
    last = B - 1
    for k in range(3, len(steps) + 1):
        assert np.array_equal(_bits(got[k][0][last]), _bits(got[2][0][last])) and np.array_equal(_bits(got[k][1][last]), _bits(got[2][1][last]))


def test_commit_only_edge_values_and_errors(ops):
    from eeadv import sqatk
    import eeadv._native as n
    shape = (2, 3, 9, 9)
    B, C, H, W = shape
    x0 = _images(shape, 3)
    sizes, s0, dsizes, eta, off, off0 = _tables(H, W)
    eta0 = eta[off0:off0 + s0 * s0].view(s0, s0)
    seed = torch.tensor([SEED], dtype=torch.int64, device=DEV)
    ones, zero = torch.ones(B, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    # n_sizes = 0 commits only
    xb, xn, c = _dev(x0 * 0.5), _dev(x0 * 0.25), _dev(x0)
    keep = xn.clone()
    norms, scal = ops.sqatk_step_l1_(xb, xn, c, torch.tensor([1, 0], dtype=torch.int32, device=DEV), ones, zero, None, None, None, seed, 1.0,
                                     sqatk.l1_eps_p(1.0))
    assert torch.equal(xb[0], keep[0]) and torch.equal(xb[1], _dev(x0 * 0.5)[1]) and torch.equal(xn, keep)
    assert not norms.any() and not scal.any()
    # eps = 0 returns x0, with no NaN
    f0 = torch.zeros(B, dtype=torch.int32, device=DEV)
    for path in ("resident", "streaming"):
        xb, xn = torch.full_like(c, float("nan")), torch.full_like(c, float("nan"))
        ops.sqatk_init_l1_(xb, xn, c, seed, eta0, 0.0, 0.0, path=path)
        assert torch.equal(xb, c) and torch.equal(xn, c)
        norms, scal = ops.sqatk_step_l1_(xb, xn, c, f0, ones, zero, dsizes, off, eta, seed, 0.0, 0.0, path=path)
        assert torch.equal(xn, c) and bool(torch.isfinite(norms).all()) and bool(torch.isfinite(scal).all())
    # error codes
    L = n.lib
    p = ctypes.c_void_p(4096)
    eps, nan, neg, big = ctypes.c_float(0.5), ctypes.c_float(float("nan")), ctypes.c_float(-0.5), ctypes.c_float(0.75)
    f = L.ee_sqatk_init_l1_f32  # x_best, x_new, x0, seed, eta, s0, scal, B, C, H, W, eps, eps_p, path, stream
    g = L.ee_sqatk_step_l1_f32  # 9 pointers, n_sizes, seed, norms, scal, B, C, H, W, eps, eps_p, path, stream
    five, nine = [p] * 5, [p] * 9
    for e, ep in ((neg, neg), (eps, neg), (eps, big), (nan, eps), (eps, nan)):
        assert f(*five, 1, p, 2, 3, 8, 8, e, ep, 0, None) == -2 and g(*nine, 5, p, p, p, 2, 3, 8, 8, e, ep, 0, None) == -2
    assert f(*five, 0, p, 2, 3, 8, 8, eps, eps, 0, None) == -2 and f(*five, 9, p, 2, 3, 8, 8, eps, eps, 0, None) == -2  # s0 out of range
    assert f(*five, 1, p, 2, 3, 8, 8, eps, eps, 3, None) == -2 and g(*nine, 5, p, p, p, 2, 3, 8, 8, eps, eps, -1, None) == -2  # no such path
    assert f(*five, 1, p, 2, 33, 8, 8, eps, eps, 0, None) == -3 and g(*nine, 5, p, p, p, 2, 33, 8, 8, eps, eps, 0, None) == -3
    assert f(*five, 12, p, 2, 3, 64, 68, eps, eps, 1, None) == -3 and g(*nine, 5, p, p, p, 2, 3, 64, 68, eps, eps, 1, None) == -3  # resident past 12288
    assert f(*([None] * 5), 1, None, 0, 3, 8, 8, eps, eps, 0, None) == 0 and g(*([None] * 9), 0, None, None, None, 0, 3, 8, 8, eps, eps, 0, None) == 0
    assert f(*five, 1, None, 2, 3, 8, 8, eps, eps, 0, None) == -1 and g(*nine, 5, p, p, None, 2, 3, 8, 8, eps, eps, 0, None) == -1
    assert (n.K_SQATK_INIT, n.K_SQATK_MARGIN, n.K_SQATK_STEP) == (23, 24, 25)
    with pytest.raises(ValueError, match="path"):
        ops.sqatk_init_l1_(xb, xn, c, seed, eta0, 1.0, 1.0, path="fast")


# ---- engine ------------------------------------------------------------------------------------------------------------------------------
class _Linear(nn.Module):
    def __init__(self, D, K=10, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.w = nn.Parameter(torch.randn(K, D, generator=g) * 0.3)

    def forward(self, x):
        return torch.nn.functional.linear(x.flatten(1), self.w)


def _problem(shape):
    B, C, H, W = shape
    m = _Linear(C * H * W).to(DEV).eval()
    x = torch.from_numpy(_images(shape, 11)).to(DEV)
    with torch.no_grad():
        y = m(x).argmax(1)
    y[0] = (y[0] + 1) % 10  # one sample starts misclassified
    return m, x, y


N_QUERIES = 40  # 39 proposals: two replays of a 16-iteration graph and an eager remainder of 7


@pytest.mark.parametrize("shape", SHAPES[:3], ids=_ids)
def test_eager_trace_against_the_reference(shape):
    from eeadv import engine
    m, x, y = _problem(shape)
    B, D, eps = shape[0], x[0].numel(), _eps(shape)
    trace = []
    xa, robust, queries = engine.square_l1_loop(m, x, y, N_QUERIES, eps, seed=SEED, use_graph=False, trace=trace, early_exit=False)
    assert len(trace) == N_QUERIES and "norms" not in trace[0] and all(k in t for t in trace[1:] for k in ("x_best_in", "x_new_in", "norms", "scal", "x_new"))
    assert [t["counter"] for t in trace[1:]] == list(range(N_QUERIES - 1))
    x0 = x.cpu().numpy()
    margins = torch.stack([t["margin"] for t in trace]).cpu().numpy()
    samples, flags, _ = R.run(x0, y.cpu().numpy(), N_QUERIES, eps, SEED, margins=margins, lam0=trace[0]["scal"][0].cpu().numpy(),
                              norms=[t["norms"].cpu().numpy() for t in trace[1:]], lam=[t["scal"][0].cpu().numpy() for t in trace[1:]])
    assert torch.stack([t["flags"] for t in trace]).cpu().bool().tolist() == flags
    assert sum(sum(f) for f in flags[1:]) >= 1, "no proposal accepted: the run shows nothing"
    for b, s in enumerate(samples):
        for q in range(N_QUERIES):
            assert np.array_equal(trace[q]["x_new"][b].cpu().numpy(), s.iterates[q]), (b, q)
        assert bool(robust[b]) == s.robust and int(queries[b]) == s.queries
        assert np.array_equal(xa[b].cpu().numpy(), x0[b] if s.robust else s.x_best), b
    assert not bool(robust[0]) and int(queries[0]) == 1
    for t in trace[2:]:  # the sample that started misclassified: frozen, its rows zero
        assert torch.equal(t["x_new"][0], trace[0]["x_new"][0]) and not bool(t["norms"][:, 0].any()) and not bool(t["scal"][:, 0].any())
    assert R.l1_excess(xa.cpu().numpy().reshape(B, -1), x0.reshape(B, -1), R.eps_p(eps)) <= D * 2.0 ** -23


@pytest.mark.parametrize("shape", SHAPES[3:], ids=_ids)
def test_graph_replay_and_early_exit_equal_eager(shape, monkeypatch):
    from eeadv import engine
    m, x, y = _problem(shape)
    eps = _eps(shape)
    eager = engine.square_l1_loop(m, x, y, N_QUERIES, eps, seed=SEED, use_graph=False)
    for _ in range(2):  # the capture, then a second run on the cached graph
        graph = engine.square_l1_loop(m, x, y, N_QUERIES, eps, seed=SEED, use_graph=True)
        assert all(torch.equal(a, b) for a, b in zip(eager, graph))
    assert any(k[0] == "square_l1" for k in engine._GRAPHS)
    assert torch.equal(eager[0][eager[1]], x[eager[1]])
    monkeypatch.setattr(engine, "SQUARE_CHECK_EVERY", 16)
    y_wrong = (y + 1) % 10
    for yy in (y, y_wrong):
        for use_graph in (False, True):
            on = engine.square_l1_loop(m, x, yy, N_QUERIES, eps, seed=SEED, use_graph=use_graph, early_exit=True)
            off = engine.square_l1_loop(m, x, yy, N_QUERIES, eps, seed=SEED, use_graph=use_graph, early_exit=False)
            assert all(torch.equal(a, b) for a, b in zip(on, off))
    for norm in ("Linf", "L2"):  # the other doors: a same-seed rerun returns the same bits, eager and replayed
        e = 8 / 255 if norm == "Linf" else 0.5
        a = engine.square_loop(m, x, y, N_QUERIES, e, seed=SEED, use_graph=False, norm=norm)
        b = engine.square_loop(m, x, y, N_QUERIES, e, seed=SEED, use_graph=True, norm=norm)
        assert all(torch.equal(p, q) for p, q in zip(a, b))
    with pytest.raises(ValueError, match="norm"):
        engine.square_loop(m, x, y, N_QUERIES, eps, seed=SEED, norm="L1")
    engine.clear_graphs()


def test_linf_and_l2_square_loops_return_what_the_commit_before_returned():
    """tests/golden/square_loop.npz was recorded by tests/golden/make_square_loop_golden.py on the commit before this attack existed."""
    import importlib.util
    from eeadv import engine
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("make_square_loop_golden", os.path.join(here, "golden", "make_square_loop_golden.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    want = np.load(os.path.join(here, "golden", "square_loop.npz"))
    for norm in G.RADII:
        eager = G.run(torch, engine, norm)
        assert not want[norm + "_robust"][0] and want[norm + "_queries"].max() == G.N_QUERIES, "the fixture must hold a full run"
        for k, v in eager.items():
            assert v.dtype == want[k].dtype and np.array_equal(v.view(np.uint8), want[k].view(np.uint8)), k
        for k, v in G.run(torch, engine, norm, use_graph=True).items():
            assert np.array_equal(v.view(np.uint8), want[k].view(np.uint8)), (k, "graph")
    engine.clear_graphs()


# ---- drivers -----------------------------------------------------------------------------------------------------------------------------
def test_ensemble_through_the_dispatch_on_the_device():
    import utils.attacks as A
    from eeadv import trainer
    torch.manual_seed(0)
    model = TinyNet(3, 8, 10, seed=0).to(DEV).eval()
    x = torch.rand(8, 3, 8, 8, device=DEV)
    with torch.no_grad():
        y = model(x).argmax(1)
    eps = 192 / 64.0
    acc = {}
    for method in ("Square-L1", "APGD-L1+FAB", "APGD-L1+FAB+Square"):
        a = Args(epsilon=eps, method_name="AT", attack_method=method, random=True, fab_iters=3, square_queries=12)
        assert trainer.norm_tag(a) == " [norm L1]"
        torch.manual_seed(1)
        out = trainer.attack_for_validation(model, a, x, y, DEV, 4, 0.1, 10)
        assert out.shape == x.shape and float(out.min()) >= 0 and float(out.max()) <= 1
        assert float((out - x).flatten(1).abs().double().sum(dim=1).max()) <= eps * (1 + 192 * 2.0 ** -23), method
        with torch.no_grad():
            acc[method] = int((model(out).argmax(1) == y).sum())
    assert acc["APGD-L1+FAB+Square"] <= acc["APGD-L1+FAB"]
    xa, robust, queries = A.Square_L1(model, Args(epsilon=eps), x, y, n_queries=12, seed=SEED)
    again = A.Square_L1(model, Args(epsilon=eps), x, y, n_queries=12, seed=SEED)
    assert all(torch.equal(p, q) for p, q in zip((xa, robust, queries), again)) and queries.dtype == torch.int32
    assert torch.equal(xa[robust], x[robust])


@pytest.mark.parametrize("method", ["Square-L1", "APGD-L1+FAB+Square"])
def test_mnist_driver_evaluates_with_l1_square(tmp_path, method):
    """The driver itself, on the device: argparse, the L1_METHODS validation, --square_queries / --fab_iters and the tagged final line."""
    cfg = open(os.path.join(PKG, "MNIST", "configs_mnist", "adversarial_training.yml")).read()
    cfg = re.sub(r"num_steps_(\d): \d+", r"num_steps_\1: 2", cfg)
    cfg = re.sub(r"batch_size: \d+", "batch_size: 8", cfg)
    path = tmp_path / "l1.yml"
    path.write_text(cfg)
    r = subprocess.run([sys.executable, "experiments_mnist.py", "-c", str(path), "--data", "synthetic:1:1", "--output-root", str(tmp_path), "-e",
                        "--attack_method", method, "--fab_iters", "2", "--square_queries", "12"], cwd=os.path.join(PKG, "MNIST"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    logs = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path)) for f in fs if f.startswith("log")]
    text = r.stdout + "".join(open(f).read() for f in logs)
    clean = re.findall(r"^ \* Clean Prec@1 ([\d.]+) Prec@5 ([\d.]+)$", text, flags=re.M)
    adv = re.findall(r"^ \* Adv Prec@1 ([\d.]+) Prec@5 ([\d.]+) \[norm L1\]$", text, flags=re.M)
    assert len(clean) >= 1 and len(adv) >= 1
    assert all(float(a1) <= float(c1) for (c1, _), (a1, _) in zip(clean, adv))
