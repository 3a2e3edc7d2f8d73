"""GPU: the Square attack kernels (ee_sqatk.hip) and engine.square_loop against tests/square_reference.py.

Bit-exact throughout: the start, the proposals and the commits are fp32 on both sides with the same operations in the same order, the
margin is one fp32 difference of two inputs, and the draws are integers."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import square_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")
EPS = 16 / 255


@pytest.fixture(scope="module")
def ops():
    from eeadv import ops
    return ops


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _seed(s):
    return torch.tensor([s], dtype=torch.int64, device=DEV)


def _images(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, C, H, W, generator=g)
    x0.view(-1)[::5] = 0.0  # the ends of [0, 1]: the clamp cuts the ball
    x0.view(-1)[2::5] = 1.0
    return x0


SHAPES = [(1, 1, 5, 7), (3, 3, 8, 8), (2, 1, 28, 28), (3, 3, 9, 130)]


# ---- start and step ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_init_and_step_kernels_bit_exact(ops, shape):
    """The last shape has W % 4 != 0, C*H*W % 4 != 0 (a 16-byte access straddles rows, channels and samples) and two 128-column stripe
    words.  Two flag patterns per size: alternating accept / reject with the last sample fooled and NOT flagged (nothing of it may be
    touched), then the opposite flags with sample 0 fooled AND flagged (its commit happens, its x_new stays)."""
    B, C, H, W = shape
    seed = 0x1234567 + H
    x0 = _images(B, C, H, W, 10 * H + W)
    x0n = x0.numpy()
    xb_d, xn_d = torch.full(shape, -7.0, device=DEV), torch.full(shape, -7.0, device=DEV)
    ops.sqatk_init_(xb_d, xn_d, x0.to(DEV), _seed(seed), EPS)
    start = np.stack([R.start_point(x0n[b], b, EPS, seed) for b in range(B)])
    assert np.array_equal(xb_d.cpu().numpy(), start) and np.array_equal(xn_d.cpu().numpy(), start)
    assert (start == 0).any() and (start == 1).any()
    g = torch.Generator().manual_seed(H)
    e32 = np.float32(EPS)
    x_new = np.clip(np.minimum(np.maximum(start + ((torch.rand(shape, generator=g).numpy() * 2 - 1) * e32).astype(np.float32), x0n - e32), x0n + e32), 0, 1)
    it = 3
    for s in sorted({1, 3, min(H, W)}):
        sizes = _i32([min(H, W), 2, 1, s, 1])
        for pattern in (0, 1):
            flags = [(b + pattern) % 2 == 0 for b in range(B)]
            fooled = [(b == B - 1 and B > 1) if pattern == 0 else b == 0 for b in range(B)]
            if pattern == 0 and B > 1:
                flags[B - 1] = False
            if pattern == 1:
                flags[0] = True
            mm = torch.tensor([-0.5 if f else 0.25 for f in fooled])
            want_b, want_n = start.copy(), x_new.copy()
            for b in range(B):
                if flags[b]:
                    want_b[b] = x_new[b]
                if not fooled[b]:
                    want_n[b] = R.propose(want_b[b], x0n[b], EPS, *R.window(seed, it, b, H, W, s)[:2], s, R.window(seed, it, b, H, W, s)[2])
            for offset in ((0, 1) if shape == (3, 3, 9, 130) and s == 3 else (0,)):  # offset 1: bases off 16 bytes, the scalar kernel
                n = x0.numel()
                bufs = [torch.zeros(n + 4, device=DEV)[offset:offset + n].view(shape) for _ in range(3)]
                for t, src in zip(bufs, (start, x_new, x0n)):
                    t.copy_(torch.from_numpy(src))
                assert all(t.is_contiguous() and (t.data_ptr() % 16 == 0) == (offset == 0) for t in bufs)
                ops.sqatk_step_(bufs[0], bufs[1], bufs[2], _i32([int(f) for f in flags]), mm.to(DEV), _i32([it]), sizes, _seed(seed), EPS)
                assert np.array_equal(bufs[0].cpu().numpy(), want_b), (s, pattern, offset)
                assert np.array_equal(bufs[1].cpu().numpy(), want_n), (s, pattern, offset)
            if pattern == 0 and B > 1:
                assert np.array_equal(want_b[B - 1], start[B - 1]) and np.array_equal(want_n[B - 1], x_new[B - 1])
            # a counter outside the table (either side), or no table: commit only
            for counter, table in ((5, sizes), (-1, sizes), (it, None)):
                b_d, n_d = torch.from_numpy(start).to(DEV), torch.from_numpy(x_new).to(DEV)
                ops.sqatk_step_(b_d, n_d, x0.to(DEV), _i32([int(f) for f in flags]), mm.to(DEV), _i32([counter]), table, _seed(seed), EPS)
                assert np.array_equal(b_d.cpu().numpy(), want_b) and np.array_equal(n_d.cpu().numpy(), x_new), (s, pattern, counter)


def test_step_and_init_launch_nothing_on_an_empty_batch(ops):
    e = torch.empty(0, 3, 8, 8, device=DEV)
    z = torch.empty(0, device=DEV)
    ops.sqatk_init_(e, e.clone(), e.clone(), _seed(1), EPS)
    ops.sqatk_step_(e, e.clone(), e.clone(), z.int(), z, _i32([0]), _i32([3, 2]), _seed(1), EPS)
    counter = _i32([4])
    ops.sqatk_margin_(torch.empty(0, 10, device=DEV), z.long(), z.clone(), z.clone(), z.int(), z.int(), counter)
    torch.cuda.synchronize()
    assert int(counter.item()) == 4


def test_wrapper_refuses_what_the_kernels_do_not_take(ops):
    from eeadv import _native as N
    x = torch.zeros(2, 33, 4, 4, device=DEV)
    with pytest.raises(N.EEError, match="not supported"):
        ops.sqatk_init_(x, x.clone(), x.clone(), _seed(1), EPS)
    z = torch.zeros(2, 1, device=DEV)
    with pytest.raises(N.EEError, match="out of range"):
        ops.sqatk_margin_(z, torch.zeros(2, dtype=torch.int64, device=DEV), z[:, 0].clone(), z[:, 0].clone(), _i32([0, 0]), _i32([0, 0]), _i32([0]))


# ---- margin --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5, 130])
@pytest.mark.parametrize("K", [2, 10, 200, 1000])
def test_margin_kernel(ops, B, K):
    g = torch.Generator().manual_seed(1000 * B + K)
    z = 3 * torch.randn(B, K, generator=g)
    y = torch.randint(0, K, (B,), generator=g)
    y[1::2] = z[1::2].argmax(1)  # odd rows: the label is the prediction (positive margins); even rows: a random label (negative ones)
    nan, inf = float("nan"), float("inf")
    if B >= 5:
        y[0], y[1] = 0, K - 1  # label first / last
        z[2, :] = -1.0
        z[2, 0] = z[2, K - 1] = 2.5  # tied maxima
        y[2] = 0
        z[3, K - 1] = nan
        z[4, 0], z[4, K - 1], y[4] = inf, -inf, 0
    if B == 130:
        y[5] = K  # labels outside the row
        y[6] = -1
        z[7, :] = inf  # inf - inf
        y[8] = K - 1
        z[8, K - 1] = nan  # the NaN is the label's own logit
        z[9, 0], y[9] = -inf, 0
    z64 = z.double().numpy()
    want = np.empty(B, dtype=np.float32)
    for b in range(B):
        yb = int(y[b])
        if not 0 <= yb < K or np.isnan(z64[b]).any():
            want[b] = np.nan
        else:
            with np.errstate(invalid="ignore"):
                want[b] = np.float32(z64[b, yb] - np.max(np.delete(z64[b], yb)))  # the exact difference, rounded once
    # state: not fooled and far above / fooled although the new margin is lower / equal to the new margin / just above it
    mm0 = np.full(B, np.inf, dtype=np.float32)
    for b in range(B):
        k = b % 4
        if k == 1:
            mm0[b] = -100.0
        elif k == 2 and not np.isnan(want[b]):
            mm0[b] = want[b]
        elif k == 3 and np.isfinite(want[b]):
            mm0[b] = np.nextafter(want[b], np.float32(np.inf))
    q0 = (np.arange(B) * 3 % 11).astype(np.int32)
    mo, mm, q = torch.full((B,), -9.0, device=DEV), torch.from_numpy(mm0).to(DEV), torch.from_numpy(q0).to(DEV)
    flags, counter = torch.full((B,), 5, dtype=torch.int32, device=DEV), _i32([41])
    ops.sqatk_margin_(z.to(DEV), y.to(DEV), mo, mm, q, flags, counter)
    assert int(counter.item()) == 42
    ops.sqatk_margin_(z.to(DEV), y.to(DEV), mo.clone(), mm.clone(), q.clone(), flags.clone(), counter)
    assert int(counter.item()) == 43
    assert np.array_equal(mo.cpu().numpy(), want, equal_nan=True)
    active = ~(mm0 <= 0)
    with np.errstate(invalid="ignore"):
        accept = active & (want < mm0)
    assert flags.cpu().numpy().tolist() == accept.astype(np.int32).tolist()
    assert np.array_equal(mm.cpu().numpy(), np.where(accept, want, mm0))
    assert q.cpu().numpy().tolist() == (q0 + active).tolist()
    if B >= 5:
        assert want[2] == 0.0  # tied maxima: the label holds one of them, the other is subtracted
        assert np.isnan(want[3]) and not accept[3] and want[4] == np.inf and not accept[4]
    if B == 130:
        assert np.isnan(want[5:9]).all() and not accept[5:9].any() and want[9] == -np.inf
        assert accept[0::4].any() and not accept[0::4].all() and not accept[1::4].any() and not accept[2::4].any() and accept[3::4].any()


# ---- teacher-forced trajectory -------------------------------------------------------------------------------------------------------
def test_teacher_forced_trajectory():
    """B = 4, 3 x 8 x 8, 40 iterations.  The classifier is replaced by a recorded sequence: logits [m, 0] with label 0 have the margin m.
       0: a falling staircase with plateaus and rises (accepts and rejects);   1: fooled at iteration 7, lower margins afterwards (frozen);
       2: a NaN at iteration 5 and a value equal to its best at 9;              3: never below its start (all rejects)."""
    from eeadv import engine
    B, n_it, seed = 4, 40, 99
    x0 = _images(B, 3, 8, 8, 3)
    seq = np.empty((n_it + 1, B), dtype=np.float32)
    rng = np.random.default_rng(4)
    seq[:, 0] = 5.0 - 0.1 * np.arange(n_it + 1) + rng.choice([0.0, 0.35], n_it + 1)
    seq[:, 1] = 3.0 + rng.random(n_it + 1)
    seq[8:, 1] = -1.0 - 0.1 * np.arange(n_it + 1 - 8)  # forward 8 = the one of iteration 7 (forward 0 is the start)
    seq[:, 2] = 2.0 - 0.03 * np.arange(n_it + 1) * rng.choice([1.0, -1.0], n_it + 1)
    seq[6, 2] = np.nan
    seq[10, 2] = seq[:10, 2][~np.isnan(seq[:10, 2])].min()
    seq[:, 3] = 1.0 + rng.random(n_it + 1)
    seq[0, 3] = 0.5
    feed = iter(torch.from_numpy(np.stack([seq, np.zeros_like(seq)], axis=2)).to(DEV))
    run = engine._SquareRun(x0.to(DEV), torch.zeros(B, dtype=torch.int64), n_it + 1, EPS)
    run.load(x0.to(DEV), torch.zeros(B, dtype=torch.int64, device=DEV), seed)
    samples = [R.Sample(x0[b].numpy(), b, n_it + 1, EPS, seed) for b in range(B)]
    model = lambda x: next(feed)  # noqa: E731

    def check(where):
        run.finish()  # the commit of the flags just written (the next step repeats it: it is idempotent)
        for b, s in enumerate(samples):
            assert np.array_equal(run.x_best[b].cpu().numpy(), s.x_best), (where, b, "x_best")
            assert np.array_equal(run.x_new[b].cpu().numpy(), s.x_new), (where, b, "x_new")
        assert np.array_equal(run.margin_min.cpu().numpy(), np.array([s.margin_min for s in samples], dtype=np.float32)), where
        assert run.queries.cpu().tolist() == [s.queries for s in samples] and run.flags.cpu().tolist() == [int(s.flag) for s in samples], where
        assert np.array_equal(run.margin_out.cpu().numpy(), seq[where], equal_nan=True)
        assert int(run.counter.item()) == where

    run.start(model)
    flags = [[s.observe(seq[0, b]) for b, s in enumerate(samples)]]
    check(0)
    for i in range(n_it):
        run.iteration(model)
        for s in samples:
            s.advance()
        flags.append([s.observe(seq[i + 1, b]) for b, s in enumerate(samples)])
        check(i + 1)
    col = lambda b: [f[b] for f in flags]  # noqa: E731
    assert all(flags[0]) and any(col(0)[1:]) and not all(col(0)[1:])
    assert col(1)[8] and not any(col(1)[9:]) and samples[1].queries == 9 and samples[1].margin_min == seq[8, 1]
    assert not col(2)[6] and not col(2)[10] and samples[2].queries == n_it + 1
    assert not any(col(3)[1:]) and np.array_equal(samples[3].x_best, R.start_point(x0[3].numpy(), 3, EPS, seed))
    x_adv, robust, queries = run.result()
    assert robust.cpu().tolist() == [True, False, True, True] and torch.equal(x_adv[0].cpu(), x0[0]) and queries.dtype == torch.int32
    assert np.array_equal(x_adv[1].cpu().numpy(), samples[1].x_best)


# ---- free-running on the ResNets -----------------------------------------------------------------------------------------------------
N_QUERIES = 49  # 48 proposals: three replays of a 16-iteration graph


def _resnet(kind):
    from eeadv import models
    torch.manual_seed(5)
    if kind == "resnet18":
        m = models.make_resnet(18, "tiny")
    else:
        m = models.make_resnet_ee(18, "tiny", kind == "resnet18_EE_square", cize=64, r=8, w=1.0, with_gf=False, low=38.0, high=76.0, alpha=0.0,
                                  sigma=1.0, type_canny="CannyFilter_step125_1", epsilon=EPS, n_queries=1)
    return m.to(DEV).eval()


def _batch(m, seed, B=4):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 3, 64, 64, generator=g).to(DEV)
    with torch.no_grad():
        z = m(x)
    y = z.argmax(1)
    y[0] = (y[0] + 1) % 200  # one sample starts misclassified
    return x, y


def _valid(xa, x0):
    e = torch.tensor(EPS, dtype=torch.float32)
    assert bool((xa >= x0 - e).all()) and bool((xa <= x0 + e).all()) and bool((xa >= 0).all()) and bool((xa <= 1).all())


@pytest.mark.parametrize("kind", ["resnet18", "resnet18_EE"])
def test_free_running(kind, monkeypatch):
    from eeadv import engine
    m = _resnet(kind)
    was_training = m.training
    x, y = _batch(m, 1)
    seed = 4242
    # eager, piece by piece, with the trace
    run = engine._SquareRun(x, y, N_QUERIES, EPS)
    run.trace = trace = []
    run.load(x, y, seed)
    run.start(m)
    for _ in range(N_QUERIES - 1):
        run.iteration(m)
    run.finish()
    run.trace = None
    assert len(trace) == N_QUERIES and int(run.counter.item()) == N_QUERIES - 1
    xa, robust, queries = run.result()
    # the trace's margins through the reference
    seen = torch.stack([t["margin"] for t in trace]).cpu().numpy()
    samples, flags, _ = R.run(x.cpu().numpy(), y.cpu().numpy(), N_QUERIES, EPS, seed, margins=seen)
    assert torch.stack([t["flags"] for t in trace]).cpu().bool().tolist() == flags
    for b, s in enumerate(samples):
        assert np.array_equal(run.x_best[b].cpu().numpy(), s.x_best), b
        assert all(a >= c for a, c in zip(s.history, s.history[1:])), "margin_min never rises"
    assert queries.cpu().tolist() == [s.queries for s in samples] and robust.cpu().tolist() == [s.robust for s in samples]
    assert np.array_equal(run.margin_min.cpu().numpy(), np.array([s.margin_min for s in samples], dtype=np.float32))
    assert not bool(robust[0]) and int(queries[0]) == 1
    assert sum(sum(f) for f in flags[1:]) >= 1, "no proposal accepted: the run shows nothing"
    _valid(xa.cpu(), x.cpu())
    assert torch.equal(xa[robust], x[robust]) and torch.equal(xa[~robust], run.x_best[~robust])
    # the loop: eager equals the pieces, the graph equals eager, a second replay on new inputs equals a fresh eager run
    for use_graph in (False, True, True):
        got = engine.square_loop(m, x, y, N_QUERIES, EPS, seed=seed, use_graph=use_graph)
        assert torch.equal(got[0], xa) and torch.equal(got[1], robust) and torch.equal(got[2], queries), use_graph
    x2, y2 = _batch(m, 2)
    e2 = engine.square_loop(m, x2, y2, N_QUERIES, EPS, seed=seed + 1, use_graph=False)
    g2 = engine.square_loop(m, x2, y2, N_QUERIES, EPS, seed=seed + 1, use_graph=True)
    assert all(torch.equal(a, b) for a, b in zip(e2, g2))
    # the seed: the same one agrees (above), another one differs
    t2 = []
    engine.square_loop(m, x, y, N_QUERIES, EPS, seed=seed + 1, use_graph=False, trace=t2)
    assert not np.array_equal(torch.stack([t["margin"] for t in t2]).cpu().numpy(), seen, equal_nan=True)
    # the early exit: with a check every 16 iterations and every sample fooled by the start, the loop stops at the first check
    monkeypatch.setattr(engine, "SQUARE_CHECK_EVERY", 16)
    y_wrong = (y2 + 1) % 200
    y_wrong[0] = y2[0]  # (sample 0's label was wrong already)
    calls = []
    monkeypatch.setattr(engine._SquareRun, "any_active", lambda self, f=engine._SquareRun.any_active: calls.append(1) or f(self))
    for yy in (y_wrong, y2):
        for use_graph in (False, True):
            del calls[:]
            on = engine.square_loop(m, x2, yy, N_QUERIES, EPS, seed=seed, use_graph=use_graph, early_exit=True)
            n_on = len(calls)
            off = engine.square_loop(m, x2, yy, N_QUERIES, EPS, seed=seed, use_graph=use_graph, early_exit=False)
            assert all(torch.equal(a, b) for a, b in zip(on, off)) and len(calls) == n_on
            assert n_on >= 1
            if yy is y_wrong:
                assert n_on == 1 and on[2].cpu().tolist() == [1, 1, 1, 1] and not bool(on[1].any())
    assert m.training == was_training
    with pytest.raises(ValueError):
        engine.square_loop(m, x, y, N_QUERIES, EPS, seed=seed, use_graph=True, trace=[])
    engine.clear_graphs()


def test_randomised_defence_invariants():
    """resnet18_EE_square redraws its Add_Square at every forward, so no trajectory can be replayed: the run must finish, stay inside the
    ball and the unit box, count its forwards, keep robust rows clean and report margin_min as the smallest accepted margin."""
    from eeadv import engine
    m = _resnet("resnet18_EE_square")
    x, y = _batch(m, 3)
    for use_graph in (False, True):
        trace = None if use_graph else []
        xa, robust, queries = engine.square_loop(m, x, y, N_QUERIES, EPS, seed=7, use_graph=use_graph, trace=trace)
        _valid(xa.cpu(), x.cpu())
        assert torch.equal(xa[robust], x[robust]) and bool((queries >= 1).all()) and bool((queries <= N_QUERIES).all())
        assert bool((queries[robust] == N_QUERIES).all())
        if trace is not None:
            best = torch.full((4,), float("inf"), device=DEV)
            for t in trace:
                acc = t["flags"].bool()
                assert bool((t["margin"][acc] < best[acc]).all()) and not bool(acc[best <= 0].any())
                best = torch.where(acc, t["margin"], best)
            assert torch.equal(best > 0, robust)
    engine.clear_graphs()


# ---- driver --------------------------------------------------------------------------------------------------------------------------
def test_tiny_imagenet_driver_evaluates_with_square(tmp_path):
    cfg = open(os.path.join(PKG, "Tiny_ImageNet", "configs_tinyimagenet", "adversarial_training.yml")).read()
    cfg = re.sub(r"num_steps_(\d): \d+", r"num_steps_\1: 2", cfg).replace("batch_size: 100", "batch_size: 8").replace("print_freq: 50", "print_freq: 1")
    path = tmp_path / "square.yml"
    path.write_text(cfg)
    r = subprocess.run([sys.executable, "experiments_tinyimagenet.py", "-c", str(path), "--output-root", str(tmp_path), "--data", "synthetic:1:1",
                        "-e", "--attack_method", "Square", "--square_queries", "20"], cwd=os.path.join(PKG, "Tiny_ImageNet"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    logs = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path)) for f in fs if f.startswith("log")]
    text = r.stdout + "".join(open(f).read() for f in logs)
    clean = re.findall(r"^ \* Clean Prec@1 ([\d.]+) Prec@5 ([\d.]+)$", text, flags=re.M)
    adv = re.findall(r"^ \* Adv Prec@1 ([\d.]+) Prec@5 ([\d.]+)$", text, flags=re.M)
    assert len(clean) >= 1 and len(clean) == len(adv)
    for (c1, _), (a1, _) in zip(clean, adv):
        assert float(a1) <= float(c1)
