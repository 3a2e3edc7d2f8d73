"""GPU: the L2 Square kernels (ee_sqatk_l2.hip) and engine.square_loop(norm="L2") against tests/square_l2_reference.py.

Given the norms a kernel emitted, every element it wrote must equal the reference bit for bit, and every emitted norm must be within one
unit in the last place of the exactly summed norm of the reference's elements at that stage.  The start emits no norm: there the
reference is given, in turn, the exact norm and its two float32 neighbours, and one of the three must reproduce the kernel's bits."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import square_l2_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 0.5
SEED = 20260
# (3,3,9,9): element-wise, the window is the image at the first sizes; (2,1,28,28): vector; (3,3,16,20): non-square; (2,3,64,64): the
# resident limit; (2,3,64,68): auto takes the streaming path
SHAPES = [(3, 3, 9, 9), (2, 1, 28, 28), (3, 3, 16, 20), (2, 3, 64, 64), (2, 3, 64, 68)]
_ids = lambda s: "x".join(map(str, s))


@pytest.fixture(scope="module")
def ops():
    from eeadv import ops
    return ops


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _images(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(*shape, generator=g)
    x0.view(-1)[::5] = 0.0  # the ends of [0, 1]: the clamp cuts the ball
    x0.view(-1)[2::5] = 1.0
    return x0


def _tables(n_queries, H, W):
    from eeadv import sqatk
    sizes = sqatk.square_schedule_l2(n_queries, H, W)
    assert sizes == R.schedule(n_queries, H, W)
    s0 = sqatk.start_size(H, W)
    eta, eta_off, off0 = sqatk.eta_tables(sizes, s0)
    return sizes, s0, torch.from_numpy(eta).to(DEV), torch.from_numpy(eta_off).to(DEV), off0


def _reference_start(x0, b, kernel_start):
    """The reference's start that reproduces the kernel's bits, with the norm it took: the exact one or a neighbour."""
    exact = R.start(x0, b, EPS, SEED)[1][0]
    for n0 in (exact, np.nextafter(exact, np.float32(0)), np.nextafter(exact, np.float32(np.inf))):
        got = R.start(x0, b, EPS, SEED, [n0])[0]
        if np.array_equal(got, kernel_start):
            return got, n0
    raise AssertionError("sample %d: no norm within one ulp of %r reproduces the kernel's start" % (b, exact))


class _Launch:
    """One state of the attack's buffers on the device, the two L2 launches on it, and the same state in the reference."""

    def __init__(self, ops, shape, path="auto", offset=0):
        B, C, H, W = shape
        self.ops, self.shape, self.path = ops, shape, path
        self.sizes, s0, self.eta, self.eta_off, off0 = _tables(40, H, W)
        self.eta0 = self.eta[off0:off0 + s0 * s0].view(s0, s0)
        n = B * C * H * W
        bufs = [torch.full((n + 4,), -7.0, device=DEV)[offset:offset + n].view(shape) for _ in range(3)]
        self.xb, self.xn, self.x0 = bufs
        self.x0_host = _images(shape, 3)
        self.x0.copy_(self.x0_host)
        self.seed = torch.tensor([SEED], dtype=torch.int64, device=DEV)
        self.sizes_d = _i32(self.sizes)
        self.norms = torch.full((3 + 2 * C, B), -1.0, device=DEV)

    def init(self):
        self.ops.sqatk_init_l2_(self.xb, self.xn, self.x0, self.seed, self.eta0, EPS, self.path)

    def step(self, i, flags, margin_min, commit_only=False):
        self.ops.sqatk_step_l2_(self.xb, self.xn, self.x0, _i32(flags), torch.tensor(margin_min, dtype=torch.float32, device=DEV), _i32([i]),
                                None if commit_only else self.sizes_d, self.eta_off, self.eta, self.seed, EPS, self.norms, self.path)

    def host(self):
        torch.cuda.synchronize()
        return self.xb.cpu().numpy(), self.xn.cpu().numpy(), self.norms.cpu().numpy()


# proposals 0 (the largest window), 1, and the last (the smallest); sample 1 accepts the first proposal, the last sample is fooled from
# the second step on
def _script(B):
    steps = []
    for k, i in enumerate((0, 1, 38)):
        flags = [1 if (k == 1 and b == 1) else 0 for b in range(B)]
        mm = [0.5] * B
        if k >= 1:
            mm[B - 1] = -0.25
        steps.append((i, flags, mm))
    return steps


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_kernels_against_the_reference(ops, shape):
    B, C, H, W = shape
    L = _Launch(ops, shape)
    L.init()
    xb, xn, _ = L.host()
    assert np.array_equal(xb, xn)
    x0 = L.x0_host.numpy()
    best = []
    for b in range(B):
        got, _ = _reference_start(x0[b], b, xb[b])
        best.append(got)
        assert got.min() >= 0 and got.max() <= 1
    new = [v.copy() for v in best]
    for i, flags, mm in _script(B):
        L.step(i, flags, mm)
        xb, xn, norms = L.host()
        for b in range(B):
            if flags[b]:
                best[b] = new[b].copy()
            assert np.array_equal(xb[b], best[b]), (i, b)
            if mm[b] <= 0:  # fooled: nothing of it is touched, its norms read zero
                assert np.array_equal(xn[b], new[b]) and not norms[:, b].any(), (i, b)
                continue
            new[b], own = R.propose(best[b], x0[b], EPS, SEED, i, b, L.sizes[i], norms=norms[:, b])
            assert np.array_equal(xn[b], new[b]), (i, b)
            worst = max(R.ulps(norms[:, b], np.array(own, dtype=np.float32)))
            assert worst <= 1, (i, b, norms[:, b], own)
            # the ball and the box
            excess = R.exact_norm(xn[b] - x0[b]) / EPS - 1
            assert excess <= 4 * 2.0 ** -23 and xn[b].min() >= 0 and xn[b].max() <= 1, (i, b, excess)
    # the commit alone: no table, the accepted proposal moves over and nothing else changes
    L.step(39, [1] * B, [0.5] * B, commit_only=True)
    xb, xn2, norms = L.host()
    assert np.array_equal(xb, xn) and np.array_equal(xn2, xn) and not norms.any()


@pytest.mark.parametrize("shape", SHAPES[:4], ids=_ids)
def test_paths_and_alignments_return_the_same_bits(ops, shape):
    B = shape[0]
    outs = []
    for path, offset in (("resident", 0), ("streaming", 0), ("resident", 1), ("streaming", 1), ("auto", 0)):
        L = _Launch(ops, shape, path, offset)
        assert (L.xb.data_ptr() % 16 == 0) == (offset == 0)
        L.init()
        got = [L.host()[0].copy()]
        for i, flags, mm in _script(B):
            L.step(i, flags, mm)
            got += [a.copy() for a in L.host()]
        outs.append(got)
    for other in outs[1:]:
        assert len(other) == len(outs[0]) and all(np.array_equal(a, b) for a, b in zip(outs[0], other))


def test_resident_path_ends_at_its_limit(ops):
    from eeadv import _native as N
    L = _Launch(ops, SHAPES[4], "resident")
    with pytest.raises(N.EEError):
        L.init()
    with pytest.raises(N.EEError):
        L.step(0, [0, 0], [0.5, 0.5])
    with pytest.raises(ValueError):
        ops.sqatk_init_l2_(L.xb, L.xn, L.x0, L.seed, L.eta0, EPS, "fast")
    torch.cuda.synchronize()


def test_eps_zero_returns_the_clean_image(ops):
    shape = SHAPES[0]
    L = _Launch(ops, shape)
    ops.sqatk_init_l2_(L.xb, L.xn, L.x0, L.seed, L.eta0, 0.0)
    ops.sqatk_step_l2_(L.xb, L.xn, L.x0, _i32([0] * 3), torch.full((3,), 0.5, device=DEV), _i32([0]), L.sizes_d, L.eta_off, L.eta, L.seed, 0.0,
                       L.norms)
    xb, xn, norms = L.host()
    assert np.array_equal(xb, L.x0_host.numpy()) and np.array_equal(xn, L.x0_host.numpy()) and np.isfinite(norms).all()


# ---- the engine ----------------------------------------------------------------------------------------------------------------------
class _Linear(nn.Module):
    """A tiny linear classifier: enough of a model for margins that move."""

    def __init__(self, D, K=10, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.w = nn.Parameter(torch.randn(K, D, generator=g) * 0.3)

    def forward(self, x):
        return torch.nn.functional.linear(x.flatten(1), self.w)


def _problem(shape):
    B, C, H, W = shape
    m = _Linear(C * H * W).to(DEV).eval()
    x = _images(shape, 11).to(DEV)
    with torch.no_grad():
        y = m(x).argmax(1)
    y[0] = (y[0] + 1) % 10  # one sample starts misclassified
    return m, x, y


N_QUERIES = 40  # 39 proposals: two replays of a 16-iteration graph and an eager remainder of 7


def _valid(xa, x0):
    xa, x0 = xa.cpu().numpy(), x0.cpu().numpy()
    for b in range(xa.shape[0]):
        assert R.exact_norm(xa[b] - x0[b]) / EPS - 1 <= 4 * 2.0 ** -23, b
    assert xa.min() >= 0 and xa.max() <= 1


@pytest.mark.parametrize("shape", SHAPES[:3], ids=_ids)
def test_eager_trace_against_the_reference(shape):
    from eeadv import engine
    m, x, y = _problem(shape)
    B = shape[0]
    trace = []
    xa, robust, queries = engine.square_loop(m, x, y, N_QUERIES, EPS, seed=SEED, use_graph=False, trace=trace, early_exit=False, norm="L2")
    assert len(trace) == N_QUERIES and "norms" not in trace[0] and all("norms" in t for t in trace[1:])
    assert [t["counter"] for t in trace[1:]] == list(range(N_QUERIES - 1))
    x0 = x.cpu().numpy()
    margins = torch.stack([t["margin"] for t in trace]).cpu().numpy()
    start = trace[1]["x_best_in"].cpu().numpy()  # the start: nothing was committed before proposal 0
    n0 = [[_reference_start(x0[b], b, start[b])[1] for b in range(B)]]
    norms = [t["norms"].cpu().numpy() for t in trace[1:]]
    samples, flags, _ = R.run(x0, y.cpu().numpy(), N_QUERIES, EPS, SEED, margins=margins, start_norms=n0, norms=norms)
    assert torch.stack([t["flags"] for t in trace]).cpu().bool().tolist() == flags
    assert sum(sum(f) for f in flags[1:]) >= 1, "no proposal accepted: the run shows nothing"
    for b, s in enumerate(samples):
        for q in range(1, N_QUERIES):
            assert np.array_equal(trace[q]["x_new"][b].cpu().numpy(), s.iterates[q]), (b, q)
        for i, own in s.norms:
            assert max(R.ulps(norms[i][:, b], np.array(own, dtype=np.float32))) <= 1, (b, i)
        assert bool(robust[b]) == s.robust and int(queries[b]) == s.queries
        assert np.array_equal(xa[b].cpu().numpy(), x0[b] if s.robust else s.x_best), b
    assert not bool(robust[0]) and int(queries[0]) == 1
    _valid(xa, x)


@pytest.mark.parametrize("shape", SHAPES[3:], ids=_ids)
def test_graph_replay_and_early_exit_equal_eager(shape, monkeypatch):
    from eeadv import engine
    m, x, y = _problem(shape)
    eager = engine.square_loop(m, x, y, N_QUERIES, EPS, seed=SEED, use_graph=False, norm="L2")
    for _ in range(2):  # the capture, then a second run on the cached graph
        graph = engine.square_loop(m, x, y, N_QUERIES, EPS, seed=SEED, use_graph=True, norm="L2")
        assert all(torch.equal(a, b) for a, b in zip(eager, graph))
    _valid(eager[0], x)
    assert torch.equal(eager[0][eager[1]], x[eager[1]])
    other = engine.square_loop(m, x, y, N_QUERIES, EPS, seed=SEED + 1, use_graph=True, norm="L2")
    assert not torch.equal(other[0], eager[0]) or bool(eager[1].all())
    monkeypatch.setattr(engine, "SQUARE_CHECK_EVERY", 16)
    y_wrong = (y + 1) % 10
    for yy in (y, y_wrong):
        for use_graph in (False, True):
            on = engine.square_loop(m, x, yy, N_QUERIES, EPS, seed=SEED, use_graph=use_graph, early_exit=True, norm="L2")
            off = engine.square_loop(m, x, yy, N_QUERIES, EPS, seed=SEED, use_graph=use_graph, early_exit=False, norm="L2")
            assert all(torch.equal(a, b) for a, b in zip(on, off))
    with pytest.raises(ValueError, match="norm"):
        engine.square_loop(m, x, y, N_QUERIES, EPS, seed=SEED, norm="L1")
    engine.clear_graphs()


def test_linf_is_what_it_was():
    """The default norm and norm="Linf" are one call: the same bits, and a Linf run owns none of the L2 state."""
    from eeadv import engine
    import utils.attacks as A
    from tiny_models import Args
    m, x, y = _problem(SHAPES[2])
    a = engine.square_loop(m, x, y, N_QUERIES, 16 / 255, seed=SEED, use_graph=False)
    b = engine.square_loop(m, x, y, N_QUERIES, 16 / 255, seed=SEED, use_graph=False, norm="Linf")
    c = A.Square(m, Args(epsilon=16 / 255), x, y, n_queries=N_QUERIES, seed=SEED)
    assert all(torch.equal(p, q) for p, q in zip(a, b)) and all(torch.equal(p, q) for p, q in zip(a, c))
    run = engine._SquareRun(x, y, N_QUERIES, 16 / 255)
    assert run.norms is None and not hasattr(run, "eta") and not hasattr(run, "eta_off")
    l2 = A.Square(m, Args(epsilon=EPS), x, y, n_queries=N_QUERIES, seed=SEED, norm="L2")
    want = engine.square_loop(m, x, y, N_QUERIES, EPS, seed=SEED, use_graph=False, norm="L2")
    assert all(torch.equal(p, q) for p, q in zip(l2, want))
