"""MI355X: the pool kernels of the attack cascade (csrc/ee_cascade.hip) bit for bit against numpy, and eeadv.cascade.evaluate end to end on
Net_2 - HIP pools against the torch statement of the same staging, eager against graph replay, and the validity of what it returns."""
import numpy as np
import pytest
import torch

from tiny_models import Args

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 4  # width of the class-order field in the kernel tests
GUARD = 2  # rows behind the pool that no launch may touch


@pytest.fixture(scope="module")
def ops():
    from eeadv import ops as o
    return o


# ---- numpy statement of the three operations (rows as int32 bits) ----------------------------------------------------------------------
class NpPool:
    """cap rows and GUARD more behind them, which stay as they are."""

    def __init__(self, x, y, ids, order, count):
        self.f = [x.copy(), y.copy(), ids.copy(), order.copy()]
        self.count = count

    def append(self, src, keep):
        cap = self.f[0].shape[0] - GUARD
        d = self.count
        for b in np.nonzero(keep)[0]:
            if d < cap:
                for dst, s in zip(self.f, src):
                    dst[d] = s[b]
            d += 1
        self.count = min(d, cap)

    def pop(self, B):
        c = self.count
        idx = np.where(np.arange(B) < c, np.arange(B), 0)
        out = [a[idx].copy() for a in self.f]
        if c > B:
            for a in self.f:
                a[:c - B] = a[B:c].copy()
        self.count = max(c - B, 0)
        return out


def _bits(rng, shape):
    """Random 32-bit patterns: every kind of float, NaNs with payloads among them; a few fixed ones so that they are always there."""
    a = rng.integers(-2 ** 31, 2 ** 31, size=shape, dtype=np.int64).astype(np.int32)
    flat = a.reshape(-1)
    special = np.array([0x7fc00001, -1, 0x7f800001, -0x00400000, 0, -2 ** 31], dtype=np.int64).astype(np.int32)  # quiet, all ones, signalling, negative NaN; 0; -0
    flat[:min(flat.size, special.size)] = special[:min(flat.size, special.size)]
    return a


def _rows(rng, n, D):
    """n rows of (x bits, label, id beyond 2^31, order)."""
    return [_bits(rng, (n, D)), rng.integers(0, 1000, n), (1 << 40) + rng.integers(0, 2 ** 33, n), rng.integers(0, 1000, (n, K))]


class DevPool:
    """The pool tensors on the device, GUARD rows longer than `cap`; the kernels get the first cap rows."""

    def __init__(self, np_pool):
        x, y, ids, order = np_pool.f
        self.cap = x.shape[0] - GUARD
        self.full = [torch.from_numpy(x).view(torch.float32).to(DEV), torch.from_numpy(y).to(DEV), torch.from_numpy(ids).to(DEV),
                     torch.from_numpy(order).to(DEV)]
        self.count = torch.tensor([np_pool.count], dtype=torch.int32, device=DEV)

    def fields(self):
        return [t[:self.cap] for t in self.full]

    def same_as(self, np_pool):
        got = [self.full[0].view(torch.int32).cpu().numpy()] + [t.cpu().numpy() for t in self.full[1:]]
        return all(np.array_equal(g, w) for g, w in zip(got, np_pool.f)) and int(self.count.item()) == np_pool.count


def _to_dev(src, misalign=False):
    x, y, ids, order = src
    if misalign:  # the batch starts 4 bytes behind a 16-byte boundary: none of its rows takes the 16-byte path unless D % 4 == 3 ...
        buf = torch.zeros(x.size + 1, dtype=torch.float32, device=DEV)
        xd = buf[1:].view(x.shape)
        xd.copy_(torch.from_numpy(x).view(torch.float32))
    else:
        xd = torch.from_numpy(x).view(torch.float32).to(DEV)
    return [xd, torch.from_numpy(y).to(DEV), torch.from_numpy(ids).to(DEV), torch.from_numpy(order).to(DEV)]


def _start(rng, B, D, count):
    """A pool of cap = 2 B rows (+ GUARD) holding `count` rows; what lies behind them is random too and must survive."""
    x, y, ids, order = _rows(rng, 2 * B + GUARD, D)
    return NpPool(x, y, ids, order, count)


@pytest.mark.parametrize("B", [1, 8, 100, 257])
@pytest.mark.parametrize("D", [1, 75, 784, 12288])
def test_pool_kernels_bit_for_bit(ops, D, B):
    rng = np.random.default_rng(1000 * D + B)
    odd = (B // 2) | 1  # an odd, non-zero starting count: 1, 5, 51, 129 - with D % 4 != 0 the first free row is misaligned
    patterns = {"zeros": np.zeros(B, bool), "ones": np.ones(B, bool), "alternating": np.arange(B) % 2 == 0, "random": rng.random(B) < 0.5}
    # append (copy launch + count launch): every pattern from the odd count; all ones from count = B fills the pool to exactly cap; from
    # count = B + 3 the last three kept rows have no place and are dropped, nothing is written behind the pool
    cases = [(name, odd) for name in patterns] + [("ones", B), ("random", B)] + ([("ones", B + 3)] if B > 3 else [])
    for i, (name, count) in enumerate(cases):
        want = _start(rng, B, D, count)
        dev = DevPool(want)
        src = _rows(rng, B, D)
        keep = patterns[name]
        want.append(src, keep)
        d = _to_dev(src, misalign=(i % 2 == 1))
        keep_dev = torch.from_numpy(keep).to(DEV)
        ops.pool_append_(*d, keep_dev if i % 2 else keep_dev.to(torch.uint8), *dev.fields(), dev.count)
        assert dev.same_as(want), (name, count)
        if (name, count) == ("ones", B):
            assert want.count == 2 * B
    # pop (copy-out launch, move-to-front launch, count launch): fewer than B rows (padding with row 0), exactly B, B <= count < 2 B
    for count in sorted({0, odd if odd < B else 0, B, B + B // 2, 2 * B - 1, 2 * B}):
        want = _start(rng, B, D, count)
        dev = DevPool(want)
        out = want.pop(B)
        batch = _to_dev(_rows(rng, B, D))
        ops.pool_pop_(*dev.fields(), dev.count, *batch)
        got = [batch[0].view(torch.int32).cpu().numpy()] + [t.cpu().numpy() for t in batch[1:]]
        assert all(np.array_equal(g, w) for g, w in zip(got, out)), count
        assert dev.same_as(want), count
        assert want.count == max(count - B, 0)
    # resolve: padding rows, an id outside [0, N), with and without adv_out
    N = 3 * B + 5
    for with_adv in (True, False):
        n_valid = B - B // 3
        robust = rng.random(B) < 0.5
        ids = rng.permutation(N)[:B].astype(np.int64)
        if B > 2:
            ids[1], robust[1] = (1 << 33) + 7, False  # broken, but no sample of this split: nothing may be written for it
            ids[2], robust[2] = -1, True
        x_adv = _bits(rng, (B, D))
        robust_out = rng.random(N) < 0.7
        stage_out = rng.integers(0, 6, N).astype(np.int32)
        adv_out = _bits(rng, (N + GUARD, D))
        keep0 = rng.random(B) < 0.5
        r_dev, s_dev = torch.from_numpy(robust_out).to(DEV), torch.from_numpy(stage_out).to(DEV)
        a_dev = torch.from_numpy(adv_out).view(torch.float32).to(DEV)
        k_dev = torch.from_numpy(keep0).to(DEV)
        ops.cascade_resolve_(torch.from_numpy(robust).to(DEV), torch.from_numpy(ids).to(DEV), torch.from_numpy(x_adv).view(torch.float32).to(DEV),
                             n_valid, 3, r_dev, s_dev, a_dev[:N] if with_adv else None, k_dev)
        keep = np.zeros(B, bool)
        for b in range(n_valid):
            if 0 <= ids[b] < N:
                keep[b] = robust[b]
                if not robust[b]:
                    robust_out[ids[b]], stage_out[ids[b]] = False, 3
                    if with_adv:
                        adv_out[ids[b]] = x_adv[b]
        assert np.array_equal(k_dev.cpu().numpy(), keep) and np.array_equal(r_dev.cpu().numpy(), robust_out)
        assert np.array_equal(s_dev.cpu().numpy(), stage_out) and np.array_equal(a_dev.view(torch.int32).cpu().numpy(), adv_out)


def test_pool_ops_check_their_shapes(ops):
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64, device=DEV)  # noqa: E731
    pool = (z(8, 6), i64(8), i64(8), i64(8, K), torch.zeros(1, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.pool_append_(z(4, 5), i64(4), i64(4), i64(4, K), torch.ones(4, dtype=torch.bool, device=DEV), *pool)
    with pytest.raises(ValueError):
        ops.pool_append_(z(4, 6), i64(4), i64(4), i64(4, K + 1), torch.ones(4, dtype=torch.bool, device=DEV), *pool)
    with pytest.raises(Exception, match="ee_pool_pop_f32"):
        ops.pool_pop_(*pool, z(5, 6), i64(5), i64(5), i64(5, K))  # cap 8 < 2 * 5


# ---- end to end on Net_2 ---------------------------------------------------------------------------------------------------------------
EPS, SEED, B, N = 0.004, 0, 8, 40  # picked on the CPU host path: there the four stages run on 37 / 22 / 17 / 17 rows
WRONG = (3, 17, 30)


@pytest.fixture(scope="module")
def e2e():
    """The three runs the tests below compare, once: HIP pools eager, torch staging eager, HIP pools under graph replay."""
    import os
    from eeadv import cascade, engine, models, runtime
    # a first graph capture creates the device draw state from a ticket of torch's generator (eeadv.runtime.draw_state): create it before the
    # runs, or the graph run's random starts would come from a generator one ticket further on than the eager run's
    runtime.draw_state(torch.device(DEV))
    torch.manual_seed(SEED)
    m = models.Net_2().eval()
    x = torch.rand(N, 1, 28, 28)
    m, x = m.to(DEV), x.to(DEV)
    with torch.no_grad():
        y = torch.cat([m(x[i:i + B]).argmax(1) for i in range(0, N, B)])
    for i in WRONG:
        y[i] = (y[i] + 1) % 10
    a = Args(epsilon=EPS, fab_iters=3, square_queries=32, n_target_classes=3)
    batches = [(x[i:i + B], y[i:i + B]) for i in range(0, N, B)]
    old = os.environ.get("EEADV_GRAPH")
    runs = {}
    try:
        for name, graph, compaction in (("hip", "0", "hip"), ("torch", "0", "torch"), ("graph", "1", "hip")):
            os.environ["EEADV_GRAPH"] = graph
            torch.manual_seed(100 + SEED)
            runs[name] = cascade.evaluate(m, a, batches, 10, keep_adv=True, compaction=compaction, num_steps=5)
    finally:
        if old is None:
            os.environ.pop("EEADV_GRAPH", None)
        else:
            os.environ["EEADV_GRAPH"] = old
        engine.clear_graphs()
    return m, x, y, runs


def _same(p, q):
    print("differing: robust %d, stage %d, adv rows %d; rows %s / %s" % (int((p.robust != q.robust).sum()), int((p.stage != q.stage).sum()),
          int((p.adv.view(torch.int32) != q.adv.view(torch.int32)).flatten(1).any(1).sum()), p.rows_attacked, q.rows_attacked))
    return (torch.equal(p.robust, q.robust) and torch.equal(p.stage, q.stage) and torch.equal(p.adv.view(torch.int32), q.adv.view(torch.int32))
            and p.rows_attacked == q.rows_attacked and p.robust_after == q.robust_after and p.batches_attacked == q.batches_attacked)


def test_every_stage_runs_and_the_flush_is_partial(e2e):
    res = e2e[3]["hip"]
    print("clean_correct %d rows_attacked %s robust_after %s batches %s" % (res.clean_correct, res.rows_attacked, res.robust_after, res.batches_attacked))
    assert res.n == N and res.clean_correct == N - len(WRONG) and all(int(res.stage[i]) == 0 for i in WRONG)
    assert all(r >= 1 for r in res.rows_attacked)  # every stage's pool received a row
    assert any(r % B for r in res.rows_attacked)  # some flush popped a padded batch
    assert all(b == -(-r // B) for r, b in zip(res.rows_attacked, res.batches_attacked))
    assert res.rows_attacked == [res.clean_correct] + res.robust_after[:-1] and res.robust_after[-1] == int(res.robust.sum())


def test_hip_pools_equal_the_torch_staging(e2e):
    assert _same(e2e[3]["hip"], e2e[3]["torch"])


def test_eager_equals_graph_replay(e2e):
    assert _same(e2e[3]["hip"], e2e[3]["graph"])


def test_broken_samples_lie_in_the_ball_and_are_misclassified(e2e):
    """adv is built from x0 by f32 operations that end in min(max(., x0 - eps), x0 + eps) (APGD, Square) or is kept under fl(adv - x0) <= eps
    (FAB-T): either way adv lies between the f32 neighbours below fl(x0 - eps) and above fl(x0 + eps) - one rounding of x0 -+ eps."""
    m, x, y, runs = e2e
    res = runs["hip"]
    broken = ~res.robust & (res.stage >= 1)
    assert int(broken.sum()) >= 1 and torch.equal(broken, (res.stage >= 1) & (res.stage <= 4))
    e = torch.tensor(EPS, dtype=torch.float32, device=DEV)
    inf = torch.tensor(float("inf"), device=DEV)
    lo, hi = torch.nextafter(x - e, -inf), torch.nextafter(x + e, inf)
    adv = res.adv
    assert bool((adv[broken] >= lo[broken]).all()) and bool((adv[broken] <= hi[broken]).all())
    assert bool((adv >= 0).all()) and bool((adv <= 1).all()) and torch.equal(adv[~broken], x[~broken])
    with torch.no_grad():  # in batches of the shape the attacks ran
        pred = torch.cat([m(adv[i:i + B]).argmax(1) for i in range(0, N, B)])
    assert bool((pred[broken] != y[broken]).all())
    assert bool((pred[res.robust] == y[res.robust]).all())
