"""CPU: the staging logic of eeadv.cascade with scripted stages in place of the attacks (held against a list-based restatement of the
cascade), the optional `order` of APGD_T / FAB_T, the dispatch, and one driver run with --attack_method Cascade on the host."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from tiny_models import Args, TinyNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")
S = 4  # stages
NCLS = 4


@pytest.fixture()
def cpu_plumbing():
    from eeadv import runtime
    runtime.allow_cpu_plumbing(True)
    yield
    runtime.allow_cpu_plumbing(False)


# ---- scripted samples ------------------------------------------------------------------------------------------------------------------
# A sample is a 1x2x2 image whose pixels carry its script: pixel 0 = the stage that breaks it (S + 1: none does), pixel 1 = its global id,
# pixel 2 = the class the "model" predicts for it.  The label is that class, or the next one for a sample that is misclassified clean.
class ScriptModel(torch.nn.Module):
    def forward(self, x):
        cls = x.flatten(1)[:, 2:3]
        return -(torch.arange(NCLS, dtype=x.dtype).view(1, -1) - cls).abs()


def make_samples(breaks, wrong):
    n = len(breaks)
    x = torch.zeros(n, 1, 2, 2)
    x[:, 0, 0, 0] = torch.tensor(breaks, dtype=torch.float32)
    x[:, 0, 0, 1] = torch.arange(n, dtype=torch.float32)
    x[:, 0, 1, 0] = torch.arange(n, dtype=torch.float32) % NCLS
    y = (torch.arange(n) % NCLS + torch.tensor(wrong, dtype=torch.int64)) % NCLS
    return x, y


def scripted_stages(log):
    """Stage k breaks the rows whose pixel 0 says k; its "adversarial point" is the row plus k plus a mark of the row's POSITION in the
    batch, so a padding row (a copy of row 0 at another position) that reached the result would be seen.  log[k - 1] gets the ids of
    every batch the stage ran on."""
    def stage(k):
        def fn(model, args, x, y, order):
            flat = x.flatten(1)
            log[k - 1].append([int(v) for v in flat[:, 1].tolist()])
            assert torch.equal(order[:, 0], flat[:, 2].to(torch.int64)) and torch.equal(order[:, 0], y)  # only clean-correct rows, fields intact
            pos = torch.arange(x.shape[0], dtype=x.dtype).view(-1, 1, 1, 1)
            return x + k + pos / 64, flat[:, 0] != k
        return "stage%d" % k, fn
    return [stage(k) for k in range(1, S + 1)]


def simulate(breaks, wrong, sizes, B):
    """The cascade on Python lists: (stage per sample, batches per stage (ids, padded), position of each broken sample in its batch)."""
    pools, runs = [[] for _ in range(S)], [[] for _ in range(S)]
    stage = [S + 1] * len(breaks)
    pos = {}

    def run(s):
        ids = pools[s][:B]
        del pools[s][:B]
        runs[s].append(ids + [ids[0]] * (B - len(ids)))
        for p, i in enumerate(ids):
            if breaks[i] == s + 1:
                stage[i], pos[i] = s + 1, p
            elif s + 1 < S:
                pools[s + 1].append(i)
        if s + 1 < S:
            drain(s + 1)

    def drain(s, flush=False):
        while len(pools[s]) >= B or (flush and pools[s]):
            run(s)

    n0 = 0
    for b in sizes:
        for i in range(n0, n0 + b):
            if wrong[i]:
                stage[i] = 0
            else:
                pools[0].append(i)
        n0 += b
        drain(0)
    for s in range(S):
        drain(s, flush=True)
    return stage, runs, pos


def split(x, y, sizes):
    out, n0 = [], 0
    for b in sizes:
        out.append((x[n0:n0 + b], y[n0:n0 + b]))
        n0 += b
    return out


CASES = {
    # B = 4 everywhere.  "exactly_B": the first pool fills to exactly B with the first batch, and again with the third
    "exactly_B": dict(breaks=[5, 1, 2, 5, 3, 4, 5, 1, 5, 5, 2, 3], wrong=[0] * 12, sizes=[4, 4, 4]),
    # "2B-1": the first pool holds B - 1 = 3 rows after batch one (one clean error), batch two brings it to 2B - 1 = 7
    "2B-1": dict(breaks=[5, 5, 5, 5, 5, 2, 5, 3, 1, 4, 5, 5, 5], wrong=[0, 1, 0, 0] + [0] * 9, sizes=[4, 4, 4, 1]),
    # "empty_stage": nothing survives stage 2, stages 3 and 4 never run
    "empty_stage": dict(breaks=[1, 2, 2, 1, 1, 2, 2, 2, 1, 1], wrong=[0, 0, 1, 0, 0, 0, 0, 1, 0, 0], sizes=[4, 4, 2]),
    # "N<B": three samples, batches of four
    "N<B": dict(breaks=[5, 2, 4], wrong=[0, 0, 0], sizes=[3]),
    "all_wrong": dict(breaks=[5, 5, 5, 5, 5], wrong=[1] * 5, sizes=[4, 1]),
}


def _random_case(seed):
    g = torch.Generator().manual_seed(seed)
    n = int(torch.randint(9, 40, (1,), generator=g))
    breaks = torch.randint(1, S + 2, (n,), generator=g).tolist()
    wrong = (torch.rand(n, generator=g) < 0.2).to(torch.int64).tolist()
    sizes = [4] * (n // 4) + ([n % 4] if n % 4 else [])
    return dict(breaks=breaks, wrong=wrong, sizes=sizes)


CASES.update({"random%d" % s: _random_case(s) for s in range(4)})


@pytest.mark.parametrize("name", sorted(CASES))
def test_staging_against_the_list_cascade(cpu_plumbing, name):
    from eeadv import cascade
    case, B = CASES[name], 4
    breaks, wrong, sizes = case["breaks"], case["wrong"], case["sizes"]
    N = len(breaks)
    x, y = make_samples(breaks, wrong)
    log = [[] for _ in range(S)]
    res = cascade.evaluate(ScriptModel(), Args(epsilon=0.1), split(x, y, sizes), NCLS, keep_adv=True, stages=scripted_stages(log), batch_size=B)
    stage, runs, pos = simulate(breaks, wrong, sizes, B)
    assert log == runs  # the same batches in the same order, padding included
    assert res.n == N and res.stage.tolist() == stage and res.stage.dtype == torch.int32
    assert res.robust.tolist() == [s == S + 1 for s in stage] and res.robust.dtype == torch.bool
    # a sample visits the stages in order and none after the one that breaks it; a clean error visits none
    for i in range(N):
        visited = [s + 1 for s in range(S) if any(i in ids[:B] for ids in runs[s])]
        want = [] if wrong[i] else list(range(1, min(breaks[i], S) + 1))
        assert visited == want, (i, visited, want)
    # the counts add up
    assert res.clean_correct == N - sum(wrong)
    assert res.rows_attacked == [sum(1 for i in range(N) if not wrong[i] and breaks[i] > s) for s in range(S)]
    assert res.robust_after == [sum(1 for i in range(N) if not wrong[i] and breaks[i] > s + 1) for s in range(S)]
    assert res.robust_after[-1] == int(res.robust.sum()) and res.clean_correct - sum(1 for s in stage if 1 <= s <= S) == res.robust_after[-1]
    assert res.batches_attacked == [len(r) for r in runs] and all(-(-a // B) <= b for a, b in zip(res.rows_attacked, res.batches_attacked))
    # adversarial points: the broken sample's own row at its own position - a padding copy would carry another position
    for i in range(N):
        want = x[i] + stage[i] + pos[i] / 64 if 1 <= stage[i] <= S else x[i]
        assert torch.equal(res.adv[i], want), i
    if name == "empty_stage":
        assert res.rows_attacked[2:] == [0, 0] and res.batches_attacked[2:] == [0, 0]
    if name == "exactly_B":
        assert runs[0][0] == [0, 1, 2, 3]
    if name == "2B-1":
        assert runs[0][0] == [0, 2, 3, 4] and runs[0][1][:3] == [5, 6, 7]


def test_evaluate_refuses_what_it_cannot_run(cpu_plumbing, monkeypatch):
    from eeadv import cascade
    x, y = make_samples([5] * 6, [0] * 6)
    a = Args(epsilon=0.1)
    with pytest.raises(ValueError, match="one batch shape"):
        cascade.evaluate(ScriptModel(), a, [(x[:2], y[:2]), (x[2:6], y[2:6])], NCLS, stages=scripted_stages([[] for _ in range(S)]))
    with pytest.raises(RuntimeError, match="compaction='torch'"):
        cascade.evaluate(ScriptModel(), a, [(x, y)], NCLS, stages=scripted_stages([[] for _ in range(S)]), compaction="hip")
    with pytest.raises(ValueError, match="compaction"):
        cascade.evaluate(ScriptModel(), a, [(x, y)], NCLS, stages=scripted_stages([[] for _ in range(S)]), compaction="numpy")
    monkeypatch.setattr(cascade, "_free_bytes", lambda device: 64)  # a device with 64 bytes left
    with pytest.raises(MemoryError, match="keep_adv needs .* without keep_adv"):
        cascade.evaluate(ScriptModel(), a, [(x, y)], NCLS, keep_adv=True, stages=scripted_stages([[] for _ in range(S)]))
    res = cascade.evaluate(ScriptModel(), a, [(x, y)], NCLS, stages=scripted_stages([[] for _ in range(S)]))
    assert res.adv is None and res.robust_after == [6] * S


def test_without_cpu_plumbing_the_cascade_refuses_host_tensors():
    from eeadv import cascade
    x, y = make_samples([5] * 4, [0] * 4)
    with pytest.raises(RuntimeError, match="allow_cpu_plumbing"):
        cascade.evaluate(ScriptModel(), Args(epsilon=0.1), [(x, y)], NCLS, stages=scripted_stages([[] for _ in range(S)]))


# ---- the real attacks underneath (host loops) --------------------------------------------------------------------------------------------
def _tiny():
    torch.manual_seed(0)
    m = TinyNet(3, 8, 10, 5).eval()
    x = torch.rand(6, 3, 8, 8)
    with torch.no_grad():
        z = m(x)
    return m, x, z.argmax(1), z


def test_apgd_t_and_fab_t_take_a_precomputed_order(cpu_plumbing):
    import utils.attacks as A
    m, x, y, z = _tiny()
    a = Args(epsilon=16 / 255)
    n_t = 3
    order = torch.sort(z, dim=1, descending=True, stable=True)[1][:, :n_t + 1].contiguous()
    noise = torch.zeros_like(x).uniform_(-a.epsilon, a.epsilon)
    calls = []
    h = m.register_forward_hook(lambda *_: calls.append(1))
    xa, ra = A.APGD_T(m, a, x, y, 4, 10, n_t, noise=noise)
    n_default = len(calls)
    xb, rb = A.APGD_T(m, a, x, y, 4, 10, n_t, noise=noise, order=order)
    assert torch.equal(xa, xb) and torch.equal(ra, rb) and len(calls) - n_default == n_default - 1  # one forward less: the clean one
    calls.clear()
    xf, rf, nf = A.FAB_T(m, a, x, y, 10, 3, n_t)
    n_default = len(calls)
    xg, rg, ng = A.FAB_T(m, a, x, y, 10, 3, n_t, order=order)
    h.remove()
    assert torch.equal(xf, xg) and torch.equal(rf, rg) and torch.equal(nf, ng) and len(calls) - n_default == n_default - 1
    with pytest.raises(ValueError, match="order must be int64"):
        A.APGD_T(m, a, x, y, 4, 10, n_t, order=order[:, :2])
    with pytest.raises(ValueError, match="order must be int64"):
        A.FAB_T(m, a, x, y, 10, 3, n_t, order=order.to(torch.int32))


def test_cascade_with_the_host_attacks(cpu_plumbing):
    """The real stages on the CPU: every broken sample's point lies in the eps-ball and is misclassified, survivors are still classified
    correctly, and a sample broken at stage k was attacked by the stages before it (rows_attacked is monotone)."""
    from eeadv import cascade
    m, x, y, _ = _tiny()
    torch.manual_seed(3)
    xs = torch.rand(14, 3, 8, 8)
    with torch.no_grad():
        ys = m(xs).argmax(1)
    ys[5] = (ys[5] + 1) % 10
    eps = 6 / 255
    a = Args(epsilon=eps, fab_iters=3, square_queries=8, n_target_classes=3, num_steps_1=4)
    res = cascade.evaluate(m, a, split(xs, ys, [4, 4, 4, 2]), 10, keep_adv=True)
    assert res.stage_names == list(cascade.STAGES) and res.n == 14 and res.clean_correct == 13 and int(res.stage[5]) == 0
    assert all(p >= q for p, q in zip([res.clean_correct] + res.rows_attacked, res.rows_attacked))
    assert res.rows_attacked == [res.clean_correct] + res.robust_after[:-1]
    e = torch.tensor(eps, dtype=torch.float32)
    broken = (res.stage >= 1) & (res.stage <= 4)
    assert torch.equal(~res.robust, broken | (res.stage == 0))
    with torch.no_grad():
        pred = m(res.adv).argmax(1)
    assert bool((pred[broken] != ys[broken]).all()) and bool((pred[res.robust] == ys[res.robust]).all())
    assert bool((res.adv >= xs - e).all()) and bool((res.adv <= xs + e).all()) and torch.equal(res.adv[~broken], xs[~broken])


# ---- ABI and dispatch ------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_pool_kernels():
    import eeadv._native as n
    L = n.lib
    for name in ("ee_pool_append_f32", "ee_pool_pop_f32", "ee_cascade_resolve_f32"):
        assert name in n.SIGNATURES and hasattr(L, name)
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    assert L.ee_pool_append_f32(p, p, p, p, p, 4, 8, 2, p, p, p, p, None, 8, None) == -1
    assert L.ee_pool_append_f32(p, p, p, p, p, 0, 8, 2, p, p, p, p, p, 8, None) == -2 and L.ee_pool_append_f32(p, p, p, p, p, 4, 0, 2, p, p, p, p, p, 8, None) == -2
    assert L.ee_pool_append_f32(p, p, p, p, p, 4097, 8, 2, p, p, p, p, p, 8, None) == -3
    assert L.ee_pool_append_f32(p, odd, p, p, p, 4, 8, 2, p, p, p, p, p, 8, None) == -4
    assert L.ee_pool_pop_f32(p, p, p, p, p, 8, 4, 8, 2, p, p, p, None, None) == -1
    assert L.ee_pool_pop_f32(p, p, p, p, p, 7, 4, 8, 2, p, p, p, p, None) == -2  # cap < 2 B
    assert L.ee_pool_pop_f32(p, p, p, odd, p, 8, 4, 8, 2, p, p, p, p, None) == -4
    assert L.ee_cascade_resolve_f32(p, p, p, 4, 4, 8, 1, 10, None, p, None, p, None) == -1
    assert L.ee_cascade_resolve_f32(p, p, None, 4, 4, 8, 1, 10, p, p, p, p, None) == -1  # adv_out without x_adv
    assert L.ee_cascade_resolve_f32(p, p, p, 4, 5, 8, 1, 10, p, p, None, p, None) == -2 and L.ee_cascade_resolve_f32(p, p, p, 4, 4, 8, 1, 0, p, p, None, p, None) == -2
    assert L.ee_cascade_resolve_f32(p, odd, p, 4, 4, 8, 1, 10, p, p, None, p, None) == -4
    from eeadv import ops
    z = torch.zeros(2, 8)
    i = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(n.EEError):
        ops.pool_append_(z, i, i, torch.zeros(2, 2, dtype=torch.int64), torch.ones(2, dtype=torch.bool), torch.zeros(4, 8), torch.zeros(4, dtype=torch.int64),
                         torch.zeros(4, dtype=torch.int64), torch.zeros(4, 2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32))


def test_dispatch_keeps_aa_stopped_and_cascade_out_of_the_batch_loop(cpu_plumbing):
    from eeadv import driver, trainer
    m, x, y, _ = _tiny()
    a = Args(epsilon=8 / 255, method_name="AT", attack_method="AA", random=True)
    with pytest.raises(NotImplementedError):
        trainer.attack_for_validation(m, a, x, y, torch.device("cpu"), 3, 2 / 255, 10)
    a.attack_method = "Cascade"
    assert trainer.CASCADE_METHOD == "Cascade" and "Cascade" not in trainer.FAB_METHODS + trainer.SQUARE_METHODS + trainer.APGD_METHODS
    with pytest.raises(NotImplementedError, match="whole split"):
        trainer.attack_for_validation(m, a, x, y, torch.device("cpu"), 3, 2 / 255, 10)
    a.method_name = "tar_AT"
    with pytest.raises(NotImplementedError, match="untargeted"):
        driver.validate_cascade([(x, y)], m, a, torch.device("cpu"), 3, 10, print)


def test_awp_driver_still_stops_at_aa(tmp_path):
    sys.path.insert(0, os.path.join(PKG, "AWP", "Tiny_imagenet"))
    try:
        import experiments_tiny_awp as drv
        with pytest.raises(SystemExit, match="autoattack"):
            drv.main(["-c", os.path.join(PKG, "AWP", "Tiny_imagenet", "configs_tiny_awp", "at_awp.yml"), "--attack_method", "AA",
                      "--output-root", str(tmp_path)])
    finally:
        sys.path.remove(os.path.join(PKG, "AWP", "Tiny_imagenet"))


def test_mnist_driver_evaluates_with_the_cascade_on_the_host(tmp_path):
    r = subprocess.run([sys.executable, "experiments_mnist.py", "-c", "configs_mnist/adversarial_training.yml", "--no-cuda", "--data", "synthetic",
                        "--output-root", str(tmp_path), "-e", "--attack_method", "Cascade", "--fab_iters", "2", "--square_queries", "6"],
                       cwd=os.path.join(PKG, "MNIST"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    logs = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path)) for f in fs if f == "log.txt"]
    assert logs
    for text in (r.stdout, "".join(open(f).read() for f in logs)):
        clean = re.findall(r"^ \* Cascade clean accuracy ([\d.]+)", text, flags=re.M)
        assert len(clean) >= 1
        per_stage = [re.findall(r"^ \* Cascade robust accuracy after %s ([\d.]+)" % re.escape(s), text, flags=re.M) for s in
                     ("APGD-CE", "APGD-T", "FAB-T", "Square")]
        assert all(len(v) == len(clean) for v in per_stage)
        for k, c in enumerate(clean):  # the five lines of one evaluation: each stage can only lower the figure
            vals = [float(c)] + [float(v[k]) for v in per_stage]
            assert all(p >= q for p, q in zip(vals, vals[1:])), vals
