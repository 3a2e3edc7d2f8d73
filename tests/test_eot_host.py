"""CPU: EOT for APGD - the plain-torch host path of utils.attacks against tests/eot_reference.py bit for bit in float64, the iterations per
captured graph, the argument errors of the new doors, and Cascade-Rand on the host (the MNIST driver, and cascade.evaluate with scripted
verdicts underneath rand_stages)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

import apgd_reference as R
import eot_reference as ER
from tiny_models import Args, TinyNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")

SEED, B, HW, NCLS, EPS, N_ITER = 2, 4, 8, 10, 0.03, 10
DRAW_S, DRAW_O = (1.0, 0.9, 1.1, 0.95, 1.05, 0.85, 1.15), (0.0, 0.02, -0.02, 0.01, -0.01, 0.03, -0.03)


@pytest.fixture()
def cpu_plumbing():
    from eeadv import runtime
    runtime.allow_cpu_plumbing(True)
    yield
    runtime.allow_cpu_plumbing(False)


def _problem(dtype=torch.float64, seed=SEED):
    torch.manual_seed(seed)
    model = ER.ScriptedDraws(TinyNet(3, HW, NCLS, seed=seed).to(dtype).eval(), DRAW_S, DRAW_O).eval()
    x0 = torch.rand(B, 3, HW, HW, dtype=dtype)
    with torch.no_grad():
        y = model.net(x0).argmax(1)
    y[0] = (y[0] + 1) % NCLS  # one sample starts misclassified
    noise = torch.zeros_like(x0).uniform_(-EPS, EPS)
    return model, x0, y, noise


KEYS = ("x", "x_old", "g", "loss", "pred", "step", "loss_best", "f_prev", "loss_best_last", "inc", "reduced_last", "robust", "x_best", "g_best",
        "x_best_adv")


def _equal_traces(got, want, E):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        for key in KEYS + (("draw_loss", "draw_g", "draw_pred") if E > 1 else ()):
            assert torch.equal(a[key], b[key].to(a[key].dtype)), (i, key)
        if i:
            for key in ("improved", "fooled", "reduced"):
                assert a[key].tolist() == b[key], (i, key)


@pytest.mark.parametrize("E", [1, 2, 3])
@pytest.mark.parametrize("kind", ["ce", "dlr"])
def test_host_path_equals_the_reference_bit_for_bit(cpu_plumbing, kind, E):
    """B = 4, 3x8x8, 10 classes, 10 iterations (a checkpoint after every iteration from the second on), float64, the draws scripted: every
    recorded quantity of _apgd_host(eot_iter=E) - the E draws' losses, gradients and preds included - equals the per-sample restatement.
    The seed was chosen so that some checkpoint halves a step and some checkpoint leaves one alone, for every case."""
    import utils.attacks as A
    model, x0, y, noise = _problem()
    x_init = torch.clamp(x0 + noise, 0, 1)
    model.calls = 0
    want_x, want_r, want_l, want_trace = ER.run(model, x0, x_init, y, N_ITER, EPS, kind, E)
    assert model.calls == (N_ITER + 1) * E
    model.calls = 0
    trace = []
    got_x, got_r, got_l = A._apgd_host(model, x0, x_init, y, N_ITER, EPS, kind, trace=trace, eot_iter=E)
    assert model.calls == (N_ITER + 1) * E
    _equal_traces(trace, want_trace, E)
    assert torch.equal(got_x, want_x) and torch.equal(got_r, want_r) and torch.equal(got_l, want_l)
    model.calls = 0
    xa, rb = A.APGD(model, Args(epsilon=EPS), x0, y, N_ITER, loss=kind, noise=noise, eot_iter=E)
    assert torch.equal(xa, want_x) and torch.equal(rb, want_r) and xa.dtype == torch.float64
    cps = [e for e in want_trace[1:] if e["k"]]
    assert len(cps) == 9
    assert any(r for e in cps for r in e["reduced"]), "no checkpoint halved a step"
    assert any(not r for e in cps for r in e["reduced"]), "no checkpoint left a step alone"
    if E > 1:  # the draws differ, so the mean is not any single draw
        assert any(not torch.equal(e["draw_g"][0], e["draw_g"][1]) for e in want_trace)
        assert not torch.equal(want_trace[1]["g_new"], want_trace[1]["draw_g"][-1])


@pytest.mark.parametrize("kind", ["ce", "dlr"])
def test_eot_iter_1_is_the_plain_host_run(cpu_plumbing, kind):
    """eot_iter = 1 (explicit or left out) is the run tests/apgd_reference.py describes - today's _apgd_host - bit for bit."""
    import utils.attacks as A
    model, x0, y, noise = _problem()
    x_init = torch.clamp(x0 + noise, 0, 1)
    model.calls = 0
    want_x, want_r, want_l, want_trace = R.run(model, x0, x_init, y, N_ITER, EPS, kind)
    for kw in ({}, {"eot_iter": 1}):
        model.calls = 0
        trace = []
        got = A._apgd_host(model, x0, x_init, y, N_ITER, EPS, kind, trace=trace, **kw)
        _equal_traces(trace, want_trace, 1)
        assert torch.equal(got[0], want_x) and torch.equal(got[1], want_r) and torch.equal(got[2], want_l)
        assert model.calls == N_ITER + 1 and "draw_g" not in trace[0]


def test_iterations_per_graph():
    from eeadv import engine
    assert engine.MAX_ITERS_PER_GRAPH == 16
    want = {(100, 20): 1, (100, 1): 10, (10, 3): 5, (7, 20): 1}
    for (n, E), c in want.items():
        assert engine._eot_chunk(n, E) == c == ER.eot_chunk(n, E), (n, E)
        assert n % c == 0 and c <= max(1, 16 // E)
    for n in (1, 7, 10, 100):
        assert engine._eot_chunk(n, 1) == engine._chunk(n)
    assert engine._eot_chunk(100, 4) == 4 and engine._eot_chunk(100, 8) == 2 and engine._eot_chunk(16, 2) == 8


def test_abi_of_the_accumulate_kernel():
    import eeadv._native as n
    L = n.lib
    assert "ee_apgd_eot_acc_f32" in n.SIGNATURES and hasattr(L, "ee_apgd_eot_acc_f32")
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    assert L.ee_apgd_eot_acc_f32(p, q, p, p, p, 0, 0, 2, 8, None) == -2  # E < 1
    assert L.ee_apgd_eot_acc_f32(p, q, p, p, p, -1, 3, 2, 8, None) == -2 and L.ee_apgd_eot_acc_f32(p, q, p, p, p, 3, 3, 2, 8, None) == -2
    assert L.ee_apgd_eot_acc_f32(None, None, None, None, None, 3, 3, 0, 8, None) == -2  # a bad k is an error for an empty batch too
    assert L.ee_apgd_eot_acc_f32(None, None, None, None, None, 1, 3, 0, 8, None) == 0 and L.ee_apgd_eot_acc_f32(None, None, None, None, None, 0, 1, 3, 0, None) == 0
    assert L.ee_apgd_eot_acc_f32(p, q, p, p, p, 0, 1, -1, 8, None) == -2
    assert L.ee_apgd_eot_acc_f32(None, q, p, p, p, 0, 2, 2, 8, None) == -1 and L.ee_apgd_eot_acc_f32(p, q, None, p, p, 0, 2, 2, 8, None) == -1
    assert L.ee_apgd_eot_acc_f32(p, q, p, p, None, 0, 2, 2, 8, None) == -1
    assert L.ee_apgd_eot_acc_f32(p, p, p, p, p, 0, 2, 2, 8, None) == -2  # the accumulator is not the draw's gradient
    assert L.ee_apgd_eot_acc_f32(ctypes.c_void_p(4098), q, p, p, p, 0, 2, 2, 8, None) == -4
    assert L.ee_apgd_eot_acc_f32(p, q, ctypes.c_void_p(4100), p, p, 0, 2, 2, 8, None) == -4  # loss_acc holds doubles
    from eeadv import ops
    z = torch.zeros(2, 8)
    with pytest.raises(n.EEError):  # no CPU fallback
        ops.apgd_eot_acc_(z, z.clone(), torch.zeros(2, dtype=torch.float64), torch.zeros(2), torch.zeros(2), 0, 2)


def _tiny(seed=0):
    torch.manual_seed(seed)
    m = TinyNet(3, 8, NCLS, 5).eval()
    x = torch.rand(6, 3, 8, 8)
    with torch.no_grad():
        y = m(x).argmax(1)
    return m, x, y


def test_argument_errors(cpu_plumbing):
    import utils.attacks as A
    from eeadv import cascade, driver, engine, trainer
    m, x, y = _tiny()
    a = Args(epsilon=EPS, method_name="AT", attack_method="APGD-CE", random=True)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="eot_iter"):
            A.APGD(m, a, x, y, 2, eot_iter=bad)
        with pytest.raises(ValueError, match="eot_iter"):
            A._apgd_host(m, x, x, y, 2, EPS, "ce", eot_iter=bad)
        with pytest.raises(ValueError, match="eot_iter"):
            A.APGD_Rand(m, a, x, y, 2, eot_iter=bad)
        with pytest.raises(ValueError, match="eot_iter"):
            engine.apgd_loop(m, x, x, y, 2, EPS, "ce", eot_iter=bad)
        with pytest.raises(ValueError, match="eot_iter"):
            cascade.rand_stages(a, 2, bad)
        a.eot_iter = bad
        with pytest.raises(ValueError, match="eot_iter"):
            trainer.attack_for_validation(m, a, x, y, "cpu", 2, 0.01, NCLS)
    # the defaults: 20 for the rand methods, 1 for the single APGD runs, which honour a value; None and 1 are fine everywhere
    for method, e, want in (("Rand", None, 20), ("Cascade-Rand", None, 20), ("Rand", 5, 5), ("Cascade-Rand", 2, 2), ("APGD-CE", None, 1),
                            ("APGD-DLR", None, 1), ("APGD-CE", 7, 7), ("APGD-DLR", 3, 3), ("PGD", None, 1), ("Square", 1, 1), ("Cascade", None, 1)):
        assert trainer.eot_iter_for(Args(attack_method=method, eot_iter=e)) == want
    assert trainer.eot_iter_for(Args(attack_method="Rand")) == 20  # an args object without the key, as older callers build it
    # every method without EOT says so instead of ignoring the flag
    for method in ("APGD-T", "APGD", "FAB-T", "Square", "APGD+Square", "APGD+FAB+Square", "Cascade", "PGD", "FGSM", "CW"):
        a = Args(epsilon=EPS, method_name="AT", attack_method=method, random=True, eot_iter=2, square_queries=4, fab_iters=2)
        with pytest.raises(NotImplementedError, match=r"--eot_iter 2 with --attack_method %s: EOT is built for APGD-CE, APGD-DLR, Rand and "
                           r"Cascade-Rand only" % re.escape(method)):
            trainer.attack_for_validation(m, a, x, y, "cpu", 2, 0.01, NCLS)
    a = Args(epsilon=EPS, method_name="AT", attack_method="Cascade", random=True, eot_iter=2)
    with pytest.raises(NotImplementedError, match="EOT is built for"):
        driver.validate_cascade([(x, y)], m, a, torch.device("cpu"), 2, NCLS, print)
    # targeted training methods: untargeted evaluation only, as for the other evaluation attacks
    for method in ("APGD-DLR", "Rand"):
        a = Args(epsilon=EPS, method_name="tar_AT", attack_method=method, random=True, eot_iter=2)
        with pytest.raises(NotImplementedError, match="untargeted"):
            trainer.attack_for_validation(m, a, x, y, "cpu", 2, 0.01, NCLS)
    a = Args(epsilon=EPS, method_name="tar_AT", attack_method="Cascade-Rand", random=True, eot_iter=2)
    with pytest.raises(NotImplementedError, match="untargeted"):
        driver.validate_cascade([(x, y)], m, a, torch.device("cpu"), 2, NCLS, print)
    a.method_name = "AT"
    with pytest.raises(NotImplementedError, match="whole split"):
        trainer.attack_for_validation(m, a, x, y, "cpu", 2, 0.01, NCLS)
    # AA still stops
    a.attack_method, a.eot_iter = "AA", None
    with pytest.raises(NotImplementedError):
        trainer.attack_for_validation(m, a, x, y, "cpu", 2, 0.01, NCLS)
    # Rand needs three classes: 10 (MNIST) run, 2 do not - the message says which bound was missed
    two = TinyNet(3, 8, 2, 5).eval()
    a = Args(epsilon=EPS, method_name="AT", attack_method="Rand", random=True, eot_iter=2)
    for kw in ({}, {"nclass": 2}):
        with pytest.raises(ValueError, match=r"at least 3 classes and this model has 2 \(MNIST's 10 are enough"):
            A.APGD_Rand(two, a, x, y % 2, 2, 2, **kw)
    with pytest.raises(ValueError, match="at least 3 classes"):
        trainer.attack_for_validation(two, a, x, y % 2, "cpu", 2, 0.01, 2)
    a.attack_method = "Cascade-Rand"
    with pytest.raises(ValueError, match="at least 3 classes"):
        driver.validate_cascade([(x, y % 2)], two, a, torch.device("cpu"), 2, 2, print)


def test_rand_on_the_host(cpu_plumbing):
    """APGD_Rand = APGD-CE then APGD-DLR on the whole batch, flags ANDed, the first fooling point kept; the dispatch reaches it."""
    import utils.attacks as A
    from eeadv import trainer
    m, x, y = _tiny()
    y[0] = (y[0] + 1) % NCLS
    a = Args(epsilon=EPS, method_name="AT", attack_method="Rand", random=True, eot_iter=2)
    noise = torch.zeros_like(x).uniform_(-EPS, EPS)
    xa, rb = A.APGD_Rand(m, a, x, y, 4, 2, noise=noise)
    xc, rc = A.APGD(m, a, x, y, 4, "ce", noise=noise, eot_iter=2)
    xd, rd = A.APGD(m, a, x, y, 4, "dlr", noise=noise, eot_iter=2)
    assert torch.equal(rb, rc & rd) and not bool(rb[0])
    for b in range(x.shape[0]):
        assert torch.equal(xa[b], xc[b] if not rc[b] else (xd[b] if not rd[b] else x[b])), b
    torch.manual_seed(11)
    out = trainer.attack_for_validation(m, a, x, y, "cpu", 4, 0.01, NCLS)
    torch.manual_seed(11)
    want, _ = A.APGD_Rand(m, a, x, y, 4, 2, NCLS)
    assert torch.equal(out, want)
    a.attack_method = "APGD-DLR"
    torch.manual_seed(12)
    out = trainer.attack_for_validation(m, a, x, y, "cpu", 4, 0.01, NCLS)
    torch.manual_seed(12)
    want, _ = A.APGD(m, a, x, y, 4, "dlr", eot_iter=2)
    assert torch.equal(out, want)


def test_cascade_with_rand_stages_on_the_torch_compaction(cpu_plumbing, monkeypatch):
    """cascade.evaluate(stages=rand_stages(...)), 3 batches of 4, torch compaction, the two APGD runs scripted by sample: APGD-CE breaks the
    samples whose first pixel is 1, APGD-DLR those whose first pixel is 2.  APGD-DLR must see only survivors of APGD-CE, in full batches of 4
    regrouped across the incoming ones, each with the eot_iter the stages were built with."""
    import utils.attacks as A
    from eeadv import cascade
    N = 12
    code = [0, 1, 2, 0, 1, 1, 0, 2, 0, 0, 2, 1]  # per sample: 0 survives, 1 broken by CE, 2 broken by DLR
    wrong = [False] * N
    wrong[3] = True  # misclassified clean: never attacked
    x = torch.zeros(N, 1, 2, 2)
    for i in range(N):
        x[i, 0, 0, 0], x[i, 0, 0, 1] = code[i], i
    y = torch.zeros(N, dtype=torch.int64)

    class Model(torch.nn.Module):
        def forward(self, v):  # class 0 unless the sample is one of the clean mistakes
            z = torch.zeros(v.shape[0], NCLS)
            ids = v[:, 0, 0, 1].long()
            z[torch.arange(v.shape[0]), torch.tensor([1 if wrong[i] else 0 for i in ids.tolist()])] = 1.0
            return z
    calls = []

    def fake_apgd(model, args, inputs, targets, num_steps, loss='ce', y_target=None, noise=None, eot_iter=1):
        ids = inputs[:, 0, 0, 1].long().tolist()
        calls.append((loss, ids, num_steps, eot_iter))
        hit = inputs[:, 0, 0, 0] == (1 if loss == 'ce' else 2)
        return inputs + hit.view(-1, 1, 1, 1) * 0.5, ~hit
    monkeypatch.setattr(A, "APGD", fake_apgd)
    a = Args(epsilon=0.1, eot_iter=3)
    stages = cascade.rand_stages(a, 7)
    assert [n for n, _ in stages] == ["APGD-CE", "APGD-DLR"]
    res = cascade.evaluate(Model(), a, [(x[i:i + 4], y[i:i + 4]) for i in (0, 4, 8)], NCLS, stages=stages, keep_adv=True, compaction="torch")
    assert res.stage_names == ["APGD-CE", "APGD-DLR"] and res.n == N and res.clean_correct == N - 1
    want_stage = [0 if wrong[i] else (1 if code[i] == 1 else 2 if code[i] == 2 else 3) for i in range(N)]
    assert res.stage.tolist() == want_stage
    assert res.robust.tolist() == [s == 3 for s in want_stage]
    ce_rows = [i for i in range(N) if not wrong[i]]
    dlr_rows = [i for i in ce_rows if code[i] != 1]
    assert res.rows_attacked == [len(ce_rows), len(dlr_rows)]
    assert res.robust_after == [len(dlr_rows), sum(1 for s in want_stage if s == 3)]
    assert all(c[2] == 7 and c[3] == 3 for c in calls)
    seen = {"ce": [], "dlr": []}
    for loss, ids, _, _ in calls:
        assert len(ids) == 4  # always the one batch shape
        seen[loss].append(ids)
    n_ce, n_dlr = -(-len(ce_rows) // 4), -(-len(dlr_rows) // 4)
    assert len(seen["ce"]) == n_ce and len(seen["dlr"]) == n_dlr
    flat = lambda runs, n: [i for r in runs for i in r][:n]  # noqa: E731  (the tail of the last run is padding)
    assert flat(seen["ce"], len(ce_rows)) == ce_rows and flat(seen["dlr"], len(dlr_rows)) == dlr_rows
    for i in range(N):
        assert torch.equal(res.adv[i], x[i] + 0.5 if want_stage[i] in (1, 2) else x[i]), i
    # the explicit argument wins over args.eot_iter; without either the default is 20
    calls.clear()
    cascade.rand_stages(a, 2, 5)[1][1](Model(), a, x[:4], y[:4], None)
    cascade.rand_stages(Args(epsilon=0.1), 2)[0][1](Model(), a, x[:4], y[:4], None)
    assert [(c[0], c[3]) for c in calls] == [("dlr", 5), ("ce", 20)]


def test_mnist_driver_evaluates_with_cascade_rand_on_the_host(tmp_path):
    cfg = open(os.path.join(PKG, "MNIST", "configs_mnist", "adversarial_training.yml")).read()
    cfg = re.sub(r"num_steps_(\d): \d+", r"num_steps_\1: 3", cfg)
    path = tmp_path / "rand.yml"
    path.write_text(cfg)
    r = subprocess.run([sys.executable, "experiments_mnist.py", "-c", str(path), "--no-cuda", "--data", "synthetic", "--output-root", str(tmp_path),
                        "-e", "--attack_method", "Cascade-Rand", "--eot_iter", "2"], cwd=os.path.join(PKG, "MNIST"), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    logs = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path)) for f in fs if f == "log.txt"]
    assert logs
    for text in (r.stdout, "".join(open(f).read() for f in logs)):
        clean = re.findall(r"^ \* Cascade clean accuracy ([\d.]+)", text, flags=re.M)
        assert len(clean) >= 1
        per_stage = [re.findall(r"^ \* Cascade robust accuracy after %s ([\d.]+)" % re.escape(s), text, flags=re.M) for s in ("APGD-CE", "APGD-DLR")]
        assert all(len(v) == len(clean) for v in per_stage)
        assert not re.search(r"after (APGD-T|FAB-T|Square)", text)
        for k, c in enumerate(clean):
            vals = [float(c)] + [float(v[k]) for v in per_stage]
            assert all(p >= q for p, q in zip(vals, vals[1:])), vals
