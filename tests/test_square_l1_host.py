"""CPU: the plain-torch host path of utils.attacks.Square_L1 against tests/square_l1_reference.py (elements bit for bit when teacher-forced
on the host's norms and multiplier, every norm within one ulp of the exact one), the invariant of DESIGN.md section 21 at every query,
the doors that stay shut, the two new --attack_method values and cascade.l1_stages."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import square_l1_reference as R
from tiny_models import Args, TinyNet

NQ, SEED, K = 40, 99, 10
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "edge-enhancement_amd")
L1_METHODS = ("APGD-L1-CE", "APGD-L1-T", "APGD-L1", "FAB-L1-T", "APGD-L1+FAB", "Square-L1", "APGD-L1+FAB+Square")


class Scripted(torch.nn.Module):
    """A classifier whose margins are a script [n_forwards, B]: forward q returns logits with z[b, y_b] = script[q, b] and 0 elsewhere, so
    which proposals are accepted, rejected or fool the model is the test's choice."""

    def __init__(self, script, y):
        super().__init__()
        self.script, self.y, self.q = script, y, 0

    def forward(self, x):
        z = torch.zeros(x.shape[0], K, dtype=x.dtype, device=x.device)
        z[torch.arange(x.shape[0]), self.y] = self.script[self.q].to(x.dtype).to(x.device)
        self.q += 1
        return z


def script(B, nq=NQ, seed=3):
    """Sample 0 is misclassified at the start, 1 accepts every proposal, 2 is fooled half way, the rest accept some and reject some."""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(nq, B, generator=g, dtype=torch.float64) + 0.5
    m[:, 0] = -1.0
    m[:, 1] = torch.linspace(3.0, 1.0, nq, dtype=torch.float64)
    if B > 2:
        m[nq // 2:, 2] = -0.25
    return m


@pytest.fixture(scope="module")
def cpu_plumbing():
    from eeadv import runtime
    runtime.allow_cpu_plumbing(True)
    yield
    runtime.allow_cpu_plumbing(False)


def images(B, C, H, W, dtype=torch.float64, seed=0):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, C, H, W, generator=g, dtype=torch.float64).to(dtype)
    x0[:, :, 0, :] = 0.0  # exact ends of [0, 1]: the box binds there
    x0[:, :, 1, :] = 1.0
    return x0


@pytest.fixture(scope="module", params=[(3, 9, 9), (1, 28, 28), (3, 16, 20)], ids=["3x9x9", "1x28x28", "3x16x20"])
def host_run(request, cpu_plumbing):
    """One traced float64 host run per shape and the reference teacher-forced on its norms and multipliers, shared by the tests below."""
    import utils.attacks as A
    C, H, W = request.param
    B, D = 4, C * H * W
    eps = D / 256.0
    assert (C + 1) * eps <= D
    x0 = images(B, C, H, W)
    y = torch.arange(B) % K
    margins = script(B)
    trace = []
    out = A._square_l1_host(Scripted(margins, y), x0, y, NQ, eps, SEED, trace=trace, early_exit=False)
    ref = R.run(x0.numpy(), y.numpy(), NQ, eps, SEED, margins=margins.numpy(), lam0=trace[0]["lam"].numpy(),
                norms=[t["norms"].numpy() for t in trace[1:]], lam=[t["lam"].numpy() for t in trace[1:]])
    return x0, y, eps, trace, out, ref


def test_host_path_equals_the_reference_bit_for_bit(host_run):
    x0, y, eps, trace, (x_best, margin_min, queries), (samples, flags, _) = host_run
    assert x_best.dtype == torch.float64 and len(trace) == NQ
    assert torch.stack([t["flags"] for t in trace]).tolist() == flags
    assert sum(sum(f) for f in flags[1:]) >= 3 and any(not f[3] for f in flags[1:]), "the script must accept and reject"
    for b, s in enumerate(samples):
        for q in range(NQ):
            assert np.array_equal(trace[q]["x_new"][b].numpy(), s.iterates[q]), (b, q)
        assert np.array_equal(x_best[b].numpy(), s.x_best) and float(margin_min[b]) == float(s.margin_min) and int(queries[b]) == s.queries
        # each host norm within one ulp of the exactly summed one, the host's multiplier next to the reference's own
        assert abs(float(trace[0]["lam"][b]) - s.start_info["lam"]) <= 1e-12 * max(1.0, s.start_info["lam"])
        for i, own, info in s.norms:
            assert max(R.ulps(trace[i + 1]["norms"][:, b].numpy(), np.array(own))) <= 1, (b, i)
            assert abs(float(trace[i + 1]["lam"][b]) - info["lam"]) <= 1e-12 * max(1.0, info["lam"]), (b, i)
    assert not samples[0].norms and len(samples[1].norms) == NQ - 1 and len(samples[2].norms) == NQ // 2


def test_invariant_at_every_query(host_run):
    x0, y, eps, trace, _, _ = host_run
    D = x0[0].numel()
    for q, t in enumerate(trace):
        xn = t["x_new"].numpy()
        assert xn.min() >= 0 and xn.max() <= 1 and np.isfinite(xn).all()
        assert R.l1_excess(xn.reshape(len(xn), -1), x0.numpy().reshape(len(xn), -1), R.eps_p(eps)) <= D * 2.0 ** -23, q
    # the ball binds: some proposal is projected back (a positive multiplier)
    assert any(float(t["lam"].max()) > 0 for t in trace[1:])


def test_fooled_samples_are_frozen_and_the_public_function_wraps_the_run(host_run, cpu_plumbing):
    import utils.attacks as A
    x0, y, eps, trace, (x_best, margin_min, queries), (samples, _, _) = host_run
    assert int(queries[0]) == 1 and not samples[0].robust  # misclassified at the start: one forward, then frozen
    for t in trace[1:]:
        assert torch.equal(t["x_new"][0], trace[0]["x_new"][0]) and not bool(t["flags"][0]) and not bool(t["norms"][:, 0].any())
    assert int(queries[2]) == NQ // 2 + 1 and torch.equal(trace[-1]["x_new"][2], trace[NQ // 2]["x_new"][2])
    # determinism under a seed; the early exit changes nothing; another seed is another run
    margins = script(4)
    again = A._square_l1_host(Scripted(margins, y), x0, y, NQ, eps, SEED)
    assert all(torch.equal(a, b) for a, b in zip(again, (x_best, margin_min, queries)))
    other = A._square_l1_host(Scripted(margins, y), x0, y, NQ, eps, SEED + 1)
    assert not torch.equal(other[0], x_best)
    xa, robust, qs = A.Square_L1(Scripted(margins, y), Args(epsilon=eps), x0, y, n_queries=NQ, seed=SEED)
    assert torch.equal(robust, margin_min > 0) and torch.equal(qs, queries)
    assert torch.equal(xa, torch.where(robust.view(-1, 1, 1, 1), x0, x_best))


def test_eps_zero_is_the_clean_image(cpu_plumbing):
    import utils.attacks as A
    x0 = images(2, 3, 9, 9)
    y = torch.zeros(2, dtype=torch.int64)
    trace = []
    A._square_l1_host(Scripted(torch.ones(5, 2, dtype=torch.float64), y), x0, y, 5, 0.0, SEED, trace=trace, early_exit=False)
    assert len(trace) == 5 and all(torch.equal(t["x_new"], x0) for t in trace)
    with pytest.raises(ValueError, match="eps"):
        A._square_l1_host(Scripted(torch.ones(5, 2), y), x0, y, 5, -1.0, SEED)


def test_eps_p_and_the_float32_run(cpu_plumbing):
    import utils.attacks as A
    from eeadv import sqatk
    for eps in (12.0, 243 / 256.0, 0.3, 0.0, 1e-3):
        assert sqatk.l1_eps_p(eps) == R.eps_p(eps) <= float(np.float32(eps))
    assert sqatk.l1_eps_p(12.0) < 12.0
    # float32 images: the same run, elements bit for bit under the host's norms and multipliers
    x0 = images(3, 3, 9, 9, torch.float32)
    y = torch.arange(3)
    eps, nq = 243 / 256.0, 12
    margins, trace = script(3, nq), []
    A._square_l1_host(Scripted(margins, y), x0, y, nq, eps, SEED, trace=trace, early_exit=False)
    samples, _, _ = R.run(x0.numpy(), y.numpy(), nq, eps, SEED, margins=margins.numpy(), lam0=trace[0]["lam"].numpy(),
                          norms=[t["norms"].numpy() for t in trace[1:]], lam=[t["lam"].numpy() for t in trace[1:]])
    for b, s in enumerate(samples):
        assert all(np.array_equal(trace[q]["x_new"][b].numpy(), s.iterates[q]) for q in range(nq)), b
        for i, own, _ in s.norms:
            assert max(R.ulps(trace[i + 1]["norms"][:, b].numpy(), np.array(own))) <= 1, (b, i)


# ---- the doors ---------------------------------------------------------------------------------------------------------------------------
def _problem(B=4):
    torch.manual_seed(0)
    model = TinyNet(3, 8, K, seed=0).eval()
    x = torch.rand(B, 3, 8, 8)
    with torch.no_grad():
        z = model(x)
    return model, x, z.argmax(1), z


def test_the_old_doors_stay_shut(cpu_plumbing):
    import utils.attacks as A
    from eeadv import cascade, engine, trainer
    model, x0, y, _ = _problem()
    args = Args(epsilon=0.5)
    for call in (lambda: A.Square(model, args, x0, y, 5, seed=1, norm="L1"),
                 lambda: A._square_host(model, x0, y, 5, 0.5, 1, norm="L1"),
                 lambda: engine.square_loop(model, x0, y, 5, 0.5, seed=1, norm="L1"),
                 lambda: engine._SquareRun(x0, y, 5, 0.5, norm="L1"),
                 lambda: cascade.default_stages(args, 5, K, norm="L1")):
        with pytest.raises(ValueError, match="norm"):
            call()
    assert engine.SQUARE_NORMS == ("Linf", "L2")
    assert trainer.L1_METHODS == L1_METHODS and trainer.L1_SQUARE_METHODS == L1_METHODS[5:]
    assert set(L1_METHODS) <= set(trainer.EVAL_METHODS) and not set(L1_METHODS) & set(trainer.L2_METHODS)
    for method in L1_METHODS:
        a = Args(epsilon=0.5, method_name="AT", attack_method=method, random=True)
        assert trainer.norm_tag(a) == " [norm L1]" and trainer.eot_iter_for(a) == 1
        for norm in ("L1", "L2"):
            a.norm = norm
            with pytest.raises((ValueError, NotImplementedError), match="norm"):
                trainer.attack_for_validation(model, a, x0, y, "cpu", 2, 0.1, K)
        a.norm, a.eot_iter = None, 2
        with pytest.raises(NotImplementedError, match="eot_iter"):
            trainer.attack_for_validation(model, a, x0, y, "cpu", 2, 0.1, K)
        a.eot_iter, a.method_name = None, "tar_AT"
        with pytest.raises(NotImplementedError, match="untargeted"):
            trainer.attack_for_validation(model, a, x0, y, "cpu", 2, 0.1, K)


def test_driver_dispatch_reaches_the_l1_square_door(cpu_plumbing, monkeypatch):
    import utils.attacks as A
    from eeadv import trainer
    model, x0, y, _ = _problem()
    B = x0.shape[0]
    calls = []
    ones = torch.ones(B, dtype=torch.bool)
    monkeypatch.setattr(A, "APGD_L1", lambda m, a, x, t, n, loss: (calls.append(("ce", n)), (x + 0, ones))[1])
    monkeypatch.setattr(A, "APGD_T_L1", lambda m, a, x, t, n, k: (calls.append(("t", n)), (x + 0, ones))[1])
    monkeypatch.setattr(A, "FAB_T_L1", lambda m, a, x, t, k, n: (calls.append(("fab", n)), (x + 0, ones, torch.zeros(B)))[1])
    monkeypatch.setattr(A, "Square_L1", lambda m, a, x, t, n: (calls.append(("sq", n)), (x + 0, ones, torch.zeros(B)))[1])
    for method, want in (("Square-L1", [("sq", 11)]), ("APGD-L1+FAB+Square", [("ce", 5), ("t", 5), ("fab", 7), ("sq", 11)])):
        a = Args(epsilon=0.5, method_name="AT", attack_method=method, random=True, fab_iters=7, square_queries=11)
        calls.clear()
        out = trainer.attack_for_validation(model, a, x0, y, "cpu", 5, 0.1, K)
        assert calls == want and out.shape == x0.shape
    # the ensemble keeps the first fooling point and ANDs the flags
    monkeypatch.setattr(A, "FAB_T_L1", lambda m, a, x, t, k, n: (x + 0.25, torch.tensor([True, False, True, True]), torch.zeros(B)))
    monkeypatch.setattr(A, "Square_L1", lambda m, a, x, t, n: (x + 0.5, torch.tensor([True, False, False, True]), torch.zeros(B)))
    out = trainer.attack_for_validation(model, Args(epsilon=0.5, method_name="AT", attack_method="APGD-L1+FAB+Square", random=True), x0, y, "cpu",
                                        5, 0.1, K)
    assert torch.equal(out[1], x0[1] + 0.25) and torch.equal(out[2], x0[2] + 0.5) and torch.equal(out[0], x0[0]) and torch.equal(out[3], x0[3])


@pytest.mark.parametrize("method", ["Square-L1", "APGD-L1+FAB+Square"])
def test_the_l1_square_run_through_the_dispatch(cpu_plumbing, method):
    from eeadv import trainer
    model, x0, y, _ = _problem()
    eps = 0.5
    a = Args(epsilon=eps, method_name="AT", attack_method=method, random=True, fab_iters=3, square_queries=8)
    torch.manual_seed(0)
    out = trainer.attack_for_validation(model, a, x0, y, "cpu", 3, 0.1, K)
    assert out.shape == x0.shape and float(out.min()) >= 0 and float(out.max()) <= 1
    dist = (out - x0).flatten(1).abs().double().sum(dim=1)
    assert bool((dist <= eps * (1 + 192 * 2.0 ** -23)).all())


def test_l1_stages_run_through_the_cascade_on_the_host(cpu_plumbing):
    from eeadv import cascade
    model, x, y, z = _problem(8)
    eps = 0.5
    args = Args(epsilon=eps, fab_iters=3, square_queries=8, num_steps_1=3, n_target_classes=2)
    stages = cascade.l1_stages(args, 3, K, n_target_classes=2)
    assert [name for name, _ in stages] == ["APGD-L1-CE", "APGD-T-L1", "FAB-T-L1", "Square-L1"]
    assert [name for name, _ in cascade.default_stages(args, 3, K)] == list(cascade.STAGES)  # unchanged
    order = torch.sort(z, dim=1, descending=True, stable=True)[1][:, :3].contiguous()
    for name, fn in stages:
        torch.manual_seed(0)
        x_adv, robust = fn(model, args, x, y, order)
        assert x_adv.shape == x.shape and robust.shape == (8,) and robust.dtype == torch.bool, name
        assert float((x_adv - x).flatten(1).abs().double().sum(dim=1).max()) <= eps * (1 + 192 * 2.0 ** -23), name
        assert float(x_adv.min()) >= 0 and float(x_adv.max()) <= 1 and torch.equal(x_adv[robust], x[robust]), name
    torch.manual_seed(0)
    res = cascade.evaluate(model, args, [(x[:4], y[:4]), (x[4:], y[4:])], K, stages=stages, num_steps=3)
    assert res.n == 8 and list(res.stage_names) == [name for name, _ in stages] and res.robust.shape == (8,)
    assert res.clean_correct == 8 and len(res.robust_after) == 4 and all(a >= b for a, b in zip(res.robust_after, res.robust_after[1:]))


# ---- a driver run ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["Square-L1", "APGD-L1+FAB+Square"])
def test_mnist_driver_evaluates_square_l1_on_the_host(tmp_path, method):
    cfg = open(os.path.join(PKG, "MNIST", "configs_mnist", "adversarial_training.yml")).read()
    cfg = re.sub(r"num_steps_(\d): \d+", r"num_steps_\1: 2", cfg)
    cfg = re.sub(r"batch_size: \d+", "batch_size: 4", cfg)
    path = tmp_path / "l1.yml"
    path.write_text(cfg)
    r = subprocess.run([sys.executable, "experiments_mnist.py", "-c", str(path), "--no-cuda", "--data", "synthetic:1:1", "--output-root",
                        str(tmp_path), "-e", "--attack_method", method, "--fab_iters", "2", "--square_queries", "4"],
                       cwd=os.path.join(PKG, "MNIST"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert re.findall(r"^ \* Adv Prec@1 [\d.]+ Prec@5 [\d.]+ \[norm L1\]$", r.stdout, flags=re.M)
