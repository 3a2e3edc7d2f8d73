"""CPU: APGD restarts.  The host restatement of the kernel's draws (eeadv.apgdstart) against the explicit Philox of
tests/apgd_start_reference.py, the keys of the starts, the start point in the three threat models, the plain-torch host runs of
utils/attacks.py with restarts against separate one-restart runs from the same starts, the ABI of the two launches, the dispatch and the
drivers."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import apgd_start_reference as S
from test_fab_u_host import _mnist, cpu_plumbing  # noqa: F401  (cpu_plumbing is a fixture)
from tiny_models import Args, TinyNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ("Linf", "L2", "L1")
EPS = {"Linf": 0.1, "L2": 1.0, "L1": 6.0}
U24 = 2.0 ** -24


# ---- the draws -------------------------------------------------------------------------------------------------------------------------
def test_the_stream_id_is_16_and_nobody_elses():
    from eeadv import apgdstart, fabstart
    assert apgdstart.STREAM_APGD_START == S.STREAM == 16
    assert S.STREAM not in S.TAKEN and len(set(S.TAKEN)) == 7 and fabstart.STREAM_FAB_START in S.TAKEN
    text = open(os.path.join(ROOT, "edge-enhancement_amd", "csrc", "ee_common.hpp")).read()
    assert re.search(r"kStreamApgdStart = 16u;", text) and re.search(r"kStreamFabStart = 15u;", text)
    # the same key under the two streams: different draws, and FAB's are the bits they were
    assert not np.array_equal(apgdstart.draw(5, 2, 8, "Linf"), fabstart.draw(5, 2, 8, "Linf"))
    assert np.array_equal(fabstart.draw(5, 2, 8, "Linf"), fabstart.draw(5, 2, 8, "Linf", 15))
    assert np.array_equal(apgdstart.draw(5, 2, 8, "L2"), fabstart.draw(5, 2, 8, "L2", 16))


@pytest.mark.parametrize("D", [1, 3, 5, 75, 192])
def test_uniform_draw_is_the_reference_bit_for_bit(D):
    from eeadv import apgdstart
    for seed, B in ((0, 1), (0x0123456789ABCDEF, 3), (2 ** 64 - 1, 2)):
        t = apgdstart.draw(seed, B, D, "Linf")
        assert t.dtype == np.float32 and t.shape == (B, D)
        want = np.stack([S.draw_row(seed, b, D, "Linf") for b in range(B)])
        assert np.array_equal(t.astype(np.float64), want)  # 2 u - 1 is exact in both
        assert (t >= -1).all() and (t < 1).all()


@pytest.mark.parametrize("metric", ["L2", "L1"])
@pytest.mark.parametrize("D", [1, 3, 5, 75, 192])
def test_normal_draw_is_the_reference_to_float32_rounding(D, metric):
    """Both sides form the value in float64 from the same words and the same float32 angle; they differ by the libm of numpy against that
    of math (a few 2^-53) and the one cast to float32: |t - ref| <= 2^-24 |ref| (1 + 2^-20)."""
    from eeadv import apgdstart
    seed, B = 0xFEDCBA9876543210, 3
    t = apgdstart.draw(seed, B, D, metric).astype(np.float64)
    want = np.stack([S.draw_row(seed, b, D, metric) for b in range(B)])
    assert (np.abs(t - want) <= U24 * np.abs(want) * (1 + 2.0 ** -20)).all()
    assert np.array_equal(apgdstart.draw(seed, B, D, "L2"), apgdstart.draw(seed, B, D, "L1"))  # one normal draw for both


def test_a_row_depends_on_seed_row_and_element_only():
    from eeadv import apgdstart
    for metric in METRICS:
        a, b = apgdstart.draw(5, 7, 75, metric), apgdstart.draw(5, 3, 75, metric)
        assert np.array_equal(a[:3], b)  # row b of a B = 7 draw is row b of a B = 3 draw
        assert np.array_equal(apgdstart.draw(5, 2, 192, metric)[:, :75], a[:2])  # nor on D
        assert not np.array_equal(a[0], a[1]) and not np.array_equal(a, apgdstart.draw(6, 7, 75, metric))


def test_every_target_index_and_restart_has_a_key_of_its_own():
    from eeadv import apgdstart, fabstart
    assert apgdstart.seed_of is fabstart.seed_of
    keys = {apgdstart.seed_of(seed, j, r) for seed in (0, 1, 2 ** 63) for j in range(10) for r in range(1, 6)}
    assert len(keys) == 3 * 10 * 5 and all(0 <= k < 2 ** 64 for k in keys)


# ---- the start point -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_start_against_the_reference(metric):
    from eeadv import apgdstart
    g = torch.Generator().manual_seed(3)
    B, D, eps = 4, 75, EPS[metric]
    x0 = torch.rand(B, 3, 5, 5, generator=g, dtype=torch.float64)
    t = torch.randn(B, 3, 5, 5, generator=g, dtype=torch.float64) if metric != "Linf" else torch.rand(B, 3, 5, 5, generator=g, dtype=torch.float64) * 2 - 1
    got = apgdstart.start(x0, eps, t, metric)
    want = np.stack([S.start_row(x0[b].reshape(-1).numpy(), eps, t[b].reshape(-1).numpy(), metric) for b in range(B)])
    # float64 on both sides, the same operations; the L2 norm is summed in another order (one ulp of n, carried into s and the product)
    assert got.dtype == torch.float64 and np.abs(got.reshape(B, D).numpy() - want).max() <= 8 * 2.0 ** -53 * max(1.0, np.abs(want).max())
    if metric == "L1":
        assert bool((got < 0).any()) and bool((got > 1).any())  # not clamped: the run projects
    else:
        assert bool((got >= 0).all()) and bool((got <= 1).all())
    # float32, in the kernel's order: Linf and L1 have no sum, so numpy float32 gives the same bits
    x32, t32 = x0.float(), t.float()
    got32 = apgdstart.start(x32, eps, t32, metric)
    assert got32.dtype == torch.float32
    if metric != "L2":
        assert np.array_equal(got32.reshape(B, D).numpy(), S.start_f32(x32.reshape(B, D).numpy(), eps, t32.reshape(B, D).numpy(), metric))
    with pytest.raises(ValueError, match="metric"):
        apgdstart.start(x0, eps, t, "L3")


def test_l2_start_on_dyadic_noise_is_the_float32_restatement_and_a_bad_row_is_x0():
    from eeadv import apgdstart
    g = torch.Generator().manual_seed(4)
    B, D = 3, 75
    x0 = torch.randint(0, 257, (B, D), generator=g).float() / 256
    t = torch.randint(-512, 513, (B, D), generator=g).float() / 256  # every double sum of squares is exact in any order
    t[1, 7] = float("inf")
    got = apgdstart.start(x0, 0.125, t, "L2").numpy()
    assert np.array_equal(got, S.start_f32(x0.numpy(), 0.125, t.numpy(), "L2"))
    assert np.array_equal(got[1], x0[1].numpy()) and not np.array_equal(got[0], x0[0].numpy())
    t[2, 0] = float("nan")
    assert np.array_equal(apgdstart.start(x0, 0.125, t, "L2")[2].numpy(), x0[2].numpy())
    # the order of utils.attacks._l2_start on a finite draw: the same bits
    import utils.attacks as A
    tf = torch.randn(B, D, generator=g)
    assert torch.equal(apgdstart.start(x0, 0.5, tf, "L2"), A._l2_start(x0, 0.5, tf))


# ---- the host runs -----------------------------------------------------------------------------------------------------------------------
def _case(dtype=torch.float32):
    """TinyNet on 3x8x8, B = 5; the labels are the clean predictions for rows 0 - 3 (robust at the start) and a wrong class for row 4."""
    torch.manual_seed(11)
    m = TinyNet(3, 8, 10, seed=5).to(dtype).eval()
    x0 = torch.rand(5, 3, 8, 8, dtype=dtype)
    with torch.no_grad():
        y = m(x0).argmax(dim=1)
    y[4] = (y[4] + 1) % 10
    return m, x0, y


def _run(metric, m, x0, x, y, n_iter=6, **kw):
    import utils.attacks as A
    if metric == "L1":
        return A._apgd_l1_host(m, x0, x, y, n_iter, EPS["L1"], "ce", **kw)
    if metric == "EOT":
        return A._apgd_host(m, x0, x, y, n_iter, EPS["Linf"], "ce", eot_iter=2, **kw)
    return A._apgd_host(m, x0, x, y, n_iter, EPS[metric], "ce", norm=metric, **kw)


def _first_start(metric, x0):
    from eeadv import apgdstart
    g = torch.Generator().manual_seed(9)
    key = "Linf" if metric == "EOT" else metric
    t = torch.randn(x0.shape, generator=g) if key != "Linf" else torch.rand(x0.shape, generator=g) * 2 - 1
    return apgdstart.start(x0, EPS[key], t.to(x0.dtype), key)


@pytest.mark.parametrize("metric", ["Linf", "L2", "EOT", "L1"])
def test_one_restart_is_the_call_without_the_argument(metric):
    m, x0, y = _case()
    x = _first_start(metric, x0)
    one = _run(metric, m, x0, x, y)
    state = torch.get_rng_state()
    again = _run(metric, m, x0, x, y, n_restarts=1, seed=None)
    assert torch.equal(torch.get_rng_state(), state)  # no ticket, no draw
    assert all(torch.equal(a, b) for a, b in zip(one, again))
    with pytest.raises(ValueError, match="n_restarts"):
        _run(metric, m, x0, x, y, n_restarts=0)


@pytest.mark.parametrize("metric", ["Linf", "L2", "EOT", "L1"])
def test_three_restarts_are_three_runs_combined_by_first_fooling(metric):
    import utils.attacks as A
    from eeadv import apgdstart
    m, x0, y = _case()
    key = "Linf" if metric == "EOT" else metric
    x = _first_start(metric, x0)
    g = torch.Generator().manual_seed(21)
    noise = torch.randn((2,) + tuple(x0.shape), generator=g) if key != "Linf" else torch.rand((2,) + tuple(x0.shape), generator=g) * 2 - 1
    three = _run(metric, m, x0, x, y, n_restarts=3, noise=noise)
    starts = [x] + [apgdstart.start(x0, EPS[key], noise[r], key) for r in range(2)]
    runs = [_run(metric, m, x0, s, y) for s in starts]
    x_adv, robust = A._first_fooling(x0, [(xa, rb) for xa, rb, _ in runs])
    assert torch.equal(three[1], robust) and torch.equal(three[0], x_adv)
    assert torch.equal(three[2], torch.stack([r[2] for r in runs]).max(dim=0)[0])
    # robust never turns from False to True across restarts
    seen = torch.ones_like(robust)
    for n in (1, 2, 3):
        rb = _run(metric, m, x0, x, y, n_restarts=n, noise=noise[:n - 1] if n > 1 else None)[1]
        assert not bool((rb & ~seen).any())
        seen = rb
    assert not bool(three[1][4])  # the mislabelled row is fooled from the start


def test_seeded_host_restarts_use_the_host_draw_and_the_target_index():
    import utils.attacks as A
    from eeadv import apgdstart
    m, x0, y = _case()
    x = _first_start("Linf", x0)
    trace = []
    A._apgd_host(m, x0, x, y, 2, 0.1, "ce", trace=trace, n_restarts=2, seed=99, target_index=4)
    assert len(trace) == 2 * 3  # per restart: the start point and two iterations
    draw = torch.from_numpy(apgdstart.draw(apgdstart.seed_of(99, 4, 1), 5, 192, "Linf")).view(x0.shape)
    assert torch.equal(trace[3]["x"], apgdstart.start(x0, 0.1, draw, "Linf")) and torch.equal(trace[0]["x"], x)
    other = []
    A._apgd_host(m, x0, x, y, 2, 0.1, "ce", trace=other, n_restarts=2, seed=99, target_index=5)
    assert not torch.equal(other[3]["x"], trace[3]["x"])


def test_public_doors_take_restarts_on_the_host(cpu_plumbing):
    import utils.attacks as A
    m, x0, y = _case()
    g = torch.Generator().manual_seed(2)
    un, nn_ = torch.rand(x0.shape, generator=g) * 0.2 - 0.1, torch.randn(x0.shape, generator=g)
    doors = ((A.APGD, dict(noise=un), 0.1), (A.APGD, dict(noise=nn_, norm="L2"), 1.0), (A.APGD_L1, dict(noise=nn_), 6.0),
             (A.APGD_T, dict(nclass=10, n_target_classes=2, noise=un), 0.1), (A.APGD_T_L1, dict(nclass=10, n_target_classes=2, noise=nn_), 6.0),
             (A.APGD_Rand, dict(eot_iter=2, nclass=10, noise=un), 0.1))
    for door, kw, eps in doors:
        one = door(m, Args(epsilon=eps), x0, y, 4, **kw)
        state = torch.get_rng_state()
        again = door(m, Args(epsilon=eps), x0, y, 4, n_restarts=1, seed=7, **kw)
        assert torch.equal(torch.get_rng_state(), state)
        assert all(torch.equal(a, b) for a, b in zip(one, again))
        three = door(m, Args(epsilon=eps), x0, y, 4, n_restarts=3, seed=7, **kw)
        same = door(m, Args(epsilon=eps), x0, y, 4, n_restarts=3, seed=7, **kw)
        assert all(torch.equal(a, b) for a, b in zip(three, same))  # the seed is all that enters the draws
        assert not bool((three[1] & ~one[1]).any())  # restart 0 is the one run: what it fooled stays fooled
        fooled = ~one[1]
        assert torch.equal(three[0][fooled], one[0][fooled])  # and keeps its first fooling point
        with pytest.raises(ValueError, match="n_restarts"):
            door(m, Args(epsilon=eps), x0, y, 4, n_restarts=0, **kw)


# ---- the dispatch ------------------------------------------------------------------------------------------------------------------------
def test_apgd_restarts_for_accepts_and_refuses_the_right_methods():
    from eeadv import trainer
    runs_apgd = ("APGD-CE", "APGD-T", "APGD", "APGD-DLR", "Rand", "APGD+Square", "APGD+FAB+Square", "APGD-L1-CE", "APGD-L1-T", "APGD-L1",
                 "APGD-L1+FAB", "APGD-L1+FAB+Square", "Cascade", "Cascade-Rand", "Custom")
    assert set(trainer.APGD_RESTART_METHODS) == set(runs_apgd)
    for method in runs_apgd:
        assert trainer.apgd_restarts_for(Args(attack_method=method, apgd_restarts=3)) == {"n_restarts": 3}
        assert trainer.apgd_restarts_for(Args(attack_method=method, apgd_restarts=1)) == {}
        assert trainer.apgd_restarts_for(Args(attack_method=method)) == {}
    for method in ("PGD", "FGSM", "CW", "Square", "Square-L1", "FAB-T", "FAB-U", "FAB-L1-T", "FAB-L1-U", "AA"):
        assert trainer.apgd_restarts_for(Args(attack_method=method, apgd_restarts=1)) == {}
        with pytest.raises(NotImplementedError, match="apgd_restarts"):
            trainer.apgd_restarts_for(Args(attack_method=method, apgd_restarts=2))
    with pytest.raises(ValueError, match="apgd_restarts"):
        trainer.apgd_restarts_for(Args(attack_method="APGD-CE", apgd_restarts=0))


def test_custom_is_an_evaluation_method_that_takes_both_counts():
    from eeadv import trainer
    assert "Custom" in trainer.EVAL_METHODS and "Custom" in trainer.FAB_RESTART_METHODS and "AA" not in trainer.EVAL_METHODS
    assert "Custom" not in trainer.L2_METHODS
    args = Args(attack_method="Custom", apgd_restarts=2, fab_restarts=2)
    assert trainer.apgd_restarts_for(args) == {"n_restarts": 2} and trainer.fab_restarts_for(args) == {"n_restarts": 2}
    with pytest.raises(NotImplementedError):
        trainer.norm_for(Args(attack_method="Custom", norm="L2"))
    with pytest.raises(NotImplementedError):
        trainer.eot_iter_for(Args(attack_method="Custom", eot_iter=2))
    # fab_restarts_for keeps refusing what runs no FAB
    with pytest.raises(NotImplementedError, match="fab_restarts"):
        trainer.fab_restarts_for(Args(attack_method="APGD-CE", fab_restarts=2))


def test_the_dispatch_and_the_cascade_stages_hand_the_count_on(cpu_plumbing, monkeypatch):
    import utils.attacks as A
    from eeadv import cascade, trainer
    seen = []

    def fake(name, n_out):
        def f(*a, **kw):
            seen.append((name, kw))
            return (a[2], torch.ones(len(a[2]), dtype=torch.bool), None)[:n_out]
        return f
    for name, n_out in (("APGD", 2), ("APGD_T", 2), ("APGD_L1", 2), ("APGD_T_L1", 2), ("FAB", 3), ("FAB_T", 3), ("FAB_T_L1", 3)):
        monkeypatch.setattr(A, name, fake(name, n_out))
    x, y = torch.rand(2, 1, 4, 4), torch.zeros(2, dtype=torch.int64)
    for restarts, want in ((None, {}), (1, {}), (3, {"n_restarts": 3})):
        args = Args(epsilon=0.1, fab_iters=2, method_name="AT")
        if restarts is not None:
            args.apgd_restarts = restarts
        del seen[:]
        for name, fn in cascade.default_stages(args, 2, 10)[:2] + cascade.l1_stages(args, 2, 10)[:2] + cascade.rand_stages(args, 2, 2):
            fn(None, args, x, y, None)
        for method in ("APGD", "APGD-L1", "APGD-DLR", "Custom"):
            args.attack_method = method
            trainer.attack_for_validation(None, args, x, y, "cpu", 2, 0.01, 10)
        apgd = [kw for name, kw in seen if name.startswith("APGD")]
        assert len(apgd) == 2 + 2 + 2 + 2 + 2 + 1 + 1
        for kw in apgd:
            assert {k: v for k, v in kw.items() if k in ("n_restarts", "seed")} == want
        assert [kw.get("n_restarts") for name, kw in seen if name == "FAB"] == [None]  # Custom's FAB reads --fab_restarts, not this


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_two_launches():
    import eeadv._native as n
    from eeadv import ops
    L = n.lib
    for name in ("ee_apgd_start_f32", "ee_apgd_merge_f32"):
        assert name in n.SIGNATURES and hasattr(L, name)
    assert hasattr(ops, "apgd_start_") and hasattr(ops, "apgd_merge_")
    assert L.ee_prof_read(29, None, None) != -2 and L.ee_prof_read(30, None, None) == -2  # no new timing family
    p = ctypes.c_void_p(4096)
    names = ("x", "x0", "noise", "B", "D", "eps", "metric", "seed", "path", "stream")
    ok = (p, p, None, 2, 8, 0.1, 0, 5, 0, None)

    def start(**kw):
        a = dict(zip(names, ok))
        a.update(kw)
        return L.ee_apgd_start_f32(*[a[k] for k in names])

    # every call below stops at an argument check (or has B = 0): nothing is launched
    for name in ("x", "x0"):
        assert start(**{name: None}) == -1, name
    assert start(B=-1) == -2 and start(D=0) == -2 and start(eps=-0.1) == -2 and start(eps=float("nan")) == -2
    assert start(metric=3) == -2 and start(metric=-1) == -2 and start(path=3) == -2 and start(path=-1) == -2
    assert start(D=12289, path=1) == -3  # the resident path ends at 3*64*64
    assert start(B=0, x=None, x0=None) == 0  # an empty batch launches nothing
    assert start(x=ctypes.c_void_p(4098)) == -4 and start(noise=ctypes.c_void_p(4098)) == -4
    mnames = ("adv_all", "robust_all", "loss_all", "x_best_adv", "robust_run", "loss_run", "B", "D", "first", "stream")
    mok = (p, p, p, p, p, p, 2, 8, 0, None)

    def merge(**kw):
        a = dict(zip(mnames, mok))
        a.update(kw)
        return L.ee_apgd_merge_f32(*[a[k] for k in mnames])

    for name in mnames[:6]:
        assert merge(**{name: None}) == -1, name
        assert merge(**{name: ctypes.c_void_p(4098)}) == -4, name
    assert merge(B=-1) == -2 and merge(D=0) == -2
    assert merge(B=0, adv_all=None) == 0
    x = torch.rand(2, 8)
    with pytest.raises(n.EEError):
        ops.apgd_start_(x.clone(), x, 0.1, "Linf")  # CPU tensors: no fallback
    with pytest.raises(ValueError, match="metric"):
        ops.apgd_start_(x.clone(), x, 0.1, "L3")


# ---- drivers ---------------------------------------------------------------------------------------------------------------------------
def test_mnist_driver_runs_custom_with_both_restart_counts_on_the_host(tmp_path):
    r = _mnist(tmp_path, "--attack_method", "Custom", "--fab_iters", "2", "--apgd_restarts", "2", "--fab_restarts", "2")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    logs = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path)) for f in fs if f.startswith("log")]
    text = r.stdout + "".join(open(f).read() for f in logs)
    assert re.search(r"^ \* Custom: APGD, 2 restarts per run, each on the whole batch$", text, flags=re.M)
    assert re.search(r"^ \* Custom: K = 10 classes, 10 backward passes per iteration, 2 iterations, 2 restarts$", text, flags=re.M)
    assert text.index("2 restarts per run") < text.index("Test_clean")  # before the first batch
    clean = re.findall(r"^ \* Clean Prec@1 ([\d.]+)", text, flags=re.M)
    adv = re.findall(r"^ \* Adv Prec@1 ([\d.]+) Prec@5 ([\d.]+)$", text, flags=re.M)
    assert len(clean) >= 1 and len(clean) == len(adv)
    for c1, (a1, _) in zip(clean, adv):
        assert float(a1) <= float(c1)


def test_mnist_driver_stops_on_restarts_for_a_method_without_apgd(tmp_path):
    r = _mnist(tmp_path, "--attack_method", "Square", "--apgd_restarts", "2")
    assert r.returncode != 0 and "NotImplementedError" in r.stderr and "apgd_restarts" in r.stderr
    assert "Adv Prec@1" not in r.stdout
