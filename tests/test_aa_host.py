"""CPU: utils/aa.py and what it stands on - the stage lists of cascade.aa_stages call by call, the unchanged stage
lists underneath, the per-stage restart counts with scripted members, and the script's main on the host path against direct calls."""
import re

import pytest
import torch

import aa_cases as C
from methods_expected import EXPECTED
from test_methods_host import MODEL, Recorder, _batch, record
from tiny_models import Args

TWO_M23 = 2.0 ** -23


@pytest.fixture()
def cpu_plumbing():
    from eeadv import runtime
    runtime.allow_cpu_plumbing(True)
    yield
    runtime.allow_cpu_plumbing(False)


# ---- the stage lists ---------------------------------------------------------------------------------------------------------------------
def _kw(norm, **kw):
    """The sorted keyword items of a recorded call: the norm only where it is not Linf."""
    if norm != "Linf":
        kw["norm"] = norm
    return tuple(sorted(kw.items()))


def _calls_of(monkeypatch, version, norm, n_class=10, **opts):
    """[(stage name, the one recorded call)] of aa_stages(version, norm): built from one args object, called with another."""
    from eeadv import cascade
    x, y, order = _batch()
    built = Args(epsilon=0.1, fab_iters=2, square_queries=7, **opts)
    args = Args(epsilon=0.1, fab_iters=9, square_queries=9, eot_iter=9, apgd_restarts=9, fab_restarts=9, n_target_classes=1)
    rec = Recorder(monkeypatch, {"model": MODEL, "x": x, "y": y, "order": order, "args": args})
    out = []
    for name, fn in cascade.aa_stages(built, 5, n_class, version, norm):
        fn(MODEL, args, x, y, order)
        calls = rec.take()
        assert len(calls) == 1, (name, calls)
        out.append((name, calls[0]))
    return out


HEAD = ("<model>", "<args>", "<x>", "<y>")


@pytest.mark.parametrize("norm", ("Linf", "L2"))
def test_plus_is_six_stages_with_their_own_restart_counts(monkeypatch, norm):
    got = _calls_of(monkeypatch, "plus", norm, apgd_restarts=3, fab_restarts=4)  # the counts of the options do not reach a stage that has its own
    assert got == [
        ("APGD-CE", ("APGD", 6, HEAD + (5, "ce"), _kw(norm, n_restarts=5))),
        ("APGD-DLR", ("APGD", 6, HEAD + (5, "dlr"), _kw(norm, n_restarts=5))),
        ("FAB-U", ("FAB", 5, HEAD + (2,), _kw(norm, n_restarts=5))),
        ("Square", ("Square", 5, HEAD + (7,), _kw(norm))),
        ("APGD-T", ("APGD_T", 7, HEAD + (5, 10, 9), _kw(norm, order="<order>"))),  # one restart: no keyword; 9 targets
        ("FAB-T", ("FAB_T", 7, HEAD + (10, 2, 9), _kw(norm, order="<order>"))),
    ]


@pytest.mark.parametrize("norm", ("Linf", "L2"))
def test_custom_is_apgd_ce_and_fab_u_with_two_restarts(monkeypatch, norm):
    assert _calls_of(monkeypatch, "custom", norm) == [
        ("APGD-CE", ("APGD", 6, HEAD + (5, "ce"), _kw(norm, n_restarts=2))),
        ("FAB-U", ("FAB", 5, HEAD + (2,), _kw(norm, n_restarts=2))),
    ]


@pytest.mark.parametrize("norm", ("Linf", "L2"))
@pytest.mark.parametrize("eot", (None, 2))
def test_rand_is_the_rand_stages_with_eot(monkeypatch, norm, eot):
    opts = {} if eot is None else {"eot_iter": eot}
    E = 20 if eot is None else eot
    assert _calls_of(monkeypatch, "rand", norm, **opts) == [
        ("APGD-CE", ("APGD", 6, HEAD + (5, "ce"), _kw(norm, eot_iter=E))),
        ("APGD-DLR", ("APGD", 6, HEAD + (5, "dlr"), _kw(norm, eot_iter=E))),
    ]


@pytest.mark.parametrize("norm,key,opts", (("Linf", "default", {}), ("L2", "default-t3-L2", {"n_target_classes": 3}), ("L1", "l1", {}),
                                           ("L1", "l1-t3", {"n_target_classes": 3})))
@pytest.mark.parametrize("tag,restarts", (("plain", {}), ("both3", {"apgd_restarts": 3, "fab_restarts": 3})))
def test_standard_is_the_stage_list_of_the_parent_commit(monkeypatch, norm, key, opts, tag, restarts):
    """standard makes, stage by stage, the calls tests/methods_expected.py recorded for default_stages / l1_stages before this file existed."""
    got = _calls_of(monkeypatch, "standard", norm, eot_iter=4, **opts, **restarts)
    assert [name for name, _ in got] == EXPECTED["stages:%s/%s" % (key, tag)]
    for name, call in got:
        assert [call] == EXPECTED["stage:%s:%s/%s" % (key, name, tag)]["calls"], name


def test_the_target_count_follows_the_class_count(monkeypatch):
    got = dict(_calls_of(monkeypatch, "plus", "Linf", n_class=5))
    assert got["APGD-T"][2][-1] == 4 and got["FAB-T"][2][-1] == 4  # min(9, n_class - 1)


def test_unsupported_combinations_stop_with_their_message():
    from eeadv import cascade
    a = Args(epsilon=0.1)
    table = {"standard": ("Linf", "L2", "L1"), "plus": ("Linf", "L2"), "rand": ("Linf", "L2"), "custom": ("Linf", "L2")}
    assert cascade.AA_VERSIONS == table
    for version, norms in table.items():
        for norm in ("Linf", "L2", "L1"):
            if norm in norms:
                assert cascade.aa_stages(a, 5, 10, version, norm)
            else:
                with pytest.raises(NotImplementedError, match="nearest supported combination is version standard under L1"):
                    cascade.aa_stages(a, 5, 10, version, norm)
    with pytest.raises(ValueError, match="version must be one of standard, plus, rand, custom"):
        cascade.aa_stages(a, 5, 10, "fast", "Linf")
    with pytest.raises(ValueError, match="norm must be one of Linf, L2, L1"):
        cascade.aa_stages(a, 5, 10, "standard", "L0")
    for version in ("plus", "rand"):
        with pytest.raises(ValueError, match="at least 4 classes and this model has 3"):
            cascade.aa_stages(a, 5, 3, version, "Linf")
    assert len(cascade.aa_stages(a, 5, 3, "standard", "Linf")) == 4 and len(cascade.aa_stages(a, 5, 3, "custom", "Linf")) == 2


def test_default_l1_and_rand_stages_are_unchanged(monkeypatch):
    """The three stage lists that existed make the calls of the parent commit (tests/methods_expected.py), names and returned tensors included."""
    got = record(monkeypatch)
    keys = [k for k in EXPECTED if k.startswith("stage")]
    assert len(keys) > 40
    for k in keys:
        assert got[k] == EXPECTED[k], k


# ---- per-stage restart counts, with scripted members ---------------------------------------------------------------------------------------
def test_every_scripted_stage_is_called_with_its_own_count(cpu_plumbing, monkeypatch):
    """Four scripted members in a cascade over 10 samples of 1x2x2 (pixel 0: the stage that breaks the sample, pixel 1: its id): a stage with
    a count gets it as both restart keywords, one restart is no keyword, a stage without one gets the counts of the options."""
    from eeadv import cascade, methods
    seen = []

    def member(k):
        def fn(model, args, x, y, ctx):
            flat = x.flatten(1)
            seen.append((k, dict(ctx.akw), dict(ctx.rkw), ctx.order.shape[0]))
            return x + k, flat[:, 0] != k
        return fn
    for k in range(1, 5):
        monkeypatch.setitem(methods.MEMBERS, "S%d" % k, member(k))
    breaks = [5, 1, 2, 3, 4, 5, 2, 5, 4, 3]
    x = torch.zeros(10, 1, 2, 2)
    x[:, 0, 0, 0] = torch.tensor(breaks, dtype=torch.float32)
    x[:, 0, 0, 1] = torch.arange(10, dtype=torch.float32)
    y = torch.zeros(10, dtype=torch.int64)

    class Zero(torch.nn.Module):
        def forward(self, x):
            return -torch.arange(4, dtype=x.dtype).repeat(x.shape[0], 1)  # class 0 everywhere: every sample is clean-correct
    a = Args(epsilon=0.1, apgd_restarts=3, fab_restarts=4)
    ctx = methods.context(a, 5, 4, **cascade._restarts(a))
    stages = cascade._stages([cascade.Stage("S1", 5), cascade.Stage("S2", 1), "S3", ("S4", 2)], ctx)
    res = cascade.evaluate(Zero(), a, [(x[i:i + 4], y[i:i + 4]) for i in range(0, 10, 4)], 4, keep_adv=True, stages=stages, per_stage_adv=True)
    assert res.stage.tolist() == breaks and res.stage_names == ["S1", "S2", "S3", "S4"]
    want = {1: ({"n_restarts": 5}, {"n_restarts": 5}), 2: ({}, {}), 3: ({"n_restarts": 3}, {"n_restarts": 4}), 4: ({"n_restarts": 2}, {"n_restarts": 2})}
    assert {k for k, *_ in seen} == {1, 2, 3, 4}
    for k, akw, rkw, b in seen:
        assert (akw, rkw) == want[k] and b == 4, (k, akw, rkw)
    # per_stage_adv: the ids a stage broke, ascending, and their rows of adv
    for k, part in enumerate(res.stage_adv, 1):
        ids = [i for i, s in enumerate(breaks) if s == k]
        assert part.name == "S%d" % k and part.ids.tolist() == ids and torch.equal(part.adv, x[ids] + k) and torch.equal(part.adv, res.adv[ids])
    with pytest.raises(ValueError, match="keep_adv"):
        cascade.evaluate(Zero(), a, [(x, y)], 4, stages=stages, per_stage_adv=True)
    with pytest.raises(ValueError, match="at least 1"):
        cascade._stages([cascade.Stage("S1", 0)], ctx)


# ---- the host restatement of the check -----------------------------------------------------------------------------------------------------
def test_pert_check_host_on_a_case_worked_by_hand(cpu_plumbing):
    from eeadv import ops
    nan, inf = float("nan"), float("inf")
    x0 = torch.tensor([[0.0, 0.5, 1.0, 0.25], [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0], [0.5, 0.5, 0.5, 0.5], [0.5, nan, 0.5, 0.5]])
    xa = torch.tensor([[0.75, 0.5, 0.0, 0.25], [nan, 2.0, -1.0, 0.0], [1.0, 1.0, 1.0, 1.0], [nan, nan, nan, nan], [0.5, 0.25, inf, 0.5]])
    norms, rng, n_nan = ops._pert_check_host(xa, x0)
    assert norms[0].tolist() == [1.0, 1.25, 1.75] and rng[0].tolist() == [0.0, 0.75] and n_nan.tolist() == [0, 1, 0, 4, 0]
    assert all(v != v for v in norms[1].tolist()) and rng[1].tolist() == [-1.0, 2.0]
    assert norms[2].tolist() == [0.0, 0.0, 0.0] and rng[2].tolist() == [1.0, 1.0]
    assert all(v != v for v in norms[3].tolist()) and rng[3].tolist() == [inf, -inf]
    assert all(v != v for v in norms[4].tolist()) and rng[4].tolist() == [0.25, inf]  # a NaN of x0 alone: NaN norms, no NaN counted
    t = ops.pert_check(xa.view(5, 1, 2, 2), x0.view(5, 1, 2, 2))  # CPU tensors under the opt-in: the same three as tensors
    assert t[0].dtype == torch.float32 and t[2].dtype == torch.int32 and t[2].tolist() == [0, 1, 0, 4, 0]


def test_pert_check_refuses_cpu_tensors_without_the_opt_in():
    from eeadv import ops
    x = torch.zeros(2, 4)
    with pytest.raises(RuntimeError, match="allow_cpu_plumbing"):
        ops.pert_check(x, x)


# ---- the script on the host ----------------------------------------------------------------------------------------------------------------
def _direct(version, norm="Linf"):
    from eeadv import cascade
    from utils.helper import set_seed
    a = C.args_for(norm)
    model = C.build_model().eval()
    set_seed(C.SEED)
    return cascade.evaluate(model, a, C.batches(), C.N_CLASS, keep_adv=True, stages=cascade.aa_stages(a, C.NUM_STEPS, C.N_CLASS, version, norm), n=C.N)


@pytest.mark.parametrize("version", ("standard", "plus", "custom"))
def test_main_on_the_host_saves_what_the_cascade_returns(cpu_plumbing, monkeypatch, tmp_path, capsys, version):
    import utils.aa as aa
    from eeadv import ops
    C.register(monkeypatch, aa)
    out = aa.main(C.script_argv(tmp_path, version, "Linf", "--no-cuda"))
    text = capsys.readouterr().out
    want = _direct(version)
    x, y = C.samples()
    saved = torch.load(out.path, weights_only=True)
    assert out.path.endswith("aa_%s_Linf_%d_eps_%.5f.pth" % (version, C.N, C.EPS["Linf"]))
    assert saved.device.type == "cpu" and saved.shape == (C.N,) + C.SHAPE and torch.equal(saved.view(torch.int32), want.adv.view(torch.int32))
    assert torch.equal(out.result.robust, want.robust) and torch.equal(out.result.stage, want.stage)
    # the printed figures: clean, one per stage, the final one = robust.mean()
    final = re.findall(r"^ \* AA robust accuracy ([\d.]+)$", text, flags=re.M)
    assert final == ["%.3f" % (100.0 * float(want.robust.float().mean()))]
    assert re.findall(r"^ \* AA clean accuracy ([\d.]+)$", text, flags=re.M) == ["%.3f" % (100.0 * (C.N - len(C.WRONG)) / C.N)]
    stages = re.findall(r"^ \* AA robust accuracy after (\S+) ([\d.]+)$", text, flags=re.M)
    assert [s for s, _ in stages] == want.stage_names and [v for _, v in stages] == ["%.3f" % (100.0 * r / C.N) for r in want.robust_after]
    assert "NOT the autoattack package" in text.splitlines()[0] and "sections 14, 23, 24" in text.splitlines()[1]
    assert "no --resume" in text
    # the same lines in the log file
    log = open(C.script_argv(tmp_path, version)[-1]).read()
    assert all(line in log for line in text.splitlines() if line.startswith(" * AA") or "perturbation" in line)
    # the points: inside the ball for every row, the clean-misclassified rows untouched
    norms, rng, n_nan = ops._pert_check_host(saved, x)
    print("Linf per row", norms[:, 0], "bound", C.EPS["Linf"] + TWO_M23)
    assert bool((norms[:, 0].astype("float64") <= C.EPS["Linf"] + TWO_M23).all()) and int(n_nan.sum()) == 0
    assert rng[:, 0].min() >= 0.0 and rng[:, 1].max() <= 1.0
    assert out.check.outside == 0 and "perturbation check: 0 of %d samples outside the Linf ball" % C.N in text and "WARNING" not in text
    assert re.search(r"^max Linf perturbation: [\d.]+, nan in tensor: 0, max: [\d.]+, min: [\d.]+$", text, flags=re.M)
    for i in C.WRONG:
        assert int(want.stage[i]) == 0 and torch.equal(saved[i].view(torch.int32), x[i].view(torch.int32))
    assert int((want.stage >= 1).sum()) >= 1  # something was attacked and broken: the comparison above is about points, not about copies of x


def test_main_warns_about_points_outside_the_ball(cpu_plumbing, monkeypatch, tmp_path, capsys):
    """A stage list whose one stage leaves the ball: the check counts the rows and the warning line names the largest norm."""
    import utils.aa as aa
    from eeadv import cascade
    C.register(monkeypatch, aa)
    monkeypatch.setattr(cascade, "aa_stages", lambda *a, **kw: [("Far", lambda model, args, x, y, order: (
        (x + 0.25).clamp(0, 1), torch.zeros(x.shape[0], dtype=torch.bool)))])
    out = aa.main(C.script_argv(tmp_path, "custom", "Linf", "--no-cuda", "--n_ex", "6"))
    text = capsys.readouterr().out
    assert out.n == 6 and out.check.outside == 5 and "WARNING: 5 samples exceed epsilon" in text  # 6 samples, one of them (2) misclassified clean


def test_main_evaluates_without_saving_when_the_points_do_not_fit(cpu_plumbing, monkeypatch, tmp_path, capsys):
    import utils.aa as aa
    from eeadv import cascade
    C.register(monkeypatch, aa)
    real = cascade.evaluate

    def evaluate(*a, keep_adv=False, **kw):
        if keep_adv:
            raise MemoryError("keep_adv needs 9.0 GiB")
        return real(*a, keep_adv=False, **kw)
    monkeypatch.setattr(cascade, "evaluate", evaluate)
    out = aa.main(C.script_argv(tmp_path, "custom", "Linf", "--no-cuda"))
    text = capsys.readouterr().out
    assert out.path is None and out.check is None and "evaluating without saving" in text and " * AA robust accuracy " in text


def test_main_reads_a_checkpoint_through_the_drivers_reader(cpu_plumbing, monkeypatch, tmp_path, capsys):
    import utils.aa as aa
    C.register(monkeypatch, aa)
    m = C.build_model()
    with torch.no_grad():
        m.w2.mul_(-1.0)  # other weights than the initialised model's: the clean accuracy moves
    state = {"module." + k: v for k, v in m.state_dict().items()}
    state["module.sobel.weight"] = torch.zeros(3)
    ckpt = str(tmp_path / "ckpt.pth")
    torch.save({"epoch": 3, "state_dict": state, "best_prec1": 0.0}, ckpt)
    out = aa.main(C.script_argv(tmp_path, "custom", "Linf", "--no-cuda", "--resume", ckpt))
    text = capsys.readouterr().out
    assert "(epoch 3); ignored keys: 1" in text and out.clean_correct < C.N - len(C.WRONG)


@pytest.mark.parametrize("version", ("custom", "standard"))
def test_individual_keeps_every_members_own_points(cpu_plumbing, monkeypatch, tmp_path, capsys, version):
    import utils.aa as aa
    import utils.attacks as A
    from eeadv import cascade
    from utils.helper import set_seed
    C.register(monkeypatch, aa)
    out = aa.main(C.script_argv(tmp_path, version, "Linf", "--no-cuda", "--individual"))
    saved = torch.load(out.path, weights_only=True)
    assert out.path.endswith("aa_%s_Linf_%d_eps_%.5f_individual.pth" % (version, C.N, C.EPS["Linf"]))
    a, model, rows = C.args_for(), C.build_model().eval(), C.batches()
    if version == "custom":  # the doors themselves, on every whole batch, from the run's seed
        doors = {"APGD-CE": lambda x, y: A.APGD(model, a, x, y, C.NUM_STEPS, "ce", n_restarts=2)[0],
                 "FAB-U": lambda x, y: A.FAB(model, a, x, y, C.FAB_ITERS, n_restarts=2)[0]}
    else:  # the stages of the version, which carry the targets' class order
        def door(fn):
            def run(x, y):
                with torch.no_grad():
                    order = torch.sort(model(x), dim=1, descending=True, stable=True)[1][:, :C.N_CLASS].contiguous()
                return fn(model, a, x, y, order)[0]
            return run
        doors = {name: door(fn) for name, fn in cascade.aa_stages(a, C.NUM_STEPS, C.N_CLASS, version, "Linf")}
    assert list(saved) == list(doors)
    for name, run in doors.items():
        set_seed(C.SEED)
        want = torch.cat([run(x, y) for x, y in rows])
        assert saved[name].shape == (C.N,) + C.SHAPE and torch.equal(saved[name].view(torch.int32), want.view(torch.int32)), name
        assert out.check[name].outside == 0
    text = capsys.readouterr().out
    assert all(" * AA individual robust accuracy of %s " % name in text for name in doors)
