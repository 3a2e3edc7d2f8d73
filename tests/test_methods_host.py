"""CPU: the dispatch from --attack_method to the doors of utils.attacks, characterised call by call.

Every door is replaced by a recording fake; trainer.attack_for_validation is driven for every evaluation method that runs per batch, and every
stage of cascade.default_stages / l1_stages / rand_stages is called once.  What is recorded per call - the door, the number of positional
arguments, their values (tensors, the model and the args objects by name), the sorted keyword items - and the returned tensor must equal
tests/methods_expected.py, which the same recorder wrote at the commit before the dispatch became a table (python tests/test_methods_host.py
prints it).

A fake keeps the doors' contract: a robust sample's row of x_adv is the clean row, a fooled one's is x plus a constant of the door.  The
dispatch may rely on that contract - A._first_fooling starts from the clean batch where a written-out torch.where ladder started from the
first member's x_adv, and the two agree exactly because of it - so a fake that moved robust rows too would test a door that does not exist.
The robust flags are one fixed pattern per door, overlapping, so that in every ensemble each member is the first to fool some sample, a
later member's point must lose against an earlier one's, and samples 4 and 5 survive everything."""
import pprint

import pytest
import torch

from tiny_models import Args

B = 6
# door (and, for APGD, loss) -> (the samples it fools, the constant it adds to their rows, outputs)
FAKES = {
    ("APGD", "ce"): ((0,), 2.0, 2), ("APGD", "dlr"): ((1,), 4.0, 2), ("APGD_T", None): ((0, 1), 8.0, 2), ("FAB_T", None): ((1, 2), 16.0, 3),
    ("FAB", None): ((1, 2), 32.0, 3), ("Square", None): ((2, 3), 64.0, 3), ("APGD_Rand", None): ((0, 1), 128.0, 2),
    ("APGD_L1", "ce"): ((0,), 256.0, 2), ("APGD_T_L1", None): ((0, 1), 512.0, 2), ("FAB_T_L1", None): ((1, 2), 1024.0, 3),
    ("FAB_L1", None): ((1, 2), 2048.0, 3), ("Square_L1", None): ((2, 3), 4096.0, 3),
}
DOORS = sorted({door for door, _ in FAKES})
APGD_DOORS = ("APGD", "APGD_T", "APGD_L1", "APGD_T_L1", "APGD_Rand")
FAB_DOORS = ("FAB", "FAB_T", "FAB_L1", "FAB_T_L1")
MODEL = object()


def _batch():
    x = torch.arange(B * 2, dtype=torch.float32).view(B, 1, 1, 2) / 64
    return x, torch.arange(B) % 3, torch.arange(B * 4).view(B, 4) % 10


class Recorder:
    """Installs the fakes on utils.attacks; .calls is what they saw, .returned the x_adv tensors they handed back."""

    def __init__(self, monkeypatch, names):
        import utils.attacks as A
        self.calls, self.returned, self.names = [], [], names
        for door in DOORS:
            monkeypatch.setattr(A, door, self._fake(door))

    def _name(self, v):
        for name, obj in self.names.items():
            if v is obj:
                return "<%s>" % name
        assert not isinstance(v, torch.Tensor), "a tensor the test did not hand in"
        return v

    def _fake(self, door):
        def fake(*a, **kw):
            self.calls.append((door, len(a), tuple(self._name(v) for v in a), tuple(sorted((k, self._name(v)) for k, v in kw.items()))))
            fooled, c, n_out = FAKES[(door, a[5] if door in ("APGD", "APGD_L1") else None)]
            x = a[2]
            robust = torch.ones(x.shape[0], dtype=torch.bool)
            robust[list(fooled)] = False
            x_adv = torch.where(robust.view(-1, 1, 1, 1), x, x + c)
            self.returned.append(x_adv)
            return (x_adv, robust, None)[:n_out]
        return fake

    def take(self):
        calls, self.calls = self.calls, []
        return calls


def _settings(trainer, method):
    """The option sets a method is driven with: none, both restart counts at 3 (refused by whatever lacks an APGD or a FAB), each count at 3
    where the method takes it, --norm L2 and --eot_iter 3 (refusals are part of the record)."""
    each = {}
    if method in trainer.APGD_RESTART_METHODS:
        each["apgd_restarts"] = 3
    if method in trainer.FAB_RESTART_METHODS:
        each["fab_restarts"] = 3
    return {"plain": {}, "both3": {"apgd_restarts": 3, "fab_restarts": 3}, "each3": each, "L2": {"norm": "L2"}, "eot3": {"eot_iter": 3}}


def _outcome(fn, rec):
    try:
        out = fn()
    except (NotImplementedError, ValueError) as e:
        return {"calls": rec.take(), "raised": (type(e).__name__, str(e))}
    return {"calls": rec.take(), "out": out.tolist()}


def record(monkeypatch):
    """{case: outcome} over the per-batch methods and the cascade's stage lists; also the method tuples, which derive from the same table."""
    from eeadv import cascade, trainer
    x, y, order = _batch()
    names = {"model": MODEL, "x": x, "y": y, "order": order}
    rec = Recorder(monkeypatch, names)
    got = {}
    for method in trainer.EVAL_METHODS:
        if method in trainer.CASCADE_METHODS:
            continue
        for tag, opts in _settings(trainer, method).items():
            args = names["args"] = Args(epsilon=0.1, method_name="AT", attack_method=method, fab_iters=2, square_queries=7, **opts)
            got["%s/%s" % (method, tag)] = _outcome(lambda: trainer.attack_for_validation(MODEL, args, x, y, "cpu", 5, 0.01, 10), rec)
    # the stage lists: built from one args object, called with another - what a builder reads, it reads when it builds
    for tag, opts in (("plain", {}), ("both3", {"apgd_restarts": 3, "fab_restarts": 3})):
        built = names["built"] = Args(epsilon=0.1, fab_iters=2, square_queries=7, eot_iter=4, **opts)
        args = names["args"] = Args(epsilon=0.1, fab_iters=9, square_queries=9, eot_iter=9, apgd_restarts=9, fab_restarts=9)
        lists = {"default": cascade.default_stages(built, 5, 10), "default-t3-L2": cascade.default_stages(built, 5, 10, n_target_classes=3, norm="L2"),
                 "l1": cascade.l1_stages(built, 5, 10), "l1-t3": cascade.l1_stages(built, 5, 10, 3), "rand": cascade.rand_stages(built, 5),
                 "rand-e2-L2": cascade.rand_stages(built, 5, 2, "L2")}
        for name, stages in lists.items():
            got["stages:%s/%s" % (name, tag)] = [stage for stage, _ in stages]
            for stage, fn in stages:
                def run(fn=fn):
                    x_adv, robust = fn(MODEL, args, x, y, order)
                    return torch.cat([x_adv.flatten(1), robust.view(-1, 1).float()], 1)  # one tensor that shows both
                got["stage:%s:%s/%s" % (name, stage, tag)] = _outcome(run, rec)
    tuples = ("APGD_METHODS", "SQUARE_METHODS", "FAB_METHODS", "RAND_METHODS", "CASCADE_METHODS", "L2_METHODS", "L1_FAB_METHODS", "L1_SQUARE_METHODS",
              "L1_METHODS", "FAB_U_METHODS", "L1_FAB_U_METHODS", "FAB_RESTART_METHODS", "APGD_RESTART_METHODS", "EVAL_METHODS")
    got["tuples"] = {name: getattr(trainer, name) for name in tuples}
    return got


def test_the_dispatch_makes_the_calls_it_made_before_the_table(monkeypatch):
    from methods_expected import EXPECTED
    got = record(monkeypatch)
    assert sorted(got) == sorted(EXPECTED)
    for case, want in EXPECTED.items():
        assert got[case] == want, case
    # the record is worth something: every member of the two full ensembles is the first to fool a sample, and two samples survive
    x = _batch()[0]
    for method, consts in (("APGD+FAB+Square", (2.0, 8.0, 16.0, 64.0)), ("APGD-L1+FAB+Square", (256.0, 512.0, 1024.0, 4096.0))):
        out = torch.tensor(got[method + "/plain"]["out"])
        assert [float((out - x)[b].max()) for b in range(B)] == [consts[0], consts[1], consts[2], consts[3], 0.0, 0.0]


def test_a_plan_of_one_member_returns_the_doors_own_tensor(monkeypatch):
    from eeadv import trainer
    x, y, order = _batch()
    rec = Recorder(monkeypatch, {"model": MODEL, "x": x, "y": y})
    single = []
    for method in trainer.EVAL_METHODS:
        if method in trainer.CASCADE_METHODS:
            continue
        args = rec.names["args"] = Args(epsilon=0.1, method_name="AT", attack_method=method, fab_iters=2, square_queries=7)
        del rec.returned[:]
        out = trainer.attack_for_validation(MODEL, args, x, y, "cpu", 5, 0.01, 10)
        if len(rec.returned) == 1:
            assert out is rec.returned[0], method  # no extra launch behind a single attack
            single.append(method)
    assert single == ["APGD-CE", "APGD-T", "Square", "FAB-T", "APGD-DLR", "Rand", "APGD-L1-CE", "APGD-L1-T", "FAB-L1-T", "Square-L1", "FAB-U", "FAB-L1-U"]


def test_the_doors_are_looked_up_when_a_member_runs(monkeypatch):
    """eeadv.trainer and eeadv.cascade are imported, and a stage list is built, BEFORE the doors are replaced: the replacement is what runs."""
    import utils.attacks as A
    from eeadv import cascade, trainer
    x, y, order = _batch()
    built = Args(epsilon=0.1)
    stages = cascade.default_stages(built, 5, 10) + cascade.l1_stages(built, 5, 10) + cascade.rand_stages(built, 5)
    rec = Recorder(monkeypatch, {"model": MODEL, "x": x, "y": y, "order": order, "args": built})
    for _, fn in stages:
        fn(MODEL, built, x, y, order)
    assert [c[0] for c in rec.take()] == ["APGD", "APGD_T", "FAB_T", "Square", "APGD_L1", "APGD_T_L1", "FAB_T_L1", "Square_L1", "APGD", "APGD"]
    args = rec.names["args"] = Args(epsilon=0.1, method_name="AT", attack_method="Custom")
    trainer.attack_for_validation(MODEL, args, x, y, "cpu", 5, 0.01, 10)
    assert [c[0] for c in rec.take()] == ["APGD", "FAB"]
    seen = []
    monkeypatch.setattr(A, "FAB", lambda *a, **kw: seen.append("second") or (a[2], torch.ones(B, dtype=torch.bool), None))
    trainer.attack_for_validation(MODEL, args, x, y, "cpu", 5, 0.01, 10)
    assert seen == ["second"] and [c[0] for c in rec.take()] == ["APGD"]


def test_the_restart_tuples_name_the_methods_that_run_an_apgd_or_a_fab(monkeypatch):
    from eeadv import cascade, trainer
    x, y, order = _batch()
    rec = Recorder(monkeypatch, {"model": MODEL, "x": x, "y": y, "order": order})
    for method in trainer.EVAL_METHODS:
        args = rec.names["args"] = Args(epsilon=0.1, method_name="AT", attack_method=method)
        if method in trainer.CASCADE_METHODS:
            stages = cascade.rand_stages(args, 5) if method == trainer.CASCADE_RAND_METHOD else cascade.default_stages(args, 5, 10)
            for _, fn in stages:
                fn(MODEL, args, x, y, order)
        else:
            trainer.attack_for_validation(MODEL, args, x, y, "cpu", 5, 0.01, 10)
        doors = {c[0] for c in rec.take()}
        assert bool(doors & set(APGD_DOORS)) == (method in trainer.APGD_RESTART_METHODS), method
        assert bool(doors & set(FAB_DOORS)) == (method in trainer.FAB_RESTART_METHODS), method


if __name__ == "__main__":  # the recorder's output as the literal of tests/methods_expected.py
    import conftest  # noqa: F401  (puts the package on sys.path)
    with pytest.MonkeyPatch.context() as mp:
        print("EXPECTED = " + pprint.pformat(record(mp), width=150, compact=True))
