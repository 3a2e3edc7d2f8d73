"""GPU: the versions of utils/aa.py on the device, with the tiny model and budgets of tests/test_aa_host.py.

Per case (version, norm) three runs of cascade.evaluate over the stage list of cascade.aa_stages from one seed - device pools eager, torch
staging eager, device pools under graph replay - must agree in robust, stage and the bits of adv; the script's saved file must hold the
same adv, and its check must find every row inside the ball under ball_tolerance."""
import os
import re

import pytest
import torch

import aa_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = (("standard", "Linf"), ("standard", "L1"), ("plus", "Linf"), ("custom", "Linf"))


class _Graph:
    """EEADV_GRAPH set for a block, put back after it."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("EEADV_GRAPH")
        os.environ["EEADV_GRAPH"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("EEADV_GRAPH", None)
        else:
            os.environ["EEADV_GRAPH"] = self.old


@pytest.fixture(scope="module")
def device_state():
    """A first graph capture creates the device draw state from a ticket of torch's generator (eeadv.runtime.draw_state): create it before
    the runs, so that every run below starts from the generator its seed gives."""
    from eeadv import engine, runtime
    torch.cuda.init()  # the generators exist once the device is initialised
    runtime.draw_state(torch.device(DEV))
    yield
    engine.clear_graphs()


def _evaluate(version, norm, graph, compaction):
    from eeadv import cascade
    from utils.helper import set_seed
    a = C.args_for(norm)
    model = C.build_model().to(DEV).eval()
    with _Graph(graph):
        set_seed(C.SEED)
        return cascade.evaluate(model, a, C.batches(DEV), C.N_CLASS, keep_adv=True, compaction=compaction,
                                stages=cascade.aa_stages(a, C.NUM_STEPS, C.N_CLASS, version, norm), n=C.N)


def _same(p, q):
    print("differing: robust %d, stage %d, adv rows %d; rows %s / %s" % (int((p.robust != q.robust).sum()), int((p.stage != q.stage).sum()),
          int((p.adv.view(torch.int32) != q.adv.view(torch.int32)).flatten(1).any(1).sum()), p.rows_attacked, q.rows_attacked))
    return torch.equal(p.robust, q.robust) and torch.equal(p.stage, q.stage) and torch.equal(p.adv.view(torch.int32), q.adv.view(torch.int32))


@pytest.mark.parametrize("version,norm", CASES)
def test_pools_staging_graph_and_script_agree(device_state, monkeypatch, tmp_path, capsys, version, norm):
    import utils.aa as aa
    from eeadv import ops
    hip = _evaluate(version, norm, "0", None)
    assert _same(hip, _evaluate(version, norm, "0", "torch"))  # device pools against the torch staging
    graph = _evaluate(version, norm, "1", None)
    assert _same(hip, graph)  # eager against graph replay
    C.register(monkeypatch, aa)
    with _Graph("1"):
        out = aa.main(C.script_argv(tmp_path, version, norm))
    text = capsys.readouterr().out
    saved = torch.load(out.path, weights_only=True)
    assert saved.device.type == "cpu" and torch.equal(saved.view(torch.int32), graph.adv.cpu().view(torch.int32))
    assert torch.equal(out.result.robust, graph.robust) and torch.equal(out.result.stage, graph.stage)
    assert re.findall(r"^ \* AA robust accuracy ([\d.]+)$", text, flags=re.M) == ["%.3f" % (100.0 * float(graph.robust.float().mean()))]
    # the check: every row inside the ball under the tolerance the attacks' own statements give, nothing outside the box, no NaN
    x, _ = C.samples(DEV)
    norms, rng, n_nan = ops.pert_check(graph.adv, x)
    col = norms[:, aa.NORM_COLUMN[norm]].double().cpu()
    tol = aa.ball_tolerance(norm, C.EPS[norm], x[0].numel())
    print("%s norms per row %s tolerance %.9g" % (norm, col.tolist(), tol))
    assert bool((col <= tol).all()) and int(n_nan.sum()) == 0 and float(rng[:, 0].min()) >= 0.0 and float(rng[:, 1].max()) <= 1.0
    assert out.check.outside == 0 and out.check.tolerance == tol and "WARNING" not in text
    assert "perturbation check: 0 of %d samples outside the %s ball" % (C.N, norm) in text
    broken = (graph.stage >= 1) & (graph.stage <= len(graph.stage_names))
    assert int(broken.sum()) >= 1 and torch.equal(graph.adv[~broken].view(torch.int32), x[~broken].view(torch.int32))
    assert bool((col[broken.cpu()] > 0).all())


def test_tolerances_are_the_stated_ones():
    import utils.aa as aa
    assert aa.ball_tolerance("Linf", 8 / 255, 192) == 8 / 255 + 2.0 ** -23
    assert aa.ball_tolerance("L2", 0.5, 192) == 0.5 * (1 + 1.5 * 2.0 ** -23) + 5 * 1.2e-8 <= 0.5 * (1 + 4 * 2.0 ** -23)  # section 16's bound at eps = 0.5
    assert aa.ball_tolerance("L1", 1.5, 192) == 1.5 + 192 * 2.0 ** -23


def test_rand_with_two_draws_completes(device_state, monkeypatch, tmp_path, capsys):
    """Plumbing: the untrained model has no randomised layer, so the two EOT draws are equal; the run must complete with flags of the
    right shape and points inside the ball."""
    import utils.aa as aa
    C.register(monkeypatch, aa)
    with _Graph("1"):
        out = aa.main(C.script_argv(tmp_path, "rand", "Linf", "--eot_iter", "2"))
    res = out.result
    assert res.stage_names == ["APGD-CE", "APGD-DLR"] and res.robust.shape == (C.N,) and res.robust.dtype == torch.bool
    assert res.stage.shape == (C.N,) and res.adv.shape == (C.N,) + C.SHAPE and len(res.robust_after) == 2
    assert out.check.outside == 0 and all(int(res.stage[i]) == 0 for i in C.WRONG)
