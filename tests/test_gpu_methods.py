"""GPU: the two full ensembles through trainer.attack_for_validation (the plans of eeadv.methods) against their members
called by hand through the real doors, in the same order from the same torch seed, and combined by the torch.where ladder written out here.
Every seed=None run takes its Philox ticket from torch's generator in call order, so the two sides draw the same bits and the comparison is
exact: a member out of order or a keyword lost on the way changes them."""
import pytest
import torch

from tiny_models import Args, TinyNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS, FAB_ITERS, QUERIES, K = 4, 2, 8, 10


def _by_hand(A, method, model, a, x, y):
    if method == "APGD+FAB+Square":
        return [A.APGD(model, a, x, y, STEPS, 'ce'), A.APGD_T(model, a, x, y, STEPS, K), A.FAB_T(model, a, x, y, K, FAB_ITERS)[:2],
                A.Square(model, a, x, y, QUERIES)[:2]]
    return [A.APGD_L1(model, a, x, y, STEPS, 'ce'), A.APGD_T_L1(model, a, x, y, STEPS, K), A.FAB_T_L1(model, a, x, y, K, FAB_ITERS)[:2],
            A.Square_L1(model, a, x, y, QUERIES)[:2]]


@pytest.mark.parametrize("method,eps", [("APGD+FAB+Square", 12 / 255), ("APGD-L1+FAB+Square", 4.0)], ids=["Linf", "L1"])
def test_an_ensemble_is_its_members_in_order(method, eps):
    import utils.attacks as A
    from eeadv import trainer
    model = TinyNet(3, 8, K, seed=0).to(DEV).eval()
    x = torch.rand(4, 3, 8, 8, generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad():
        y = model(x).argmax(1)
    a = Args(epsilon=eps, method_name="AT", attack_method=method, random=True, fab_iters=FAB_ITERS, square_queries=QUERIES)
    torch.manual_seed(17)
    got = trainer.attack_for_validation(model, a, x, y, DEV, STEPS, 0.1, K)
    torch.manual_seed(17)
    runs = _by_hand(A, method, model, a, x, y)
    x_adv, robust = runs[0]
    for xt, rt in runs[1:]:
        x_adv = torch.where((robust & ~rt).view(-1, 1, 1, 1), xt, x_adv)
        robust = robust & rt
    assert got.shape == x.shape and torch.equal(got, x_adv)
    # the radius is one at which the order matters: APGD-CE leaves samples standing that a later member fools, and the seed decides the points
    assert bool(runs[0][1].any()) and not torch.equal(x_adv, runs[0][0])
    torch.manual_seed(18)
    assert not torch.equal(trainer.attack_for_validation(model, a, x, y, DEV, STEPS, 0.1, K), got)
