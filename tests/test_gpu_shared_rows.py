"""What csrc/ee_rows.hpp and engine._cached promise: the kernels that share a logit-row expression give each other's bits, and the five
captured attack loops share one cache path (eager = graph, BatchNorm statistics shielded from the capture, no stale graph)."""
import gc

import pytest
import torch

import apgd_reference as R
from tiny_models import TinyBNNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from eeadv import ops
    return ops


# ---- shared CE arithmetic ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("K", [3, 64, 65, 200])  # 65: one class in the lane-stride tail
def test_apgd_ce_gradient_is_ee_ce_gradient(ops, B, K):
    g = torch.Generator().manual_seed(100 * B + K)
    z = (3 * torch.randn(B, K, generator=g)).to(DEV)
    y = torch.randint(0, K, (B,), generator=g).to(DEV)
    assert torch.equal(ops.apgd_loss(z, y, "ce")[1], ops.ce(z, y, "sum", 0.0, False, True)[1])


# ---- one order -----------------------------------------------------------------------------------------------------------------------
def test_topk_fab_and_apgd_share_one_order(ops, monkeypatch):
    B, K = 6, 130
    g = torch.Generator().manual_seed(5)
    z = 3 * torch.randn(B, K, generator=g)
    z[0] = torch.rand(K, generator=g) * 0.9  # the tie row [2, 5, 5, 5, 1, <1 ...]: the order begins 1, 2, 3, 0
    z[0, :5] = torch.tensor([2.0, 5.0, 5.0, 5.0, 1.0])
    z[1, 77] = float("nan")  # NaN on top
    y = torch.tensor([1, 77, 3, 4, 5, 6])
    y[2:] = z[2:].argmax(1)  # random rows, labelled with their prediction ...
    y[5] = (y[5] + 1) % K    # ... but one
    t = (y + 64) % K
    zd, yd, td = z.to(DEV), y.to(DEV), t.to(DEV)
    idx = ops.topk(zd, None, 4)[0].cpu()
    assert idx[0].tolist() == [1, 2, 3, 0] and idx[1, 0] == 77
    assert torch.equal(ops.fab_diff(zd, yd, td)[2].cpu().long(), idx[:, 0])
    for kind in ("ce", "dlr", "dlr_t"):
        loss, _, pred = ops.apgd_loss(zd, yd, kind, td)
        assert torch.equal(pred.cpu().bool(), idx[:, 0] == y), kind
        if kind == "ce":
            continue
        for b in range(B):  # the float64 row reference on topk's order
            monkeypatch.setattr(R, "order_row", lambda row, b=b: idx[b].tolist())
            want = R.row_loss(z[b].double(), y[b], kind, t[b])
            assert torch.allclose(loss[b].cpu().double(), want, rtol=1e-6, atol=0, equal_nan=True), (kind, b)  # test_loss_kernel's bound
    assert bool(torch.isnan(ops.apgd_loss(zd, yd, "dlr", td)[0][1]))


# ---- one cache path ------------------------------------------------------------------------------------------------------------------
EPS = 8 / 255


def _call(loop, model, use_graph):
    from eeadv import engine
    g = torch.Generator().manual_seed(11)
    x0 = torch.rand(4, 3, 8, 8, generator=g).to(DEV)
    x_init = torch.clamp(x0 + (torch.rand(4, 3, 8, 8, generator=g).to(DEV) * 2 - 1) * EPS, 0, 1)
    y = torch.randint(0, 10, (4,), generator=g).to(DEV)
    t = (y + 3) % 10
    if loop == "pgd":
        out = (engine.pgd_loop(model, x0, x_init, engine.LossSpec(engine.CE_SUM, y), 4, 2 / 255, EPS, use_graph=use_graph),)
    elif loop == "apgd":
        out = engine.apgd_loop(model, x0, x_init, y, 4, EPS, "ce", use_graph=use_graph)
    elif loop == "apgd_l1":
        out = engine.apgd_l1_loop(model, x0, x_init, y, 4, 1.0, "ce", use_graph=use_graph)
    elif loop == "square":
        out = engine.square_loop(model, x0, y, 5, EPS, seed=7, use_graph=use_graph)
    else:
        out = engine.fab_loop(model, x0, y, t, 4, EPS, use_graph=use_graph)
    return [o.clone() for o in out]


def _bn_state(model):
    return {k: v.clone() for k, v in model.state_dict().items() if "running_" in k or "num_batches" in k}


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("loop", ["pgd", "apgd", "apgd_l1", "square", "fab"])
def test_one_cache_path(loop):
    from eeadv import engine
    engine.clear_graphs()
    model = TinyBNNet(3, 8, 10, 3).to(DEV).train()
    init = {k: v.clone() for k, v in model.state_dict().items()}
    eager = _call(loop, model, False)
    bn_eager = _bn_state(model)
    assert int(bn_eager["bn.num_batches_tracked"]) > 0  # the loop's own train-mode forwards count
    for second in (False, True):
        model.load_state_dict(init)
        n = len(engine._GRAPHS)
        got = _call(loop, model, True)
        assert _same(got, eager), (loop, second)
        bn = _bn_state(model)  # the start point and the warm-up passes of the capture left no trace
        assert bn.keys() == bn_eager.keys() and all(torch.equal(bn[k], bn_eager[k]) for k in bn), (loop, second)
        assert len(engine._GRAPHS) == n + (0 if second else 1), (loop, second)
    del model
    gc.collect()
    fresh = TinyBNNet(3, 8, 10, 4).to(DEV).train()  # other weights; CPython may give it the old id
    init = {k: v.clone() for k, v in fresh.state_dict().items()}
    eager = _call(loop, fresh, False)
    fresh.load_state_dict(init)
    assert _same(_call(loop, fresh, True), eager), loop
    engine.clear_graphs()
