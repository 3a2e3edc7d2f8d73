"""tests/loss_edge_cases.py on the CPU: the inputs and references tests/test_gpu_loss_edges.py feeds ee_loss.hip are proved here, before
they reach a GPU.  For every FINITE case and every (B, K): the float64 reference is finite, the fp32 C oracle (the sibling under the bar)
is finite on the same input and meets the bar with itself as "got" - the bar is attainable by fp32 arithmetic on these inputs - and its
top-k equals the reference order.  For every POISON case the oracle's NaN pattern is the float64 reference's.

Dropped from the table: only the oracle's top-k on the `nan` case (loss_edge_cases.NO_TOPK_SIBLING).  orc_topk_i64 picks with `z[c] >
z[best]`, which is false for a NaN on either side: a NaN stays wherever the scan meets it, while ee_rows.hpp (and torch.topk) put it
first.  The reference order itself is checked against torch.topk on that case below; every finite case stays."""
import numpy as np
import pytest
import torch

import loss_edge_cases as E

SHAPES = [(B, K) for B in E.BS for K in E.KS]


def _finite(*ts):
    return all(bool(torch.isfinite(torch.as_tensor(t)).all()) for t in ts)


@pytest.mark.parametrize("case", E.FINITE)
def test_finite_cases_reference_and_oracle(case):
    for B, K in SHAPES:
        tag = "%s B=%d K=%d" % (case, B, K)
        z, zp, y = E.logits(case, B, K), E.logits(case, B, K, side=1), E.labels(B, K)
        assert z.dtype == torch.float32 and _finite(z, zp), tag
        for reduction, smoothing in (("sum", 0.0), ("mean", 0.0), ("mean", E.SMOOTHING)):
            if smoothing and K < 2:
                continue
            loss, grad, _ = E.ce_ref(z, y, reduction, smoothing)
            s_loss, s_grad = E.sib_ce(z, y, reduction, smoothing)
            assert _finite(loss, grad, s_loss, s_grad), tag
            E.within_bar(s_loss, s_loss, loss, "ce-loss " + tag)
            E.within_bar(s_grad, s_grad, grad, "ce-grad " + tag)
        ref, sib = E.kl_ref(z, zp)[:3], E.sib_kl(z, zp)
        assert _finite(*ref) and _finite(*sib), tag
        for r, s in zip(ref, sib):
            E.within_bar(s, s, r, "kl " + tag)
        if K >= 2:
            t = E.soft_targets(B, K)
            assert bool((t[0] == 0).any()) and bool(((t.sum(1) - 1).abs() < 1e-12).all())
            ref, sib = E.softce_ref(z, t, 1.0 / B)[:2], E.sib_softce(z, t, 1.0 / B)
            assert _finite(*ref) and _finite(*sib), tag
            for r, s in zip(ref, sib):
                E.within_bar(s, s, r, "softce " + tag)
        for k in sorted({min(5, K)} | ({16} if K >= 16 else set())):
            idx, correct = E.topk_ref(z, y, k)
            s_idx, s_correct = E.sib_topk(z, y, k)
            assert np.array_equal(idx, s_idx) and np.array_equal(correct, s_correct), tag
            # the restated order picks torch's values (the indices may differ where two values tie: fp32 is coarse at `offset`)
            assert torch.equal(z.gather(1, torch.from_numpy(idx)), torch.topk(z, k, 1).values), tag


def test_cases_are_what_their_names_say():
    B, K = 5, 129
    lp = E.ce_ref(E.logits("wide", B, K), E.labels(B, K))[2]
    assert float((lp < E.UNDERFLOW_LOGP).float().mean()) > 0.5      # most classes underflow
    z = E.logits("offset", B, K)
    assert float(z.min()) > 9e3 and not _finite(torch.exp(z))        # finite only through the max subtraction
    z = E.logits("constant", B, K)
    assert bool((z == z[:, :1]).all()) and len(set(z[:, 0].tolist())) == B
    z = E.logits("dominant", B, K)
    top2 = torch.topk(z, 2, 1).values
    assert bool((top2[:, 0] - top2[:, 1] >= 199.99).all())
    lp = E.ce_ref(z, E.labels(B, K))[2]
    assert int((lp < E.UNDERFLOW_LOGP).sum()) == B * (K - 1)
    z = E.logits("two_tied_max", B, K)
    assert bool(((z == z.max(1, keepdim=True).values).sum(1) == 2).all())
    for kind in E.POISON:
        zt, (zk, row) = E.logits("tame", B, K), E.poisoned(kind, B, K)
        clean = [b for b in range(B) if b != row]
        assert torch.equal(zk[clean], zt[clean]) and not _finite(zk[row])
        assert int((~torch.isfinite(zk[row])).sum()) == (K if kind == "all_neg_inf" else 1)


@pytest.mark.parametrize("kind", E.POISON)
def test_poisoned_rows_nan_pattern_of_the_oracle_is_the_references(kind):
    for B, K in SHAPES:
        tag = "%s B=%d K=%d" % (kind, B, K)
        (z, row), zt, y = E.poisoned(kind, B, K), E.logits("tame", B, K, side=1), E.labels(B, K)
        pairs = [(E.ce_ref(z, y, "sum")[1], E.sib_ce(z, y, "sum")[1])]
        if K >= 2:
            pairs.append((E.ce_ref(z, y, "mean", E.SMOOTHING)[1], E.sib_ce(z, y, "mean", E.SMOOTHING)[1]))
            t = E.soft_targets(B, K)
            pairs.append((E.softce_ref(z, t, 1.0 / B)[1], E.sib_softce(z, t, 1.0 / B)[1]))
        for a, b in ((z, zt), (zt, z)):  # the poisoned row as the model's output, and as the target distribution
            ref, sib = E.kl_ref(a, b), E.sib_kl(a, b)
            pairs += [(ref[1], sib[1]), (ref[2], sib[2])]
        for i, (ref, sib) in enumerate(pairs):
            assert torch.equal(torch.isnan(ref), torch.isnan(sib)), "%s output %d" % (tag, i)
            clean = [b for b in range(B) if b != row]
            assert _finite(ref[clean], sib[clean]), tag
        k = min(5, K)
        idx, correct = E.topk_ref(z, y, k)
        got, want = z.gather(1, torch.from_numpy(idx)).numpy(), torch.topk(z, k, 1).values.numpy()  # torch.topk: NaN above everything
        assert np.array_equal(got, want, equal_nan=True), tag
        if kind not in E.NO_TOPK_SIBLING:
            s_idx, s_correct = E.sib_topk(z, y, k)
            assert np.array_equal(idx, s_idx) and np.array_equal(correct, s_correct), tag


def test_the_oracle_top_k_does_not_order_a_nan():
    """why NO_TOPK_SIBLING holds the `nan` case: the first pick of the oracle skips the NaN"""
    (z, row), y = E.poisoned("nan", 5, 65), E.labels(5, 65)
    assert E.topk_ref(z, y, 1)[0][row, 0] == (2 * 65) // 3
    assert E.sib_topk(z, y, 1)[0][row, 0] != (2 * 65) // 3


def test_topk_reference_order():
    z = torch.tensor([[0.0, 1.0, 1.0, float("nan"), -float("inf"), float("inf")], [2.0, 2.0, 2.0, 2.0, 2.0, 2.0]])
    idx, correct = E.topk_ref(z, torch.tensor([1, 3]), 4)
    assert idx.tolist() == [[3, 5, 1, 2], [0, 1, 2, 3]]
    assert correct.tolist() == [0, 0, 1, 2]


@pytest.mark.parametrize("kind", E.MSE_KINDS)
def test_mse_inputs(kind):
    for n in E.MSE_NS:
        a, b = E.mse_inputs(kind, n)
        ref, sib = E.mse_ref(a, b), E.sib_mse(a, b)
        assert _finite(*ref) and _finite(*sib), (kind, n)
        for r, s in zip(ref, sib):
            E.within_bar(s, s, r, "mse %s n=%d" % (kind, n))
        d = a.double() - b.double()
        if kind == "const":
            assert bool((d == float(np.float32(1e-3))).all())
        if kind == "big" and n > 255:
            assert 4e3 < float(d.abs().max()) <= 1e4
