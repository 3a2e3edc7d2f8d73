"""ee_loss.hip, ee_head.hip and ee_elementwise.hip's l2_step_kernel against float64 at their edges.

1. the row kernels (ee_ce_f32, ee_kl_f32, ee_softce_f64, ee_topk_i64) over every case x shape of tests/loss_edge_cases.py
2. row independence: a poisoned row (inf, NaN) changes no bit of another row, nor does the launch geometry
3. labels outside the row: NaN loss, zero gradient, never dereferenced
4. ee_mse_f32 and ee_reduce_rows_f64 at their chunk boundaries
5. the classifier head: every alignment and tail branch of ee_pool_linear_fwd_f32, both backward kernels
6. ee_l2_step_f32 against a float64 restatement of the TRADES L2 update

The bar of 1, 4 and 5 (loss_edge_cases.within_bar, the shape and constants of test_gpu_attack_route._twice_the_sibling): the kernel is no
further from the float64 reference than twice the sibling, plus 1e-7 of the reference's largest entry.  The sibling is fp32 arithmetic
on the host - the C oracle for the losses, fp32 torch on the CPU for the head - never a kernel of this library.  Every test prints, per
output, the case that came closest to its bar (kernel error, sibling error, largest reference entry)."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_edge_cases as E
from test_gpu_kernels import assert_bitexact

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from eeadv import ops as _ops
    return _ops


def same_bits(got, want, what):
    got, want = got.detach().cpu().numpy(), want.detach().cpu().numpy()
    if got.dtype == np.float64:  # assert_bitexact's float path is fp32's
        assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64)), what
    else:
        assert_bitexact(got, want, what)


# The cases that need more than the bar on the MI355X (11 of the 1700 comparisons of sections 1 and 4), each with the smallest margin, in
# steps of 0.5e-7, that holds; every other comparison keeps 1e-7.  Measured: kernel error / sibling error / largest reference entry.
#   kl-loss, kl-dp: the row's divergence is sum_k p_k (log p_k - log q_k) with sum_k p_k |log p_k - log q_k| of 6 ... 9 in these rows, p_k = expf(.)
#     and both log-sum-exps from logf(.): where the device's expf / logf differ from the host libm's (correctly rounded) ones by an ulp or two
#     the sum moves by a few 1e-7 of itself, and dp = p_k ((log p_k - log q_k) - KL) carries p_k times that.  The oracle runs the same fp32
#     expression tree on the host libm and happens to land within 1e-8 ... 5e-8 on the same rows.
#   ce-loss (constant, K=1000, B=5): every row is logf(1000.0f); the device's value is the fp32 number above the correctly rounded one (0.8 ulp
#     off, seen at B=3 and B=1 too), five equal rows add up to half an ulp of their sum, which the fp32 result then rounds to a whole one.
#   mse-grad (const, n=255): ee_mse_f32 is given gscale = float(2 / n) and multiplies - two roundings, at most 2^-23 = 1.19e-7 relative, where
#     the oracle's (2 d) / n has one; every element is the same number here, so the largest error is that of one draw.
FLOORS = {
    ("kl-loss", "(tame, K=128, B=5)"): 2e-7,            # 1.333e-06 / 9.766e-08 / 6.334
    ("kl-loss", "(offset, K=129, B=1)"): 3.5e-7,        # 2.784e-06 / 7.732e-08 / 8.549
    ("kl-dp", "(offset, K=129, B=1)"): 5.5e-7,          # 5.593e-07 / 6.358e-08 / 0.8389
    ("kl-loss", "(offset, K=1000, B=1)"): 1.5e-7,       # 1.241e-06 / 2.872e-07 / 5.621
    ("kl-dp", "(offset, K=1000, B=1)"): 5e-7,           # 2.054e-07 / 4.149e-08 / 0.2728
    ("kl-loss", "(two_tied_max, K=65, B=1)"): 1.5e-7,   # 1.017e-06 / 6.335e-08 / 8.596
    ("kl-dp", "(two_tied_max, K=65, B=1)"): 2e-7,       # 3.387e-07 / 8.182e-08 / 1.015
    ("kl-loss", "(two_tied_max, K=129, B=3)"): 1.5e-7,  # 1.110e-06 / 1.566e-07 / 7.933
    ("kl-dp", "(two_tied_max, K=64, B=5)"): 1.5e-7,     # 7.938e-08 / 2.127e-08 / 0.2608
    ("ce-loss[sum,hard]", "(constant, K=1000, B=5)"): 1.5e-7,  # 3.812e-06 / 2.794e-09 / 34.54
    ("mse-grad", "(const, n=255)"): 2.0 ** -23,         # 8.917e-13 / 1.783e-14 / 7.843e-06
}


def _ks(K):
    return sorted({min(5, K)} | ({16} if K >= 16 else set()))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the row kernels against float64
# ---------------------------------------------------------------------------------------------------------------------------------------
def _row_case(ops, case, B, K, bar):
    tag = "(%s, K=%d, B=%d)" % (case, K, B)
    z, zp, y = E.logits(case, B, K), E.logits(case, B, K, side=1), E.labels(B, K)
    zd, zpd, yd = z.to(DEV), zp.to(DEV), y.to(DEV)
    for reduction, smoothing in (("sum", 0.0), ("mean", 0.0), ("mean", E.SMOOTHING)):
        if smoothing and K < 2:
            continue
        name = "[%s,%s]" % (reduction, "smooth" if smoothing else "hard")
        loss, d = ops.ce(zd, yd, reduction, smoothing)
        r_loss, r_d, lp = E.ce_ref(z, y, reduction, smoothing)
        s_loss, s_d = E.sib_ce(z, y, reduction, smoothing)
        assert loss.dtype == torch.float32 and d.dtype == torch.float32
        bar.check(loss, s_loss, r_loss, "ce-loss" + name, tag)
        bar.check(d, s_d, r_d, "ce-grad" + name, tag)
        under = lp < E.UNDERFLOW_LOGP
        if case in ("wide", "dominant"):
            assert K < 63 or bool(under.any()), tag
        else:
            assert not bool(under.any()), tag
        if bool(under.any()):  # where the softmax underflows the gradient is (0 - target) * gscale, bit for bit
            gscale = torch.tensor(1.0 / B if reduction == "mean" else 1.0, dtype=torch.float32)
            want = (torch.zeros(B, K) - E.smooth_weights32(y, K, smoothing)) * gscale
            assert_bitexact(d.cpu()[under].numpy(), want[under].numpy(), "ce-grad of underflowed classes " + name + tag)
    loss, dq, dp = ops.kl_batchmean(zd, zpd, want_dp=True)
    r_loss, r_dq, r_dp, logp = E.kl_ref(z, zp)
    s_loss, s_dq, s_dp = E.sib_kl(z, zp)
    bar.check(loss, s_loss, r_loss, "kl-loss", tag)
    bar.check(dq, s_dq, r_dq, "kl-dq", tag)
    bar.check(dp, s_dp, r_dp, "kl-dp", tag)
    under = logp < E.UNDERFLOW_LOGP
    if bool(under.any()):
        assert bool((dp.cpu()[under] == 0).all()), "kl-dp of underflowed target classes " + tag
    if K >= 2:
        t, scale = E.soft_targets(B, K), 1.0 / B
        loss, dz = ops.softce(zd, t.to(DEV), scale)
        r_loss, r_dz, lp = E.softce_ref(z, t, scale)
        s_loss, s_dz = E.sib_softce(z, t, scale)
        assert loss.dtype == torch.float64 and dz.dtype == torch.float64
        bar.check(loss, s_loss, r_loss, "softce-loss", tag)
        bar.check(dz, s_dz, r_dz, "softce-grad", tag)
        under = lp < E.UNDERFLOW_LOGP
        if bool(under.any()):
            want = scale * (0.0 * t.sum(1, keepdim=True) - t)
            same_bits(dz.cpu()[under], want[under], "softce-grad of underflowed classes " + tag)
    for k in _ks(K):
        idx, correct = ops.topk(zd, yd, k)
        r_idx, r_correct = E.topk_ref(z, y, k)
        assert np.array_equal(idx.cpu().numpy(), r_idx), "top-%d indices %s" % (k, tag)
        assert np.array_equal(correct.cpu().numpy(), r_correct), "top-%d correct %s" % (k, tag)


@pytest.mark.parametrize("case", E.FINITE)
def test_row_kernels_against_float64(ops, case):
    """ops.ce (sum, mean, smoothing 0.1), ops.kl_batchmean(want_dp=True), ops.softce and ops.topk (k = min(5, K), and 16 at K >= 16) for
    K in {1, 2, 63, 64, 65, 128, 129, 1000} x B in {1, 3, 5, 9}: losses and gradients under the bar, top-k indices and `correct` equal to
    the reference order, and where the softmax underflows (`wide`, `dominant`) the gradient of an underflowed class is -target * gscale bit
    for bit, the KL dp there exactly 0.  FLOORS lists the ten comparisons here that need more than 1e-7 of the largest entry, and why.
    Measured on MI355X otherwise (kernel / sibling error): gradients 1e-8 ... 2.3e-7 / the same to 4x less; losses of `wide` and `dominant`
    equal the sibling's to every digit (5.1e-4 of 7984, 5.5e-5 of 1026); ce-loss at most 1.04e-6 of 11.45 against 8.7e-8."""
    bar = E.Bar(FLOORS)
    try:
        for B in E.BS:
            for K in E.KS:
                _row_case(ops, case, B, K, bar)
    finally:
        bar.finish()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. row independence
# ---------------------------------------------------------------------------------------------------------------------------------------
def _per_element(ops, z, y, t):
    """the per-element outputs that do not depend on the batch size (reduction 'sum', a fixed soft-CE scale)"""
    K = z.shape[1]
    zd, yd = z.to(DEV), y.to(DEV)
    out = {"ce-grad": ops.ce(zd, yd, "sum", want_loss=False)[1], "top-k": ops.topk(zd, yd, min(5, K))[0]}
    if K >= 2:
        out["ce-grad smooth"] = ops.ce(zd, yd, "sum", E.SMOOTHING, want_loss=False)[1]
        out["softce-grad"] = ops.softce(zd, t.to(DEV), 0.125, want_loss=False)[1]
    return {k: v.cpu() for k, v in out.items()}


def _per_element_ref(z, y, t):
    K = z.shape[1]
    out = {"ce-grad": E.ce_ref(z, y, "sum")[1], "top-k": torch.from_numpy(E.topk_ref(z, y, min(5, K))[0])}
    if K >= 2:
        out["ce-grad smooth"] = E.ce_ref(z, y, "sum", E.SMOOTHING)[1]
        out["softce-grad"] = E.softce_ref(z, t, 0.125)[1]
    return out


def _kl(ops, zq, zp):
    _, dq, dp = ops.kl_batchmean(zq.to(DEV), zp.to(DEV), want_loss=False, want_dp=True)
    return {"kl-dq": dq.cpu(), "kl-dp": dp.cpu()}


@pytest.mark.parametrize("kind", E.POISON)
def test_a_poisoned_row_stays_in_its_row(ops, kind):
    """One row of `tame` holds +inf, -inf, only -inf, or a NaN.  The NaN pattern of every per-element output is the float64 reference's
    (top-k: the reference order, NaN first), and every other row has the bits it has (a) in the same batch with the row not poisoned,
    (b) in the batch without that row (the rows after it move to other wavefronts and workgroups)."""
    for B in E.BS:
        for K in E.KS:
            tag = "(%s, K=%d, B=%d)" % (kind, K, B)
            (z, row), zt, z1, y, t = E.poisoned(kind, B, K), E.logits("tame", B, K), E.logits("tame", B, K, side=1), E.labels(B, K), E.soft_targets(B, K)
            clean = [b for b in range(B) if b != row]
            got, ref, tame = _per_element(ops, z, y, t), _per_element_ref(z, y, t), _per_element(ops, zt, y, t)
            for name, a, b in (("poisoned zq ", z, z1), ("poisoned zp ", z1, z)):
                r = E.kl_ref(a, b)
                for k, v in _kl(ops, a, b).items():
                    got[name + k], ref[name + k] = v, r[1] if k == "kl-dq" else r[2]
                for k, v in _kl(ops, zt if a is z else a, zt if b is z else b).items():
                    tame[name + k] = v
            for name in got:
                if name == "top-k":
                    assert torch.equal(got[name], ref[name]), "top-k " + tag
                else:
                    assert torch.equal(torch.isnan(got[name]), torch.isnan(ref[name])), "NaN pattern of %s %s" % (name, tag)
                    assert not bool(torch.isnan(got[name][clean]).any())
                same_bits(got[name][clean], tame[name][clean], "clean rows of %s next to the poisoned one %s" % (name, tag))
            if clean:
                less = _per_element(ops, z[clean].contiguous(), y[clean], t[clean].contiguous())
                for name in less:
                    same_bits(got[name][clean], less[name], "clean rows of %s without the poisoned one %s" % (name, tag))


@pytest.mark.parametrize("case", E.FINITE)
def test_a_row_alone_gives_the_rows_bits(ops, case):
    """ee_loss.hip: 'the result does not depend on launch geometry' - rows 0, 3, 4 and 8 of a batch of 9, each computed alone"""
    for K in E.KS:
        z, y, t = E.logits(case, 9, K), E.labels(9, K), E.soft_targets(9, K)
        nine = _per_element(ops, z, y, t)
        for b in (0, 3, 4, 8):
            one = _per_element(ops, z[b:b + 1].contiguous(), y[b:b + 1], t[b:b + 1].contiguous())
            for name in one:
                same_bits(nine[name][b:b + 1], one[name], "%s of row %d alone (%s, K=%d)" % (name, b, case, K))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. labels outside the row
# ---------------------------------------------------------------------------------------------------------------------------------------
BAD_ROWS, GOOD_ROWS = [0, 2, 4], [1, 3]


def _bad_labels(K):
    return (-1, K, 2 ** 32 + 1, -2 ** 40)  # the last two are classes 1 and 0 once truncated to 32 bits


@pytest.mark.parametrize("K", [3, 65])
def test_ce_and_topk_with_labels_outside_the_row(ops, K):
    """ee_ce_f32 with a label outside [0, K) in rows 0, 2 and 4 of 5: the scalar loss is NaN, those rows' gradient exactly zero, the other
    rows have the bits of the batch with valid labels; ee_topk_i64 counts no such label as correct."""
    z, y = E.logits("tame", 5, K), E.labels(5, K)
    zd = z.to(DEV)
    for bad in _bad_labels(K):
        yb = y.clone()
        yb[BAD_ROWS] = bad
        for smoothing in (0.0, E.SMOOTHING):
            for reduction in ("sum", "mean"):
                what = "label %d, K=%d, smoothing %g, %s" % (bad, K, smoothing, reduction)
                loss, d = ops.ce(zd, yb.to(DEV), reduction, smoothing)
                _, d_ok = ops.ce(zd, y.to(DEV), reduction, smoothing)
                assert math.isnan(loss.item()), what
                assert bool((d[BAD_ROWS] == 0).all()), what
                same_bits(d[GOOD_ROWS], d_ok[GOOD_ROWS], "rows with valid labels: " + what)
        k = min(5, K)
        idx, correct = ops.topk(zd, yb.to(DEV), k)
        idx_ok, _ = ops.topk(zd, y.to(DEV), k)
        assert torch.equal(idx, idx_ok)
        _, want = E.topk_ref(z[GOOD_ROWS], y[GOOD_ROWS], k)
        assert np.array_equal(correct.cpu().numpy(), want), "top-k correct with label %d, K=%d" % (bad, K)


@pytest.mark.parametrize("K", [3, 65])
def test_head_backward_with_labels_outside_the_row(ops, K):
    """ee_ce_pool_linear_bwd_f32: dfeat of an image with a label outside [0, K) is exactly zero, the other images have the bits of the
    batch with valid labels, and the whole batch still equals ops.ce followed by ops.pool_linear_bwd bit for bit."""
    g = torch.Generator().manual_seed(K)
    B, C, shape = 5, 300, (5, 300, 2, 2)
    z, y = E.logits("tame", B, K).to(DEV), E.labels(B, K)
    w = (torch.randn(K, C, generator=g) / C ** 0.5).to(DEV)
    for bad in _bad_labels(K):
        yb = y.clone()
        yb[BAD_ROWS] = bad
        for reduction in ("sum", "mean"):
            what = "label %d, K=%d, %s" % (bad, K, reduction)
            got = ops.ce_pool_linear_bwd(z, yb.to(DEV), w, shape, reduction)
            ok = ops.ce_pool_linear_bwd(z, y.to(DEV), w, shape, reduction)
            assert bool((got[BAD_ROWS] == 0).all()), what
            same_bits(got[GOOD_ROWS], ok[GOOD_ROWS], "images with valid labels: " + what)
            two = ops.pool_linear_bwd(ops.ce(z, yb.to(DEV), reduction, want_loss=False)[1], w, shape)
            same_bits(got, two, "one launch against two: " + what)


@pytest.mark.parametrize("K,Hd", [(10, 100), (33, 1500)], ids=["small-kernel", "general-kernel"])
def test_fc_ce_grad_with_labels_outside_the_row(ops, K, Hd):
    """ee_fc_ce_grad_f32, both kernels: dz1 of an image with a label outside [0, K) is exactly zero, the other images and every image's
    logits have the bits of the batch with valid labels."""
    g = torch.Generator().manual_seed(K + Hd)
    B = 5
    z1 = torch.randn(B, Hd, generator=g).to(DEV)
    w2, b2 = (torch.randn(K, Hd, generator=g) / Hd ** 0.5).to(DEV), torch.randn(K, generator=g).to(DEV)
    y = E.labels(B, K)
    for bad in _bad_labels(K):
        yb = y.clone()
        yb[BAD_ROWS] = bad
        for reduction in ("sum", "mean"):
            what = "label %d, K=%d, Hd=%d, %s" % (bad, K, Hd, reduction)
            got, lg = ops.fc_ce_grad(z1, w2, b2, yb.to(DEV), reduction, want_logits=True)
            ok, lg_ok = ops.fc_ce_grad(z1, w2, b2, y.to(DEV), reduction, want_logits=True)
            assert bool((got[BAD_ROWS] == 0).all()), what
            assert bool((ok[GOOD_ROWS] != 0).any())
            same_bits(got[GOOD_ROWS], ok[GOOD_ROWS], "images with valid labels: " + what)
            same_bits(lg, lg_ok, "logits: " + what)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. the mean-squared error and the row reduction
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", E.MSE_KINDS)
def test_mse_at_the_chunk_boundaries(ops, kind):
    """ops.mse at n in {1, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 5}: loss and gradient under the bar; `const` has a - b = 1e-3 at
    every element, `big` |a - b| up to 1e4."""
    bar = E.Bar(FLOORS)
    try:
        for n in E.MSE_NS:
            a, b = E.mse_inputs(kind, n)
            loss, da = ops.mse(a.to(DEV), b.to(DEV))
            (r_loss, r_da), (s_loss, s_da) = E.mse_ref(a, b), E.sib_mse(a, b)
            bar.check(loss, s_loss, r_loss, "mse-loss", "(%s, n=%d)" % (kind, n))
            bar.check(da, s_da, r_da, "mse-grad", "(%s, n=%d)" % (kind, n))
    finally:
        bar.finish()


def test_mse_writes_all_of_the_second_chunk_and_nothing_behind_it(ops):
    """n = 4097 through the C ABI into buffers with guards: da[4096] is written, nothing before da[0] or from da[n] on, two partials"""
    from eeadv import _native as N
    n, guard = 4097, -7.0
    a, b = (t.to(DEV) for t in E.mse_inputs("randn", n))
    _, want = ops.mse(a, b)
    buf = torch.full((n + 65,), guard, dtype=torch.float32, device=DEV)
    part = torch.full((2 + 2,), guard, dtype=torch.float64, device=DEV)
    da = buf[1:n + 1]  # one float into the buffer
    assert N.lib.ee_mse_num_partials(n) == 2
    N.check(N.lib.ee_mse_f32(ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()), n, 2.0 / n, ctypes.c_void_p(part[1:].data_ptr()),
                             ctypes.c_void_p(da.data_ptr()), ops._stream()), "ee_mse_f32")
    torch.cuda.synchronize()
    same_bits(da, want, "da")
    assert bool((da[4096:] != guard).all()) and float(buf[0]) == guard and bool((buf[n + 1:] == guard).all())
    assert float(part[0]) == guard and float(part[3]) == guard and bool((part[1:3] >= 0).all())
    d = a.double() - b.double()
    assert abs(float(part[1:3].sum()) - float((d * d).sum())) <= 1e-6 * float((d * d).sum())


def test_reduce_rows_is_a_fixed_order_float64_sum(ops):
    """ee_reduce_rows_f64 through ops._reduce_rows: within 1e-15 * n relative of math.fsum (float64 rounding of a sum of n terms in a fixed
    order: at most (n - 1) * 2^-53 of the sum of magnitudes), and the same bits from a second call."""
    for n in E.MSE_NS:
        g = torch.Generator().manual_seed(n)
        for name, rows in (("positive", (torch.rand(n, generator=g, dtype=torch.float64) + 0.5) * 10),
                           ("mixed signs", torch.randn(n, generator=g, dtype=torch.float64) * 1e3)):
            rd = rows.to(DEV)
            got, again = ops._reduce_rows(rd, 0.25), ops._reduce_rows(rd, 0.25)
            want, mag = 0.25 * math.fsum(rows.tolist()), 0.25 * math.fsum(rows.abs().tolist())
            err = abs(got.item() - want)
            print("    reduce_rows n=%5d %-12s |got - fsum| %.3e, allowed %.3e" % (n, name, err, 1e-15 * n * mag))
            assert err <= 1e-15 * n * mag, (n, name)
            same_bits(got, again, "two calls, n=%d" % n)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. the classifier head
# ---------------------------------------------------------------------------------------------------------------------------------------
HEAD_CK = [(C, 65) for C in (4096, 516, 300, 4)] + [(300, K) for K in (1, 15, 16, 17, 64, 129)]
MAPS = {1: (1, 1), 4: (2, 2), 6: (2, 3)}


def _one_float_in(t):
    """the same values as a contiguous view one float into a larger buffer: 4-byte aligned, not 16"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 and t.data_ptr() % 16 == 0
    return v


def _head_case(ops, B, C, HW, K, bar):
    tag = "(C=%d, K=%d, HW=%d, B=%d)" % (C, K, HW, B)
    g = torch.Generator().manual_seed(C + 7 * K + 31 * HW + B)
    feat = torch.randn(B, C, *MAPS[HW], generator=g)
    w, bias = torch.randn(K, C, generator=g) / C ** 0.5, torch.randn(K, generator=g)
    dl, y = torch.randn(B, K, generator=g), torch.randint(0, K, (B,), generator=g)

    def host(dtype):  # F.linear of the mean and its autograd; the cross-entropy gradient is taken at the fp32 logits `lg` below
        f = feat.to(dtype).requires_grad_(True)
        pooled = f.mean((2, 3))
        logits = F.linear(pooled, w.to(dtype), bias.to(dtype))
        return f, pooled, logits

    f64, pooled64, logits64 = host(torch.float64)
    f32, pooled32, logits32 = host(torch.float32)
    lg = logits32.detach().clone()
    bwd64 = torch.autograd.grad(logits64, f64, dl.double(), retain_graph=True)[0]
    bwd32 = torch.autograd.grad(logits32, f32, dl, retain_graph=True)[0]
    z64, z32 = lg.double().requires_grad_(True), lg.clone().requires_grad_(True)
    ce64 = torch.autograd.grad(logits64, f64, torch.autograd.grad(F.cross_entropy(z64, y, reduction="sum"), z64)[0])[0]
    ce32 = torch.autograd.grad(logits32, f32, torch.autograd.grad(F.cross_entropy(z32, y, reduction="sum"), z32)[0])[0]

    fd, wd, bd = feat.to(DEV), w.to(DEV), bias.to(DEV)
    logits, pooled = ops.pool_linear_fwd(fd, wd, bd)
    bar.check(pooled, pooled32.detach(), pooled64.detach(), "pooled", tag)
    bar.check(logits, logits32.detach(), logits64.detach(), "logits", tag)
    bar.check(ops.pool_linear_bwd(dl.to(DEV), wd, feat.shape), bwd32, bwd64, "dfeat", tag)
    bar.check(ops.ce_pool_linear_bwd(lg.to(DEV), y.to(DEV), wd, feat.shape, "sum"), ce32, ce64, "ce-dfeat", tag)
    if C % 4 == 0:  # the scalar path at a vec4 shape
        l_m, p_m = ops.pool_linear_fwd(fd, _one_float_in(wd), bd)
        same_bits(p_m, pooled, "pooled, weight one float in " + tag)
        bar.check(l_m, logits32.detach(), logits64.detach(), "logits-misaligned-weight", tag)
        top = float(logits.abs().max())
        assert float((l_m - logits).abs().max()) <= 1e-6 * top, "logits, weight one float in %s: %.3e of %.3e" % (tag, float((l_m - logits).abs().max()), top)
    if HW == 4:  # without the 16-byte load per channel: the same summation order
        l_f, p_f = ops.pool_linear_fwd(_one_float_in(fd), wd, bd)
        same_bits(p_f, pooled, "pooled, feat one float in " + tag)
        same_bits(l_f, logits, "logits, feat one float in " + tag)


@pytest.mark.parametrize("C,K", HEAD_CK)
def test_head_against_float64(ops, C, K):
    """ops.pool_linear_fwd (pooled, every row, and logits), ops.pool_linear_bwd and ops.ce_pool_linear_bwd for HW in {1, 4, 6} x B in {1, 3}
    against a float64 F.linear of the float64 mean and its autograd, the sibling fp32 torch on the CPU.  C = 300 (C / 4 = 75: a partly
    filled second 64-lane group), 516 (129: a second round of one lane), 4 and 4096 (the LDS limit); K around the 16 logits of a wavefront
    and the 64 of a workgroup.  With the weight one float into a buffer (the scalar path at a vec4 shape): the same bar, and within 1e-6 of
    the aligned call's largest logit; with feat one float into a buffer at HW == 4: the aligned call's bits.
    The weight at C = 4096, K = 65 is the largest tensor here, 1.06 MB."""
    bar = E.Bar(FLOORS)
    try:
        for HW in MAPS:
            for B in (1, 3):
                _head_case(ops, B, C, HW, K, bar)
    finally:
        bar.finish()


def test_head_limits(ops):
    """C = 4097 (the pooled row no longer fits the 16 KB of LDS) and K = 8193 (both backward entry points) are refused by the library"""
    from eeadv import _native as N
    with pytest.raises(N.EEError):
        ops.pool_linear_fwd(torch.zeros(1, 4097, 1, 1, device=DEV), torch.zeros(2, 4097, device=DEV), None)
    w = torch.zeros(8193, 4, device=DEV)
    with pytest.raises(N.EEError):
        ops.pool_linear_bwd(torch.zeros(1, 8193, device=DEV), w, (1, 4, 1, 1))
    with pytest.raises(N.EEError):
        ops.ce_pool_linear_bwd(torch.zeros(1, 8193, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV), w, (1, 4, 1, 1))
    logits, pooled = ops.pool_linear_fwd(torch.ones(1, 4096, 1, 1, device=DEV), torch.ones(2, 4096, device=DEV), None)  # the limit itself
    assert logits.tolist() == [[4096.0, 4096.0]] and bool((pooled == 1).all())


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. the TRADES L2 step
# ---------------------------------------------------------------------------------------------------------------------------------------
STEP, EPS = 0.05, 0.03  # tests/golden/linf_loops.npz: tradesl2_step_eps
L2_KINDS = ("ordinary", "zero_grad", "inside", "far", "clamp", "tiny_grad", "huge_grad", "nan_grad")
f32 = np.float32


def l2_step_ref(x, g, x0, step, eps, lo=0.0, hi=1.0):
    """attacks.py:389-400 on float64 arrays [B, per]: grad /= l2_norm(grad) + 1e-8 (l2_norm: the root of the MEAN of squares), the step,
    delta scaled onto the RMS ball only where delta_norm > eps, the clamp.  step and eps are the fp32 numbers the kernel is given."""
    step, eps = float(f32(step)), float(f32(eps))
    gn = np.sqrt((g * g).mean(1, keepdims=True)) + 1e-8
    d = (x + step * (g / gn)) - x0
    dn = np.sqrt((d * d).mean(1, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.where(dn > eps, d * (eps / dn), d)
    return np.clip(x0 + d, lo, hi)


def l2_step_fp32_no_shrink(x, g, x0, step, lo=0.0, hi=1.0):
    """one sample that stays inside the ball, as l2_step_kernel evaluates it: fp32 squares summed in float64 and rounded once, then
    clamp(x0 + ((x + step * (g / gn)) - x0)) - attacks.py:394-398 re-adds delta to x_natural, so this is clamp(x + step * g / gn) up to
    the roundings of that subtraction and addition"""
    gn = np.sqrt(f32(math.fsum((g * g).astype(np.float64).tolist()) / g.size)) + f32(1e-8)
    assert gn.dtype == np.float32
    return np.clip(x0 + ((x + f32(step) * (g / gn)) - x0), f32(lo), f32(hi))


def _l2_sample(kind, per, seed):
    rng = np.random.RandomState(seed)
    x0 = rng.uniform(0.2, 0.8, per).astype(f32)
    g = rng.randn(per).astype(f32)
    x = (x0 + f32(0.001) * rng.randn(per).astype(f32)).astype(f32)
    if kind == "zero_grad":  # multiples of 2^-12: x - x0 and x0 + (x - x0) are exact, RMS(x - x0) <= 2^-6 < eps
        x0 = (rng.randint(0, 4097, per) / 4096.0).astype(f32)
        x0[0], x0[-1] = 1.0, 0.0
        x = (x0 + rng.randint(-64, 65, per) / 4096.0).astype(f32)
        g[:] = 0.0
    elif kind == "inside":  # after the step delta is 0.4 * step * g / rms(g): RMS 0.02
        x = (x0 - 0.6 * STEP * g / np.sqrt((g.astype(np.float64) ** 2).mean())).astype(f32)
    elif kind == "far":
        x = (x0 + 0.5 * rng.randn(per)).astype(f32)
    elif kind == "clamp":
        x0 = rng.randint(0, 2, per).astype(f32)
        x = (x0 + f32(0.001) * rng.randn(per).astype(f32)).astype(f32)
    elif kind == "tiny_grad":
        g = (g * f32(1e-20)).astype(f32)
    elif kind == "huge_grad":
        g = (g * f32(1e15)).astype(f32)
    elif kind == "nan_grad":
        g[per // 2] = np.nan
    return x, g, x0


def _l2_run(ops, x, g, x0, step=STEP, eps=EPS):
    xd = torch.from_numpy(x).to(DEV)
    ops.l2_step_(xd, torch.from_numpy(g).to(DEV), torch.from_numpy(x0).to(DEV), step, eps, 0.0, 1.0)
    return xd.cpu().numpy()


@pytest.mark.parametrize("per", [1, 3, 1023, 1024, 1025, 12288])
def test_l2_step_against_float64(ops, per):
    """ops.l2_step_ (step 0.05, eps 0.03) on batches of 1 and 3 that mix the sample kinds: every finite sample within 5e-7 of the float64
    restatement (the tolerance of test_trades_pgd_l2_vs_reference) and inside the RMS ball (eps * (1 + 1e-5)); a zero gradient leaves
    clamp(x) bit for bit; a sample that stays inside the ball has the bits of the kernel's documented fp32 expression; a NaN gradient entry
    makes its sample NaN throughout, as torch's result is, and changes no bit of its neighbours."""
    worst = 0.0
    for B in (1, 3):
        for i in range(0, len(L2_KINDS), B):
            kinds = (L2_KINDS[i:i + B] + ("ordinary",) * B)[:B]
            x, g, x0 = (np.stack(a) for a in zip(*[_l2_sample(k, per, 1000 * per + 10 * i + j) for j, k in enumerate(kinds)]))
            got = _l2_run(ops, x, g, x0)
            ref = l2_step_ref(x.astype(np.float64), g.astype(np.float64), x0.astype(np.float64), STEP, EPS)
            for j, kind in enumerate(kinds):
                what = "%s (sample %d of %s, per_sample %d)" % (kind, j, kinds, per)
                if kind == "nan_grad":
                    assert np.isnan(ref[j]).all() and np.isnan(got[j]).all(), what
                    continue
                assert np.isfinite(got[j]).all(), what
                worst = max(worst, float(np.abs(got[j] - ref[j]).max()))
                np.testing.assert_allclose(got[j], ref[j], rtol=0, atol=5e-7, err_msg=what)
                rms = math.sqrt(float(((got[j].astype(np.float64) - x0[j]) ** 2).mean()))
                assert rms <= float(f32(EPS)) * (1 + 1e-5), (what, rms)
                if kind == "zero_grad":
                    assert ((x[j] < 0) | (x[j] > 1)).any() or per < 16
                    assert_bitexact(got[j], np.clip(x[j], f32(0), f32(1)), what)
                if kind in ("inside", "tiny_grad"):
                    assert_bitexact(got[j], l2_step_fp32_no_shrink(x[j], g[j], x0[j], STEP), what)
            if "nan_grad" in kinds and B > 1:
                j = kinds.index("nan_grad")
                g2 = g.copy()
                g2[j, per // 2] = 1.0
                got2 = _l2_run(ops, x, g2, x0)
                assert np.isfinite(got2).all()
                others = [k for k in range(B) if k != j]
                assert_bitexact(got[others], got2[others], "the neighbours of the NaN sample, per_sample %d" % per)
    print("\n    l2_step per_sample %5d: max |kernel - float64| %.3e (allowed 5e-7)" % (per, worst))


def test_l2_step_on_the_ball_and_with_an_empty_ball(ops):
    """dn == eps exactly (every |delta| = 2^-5 = eps, zero gradient): no shrink, x stays bit for bit.  eps = 0: every sample that moved
    returns clamp(x0); one that did not move (x == x0, zero gradient: dn == 0 is not > 0) stays clamp(x0) too and is not 0 / 0."""
    per, rng = 1025, np.random.RandomState(7)
    x0 = (rng.randint(1024, 3073, (3, per)) / 4096.0).astype(f32)
    x = (x0 + np.where(rng.rand(3, per) < 0.5, -1, 1) * 2.0 ** -5).astype(f32)
    assert_bitexact(_l2_run(ops, x, np.zeros_like(x), x0, eps=2.0 ** -5), x, "dn == eps")
    xa, ga, x0a = _l2_sample("ordinary", per, 1)
    xb, gb, x0b = _l2_sample("far", per, 2)
    x0b = rng.uniform(-0.1, 1.1, per).astype(f32)  # the clamp binds
    x0c = x0[0]
    x, g, x0 = np.stack([xa, xb, x0c]), np.stack([ga, gb, np.zeros(per, f32)]), np.stack([x0a, x0b, x0c])
    assert_bitexact(_l2_run(ops, x, g, x0, eps=0.0), np.clip(x0, f32(0), f32(1)), "eps = 0")


def test_l2_step_on_a_view_one_float_into_a_buffer(ops):
    B, per = 3, 1025
    x, g, x0 = (np.stack(a) for a in zip(*[_l2_sample(k, per, 50 + j) for j, k in enumerate(("ordinary", "far", "inside"))]))
    want = _l2_run(ops, x, g, x0)
    bufs = [torch.full((B * per + 3,), -7.0, dtype=torch.float32, device=DEV) for _ in range(3)]
    views = [b[1:B * per + 1].view(B, per) for b in bufs]
    for v, a in zip(views, (x, g, x0)):
        v.copy_(torch.from_numpy(a))
    assert views[0].data_ptr() % 16 == 4
    ops.l2_step_(views[0], views[1], views[2], STEP, EPS, 0.0, 1.0)
    assert_bitexact(views[0].cpu().numpy(), want, "unaligned view")
    for b in bufs:
        assert float(b[0]) == -7.0 and bool((b[B * per + 1:] == -7.0).all())
    assert_bitexact(views[1].cpu().numpy(), g, "g untouched")
