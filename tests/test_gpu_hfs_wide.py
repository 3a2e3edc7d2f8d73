"""GPU: the wide low-pass kernel ee_hfs_wide_f32 (csrc/ee_hfs_mfma.hip: planes past 256 x 256 up to 320 x 320, two 16-row bands
per wavefront, [P | Q] up to 64 columns) - the operator, its fused Add_Square modes and the ImageNet front end at the fast-AT
phase-3 shape (ImageNet/fgsm_imagenet/configs_ee: crop_size 288, r 18), with the bars of the band kernel's tests in test_gpu_chain.py.

Parity UNPINNED like the sibling (torch.rfft is gone): the float64 dense operator and the oracle's FFT restatement are the references.
A sequential-k float32 emulation of the chain is 0.9 - 1.2e-6 from float64 at these shapes on uniform inputs and the oracle's FFT form
2.6e-7, so 2e-6 / 3e-6 hold with margin."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (H, W, r, C): the required shape | 17 bands (the last wavefront owns one), one narrow strip | W past 256, W % 4 != 0, a partial last
# strip | odd sizes, NU = 37, NV = 19 | nu_pad 48 with nv_pad 32 off the square | the class limit
SHAPES = [(288, 288, 18, 3), (260, 40, 3, 1), (33, 262, 5, 2), (289, 291, 18, 1), (272, 304, 20, 1), (320, 320, 24, 1)]
B = 2


@pytest.fixture(scope="module")
def ops():
    from eeadv import ops as _ops
    return _ops


def _operator(H, W, r):
    from eeadv import hfs as HF
    op = HF.HFSOperator(H, W, r, DEV)
    assert op.wide is not None and op.kernel is None and op.mfma is None
    return op


def _check_operator(ops, x, op, H, W, r):
    from eeadv import hfs as HF
    from oracle import ref_path as R
    y = ops.hfs_wide(x, *op.wide)
    Ar, Ai, B1, B2 = HF.hfs_matrices(H, W, r)
    xd = x.cpu().double().numpy()
    want = np.einsum("hk,bckw->bchw", Ar, xd @ B1) + np.einsum("hk,bckw->bchw", Ai, xd @ B2)
    err = np.abs(y.cpu().numpy() - want).max()
    print("%dx%d r=%d: %.3g from the float64 operator" % (H, W, r, err))
    assert err < 2e-6
    np.testing.assert_allclose(y.cpu().numpy(), R.HighFreqSuppress(H, W, r)(x.cpu()).numpy(), atol=3e-6)
    assert torch.equal(y, ops.hfs_wide(x, *op.wide))  # the bands are added in band order: reproducible
    assert torch.equal(y, op.forward(x)) and torch.equal(y, op.adjoint(x))  # ... and this is where the operator routes
    u = torch.randn_like(x)
    lhs, rhs = float((y * u).sum()), float((x * ops.hfs_wide(u, *op.wide)).sum())
    assert abs(lhs - rhs) < 1e-3 * (abs(lhs) + 1)  # self-adjoint
    return y


@pytest.mark.parametrize("H,W,r,C", SHAPES)
def test_wide_lowpass_kernel_vs_float64_operator_UNPINNED(ops, H, W, r, C):
    torch.manual_seed(H * W + r)
    x = torch.rand(B, C, H, W, device=DEV)
    _check_operator(ops, x, _operator(H, W, r), H, W, r)


def test_wide_lowpass_kernel_on_a_view_one_float_off_alignment(ops):
    """The strips are then loaded and stored element-wise; the staged values, and so the bits, are those of the aligned call."""
    H, W, r, C = 288, 288, 18, 3
    torch.manual_seed(7)
    buf = torch.rand(B * C * H * W + 1, device=DEV)
    x = buf[1:].view(B, C, H, W)
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    op = _operator(H, W, r)
    y = _check_operator(ops, x, op, H, W, r)
    assert torch.equal(y, ops.hfs_wide(x.clone(), *op.wide))


@pytest.mark.parametrize("n,r,C", [(288, 18, 3), (260, 3, 1)])
def test_wide_lowpass_fused_add_square(ops, n, r, C):
    """sq_mode 1 / 2 of ee_hfs_wide_f32 against Add_Square (its own kernels, pinned to the reference) around the plain operator."""
    import utils.core as core
    torch.manual_seed(n)
    Bq, eps = 3, 16 / 255
    x = torch.rand(Bq, C, n, n, device=DEV)
    x[0, 0, 0, :4] = torch.tensor([0.0, 1.0, eps, 1 - eps], device=DEV)
    sq = core.Add_Square(C, n, eps, n_queries=1)
    d = sq.prepare(x)
    tab, nu_pad, nv_pad = _operator(n, n, r).wide
    xs = ops.add_square_fwd(x, eps, d["stripe"], d["sq_sign"], d["sq_pos"], d["sq_size"])
    fused = ops.hfs_wide(x, tab, nu_pad, nv_pad, 1, None, eps, d["stripe"], d["sq_sign"], d["sq_pos"], d["sq_size"])
    assert torch.equal(fused, ops.hfs_wide(xs, tab, nu_pad, nv_pad))  # same kernel, same staged values
    g = torch.randn_like(x)
    mask = ops.add_square_bwd(torch.ones_like(x), x, eps, d["stripe"], d["sq_sign"], d["sq_pos"], d["sq_size"])
    back = ops.hfs_wide(g, tab, nu_pad, nv_pad, 2, x, eps, d["stripe"], d["sq_sign"], d["sq_pos"], d["sq_size"])
    assert torch.equal(back, ops.hfs_wide(g, tab, nu_pad, nv_pad) * mask)


@pytest.fixture(scope="module")
def phase3():
    """resnet18_EE_square's front end at 288 / r = 18, the oracle's front end and one set of draws."""
    from eeadv import models
    from oracle import ref_path as R
    torch.manual_seed(5)
    m = models.make_resnet_ee(18, "imagenet", True, cize=288, r=18, w=1.0, with_gf=False, low=38.0, high=76.0, alpha=0.0, sigma=1.0,
                              type_canny="CannyFilter_step125_1", epsilon=16 / 255, n_queries=1).to(DEV).eval()
    x = torch.rand(2, 3, 288, 288)
    front = R.EEFront(288, 3, 18, 1.0, 38.0, 76.0, 0.0, 1.0, "CannyFilter_step125_1", False, True, 16 / 255, 1)
    draws = front.add_square.draw(2)
    ddev = {"stripe": draws["stripe"].to(DEV), "sq_pos": draws["sq_pos"].to(DEV), "sq_sign": draws["sq_sign"].reshape(1, 3).to(DEV)}
    return m, front, x, draws, ddev


def test_imagenet_ee_square_front_end_at_288_runs_on_the_wide_kernel(phase3, monkeypatch):
    """Forward and input gradient of the front end against the oracle's FFT restatement, one low-pass launch each way."""
    from eeadv import ops as _ops
    m, front, x, draws, ddev = phase3
    op = m.hfs.operator(torch.device(DEV))
    assert op.kernel is None and op.mfma is None and op.wide is not None and op.fused_square
    modes, real = [], _ops.hfs_wide
    monkeypatch.setattr(_ops, "hfs_wide", lambda x, t, nu, nv, sq_mode=0, *a: (modes.append(sq_mode), real(x, t, nu, nv, sq_mode, *a))[1])
    xr = x.clone().requires_grad_(True)
    want = front(xr, draws)
    xd = x.to(DEV).requires_grad_(True)
    got = m.front(xd, ddev)
    assert float(((got.detach().cpu() - want.detach()).abs() > 1e-5).float().mean()) == 0.0
    u = torch.randn_like(x)
    (want * u).sum().backward()
    (got * u.to(DEV)).sum().backward()
    assert modes == [1, 2]  # hfs(add_square(x)) in one launch, its backward in one
    g, gr = xd.grad.cpu().numpy(), xr.grad.numpy()
    assert np.array_equal(np.isnan(g), np.isnan(gr))
    fin = ~np.isnan(gr)
    assert np.abs(g[fin] - gr[fin]).max() < 2e-5 * np.abs(gr[fin]).max() + 1e-6


def test_manual_front_end_at_288_gives_the_bits_of_autograd_and_replays_from_a_graph(phase3):
    """front_manual / front_manual_backward (the attack loop's explicit chain) against autograd through `front`, then captured alone
    - no convolutions - in a graph: the replay equals the eager call bit for bit."""
    m, _, x, _, ddev = phase3
    torch.manual_seed(9)
    xdev = x.to(DEV)
    g_up = torch.randn(2, 3, 288, 288, device=DEV)
    xa = xdev.clone().requires_grad_(True)
    x_in = m.front(xa, ddev)
    x_in.backward(g_up)
    with torch.no_grad():
        x_in2, ctx = m.front_manual(xdev, ddev)
        g_lp, g_edge = m.front_manual_backward(g_up, ctx)
    assert torch.equal(x_in2, x_in.detach())
    assert np.array_equal((g_lp + g_edge).cpu().numpy(), xa.grad.cpu().numpy(), equal_nan=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        c_in, c_ctx = m.front_manual(xdev, ddev)
        c_lp, c_edge = m.front_manual_backward(g_up, c_ctx)
    for t in (c_in, c_lp, c_edge):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(c_in, x_in2) and torch.equal(c_lp, g_lp)
    assert np.array_equal(c_edge.cpu().numpy(), g_edge.cpu().numpy(), equal_nan=True)


def test_band_kernel_class_never_reaches_the_wide_kernel(ops, monkeypatch):
    from eeadv import hfs as HF
    import utils.core as core
    calls = []
    monkeypatch.setattr(ops, "hfs_wide", lambda *a, **k: calls.append(a) or pytest.fail("224 x 224 went to the wide kernel"))
    op = HF.HFSOperator(224, 224, 16, DEV)
    assert op.mfma is not None and op.wide is None
    torch.manual_seed(3)
    x = torch.rand(2, 3, 224, 224, device=DEV)
    d = core.Add_Square(3, 224, 16 / 255, n_queries=1).prepare(x)
    y = op.forward(x)
    assert torch.equal(y, ops.hfs_mfma(x, *op.mfma)) and torch.equal(op.adjoint(x), y)
    op.forward_square(x, 16 / 255, d)
    op.backward_square(y, x, 16 / 255, d)
    assert not calls
