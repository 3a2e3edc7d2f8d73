"""CPU: the feature-denoising ResNets (resnet*_fd).  The float64 restatement of the product (tests/fd_reference.py) against itself and
autograd, ops.fd_fwd / ops.fd_bwd on host tensors against it, models.Denoising and the state_dict layout against fixtures written by the
reference's own resnet_fd.py (scripts/gen_fd_golden.py), the ABI's argument checks, and experiments_imagenet.py --no-cuda on resnet18_fd."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fake_imagenet as FI
import fd_reference as R

PKG = FI.PKG
SHAPES = [(2, 8, 15), (2, 32, 15), (1, 16, 16), (2, 64, 3), (1, 64, 1)]  # channel, spatial, the tie, spatial with a tiny P, P = 1


@pytest.mark.parametrize("shape", SHAPES)
def test_restated_associations_agree_and_gradients_equal_autograd(shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    d = torch.randn(shape, generator=g, dtype=torch.float64)
    s = 1.0 / shape[2]
    fc, fs = R.fwd_channel(x, s), R.fwd_spatial(x, s)
    assert (fc - fs).abs().max() <= 1e-13 * R.fwd_bound(x).max() * s
    for f in (R.fwd_channel, R.fwd_spatial):
        xi = x.clone().requires_grad_(True)
        (ga,) = torch.autograd.grad(f(xi, s), xi, d)
        for b in (R.bwd_channel, R.bwd_spatial):
            assert (b(x, d, s) - ga).abs().max() <= 1e-13 * R.bwd_bound(x, d).max() * s
    # exact on integer data: every sum is an integer far below 2^53
    xi_, di_ = R.integer_case(*shape, seed=3)
    assert torch.equal(R.fwd_channel(xi_, 1.0), R.fwd_spatial(xi_, 1.0))
    assert torch.equal(R.bwd_channel(xi_, di_, 1.0), R.bwd_spatial(xi_, di_, 1.0))
    xa = xi_.double().requires_grad_(True)
    (ga,) = torch.autograd.grad(R.fwd_channel(xa, 1.0), xa, di_.double())
    assert torch.equal(R.bwd_channel(xi_, di_, 1.0), ga)


@pytest.mark.parametrize("shape", SHAPES + [(1, 320, 300)])
def test_ops_on_host_tensors_equal_the_restatement_exactly_on_integer_data(shape):
    from eeadv import ops
    x, d = R.integer_case(*shape, seed=11)
    s = R.scale_of(shape[2])
    assert R.fwd_bound(x).max() < 2 ** 24 and R.bwd_bound(x, d).max() < 2 ** 24  # every fp32 sum is exact, in any order
    f, gram = ops.fd_fwd(x, s)
    dm = min(shape[1], shape[2])
    assert f.dtype == torch.float32 and tuple(gram.shape) == (shape[0], dm, dm)
    assert torch.equal(f, (R.fwd(x, 1.0) * s).float())
    xd = x.double()
    assert torch.equal(gram.double(), torch.matmul(xd.transpose(1, 2), xd) if R.spatial(*shape[1:]) else torch.matmul(xd, xd.transpose(1, 2)))
    assert torch.equal(ops.fd_bwd(x, d, gram, s), (R.bwd(x, d, 1.0) * s).float())
    with pytest.raises(ValueError):
        ops.fd_bwd(x, d[:, :, :-1], gram, s) if shape[2] > 1 else ops.fd_bwd(x, d, gram[:, :0], s)


def test_supported_class_and_argument_checks_happen_before_any_launch():
    from eeadv import _native as N, ops
    L = N.lib
    for C, P in ((64, 3136), (128, 784), (256, 196), (512, 49), (256, 3136), (1024, 196), (2048, 49), (64, 35), (512, 1), (64, 64), (256, 257),
                 (2048, 4096 // 16), (64, 4096)):
        assert ops.fd_supported(C, P), (C, P)
    for C, P in ((320, 300), (512, 784), (32, 64), (96, 64), (2112, 4), (64, 4097), (64, 0), (0, 64)):
        assert not ops.fd_supported(C, P), (C, P)
    assert L.ee_fd_scratch_floats(2, 320, 300) == 0 and L.ee_fd_scratch_floats(0, 64, 64) == 0
    # one split: the partial tile and the backward's symmetrised sum; a long contraction is split (at most P / 64 ways)
    assert L.ee_fd_scratch_floats(2, 64, 64) == 2 * 64 * 64 * 2
    n = L.ee_fd_scratch_floats(32, 64, 3136)
    assert n % (32 * 64 * 64) == 0 and 2 < n // (32 * 64 * 64) <= 50
    q, off = ctypes.c_void_p(4096), ctypes.c_void_p(4098)
    assert L.ee_fd_fwd_f32(q, q, q, q, 2, 320, 300, 1.0, None) == -3 and L.ee_fd_bwd_f32(q, q, q, q, q, 2, 96, 64, 1.0, None) == -3
    assert L.ee_fd_fwd_f32(None, q, q, q, 2, 64, 64, 1.0, None) == -1 and L.ee_fd_bwd_f32(q, q, None, q, q, 2, 64, 64, 1.0, None) == -1
    assert L.ee_fd_fwd_f32(q, q, q, q, -1, 64, 64, 1.0, None) == -2 and L.ee_fd_fwd_f32(q, q, q, q, 2, 64, 64, float("nan"), None) == -2
    assert L.ee_fd_fwd_f32(q, off, q, q, 2, 64, 64, 1.0, None) == -4 and L.ee_fd_bwd_f32(q, q, q, off, q, 2, 64, 64, 1.0, None) == -4
    p2 = ctypes.c_void_p(8192)
    assert L.ee_fd_fwd_f32(q, q, p2, p2, 2, 64, 64, 1.0, None) == -2 and L.ee_fd_bwd_f32(q, p2, p2, q, p2, 2, 64, 64, 1.0, None) == -2  # in place
    assert L.ee_fd_fwd_f32(None, None, None, None, 0, 64, 64, 1.0, None) == 0  # an empty batch launches nothing


@pytest.mark.parametrize("tag", ["channel", "spatial"])
def test_denoising_matches_the_reference_block_in_float64(golden, tag):
    from eeadv import models
    z = golden("fd_denoise")
    n_in, H, W = (int(v) for v in z[tag + "_dims"])
    blk = models.Denoising(n_in, H, W).double().train()
    assert (n_in > H * W) == (tag == "spatial")
    with torch.no_grad():
        for mod, name in ((blk.conv3.weight, "conv3_weight"), (blk.conv3.bias, "conv3_bias"), (blk.bn.weight, "bn_weight"), (blk.bn.bias, "bn_bias")):
            mod.copy_(torch.from_numpy(z["%s_%s" % (tag, name)]))
    x = torch.from_numpy(z[tag + "_x"]).requires_grad_(True)
    y = blk(x)
    (dx,) = torch.autograd.grad(y, x, torch.from_numpy(z[tag + "_dy"]))
    for got, want in ((y.detach(), z[tag + "_y"]), (dx, z[tag + "_dx"])):
        want = torch.from_numpy(want)
        assert (got - want).abs().max() <= 1e-12 * want.abs().max()


@pytest.mark.parametrize("depth", [18, 50])
def test_state_dict_layout_is_the_references(golden, depth):
    from eeadv import models
    z = golden("fd_keys")
    sd = models.make_resnet_fd(depth).state_dict()
    assert list(sd.keys()) == [str(k) for k in z["resnet%d_fd_keys" % depth]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in z["resnet%d_fd_shapes" % depth]]


def test_resnet_fd_blocks_follow_the_crop_and_segments_partition_the_model():
    from eeadv import models
    net = models.make_resnet_fd(18, size=64, num_classes=7)
    assert [(d.n_in, d.H, d.W) for d in (net.denoise1, net.denoise2, net.denoise3, net.denoise4)] == [(64, 16, 16), (128, 8, 8), (256, 4, 4), (512, 2, 2)]
    owned = [id(p) for seg in net.grad_segments() for p in seg]
    assert sorted(owned) == sorted(id(p) for p in net.parameters()) and len(set(owned)) == len(owned)
    net.avgpool = torch.nn.AvgPool2d(2, stride=1)
    net.train()  # batch statistics keep the four cubic blocks in range (a freshly initialised model overflows in eval mode, the reference's too)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        whole = net(x)
        piece = x
        for fn in net.segment_fns():
            piece = fn(piece)
    assert torch.isfinite(whole).all() and torch.equal(whole, piece) and whole.shape == (2, 7)
    with pytest.raises(ValueError):
        models.make_resnet_fd(18, size=100)


def test_imagenet_driver_trains_resnet18_fd_on_cpu(tmp_path):
    cfg = FI.small_config(tmp_path, num_classes=10, crop_size=64, resize_size=72)
    text = open(cfg).read()
    assert "arch: 'resnet18'\n" in text
    open(cfg, "w").write(text.replace("arch: 'resnet18'\n", "arch: 'resnet18_fd'\n"))
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, "experiments_imagenet.py", "-c", cfg, "--no-cuda", "--data", "synthetic:1:1", "--max-epochs", "1",
                        "--output-root", str(out)], cwd=os.path.join(PKG, "ImageNet"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    logs = [os.path.join(d, f) for d, _, fs in os.walk(str(out)) for f in fs if f == "log.txt"]
    assert len(logs) == 1
    lines = open(logs[0]).read().splitlines()
    assert lines[0].startswith("Epoch: [0][0/1]") and np.isfinite(float(lines[0].split("Loss ")[1].split(" ")[0]))
    assert any(l.startswith(" * Clean Prec@1") for l in lines) and lines[-1].startswith(" * Adv Prec@1")
    ckpts = [os.path.join(d, f) for d, _, fs in os.walk(str(out)) for f in fs if f.endswith("_0.pth")]
    assert len(ckpts) == 1
    sd = torch.load(ckpts[0], weights_only=True)["state_dict"]
    assert sd["denoise4.conv3.weight"].shape == (512, 512, 1, 1) and sd["denoise1.conv1.bias"].shape == (32,)
