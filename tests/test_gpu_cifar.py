"""GPU: CIFAR-100 on the HIP path - ee_batch_aug_u8_f32 against its numpy twin eeadv.data.host_batch_aug (which tests/test_cifar_host.py
holds against PIL) bit for bit, its argument checks, the CIFAR PreActResNet18 against tests/golden/cifar_preact.npz and against
EEADV_STOCK_GLUE, the attack engine eager against graph replay, and one AWP step of the driver's core on a generated dataset."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from fake_cifar import aug_draws, cifar_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")
CIFAR = os.path.join(PKG, "AWP", "Cifar100")
TINY = os.path.join(PKG, "AWP", "Tiny_imagenet")
for p in (TINY, CIFAR):
    if p not in sys.path:
        sys.path.insert(0, p)
DEV = "cuda:0"
ALL_STOCK = "bn,pool,head,conv,stem,dense,conv3,preact"  # every piece models._STOCK names


# ---- the batch kernel ------------------------------------------------------------------------------------------------------------
def _aug_case(N, B, C, H, W, pad, seed):
    from eeadv import data as D
    g = torch.Generator().manual_seed(seed)
    images = torch.randint(0, 256, (N, H, W, C), generator=g, dtype=torch.uint8)
    images[0] = 255  # a full image: every fill pixel shows
    labels = torch.randint(0, 100, (N,), generator=g, dtype=torch.int64)
    ids, offs, flip, angles = aug_draws(B, N, pad, seed)
    coef = torch.from_numpy(D.aug_coeffs(angles, H, W))
    return images, labels, torch.from_numpy(ids), torch.from_numpy(offs), torch.from_numpy(flip), coef


def _device_aug(images, labels, ids, offs, flip, coef, pad):
    from eeadv import data as D, ops
    ids32 = ids.to(torch.int32)
    return ops.batch_aug(images.to(DEV), labels.to(DEV), ids32.to(DEV), offs.to(DEV), None if flip is None else flip.to(DEV), coef.to(DEV),
                         D.LUT.to(DEV), ids32, offs, pad)


@pytest.mark.gpu
@pytest.mark.parametrize("N,B,C,H,W,pad", [
    (10, 7, 3, 32, 32, 4),   # the reference case: the 16-byte stores
    (5, 3, 1, 9, 13, 3),     # odd, not square, W % 4 != 0: the scalar path
    (10, 1, 3, 32, 32, 4),
    (6, 300, 3, 32, 32, 4),  # more than one workgroup per (sample, channel) row group, repeats of few samples
    (4, 9, 2, 8, 12, 0),     # no padding: the crop is the image
])
def test_batch_aug_kernel_is_bit_identical_to_the_host_twin(N, B, C, H, W, pad):
    from eeadv import data as D
    images, labels, ids, offs, flip, coef = _aug_case(N, B, C, H, W, pad, seed=B * 7 + W)
    x, y = _device_aug(images, labels, ids, offs, flip, coef, pad)
    xr, yr = D.host_batch_aug(images, labels, ids, offs, flip, coef, pad)
    assert x.shape == (B, C, H, W) and x.is_contiguous() and x.dtype == torch.float32 and y.dtype == torch.int64
    assert torch.equal(x.cpu(), xr) and torch.equal(y.cpu(), yr)
    x2, _ = _device_aug(images, labels, ids, offs, None, coef, pad)  # flip = NULL: nobody is mirrored
    assert torch.equal(x2.cpu(), D.host_batch_aug(images, labels, ids, offs, torch.zeros_like(flip), coef, pad)[0])


def _abi_call(t, B, N=None, pad=4, idx_host=None, offs_host=None, null=None, shape=None):
    """ee_batch_aug_u8_f32 on the device tensors of `t` with one argument replaced"""
    from eeadv import _native as Nat
    p = {k: ctypes.c_void_p(v.data_ptr()) for k, v in t.items()}
    if null:
        p[null] = None
    n, H, W, C = t["data"].shape
    C, H, W = shape or (C, H, W)
    ih = t["idx_host"] if idx_host is None else idx_host
    oh = t["offs_host"] if offs_host is None else offs_host
    return Nat.lib.ee_batch_aug_u8_f32(p["data"], p["labels"], p["idx"], p["offs"], p["flip"], p["coef"], p["lut"],
                                       None if null == "idx_host" else ctypes.c_void_p(ih.data_ptr()),
                                       None if null == "offs_host" else ctypes.c_void_p(oh.data_ptr()),
                                       n if N is None else N, B, C, H, W, pad, p["out"], p["labels_out"], None)


@pytest.mark.gpu
def test_batch_aug_argument_checks_launch_nothing():
    """EE_ERR_NULL / EE_ERR_SHAPE before any launch: the output buffers keep their sentinel.  The out-of-range sample id and crop offset
    sit in the HOST copies the library checks; the device arrays the kernel would read stay in range throughout."""
    from eeadv import data as D
    images, labels, ids, offs, flip, coef = _aug_case(10, 7, 3, 32, 32, 4, seed=1)
    ids32 = ids.to(torch.int32)
    t = dict(data=images.to(DEV), labels=labels.to(DEV), idx=ids32.to(DEV), offs=offs.to(DEV), flip=flip.to(DEV), coef=coef.to(DEV),
             lut=D.LUT.to(DEV), out=torch.full((7, 3, 32, 32), -7.0, device=DEV), labels_out=torch.full((7,), -9, dtype=torch.int64, device=DEV))
    t_host = dict(idx_host=ids32, offs_host=offs)
    t.update(t_host)
    OK, NULL, SHAPE = 0, -1, -2
    assert _abi_call(t, 0) == OK  # B == 0: nothing to do
    for name in ("data", "labels", "idx", "offs", "coef", "lut", "out", "labels_out", "idx_host", "offs_host"):
        assert _abi_call(t, 7, null=name) == NULL, name
    assert _abi_call(t, -1) == SHAPE and _abi_call(t, 7, N=0) == SHAPE and _abi_call(t, 7, N=-5) == SHAPE and _abi_call(t, 7, pad=-1) == SHAPE
    assert _abi_call(t, 7, shape=(3, 0, 32)) == SHAPE and _abi_call(t, 7, shape=(3, 32, -32)) == SHAPE and _abi_call(t, 7, shape=(0, 32, 32)) == SHAPE
    for b, bad in ((0, 10), (6, 11), (3, -1)):  # a sample id >= N (or negative) at any batch position
        ih = ids32.clone()
        ih[b] = bad
        assert _abi_call(t, 7, idx_host=ih) == SHAPE, (b, bad)
    assert _abi_call(t, 7, N=int(ids32.max())) == SHAPE  # the same ids against a smaller split
    for b, col, bad in ((0, 0, 9), (6, 1, 9), (2, 1, -1), (4, 0, 1 << 20)):  # a crop offset beyond 2 pad = 8 (or negative)
        oh = offs.clone()
        oh[b, col] = bad
        assert _abi_call(t, 7, offs_host=oh) == SHAPE, (b, col, bad)
    assert _abi_call(t, 7, pad=int(offs.max()) // 2 - 1 if int(offs.max()) >= 2 else 0) == SHAPE  # the same offsets against a smaller pad
    torch.cuda.synchronize()
    assert bool((t["out"] == -7.0).all()) and bool((t["labels_out"] == -9).all())
    assert _abi_call(t, 7) == OK  # and the same arguments unreplaced do launch
    torch.cuda.synchronize()
    xr, yr = D.host_batch_aug(images, labels, ids, offs, flip, coef, 4)
    assert torch.equal(t["out"].cpu(), xr) and torch.equal(t["labels_out"].cpu(), yr)


@pytest.mark.gpu
def test_aug_loader_on_the_device_yields_the_host_loaders_batches(tmp_path, monkeypatch):
    from eeadv import data as D
    monkeypatch.setenv("EEADV_DATA_CACHE", str(tmp_path / "cache"))
    root = str(tmp_path / "c100")
    cifar_tree(root, n_train=40, n_test=24)
    spec = {"shape": (3, 32, 32), "num_classes": 100}
    for k in (0, 1):  # train (ee_batch_aug_u8_f32), test (ee_batch_u8_f32)
        dev, host = D.make_loaders("cifar100", root, spec, DEV, 16, seed=2)[k], D.make_loaders("cifar100", root, spec, "cpu", 16, seed=2)[k]
        for epoch in (0, 1):
            dev.set_epoch(epoch), host.set_epoch(epoch)
            n = 0
            for (x, y), (xh, yh) in zip(dev, host):
                assert x.is_cuda and y.is_cuda and torch.equal(x.cpu(), xh) and torch.equal(y.cpu(), yh)
                n += 1
            assert n == len(dev) == len(host)


# ---- the model -------------------------------------------------------------------------------------------------------------------
_MODEL_CHILD = r"""
import os, sys, numpy as np, torch, torch.nn.functional as F
sys.path[:0] = [%r, %r, %r]
import models_cifar100_awp as Z
from eeadv import models as M, preact as P
G = np.load(%r)
torch.manual_seed(int(G["seed"]))
net = Z.PreActResNet18(dataset="CIFAR100").cuda()
x, y = torch.from_numpy(G["x"]).cuda(), torch.from_numpy(G["y"]).cuda()
out = {}
for mode in ("train", "eval"):
    net.train(mode == "train")
    net.zero_grad()
    xi = x.clone().requires_grad_(True)
    logits = net(xi)
    F.cross_entropy(logits, y).backward()
    out[mode + "_logits"] = logits.detach().cpu().numpy()
    out[mode + "_gx"] = xi.grad.cpu().numpy()
    for k, p in net.named_parameters():
        out["%%s_g_%%s" %% (mode, k)] = p.grad.cpu().numpy()
    out[mode + "_routes"] = np.array(M.fallback_report(net)["layers"] + ["-"])
    out[mode + "_all_routes"] = np.array(["%%s:%%s" %% (n, m.__dict__["_ee_route"]) for n, m in net.named_modules() if "_ee_route" in m.__dict__])
    out[mode + "_boundaries"] = np.array(sorted("%%s:%%s" %% kv for kv in P.boundary_report(net).items()))
np.savez(sys.argv[1], **out)
"""


def _child(tmp_path, tag, env, code):
    path = str(tmp_path / (tag + ".npz"))
    r = subprocess.run([sys.executable, "-c", code, path], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(path)


@pytest.fixture(scope="module")
def model_runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cifar")
    code = _MODEL_CHILD % (os.path.dirname(__file__), PKG, CIFAR, os.path.join(ROOT, "tests", "golden", "cifar_preact.npz"))
    return _child(tmp, "default", {}, code), _child(tmp, "stock", {"EEADV_STOCK_GLUE": ALL_STOCK}, code)


def _rel(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / max(1e-30, np.abs(b).max()))


def _rel2(a, b):
    return float(np.linalg.norm((a.astype(np.float64) - b).ravel()) / max(1e-30, np.linalg.norm(b.ravel())))


def _sample(a, n):
    flat = np.asarray(a).reshape(-1)
    return flat[::-(-flat.size // n)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_cifar_model_on_the_device_matches_the_reference_fixture(model_runs, golden, mode):
    """The bars of tests/test_gpu_preact.py: logits within 1e-4 of the reference fixture's (test_seeded_model_on_the_device_matches_the_
    reference_fixture), gradients within 1e-2 in the relative 2-norm (test_fused_route_matches_a_float64_cpu_copy: a ReLU mask decided
    the other way moves a whole entry).  The fixture holds flat[::stride] of the larger parameter gradients; the same slice is taken here."""
    G = golden("cifar_preact")
    run = model_runs[0]
    err = float(np.abs(run[mode + "_logits"] - G["logits_" + mode]).max())
    print("%s: logits max abs error %.3g" % (mode, err))
    np.testing.assert_allclose(run[mode + "_logits"], G["logits_" + mode], rtol=0, atol=1e-4)
    e = _rel2(run[mode + "_gx"], G["grad_x_" + mode])
    print("%s: input gradient rel 2-norm error %.3g" % (mode, e))
    assert e < 1e-2, e
    for k in G["params"]:
        e = _rel2(_sample(run["%s_g_%s" % (mode, k)], int(G["sample"])), G["g_%s_%s" % (mode, k)])
        print("%s: d %s rel 2-norm error %.3g" % (mode, k, e))
        assert e < 1e-2, (k, e)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_cifar_default_route_matches_every_piece_stock(model_runs, mode):
    """Default route against EEADV_STOCK_GLUE=bn,pool,head,conv,stem,dense,conv3,preact in a fresh process, at the bars of
    test_fused_boundary_matches_the_stock_add_and_bn_act; and which layer took which route."""
    fused, stock = model_runs
    e = _rel(fused[mode + "_logits"], stock[mode + "_logits"])
    print("%s: logits %.3g" % (mode, e))
    assert e < 1e-4
    e = _rel(fused[mode + "_gx"], stock[mode + "_gx"])
    print("%s: gx %.3g" % (mode, e))
    assert e < 1e-3
    keys = [k for k in stock.files if k.startswith(mode + "_g_")]
    assert len(keys) == len([k for k in fused.files if k.startswith(mode + "_g_")]) > 40
    worst = max((_rel(fused[k], stock[k]), k) for k in keys)
    print("%s: worst parameter gradient %.3g at %s" % (mode, worst[0], worst[1]))
    for k in keys:
        assert _rel(fused[k], stock[k]) < 2e-3, k
    routes = dict(r.split(":", 1) for r in fused[mode + "_all_routes"])
    # the stem and layer1 (32x32 maps) and the stride-2 pair out of them are MIOpen's; every other 3x3 and both other shortcuts are csrc/'s
    vendor = sorted(k for k, how in routes.items() if how.startswith(("miopen", "tensile")))
    assert vendor == sorted(["conv1", "layer2.0.conv1", "layer2.0.shortcut.0"] + ["layer1.%d.conv%d" % (b, c) for b in (0, 1) for c in (1, 2)]), routes
    assert len(routes) == 20
    assert all(how.startswith("miopen") for how in dict(r.split(":", 1) for r in stock[mode + "_all_routes"]).values())
    b = dict(t.rsplit(":", 1) for t in fused[mode + "_boundaries"])
    assert sorted(b) == ["bn"] + ["layer%d.%d.bn1" % (i, j) for i in range(1, 5) for j in range(2) if (i, j) != (1, 0)]
    assert set(b.values()) == {"ee_bn.sum_act"}  # B = 4: even the 32x32 maps fit the register-cached kernel
    assert set(dict(t.rsplit(":", 1) for t in stock[mode + "_boundaries"]).values()) == {"add+bn_act"}


@pytest.mark.gpu
def test_cifar_boundaries_fall_back_where_the_kernel_refuses_the_shape():
    """B = 64 on 32x32 maps is beyond ee_bn_sum_act's register cache: layer1's boundary and layer2's first take add + bn_act, the rest fuse"""
    import models_cifar100_awp as Z
    from eeadv import ops, preact as P
    assert not ops.bn_sum_act_supported(torch.empty(64, 64, 32, 32, device="meta")) and ops.bn_sum_act_supported(torch.empty(64, 128, 16, 16, device="meta"))
    torch.manual_seed(0)
    net = Z.PreActResNet18(dataset="CIFAR100").to(DEV).eval()
    with torch.no_grad():
        out = net(torch.rand(64, 3, 32, 32, device=DEV))
    assert out.shape == (64, 100) and bool(torch.isfinite(out).all())
    b = P.boundary_report(net)
    assert {k for k, v in b.items() if v == "add+bn_act"} == {"layer1.1.bn1", "layer2.0.bn1"}


# ---- the attack engine -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_cifar_pgd_graph_replay_equals_eager_bit_for_bit(mode):
    import models_cifar100_awp as Z
    from eeadv import engine, ops
    torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = False, True
    engine.clear_graphs()
    torch.manual_seed(2)
    net = Z.PreActResNet18(dataset="CIFAR100").to(DEV).train(mode == "train")
    g = torch.Generator().manual_seed(5)
    x = torch.rand(8, 3, 32, 32, generator=g).to(DEV)
    y = torch.randint(0, 100, (8,), generator=g).to(DEV)
    noise = ((torch.rand(8, 3, 32, 32, generator=g) * 2 - 1) * 8 / 255).to(DEV)
    spec = engine.LossSpec(engine.CE_SUM, y)
    assert net.head_grad(net.body_pre(x).detach(), y, "sum") is not None  # AvgPool2d(4) on the 4x4 map: the fused head takes it
    eager = engine.pgd_loop(net, x, ops.pgd_init(x, noise), spec, 2, 2 / 255, 8 / 255, use_graph=False)
    graph = engine.pgd_loop(net, x, ops.pgd_init(x, noise), spec, 2, 2 / 255, 8 / 255, use_graph=True)
    again = engine.pgd_loop(net, x, ops.pgd_init(x, noise), spec, 2, 2 / 255, 8 / 255, use_graph=True)  # the cached graph
    engine.clear_graphs()
    print("%s: %d of %d pixels differ between eager and replay" % (mode, int((eager != graph).sum()), eager.numel()))
    assert torch.equal(graph, again)
    assert torch.equal(eager, graph)
    assert float((eager - x).abs().max()) > 1 / 255 and float((eager - x).abs().max()) <= 8 / 255 + 1e-6


# ---- one AWP step ----------------------------------------------------------------------------------------------------------------
def _awp_step(root):
    """the driver's core on the generated dataset: its loaders, models, optimiser and eeadv.trainer.awp_train_batch, from seed 0"""
    import importlib
    from eeadv import data as D, engine, trainer
    from tiny_models import Args
    drv = importlib.import_module("experiments_cifar100_awp")
    engine.clear_graphs()
    torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = False, True
    torch.manual_seed(0)
    args = Args(arch="PreActResNet18", method_name="AT_AWP", random=True, epsilon=8 / 255, num_steps_1=2, step_size_1=2 / 255, awp_warmup=0, awp_gamma=0.01,
                l1=0, l2=0, lr=0.1, momentum=0.9, weight_decay=2e-4, data=root, seed=0)
    net, proxy = drv.build_model(args).to(DEV), drv.build_model(args).to(DEV)
    opt = drv.make_optimizer(net, args)
    adv = drv.AdvWeightPerturb(model=net, proxy=proxy, proxy_optim=trainer.make_sgd(proxy.parameters(), lr=0.01), gamma=args.awp_gamma)
    train_loader, _ = drv.driver.make_loaders(args, drv.SPEC, torch.device(DEV), 8)
    assert type(train_loader) is D.AugDeviceLoader
    x, y = next(iter(train_loader))
    assert x.shape == (8, 3, 32, 32) and x.is_cuda
    seen = {}
    perturb, restore = adv.perturb, adv.restore

    def checked_perturb(diff):
        seen["before"] = {k: p.detach().clone() for k, p in net.named_parameters()}
        perturb(diff)
        seen["perturbed"] = max(float((p.detach() - (seen["before"][k] + args.awp_gamma * diff[k] if k in diff else seen["before"][k])).abs().max())
                                for k, p in net.named_parameters())

    def checked_restore(diff):
        stepped = {k: p.detach().clone() for k, p in net.named_parameters()}
        restore(diff)
        # after restore: the weights before perturb plus the optimiser's step (stepped - perturbed weights)
        seen["restored"] = max(float((p.detach() - (seen["before"][k] + (stepped[k] - (seen["before"][k] + args.awp_gamma * diff[k] if k in diff
                                                                                    else seen["before"][k])))).abs().max())
                               for k, p in net.named_parameters())
        seen["moved"] = max(float((p.detach() - seen["before"][k]).abs().max()) for k, p in net.named_parameters())
        seen["diff_keys"] = len(diff)
    adv.perturb, adv.restore = checked_perturb, checked_restore
    net.train()
    loss, logits = trainer.awp_train_batch(net, adv, trainer.make_criterion(args), opt, args, x, y, 0, torch.device(DEV))
    engine.clear_graphs()
    return loss.cpu(), logits.cpu(), torch.cat([p.detach().reshape(-1) for p in net.parameters()]).cpu(), seen, x.cpu()


@pytest.mark.gpu
def test_one_awp_step_through_the_driver_core_twice(tmp_path, monkeypatch):
    monkeypatch.setenv("EEADV_DATA_CACHE", str(tmp_path / "cache"))
    monkeypatch.setenv("EEADV_GRAPH", "1")
    root = str(tmp_path / "c100")
    cifar_tree(root, n_train=16, n_test=8)
    a, b = _awp_step(root), _awp_step(root)
    for loss, logits, w, seen, x in (a, b):
        assert bool(torch.isfinite(loss)) and 1.0 < float(loss) < 20.0 and bool(torch.isfinite(logits).all()) and bool(torch.isfinite(w).all())
        print("loss %.6f; perturb %.3g, restore %.3g, moved %.3g" % (float(loss), seen["perturbed"], seen["restored"], seen["moved"]))
        # fp32 rounding of (w + gamma d) + step - gamma d against w + step: the 1e-5 of test_three_awp_steps_match_the_eager_stock_route
        assert seen["perturbed"] < 1e-5 and seen["restored"] < 1e-5 and seen["moved"] > 1e-4 and seen["diff_keys"] == 21
    print("weights differing between the two runs: %d of %d" % (int((a[2] != b[2]).sum()), a[2].numel()))
    assert torch.equal(a[4], b[4])  # the same batch
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])  # the same step, bit for bit
