"""Host: CIFAR-100 on the HIP path without a launch - the pickle reader, the numpy twin of ee_batch_aug_u8_f32 against PIL itself, the
augmenting loader's draws, the CIFAR PreActResNets against tests/golden/cifar_preact.npz (written by the reference's own
AWP/Cifar100/models_cifar100_awp/preactresnet.py, tests/golden/make_cifar_golden.py) and the driver's command line and names."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from fake_cifar import aug_draws, cifar_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")
CIFAR = os.path.join(PKG, "AWP", "Cifar100")
TINY = os.path.join(PKG, "AWP", "Tiny_imagenet")
for p in (TINY, CIFAR):
    if p not in sys.path:
        sys.path.insert(0, p)


@pytest.fixture()
def cache(tmp_path, monkeypatch):
    monkeypatch.setenv("EEADV_DATA_CACHE", str(tmp_path / "cache"))
    return tmp_path / "cache"


# ---- the reader ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subdir", ["cifar-100-python", ""])
def test_reader_round_trips_pixels_and_fine_labels(tmp_path, cache, subdir):
    from eeadv import data as D
    root = str(tmp_path / "c100")
    want = cifar_tree(root, subdir=subdir)
    assert D.recognised("cifar100", root) and not D.recognised("cifar100", str(tmp_path / "nope")) and not D.recognised("mnist", root)
    for split in ("train", "test"):
        for _ in range(2):  # decoded, then from the cache
            x, y = D.load_cifar100(root, split)
            assert x.dtype == np.uint8 and y.dtype == np.int64 and x.shape == want[split][0].shape
            assert np.array_equal(x, want[split][0]) and np.array_equal(y, want[split][1])
    assert sorted(f.split("-")[1] for f in os.listdir(cache)) == ["test", "train"]


def test_reader_errors_name_the_file(tmp_path, cache):
    import pickle
    from eeadv import data as D
    root = str(tmp_path / "c100")
    cifar_tree(root)
    test = os.path.join(root, "cifar-100-python", "test")
    os.remove(test)
    with pytest.raises(D.DataError, match="cifar-100-python/test does not exist"):
        D.load_cifar100(root, "test")
    assert not D.recognised("cifar100", root)
    with open(test, "wb") as f:
        pickle.dump({"data": np.zeros((3, 3072), np.uint8), "fine_labels": [1, 2]}, f)
    with pytest.raises(D.DataError, match="test holds 3 images and 2 fine labels"):
        D.load_cifar100(root, "test")
    with open(test, "wb") as f:
        pickle.dump({"data": np.zeros((2, 3072), np.uint8), "fine_labels": [1, 100]}, f)
    with pytest.raises(D.DataError, match="test: fine label 100"):
        D.load_cifar100(root, "test")
    with open(test, "wb") as f:
        pickle.dump({"data": np.zeros((2, 3000), np.uint8), "fine_labels": [1, 2]}, f)
    with pytest.raises(D.DataError, match=r"test: data is 2x3000, expected \[N,3072\]"):
        D.load_cifar100(root, "test")
    with open(test, "wb") as f:
        f.write(b"not a pickle")
    with pytest.raises(D.DataError, match="test is not a CIFAR-100 python pickle"):
        D.load_cifar100(root, "test")
    from eeadv import driver
    with pytest.raises(NotImplementedError, match="cifar100 directory"):
        driver.data_source(str(tmp_path / "nope"), {"data": "cifar100"})


# ---- host_batch_aug against PIL --------------------------------------------------------------------------------------------------
def pil_pipeline(img, top, left, flip, angle, pad):
    """RandomCrop(padding=pad) at (top, left) -> RandomHorizontalFlip -> RandomRotation's img.rotate(...), by PIL itself"""
    H, W, C = img.shape
    padded = np.zeros((H + 2 * pad, W + 2 * pad, C), dtype=np.uint8)
    padded[pad:pad + H, pad:pad + W] = img
    im = Image.fromarray(padded[..., 0] if C == 1 else padded)
    im = im.crop((left, top, left + W, top + H))
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    im = im.rotate(float(angle), resample=Image.NEAREST, expand=False, fillcolor=0)
    return np.array(im, dtype=np.uint8).reshape(H, W, C)


@pytest.mark.parametrize("C,H,W,pad,n", [(3, 32, 32, 4, 2400), (1, 9, 13, 3, 2400)])
def test_host_batch_aug_equals_the_pil_pipeline_on_every_pixel(C, H, W, pad, n):
    from eeadv import data as D
    rng = np.random.default_rng(C * 100 + W)
    images = rng.integers(0, 256, (12, H, W, C), dtype=np.uint8)
    images[0] = 255  # a full image: every fill pixel shows
    labels = torch.arange(100, 112)
    ids, offs, flip, angles = aug_draws(n, 12, pad, seed=H)
    assert {0.0, 15.0, -15.0, 1e-6, -1e-6} <= set(angles.tolist()) and set(flip.tolist()) == {0, 1}
    assert [0, 0] in offs.tolist() and [2 * pad, 2 * pad] in offs.tolist()
    coef = D.aug_coeffs(angles, H, W)
    assert coef.dtype == np.int32 and coef[0].tolist() == list(D.AUG_IDENTITY)
    x, y = D.host_batch_aug(torch.from_numpy(images), labels, torch.from_numpy(ids), offs, flip, coef, pad)
    assert x.shape == (n, C, H, W) and x.dtype == torch.float32 and x.is_contiguous() and torch.equal(y, labels[torch.from_numpy(ids)])
    for k in range(n):
        want = pil_pipeline(images[ids[k]], int(offs[k, 0]), int(offs[k, 1]), int(flip[k]), angles[k], pad)
        ref = torch.from_numpy(want).permute(2, 0, 1).float().div(255)  # ToTensor
        assert torch.equal(x[k], ref), (k, ids[k], offs[k].tolist(), int(flip[k]), angles[k])


def test_rotate_matrix_follows_pil_and_the_copy_shortcut():
    from eeadv import data as D
    assert D.rotate_matrix(0.0, 32, 32) is None and D.rotate_matrix(360.0, 32, 32) is None and D.rotate_matrix(-720.0, 9, 13) is None
    m = D.rotate_matrix(90.0, 13, 9)  # cos(-pi/2) rounds to 0 at 15 digits, as in PIL
    assert m[0] == 0.0 and m[1] == -1.0 and m[3] == 1.0 and m[4] == 0.0
    with pytest.raises(ValueError, match="crop offset"):
        D.host_batch_aug(torch.zeros(2, 4, 4, 1, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64), torch.tensor([0]), [[0, 3]], [0],
                         [D.AUG_IDENTITY], 1)
    with pytest.raises(ValueError, match="sample id"):
        D.host_batch_aug(torch.zeros(2, 4, 4, 1, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64), torch.tensor([2]), [[0, 0]], [0],
                         [D.AUG_IDENTITY], 1)


# ---- the loader ------------------------------------------------------------------------------------------------------------------
def test_loader_draws_are_seeded_per_epoch_and_in_range(tmp_path, cache):
    from eeadv import data as D
    root = str(tmp_path / "c100")
    want = cifar_tree(root, n_train=40, n_test=24)
    spec = {"shape": (3, 32, 32), "num_classes": 100}
    train, test = D.make_loaders("cifar100", root, spec, "cpu", 16, seed=3)
    train2, _ = D.make_loaders("cifar100", root, spec, "cpu", 16, seed=3)
    assert type(train) is D.AugDeviceLoader and type(test) is D.DeviceLoader and len(train) == 3 and len(test) == 2
    a, b = train.epoch_draws(), train2.epoch_draws()
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    train2.set_epoch(1)
    c = train2.epoch_draws()
    assert not any(torch.equal(s, t) for s, t in zip(a, c))
    train3, _ = D.make_loaders("cifar100", root, spec, "cpu", 16, seed=4)
    assert not any(torch.equal(s, t) for s, t in zip(a, train3.epoch_draws()))
    for ids, flip, offs, angles in (a, c):
        assert sorted(ids.tolist()) == list(range(40)) and flip.dtype == torch.bool and flip.shape == (40,)
        assert offs.dtype == torch.int32 and offs.shape == (40, 2) and int(offs.min()) >= 0 and int(offs.max()) <= 8
        assert angles.dtype == torch.float64 and float(angles.min()) >= -15.0 and float(angles.max()) <= 15.0
    # over many samples every offset and both signs of the angle are drawn
    big = D.AugDeviceLoader(lambda: (np.zeros((4000, 2, 2, 1), np.uint8), np.zeros(4000, np.int64)), 100, "cpu", seed=0, pad=4, rank=0, world=1)
    _, flip, offs, angles = big.epoch_draws()
    assert sorted(set(offs.reshape(-1).tolist())) == list(range(9)) and 0.4 < float(flip.float().mean()) < 0.6
    assert float(angles.min()) < -14.5 and float(angles.max()) > 14.5
    # a host epoch: each batch is host_batch_aug of the epoch's draws; the test split comes in file order, unchanged
    ids, flip, offs, angles = a
    batches = list(train)
    assert [x.shape[0] for x, _ in batches] == [16, 16, 8]
    coef = D.aug_coeffs(angles[ids].numpy(), 32, 32)
    x0, y0 = D.host_batch_aug(torch.from_numpy(want["train"][0]), torch.from_numpy(want["train"][1]), ids[:16], offs[ids][:16], flip[ids][:16],
                              coef[:16], 4)
    assert torch.equal(batches[0][0], x0) and torch.equal(batches[0][1], y0)
    assert torch.equal(torch.cat([x for x, _ in train]), torch.cat([x for x, _ in batches]))  # the same epoch again: the same draws
    tx = torch.cat([x for x, _ in test])
    assert torch.equal(tx, torch.from_numpy(want["test"][0]).permute(0, 3, 1, 2).float().div(255))
    assert torch.equal(torch.cat([y for _, y in test]), torch.from_numpy(want["test"][1]))
    with pytest.raises(ValueError, match="unknown dataset kind"):
        D.make_loaders("cifar10", root, spec, "cpu", 16, seed=3)


# ---- the models ------------------------------------------------------------------------------------------------------------------
def _seeded(golden):
    import models_cifar100_awp as Z
    torch.manual_seed(int(golden("cifar_preact")["seed"]))
    return Z.PreActResNet18(dataset="CIFAR100")


def sample(a, n):
    flat = np.asarray(a).reshape(-1)
    return flat[::-(-flat.size // n)]


def test_cifar_models_export_the_reference_names():
    import models_cifar100_awp as Z
    import models_cifar100_awp.preactresnet as P
    import models_tiny_awp as T
    for mod in (Z, P):
        for name in ("PreActResNet18", "PreActResNet34", "PreActResNet50", "PreActResNet101", "PreActResNet152"):
            assert callable(getattr(mod, name))
    assert callable(Z.AdvWeightPerturb) and Z.AdvWeightPerturb is T.AdvWeightPerturb
    m = Z.PreActResNet18()  # the reference's default: CIFAR10
    assert m.dataset == "CIFAR10" and m.linear.out_features == 10
    m = Z.PreActResNet50(dataset="CIFAR100")
    assert m.linear.in_features == 2048 and m.linear.out_features == 100 and "layer1.0.shortcut.0.weight" in m.state_dict()
    for bad in ("Tiny-ImageNet", "ImageNet"):
        with pytest.raises(NotImplementedError):
            Z.PreActResNet18(dataset=bad)
    with pytest.raises(NotImplementedError):  # the Tiny door keeps refusing the CIFAR datasets
        T.PreActResNet18(dataset="CIFAR100")
    with pytest.raises(NotImplementedError):
        T.PreActResNet18()


def test_cifar_state_dict_names_shapes_and_seeded_weights_match_the_reference(golden):
    G = golden("cifar_preact")
    sd = _seeded(golden).state_dict()
    assert list(sd.keys()) == list(G["names"])
    shapes = dict(zip(sd.keys(), [",".join(str(d) for d in v.shape) for v in sd.values()]))
    assert list(shapes.values()) == list(G["shapes"])
    assert shapes["linear.weight"] == "100,512" and shapes["conv1.weight"] == "64,3,3,3" and not [k for k in sd if k.startswith(("bn1.", "fc."))]
    assert np.array_equal(np.array([v.numpy().astype(np.float64).sum() for v in sd.values()]), G["checksum"])  # numpy: a fixed summation order


def test_cifar_cpu_logits_gradients_and_statistics_are_the_reference_bits(golden):
    """One CPU thread, the same torch ops in the same order as the reference's preactresnet.py: bit-identical, as for the Tiny zoo."""
    import torch.nn.functional as F
    from eeadv import runtime
    G = golden("cifar_preact")
    prev = torch.get_num_threads()
    torch.set_num_threads(1)
    runtime.allow_cpu_plumbing(True)
    try:
        net = _seeded(golden)
        x, y = torch.from_numpy(G["x"]), torch.from_numpy(G["y"])
        for mode in ("train", "eval"):
            net.train(mode == "train")
            net.zero_grad()
            xr = x.clone().requires_grad_(True)
            logits = net(xr)
            F.cross_entropy(logits, y).backward()
            assert np.array_equal(logits.detach().numpy(), G["logits_" + mode]), mode
            assert np.array_equal(xr.grad.numpy(), G["grad_x_" + mode]), mode
            named = dict(net.named_parameters())
            for k in G["params"]:
                assert np.array_equal(sample(named[str(k)].grad.numpy(), int(G["sample"])), G["g_%s_%s" % (mode, k)]), (mode, k)
            if mode == "train":
                sd = net.state_dict()
                assert np.array_equal(np.concatenate([sd[k].numpy().reshape(-1) for k in G["stat_names"]]), G["stats"])
                assert all(int(v) == 1 for k, v in sd.items() if k.endswith("num_batches_tracked"))
    finally:
        runtime.allow_cpu_plumbing(False)
        torch.set_num_threads(prev)


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def test_cifar_awp_driver_keeps_the_reference_command_line_and_names(tmp_path):
    """experiments_cifar100_awp.py:118-134 (every flag, its default), the output directory (:221-234) and checkpoint names (:249-268)."""
    from utils.helper import parse_config_file
    drv = importlib.import_module("experiments_cifar100_awp")
    cfg = os.path.join(CIFAR, "configs_cifar100_awp", "at_awp.yml")
    p = drv.make_parser()
    assert p.description == "PyTorch Cifar100 AWP Training"
    a = p.parse_args([])
    assert (a.config, a.pretrained, a.resume, a.evaluate, a.attack_method, a.no_cuda) == ("configs.yml", False, "", False, "PGD", False)
    a = p.parse_args(["-c", cfg, "--output-root", str(tmp_path), "--pretrained", "-e", "--resume", "x.pth", "--attack_method", "PGD", "--no-cuda",
                      "--data", "synthetic:1:1"])
    assert (a.pretrained, a.evaluate, a.resume, a.no_cuda, a.data) == (True, True, "x.pth", True, "synthetic:1:1")
    args = parse_config_file(a)
    assert (args.method_name, args.arch, args.batch_size, args.awp_gamma, args.awp_warmup, args.num_steps_1, args.num_steps_2, args.num_steps_3, args.l1,
            args.l2, args.epochs) == ("AT_AWP", "PreActResNet18", 128, 0.01, 0, 10, 20, 100, 0, 0, 200)
    assert abs(args.epsilon - 8 / 255) < 1e-12 and abs(args.step_size_1 - 2 / 255) < 1e-12
    d = drv.output_dirs(args)
    assert d["root"] == str(tmp_path) + "/checkpoint_Cifar100_AWP1/AT_AWP/PreActResNet18-bs128-lr0.1-momentum0.9-wd0.0002-seed0/"
    assert all(os.path.isdir(d[k]) for k in ("model", "best", "log"))
    f, best = drv.driver.checkpoint_names(args, d, 3)
    assert f == d["model"] + "at_numstep10_epsilon8_r0_canny_sigma0_alpha0-bs128-lr_0.1-w0-gfFalse-l0-h0_3.pth"
    assert best == d["best"] + "at_numstep10_epsilon8r0_canny_sigma0_alpha0-bs128-lr_0.1-w0-gfFalse-l0-h0.pth"
    args.arch = "WideResNet"
    with pytest.raises(NotImplementedError):
        drv.build_model(args)
    with pytest.raises(NotImplementedError):
        drv.main(["-c", cfg, "--attack_method", "AA", "--output-root", str(tmp_path)])
    with pytest.raises(NotImplementedError, match="cifar100 directory"):
        drv.main(["-c", cfg, "--data", str(tmp_path / "nope"), "--output-root", str(tmp_path)])
    opt = drv.make_optimizer(drv.build_model(parse_config_file(a)), type(args)(l2=0.01, lr=0.1, momentum=0.9, weight_decay=2e-4))
    assert [g["weight_decay"] for g in opt.param_groups] == [0.01, 0]


def test_cifar_awp_driver_runs_one_epoch_on_the_host(tmp_path):
    """--no-cuda --data synthetic:2:1, one epoch of AT_AWP in a child process (batch 4 and PGD-1 from a copy of the config: host speed)"""
    cfg = open(os.path.join(CIFAR, "configs_cifar100_awp", "at_awp.yml")).read()
    for k, v in (("batch_size", 4), ("num_steps_1", 1), ("num_steps_2", 1), ("print_freq", 1)):
        assert "\n%s: " % k in cfg
        cfg = "\n".join("%s: %s" % (k, v) if line.startswith(k + ": ") else line for line in cfg.split("\n"))
    path = tmp_path / "at_awp.yml"
    path.write_text(cfg)
    r = subprocess.run([sys.executable, os.path.join(CIFAR, "experiments_cifar100_awp.py"), "-c", str(path), "--no-cuda", "--data", "synthetic:2:1",
                        "--max-epochs", "1", "--output-root", str(tmp_path)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, OMP_NUM_THREADS="4"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "=> creating model 'PreActResNet18'" in r.stdout and "Epoch: [0][1/2]\t" in r.stdout and "Robust Loss " in r.stdout
    assert "Test_adv: [0/1]\t" in r.stdout and " * Adv Prec@1 " in r.stdout
    root = str(tmp_path) + "/checkpoint_Cifar100_AWP1/AT_AWP/PreActResNet18-bs4-lr0.1-momentum0.9-wd0.0002-seed0/"
    assert os.path.isfile(root + "log/log.txt")
    ckpts = os.listdir(root + "model_pth")
    assert len(ckpts) == 1 and ckpts[0].endswith("_0.pth")
    ck = torch.load(root + "model_pth/" + ckpts[0], map_location="cpu", weights_only=True)
    assert ck["epoch"] == 1 and "linear.weight" in ck["state_dict"] and "fc.weight" not in ck["state_dict"]
