"""GPU: ee_batch_u8_f32 against the host formula (bit for bit), under graph capture, DeviceLoader on the device against the
same loader on the host, and the Tiny-ImageNet driver training / evaluating on a generated dataset tree."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fake_datasets as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")
DEV = "cuda:0"


def _case(B, C, H, W, N, flip, seed):
    g = torch.Generator().manual_seed(seed)
    data = torch.randint(0, 256, (N, H, W, C), generator=g, dtype=torch.uint8)
    labels = torch.randint(0, 200, (N,), generator=g, dtype=torch.int64)
    idx = torch.randint(0, N, (B,), generator=g, dtype=torch.int32)  # arbitrary order, repeats
    f = (torch.rand(N, generator=g) < 0.5) if flip else None
    return data, labels, idx, f


def _device_batch(data, labels, idx, f):
    from eeadv import data as D, ops
    return ops.batch_u8(data.to(DEV), labels.to(DEV), idx.to(DEV), None if f is None else f.to(torch.uint8).to(DEV), D.LUT.to(DEV))


@pytest.mark.gpu
@pytest.mark.parametrize("B,C,H,W,N,flip", [
    (100, 3, 64, 64, 500, True),    # the headline shape
    (50, 1, 28, 28, 300, False),    # MNIST, flip = NULL
    (7, 3, 30, 30, 20, True),       # W % 4 != 0: the scalar path
    (1, 3, 64, 64, 3, True),
    (64, 3, 64, 64, 5, True),       # many repeats of few samples
    (33, 1, 28, 28, 40, True),
])
def test_batch_kernel_is_bit_identical_to_the_host_formula(B, C, H, W, N, flip):
    from eeadv import data as D
    data, labels, idx, f = _case(B, C, H, W, N, flip, seed=B * 131 + W)
    x, y = _device_batch(data, labels, idx, f)
    xr, yr = D.host_batch(data, labels, idx.long(), f)
    assert x.shape == (B, C, H, W) and x.is_contiguous()
    assert torch.equal(x.cpu(), xr) and torch.equal(y.cpu(), yr)
    # ToTensor's arithmetic, spelled out
    ref = data[idx.long()].permute(0, 3, 1, 2).float().div(255)
    if f is not None:
        ref = torch.where(f[idx.long()][:, None, None, None], ref.flip(-1), ref)
    assert torch.equal(x.cpu(), ref)


@pytest.mark.gpu
def test_batch_kernel_replays_from_a_captured_graph_with_new_ids():
    from eeadv import data as D, ops
    data, labels, idx, f = _case(100, 3, 64, 64, 400, True, seed=7)
    d_data, d_labels, d_flip, lut = data.to(DEV), labels.to(DEV), f.to(torch.uint8).to(DEV), D.LUT.to(DEV)
    ids = idx.to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.batch_u8(d_data, d_labels, ids, d_flip, lut)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        x, y = ops.batch_u8(d_data, d_labels, ids, d_flip, lut)
    new = torch.randperm(400, generator=torch.Generator().manual_seed(3))[:100].to(torch.int32)
    ids.copy_(new.to(DEV))
    g.replay()
    torch.cuda.synchronize()
    xe, ye = ops.batch_u8(d_data, d_labels, new.to(DEV), d_flip, lut)
    assert torch.equal(x, xe) and torch.equal(y, ye)
    xr, yr = D.host_batch(data, labels, new.long(), f)
    assert torch.equal(x.cpu(), xr) and torch.equal(y.cpu(), yr)


@pytest.mark.gpu
def test_device_loader_yields_the_host_loaders_batches(tmp_path, monkeypatch):
    from eeadv import data as D
    monkeypatch.setenv("EEADV_DATA_CACHE", str(tmp_path / "cache"))
    root = str(tmp_path / "tiny")
    _, n_train, _ = F.tiny_tree(root, n_classes=200, per_class=1, extra=5, n_val=20, ext=".JPEG")
    assert n_train % 16 != 0
    for split, shuffle, flip in (("train", True, True), ("val", False, False)):
        load = lambda: D.load_tiny_imagenet(root, split)
        dev = D.DeviceLoader(load, 16, DEV, seed=1, shuffle=shuffle, flip=flip, rank=0, world=1)
        host = D.DeviceLoader(load, 16, "cpu", seed=1, shuffle=shuffle, flip=flip, rank=0, world=1)
        assert len(dev) == len(host) == math.ceil((n_train if split == "train" else 20) / 16)
        for epoch in (0, 1):
            dev.set_epoch(epoch)
            host.set_epoch(epoch)
            nb = 0
            for (x, y), (xh, yh) in zip(dev, host):
                assert x.is_cuda and y.is_cuda and x.dtype == torch.float32 and y.dtype == torch.int64
                assert torch.equal(x.cpu(), xh) and torch.equal(y.cpu(), yh)
                nb += 1
            assert nb == len(dev)
        if split == "train":
            assert x.shape[0] == n_train % 16  # the partial last batch


def _tiny_cfg(tmp_path):
    base = open(os.path.join(PKG, "Tiny_ImageNet/configs_tinyimagenet/ee_at_bpda3_square.yml")).read()
    for a, b in (("batch_size: 100\n", "batch_size: 20\n"), ("num_steps_2: 50\n", "num_steps_2: 2\n"), ("num_steps_3: 100\n", "num_steps_3: 2\n")):
        assert a in base
        base = base.replace(a, b)
    cfg = tmp_path / "ee.yml"
    cfg.write_text(base)
    return str(cfg)


def _run(cfg, data, out, env, *extra):
    r = subprocess.run([sys.executable, "experiments_tinyimagenet.py", "-c", cfg, "--data", data, "--max-epochs", "1", "--output-root", out]
                       + list(extra), cwd=os.path.join(PKG, "Tiny_ImageNet"), capture_output=True, text=True, timeout=1200, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    logs = [os.path.join(d, f) for d, _, fs in os.walk(out) for f in fs if f == "log.txt"]
    assert len(logs) == 1
    return open(logs[0]).read().splitlines()


def _parse_like_read_log(line):
    parts = line.split(" ")  # utils/read_log.py: fields 4 and 6 of the summary lines
    return float(parts[4]), float(parts[6])


@pytest.mark.gpu
def test_tiny_driver_trains_and_evaluates_on_a_generated_tree(tmp_path):
    root = str(tmp_path / "tiny")
    _, n_train, _ = F.tiny_tree(root, n_classes=200, per_class=1, extra=10, n_val=50, ext=".JPEG")
    cfg = _tiny_cfg(tmp_path)
    env = dict(os.environ, EEADV_DATA_CACHE=str(tmp_path / "cache"))
    lines = _run(cfg, root, str(tmp_path / "out"), env)
    K = math.ceil(n_train / 20)
    assert lines[0].startswith("Epoch: [0][0/%d]\t" % K)
    loss = float(lines[0].split("Loss ")[1].split(" ")[0])
    assert math.isfinite(loss)
    clean = [l for l in lines if l.startswith(" * Clean")]
    adv = [l for l in lines if l.startswith(" * Adv")]
    assert len(clean) == len(adv) == 1
    for l in clean + adv:
        p1, p5 = _parse_like_read_log(l)
        assert 0.0 <= p1 <= p5 <= 100.0
    cached = sorted(f.split("-")[1] for f in os.listdir(str(tmp_path / "cache")))
    assert cached == ["train", "val"]
    # --evaluate decodes the val split only
    env = dict(os.environ, EEADV_DATA_CACHE=str(tmp_path / "cache_eval"))
    lines = _run(cfg, root, str(tmp_path / "out_eval"), env, "--evaluate")
    assert sum(l.startswith(" * Adv") for l in lines) == 3
    assert [f.split("-")[1] for f in os.listdir(str(tmp_path / "cache_eval"))] == ["val"]
