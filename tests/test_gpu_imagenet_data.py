"""GPU: ee_batch_rrc_u8_f32 (crop + PIL-BILINEAR resample + flip + u8 -> f32, one launch per batch) against the host restatement
bit for bit through ops.batch_rrc, its argument handling, RaggedDeviceLoader on the device against the same loader on the host,
and experiments_imagenet.py training on a generated ImageNet-style tree."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fake_imagenet as FI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")
DEV = "cuda:0"
BOX_KINDS = ["whole", "1x1", "row", "column", "corner"]


class Split:
    """A ragged split of `sources`, on the host and on the device."""

    def __init__(self, sources):
        self.images = [FI.source(H, W) for H, W in sources]
        pixels, offsets, sizes = FI.pack(self.images)
        n = len(sources)
        self.host = (torch.from_numpy(pixels), torch.from_numpy(offsets), torch.from_numpy(sizes), torch.arange(100, 100 + n))
        self.dev = None

    def on_device(self):
        if self.dev is None:
            self.dev = tuple(t.to(DEV) for t in self.host)
        return self.dev

    def kernel(self, idx, boxes, flip, S):
        from eeadv import data as D, ops
        pixels, offsets, sizes, labels = self.on_device()
        return ops.batch_rrc(pixels, offsets, sizes, labels, idx.to(DEV), boxes.to(DEV), None if flip is None else flip.to(DEV),
                             D.LUT.to(DEV), S)

    def both(self, idx, boxes, flip, S):
        """(kernel's batch, host restatement's batch)"""
        from eeadv import data as D
        return self.kernel(idx, boxes, flip, S), D.host_batch_rrc(*self.host, idx.long(), boxes, flip, S)


@pytest.fixture(scope="module")
def common():
    return Split(FI.SOURCES)


@pytest.fixture(scope="module")
def extreme():
    return Split(FI.EXTREME_SOURCES)


def _boxes(sources, kind):
    return torch.tensor([FI.boxes_of(H, W)[BOX_KINDS.index(kind)] for H, W in sources], dtype=torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("S", FI.SIDES)
@pytest.mark.parametrize("kind", BOX_KINDS)
def test_kernel_is_bit_identical_to_the_host_restatement(common, kind, S):
    """B = 7 over the 5 sources: reversed order, two repeated ids, every second sample mirrored.  9x11 -> S upscales (ksize 3),
    500x375 -> 24 downscales by 20 (ksize 43); S = 43 takes the scalar stores and a partial last group of 4 columns."""
    idx = torch.tensor([4, 3, 2, 1, 0, 2, 4], dtype=torch.int32)
    flip = torch.tensor([1, 0, 1, 0, 1], dtype=torch.uint8)
    (x, y), (xr, yr) = common.both(idx, _boxes(FI.SOURCES, kind), flip, S)
    assert x.shape == (7, 3, S, S) and x.is_contiguous() and x.dtype == torch.float32 and y.dtype == torch.int64
    assert torch.equal(y.cpu(), yr) and yr.tolist() == [104, 103, 102, 101, 100, 102, 104]
    assert torch.equal(x.cpu(), xr)
    assert torch.equal(x[2], x[5]) and torch.equal(x[0], x[6])


@pytest.mark.gpu
def test_kernel_matches_pil_at_the_headline_shape(common):
    """B = 2, S = 224 from the 500x375 source with RandomResizedCrop-sized boxes, no flips: ToTensor(resize(crop(img)))."""
    boxes = torch.tensor([[0, 0, 1, 1]] * 4 + [[37, 12, 353, 362]], dtype=torch.int32)
    idx = torch.tensor([4, 4], dtype=torch.int32)
    (x, y), (xr, _) = common.both(idx, boxes, None, 224)
    assert torch.equal(x.cpu(), xr) and y.tolist() == [104, 104]
    ref = FI.pil_crop_resize(common.images[4], (37, 12, 353, 362), 224)
    assert torch.equal(x[0].cpu(), torch.from_numpy(ref.copy()).permute(2, 0, 1).float().div(255))


@pytest.mark.gpu
@pytest.mark.parametrize("S", [24, 43])
def test_crops_that_outgrow_the_lds_stage(extreme, S):
    """1 x 4800 -> S: the column tables alone are larger than the stage, every output is formed directly from global memory.
    1600 x 16 -> S: a band's 16 result rows need more source rows than the stage holds and are done in several stages."""
    idx = torch.tensor([1, 0, 1], dtype=torch.int32)
    flip = torch.tensor([1, 0], dtype=torch.uint8)
    for kind in ("whole", "corner"):
        (x, y), (xr, yr) = extreme.both(idx, _boxes(FI.EXTREME_SOURCES, kind), flip, S)
        assert torch.equal(x.cpu(), xr) and torch.equal(y.cpu(), yr), kind


@pytest.mark.gpu
def test_bad_ids_and_boxes_give_nan_and_minus_one_and_leave_the_neighbours_exact(common):
    S = 24
    good = _boxes(FI.SOURCES, "corner")
    idx = torch.tensor([0, -1, 1, 5, 2, 3, 4], dtype=torch.int32)  # -1 and N = 5 are outside [0, N)
    x, y = common.kernel(idx, good, None, S)
    from eeadv import data as D, ops
    xr, _ = D.host_batch_rrc(*common.host, torch.tensor([0, 1, 2, 3, 4]), good, None, S)
    assert y.tolist() == [100, -1, 101, -1, 102, 103, 104]
    assert bool(torch.isnan(x[1]).all()) and bool(torch.isnan(x[3]).all())
    assert torch.equal(x[[0, 2, 4, 5, 6]].cpu(), xr)
    bad = good.clone()
    H, W = FI.SOURCES[1]
    bad[0] = torch.tensor([0, 0, 0, 5])           # h = 0
    bad[1] = torch.tensor([H - 3, 0, 4, W])       # one row below the image
    bad[2] = torch.tensor([0, -1, 4, 4])          # starts left of the image
    bad[3] = torch.tensor([0, 200, 10, 12])       # 300 x 211: leaves on the right
    x, y = common.kernel(torch.tensor([0, 1, 2, 3, 4], dtype=torch.int32), bad, None, S)
    assert y.tolist() == [-1, -1, -1, -1, 104]
    assert bool(torch.isnan(x[:4]).all()) and torch.equal(x[4].cpu(), xr[4])
    # an image that leaves the pixel buffer is not read either
    pixels, offsets, sizes, labels = common.on_device()
    off = offsets.clone()
    off[4] = pixels.numel() - 100
    x, y = ops.batch_rrc(pixels, off, sizes, labels, torch.tensor([3, 4], dtype=torch.int32, device=DEV), good.to(DEV), None, D.LUT.to(DEV), S)
    assert y.tolist() == [103, -1] and bool(torch.isnan(x[1]).all()) and torch.equal(x[0].cpu(), xr[3])


@pytest.mark.gpu
def test_empty_batch_cpu_tensors_and_misaligned_out_are_refused(common):
    from eeadv import _native as N, data as D, ops
    pixels, offsets, sizes, labels = common.on_device()
    boxes, lut = _boxes(FI.SOURCES, "whole").to(DEV), D.LUT.to(DEV)
    x, y = ops.batch_rrc(pixels, offsets, sizes, labels, torch.empty(0, dtype=torch.int32, device=DEV), boxes, None, lut, 24)
    assert x.shape == (0, 3, 24, 24) and y.shape == (0,)
    idx = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    with pytest.raises(N.EEError, match="no CPU fallback"):
        ops.batch_rrc(pixels.cpu(), offsets, sizes, labels, idx, boxes, None, lut, 24)
    with pytest.raises(N.EEError, match="no CPU fallback"):
        ops.batch_rrc(pixels, offsets, sizes, labels, idx, boxes.cpu(), None, lut, 24)
    out = torch.empty(2 * 3 * 24 * 24 + 1, dtype=torch.float32, device=DEV)
    yo = torch.empty(2, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    call = lambda o: N.lib.ee_batch_rrc_u8_f32(p(pixels), pixels.numel(), p(offsets), p(sizes), p(labels), p(idx), p(boxes), None, p(lut), 5, 2,
                                               24, ctypes.c_void_p(o), p(yo), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert call(out.data_ptr() + 2) == -4  # EE_ERR_ALIGN, as ee_batch_u8_f32
    assert call(out.data_ptr() + 4) == 0   # 4-byte aligned only: the scalar stores
    torch.cuda.synchronize()
    xr, _ = D.host_batch_rrc(*common.host, torch.tensor([0, 1]), boxes.cpu(), None, 24)
    assert torch.equal(out[1:].view(2, 3, 24, 24).cpu(), xr)


@pytest.mark.gpu
def test_ragged_loader_on_the_device_yields_the_host_loaders_batches(tmp_path, monkeypatch):
    from eeadv import data as D
    monkeypatch.setenv("EEADV_DATA_CACHE", str(tmp_path / "cache"))
    monkeypatch.delenv("EEADV_IMAGENET_SHORT", raising=False)
    root = str(tmp_path / "inet")
    FI.tree(root)
    spec = {"shape": (3, 24, 24), "num_classes": 3, "resize": 28}
    dev, dev_val = D.make_loaders("imagenet", root, spec, torch.device(DEV), 3, seed=1)
    host, host_val = D.make_loaders("imagenet", root, spec, torch.device("cpu"), 3, seed=1)
    assert isinstance(dev, D.RaggedDeviceLoader) and len(dev) == len(host) == 3 and len(dev_val) == 2
    for epoch in (0, 1):
        seen = []
        for ld in (dev, host):
            ld.set_epoch(epoch)
        for (x, y), (xh, yh) in zip(dev, host):
            assert x.is_cuda and y.is_cuda and x.dtype == torch.float32 and y.dtype == torch.int64
            assert torch.equal(x.cpu(), xh) and torch.equal(y.cpu(), yh)
            seen.append(x.shape[0])
        assert seen == [3, 3, 2]
    # every sample exactly once per epoch, read off what the device loader yields: the same split with label = sample id
    load = lambda: D.load_imagenet(root, "train", (3, 24, 24), 3, 28)
    uniq = D.RaggedDeviceLoader(lambda: load()[:3] + (np.arange(8, dtype=np.int64),), 24, 3, DEV, 1, rank=0, world=1)
    orders = []
    for epoch in (0, 1):
        uniq.set_epoch(epoch)
        _, flip, boxes = uniq.epoch_draws()
        batches = list(uniq)
        ys = torch.cat([y for _, y in batches]).tolist()
        assert sorted(ys) == list(range(8)) and ys == uniq.epoch_draws()[0].tolist()
        xr, _ = D.host_batch_rrc(*(torch.from_numpy(a) for a in load()), torch.tensor(ys), boxes, flip, 24)
        assert torch.equal(torch.cat([x for x, _ in batches]).cpu(), xr)  # and each one is that sample, cropped by its own box
        orders.append(ys)
    assert orders[0] != orders[1]
    for (x, y), (xh, yh) in zip(dev_val, host_val):
        assert torch.equal(x.cpu(), xh) and torch.equal(y.cpu(), yh) and x.shape[1:] == (3, 24, 24)
    # a sample's box and flip at world size 2 are those of world size 1
    _, flip1, box1 = dev.epoch_draws()
    got = {}
    for r in (0, 1):
        ld = D.RaggedDeviceLoader(load, 24, 3, DEV, 1, rank=r, world=2)
        ld.set_epoch(1)
        ids, flip, box = ld.epoch_draws()
        assert torch.equal(flip, flip1) and torch.equal(box, box1)
        xs = torch.cat([x for x, _ in ld]).cpu()
        for s, x in zip(ids.tolist(), xs):
            got[s] = x
    one = D.RaggedDeviceLoader(load, 24, 8, "cpu", 1, rank=0, world=1)
    one.set_epoch(1)
    (x, y), = list(one)
    assert sorted(got) == list(range(8))
    for s, xs in zip(one.epoch_draws()[0].tolist(), x):
        assert torch.equal(got[s], xs)


@pytest.mark.gpu
def test_imagenet_driver_trains_on_a_generated_tree(tmp_path):
    root = str(tmp_path / "inet")
    FI.tree(root)
    out = str(tmp_path / "out")
    env = dict(os.environ, EEADV_DATA_CACHE=str(tmp_path / "cache"))
    env.pop("EEADV_IMAGENET_SHORT", None)
    cfg = FI.small_config(tmp_path, crop_size=64, resize_size=72)
    r = subprocess.run([sys.executable, "experiments_imagenet.py", "-c", cfg, "--data", root, "--max-epochs", "1", "--output-root", out],
                       cwd=os.path.join(PKG, "ImageNet"), capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    logs = [os.path.join(d, f) for d, _, fs in os.walk(out) for f in fs if f == "log.txt"]
    assert len(logs) == 1
    lines = open(logs[0]).read().splitlines()
    train = [l for l in lines if l.startswith("Epoch: [0]")]
    assert len(train) == math.ceil(8 / 4) and train[0].startswith("Epoch: [0][0/2]\t")
    for l in train:
        assert math.isfinite(float(l.split("Loss ")[1].split(" ")[0]))
    assert sum(l.startswith(" * Clean Prec@1") for l in lines) == 1 and sum(l.startswith(" * Adv Prec@1") for l in lines) == 1
    ckpts = [os.path.join(d, f) for d, _, fs in os.walk(out) for f in fs if f.endswith("_0.pth")]
    assert len(ckpts) == 1
    ck = torch.load(ckpts[0], weights_only=True)
    assert ck["epoch"] == 1 and ck["state_dict"]["fc.weight"].shape == (3, 512)
    assert bool(torch.isfinite(ck["state_dict"]["fc.weight"]).all())
    assert sorted(f.split("-")[1] for f in os.listdir(str(tmp_path / "cache"))) == ["train", "val"]
