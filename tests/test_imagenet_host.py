"""CPU: ImageNet for the ImageNet driver (eeadv.data kind `imagenet`) - the numpy restatement of PIL's 8-bit BILINEAR resample
against PIL itself, RandomResizedCrop's boxes, the ragged train split and the Resize + CenterCrop val split with their caches,
the host loader, the ABI checks of ee_batch_rrc_u8_f32, and experiments_imagenet.py on a generated tree with --no-cuda."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import fake_imagenet as FI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")


@pytest.fixture
def D(monkeypatch):
    monkeypatch.delenv("EEADV_DATA_CACHE", raising=False)
    monkeypatch.delenv("EEADV_IMAGENET_SHORT", raising=False)
    from eeadv import data
    return data


# ---- the resample rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", FI.SOURCES + FI.EXTREME_SOURCES)
def test_host_restatement_is_pils_bilinear_resize_byte_for_byte(D, H, W):
    img = FI.source(H, W)
    for S in FI.SIDES:
        for box in FI.boxes_of(H, W):
            top, left, h, w = box
            got = D.resample_u8(img[top:top + h, left:left + w], S, S)
            assert got.dtype == np.uint8 and got.shape == (S, S, 3)
            if FI.in_pils_vertical_first_exception(box, S):  # only 1600 x 16's corner crop: PIL's passes in the other order
                assert (H, W) == (1600, 16) and np.array_equal(got, FI.pil_crop_resize_horizontal_first(img, box, S)), (H, W, S, box)
                assert not np.array_equal(got, FI.pil_crop_resize(img, box, S))
                continue
            assert np.array_equal(got, FI.pil_crop_resize(img, box, S)), (H, W, S, box)


def test_resample_to_another_aspect_and_identity(D):
    img = FI.source(64, 48)
    assert np.array_equal(D.resample_u8(img, 32, 43), np.asarray(Image.fromarray(img).resize((43, 32), Image.BILINEAR)))
    same = FI.source(24, 24)
    assert np.array_equal(D.resample_u8(same, 24, 24), same)
    xmin, n, k = D.resample_coeffs(500, 224)
    assert k.shape == (224, 7) and int(n.max()) <= 7 and bool((k >= 0).all())          # downscale by more than 2: ksize 7
    assert bool((np.abs(k.sum(1) - (1 << 22)) <= 7).all()) and bool((xmin + n <= 500).all())
    assert D.resample_coeffs(9, 24)[2].shape == (24, 3)                                 # upscale: support 1


# ---- RandomResizedCrop's boxes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(9, 11), (500, 375), (32, 600)])
def test_rrc_boxes_lie_inside_keep_the_ratio_range_and_fall_back(D, H, W):
    n = 20000
    sizes = np.tile(np.array([[H, W]], dtype=np.int32), (n, 1))
    box = D.rrc_boxes(sizes, torch.Generator().manual_seed(11))
    assert box.dtype == torch.int32 and box.shape == (n, 4)
    top, left, h, w = (box[:, i].long() for i in range(4))
    assert bool(((h >= 1) & (w >= 1) & (top >= 0) & (left >= 0) & (top + h <= H) & (left + w <= W)).all())
    in_ratio = W / H
    fw = int(round(H * 4 / 3)) if in_ratio > 4 / 3 else W
    fh = int(round(W / (3 / 4))) if in_ratio < 3 / 4 else H
    fallback = (h == fh) & (w == fw) & (top == (H - fh) // 2) & (left == (W - fw) // 2)
    # an accepted try has w = round(sqrt(a r)), h = round(sqrt(a / r)) with r in [3/4, 4/3]: sqrt(a r) / sqrt(a / r) = r, and each
    # of the two is within 0.5 of its rounded value
    acc = ~fallback
    lo = (w.double() - 0.5) / (h.double() + 0.5)
    hi = (w.double() + 0.5) / (h.double() - 0.5).clamp_min(1e-9)
    assert bool(((lo <= 4 / 3) & (hi >= 3 / 4))[acc].all())
    area = (h * w).double() / (H * W)
    assert bool((area[acc] <= 1.0).all())
    if (H, W) == (32, 600):  # ratio 18.75: no try can fit h <= 32 at 8 % of the area, so the central 32 x 43 crop it is
        assert fh == 32 and fw == 43 and int(fallback.sum()) > 0
        assert bool((box[fallback] == torch.tensor([0, (600 - 43) // 2, 32, 43], dtype=torch.int32)).all())
    if (H, W) == (500, 375):
        assert int(fallback.sum()) < n // 100 and 0.3 < float(area.mean()) < 0.6  # U(0.08, 1) thinned at the large end by rejection
        assert int(top.max()) > 250 and int(left.max()) > 180 and int(top.min()) == 0 and int(left.min()) == 0


def test_rrc_boxes_repeat_for_a_seed_and_epoch_and_change_across_epochs(D):
    images = [FI.source(H, W) for H, W in ((40, 60), (64, 48), (30, 30), (50, 20))] * 5
    pixels, offsets, sizes = FI.pack(images)
    labels = np.arange(len(images), dtype=np.int64)
    mk = lambda **kw: D.RaggedDeviceLoader(lambda: (pixels, offsets, sizes, labels), 24, 6, "cpu", seed=4, **kw)
    a, b = mk(rank=0, world=1), mk(rank=0, world=1)
    a.set_epoch(2), b.set_epoch(2)
    ia, fa, ba = a.epoch_draws()
    ib, fb, bb = b.epoch_draws()
    assert torch.equal(ia, ib) and torch.equal(fa, fb) and torch.equal(ba, bb)
    b.set_epoch(3)
    assert not torch.equal(ba, b.epoch_draws()[2]) and not torch.equal(ia, b.epoch_draws()[0])
    # indexed by sample id: the same at world size 2, whichever rank asks
    for r in (0, 1):
        ld = mk(rank=r, world=2)
        ld.set_epoch(2)
        ids, f, bx = ld.epoch_draws()
        assert torch.equal(f, fa) and torch.equal(bx, ba) and ids.tolist() == (ia.tolist()[r::2])
    assert not torch.equal(ba, D.rrc_boxes(sizes, torch.Generator().manual_seed(99)))


def test_host_loader_yields_every_sample_once_cropped_resized_and_flipped(D):
    images = [FI.source(H, W, seed=k) for k, (H, W) in enumerate(((40, 60), (64, 48), (30, 30), (50, 20), (9, 11), (80, 80), (33, 47)))]
    pixels, offsets, sizes = FI.pack(images)
    labels = np.arange(len(images), dtype=np.int64)
    ld = D.RaggedDeviceLoader(lambda: (pixels, offsets, sizes, labels), 24, 3, "cpu", seed=1, rank=0, world=1)
    assert len(ld) == 3
    for epoch in (0, 1):
        ld.set_epoch(epoch)
        _, flip, boxes = ld.epoch_draws()
        seen = []
        for x, y in ld:
            assert x.dtype == torch.float32 and x.shape[1:] == (3, 24, 24) and x.is_contiguous()
            for xb, s in zip(x, y.tolist()):
                ref = FI.pil_crop_resize(images[s], tuple(boxes[s].tolist()), 24)
                ref = torch.from_numpy(ref.copy()).permute(2, 0, 1).float().div(255)  # ToTensor
                assert torch.equal(xb, ref.flip(-1) if bool(flip[s]) else ref)
            seen += y.tolist()
        assert sorted(seen) == list(range(7))


# ---- listing, decode, cache ---------------------------------------------------------------------------------------------------------
def _boom(*a, **k):
    raise AssertionError("decoded although the cache is valid")


def test_train_split_is_ragged_in_imagefolder_order_and_cached(tmp_path, D, monkeypatch):
    root = str(tmp_path / "inet")
    ref = FI.tree(root)["train"]
    assert D.recognised("imagenet", root) and not D.recognised("imagenet", str(tmp_path))
    classes, samples = D.imagenet_listing(root, "train", 3)
    assert classes == FI.CLASSES
    rel = [os.path.relpath(p, os.path.join(root, "train")) for p, _ in samples]
    assert rel == ["n01440764/a_0.png", "n01440764/b_1.JPEG", "n01440764/sub/c_2.png", "n01530575/d_0.JPEG", "n01530575/e_1.png",
                   "n02085620/f_0.png", "n02085620/g_1.jpg", "n02085620/h_2.png"]   # notes.txt is no image
    pixels, offsets, sizes, labels = D.load_imagenet(root, "train", (3, 32, 32), 3, 40)
    assert pixels.dtype == np.uint8 and offsets.dtype == np.int64 and sizes.dtype == np.int32 and labels.dtype == np.int64
    assert labels.tolist() == [0, 0, 0, 1, 1, 2, 2, 2] == [lab for _, lab, _ in ref]
    assert sizes.tolist() == [list(a.shape[:2]) for _, _, a in ref]
    nbytes = [a.size for _, _, a in ref]
    assert offsets.tolist() == [sum(nbytes[:i]) for i in range(8)] and pixels.size == sum(nbytes)
    for (_, _, a), o in zip(ref, offsets.tolist()):
        assert np.array_equal(pixels[o:o + a.size].reshape(a.shape), a)
    gray = ref[3][2]  # the grayscale JPEG: three equal channels
    assert np.array_equal(gray[..., 0], gray[..., 1]) and np.array_equal(gray[..., 0], gray[..., 2])
    cache = os.path.join(root, ".eeadv_cache")
    assert [f.split("-")[:2] for f in os.listdir(cache)] == [["imagenet", "train"]]
    import PIL.Image
    with monkeypatch.context() as m:
        m.setattr(PIL.Image, "open", _boom)
        again = D.load_imagenet(root, "train", (3, 32, 32), 3, 40)  # from the cache
        assert all(np.array_equal(a, b) for a, b in zip(again, (pixels, offsets, sizes, labels)))
        st = os.stat(ref[4][0])
        os.utime(ref[4][0], ns=(st.st_atime_ns, st.st_mtime_ns + 10 ** 9))
        with pytest.raises(AssertionError, match="decoded although"):  # a changed file: a new key
            D.load_imagenet(root, "train", (3, 32, 32), 3, 40)
    assert len(os.listdir(cache)) == 1
    D.load_imagenet(root, "train", (3, 32, 32), 3, 40)
    assert len(os.listdir(cache)) == 2


def test_imagenet_short_changes_the_key_and_the_sizes(tmp_path, D, monkeypatch):
    root = str(tmp_path / "inet")
    ref = FI.tree(root)["train"]
    _, _, full, _ = D.load_imagenet(root, "train", (3, 32, 32), 3, 40)
    monkeypatch.setenv("EEADV_IMAGENET_SHORT", "30")
    pixels, offsets, sizes, _ = D.load_imagenet(root, "train", (3, 32, 32), 3, 40)
    assert len(os.listdir(os.path.join(root, ".eeadv_cache"))) == 2
    for k, (_, _, a) in enumerate(ref):
        H, W = a.shape[:2]
        if min(H, W) <= 30:
            want = a
        else:
            size = (30, int(30 * H / W)) if W <= H else (int(30 * W / H), 30)
            want = np.asarray(Image.fromarray(a).resize(size, Image.BILINEAR))
            assert min(want.shape[:2]) == 30
        assert sizes[k].tolist() == list(want.shape[:2])
        assert np.array_equal(pixels[offsets[k]:offsets[k] + want.size].reshape(want.shape), want)
    assert sizes.tolist() != full.tolist()
    monkeypatch.setenv("EEADV_IMAGENET_SHORT", "many")
    with pytest.raises(D.DataError, match="EEADV_IMAGENET_SHORT=many"):
        D.load_imagenet(root, "train", (3, 32, 32), 3, 40)


def test_val_split_is_pils_resize_and_center_crop(tmp_path, D, monkeypatch):
    root = str(tmp_path / "inet")
    ref = FI.tree(root)["val"]
    x, y = D.load_imagenet(root, "val", (3, 32, 32), 3, 40)
    assert x.shape == (4, 32, 32, 3) and x.dtype == np.uint8 and y.tolist() == [0, 1, 1, 2]
    for k, (_, _, a) in enumerate(ref):
        H, W = a.shape[:2]
        size = (40, int(40 * H / W)) if W <= H else (int(40 * W / H), 40)       # Resize(40): (w, h)
        im = Image.fromarray(a).resize(size, Image.BILINEAR)
        top, left = int(round((size[1] - 32) / 2.0)), int(round((size[0] - 32) / 2.0))  # CenterCrop(32)
        assert np.array_equal(x[k], np.asarray(im.crop((left, top, left + 32, top + 32)))), k
    import PIL.Image
    with monkeypatch.context() as m:
        m.setattr(PIL.Image, "open", _boom)
        x2, y2 = D.load_imagenet(root, "val", (3, 32, 32), 3, 40)
        assert np.array_equal(x, x2) and np.array_equal(y, y2)
        with pytest.raises(AssertionError, match="decoded although"):  # another crop size: another key
            D.load_imagenet(root, "val", (3, 24, 24), 3, 40)
    monkeypatch.setenv("EEADV_IMAGENET_SHORT", "30")  # the val split does not depend on it
    with monkeypatch.context() as m:
        m.setattr(PIL.Image, "open", _boom)
        D.load_imagenet(root, "val", (3, 32, 32), 3, 40)


def test_wrong_class_counts_and_sizes_are_refused(tmp_path, D):
    root = str(tmp_path / "inet")
    FI.tree(root)
    with pytest.raises(D.DataError, match="3 class directories, expected 1000"):
        D.load_imagenet(root, "train")
    with pytest.raises(D.DataError, match="3 class directories, expected 4"):
        D.load_imagenet(root, "val", (3, 32, 32), 4, 40)
    with pytest.raises(D.DataError, match="resize 24"):
        D.load_imagenet(root, "val", (3, 32, 32), 3, 24)
    os.makedirs(os.path.join(root, "val", "n09999999"))
    with pytest.raises(D.DataError, match="class directories of .*val differ"):
        D.load_imagenet(root, "val", (3, 32, 32), 3, 40)


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def test_batch_rrc_argument_checks_happen_before_any_launch():
    import eeadv._native as n
    L = n.lib
    q = ctypes.c_void_p(4096)
    names = (("pixels", q), ("nbytes", 1000), ("offsets", q), ("sizes", q), ("labels", q), ("idx", q), ("boxes", q), ("flip", None),
             ("lut", q), ("N", 10), ("B", 4), ("S", 24), ("out", q), ("labels_out", q))
    args = lambda **kw: [kw.get(k, d) for k, d in names] + [None]
    for k in ("pixels", "offsets", "sizes", "labels", "idx", "boxes", "lut", "out", "labels_out"):
        assert L.ee_batch_rrc_u8_f32(*args(**{k: None})) == -1, k
    assert L.ee_batch_rrc_u8_f32(*args(B=-1)) == -2 and L.ee_batch_rrc_u8_f32(*args(N=0)) == -2
    assert L.ee_batch_rrc_u8_f32(*args(S=0)) == -2 and L.ee_batch_rrc_u8_f32(*args(nbytes=0)) == -2
    assert L.ee_batch_rrc_u8_f32(*args(S=5000)) == -3
    assert L.ee_batch_rrc_u8_f32(*args(out=ctypes.c_void_p(4098))) == -4
    assert L.ee_batch_rrc_u8_f32(*args(offsets=ctypes.c_void_p(4100))) == -4
    assert L.ee_batch_rrc_u8_f32(*args(B=0, pixels=None, out=None)) == 0  # empty batch: nothing to do


# ---- driver ---------------------------------------------------------------------------------------------------------------------
def _find(out, name):
    return [os.path.join(d, f) for d, _, fs in os.walk(str(out)) for f in fs if f == name or f.endswith(name)]


def test_imagenet_driver_trains_on_a_generated_tree_on_cpu(tmp_path):
    root = str(tmp_path / "inet")
    FI.tree(root)
    out = tmp_path / "out"
    env = dict(os.environ, EEADV_DATA_CACHE=str(tmp_path / "cache"))
    env.pop("EEADV_IMAGENET_SHORT", None)
    r = subprocess.run([sys.executable, "experiments_imagenet.py", "-c", FI.small_config(tmp_path), "--no-cuda", "--data", root,
                        "--max-epochs", "1", "--output-root", str(out)], cwd=os.path.join(PKG, "ImageNet"), capture_output=True, text=True,
                       timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    logs = _find(out, "log.txt")
    assert len(logs) == 1
    lines = open(logs[0]).read().splitlines()
    assert lines[0].startswith("Epoch: [0][0/%d]" % math.ceil(8 / 4))
    assert math.isfinite(float(lines[0].split("Loss ")[1].split(" ")[0]))
    assert any(l.startswith("Test_clean: [0/1]") for l in lines)
    assert sum(l.startswith(" * Clean Prec@1") for l in lines) == 1 and sum(l.startswith(" * Adv Prec@1") for l in lines) == 1
    ckpts = _find(out, "_0.pth")
    assert len(ckpts) == 1
    ck = torch.load(ckpts[0], weights_only=True)
    assert ck["epoch"] == 1 and ck["state_dict"]["fc.weight"].shape == (3, 512)  # bare keys, 3 classes
    assert sorted(f.split("-")[1] for f in os.listdir(str(tmp_path / "cache"))) == ["train", "val"]


def test_imagenet_driver_names_a_wrong_class_count(tmp_path):
    root = str(tmp_path / "inet")
    FI.tree(root)
    r = subprocess.run([sys.executable, "experiments_imagenet.py", "-c", FI.small_config(tmp_path, num_classes=5), "--no-cuda", "--data", root,
                        "--max-epochs", "1", "--output-root", str(tmp_path / "out")], cwd=os.path.join(PKG, "ImageNet"), capture_output=True,
                       text=True, timeout=900)
    assert r.returncode != 0 and "3 class directories, expected 5" in r.stderr
