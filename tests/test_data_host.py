"""CPU: the real-dataset path of the drivers (eeadv.data) - ImageFolder / Tiny val / MNIST IDX readers, the decode cache, the
per-epoch order and flips, DistributedSampler sharding, the ABI checks of ee_batch_u8_f32, and the MNIST driver on a generated
IDX directory with --no-cuda."""
import ctypes
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


@pytest.fixture
def D(monkeypatch):
    monkeypatch.delenv("EEADV_DATA_CACHE", raising=False)
    from eeadv import data
    return data


def _png(path, arr):
    F.write_image(str(path), arr, fmt="PNG")


# ---- ImageFolder semantics -----------------------------------------------------------------------------------------------------
def test_image_folder_order_labels_nesting_extensions_and_grayscale(tmp_path, D):
    rng = np.random.default_rng(1)
    img = {k: rng.integers(0, 256, (8, 8, 3), dtype=np.uint8) for k in "abcdef"}
    tr = tmp_path / "train"
    _png(tr / "n2" / "b.png", img["a"])
    _png(tr / "n2" / "a.PNG", img["b"])              # upper-case extension counts
    _png(tr / "n2" / "sub" / "0.png", img["c"])      # nested directory, walked after n2/ itself
    (tr / "n2" / "n2_boxes.txt").write_text("x\n")   # not an image
    _png(tr / "n1" / "z.png", img["d"])
    gray = rng.integers(0, 256, (8, 8), dtype=np.uint8)
    F.write_image(str(tr / "n1" / "g.JPEG"), gray, fmt="JPEG")  # grayscale JPEG -> convert('RGB')
    _png(tr / "n3" / "deep" / "er" / "q.png", img["e"])
    (tr / "n3" / "readme.md").write_text("x")
    classes, samples, _ = D.tiny_listing(str(tmp_path), "train", 3)
    assert classes == ["n1", "n2", "n3"]
    rel = [(os.path.relpath(p, str(tr)), lab) for p, lab in samples]
    assert rel == [("n1/g.JPEG", 0), ("n1/z.png", 0), ("n2/a.PNG", 1), ("n2/b.png", 1), ("n2/sub/0.png", 1), ("n3/deep/er/q.png", 2)]
    x, y = D.load_tiny_imagenet(str(tmp_path), "train", (3, 8, 8), 3)
    assert x.shape == (6, 8, 8, 3) and x.dtype == np.uint8 and y.tolist() == [0, 0, 1, 1, 1, 2]
    from PIL import Image
    g = np.asarray(Image.open(str(tr / "n1" / "g.JPEG")).convert("L"))
    assert np.array_equal(x[0, :, :, 0], g) and np.array_equal(x[0, :, :, 1], g) and np.array_equal(x[0, :, :, 2], g)
    assert np.array_equal(x[1], img["d"]) and np.array_equal(x[2], img["b"]) and np.array_equal(x[4], img["c"])


def test_wrong_class_count_and_wrong_image_size_are_refused(tmp_path, D):
    F.tiny_tree(str(tmp_path), n_classes=4, size=8, n_val=2)
    with pytest.raises(D.DataError, match="4 class directories, expected 5"):
        D.load_tiny_imagenet(str(tmp_path), "train", (3, 8, 8), 5)
    bad = tmp_path / "train" / F.wnids(4)[2] / "images" / "odd.png"
    _png(bad, np.zeros((8, 9, 3), np.uint8))
    with pytest.raises(D.DataError, match="odd.png is 9x8 .*expected 8x8"):
        D.load_tiny_imagenet(str(tmp_path), "train", (3, 8, 8), 4)


def test_tiny_val_raw_and_imagefolder_layouts_give_the_same_labels(tmp_path, D):
    raw, folder = tmp_path / "raw", tmp_path / "folder"
    F.tiny_tree(str(raw), n_classes=6, size=8, n_val=12, val_layout="raw", seed=3)
    F.tiny_tree(str(folder), n_classes=6, size=8, n_val=12, val_layout="folder", seed=3)
    _, sr, _ = D.tiny_listing(str(raw), "val", 6)
    _, sf, _ = D.tiny_listing(str(folder), "val", 6)
    by_name_r = {os.path.basename(p): lab for p, lab in sr}
    by_name_f = {os.path.basename(p): lab for p, lab in sf}
    assert len(by_name_r) == 12 and by_name_r == by_name_f
    xr, yr = D.load_tiny_imagenet(str(raw), "val", (3, 8, 8), 6)
    xf, yf = D.load_tiny_imagenet(str(folder), "val", (3, 8, 8), 6)
    order_r = [os.path.basename(p) for p, _ in sr]
    order_f = [os.path.basename(p) for p, _ in sf]
    for k, name in enumerate(order_r):
        j = order_f.index(name)
        assert np.array_equal(xr[k], xf[j]) and yr[k] == yf[j]
    # a file the annotations do not list is named
    _png(raw / "val" / "images" / "stray.png", np.zeros((8, 8, 3), np.uint8))
    with pytest.raises(D.DataError, match="stray.png is not listed"):
        D.tiny_listing(str(raw), "val", 6)


# ---- MNIST IDX ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gz", [False, True])
@pytest.mark.parametrize("torchvision_layout", [True, False])
def test_mnist_idx_plain_gz_and_both_layouts(tmp_path, D, gz, torchvision_layout):
    ref = F.mnist_tree(str(tmp_path), n_train=13, n_test=7, gz=gz, torchvision_layout=torchvision_layout)
    assert D.recognised("mnist", str(tmp_path))
    for split in ("train", "test"):
        x, y = D.load_mnist(str(tmp_path), split)
        assert x.shape == (len(ref[split][0]), 28, 28, 1) and y.dtype == np.int64
        assert np.array_equal(x[..., 0], ref[split][0]) and np.array_equal(y, ref[split][1].astype(np.int64))


def test_mnist_bad_magic_and_missing_files_are_refused(tmp_path, D):
    F.mnist_tree(str(tmp_path), n_train=5, n_test=3)
    p = tmp_path / "MNIST" / "raw" / "train-images-idx3-ubyte"
    raw = bytearray(p.read_bytes())
    raw[3] = 0x04  # 2051 -> 2052
    p.write_bytes(bytes(raw))
    with pytest.raises(D.DataError, match="magic number 2052, expected 2051"):
        D.load_mnist(str(tmp_path), "train")
    assert not D.recognised("mnist", str(tmp_path / "MNIST"))
    assert not D.recognised("tiny_imagenet", str(tmp_path))


# ---- cache ----------------------------------------------------------------------------------------------------------------------
def _boom(*a, **k):
    raise AssertionError("decoded although the cache is valid")


def test_cache_is_reused_invalidated_by_a_touched_file_and_relocatable(tmp_path, D, monkeypatch):
    root = tmp_path / "tiny"
    F.tiny_tree(str(root), n_classes=4, size=8, n_val=3)
    x1, y1 = D.load_tiny_imagenet(str(root), "train", (3, 8, 8), 4)
    cached = sorted(os.listdir(str(root / ".eeadv_cache")))
    assert len(cached) == 1 and cached[0].startswith("tiny_imagenet-train-")
    import PIL.Image
    with monkeypatch.context() as m:
        m.setattr(PIL.Image, "open", _boom)
        x2, y2 = D.load_tiny_imagenet(str(root), "train", (3, 8, 8), 4)  # no decode
        assert np.array_equal(x1, x2) and np.array_equal(y1, y2)
        one = root / "train" / F.wnids(4)[1] / "images" / (F.wnids(4)[1] + "_0.png")
        st = os.stat(str(one))
        os.utime(str(one), ns=(st.st_atime_ns, st.st_mtime_ns + 10 ** 9))
        with pytest.raises(AssertionError, match="decoded although"):  # the touched file forces a rebuild
            D.load_tiny_imagenet(str(root), "train", (3, 8, 8), 4)
    x3, _ = D.load_tiny_imagenet(str(root), "train", (3, 8, 8), 4)
    assert np.array_equal(x1, x3) and len(os.listdir(str(root / ".eeadv_cache"))) == 2
    other = tmp_path / "elsewhere"
    monkeypatch.setenv("EEADV_DATA_CACHE", str(other))
    D.load_tiny_imagenet(str(root), "val", (3, 8, 8), 4)
    assert [f.split("-")[1] for f in os.listdir(str(other))] == ["val"]
    assert not any("-val-" in f for f in os.listdir(str(root / ".eeadv_cache")))


def test_unwritable_cache_decodes_in_memory(tmp_path, D, monkeypatch, capsys):
    root = tmp_path / "tiny"
    F.tiny_tree(str(root), n_classes=2, size=8, n_val=2)
    blocker = tmp_path / "file"
    blocker.write_text("not a directory")
    monkeypatch.setenv("EEADV_DATA_CACHE", str(blocker / "cache"))
    x, y = D.load_tiny_imagenet(str(root), "train", (3, 8, 8), 2)
    assert x.shape == (2, 8, 8, 3) and y.tolist() == [0, 1]
    assert "not writable" in capsys.readouterr().out


# ---- epoch order, flips, sharding, lengths ----------------------------------------------------------------------------------------
def _array_split(n, H=4, W=4, C=3, seed=0):
    rng = np.random.default_rng(seed)
    return lambda: (rng.integers(0, 256, (n, H, W, C), dtype=np.uint8), np.arange(n, dtype=np.int64) % 7)


def _id_split(n, H=2, W=4, C=1):
    """a split whose label is the sample id"""
    return lambda: (np.zeros((n, H, W, C), np.uint8), np.arange(n, dtype=np.int64))


def _ids(batches):
    return torch.cat([y for _, y in batches]).tolist()


def test_same_seed_and_epoch_give_the_same_batches_other_epochs_another_order(D):
    mk = lambda: D.DeviceLoader(_array_split(300), 32, "cpu", seed=5, shuffle=True, flip=True, rank=0, world=1)
    a, b = mk(), mk()
    for e in (0, 3):
        a.set_epoch(e)
        b.set_epoch(e)
        for (xa, ya), (xb, yb) in zip(a, b):
            assert torch.equal(xa, xb) and torch.equal(ya, yb)
    ld = D.DeviceLoader(_id_split(300), 32, "cpu", seed=5, shuffle=True, flip=False, rank=0, world=1)
    orders = []
    for e in (0, 1):
        ld.set_epoch(e)
        orders.append(_ids(list(ld)))
    assert orders[0] != orders[1] and sorted(orders[0]) == sorted(orders[1]) == list(range(300))


def test_flip_flags_are_fair_and_applied(D):
    n = 20000
    ld = D.DeviceLoader(_array_split(n), 1000, "cpu", seed=0, shuffle=True, flip=True, rank=0, world=1)
    _, flip = ld.epoch_order()
    assert abs(float(flip.float().mean()) - 0.5) < 0.02
    x, y = next(iter(D.DeviceLoader(_array_split(8, H=3, W=5), 8, "cpu", seed=2, shuffle=False, flip=True, rank=0, world=1)))
    images, _ = _array_split(8, H=3, W=5)()
    ld = D.DeviceLoader(_array_split(8, H=3, W=5), 8, "cpu", seed=2, shuffle=False, flip=True, rank=0, world=1)
    _, f = ld.epoch_order()
    ref = torch.from_numpy(images).permute(0, 3, 1, 2).float() / 255
    ref = torch.where(f[:, None, None, None], ref.flip(-1), ref)
    assert torch.equal(x, ref) and x.shape == (8, 3, 3, 5) and x.stride() == (45, 15, 5, 1)
    x1, _ = next(iter(D.DeviceLoader(_array_split(8, C=1), 8, "cpu", seed=2, shuffle=True, flip=True, rank=0, world=1)))
    assert x1.stride() == (16, 16, 4, 1)  # NCHW strides at C = 1 too (a channels-last float tensor breaks Net_2's .view)


def test_sharding_at_world_two(D):
    n, B = 101, 8
    w1 = D.DeviceLoader(_id_split(n), B, "cpu", seed=9, shuffle=True, flip=True, rank=0, world=1)
    ranks = [D.DeviceLoader(_id_split(n), B, "cpu", seed=9, shuffle=True, flip=True, rank=r, world=2) for r in (0, 1)]
    assert len(ranks[0]) == len(ranks[1]) == math.ceil(51 / B)
    ids = [_ids(list(ld)) for ld in ranks]
    assert len(ids[0]) == len(ids[1]) == 51
    assert sorted(ids[0] + ids[1]) == sorted(list(range(n)) + [w1.epoch_order()[0][0].item()])  # one sample padded by wrap-around
    assert torch.equal(ranks[0].epoch_order()[1], w1.epoch_order()[1]) and torch.equal(ranks[1].epoch_order()[1], w1.epoch_order()[1])
    perm = w1.epoch_order()[0].tolist()
    assert ids[0] == perm[0::2] and ids[1] == perm[1::2] + perm[:1]


def test_len_and_the_partial_last_batch(D):
    ld = D.DeviceLoader(_array_split(45), 8, "cpu", seed=0, shuffle=True, flip=False, rank=0, world=1)
    sizes = [x.shape[0] for x, _ in ld]
    assert len(ld) == 6 and sizes == [8, 8, 8, 8, 8, 5]


def test_loaders_are_lazy(tmp_path, D):
    calls = []
    ld = D.DeviceLoader(lambda: calls.append(1) or _array_split(5)(), 2, "cpu", seed=0, shuffle=False, flip=False)
    assert calls == []
    assert len(ld) == 3 and calls == [1]


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def test_batch_u8_argument_checks_happen_before_any_launch():
    import eeadv._native as n
    L = n.lib
    q = ctypes.c_void_p(4096)
    args = lambda **kw: [kw.get(k, d) for k, d in (("data", q), ("labels", q), ("idx", q), ("flip", None), ("lut", q), ("N", 10),
                                                       ("B", 4), ("C", 3), ("H", 8), ("W", 8), ("out", q), ("labels_out", q))] + [None]
    assert L.ee_batch_u8_f32(*args(data=None)) == -1
    assert L.ee_batch_u8_f32(*args(lut=None)) == -1
    assert L.ee_batch_u8_f32(*args(labels_out=None)) == -1
    assert L.ee_batch_u8_f32(*args(B=-1)) == -2
    assert L.ee_batch_u8_f32(*args(N=0)) == -2
    assert L.ee_batch_u8_f32(*args(H=0)) == -2
    assert L.ee_batch_u8_f32(*args(C=2)) == -3 and L.ee_batch_u8_f32(*args(C=4)) == -3
    assert L.ee_batch_u8_f32(*args(out=ctypes.c_void_p(4098))) == -4
    assert L.ee_batch_u8_f32(*args(B=0, data=None, out=None)) == 0  # empty batch: nothing to do


# ---- drivers --------------------------------------------------------------------------------------------------------------------
def _find(out, name):
    return [os.path.join(d, f) for d, _, fs in os.walk(str(out)) for f in fs if f == name or f.endswith(name)]


def test_mnist_driver_trains_on_a_generated_idx_directory_on_cpu(tmp_path):
    F.mnist_tree(str(tmp_path / "mnist"), n_train=45, n_test=20, gz=True)
    base = open(os.path.join(PKG, "MNIST/configs_mnist/standard_training.yml")).read()
    assert "batch_size: 50\n" in base
    cfg = tmp_path / "st.yml"
    cfg.write_text(base.replace("batch_size: 50\n", "batch_size: 8\n"))
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, "experiments_mnist.py", "-c", str(cfg), "--no-cuda", "--data", str(tmp_path / "mnist"),
                        "--max-epochs", "1", "--output-root", str(out)], cwd=os.path.join(PKG, "MNIST"), capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    logs = _find(out, "log.txt")
    assert len(logs) == 1
    lines = open(logs[0]).read().splitlines()
    assert lines[0].startswith("Epoch: [0][0/%d]" % math.ceil(45 / 8))
    assert any(l.startswith(" * Clean Prec@1") for l in lines) and any(l.startswith(" * Adv Prec@1") for l in lines)
    ckpts = _find(out, "_0.pth")
    assert len(ckpts) == 1
    ck = torch.load(ckpts[0], weights_only=True)
    assert ck["epoch"] == 1 and any(k.startswith("module.") for k in ck["state_dict"])


def test_drivers_without_a_data_kind_refuse_a_directory(tmp_path):
    r = subprocess.run([sys.executable, "experiments_imagenet.py", "-c", "configs_imagenet/standard_training.yml", "--no-cuda",
                        "--data", str(tmp_path), "--output-root", str(tmp_path)], cwd=os.path.join(PKG, "ImageNet"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "synthetic" in r.stderr and "NotImplementedError" in r.stderr
    r = subprocess.run([sys.executable, "AT_free_imagenet_ddp.py", "--data", str(tmp_path)], cwd=os.path.join(PKG, "ImageNet", "free_imagenet"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "supports only --data synthetic" in r.stderr


def test_unrecognised_directory_names_the_expected_layout(tmp_path):
    (tmp_path / "train").mkdir()
    r = subprocess.run([sys.executable, "experiments_tinyimagenet.py", "-c", "configs_tinyimagenet/standard_training.yml", "--no-cuda",
                        "--data", str(tmp_path), "--output-root", str(tmp_path)], cwd=os.path.join(PKG, "Tiny_ImageNet"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "synthetic" in r.stderr and "val_annotations.txt" in r.stderr
