"""Generators for the ImageNet tests (eeadv.data kind `imagenet`): a small ImageFolder tree with files of mixed sizes and
formats, the sources / boxes / result sides of the resample checks, and a ragged split packed from arrays.  Nothing here is a
real dataset; every pixel comes from a seeded generator."""
import os

import numpy as np
from PIL import Image

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "edge-enhancement_amd")
CLASSES = ["n01440764", "n01530575", "n02085620"]

# (H, W) of the random RGB sources of the resample checks.  Beyond the common sizes: 1 x 4800 makes the kernel's coefficient
# tables outgrow its LDS stage at S = 24 (the direct path), 1600 x 16 makes a 16-row band need more source rows than the stage
# holds (several stages per band).  Every box of boxes_of() is checked against PIL on every source.  The one crop family where PIL's
# bytes are not the restatement's (eeadv.data.resample_u8: h > 100 w, w >= 2, S < h) has no member among SOURCES' boxes - the full
# columns have w = 1 - and one among EXTREME_SOURCES': the corner crop (800, 11, 800, 5) of 1600 x 16 at every S.  That one is held
# against PIL's two passes run one after the other in the restatement's order, and is asserted to differ from the one-call resize.
SOURCES = [(9, 11), (37, 53), (64, 48), (300, 211), (500, 375)]
EXTREME_SOURCES = [(1, 4800), (1600, 16)]
SIDES = [24, 43, 224]


def boxes_of(H, W):
    """(top, left, h, w): the whole image, 1 x 1, one full row, one full column, a crop touching the bottom-right corner."""
    h, w = max(1, H // 2), max(1, W // 3)
    return [(0, 0, H, W), (H // 2, W // 2, 1, 1), (H // 3, 0, 1, W), (0, W // 3, H, 1), (H - h, W - w, h, w)]


def source(H, W, seed=0):
    return np.random.default_rng(seed * 100003 + H * 1009 + W).integers(0, 256, (H, W, 3), dtype=np.uint8)


def pil_crop_resize(img, box, S):
    top, left, h, w = box
    return np.asarray(Image.fromarray(img).crop((left, top, left + w, top + h)).resize((S, S), Image.BILINEAR))


def in_pils_vertical_first_exception(box, S):
    """The crops whose bytes PIL forms in the other pass order (eeadv.data.resample_u8 states the condition)."""
    return box[2] > 100 * box[3] and box[3] >= 2 and S < box[2]


def pil_crop_resize_horizontal_first(img, box, S):
    """PIL's own arithmetic in the order the restatement and the kernel keep everywhere: the crop resized along w only (PIL then
    runs its horizontal pass alone), then along h only."""
    top, left, h, w = box
    rows = Image.fromarray(img).crop((left, top, left + w, top + h)).resize((S, h), Image.BILINEAR)
    return np.asarray(rows.resize((S, S), Image.BILINEAR))


def pack(images):
    """[uint8 [H,W,3]] -> the ragged (pixels [bytes], offsets int64 [N], sizes int32 [N,2])."""
    sizes = np.array([a.shape[:2] for a in images], dtype=np.int32)
    nbytes = sizes[:, 0].astype(np.int64) * sizes[:, 1] * 3
    offsets = np.concatenate([np.zeros(1, np.int64), np.cumsum(nbytes)[:-1]])
    return np.concatenate([a.reshape(-1) for a in images]), offsets, sizes


def _save(path, arr, fmt):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path, format=fmt)


# train files per class in ImageFolder order: (relative path, (H, W), format, grayscale)
TRAIN = [
    [("a_0.png", (20, 31), "PNG", False), ("b_1.JPEG", (48, 36), "JPEG", False), ("sub/c_2.png", (33, 33), "PNG", False)],
    [("d_0.JPEG", (40, 64), "JPEG", True), ("e_1.png", (17, 52), "PNG", False)],
    [("f_0.png", (64, 40), "PNG", False), ("g_1.jpg", (25, 25), "JPEG", False), ("h_2.png", (90, 70), "PNG", False)],
]
VAL = [[("v0.png", (50, 70), "PNG", False)], [("v1.JPEG", (80, 45), "JPEG", False), ("v2.png", (40, 40), "PNG", False)],
       [("v3.png", (33, 77), "PNG", False)]]


def tree(root, seed=0, classes=CLASSES):
    """<root>/{train,val}/<wnid>/... with PNG and JPEG files of mixed sizes, one grayscale JPEG and one file that is no image.
    Returns {split: [(path, label, uint8 [H,W,3] as PIL decodes it with convert('RGB'))]} in ImageFolder order."""
    rng = np.random.default_rng(seed)
    out = {}
    for split, spec in (("train", TRAIN), ("val", VAL)):
        items = []
        for label, (cls, files) in enumerate(zip(classes, spec)):
            for rel, (H, W), fmt, gray in sorted(files, key=lambda f: (os.path.dirname(f[0]), f[0])):
                path = os.path.join(root, split, cls, rel)
                # uniform noise; PNG keeps the bytes, a JPEG's are whatever PIL reads back below
                arr = rng.integers(0, 256, (H, W) if gray else (H, W, 3), dtype=np.uint8)
                _save(path, arr, fmt)
                items.append((path, label))
        with open(os.path.join(root, split, classes[0], "notes.txt"), "w") as f:
            f.write("not an image\n")
        out[split] = [(p, lab, np.asarray(Image.open(p).convert("RGB"))) for p, lab in items]
    return out


def small_config(tmp_path, **over):
    """ImageNet/configs_imagenet/standard_training.yml shrunk to a batch of 4, one attack step, 3 classes and 32 x 32 crops of
    images resized to 40 (`over` replaces the three size keys); written into tmp_path, returns its path."""
    base = open(os.path.join(PKG, "ImageNet/configs_imagenet/standard_training.yml")).read()
    for a, b in (("batch_size: 256\n", "batch_size: 4\n"), ("num_steps_1: 10\n", "num_steps_1: 1\n"), ("cize: 224\n", "cize: 32\n"),
                 ("print_freq: 100\n", "print_freq: 1\n")):
        assert a in base
        base = base.replace(a, b)
    keys = dict(num_classes=3, crop_size=32, resize_size=40)
    keys.update(over)
    cfg = tmp_path / "st.yml"
    cfg.write_text(base + "".join("%s: %s\n" % kv for kv in keys.items()))
    return str(cfg)
