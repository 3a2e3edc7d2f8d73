"""Generators of small fake dataset trees for the eeadv.data tests: Tiny-ImageNet-style ImageFolder trees (PNG / JPEG written
with PIL) and MNIST IDX files (numpy).  Nothing here is a real dataset; every pixel comes from a seeded generator."""
import gzip
import os
import struct

import numpy as np
from PIL import Image


def wnids(n):
    return ["n%08d" % (1000 + 7 * k) for k in range(n)]


def write_image(path, arr, fmt=None):
    """arr uint8 [H,W,3] or [H,W] (grayscale).  PNG is lossless; JPEG is not (compare against what PIL decodes back)."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path, format=fmt)


def tiny_tree(root, n_classes=200, per_class=1, extra=0, n_val=10, size=64, val_layout="raw", seed=0, ext=".png"):
    """<root>/train/<wnid>/images/<wnid>_<k><ext> (+ <wnid>_boxes.txt, which is not an image), one more image in each of the
    first `extra` classes, and <root>/val in the raw (images/ + val_annotations.txt) or the ImageFolder layout.
    Returns (classes, n_train, n_val)."""
    rng = np.random.default_rng(seed)
    classes = wnids(n_classes)
    n_train = 0
    for ci, w in enumerate(classes):
        d = os.path.join(root, "train", w, "images")
        for k in range(per_class + (1 if ci < extra else 0)):
            write_image(os.path.join(d, "%s_%d%s" % (w, k, ext)), rng.integers(0, 256, (size, size, 3), dtype=np.uint8))
            n_train += 1
        with open(os.path.join(root, "train", w, w + "_boxes.txt"), "w") as f:
            f.write("%s_0%s\t0\t0\t%d\t%d\n" % (w, ext, size - 1, size - 1))
    lines = []
    for k in range(n_val):
        w = classes[(3 * k) % n_classes]
        name = "val_%d%s" % (k, ext)
        arr = rng.integers(0, 256, (size, size, 3), dtype=np.uint8)
        if val_layout == "raw":
            write_image(os.path.join(root, "val", "images", name), arr)
            lines.append("%s\t%s\t0\t0\t%d\t%d\n" % (name, w, size - 1, size - 1))
        else:
            write_image(os.path.join(root, "val", w, name), arr)
    if val_layout == "raw":
        with open(os.path.join(root, "val", "val_annotations.txt"), "w") as f:
            f.writelines(lines)
    else:
        for w in classes:
            os.makedirs(os.path.join(root, "val", w), exist_ok=True)
    return classes, n_train, n_val


def write_idx(path, arr, magic, gz=False):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    head = struct.pack(">i", magic) + struct.pack(">%di" % arr.ndim, *arr.shape)
    with (gzip.open if gz else open)(path, "wb") as f:
        f.write(head + np.ascontiguousarray(arr, dtype=np.uint8).tobytes())


def mnist_tree(root, n_train=45, n_test=20, gz=False, torchvision_layout=True, seed=0):
    """IDX files of random 28x28 images and labels 0..9 in <root>/MNIST/raw/ (torchvision's layout) or <root>/.
    Returns {split: (images uint8 [N,28,28], labels uint8 [N])}."""
    rng = np.random.default_rng(seed)
    d = os.path.join(root, "MNIST", "raw") if torchvision_layout else str(root)
    out = {}
    for split, stem, n in (("train", "train", n_train), ("test", "t10k", n_test)):
        x = rng.integers(0, 256, (n, 28, 28), dtype=np.uint8)
        y = rng.integers(0, 10, (n,), dtype=np.uint8)
        sfx = ".gz" if gz else ""
        write_idx(os.path.join(d, "%s-images-idx3-ubyte%s" % (stem, sfx)), x, 2051, gz)
        write_idx(os.path.join(d, "%s-labels-idx1-ubyte%s" % (stem, sfx)), y, 2049, gz)
        out[split] = (x, y)
    return out
