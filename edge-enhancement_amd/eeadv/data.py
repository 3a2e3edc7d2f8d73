"""Real Tiny-ImageNet, MNIST and ImageNet for the drivers, held whole in device memory.

The reference (utils/data_loader.py) reads the first two with torchvision: ImageFolder + PIL + RandomHorizontalFlip (Tiny train) +
ToTensor in DataLoader workers, and datasets.MNIST + ToTensor.  Here each split is decoded once on the host into uint8
[N,H,W,C] + int64 labels, cached on disk, uploaded to the device once, and every batch is assembled by ONE launch of
ee_batch_u8_f32 (gather the epoch's sample ids, mirror the flagged ones, u8 -> f32 / 255 through a table built with torch's
own division, HWC -> NCHW, gather the labels).  Per step nothing is copied from the host and nothing waits on the device.

Kept semantics
  - ImageFolder: classes = sorted subdirectory names, label = index in that order; samples class by class, each class
    directory walked recursively in sorted order with sorted file names; a file is an image when its lower-cased extension
    is one of IMG_EXTENSIONS (Tiny's train/<wnid>/*_boxes.txt is skipped); images are convert('RGB')'d (Tiny holds a few
    grayscale JPEGs).
  - Tiny val: ImageFolder layout val/<wnid>/..., or the download's own val/images/*.JPEG + val/val_annotations.txt with labels
    mapped through the train split's classes (which the reference's ImageFolder cannot read: it would see one class `images`).
  - MNIST: the IDX files, plain or .gz, in <root>/MNIST/raw/ (torchvision's layout) or <root>/; never downloaded.
  - Loaders: Tiny train shuffled + flipped, Tiny val in file order, MNIST train and test shuffled (as the reference), no
    drop_last (the last batch may be partial).  The reference's draws depend on DataLoader worker seeding and cannot be
    reproduced; the distribution is kept: a uniform permutation per epoch, each sample mirrored with probability 1/2 per epoch.

Not kept: Tiny / MNIST images must already be H x W (the reference has no resize either; a different size is an error naming the file).

ImageNet (utils/data_loader.py:98-120: ImageFolder + RandomResizedCrop(224) + RandomHorizontalFlip + ToTensor for train,
Resize(256) + CenterCrop(224) + ToTensor for val)
  - train: every file is decoded once (convert('RGB')) and kept at its own size in one ragged uint8 buffer (HWC images back to
    back + byte offsets + (H, W) + labels), cached as one .npz and uploaded once.  A batch is ONE launch of ee_batch_rrc_u8_f32:
    crop the epoch's box of each sample, resample it to S x S, mirror, u8 -> f32 through LUT, HWC -> NCHW.  torchvision resizes
    PIL images, and PIL's 8-bit BILINEAR resample is integer fixed-point arithmetic (two passes, 22-bit coefficients formed in
    double); `resample_u8` restates it in numpy and the kernel restates it again, so a batch is ToTensor(resize(crop(img)))
    bit for bit.  `host_batch_rrc` is that restatement for a batch (and what --no-cuda runs).
  - the boxes are RandomResizedCrop.get_params (scale (0.08, 1), ratio (3/4, 4/3), 10 tries, central fallback), drawn on the
    host for the whole split per epoch from torch.Generator(seed + epoch) after the order and the flips, indexed by sample id
    (so they do not depend on world size) and uploaded once per epoch.  As for the flips, the reference's own draws depend on
    DataLoader worker seeding and cannot be reproduced; the distribution is kept.
  - val: Resize + CenterCrop is deterministic, so it is applied once at decode by PIL itself and the split is cached as fixed
    [N,S,S,3]; it is served by DeviceLoader / ee_batch_u8_f32 like Tiny's.
  - the train split must fit in device memory next to the model (checked before the upload, DataError otherwise).  Departure
    from the reference, off by default: EEADV_IMAGENET_SHORT=<pixels> shrinks, at decode, every train image whose shorter side
    exceeds it to that shorter side (PIL BILINEAR, aspect ratio kept); the value is part of the cache key.

CIFAR-100 (utils/data_loader.py:27-60: datasets.CIFAR100 + RandomCrop(32, padding=4) + RandomHorizontalFlip + RandomRotation(15) +
ToTensor for train, ToTensor for test)
  - the two python pickles are read once (`data` [N,3072] planar CHW -> HWC, `fine_labels`), cached and uploaded like Tiny's.
  - train: a batch is ONE launch of ee_batch_aug_u8_f32.  torchvision rotates PIL images with Image.rotate(angle, NEAREST, fillcolor
    = 0): the inverse matrix formed in Python floats (rotate_matrix), walked in 16.16 fixed point by PIL's C code (aug_coeffs).  The
    crop from the zero-padded image, the mirror and that walk are integer arithmetic, restated in `host_batch_aug` (numpy; what
    --no-cuda runs) and in the kernel, so a batch is ToTensor(rotate(flip(crop(pad(img))))) bit for bit.  The draws are per epoch on
    the host, as above; the distribution is the reference's (offsets uniform in [0, 8], angles uniform in [-15, 15]).
  - test: in file order through DeviceLoader / ee_batch_u8_f32.
"""
import gzip
import hashlib
import json
import math
import multiprocessing
import os
import struct

import numpy as np
import torch

from . import ddp

FORMAT_VERSION = 1
IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")
MNIST_FILES = {"train": ("train-images-idx3-ubyte", "train-labels-idx1-ubyte"), "test": ("t10k-images-idx3-ubyte", "t10k-labels-idx1-ubyte")}
LAYOUTS = {
    "tiny_imagenet": "<root>/train/<wnid>/**/*.JPEG and <root>/val/ (val/<wnid>/... or val/images/ + val/val_annotations.txt)",
    "mnist": "the IDX files {train,t10k}-{images-idx3,labels-idx1}-ubyte[.gz] in <root>/MNIST/raw/ or <root>/",
    "imagenet": "<root>/train/<wnid>/**/*.JPEG and <root>/val/<wnid>/**/*.JPEG (the same class directories in both)",
    "cifar100": "the python pickles <root>/cifar-100-python/train and <root>/cifar-100-python/test (or <root>/train and <root>/test)",
}
_CHUNK = 512  # images per decode task

# lut[v] = float(v) / 255 with torch's own division: the batches are ToTensor's values bit for bit, on either device
LUT = torch.arange(256, dtype=torch.uint8).float().div(255)


class DataError(ValueError):
    """A dataset directory that breaks the layout rules (names the file or the count)."""


# ---- listing ------------------------------------------------------------------------------------------------------------------
def is_image(name):
    return name.lower().endswith(IMG_EXTENSIONS)


def find_classes(d):
    return sorted(e.name for e in os.scandir(d) if e.is_dir())


def image_folder(d, classes=None):
    """ImageFolder(d)'s (classes, [(path, label)]); `classes` overrides the directory's own list."""
    classes = find_classes(d) if classes is None else classes
    samples = []
    for label, cls in enumerate(classes):
        for dirpath, _, fnames in sorted(os.walk(os.path.join(d, cls), followlinks=True)):
            samples += [(os.path.join(dirpath, f), label) for f in sorted(fnames) if is_image(f)]
    return classes, samples


def tiny_listing(root, split, num_classes):
    """(classes, [(path, label)], extra source files) of Tiny-ImageNet's `train` or `val` split."""
    train = os.path.join(root, "train")
    classes = find_classes(train)
    if len(classes) != num_classes:
        raise DataError("%s holds %d class directories, expected %d" % (train, len(classes), num_classes))
    if split == "train":
        return classes, image_folder(train, classes)[1], []
    val = os.path.join(root, "val")
    ann, images = os.path.join(val, "val_annotations.txt"), os.path.join(val, "images")
    if os.path.isfile(ann) and os.path.isdir(images):  # the download's layout: val/images/<file> + "<file>\t<wnid>\t..." lines
        to_idx = {c: i for i, c in enumerate(classes)}
        wnid = {}
        with open(ann) as f:
            for line in f:
                parts = line.rstrip("\r\n").split("\t")
                if len(parts) >= 2:
                    wnid[parts[0]] = parts[1]
        samples = []
        for name in sorted(os.listdir(images)):
            if not is_image(name):
                continue
            if name not in wnid:
                raise DataError("%s is not listed in %s" % (os.path.join(images, name), ann))
            if wnid[name] not in to_idx:
                raise DataError("%s: class %s of %s is not a directory of %s" % (ann, wnid[name], name, train))
            samples.append((os.path.join(images, name), to_idx[wnid[name]]))
        return classes, samples, [ann]
    if not os.path.isdir(val):
        raise DataError("%s does not exist" % val)
    vclasses = find_classes(val)
    if len(vclasses) != num_classes:
        raise DataError("%s holds %d class directories (and no images/ + val_annotations.txt), expected %d" % (val, len(vclasses), num_classes))
    if vclasses != classes:
        raise DataError("the class directories of %s differ from those of %s" % (val, train))
    return classes, image_folder(val, classes)[1], []


def recognised(kind, root):
    """Does `root` look like a `kind` dataset directory (LAYOUTS)?  Nothing is decoded."""
    if not os.path.isdir(root):
        return False
    if kind in ("tiny_imagenet", "imagenet"):
        return os.path.isdir(os.path.join(root, "train")) and os.path.isdir(os.path.join(root, "val"))
    if kind == "mnist":
        return all(_mnist_file(root, n) for pair in MNIST_FILES.values() for n in pair)
    if kind == "cifar100":
        return all(os.path.isfile(os.path.join(_cifar_dir(root), n)) for n in ("train", "test"))
    return False


# ---- decode + cache -----------------------------------------------------------------------------------------------------------
def _decode(job):
    from PIL import Image
    paths, H, W, C = job
    out = np.empty((len(paths), H, W, C), dtype=np.uint8)
    for i, p in enumerate(paths):
        with open(p, "rb") as f:
            img = Image.open(f).convert("RGB" if C == 3 else "L")
        if img.size != (W, H):
            raise DataError("%s is %dx%d after convert('RGB'), expected %dx%d (no resize is applied)" % (p, img.size[0], img.size[1], W, H))
        out[i] = np.asarray(img, dtype=np.uint8).reshape(H, W, C)
    return out


def decode_images(paths, H, W, C):
    """uint8 [len(paths),H,W,C], decoded by up to 16 forked processes (the CPUs this process may run on, not the machine's)."""
    out = np.empty((len(paths), H, W, C), dtype=np.uint8)
    jobs = [(paths[i:i + _CHUNK], H, W, C) for i in range(0, len(paths), _CHUNK)]
    procs = min(16, len(os.sched_getaffinity(0)), len(jobs))
    if procs <= 1:
        parts = map(_decode, jobs)
        for k, part in enumerate(parts):
            out[k * _CHUNK:k * _CHUNK + len(part)] = part
        return out
    with multiprocessing.get_context("fork").Pool(procs) as pool:  # the workers only run PIL + numpy, never the device
        for k, part in enumerate(pool.imap(_decode, jobs)):
            out[k * _CHUNK:k * _CHUNK + len(part)] = part
    return out


def cache_dir(root):
    return os.environ.get("EEADV_DATA_CACHE") or os.path.join(root, ".eeadv_cache")


def cache_key(root, parts, files):
    """Hash of the format version, `parts` (dataset, split, shape, class list) and every source file's (path relative to the
    dataset root, size, mtime_ns): any changed file gives a new key."""
    stats = []
    for p in files:
        st = os.stat(p)
        stats.append((os.path.relpath(p, root), st.st_size, st.st_mtime_ns))
    blob = json.dumps([FORMAT_VERSION, list(parts), sorted(stats)], separators=(",", ":"))
    return hashlib.sha256(blob.encode()).hexdigest()[:24]


def cached(root, name, build, keys=("images", "labels")):
    """The arrays `keys` from <cache_dir(root)>/<name>, or build() them and publish the file atomically (temporary name +
    os.replace: concurrent ranks at worst decode twice, none reads a half-written file).  An unwritable cache directory
    leaves the split decoded in memory only."""
    d = cache_dir(root)
    path = os.path.join(d, name)
    if os.path.isfile(path):
        with np.load(path) as z:
            return tuple(z[k] for k in keys)
    arrays = tuple(build())
    tmp = "%s.%d.tmp" % (path, os.getpid())
    try:
        os.makedirs(d, exist_ok=True)
        with open(tmp, "wb") as f:
            np.savez(f, **dict(zip(keys, arrays)))
        os.replace(tmp, path)
    except OSError as exc:
        print("eeadv.data: cache directory %s is not writable (%s): %s is decoded in memory only" % (d, exc.strerror or exc, name))
        try:
            os.remove(tmp)
        except OSError:
            pass
    return arrays


def load_tiny_imagenet(root, split, shape=(3, 64, 64), num_classes=200):
    """Tiny-ImageNet `train` / `val` as (uint8 [N,64,64,3], int64 [N]); decoded once, then read from the cache."""
    C, H, W = shape
    classes, samples, extra = tiny_listing(root, split, num_classes)
    if not samples:
        raise DataError("no images in the %s split of %s" % (split, root))
    paths = [p for p, _ in samples]
    key = cache_key(root, ["tiny_imagenet", split, list(shape), classes], paths + extra)

    def build():
        print("eeadv.data: decoding %d images of %s/%s" % (len(paths), root, split))
        return decode_images(paths, H, W, C), np.array([lab for _, lab in samples], dtype=np.int64)
    return cached(root, "tiny_imagenet-%s-%s.npz" % (split, key), build)


def _mnist_file(root, name):
    for d in (os.path.join(root, "MNIST", "raw"), root):
        for n in (name, name + ".gz"):
            if os.path.isfile(os.path.join(d, n)):
                return os.path.join(d, n)
    return None


def read_idx(path, magic, ndim):
    with (gzip.open if path.endswith(".gz") else open)(path, "rb") as f:
        raw = f.read()
    head = 4 + 4 * ndim
    if len(raw) < head:
        raise DataError("%s is too short for an IDX header" % path)
    (m,) = struct.unpack(">i", raw[:4])
    if m != magic:
        raise DataError("%s: magic number %d, expected %d" % (path, m, magic))
    dims = struct.unpack(">%di" % ndim, raw[4:head])
    body = np.frombuffer(raw, dtype=np.uint8, offset=head)
    if body.size != int(np.prod(dims)):
        raise DataError("%s holds %d data bytes, its header %s says %d" % (path, body.size, dims, int(np.prod(dims))))
    return body.reshape(dims)


def load_mnist(root, split, shape=(1, 28, 28), num_classes=10):
    """MNIST `train` / `test` as (uint8 [N,28,28,1], int64 [N]) straight from the IDX files (already uint8: no cache)."""
    fi, fl = (_mnist_file(root, n) for n in MNIST_FILES[split])
    if fi is None or fl is None:
        raise DataError("%s: no %s / %s (.gz) in %s/MNIST/raw or %s" % (root, MNIST_FILES[split][0], MNIST_FILES[split][1], root, root))
    images, labels = read_idx(fi, 2051, 3), read_idx(fl, 2049, 1)
    if images.shape[0] != labels.shape[0]:
        raise DataError("%s holds %d images, %s %d labels" % (fi, images.shape[0], fl, labels.shape[0]))
    if images.shape[1:] != tuple(shape[1:]):
        raise DataError("%s: images are %dx%d, expected %dx%d" % (fi, images.shape[1], images.shape[2], shape[1], shape[2]))
    if labels.size and int(labels.max()) >= num_classes:
        raise DataError("%s: label %d, expected < %d" % (fl, int(labels.max()), num_classes))
    return images.reshape(images.shape + (1,)).copy(), labels.astype(np.int64)


# ---- CIFAR-100 ----------------------------------------------------------------------------------------------------------------
def _cifar_dir(root):
    """<root>/cifar-100-python (torchvision's layout, what the archive unpacks to) when it exists, else <root> itself"""
    d = os.path.join(root, "cifar-100-python")
    return d if os.path.isdir(d) else root


def load_cifar100(root, split, shape=(3, 32, 32), num_classes=100):
    """CIFAR-100 `train` / `test` as (uint8 [N,32,32,3], int64 [N]) from the python pickle (torchvision's CIFAR100: encoding
    latin1, `data` [N,3072] planar CHW, `fine_labels`); transposed to HWC once, then read from the cache."""
    C, H, W = shape
    path = os.path.join(_cifar_dir(root), split)
    if not os.path.isfile(path):
        raise DataError("%s does not exist (expected %s)" % (path, LAYOUTS["cifar100"]))
    key = cache_key(root, ["cifar100", split, list(shape), num_classes], [path])

    def build():
        import pickle
        with open(path, "rb") as f:
            try:
                entry = pickle.load(f, encoding="latin1")
            except Exception as exc:
                raise DataError("%s is not a CIFAR-100 python pickle (%s)" % (path, exc))
        if not isinstance(entry, dict) or "data" not in entry or "fine_labels" not in entry:
            raise DataError("%s holds no `data` / `fine_labels` entries" % path)
        data, labels = np.asarray(entry["data"], dtype=np.uint8), np.asarray(entry["fine_labels"], dtype=np.int64)
        if data.ndim != 2 or data.shape[1] != C * H * W:
            raise DataError("%s: data is %s, expected [N,%d]" % (path, "x".join(str(d) for d in data.shape), C * H * W))
        if data.shape[0] != labels.shape[0]:
            raise DataError("%s holds %d images and %d fine labels" % (path, data.shape[0], labels.shape[0]))
        if not data.shape[0]:
            raise DataError("no images in %s" % path)
        if int(labels.min()) < 0 or int(labels.max()) >= num_classes:
            raise DataError("%s: fine label %d, expected 0 <= label < %d" % (path, int(labels.max() if labels.min() >= 0 else labels.min()), num_classes))
        return np.ascontiguousarray(data.reshape(-1, C, H, W).transpose(0, 2, 3, 1)), labels
    return cached(root, "cifar100-%s-%s.npz" % (split, key), build)


# RandomCrop(32, padding=4) + RandomHorizontalFlip() + RandomRotation(15) (utils/data_loader.py:30-36).  torchvision's rotate of a PIL
# image ends in img.rotate(angle, resample=NEAREST, expand=False, fillcolor=0): PIL/Image.py::rotate forms the inverse matrix in Python
# floats, and ImagingTransformAffine (Geometry.c, affine_fixed) walks it in 16.16 fixed point.  Both are restated here; the inner
# arithmetic is integer, so a batch is the PIL pipeline bit for bit.
AUG_IDENTITY = (65536, 0, 32768, 0, 65536, 32768)


def rotate_matrix(angle, w, h):
    """PIL's Image.rotate(angle) matrix (destination -> source) of a w x h image as six Python floats, or None where rotate()
    returns a copy (angle % 360 == 0)."""
    angle = float(angle) % 360.0
    if angle == 0:
        return None
    cx, cy = w / 2, h / 2
    angle = -math.radians(angle)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    x, y = -cx, -cy
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return m


def _fix(v):
    """Geometry.c's FIX: 16.16 fixed point, rounded half away from zero"""
    return int(v * 65536.0 + (-0.5 if v < 0 else 0.5))


def aug_coeffs(angles, H, W):
    """int32 [n,6]: the 16.16 fixed-point inverse map of Image.rotate(angle) on a W x H image for every angle (degrees), with the
    half-pixel offset of the pixel centres folded into the constant terms as affine_fixed does: output pixel (x, y) reads source
    pixel ((a2 + x a0 + y a1) >> 16, (a5 + x a3 + y a4) >> 16), or the fill where that lies outside the image."""
    out = np.empty((len(angles), 6), dtype=np.int32)
    for k, angle in enumerate(np.asarray(angles, dtype=np.float64).tolist()):
        m = rotate_matrix(angle, W, H)
        if m is None:
            out[k] = AUG_IDENTITY
        else:
            out[k] = (_fix(m[0]), _fix(m[1]), _fix(m[2] + m[0] * 0.5 + m[1] * 0.5), _fix(m[3]), _fix(m[4]), _fix(m[5] + m[3] * 0.5 + m[4] * 0.5))
    return out


# ---- ImageNet -----------------------------------------------------------------------------------------------------------------
def imagenet_listing(root, split, num_classes):
    """(classes, [(path, label)]) of ImageNet's `train` or `val` split: ImageFolder over <root>/<split>/<wnid>/**."""
    train = os.path.join(root, "train")
    if not os.path.isdir(train):
        raise DataError("%s does not exist" % train)
    classes = find_classes(train)
    if len(classes) != num_classes:
        raise DataError("%s holds %d class directories, expected %d" % (train, len(classes), num_classes))
    if split == "train":
        return classes, image_folder(train, classes)[1]
    val = os.path.join(root, "val")
    if not os.path.isdir(val):
        raise DataError("%s does not exist" % val)
    if find_classes(val) != classes:
        raise DataError("the class directories of %s differ from those of %s" % (val, train))
    return classes, image_folder(val, classes)[1]


def imagenet_short():
    """EEADV_IMAGENET_SHORT as an int (0 = off): the shorter side train images are shrunk to at decode."""
    v = os.environ.get("EEADV_IMAGENET_SHORT", "").strip()
    if not v:
        return 0
    if not v.isdigit() or int(v) < 1:
        raise DataError("EEADV_IMAGENET_SHORT=%s: expected a number of pixels >= 1" % v)
    return int(v)


def resized_size(w, h, short):
    """torchvision's Resize(short) on a w x h image: the shorter side becomes `short`, the longer int(short * long / short side)."""
    if w <= h:
        return short, int(short * h / w)
    return int(short * w / h), short


def center_crop_u8(a, S):
    """torchvision's CenterCrop(S) (transforms.functional.center_crop) on a uint8 [H, W, C] array: an image smaller than S along an axis
    is first padded with zeros there, (S - n) // 2 before and (S - n + 1) // 2 after - the odd pixel goes to the right / bottom -, then the
    window starts at int(round((n - S) / 2.0)) along each axis (Python's round: halves go to the even number)."""
    h, w = a.shape[:2]
    if S > w or S > h:
        pl, pt = ((S - w) // 2 if S > w else 0), ((S - h) // 2 if S > h else 0)
        pr, pb = ((S - w + 1) // 2 if S > w else 0), ((S - h + 1) // 2 if S > h else 0)
        a = np.pad(a, ((pt, pb), (pl, pr), (0, 0)))
        h, w = a.shape[:2]
    top, left = int(round((h - S) / 2.0)), int(round((w - S) / 2.0))
    return a[top:top + S, left:left + S]


def _decode_ragged(job):
    from PIL import Image
    paths, short = job[:2]
    img_size = job[2] if len(job) > 2 else 0
    out = []
    for p in paths:
        with open(p, "rb") as f:
            img = Image.open(f).convert("RGB")
        if img_size and min(img.size) != img_size:  # Resize(img_size): up and down
            img = img.resize(resized_size(img.size[0], img.size[1], img_size), Image.BILINEAR)
        if short and min(img.size) > short:
            img = img.resize(resized_size(img.size[0], img.size[1], short), Image.BILINEAR)
        out.append(np.asarray(img, dtype=np.uint8).reshape(img.size[1], img.size[0], 3))
    sizes = np.array([a.shape[:2] for a in out], dtype=np.int32).reshape(len(out), 2)
    return np.concatenate([a.reshape(-1) for a in out]) if out else np.empty(0, np.uint8), sizes


def _decode_val(job):
    from PIL import Image
    paths, S, resize = job[:3]
    out = np.empty((len(paths), S, S, 3), dtype=np.uint8)
    for i, p in enumerate(paths):
        with open(p, "rb") as f:
            img = Image.open(f).convert("RGB")
        if len(job) > 3:  # the fast-AT pipeline: [Resize(img_size)] + CenterCrop(S), which pads what is smaller than S
            if job[3] and min(img.size) != job[3]:
                img = img.resize(resized_size(img.size[0], img.size[1], job[3]), Image.BILINEAR)
            out[i] = center_crop_u8(np.asarray(img, dtype=np.uint8).reshape(img.size[1], img.size[0], 3), S)
            continue
        size = resized_size(img.size[0], img.size[1], resize)
        if size != img.size:
            img = img.resize(size, Image.BILINEAR)
        top, left = int(round((size[1] - S) / 2.0)), int(round((size[0] - S) / 2.0))  # torchvision's center_crop
        out[i] = np.asarray(img.crop((left, top, left + S, top + S)), dtype=np.uint8)
    return out


def _pool_map(fn, jobs):
    """fn over jobs in order, by up to 16 forked processes (the CPUs this process may run on, not the machine's)."""
    procs = min(16, len(os.sched_getaffinity(0)), len(jobs))
    if procs <= 1:
        return [fn(j) for j in jobs]
    with multiprocessing.get_context("fork").Pool(procs) as pool:  # the workers only run PIL + numpy, never the device
        return list(pool.imap(fn, jobs))


def load_imagenet(root, split, shape=(3, 224, 224), num_classes=1000, resize=256, img_size=None):
    """ImageNet `train` as the ragged (pixels uint8 [sum H*W*3], offsets int64 [N], sizes int32 [N,2] = (H, W), labels int64 [N]),
    `val` as (uint8 [N,S,S,3], int64 [N]) after Resize(resize) + CenterCrop(S); decoded once, then read from the cache.
    img_size (an int, the fast-AT pipeline of fgsm_imagenet/main_fast.py:136-160; `resize` is then unused): > 0 is Resize(img_size) at
    decode in both splits - the shorter side to img_size, PIL BILINEAR, up and down -, `val` is CenterCrop(S) of that or, with 0, of the
    file as it is (center_crop_u8: zero padding where the image is smaller).  img_size is part of the cache key."""
    C, S, S2 = shape
    if img_size is not None and (int(img_size) != img_size or img_size < 0):
        raise DataError("img_size must be an integer >= 0, got %r" % (img_size,))
    if C != 3 or S != S2 or (img_size is None and resize < S):
        raise DataError("ImageNet batches are 3 x S x S with S <= the resize size, got shape %s and resize %d" % (tuple(shape), resize))
    classes, samples = imagenet_listing(root, split, num_classes)
    if not samples:
        raise DataError("no images in the %s split of %s" % (split, root))
    paths = [p for p, _ in samples]
    labels = np.array([lab for _, lab in samples], dtype=np.int64)
    if split == "val":
        key = cache_key(root, ["imagenet", "val", list(shape), resize, classes] if img_size is None else
                        ["imagenet", "val", list(shape), "img_size", int(img_size), classes], paths)
        tail = () if img_size is None else (int(img_size),)

        def build_val():
            print("eeadv.data: decoding %d images of %s/val" % (len(paths), root))
            parts = _pool_map(_decode_val, [(paths[i:i + _CHUNK], S, resize) + tail for i in range(0, len(paths), _CHUNK)])
            return np.concatenate(parts), labels
        return cached(root, "imagenet-val-%s.npz" % key, build_val)
    short = imagenet_short()
    key = cache_key(root, ["imagenet", "train", short, classes] + (["img_size", int(img_size)] if img_size else []), paths)

    def build():
        print("eeadv.data: decoding %d images of %s/train%s" % (len(paths), root, " (shorter side <= %d)" % short if short else ""))
        parts = _pool_map(_decode_ragged, [(paths[i:i + _CHUNK], short, int(img_size or 0)) for i in range(0, len(paths), _CHUNK)])
        sizes = np.concatenate([s for _, s in parts])
        nbytes = sizes[:, 0].astype(np.int64) * sizes[:, 1] * 3
        offsets = np.concatenate([np.zeros(1, np.int64), np.cumsum(nbytes)[:-1]])
        return np.concatenate([p for p, _ in parts]), offsets, sizes, labels
    return cached(root, "imagenet-train-%s.npz" % key, build, keys=("pixels", "offsets", "sizes", "labels"))


# PIL's 8-bit resample (ImagingResample, BILINEAR): coefficients in double, then 22-bit fixed point
_PRECISION_BITS = 22


def resample_coeffs(n_in, n_out):
    """(xmin int64 [n_out], n int64 [n_out], k int64 [n_out, ksize]) of one axis: result pixel xx is
    clip8((2^21 + sum_{x < n[xx]} src[xmin[xx] + x] * k[xx, x]) >> 22); k is 0 at x >= n[xx]."""
    scale = float(n_in) / float(n_out)
    fs = max(scale, 1.0)
    support = fs
    ksize = int(np.ceil(support)) * 2 + 1
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(0, np.trunc(center - support + 0.5).astype(np.int64))
    n = np.minimum(n_in, np.trunc(center + support + 0.5).astype(np.int64)) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    w = np.maximum(0.0, 1.0 - np.abs(((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) / fs))
    w[x >= n[:, None]] = 0.0
    ww = np.zeros(n_out, dtype=np.float64)
    for j in range(ksize):  # the sum in ascending x, as PIL forms it
        ww = ww + w[:, j]
    w = w / ww[:, None]
    return xmin, n, np.trunc(0.5 + w * float(1 << _PRECISION_BITS)).astype(np.int64)


def _resample_axis1(a, n_out):
    """a uint8 [R, n_in, C] -> uint8 [R, n_out, C] along axis 1."""
    xmin, _, k = resample_coeffs(a.shape[1], n_out)
    acc = np.full((a.shape[0], n_out, a.shape[2]), 1 << (_PRECISION_BITS - 1), dtype=np.int64)
    for j in range(k.shape[1]):
        acc += a[:, np.minimum(xmin + j, a.shape[1] - 1), :].astype(np.int64) * k[None, :, j, None]
    return np.clip(acc >> _PRECISION_BITS, 0, 255).astype(np.uint8)


def resample_u8(img, out_h, out_w):
    """PIL's Image.resize((out_w, out_h), BILINEAR) of a uint8 [H,W,C] array, byte for byte: the horizontal pass to uint8, then
    the vertical pass over that.

    The one exception, stated here for the kernel and the documents too: Image.resize takes the vertical pass first when the image
    (here: the crop) has H > 100 W and out_h < H.  At W = 1 the horizontal pass copies its single pixel (one coefficient, 2^22), so
    the order cannot change a byte; at W >= 2 some bytes then differ by one.  So the bytes are PIL's except for H > 100 W with
    W >= 2 and out_h < H.  RandomResizedCrop's ratio range [3/4, 4/3] never draws such a crop, and the kernel keeps this order."""
    tmp = _resample_axis1(np.ascontiguousarray(img), out_w)
    return _resample_axis1(tmp.transpose(1, 0, 2), out_h).transpose(1, 0, 2)


def rrc_boxes(sizes, generator, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """torchvision's RandomResizedCrop.get_params for every image of `sizes` [N,2] = (H, W) at once -> int32 [N,4] = (top, left,
    h, w): up to 10 tries of area * U(scale) and exp(U(log ratio)), w = round(sqrt(a * r)), h = round(sqrt(a / r)), the first
    try with 0 < w <= W and 0 < h <= H at a uniform integer position; otherwise the central crop with the ratio clamped."""
    sizes = torch.as_tensor(np.asarray(sizes)).to(torch.int64).reshape(-1, 2)
    n = sizes.shape[0]
    H, W = sizes[:, 0], sizes[:, 1]
    area = (H * W).double()[:, None]
    target = area * (scale[0] + (scale[1] - scale[0]) * torch.rand(n, 10, dtype=torch.float64, generator=generator))
    lo, hi = np.log(ratio[0]), np.log(ratio[1])
    aspect = torch.exp(lo + (hi - lo) * torch.rand(n, 10, dtype=torch.float64, generator=generator))
    w = torch.round(torch.sqrt(target * aspect)).to(torch.int64)  # round half to even, as Python's round()
    h = torch.round(torch.sqrt(target / aspect)).to(torch.int64)
    ok = (w > 0) & (w <= W[:, None]) & (h > 0) & (h <= H[:, None])
    first = torch.argmax(ok.to(torch.int8), dim=1, keepdim=True)
    found = ok.any(dim=1)
    w, h = w.gather(1, first)[:, 0], h.gather(1, first)[:, 0]
    u = torch.rand(n, 2, dtype=torch.float64, generator=generator)
    top = torch.minimum((u[:, 0] * (H - h + 1).double()).to(torch.int64), H - h)
    left = torch.minimum((u[:, 1] * (W - w + 1).double()).to(torch.int64), W - w)
    in_ratio = W.double() / H.double()
    fw = torch.where(in_ratio > ratio[1], torch.round(H.double() * ratio[1]).to(torch.int64), W)
    fh = torch.where(in_ratio < ratio[0], torch.round(W.double() / ratio[0]).to(torch.int64), H)
    box = torch.where(found[:, None], torch.stack([top, left, h, w], 1), torch.stack([(H - fh) // 2, (W - fw) // 2, fh, fw], 1))
    return box.to(torch.int32)


# ---- batches ------------------------------------------------------------------------------------------------------------------
def host_batch(images, labels, ids, flip):
    """The batch on the host with torch ops: what ee_batch_u8_f32 computes (and --no-cuda runs)."""
    x = images[ids].permute(0, 3, 1, 2).float().div(255).clone(memory_format=torch.contiguous_format)  # NCHW strides also at C = 1
    if flip is not None:
        f = flip[ids].bool()
        x[f] = x[f].flip(-1)
    return x, labels[ids]


def host_batch_rrc(pixels, offsets, sizes, labels, ids, boxes, flip, S):
    """The ImageNet train batch on the host: what ee_batch_rrc_u8_f32 computes (and --no-cuda runs).  pixels uint8 [bytes],
    offsets int64 [N], sizes int32 [N,2], labels int64 [N], ids int64 [B], boxes int32 [N,4], flip bool / uint8 [N] or None."""
    pix = pixels.numpy()
    x = torch.empty((len(ids), 3, S, S), dtype=torch.float32)
    for b, s in enumerate(ids.tolist()):
        H, W = sizes[s].tolist()
        top, left, h, w = boxes[s].tolist()
        img = pix[int(offsets[s]):int(offsets[s]) + H * W * 3].reshape(H, W, 3)
        r = torch.from_numpy(resample_u8(img[top:top + h, left:left + w], S, S))
        if flip is not None and bool(flip[s]):
            r = r.flip(1)
        x[b] = r.permute(2, 0, 1).float().div(255)
    return x, labels[ids]


def host_batch_aug(images, labels, ids, offs, flip, coef, pad):
    """The CIFAR train batch on the host: what ee_batch_aug_u8_f32 computes (and --no-cuda runs).  images uint8 [N,H,W,C], labels
    int64 [N]; per batch position: ids int64 [B], offs int32 [B,2] = the crop's (top, left) in the image zero-padded by `pad`, flip
    bool / uint8 [B], coef int32 [B,6] (aug_coeffs).  The inverse maps are composed in the transform order crop, flip, rotate: output
    pixel -> rotation source in the crop's frame -> un-mirrored column -> image pixel = crop offset - pad; outside the rotated frame
    or outside the image gives 0."""
    img = images.numpy()
    N, H, W, C = img.shape
    B = len(ids)
    idn, o, f, a = np.asarray(ids, dtype=np.int64), np.asarray(offs, dtype=np.int64).reshape(B, 2), np.asarray(flip).astype(bool).reshape(B), \
        np.asarray(coef, dtype=np.int64).reshape(B, 6)
    if B and (idn.min() < 0 or idn.max() >= N or o.min() < 0 or o.max() > 2 * pad):
        raise ValueError("host_batch_aug: a sample id outside [0, %d) or a crop offset outside [0, %d]" % (N, 2 * pad))
    y, x = np.arange(H, dtype=np.int64)[None, :, None], np.arange(W, dtype=np.int64)[None, None, :]
    a = a[:, :, None, None]
    xin = (a[:, 2] + x * a[:, 0] + y * a[:, 1]) >> 16
    yin = (a[:, 5] + x * a[:, 3] + y * a[:, 4]) >> 16
    ok = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    xs = np.where(f[:, None, None], W - 1 - xin, xin) + o[:, 1, None, None] - pad
    ys = yin + o[:, 0, None, None] - pad
    ok &= (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
    u8 = img[idn[:, None, None], np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)] * ok[..., None].astype(np.uint8)  # [B,H,W,C]
    xb = torch.from_numpy(u8).permute(0, 3, 1, 2).float().div(255).clone(memory_format=torch.contiguous_format)
    return xb, labels[torch.as_tensor(idn)]


class DeviceLoader:
    """One split held on `device`; len() batches of `batch_size` (the last one may be partial), iterating yields (x f32
    [B,C,H,W], y int64 [B]) already on the device - as driver.SyntheticLoader.

    `load()` -> (uint8 [N,H,W,C], int64 [N]) runs on the first len() / iteration (--evaluate never decodes the train split).
    Per epoch the order and the flip flags are drawn on the host from torch.Generator(seed + epoch), the same on every rank
    (DistributedSampler's seeding), and uploaded once; this rank takes the positions ddp.shard_indices gives it (strided,
    padded by wrap-around).  The flags are indexed by sample id, so a sample's flip does not depend on world size."""

    def __init__(self, load, batch_size, device, seed, shuffle, flip, rank=None, world=None):
        self._load, self.batch_size, self.device, self.seed = load, int(batch_size), torch.device(device), int(seed)
        self.shuffle, self.flip = shuffle, flip
        self.rank = ddp.rank() if rank is None else rank
        self.world = ddp.world() if world is None else world
        self.epoch = 0
        self._split = None

    def _ready(self):
        if self._split is None:
            images, labels = self._load()
            images, labels = torch.from_numpy(np.ascontiguousarray(images)), torch.from_numpy(np.ascontiguousarray(labels))
            self.n = images.shape[0]
            self.positions = torch.tensor(ddp.shard_indices(self.n, self.rank, self.world), dtype=torch.int64)
            if self.device.type == "cuda":
                images, labels, self.lut = images.to(self.device), labels.to(self.device), LUT.to(self.device)
            self._split = (images, labels)
        return self._split

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        self._ready()
        return (len(self.positions) + self.batch_size - 1) // self.batch_size

    def epoch_order(self):
        """(sample ids of this rank in batch order, int64; per-sample flip flags [N] bool or None), on the host."""
        self._ready()
        g = torch.Generator().manual_seed(self.seed + self.epoch)
        perm = torch.randperm(self.n, generator=g) if self.shuffle else torch.arange(self.n)
        flip = (torch.rand(self.n, generator=g) < 0.5) if self.flip else None
        return perm[self.positions], flip

    def __iter__(self):
        images, labels = self._ready()
        ids, flip = self.epoch_order()
        B = self.batch_size
        if self.device.type != "cuda":
            for k in range(0, ids.numel(), B):
                yield host_batch(images, labels, ids[k:k + B], flip)
            return
        from . import ops
        ids = ids.to(torch.int32).to(self.device)  # the epoch's only host -> device copies
        flip = None if flip is None else flip.to(torch.uint8).to(self.device)
        for k in range(0, ids.numel(), B):
            yield ops.batch_u8(images, labels, ids[k:k + B], flip, self.lut)


HBM_RESERVE = 16 << 30  # bytes of device memory left to the model, its activations and the attack next to a resident split


def check_hbm(nbytes, device, what):
    """DataError when `nbytes` of `what` do not fit in the free memory of `device` minus HBM_RESERVE."""
    free, total = torch.cuda.mem_get_info(device)
    if nbytes > free - HBM_RESERVE:
        raise DataError("%s is %.1f GB as uint8; the device has %.1f of %.1f GB free and %.1f GB are kept for the model: set "
                        "EEADV_IMAGENET_SHORT=<pixels> (e.g. 160) to shrink the images at decode, so that the split fits"
                        % (what, nbytes / 1e9, free / 1e9, total / 1e9, HBM_RESERVE / 1e9))


class RaggedDeviceLoader(DeviceLoader):
    """DeviceLoader over a split of images of different sizes (ImageNet train): `load()` -> (pixels, offsets, sizes, labels),
    every batch is RandomResizedCrop(S) + flip by ONE launch of ee_batch_rrc_u8_f32.  The boxes are drawn per epoch for the whole
    split after the order and the flips, from the same generator, indexed by sample id like the flips."""

    def __init__(self, load, S, batch_size, device, seed, rank=None, world=None, what="the train split"):
        super().__init__(load, batch_size, device, seed, shuffle=True, flip=True, rank=rank, world=world)
        self.S, self.what = int(S), what

    def _ready(self):
        if self._split is None:
            split = [torch.from_numpy(np.ascontiguousarray(a)) for a in self._load()]
            self.n = split[1].shape[0]
            self.positions = torch.tensor(ddp.shard_indices(self.n, self.rank, self.world), dtype=torch.int64)
            self.sizes_host = split[2]
            if self.device.type == "cuda":
                check_hbm(split[0].numel(), self.device, self.what)
                split, self.lut = [a.to(self.device) for a in split], LUT.to(self.device)
            self._split = tuple(split)
        return self._split

    def epoch_draws(self):
        """(sample ids of this rank in batch order, flip flags [N] bool, boxes int32 [N,4]) of this epoch, on the host."""
        self._ready()
        g = torch.Generator().manual_seed(self.seed + self.epoch)
        perm = torch.randperm(self.n, generator=g)
        flip = torch.rand(self.n, generator=g) < 0.5
        return perm[self.positions], flip, rrc_boxes(self.sizes_host, g)

    def __iter__(self):
        pixels, offsets, sizes, labels = self._ready()
        ids, flip, boxes = self.epoch_draws()
        B = self.batch_size
        if self.device.type != "cuda":
            for k in range(0, ids.numel(), B):
                yield host_batch_rrc(pixels, offsets, sizes, labels, ids[k:k + B], boxes, flip, self.S)
            return
        from . import ops
        ids = ids.to(torch.int32).to(self.device)  # the epoch's only host -> device copies
        flip, boxes = flip.to(torch.uint8).to(self.device), boxes.to(self.device)
        for k in range(0, ids.numel(), B):
            yield ops.batch_rrc(pixels, offsets, sizes, labels, ids[k:k + B], boxes, flip, self.lut, self.S)


class AugDeviceLoader(DeviceLoader):
    """DeviceLoader whose every batch is RandomCrop(H, padding=pad) + RandomHorizontalFlip + RandomRotation(degrees) by ONE launch of
    ee_batch_aug_u8_f32 (CIFAR-100 train).  Per epoch the order, the flips, the crop offsets (uniform integers in [0, 2 pad], as
    RandomCrop.get_params) and the angles (uniform in [-degrees, degrees], as RandomRotation.get_params) are drawn on the host for
    the whole split from torch.Generator(seed + epoch), indexed by sample id like the flips; the angles become the 16.16 fixed-point
    matrices of aug_coeffs there, and this rank's draws go to the device once, in batch order."""

    def __init__(self, load, batch_size, device, seed, pad=4, degrees=15.0, rank=None, world=None):
        super().__init__(load, batch_size, device, seed, shuffle=True, flip=True, rank=rank, world=world)
        self.pad, self.degrees = int(pad), float(degrees)

    def epoch_draws(self):
        """(sample ids of this rank in batch order int64, flip flags [N] bool, crop offsets int32 [N,2] = (top, left), angles float64
        [N] in degrees) of this epoch, on the host."""
        self._ready()
        g = torch.Generator().manual_seed(self.seed + self.epoch)
        perm = torch.randperm(self.n, generator=g)
        flip = torch.rand(self.n, generator=g) < 0.5
        offs = torch.randint(0, 2 * self.pad + 1, (self.n, 2), generator=g, dtype=torch.int32)
        angles = (torch.rand(self.n, dtype=torch.float64, generator=g) * 2.0 - 1.0) * self.degrees
        return perm[self.positions], flip, offs, angles

    def __iter__(self):
        images, labels = self._ready()
        ids, flip, offs, angles = self.epoch_draws()
        H, W = images.shape[1], images.shape[2]
        # this rank's draws in batch order
        offs, flip = offs[ids].contiguous(), flip[ids].to(torch.uint8)
        coef = torch.from_numpy(aug_coeffs(angles[ids].numpy(), H, W))
        B = self.batch_size
        if self.device.type != "cuda":
            for k in range(0, ids.numel(), B):
                yield host_batch_aug(images, labels, ids[k:k + B], offs[k:k + B], flip[k:k + B], coef[k:k + B], self.pad)
            return
        from . import ops
        ids = ids.to(torch.int32)
        d_ids, d_offs, d_flip, d_coef = (t.to(self.device) for t in (ids, offs, flip, coef))  # the epoch's only host -> device copies
        for k in range(0, ids.numel(), B):
            yield ops.batch_aug(images, labels, d_ids[k:k + B], d_offs[k:k + B], d_flip[k:k + B], d_coef[k:k + B], self.lut,
                                ids[k:k + B], offs[k:k + B], self.pad)


def make_loaders(kind, root, spec, device, batch_size, seed):
    """(train, val) loaders of a `kind` directory, with the reference's shuffle / flip (/ crop) per split."""
    root = os.path.abspath(root)
    shape, k = tuple(spec["shape"]), spec["num_classes"]
    if kind == "tiny_imagenet":
        return (DeviceLoader(lambda: load_tiny_imagenet(root, "train", shape, k), batch_size, device, seed, shuffle=True, flip=True),
                DeviceLoader(lambda: load_tiny_imagenet(root, "val", shape, k), batch_size, device, seed, shuffle=False, flip=False))
    if kind == "mnist":
        return (DeviceLoader(lambda: load_mnist(root, "train", shape, k), batch_size, device, seed, shuffle=True, flip=False),
                DeviceLoader(lambda: load_mnist(root, "test", shape, k), batch_size, device, seed, shuffle=True, flip=False))
    if kind == "imagenet":
        resize, img_size = int(spec.get("resize", 256)), spec.get("img_size")  # img_size: the fast-AT pipeline (load_imagenet)
        return (RaggedDeviceLoader(lambda: load_imagenet(root, "train", shape, k, resize, img_size), shape[-1], batch_size, device, seed,
                                   what="the train split of %s" % root),
                DeviceLoader(lambda: load_imagenet(root, "val", shape, k, resize, img_size), batch_size, device, seed, shuffle=False,
                             flip=False))
    if kind == "cifar100":
        return (AugDeviceLoader(lambda: load_cifar100(root, "train", shape, k), batch_size, device, seed, pad=int(spec.get("pad", 4)),
                                degrees=float(spec.get("degrees", 15.0))),
                DeviceLoader(lambda: load_cifar100(root, "test", shape, k), batch_size, device, seed, shuffle=False, flip=False))
    raise ValueError("unknown dataset kind %r" % (kind,))
