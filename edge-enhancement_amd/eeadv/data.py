"""Real Tiny-ImageNet and MNIST for the drivers, held whole in device memory.

The reference (utils/data_loader.py) reads both with torchvision: ImageFolder + PIL + RandomHorizontalFlip (Tiny train) +
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

Not kept: the images must already be H x W (the reference has no resize either; a different size is an error naming the file).
"""
import gzip
import hashlib
import json
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
    if kind == "tiny_imagenet":
        return os.path.isdir(os.path.join(root, "train")) and os.path.isdir(os.path.join(root, "val"))
    if kind == "mnist":
        return all(_mnist_file(root, n) for pair in MNIST_FILES.values() for n in pair)
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


def cached(root, name, build):
    """(images, labels) from <cache_dir(root)>/<name>, or build() them and publish the file atomically (temporary name +
    os.replace: concurrent ranks at worst decode twice, none reads a half-written file).  An unwritable cache directory
    leaves the split decoded in memory only."""
    d = cache_dir(root)
    path = os.path.join(d, name)
    if os.path.isfile(path):
        with np.load(path) as z:
            return z["images"], z["labels"]
    images, labels = build()
    tmp = "%s.%d.tmp" % (path, os.getpid())
    try:
        os.makedirs(d, exist_ok=True)
        with open(tmp, "wb") as f:
            np.savez(f, images=images, labels=labels)
        os.replace(tmp, path)
    except OSError as exc:
        print("eeadv.data: cache directory %s is not writable (%s): %s is decoded in memory only" % (d, exc.strerror or exc, name))
        try:
            os.remove(tmp)
        except OSError:
            pass
    return images, labels


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


# ---- batches ------------------------------------------------------------------------------------------------------------------
def host_batch(images, labels, ids, flip):
    """The batch on the host with torch ops: what ee_batch_u8_f32 computes (and --no-cuda runs)."""
    x = images[ids].permute(0, 3, 1, 2).float().div(255).clone(memory_format=torch.contiguous_format)  # NCHW strides also at C = 1
    if flip is not None:
        f = flip[ids].bool()
        x[f] = x[f].flip(-1)
    return x, labels[ids]


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


def make_loaders(kind, root, spec, device, batch_size, seed):
    """(train, val) DeviceLoaders of a `kind` directory, with the reference's shuffle / flip per split."""
    root = os.path.abspath(root)
    shape, k = tuple(spec["shape"]), spec["num_classes"]
    if kind == "tiny_imagenet":
        return (DeviceLoader(lambda: load_tiny_imagenet(root, "train", shape, k), batch_size, device, seed, shuffle=True, flip=True),
                DeviceLoader(lambda: load_tiny_imagenet(root, "val", shape, k), batch_size, device, seed, shuffle=False, flip=False))
    if kind == "mnist":
        return (DeviceLoader(lambda: load_mnist(root, "train", shape, k), batch_size, device, seed, shuffle=True, flip=False),
                DeviceLoader(lambda: load_mnist(root, "test", shape, k), batch_size, device, seed, shuffle=True, flip=False))
    raise ValueError("unknown dataset kind %r" % (kind,))
