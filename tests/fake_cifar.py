"""A small fake CIFAR-100 tree for the eeadv.data tests: the two python pickles of torchvision's layout, written with the entries the
real archive has (`data` uint8 [N,3072] planar CHW, `fine_labels`, `coarse_labels`, `filenames`, `batch_label`).  Nothing here is a real
dataset; every pixel comes from a seeded generator."""
import os
import pickle

import numpy as np


def cifar_tree(root, n_train=40, n_test=24, seed=0, subdir="cifar-100-python"):
    """<root>/<subdir>/{train,test}.  Returns {split: (images uint8 [N,32,32,3] HWC, fine labels int64 [N])}."""
    rng = np.random.default_rng(seed)
    d = os.path.join(str(root), subdir) if subdir else str(root)
    os.makedirs(d, exist_ok=True)
    out = {}
    for split, n in (("train", n_train), ("test", n_test)):
        chw = rng.integers(0, 256, (n, 3, 32, 32), dtype=np.uint8)
        fine = rng.integers(0, 100, (n,)).tolist()
        entry = {"data": chw.reshape(n, 3072), "fine_labels": fine, "coarse_labels": [f // 5 for f in fine],
                 "filenames": ["img_%05d.png" % k for k in range(n)], "batch_label": "%sing batch 1 of 1" % split}
        with open(os.path.join(d, split), "wb") as f:
            pickle.dump(entry, f, protocol=2)
        out[split] = (np.ascontiguousarray(chw.transpose(0, 2, 3, 1)), np.array(fine, dtype=np.int64))
    return out


def aug_draws(n_items, n_samples, pad, seed):
    """Seeded draws for the augmentation tests, per batch position: (ids int64 [n], offs int32 [n,2], flip uint8 [n], angles float64
    [n]).  The first positions hold the special cases: angles 0.0, +-15.0, +-1e-6 and 360.0, crop corners (0, 0) and (2 pad, 2 pad),
    both flip values; the rest are uniform."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, n_samples, n_items).astype(np.int64)
    offs = rng.integers(0, 2 * pad + 1, (n_items, 2)).astype(np.int32)
    flip = rng.integers(0, 2, n_items).astype(np.uint8)
    angles = rng.uniform(-15.0, 15.0, n_items)
    special = [0.0, 15.0, -15.0, 1e-6, -1e-6, 360.0, 0.0, -15.0]
    for k, a in enumerate(special[:n_items]):
        angles[k] = a
        offs[k] = (0, 0) if k % 2 == 0 else (2 * pad, 2 * pad)
        flip[k] = (k // 2) % 2
    return ids, offs, flip, angles
