#!/usr/bin/env python
"""Writes tests/golden/fd_denoise.npz and tests/golden/fd_keys.npz from the reference's own ImageNet/models_imagenet/resnet_fd.py.

    python scripts/gen_fd_golden.py <reference checkout>

The reference file is loaded by path, here and only here; the fixtures hold data alone (float64 arrays, names, shapes):
  fd_denoise.npz  for denoising(8, 3, 5) (n_in <= H * W: the channel form) and denoising(32, 3, 5) (n_in > H * W: the spatial form), both
                  embed=False, softmax=False, in float64 and train mode: the input, conv3's weight and bias, the BatchNorm's weight and bias
                  (moved off 1 / 0), the upstream gradient, the output and the input gradient;
  fd_keys.npz     the ordered state_dict keys and shapes of resnet18_fd and resnet50_fd.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = {"channel": (8, 3, 5), "spatial": (32, 3, 5)}


def load_reference(ref_root):
    path = os.path.join(ref_root, "ImageNet", "models_imagenet", "resnet_fd.py")
    spec = importlib.util.spec_from_file_location("reference_resnet_fd", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(ref_root):
    ref = load_reference(ref_root)
    out = {}
    for tag, (n_in, H, W) in CASES.items():
        torch.manual_seed(1000 + n_in)
        blk = ref.denoising(n_in=n_in, H=H, W=W, embed=False, softmax=False).double().train()
        with torch.no_grad():
            blk.bn.weight.uniform_(0.5, 1.5)
            blk.bn.bias.normal_(0, 0.2)
        x = torch.randn(3, n_in, H, W, dtype=torch.float64, requires_grad=True)
        dy = torch.randn(3, n_in, H, W, dtype=torch.float64)
        y = blk(x)
        (dx,) = torch.autograd.grad(y, x, dy)
        for k, v in (("x", x), ("dy", dy), ("y", y), ("dx", dx), ("conv3_weight", blk.conv3.weight), ("conv3_bias", blk.conv3.bias),
                     ("bn_weight", blk.bn.weight), ("bn_bias", blk.bn.bias)):
            out["%s_%s" % (tag, k)] = v.detach().numpy().copy()
        out["%s_dims" % tag] = np.array([n_in, H, W], dtype=np.int64)
    np.savez_compressed(os.path.join(GOLDEN, "fd_denoise.npz"), **out)
    keys = {}
    for name in ("resnet18_fd", "resnet50_fd"):
        sd = getattr(ref, name)().state_dict()
        keys[name + "_keys"] = np.array(list(sd.keys()))
        keys[name + "_shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
    np.savez_compressed(os.path.join(GOLDEN, "fd_keys.npz"), **keys)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
