#!/usr/bin/env python3
"""Write tests/golden/preact.npz from the REFERENCE's own AWP/Tiny_imagenet/models_tiny_awp/preactresnet.py (loaded as a plain file,
as make_golden.py loads resnet.py; it needs only torch).  Data only: the state-dict names and shapes, a weight checksum after
torch.manual_seed(k), and for a fixed B = 2 input on one CPU thread: train-mode logits, the running statistics after that forward,
eval-mode logits and the input gradient of the summed train-mode logits.

    python tests/golden/make_preact_golden.py [/path/to/reference]
"""
import importlib.util
import os
import sys

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "preact.npz")
SEED = 7


def main():
    torch.set_num_threads(1)
    spec = importlib.util.spec_from_file_location("ref_preactresnet", os.path.join(REF, "AWP", "Tiny_imagenet", "models_tiny_awp", "preactresnet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(SEED)
    net = mod.PreActResNet18(dataset="Tiny-ImageNet")
    sd = net.state_dict()
    names = np.array(list(sd.keys()))
    shapes = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
    checksum = np.array([v.numpy().astype(np.float64).sum() for v in sd.values()])
    g = torch.Generator().manual_seed(11)
    x = torch.rand(2, 3, 64, 64, generator=g)
    net.train()
    xr = x.clone().requires_grad_(True)
    logits_train = net(xr)
    logits_train.sum().backward()
    stats = {k: v.numpy().copy() for k, v in net.state_dict().items() if "running_" in k}
    net.eval()
    with torch.no_grad():
        logits_eval = net(x)
    np.savez_compressed(OUT, seed=np.array(SEED), names=names, shapes=shapes, checksum=checksum, x=x.numpy(),
                        logits_train=logits_train.detach().numpy(), logits_eval=logits_eval.numpy(), grad_x=xr.grad.numpy(),
                        stat_names=np.array(list(stats.keys())), stats=np.concatenate([v.reshape(-1) for v in stats.values()]))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
