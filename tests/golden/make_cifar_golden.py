#!/usr/bin/env python3
"""Write tests/golden/cifar_preact.npz from the REFERENCE's own AWP/Cifar100/models_cifar100_awp/preactresnet.py (loaded as a plain
file, as make_preact_golden.py loads the Tiny one; it needs only torch).  Data only, for PreActResNet18(dataset="CIFAR100") after
torch.manual_seed(k), a fixed B = 4 input of 3 x 32 x 32 and labels, on one CPU thread, in train and in eval mode: the logits, the
input gradient of the (mean) cross-entropy, the running statistics after the train-mode forward, and the gradient of one parameter
of every layer (PARAMS).

The 11 M weights are 45 MB and a committed file may hold 1 MiB: as in preact.npz they are recorded as the seed that reproduces them
plus every state-dict entry's name, shape and float64 sum.  For the same reason a parameter gradient larger than SAMPLE entries is
recorded as flat[::stride] with stride = ceil(numel / SAMPLE) (tests take the same slice of theirs), next to its 2-norm.

    python tests/golden/make_cifar_golden.py /path/to/reference
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REF = sys.argv[1] if len(sys.argv) > 1 else sys.exit(__doc__)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cifar_preact.npz")
SEED = 7
SAMPLE = 2048
PARAMS = (["conv1.weight"] + ["layer%d.0.conv1.weight" % i for i in (1, 2, 3, 4)] + ["layer%d.1.conv2.weight" % i for i in (1, 2, 3, 4)] +
          ["layer%d.0.shortcut.0.weight" % i for i in (2, 3, 4)] + ["layer%d.0.bn1.weight" % i for i in (1, 2, 3, 4)] +
          ["layer%d.1.bn2.bias" % i for i in (1, 2, 3, 4)] + ["bn.weight", "bn.bias", "linear.weight", "linear.bias"])


def sample(a):
    flat = np.asarray(a).reshape(-1)
    return flat[::-(-flat.size // SAMPLE)]


def main():
    torch.set_num_threads(1)
    spec = importlib.util.spec_from_file_location("ref_cifar_preactresnet", os.path.join(REF, "AWP", "Cifar100", "models_cifar100_awp", "preactresnet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(SEED)
    net = mod.PreActResNet18(dataset="CIFAR100")
    sd = net.state_dict()
    out = dict(seed=np.array(SEED), sample=np.array(SAMPLE), names=np.array(list(sd.keys())),
               shapes=np.array([",".join(str(d) for d in v.shape) for v in sd.values()]),
               checksum=np.array([v.numpy().astype(np.float64).sum() for v in sd.values()]), params=np.array(PARAMS))
    g = torch.Generator().manual_seed(11)
    x = torch.rand(4, 3, 32, 32, generator=g)
    y = torch.randint(0, 100, (4,), generator=g)
    out["x"], out["y"] = x.numpy(), y.numpy()
    for mode in ("train", "eval"):
        net.train(mode == "train")
        net.zero_grad()
        xr = x.clone().requires_grad_(True)
        logits = net(xr)
        F.cross_entropy(logits, y).backward()
        out["logits_" + mode], out["grad_x_" + mode] = logits.detach().numpy().copy(), xr.grad.numpy().copy()
        named = dict(net.named_parameters())
        for k in PARAMS:
            out["g_%s_%s" % (mode, k)] = sample(named[k].grad.numpy()).copy()
        out["gnorm_" + mode] = np.array([float(np.linalg.norm(named[k].grad.numpy().astype(np.float64))) for k in PARAMS])
        if mode == "train":
            stats = {k: v.numpy().copy() for k, v in net.state_dict().items() if "running_" in k}
            out["stat_names"], out["stats"] = np.array(list(stats.keys())), np.concatenate([v.reshape(-1) for v in stats.values()])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
