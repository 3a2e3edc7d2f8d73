#!/usr/bin/env python
# -*- encoding: utf-8 -*-
"""ImageNet DDP driver (reference: ImageNet/experiments_imagenet.py): one process per GPU over RCCL, SyncBatchNorm,
per-rank batch = batch_size / world, seeds seed + rank, 30-epoch step LR.

    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 experiments_imagenet.py \
        -c configs_imagenet/ee_at_bpda3_square.yml

--data DIR reads <DIR>/train/<wnid>/** and <DIR>/val/<wnid>/** (eeadv.data: RandomResizedCrop + flip for train on the device,
Resize + CenterCrop for val).  The optional YAML keys num_classes, crop_size (a multiple of 32) and resize_size shrink the
problem for subsets and tests; absent, they are the reference's 1000, 224 and 256.
"""
import os
import sys

sys.path.append(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch.nn as nn  # noqa: E402

import models_imagenet as zoo  # noqa: E402
from eeadv import driver  # noqa: E402

SPEC = {"description": "PyTorch ImageNet Training", "ckpt_dir": "checkpoint_ImageNet", "shape": (3, 224, 224), "num_classes": 1000,
        "ddp": True, "sync_bn": True, "lr_schedule": "step30", "data": "imagenet", "resize": 256,
        "yaml_sizes": ("num_classes", "crop_size", "resize_size")}


def build_model(args):
    """experiments_imagenet.py:66-122."""
    model = _build(args, num_classes=args.num_classes)
    if args.crop_size != 224:  # the reference's AvgPool2d(7) is the global pool of a 224 x 224 input: keep it global
        if args.crop_size % 32 != 0:
            raise ValueError("crop_size %d: the ImageNet ResNets need a multiple of 32" % args.crop_size)
        model.avgpool = nn.AvgPool2d(args.crop_size // 32, stride=1)
    return model


def _build(args, **size):
    arch = args.arch
    if arch in ('resnet18', 'resnet34', 'resnet50', 'resnet101', 'resnet152'):
        return getattr(zoo, arch)(pretrained=args.pretrained, **size)
    if arch in ('resnet18_fd', 'resnet34_fd', 'resnet50_fd', 'resnet101_fd', 'resnet152_fd'):  # experiments_imagenet.py:110-119
        return getattr(zoo, arch)(pretrained=args.pretrained, size=args.crop_size, **size)
    ee = dict(pretrained=args.pretrained, cize=args.cize, r=args.r, w=args.w, with_gf=args.gf, low=args.low, high=args.high,
              alpha=args.alpha, sigma=args.sigma, type_canny=args.type_canny if args.type_canny not in (None, "None") else 'CannyFilter', **size)
    if arch.endswith('_EE_square'):
        return getattr(zoo, arch)(epsilon=args.epsilon, n_queries=args.n_queries, **ee)
    if arch.endswith('_EE'):
        return getattr(zoo, arch)(**ee)
    raise NotImplementedError


if __name__ == '__main__':
    driver.run(SPEC, build_model)
