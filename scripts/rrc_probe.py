"""ee_batch_rrc_u8_f32 at the ImageNet batch: B = 256, S = 224, 512 random images around 500 x 375 (half of them 375 x 500 or
500 x 375, the rest 333-500 on each side) with RandomResizedCrop boxes and flips; 23 launches, the torch-event time of 20 of them,
a check of 4 samples against the host restatement, and 3 launches of ee_batch_u8_f32 at the same output size for scale.

    rocprofv3 --kernel-trace --stats -- python scripts/rrc_probe.py      (profiles/imagenet_data_kernel.txt)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "edge-enhancement_amd")]
import numpy as np
import torch

from eeadv import data as D, ops
rng = np.random.default_rng(0)
N = 512
sizes = np.stack([rng.integers(333, 501, N), rng.integers(333, 501, N)], 1).astype(np.int32)
sizes[::2] = (375, 500)
sizes[1::4] = (500, 375)
nbytes = sizes[:, 0].astype(np.int64) * sizes[:, 1] * 3
offsets = np.concatenate([np.zeros(1, np.int64), np.cumsum(nbytes)[:-1]])
pixels = rng.integers(0, 256, int(nbytes.sum()), dtype=np.uint8)
dev = "cuda:0"
g = torch.Generator().manual_seed(0)
boxes = D.rrc_boxes(sizes, g)
flip = (torch.rand(N, generator=g) < 0.5).to(torch.uint8)
t = [torch.from_numpy(a).to(dev) for a in (pixels, offsets, sizes)] + [torch.arange(N).to(dev)]
boxes_d, flip_d, lut = boxes.to(dev), flip.to(dev), D.LUT.to(dev)
idx = torch.randperm(N, generator=g).to(torch.int32).to(dev)
for k in range(3):
    ops.batch_rrc(*t, idx[:256], boxes_d, flip_d, lut, 224)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for k in range(20):
    x, y = ops.batch_rrc(*t, idx[256 * (k % 2):256 * (k % 2) + 256], boxes_d, flip_d, lut, 224)
e1.record()
torch.cuda.synchronize()
print("ee_batch_rrc_u8_f32 B=256 S=224: %.1f us per launch (20 back-to-back launches, events)" % (e0.elapsed_time(e1) * 1000 / 20))
print("mean crop %.0f x %.0f" % (boxes[:, 2].float().mean(), boxes[:, 3].float().mean()))
xr, yr = D.host_batch_rrc(*[a.cpu() for a in t], idx[256:260].long().cpu(), boxes, flip, 224)
print("matches host restatement on 4 samples:", torch.equal(x[:4].cpu(), xr))
# ee_batch_u8_f32 at the same output size for scale
data = torch.randint(0, 256, (512, 224, 224, 3), dtype=torch.uint8, device=dev)
for k in range(3):
    ops.batch_u8(data, t[3], idx[:256], flip_d, lut)
torch.cuda.synchronize()
