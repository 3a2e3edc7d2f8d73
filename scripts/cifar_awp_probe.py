#!/usr/bin/env python3
"""The CIFAR-100 AWP workload (AWP/Cifar100/experiments_cifar100_awp.py with configs_cifar100_awp/at_awp.yml): PreActResNet18(CIFAR100),
batch 128 of synthetic 3x32x32 images, train mode, one whole AWP step = PGD-10 + proxy step + robust step (eeadv.trainer.awp_train_batch).

Time: graph replay as the driver runs it (EEADV_GRAPH=1), CUDA events, median of `reps` after 3 warm-up steps.  Launches: the same step run
eagerly (EEADV_GRAPH=0) under torch.profiler, device kernels counted - a replayed graph issues the same kernels.  Also the time of one
train batch of ee_batch_aug_u8_f32 (batch 128 out of 1024 resident images).

    python scripts/cifar_awp_probe.py [reps]       -> one JSON line per child, then a summary line
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")


def child(reps):
    sys.path[:0] = [PKG, os.path.join(PKG, "AWP", "Tiny_imagenet"), os.path.join(PKG, "AWP", "Cifar100")]
    import numpy as np
    import torch
    import models_cifar100_awp as Z
    import utils.attacks as A
    from eeadv import data as D, models as M, ops, trainer

    class Args:
        method_name, random, epsilon, num_steps_1, step_size_1, awp_warmup = "AT_AWP", True, 8 / 255, 10, 2 / 255, 0

    torch.manual_seed(0)
    net, proxy = Z.PreActResNet18(dataset="CIFAR100").cuda().train(), Z.PreActResNet18(dataset="CIFAR100").cuda()
    opt = trainer.make_sgd(net.parameters(), lr=0.1, momentum=0.9, weight_decay=2e-4)
    adv = Z.AdvWeightPerturb(model=net, proxy=proxy, proxy_optim=trainer.make_sgd(proxy.parameters(), lr=0.01), gamma=0.01)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(128, 3, 32, 32, generator=g).cuda()
    y = torch.randint(0, 100, (128,), generator=g).cuda()
    pgd = lambda k: A.PGD(net, Args, x, y, k, Args.step_size_1)
    step = lambda: trainer.awp_train_batch(net, adv, trainer.Criterion(), opt, Args, x, y, 0, x.device)

    def timed(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return sorted(ts)[len(ts) // 2]

    def launches(fn):
        fn()
        torch.cuda.synchronize()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name
                   and "Memset" not in e.name)

    out = {"graph": os.environ.get("EEADV_GRAPH")}
    if os.environ.get("EEADV_GRAPH") == "0":
        out["launches_pgd1"] = launches(lambda: pgd(1))
        out["launches_pgd10"] = launches(lambda: pgd(10))
        out["launches_awp_step"] = launches(step)
        out["vendor_convolutions"] = M.fallback_report(net)
    else:
        out["ms_pgd10"] = timed(lambda: pgd(10))
        out["ms_awp_step"] = timed(step)
        out["img_per_s"] = 128 / out["ms_awp_step"] * 1e3
        rng = np.random.default_rng(0)
        images = torch.from_numpy(rng.integers(0, 256, (1024, 32, 32, 3), dtype=np.uint8)).cuda()
        labels = torch.zeros(1024, dtype=torch.int64).cuda()
        ids = torch.from_numpy(rng.integers(0, 1024, 128).astype(np.int32))
        offs = torch.from_numpy(rng.integers(0, 9, (128, 2)).astype(np.int32))
        flip = torch.from_numpy(rng.integers(0, 2, 128).astype(np.uint8))
        coef = torch.from_numpy(D.aug_coeffs(rng.uniform(-15, 15, 128), 32, 32))
        dev = [t.cuda() for t in (ids, offs, flip, coef)]
        lut = D.LUT.cuda()
        out["ms_batch_aug"] = timed(lambda: ops.batch_aug(images, labels, dev[0], dev[1], dev[2], dev[3], lut, ids, offs, 4))
    print(json.dumps(out), flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    rows = {}
    for graph in ("1", "0"):
        env = dict(os.environ, EEADV_GRAPH=graph, CIFAR_PROBE_CHILD=str(reps))
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-3000:])
            raise SystemExit("probe child failed (graph=%s): exit %d" % (graph, r.returncode))
        line = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(line), flush=True)
        rows.update(line)
    print(json.dumps({"summary": "CIFAR-100 AWP step, PreActResNet18, batch 128, PGD-10", "awp_step_ms": round(rows["ms_awp_step"], 2),
                      "img_per_s": round(rows["img_per_s"]), "pgd_iter_ms": round(rows["ms_pgd10"] / 10, 3),
                      "launches_per_pgd_iter": (rows["launches_pgd10"] - rows["launches_pgd1"]) / 9, "launches_awp_step": rows["launches_awp_step"],
                      "batch_aug_ms": round(rows["ms_batch_aug"], 4)}))


if __name__ == "__main__":
    if os.environ.get("CIFAR_PROBE_CHILD"):
        child(int(os.environ["CIFAR_PROBE_CHILD"]))
    else:
        main()
