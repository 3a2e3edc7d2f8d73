"""What tests/test_aa_host.py and tests/test_gpu_aa.py share: the tiny model, its 12 samples, the budgets and a `--dataset unit` entry for
utils/aa.py."""
import os

import torch

from tiny_models import Args, TinyNet

N_CLASS, SHAPE, N, B, SEED = 10, (3, 8, 8), 12, 4, 7
WRONG = (2, 9)  # the two samples whose label is not the model's clean prediction
EPS = {"Linf": 8 / 255, "L2": 0.5, "L1": 1.5}
NUM_STEPS, FAB_ITERS, SQUARE_QUERIES = 5, 3, 16
SPEC = {"shape": SHAPE, "num_classes": N_CLASS}


def build_model(args=None):
    """One 3x3 convolution, ReLU, 2x2 average pool, linear; seeded, so every call gives the same weights."""
    return TinyNet(SHAPE[0], SHAPE[1], N_CLASS, 5)


def samples(device="cpu"):
    """(x [12, 3, 8, 8], y [12]) on `device`: seeded images, labels the model's own clean predictions on all but WRONG."""
    g = torch.Generator().manual_seed(11)
    x = torch.rand((N,) + SHAPE, generator=g)
    with torch.no_grad():
        y = build_model().eval()(x).argmax(1)
    for i in WRONG:
        y[i] = (y[i] + 1) % N_CLASS
    return x.to(device), y.to(device)


def batches(device="cpu"):
    x, y = samples(device)
    return [(x[i:i + B], y[i:i + B]) for i in range(0, N, B)]


def args_for(norm="Linf", **kw):
    """What a direct call of cascade.evaluate / aa_stages takes in the place of the script's parsed options."""
    return Args(epsilon=EPS[norm], fab_iters=FAB_ITERS, square_queries=SQUARE_QUERIES, num_steps_1=NUM_STEPS, **kw)


def register(monkeypatch, aa):
    """`--dataset unit`: the model and the samples above in the place of a zoo and a loader."""
    monkeypatch.setitem(aa.DATASETS, "unit", lambda: (SPEC, build_model, lambda args, spec, device, batch: (None, batches(device))))


def script_argv(tmp_path, version, norm="Linf", *extra):
    """The command line of one run of the script on the unit dataset, its config written under tmp_path."""
    cfg = os.path.join(str(tmp_path), "unit_%s.yml" % norm)
    with open(cfg, "w") as f:
        f.write("arch: tiny\nbatch_size: %d\nepsilon: %r\nseed: %d\nnum_steps_1: %d\n" % (B, EPS[norm], SEED, NUM_STEPS))
    return ["--dataset", "unit", "-c", cfg, "--version", version, "--norm", norm, "--fab_iters", str(FAB_ITERS), "--square_queries",
            str(SQUARE_QUERIES), "--save_dir", os.path.join(str(tmp_path), "out"), "--log_path", os.path.join(str(tmp_path), "log", "aa.txt")] + list(extra)
