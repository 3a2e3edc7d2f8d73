#!/usr/bin/env python
# -*- encoding: utf-8 -*-
"""The reference's evaluation entry point (utils/aa.py) on eeadv's own ensemble.

It loads a checkpoint and a test split, runs `--version standard | plus | rand | custom` under `--norm Linf | L2 | L1` - on the survivors
(eeadv.cascade.evaluate over the stage list of cascade.aa_stages) or, with `--individual`, every member on all points -, prints the clean
accuracy and the robust accuracy after every stage, checks that the points lie in the ball they were made for (ops.pert_check, the line the
`autoattack` package prints after a run) and writes them to `--save_dir`.

    python utils/aa.py --dataset tiny -c Tiny_ImageNet/configs_tinyimagenet/ee_at_bpda3_square.yml --version standard --data synthetic:1:2

This is NOT the `autoattack` package: the attacks are the ones of utils/attacks.py on the captured attack engine, with the departures the
log names in its first lines.  One script serves every model zoo (`--dataset`), where the reference keeps a copy per tree; its `managpu`
import, its missing `CannyFilter_pre` import and its broken file-name format string are not restated.  APGD runs args.num_steps_1
iterations, as `--attack_method Cascade` does in the drivers.
"""
import argparse
import importlib
import os
import sys
import time
import types

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

import torch  # noqa: E402

from eeadv import cascade, driver, ops, runtime  # noqa: E402
from utils.helper import parse_config_file, set_seed  # noqa: E402

VERSIONS = tuple(cascade.AA_VERSIONS)
NORMS = cascade.AA_VERSIONS["standard"]
NORM_COLUMN = {"Linf": 0, "L2": 1, "L1": 2}  # the column of ops.pert_check's norms


def _driver(subdir, module):
    """() -> (SPEC, build_model, make_loaders) of the driver script `module` under <package>/<subdir>, imported when it is asked for."""
    def load():
        d = os.path.join(_PKG, *subdir.split("/"))
        if d not in sys.path:
            sys.path.insert(0, d)
        m = importlib.import_module(module)
        return m.SPEC, m.build_model, driver.make_loaders
    return load


# --dataset -> the model zoo and the data spec of the matching driver
DATASETS = {"tiny": _driver("Tiny_ImageNet", "experiments_tinyimagenet"), "mnist": _driver("MNIST", "experiments_mnist"),
            "imagenet": _driver("ImageNet", "experiments_imagenet"), "cifar100": _driver("AWP/Cifar100", "experiments_cifar100_awp")}


def make_parser():
    """The reference's options (utils/aa.py:31-46) and the additions every driver here has."""
    p = argparse.ArgumentParser(description="eeadv's AutoAttack-style evaluation: the versions of the reference's utils/aa.py on the project's own ensemble")
    p.add_argument('--data', type=str, default='synthetic', help='path to dataset, or synthetic[:train_batches[:val_batches]] (default)')
    p.add_argument('--norm', type=str, default='Linf', choices=NORMS, help='threat model, radius epsilon of the config')
    p.add_argument('-c', '--config', default='configs.yml', type=str, metavar='Path', help='path to the config file (default: configs.yml)')
    p.add_argument('--resume', default='', type=str, metavar='PATH', help='path to the checkpoint to evaluate (default: none, the initialised model)')
    p.add_argument('--n_ex', type=int, default=0, help='evaluate the first n_ex samples of the test split (default 0: all of it)')
    p.add_argument('--individual', action='store_true', help='run every attack of the version on all points instead of on the survivors')
    p.add_argument('--save_dir', type=str, default='./results/ee')
    p.add_argument('--log_path', type=str, default='./Log/log_aa.txt')
    p.add_argument('--version', type=str, default='standard', choices=VERSIONS)
    p.add_argument('--no-cuda', action='store_true', default=False, help='run the host plumbing path')
    p.add_argument('--pretrained', dest='pretrained', action='store_true', help='use pre-trained model')
    p.add_argument('--dataset', type=str, default='tiny', choices=sorted(DATASETS), help='the model zoo and data spec (default: tiny)')
    p.add_argument('--fab_iters', default=100, type=int, help='iterations of every FAB run (default: 100)')
    p.add_argument('--square_queries', default=5000, type=int, help='forwards per sample of the Square attack at most (default: 5000)')
    p.add_argument('--eot_iter', default=None, type=int, help='forwards every APGD gradient of `rand` is averaged over (default: 20)')
    return p


def ball_tolerance(norm, eps, D):
    """The largest norm of x_adv - x0 that the attacks' own statements allow a point of the eps-ball, for samples of D values:
        Linf  eps + 2^-23: clamp(x0 +- eps) in float32 exceeds eps by one rounding of the difference at most
        L2    eps (1 + 1.5 * 2^-23) + 5 * 1.2e-8: what the rescale leaves plus five deviations of the last addition's absolute
              rounding (eps (1 + 4 * 2^-23) at eps = 0.5); the FAB and Square points lie below it (sections 17, 18)
        L1    eps + D 2^-23: the invariant of the exact projection; the Square-L1 points are projected onto
              eps (1 - 1e-6) and lie below it (section 21)"""
    eps = float(eps)
    if norm == "Linf":
        return eps + 2.0 ** -23
    if norm == "L2":
        return eps * (1.0 + 1.5 * 2.0 ** -23) + 5 * 1.2e-8
    if norm == "L1":
        return eps + D * 2.0 ** -23
    raise ValueError("norm must be one of %s, got %r" % (", ".join(NORMS), norm))


def check_points(adv, x0, norm, eps, log, tag=""):
    """ops.pert_check of adv against x0, the package's line, and a warning if a sample lies outside the ball.  Returns a namespace: norms
    [n] of the run's norm, outside (the number of samples above ball_tolerance, NaN norms included), tolerance, n_nan, lo, hi."""
    norms, rng, n_nan = ops.pert_check(adv.contiguous(), x0.contiguous())
    col = norms[:, NORM_COLUMN[norm]].double()
    tol = ball_tolerance(norm, eps, adv[0].numel())
    outside, worst = int((~(col <= tol)).sum()), float(torch.nan_to_num(col, nan=float("inf")).max())
    lo, hi, nans = float(rng[:, 0].min()), float(rng[:, 1].max()), int(n_nan.sum())
    log('{0}max {1} perturbation: {2:.5f}, nan in tensor: {3}, max: {4:.5f}, min: {5:.5f}'.format(tag, norm, worst, nans, hi, lo))
    log('{0}perturbation check: {1} of {2} samples outside the {3} ball of radius {4:.5f} (tolerance {5:.3e} above it)'.format(
        tag, outside, adv.shape[0], norm, float(eps), tol - float(eps)))
    if outside:
        log('{0}WARNING: {1} samples exceed epsilon by more than the tolerance; the largest {2} norm is {3:.8f}'.format(tag, outside, norm, worst))
    return types.SimpleNamespace(norms=col, outside=outside, tolerance=tol, n_nan=nans, lo=lo, hi=hi)


def first_samples(loader, n_ex, device):
    """The batches of the first n_ex samples of `loader` (0: all), on `device`; the last one cut to size."""
    out, left = [], int(n_ex) if n_ex else None
    for x, y in loader:
        if left is not None:
            if left <= 0:
                break
            x, y = x[:left], y[:left]
            left -= int(y.shape[0])
        out.append((x.to(device), y.to(device)))
    return out


def main(argv=None):
    """Returns a namespace of what was printed and saved: n, clean_correct, robust_accuracy (percent), path (None when nothing was saved),
    check (check_points' result; per member under --individual), and result (cascade.evaluate's) or members ({name: (adv, robust)})."""
    args = parse_config_file(make_parser().parse_args(argv))
    spec, build_model, make_loaders = DATASETS[args.dataset]()
    spec = driver.sized(spec, args)
    for key, default in (("type_canny", None), ("n_queries", 1), ("cize", spec["shape"][-1])):
        if key not in args:
            args[key] = default  # keys the zoos read unconditionally but several configs omit, as in driver.run
    args.num_classes, args.crop_size = spec["num_classes"], spec["shape"][-1]
    n_class, eps = int(spec["num_classes"]), float(args.epsilon)
    cascade.aa_stages(args, int(args.num_steps_1), n_class, args.version, args.norm)  # an unsupported combination stops here, before a model is built
    use_cuda = not args.no_cuda and torch.cuda.is_available()
    if use_cuda:
        device = torch.device("cuda", 0)
        os.environ.setdefault("EEADV_GRAPH", "1")  # the attack loops replay captured graphs, as in the drivers
    else:
        device = torch.device("cpu")
        runtime.allow_cpu_plumbing(True)
    if os.path.dirname(args.log_path):
        os.makedirs(os.path.dirname(args.log_path), exist_ok=True)

    def log(line):
        print(line)
        with open(args.log_path, 'a') as f:
            print(line, file=f)

    log("eeadv evaluation, version {0}, norm {1}, eps {2:.5f}: this is eeadv's own ensemble on the captured attack engine, NOT the autoattack "
        "package".format(args.version, args.norm, eps))
    log("departures (DESIGN.md sections 14, 23, 24): the uniform start of APGD is not rescaled to the full radius; a restart inside a stage runs "
        "on the whole batch, not on its survivors; random draws are made per regrouped batch, not per sample id")
    set_seed(args.seed)
    print("=> creating model '{}'".format(args.arch))
    model = build_model(args).to(device)
    if args.resume:
        ckpt, missing = driver.load_model_checkpoint(model, args.resume, device)
        log("=> loaded checkpoint '{}' (epoch {}); ignored keys: {}".format(args.resume, ckpt.get('epoch'), len(missing.unexpected_keys)))
    else:
        log("=> no --resume: evaluating the initialised model")
    model.eval()

    _, test_loader = make_loaders(args, spec, device, args.batch_size)
    batches = first_samples(test_loader, args.n_ex, device)
    n = sum(int(y.shape[0]) for _, y in batches)
    x0 = torch.cat([x for x, _ in batches])
    stages = cascade.aa_stages(args, int(args.num_steps_1), n_class, args.version, args.norm)
    os.makedirs(args.save_dir, exist_ok=True)
    stem = '{}/aa_{}_{}_{}_eps_{:.5f}'.format(args.save_dir, args.version, args.norm, n, eps)
    out = types.SimpleNamespace(n=n, path=None, check=None, result=None, members=None)
    start = time.time()

    if args.individual:
        # every member from the run's seed: an entry is the member's door on every whole batch after set_seed(args.seed)
        members = cascade.individual(model, args, batches, n_class, stages, before_member=lambda name: set_seed(args.seed))
        with torch.no_grad():
            correct = torch.cat([model(x).argmax(1) == y for x, y in batches])
        out.clean_correct, out.members, out.check = int(correct.sum()), members, {}
        log(' * AA clean accuracy {0:.3f}'.format(100.0 * out.clean_correct / n))
        robust_all = correct.clone()
        for name, (adv, robust) in members.items():
            robust_all &= robust
            log(' * AA individual robust accuracy of {0} {1:.3f}'.format(name, 100.0 * float((robust & correct).float().mean())))
            out.check[name] = check_points(adv, x0, args.norm, eps, log, tag='{0}: '.format(name))
        out.robust_accuracy = 100.0 * float(robust_all.float().mean())
        log(' * AA robust accuracy {0:.3f} ({1:.1f} s)'.format(out.robust_accuracy, time.time() - start))
        out.path = stem + '_individual.pth'
        torch.save({name: adv.cpu() for name, (adv, _) in members.items()}, out.path)
        log('=> saved the points of every member to {0}'.format(out.path))
        return out

    set_seed(args.seed)  # the draws of the evaluation follow from the seed alone, not from what building the model drew
    try:
        res = cascade.evaluate(model, args, batches, n_class, keep_adv=True, stages=stages, n=n)
    except MemoryError as e:
        log('=> {0}'.format(e))
        log('=> the adversarial points do not fit next to the model: evaluating without saving them')
        set_seed(args.seed)
        res = cascade.evaluate(model, args, batches, n_class, keep_adv=False, stages=stages, n=n)
    out.result, out.clean_correct = res, res.clean_correct
    log(' * AA: {0} samples, {1} attacked rows per stage {2}, {3:.1f} s'.format(
        res.n, '/'.join(res.stage_names), '/'.join(str(r) for r in res.rows_attacked), time.time() - start))
    log(' * AA clean accuracy {0:.3f}'.format(100.0 * res.clean_correct / res.n))
    for name, left in zip(res.stage_names, res.robust_after):
        log(' * AA robust accuracy after {0} {1:.3f}'.format(name, 100.0 * left / res.n))
    out.robust_accuracy = 100.0 * float(res.robust.float().mean())
    log(' * AA robust accuracy {0:.3f}'.format(out.robust_accuracy))
    if res.adv is not None:
        out.check = check_points(res.adv, x0, args.norm, eps, log)
        out.path = stem + '.pth'
        torch.save(res.adv.cpu(), out.path)
        log('=> saved the adversarial points [{0}] to {1}'.format(', '.join(str(s) for s in res.adv.shape), out.path))
    return out


if __name__ == '__main__':
    main()
