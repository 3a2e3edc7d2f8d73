#!/usr/bin/env python
# -*- encoding: utf-8 -*-
"""Fast adversarial training - FGSM from a uniform random start, three phases at 128 / 224 / 288 pixels, a learning rate interpolated per
iteration, PGD-with-restarts evaluation (reference: ImageNet/fgsm_imagenet/main_fast.py, lib/utils.py, lib/validation.py; DESIGN.md
section 28).

Kept from the reference: the command line (:34-55), the YAML sections TRAIN / ADV / DATA, output_name formed BEFORE the scaling
(utils.py:89-91), epochs / n_repeats and the /max_color_value scalings (:67-69), the two SGD groups (:107-112), the per-iteration learning
rate (:228-230), the directory layout (trained_models/<name>/checkpoint_epoch<E>.pth.tar + model_best.pth.tar, output/<name>/log.txt or
eval.txt, both under the working directory), `module.`-prefixed checkpoint keys (the reference saves the DataParallel model; --resume
reads either form; ours add `noise_step`, the counter of the drawn starts), --evaluate = every ADV.pgd_attack pair, then the clean pass (:165-170), the log and print formats.
Different: the run is fp32 on one device - `half: true` is read and answered with one log line (apex is not used); --pretrained stops
(nothing is downloaded); `data` may be synthetic[:train_batches[:val_batches]] and --no-cuda runs the host plumbing; the classifier pools
with AdaptiveAvgPool2d(1) - the global mean the reference's AvgPool2d(7) is at 224 pixels, and defined at 128 and 288 where that one is not.

    cd ImageNet/fgsm_imagenet && python main_fast.py synthetic -c configs/configs_fast_4px_phase1.yml
"""
import argparse
import datetime
import logging
import math
import os
import shutil
import sys
import time

sys.path.append(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.append(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

from utils.helper import AverageMeter, accuracy, set_seed  # noqa: E402

try:  # the reference's config object; a small attribute dict stands in where the package is absent
    from easydict import EasyDict
except ImportError:
    class EasyDict(dict):
        """dict whose keys read as attributes, nested dicts included (what the reference uses of easydict.EasyDict)"""

        def __init__(self, d=None, **kw):
            super().__init__()
            for k, v in dict(d or {}, **kw).items():
                self[k] = v

        def __setitem__(self, k, v):
            if isinstance(v, dict) and not isinstance(v, EasyDict):
                v = EasyDict(v)
            elif isinstance(v, (list, tuple)):
                v = type(v)(EasyDict(e) if isinstance(e, dict) else e for e in v)
            super().__setitem__(k, v)

        __setattr__ = __setitem__

        def __getattr__(self, k):
            try:
                return self[k]
            except KeyError:
                raise AttributeError(k) from None


class _ConfigLoader(yaml.SafeLoader):
    """SafeLoader that also reads the reference's `!!python/tuple [..]` sequences (as tuples); ours are plain lists"""


_ConfigLoader.add_constructor("tag:yaml.org,2002:python/tuple", lambda loader, node: tuple(loader.construct_sequence(node)))


def parse_args(argv=None):
    """main_fast.py:34-55, plus --no-cuda"""
    p = argparse.ArgumentParser(description='PyTorch ImageNet Training')
    p.add_argument('data', metavar='DIR', help='path to dataset, or synthetic[:train_batches[:val_batches]]')
    p.add_argument('--output_prefix', default='fast_adv', type=str, help='prefix used to define output path')
    p.add_argument('-c', '--config', default='configs.yml', type=str, metavar='Path', help='path to the config file (default: configs.yml)')
    p.add_argument('--resume', default='', type=str, metavar='PATH', help='path to latest checkpoint (default: none)')
    p.add_argument('-e', '--evaluate', dest='evaluate', action='store_true', help='evaluate model on validation set')
    p.add_argument('--pretrained', dest='pretrained', action='store_true', help='use pre-trained model')
    p.add_argument('--restarts', default=1, type=int)
    p.add_argument('--no-cuda', action='store_true', default=False, help='plain torch ops on the host (plumbing runs)')
    return p.parse_args(argv)


def parse_config_file(args):
    """utils.py:80-92: the YAML, the command line on top, output_name from the UNSCALED step and eps"""
    with open(args.config) as f:
        config = EasyDict(yaml.load(f, Loader=_ConfigLoader))
    for k, v in vars(args).items():
        config[k] = v
    config.output_name = '{:s}_step{:d}_eps{:d}_repeat{:d}'.format(args.output_prefix, int(config.ADV.fgsm_step), int(config.ADV.clip_eps),
                                                                   config.ADV.n_repeats)
    return config


def scale_config(configs):
    """main_fast.py:67-69, in place"""
    configs.TRAIN.epochs = int(math.ceil(configs.TRAIN.epochs / configs.ADV.n_repeats))
    configs.ADV.fgsm_step /= configs.DATA.max_color_value
    configs.ADV.clip_eps /= configs.DATA.max_color_value
    return configs


def lr_at(configs, t):
    """main_fast.py:172"""
    return np.interp([t], configs.TRAIN.lr_epochs, configs.TRAIN.lr_values)[0]


def pad_str(msg, total_len=70):
    """utils.py:76-78"""
    rem_len = total_len - len(msg)
    return '*' * int(rem_len / 2) + msg + '*' * int(rem_len / 2)


def initiate_logger(output_path, evaluate):
    """utils.py:59-69: output/<name>/log.txt (eval.txt with --evaluate), opened 'w', and the console"""
    os.makedirs(os.path.join('output', output_path), exist_ok=True)
    logger = logging.getLogger('main_fast')
    logger.setLevel(logging.INFO)
    logger.propagate = False
    for h in list(logger.handlers):  # a second main() in one process (tests) starts its own files
        logger.removeHandler(h)
        h.close()
    logger.addHandler(logging.StreamHandler(sys.stdout))
    logger.addHandler(logging.FileHandler(os.path.join('output', output_path, 'eval.txt' if evaluate else 'log.txt'), 'w'))
    logger.info(pad_str(' LOGISTICS '))
    logger.info('Experiment Date: {}'.format(datetime.datetime.now().strftime('%Y-%m-%d %H:%M')))
    logger.info('Output Name: {}'.format(output_path))
    logger.info('User: {}'.format(os.getenv('USER')))
    return logger


def save_checkpoint(state, is_best, filepath, epoch):
    """utils.py:95-101"""
    filename = os.path.join(filepath, 'checkpoint_epoch{}.pth.tar'.format(epoch))
    torch.save(state, filename)
    if is_best:
        shutil.copyfile(filename, os.path.join(filepath, 'model_best.pth.tar'))


def build_model(configs):
    """main_fast.py:88-93"""
    import models_imagenet as zoo
    k = int(configs.DATA.get('num_classes', 1000))
    if configs.TRAIN.arch == 'resnet50':
        model = zoo.resnet50(pretrained=configs.pretrained, num_classes=k)
    elif configs.TRAIN.arch == 'resnet50_EE':
        model = zoo.resnet50_EE(pretrained=configs.pretrained, num_classes=k, cize=configs.DATA.crop_size, r=configs.DATA.r, w=configs.DATA.w,
                                low=configs.DATA.low, high=configs.DATA.high)
    else:
        raise NotImplementedError
    model.avgpool = torch.nn.AdaptiveAvgPool2d(1)  # the three phases feed 4x4, 7x7 and 9x9 maps (see the module docstring)
    return model


def make_loaders(configs, device):
    """main_fast.py:133-162 on the device loaders: RandomResizedCrop(crop_size) + flip for train, CenterCrop(crop_size) for val, both after
    Resize(img_size) when DATA.img_size > 0"""
    from eeadv import data as D, driver
    S, k = int(configs.DATA.crop_size), int(configs.DATA.get('num_classes', 1000))
    spec = {"data": "imagenet", "shape": (3, S, S), "num_classes": k, "img_size": int(configs.DATA.img_size)}
    seed = int(configs.get('seed', 1))
    if driver.data_source(configs.data, spec) == "synthetic":
        parts = str(configs.data).split(":")
        n_train, n_val = (int(parts[1]) if len(parts) > 1 else 4), (int(parts[2]) if len(parts) > 2 else 2)
        return (driver.SyntheticLoader(n_train, configs.DATA.batch_size, spec["shape"], k, device, 1000 + seed),
                driver.SyntheticLoader(n_val, configs.DATA.batch_size, spec["shape"], k, device, 2000 + seed))
    return D.make_loaders("imagenet", configs.data, spec, device, int(configs.DATA.batch_size), seed)


_TRAIN_FMT = ('Train Epoch: [{0}][{1}/{2}]\t'
              'Time {batch_time.val:.3f} ({batch_time.avg:.3f})\t'
              'Data {data_time.val:.3f} ({data_time.avg:.3f})\t'
              'Loss {cls_loss.val:.4f} ({cls_loss.avg:.4f})\t'
              'Prec@1 {top1.val:.3f} ({top1.avg:.3f})\t'
              'Prec@5 {top5.val:.3f} ({top5.avg:.3f})\t'
              'LR {lr:.3f}')
_TEST_FMT = ('{0}: [{1}/{2}]\t'
             'Time {batch_time.val:.3f} ({batch_time.avg:.3f})\t'
             'Loss {loss.val:.4f} ({loss.avg:.4f})\t'
             'Prec@1 {top1.val:.3f} ({top1.avg:.3f})\t'
             'Prec@5 {top5.val:.3f} ({top5.avg:.3f})')


def _top5(configs):
    return min(5, int(configs.DATA.get('num_classes', 1000)))


def train(train_loader, model, step, epoch, configs, device, log):
    """main_fast.py:202-288.  The meters take every iteration, as the reference's do (:268-271), but on the device (driver._DeviceMeters):
    the host reads them where the reference prints instead of syncing with .item() on every iteration (:269)."""
    from eeadv.driver import _DeviceMeters
    batch_time, data_time = AverageMeter(), AverageMeter()
    meters = _DeviceMeters(3, device)
    model.train()
    end = time.time()
    R = configs.ADV.n_repeats
    for i, (input, target) in enumerate(train_loader):
        input, target = input.to(device), target.to(device)
        data_time.update(time.time() - end)
        for j in range(R):
            lr = lr_at(configs, epoch + (i * R + j + 1) / len(train_loader))  # :228-230
            step.set_lr(lr)
            loss, output = step(input, target, j=j)
            prec1, prec5 = accuracy(output, target, topk=(1, _top5(configs)))
            meters.update([loss, prec1, prec5], input.size(0))
            batch_time.update(time.time() - end)
            end = time.time()
            if i % configs.TRAIN.print_freq == 0:
                losses, top1, top5 = meters.read()
                log(_TRAIN_FMT.format(epoch, i, len(train_loader), batch_time=batch_time, data_time=data_time, top1=top1, top5=top5,
                                      cls_loss=losses, lr=lr))


def _validate(val_loader, model, criterion, configs, device, log, attack=None):
    """validation.py:8-88 (attack = (K, step)) and :90-138 (attack None)"""
    from eeadv import trainer
    batch_time, losses, top1, top5 = (AverageMeter() for _ in range(4))
    model.eval()
    end = time.time()
    eps = configs.ADV.clip_eps
    if attack is not None:
        log(pad_str(' PGD eps: {}, K: {}, step: {}, restarts: {} '.format(eps, attack[0], attack[1], configs.restarts)))
    for i, (input, target) in enumerate(val_loader):
        input, target = input.to(device), target.to(device)
        if attack is not None:
            _, output = trainer.pgd_restarts(model, input, target, eps, int(attack[0]), float(attack[1]), int(configs.restarts),
                                             seed=int(configs.get('seed', 1)) * 1000003 + i)
        else:
            with torch.no_grad():
                output = model(input)
        with torch.no_grad():
            loss = criterion(output, target)
        prec1, prec5 = accuracy(output, target, topk=(1, _top5(configs)))
        losses.update(loss.item(), input.size(0))
        top1.update(prec1.item(), input.size(0))
        top5.update(prec5.item(), input.size(0))
        batch_time.update(time.time() - end)
        end = time.time()
        if i % configs.TRAIN.print_freq == 0:
            log(_TEST_FMT.format('Test' if attack is None else 'PGD Test', i, len(val_loader), batch_time=batch_time, loss=losses, top1=top1,
                                 top5=top5))
    log((' Final Prec@1 {top1.avg:.3f} Prec@5 {top5.avg:.3f}' if attack is None else
         ' PGD Final Prec@1 {top1.avg:.3f} Prec@5 {top5.avg:.3f}').format(top1=top1, top5=top5))
    return top1.avg


def validate(val_loader, model, criterion, configs, device, log):
    return _validate(val_loader, model, criterion, configs, device, log)


def validate_pgd(val_loader, model, criterion, K, step, configs, device, log):
    return _validate(val_loader, model, criterion, configs, device, log, attack=(K, step))


def main(argv=None, build=build_model):
    """`build`: configs -> model (tests train a small classifier through the same loop)"""
    from eeadv import driver, runtime, trainer
    args = parse_args(argv)
    if args.pretrained:
        raise SystemExit("--pretrained: the reference downloads torchvision weights; nothing is downloaded here - pass --resume <checkpoint>")
    configs = parse_config_file(args)
    logger = initiate_logger(configs.output_name, configs.evaluate)
    log = logger.info
    best_prec1, noise_step = 0, 0
    scale_config(configs)
    os.makedirs(os.path.join('trained_models', configs.output_name), exist_ok=True)
    log(pad_str(' ARGUMENTS '))
    for k, v in configs.items():
        log('{}: {}'.format(k, v))
    log(pad_str(''))
    if configs.no_cuda:
        runtime.allow_cpu_plumbing(True)
        device = torch.device("cpu")
    else:
        device = torch.device("cuda", 0)
        torch.cuda.set_device(device)
        os.environ.setdefault("EEADV_GRAPH", "1")  # one rank: the step and the evaluation attack replay captured HIP graphs
    set_seed(int(configs.get('seed', 1)))
    log("=> creating model '{}'".format(configs.TRAIN.arch))
    model = build(configs).to(device)
    criterion = trainer.Criterion()
    optimizer = trainer.make_fast_sgd(model, configs.TRAIN.lr, momentum=configs.TRAIN.momentum, weight_decay=configs.TRAIN.weight_decay)
    if configs.TRAIN.get('half', False) and not configs.evaluate:
        log("=> TRAIN.half is set: this run is fp32 (apex mixed precision is not used)")
    if configs.resume:  # :119-130
        if os.path.isfile(configs.resume):
            log("=> loading checkpoint '{}'".format(configs.resume))
            checkpoint = torch.load(configs.resume, map_location=device, weights_only=True)
            configs.TRAIN.start_epoch = checkpoint['epoch']
            best_prec1 = checkpoint['best_prec1']
            model.load_state_dict(driver.strip_module_prefix(checkpoint['state_dict']))
            optimizer.load_state_dict(checkpoint['optimizer'])
            noise_step = int(checkpoint.get('noise_step', 0))  # ours: the counter of the drawn starts, so a resumed run draws on
            log("=> loaded checkpoint '{}' (epoch {})".format(configs.resume, checkpoint['epoch']))
        else:
            log("=> no checkpoint found at '{}'".format(configs.resume))
    train_loader, val_loader = make_loaders(configs, device)
    if configs.evaluate:  # :165-170
        log(pad_str(' Performing PGD Attacks '))
        for pgd_param in configs.ADV.pgd_attack:
            validate_pgd(val_loader, model, criterion, pgd_param[0], pgd_param[1], configs, device, log)
        validate(val_loader, model, criterion, configs, device, log)
        return best_prec1
    S = int(configs.DATA.crop_size)
    noise = torch.zeros([configs.DATA.batch_size, 3, S, S], device=device)  # :201
    step = trainer.FastAtStep(model, criterion, optimizer, noise, configs.ADV.fgsm_step, configs.ADV.clip_eps,
                              random_init=bool(configs.TRAIN.random_init), seed=int(configs.get('seed', 1)))
    step.step_ctr.fill_(noise_step)
    for epoch in range(configs.TRAIN.start_epoch, configs.TRAIN.epochs):
        train(train_loader, model, step, epoch, configs, device, log)
        prec1 = validate(val_loader, model, criterion, configs, device, log)
        is_best = prec1 > best_prec1
        best_prec1 = max(prec1, best_prec1)
        save_checkpoint({'epoch': epoch + 1, 'arch': configs.TRAIN.arch, 'state_dict': driver.with_module_prefix(model.state_dict()),
                         'best_prec1': best_prec1, 'optimizer': step.state_dict(), 'noise_step': int(step.step_ctr.item())}, is_best,
                        os.path.join('trained_models', configs.output_name), epoch + 1)
    return best_prec1


if __name__ == '__main__':
    main()
