#!/usr/bin/env python
# -*- encoding: utf-8 -*-
"""Adversarial Weight Perturbation on CIFAR-100 (reference: AWP/Cifar100/experiments_cifar100_awp.py).  Same CLI, YAML keys, `arch` /
`method_name` strings (AT_AWP), output directory, log lines and checkpoint names; the CIFAR PreActResNet runs on the HIP path
(eeadv.preact.PreActResNetCifar), one step is eeadv.trainer.awp_train_batch, and the train batches are RandomCrop(32, padding=4) +
RandomHorizontalFlip + RandomRotation(15) by one launch each (eeadv.data.AugDeviceLoader).

    python experiments_cifar100_awp.py -c configs_cifar100_awp/at_awp.yml --data /path/to/CIFAR100

Added, as in the other drivers: `--data synthetic[:train_batches[:val_batches]]`, `--output-root`, `--max-epochs`.  `--arch WideResNet`
raises NotImplementedError, as the reference does.  Keys the reference's -e path reads but its config omits (step_size_2, num_steps_3,
step_size_3) default to the previous setting's value.
"""
import os
import sys
import time

sys.path.append(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch  # noqa: E402
import torch.optim as optim  # noqa: E402

from eeadv import driver, runtime, trainer  # noqa: E402
from utils.helper import AverageMeter, adjust_learning_rate_1, parse_config_file, save_checkpoint, set_seed  # noqa: E402
from models_cifar100_awp import AdvWeightPerturb, PreActResNet18  # noqa: E402

SPEC = {"description": "PyTorch Cifar100 AWP Training", "ckpt_dir": "checkpoint_Cifar100_AWP1", "shape": (3, 32, 32), "num_classes": 100,
        "data": "cifar100"}


def make_parser():
    """experiments_cifar100_awp.py:118-134 (+ the flags every driver here takes: driver.make_parser)"""
    return driver.make_parser(SPEC["description"])


def build_model(args):
    """experiments_cifar100_awp.py:156-162: the model, and a proxy of the same arch"""
    if args.arch == 'PreActResNet18':
        return PreActResNet18(dataset="CIFAR100")
    raise NotImplementedError  # 'WideResNet' included, as the reference


def output_dirs(args):
    """experiments_cifar100_awp.py:221-234"""
    root = args.output_root or os.getcwd()
    d = (root + '/' + SPEC["ckpt_dir"] + '/' + str(args.method_name) + '/' + str(args.arch) + '-bs' + str(args.batch_size) + '-lr' + str(args.lr) +
         '-momentum' + str(args.momentum) + '-wd' + str(args.weight_decay) + '-seed' + str(args.seed) + '/')
    dirs = {"root": d, "model": d + 'model_pth/', "best": d + 'best_model_pth/', "log": d + 'log/'}
    for k in ("log", "model", "best"):
        os.makedirs(dirs[k], exist_ok=True)
    return dirs


def _log(line, path):
    print(line)
    with open(path, 'a') as f:
        print(line, file=f)


def make_optimizer(model, args):
    """experiments_cifar100_awp.py:169-183: with `l2`, weight decay `l2` on every parameter whose name holds neither 'bn' nor 'bias'"""
    if args.l2:
        decay, no_decay = [], []
        for name, param in model.named_parameters():
            (decay if 'bn' not in name and 'bias' not in name else no_decay).append(param)
        params = [{'params': decay, 'weight_decay': args.l2}, {'params': no_decay, 'weight_decay': 0}]
        return optim.SGD(params, lr=args.lr, momentum=args.momentum, weight_decay=args.weight_decay)
    return trainer.make_sgd(model.parameters(), lr=args.lr, momentum=args.momentum, weight_decay=args.weight_decay)


def train(train_loader, model, awp_adversary, criterion, optimizer, epoch, args, device, log_dir):
    """experiments_cifar100_awp.py:271-350"""
    batch_time, data_time = AverageMeter(), AverageMeter()
    meters = driver._DeviceMeters(3, device)
    model.train()
    end = time.time()
    for i, (input, target) in enumerate(train_loader):
        target, input = target.to(device), input.to(device)
        data_time.update(time.time() - end)
        adjust_learning_rate_1(optimizer, epoch + (i + 1) / len(train_loader), args.lr, args.epochs)
        loss, output = trainer.awp_train_batch(model, awp_adversary, criterion, optimizer, args, input, target, epoch, device, l1=args.l1)
        prec1, prec5 = trainer.accuracy(output, target, topk=(1, 5))
        meters.update([loss, prec1, prec5], input.size(0))
        batch_time.update(time.time() - end)
        end = time.time()
        if i % args.print_freq == 0:
            losses, top1, top5 = meters.read()
            _log('Epoch: [{0}][{1}/{2}]\t'
                 'Time {batch_time.val:.3f} ({batch_time.avg:.3f})\t'
                 'Data {data_time.val:.3f} ({data_time.avg:.3f})\t'
                 'Robust Loss {loss.val:.4f} ({loss.avg:.4f})\t'
                 'Prec@1 {top1.val:.3f} ({top1.avg:.3f})\t'
                 'Prec@5 {top5.val:.3f} ({top5.avg:.3f})\t'.format(epoch, i, len(train_loader), batch_time=batch_time, data_time=data_time,
                                                                  loss=losses, top1=top1, top5=top5), log_dir + 'log.txt')


def validate(val_loader, model, criterion, args, device, num_steps, step_size, log_dir):
    """experiments_cifar100_awp.py:353-435: PGD-`num_steps` in eval mode; lines to log/log.txt.  Returns (adv top-1, adv top-5)."""
    if args.attack_method in trainer.CASCADE_METHODS:
        return driver.validate_cascade(val_loader, model, args, device, num_steps, SPEC["num_classes"], lambda line: _log(line, log_dir + 'log.txt'))
    batch_time = AverageMeter()
    meters = driver._DeviceMeters(6, device)
    model.eval()
    end = time.time()
    for i, (input, target) in enumerate(val_loader):
        target, input = target.to(device), input.to(device)
        vals = trainer.validate_batch(model, criterion, args, input, target, device, num_steps, step_size, SPEC["num_classes"])
        meters.update(list(vals), input.size(0))
        batch_time.update(time.time() - end)
        end = time.time()
        if i % args.print_freq == 0:
            lc, la, t1c, t5c, t1a, t5a = meters.read()
            fmt = ('{tag}: [{0}/{1}]\tTime {batch_time.val:.3f} ({batch_time.avg:.3f})\tLoss {loss.val:.4f} ({loss.avg:.4f})\t'
                   'Prec@1 {top1.val:.3f} ({top1.avg:.3f})\tPrec@5 {top5.val:.3f} ({top5.avg:.3f})')
            _log(fmt.format(i, len(val_loader), tag='Test_clean', batch_time=batch_time, loss=lc, top1=t1c, top5=t5c), log_dir + 'log.txt')
            _log(fmt.format(i, len(val_loader), tag='Test_adv', batch_time=batch_time, loss=la, top1=t1a, top5=t5a), log_dir + 'log.txt')
    lc, la, t1c, t5c, t1a, t5a = meters.read()
    _log(' * Clean Prec@1 {top1.avg:.3f} Prec@5 {top5.avg:.3f}'.format(top1=t1c, top5=t5c), log_dir + 'log.txt')
    _log(' * Adv Prec@1 {top1.avg:.3f} Prec@5 {top5.avg:.3f}'.format(top1=t1a, top5=t5a) + trainer.norm_tag(args), log_dir + 'log.txt')
    return t1a.avg, t5a.avg


def main(argv=None):
    """experiments_cifar100_awp.py:138-269"""
    args = parse_config_file(make_parser().parse_args(argv))
    if args.attack_method != 'PGD' and args.attack_method not in trainer.EVAL_METHODS:
        raise NotImplementedError("--attack_method %s: validation runs %s or %s" % (args.attack_method, ", ".join(('PGD',) + trainer.EVAL_METHODS[:-1]),
                                                                                    trainer.EVAL_METHODS[-1]))  # experiments_cifar100_awp.py:374-380
    driver.data_source(args.data, SPEC)  # an unusable --data fails here, before a model is built
    trainer.eot_iter_for(args)  # so does an --eot_iter the chosen attack cannot honour
    trainer.fab_restarts_for(args)  # and a --fab_restarts on a method that runs no FAB
    trainer.apgd_restarts_for(args)  # and an --apgd_restarts on a method that runs no APGD
    trainer.norm_for(args)  # and a --norm it has no L2 for
    for key, default in (("step_size_2", args.get("step_size_1")), ("num_steps_3", args.get("num_steps_2"))):
        args.setdefault(key, default)
    args.setdefault("step_size_3", args.step_size_2)
    args.setdefault("cize", 32)
    args.num_classes = SPEC["num_classes"]
    use_cuda = not args.no_cuda and torch.cuda.is_available()
    if use_cuda:
        device = torch.device("cuda", 0)
        os.environ.setdefault("EEADV_GRAPH", "1")
    else:
        device = torch.device("cpu")
        runtime.allow_cpu_plumbing(True)
    set_seed(args.seed)
    if args.awp_gamma <= 0.0:
        args.awp_warmup = float('inf')

    print("=> using pre-trained model '{}'".format(args.arch) if args.pretrained else "=> creating model '{}'".format(args.arch))
    model = build_model(args).to(device)
    proxy = build_model(args).to(device)
    optimizer = make_optimizer(model, args)
    proxy_optimizer = trainer.make_sgd(proxy.parameters(), lr=0.01)
    awp_adversary = AdvWeightPerturb(model=model, proxy=proxy, proxy_optim=proxy_optimizer, gamma=args.awp_gamma)
    criterion = trainer.make_criterion(args)

    best_prec1 = 0.0
    if args.resume:
        if os.path.isfile(args.resume):
            print("=> loading checkpoint '{}'".format(args.resume))
            checkpoint = torch.load(args.resume, map_location=device, weights_only=True)
            args.start_epoch = checkpoint['epoch']
            best_prec1 = checkpoint['best_prec1']
            model.load_state_dict(driver.strip_module_prefix(checkpoint['state_dict']))
            optimizer.load_state_dict(checkpoint['optimizer'])
            print("=> loaded checkpoint '{}' (epoch {})".format(args.resume, checkpoint['epoch']))
    else:
        print("=> no checkpoint found at '{}'".format(args.resume))

    train_loader, val_loader = driver.make_loaders(args, SPEC, device, args.batch_size)
    dirs = output_dirs(args)

    if args.evaluate:  # PGD10, PGD50, PGD100 in the reference's comments: whatever the three settings say
        for k, s in ((args.num_steps_1, args.step_size_1), (args.num_steps_2, args.step_size_2), (args.num_steps_3, args.step_size_3)):
            print("=> evaluate.tar_num_step:{},step_size:{}".format(k, s))
            validate(val_loader, model, criterion, args, device, k, s, dirs["log"])
        return best_prec1

    print("Output dir:" + dirs["root"])
    last_epoch = args.epochs if args.max_epochs is None else min(args.epochs, args.start_epoch + args.max_epochs)
    for epoch in range(args.start_epoch, last_epoch):
        for loader in (train_loader, val_loader):
            if hasattr(loader, "set_epoch"):
                loader.set_epoch(epoch)
        train(train_loader, model, awp_adversary, criterion, optimizer, epoch, args, device, dirs["log"])
        prec1, _ = validate(val_loader, model, criterion, args, device, args.num_steps_2, args.step_size_1, dirs["log"])
        is_best = prec1 > best_prec1
        best_prec1 = max(prec1, best_prec1)
        fname, best = driver.checkpoint_names(args, dirs, epoch)  # experiments_cifar100_awp.py:249-268: the same names as the Tiny drivers'
        save_checkpoint({'epoch': epoch + 1, 'arch': args.arch, 'state_dict': model.state_dict(), 'best_prec1': best_prec1,
                         'optimizer': optimizer.state_dict()}, is_best, fname, best)
    return best_prec1


if __name__ == '__main__':
    main()
