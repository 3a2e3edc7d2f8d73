"""Shared machinery of the experiments_*.py drivers: the reference has three near-identical
400-line scripts (MNIST/experiments_mnist.py, Tiny_ImageNet/experiments_tinyimagenet.py,
ImageNet/experiments_imagenet.py); here each dataset script only declares what differs and calls `run`.

Kept surface: CLI flags, flat YAML keys merged under the CLI, `method_name` / `arch`
strings, the SGD + step-LR recipe, the checkpoint dict keys and file names, the output directory layout and the
exact log.txt line formats that utils/read_log.py parses.  Fixed while keeping the surface: missing
`type_canny` / `step_size_3` keys are tolerated, `--evaluate` runs the PGD evaluations instead of calling an
undefined function, DataParallel is replaced by one process per GPU (eeadv.ddp).

Data: `--data synthetic` (optionally `synthetic:<n_train_batches>:<n_val_batches>`, what the benchmark and most tests use) gives
seeded NCHW batches generated on the device.  A dataset directory is read by eeadv.data in place of the reference's
torchvision loaders (utils/data_loader.py) for the scripts whose SPEC names a "data" kind - Tiny-ImageNet, MNIST and ImageNet: each
split decoded once, cached as uint8, held on the device, one HIP launch per batch (ImageNet train: images of their own sizes,
RandomResizedCrop + flip in that launch; ImageNet val: Resize + CenterCrop applied once at decode).  The free-AT scripts stay
synthetic-only and refuse a directory.

A SPEC may list YAML keys that resize its problem under "yaml_sizes" (the ImageNet driver: num_classes, crop_size, resize_size;
absent keys keep the reference's 1000 / 224 / 256) - see `sized`.
"""
import argparse
import os
import time

import torch
import torch.optim as optim

from utils.helper import AverageMeter, adjust_learning_rate, adjust_learning_rate_1, parse_config_file, save_checkpoint, set_seed

from . import ddp, methods, runtime, trainer


def make_parser(description, default_data="synthetic", with_local_rank=False):
    """The reference's argparse block (experiments_tinyimagenet.py:28-46, experiments_imagenet.py:29-46)."""
    parser = argparse.ArgumentParser(description=description)
    parser.add_argument('--data', metavar='DIR', default=default_data, help='path to dataset, or synthetic[:train_batches[:val_batches]]')
    parser.add_argument('-c', '--config', default='configs.yml', type=str, metavar='Path', help='path to the config file (default: configs.yml)')
    parser.add_argument('--pretrained', dest='pretrained', action='store_true', help='use pre-trained model')
    parser.add_argument('--resume', default='', type=str, metavar='PATH', help='path to latest checkpoint, (default: None)')
    parser.add_argument('-e', '--evaluate', dest='evaluate', action='store_true', help='evaluate model on validation set')
    parser.add_argument('--attack_method', default='PGD', type=str, metavar='PATH', help='attack method in validation: PGD, FGSM, CW, APGD-CE, APGD-T, APGD (CE then T), Square, APGD+Square (CE, T, then Square), FAB-T, APGD+FAB+Square (CE, T, FAB-T, then Square, each on the whole batch) Cascade (the same four, each on the samples still robust, over the whole split), APGD-DLR, Rand (APGD-CE then APGD-DLR, every gradient averaged over --eot_iter forwards: for defences that redraw at every forward) or Cascade-Rand (the same two, APGD-DLR on the survivors only), APGD-L1-CE, APGD-L1-T or APGD-L1 (CE then T): APGD in the L1 threat model, radius --epsilon, FAB-U (untargeted FAB: one backward pass per class and iteration), FAB-L1-T or APGD-L1+FAB (CE, T, then FAB-T): FAB-T in the L1 threat model, FAB-L1-U (untargeted FAB in L1), Square-L1 or APGD-L1+FAB+Square (CE, T, FAB-T, then Square, each on the whole batch: the full L1 ensemble): Square in the L1 threat model, Custom (the reference\'s `custom` AutoAttack version: APGD-CE then untargeted FAB, each on the whole batch; with --apgd_restarts 2 --fab_restarts 2 the setting of its utils/aa.py) (default: PGD)')
    parser.add_argument('--eot_iter', default=None, type=int, help='forwards every APGD gradient is averaged over (EOT); default: 20 for Rand and Cascade-Rand, 1 for APGD-CE and APGD-DLR; the other attacks have no EOT and refuse a value above 1')
    parser.add_argument('--norm', default='Linf', type=str, help='threat model of the evaluation attack, radius --epsilon of the config: Linf (default) or L2; L2 exists for APGD-CE, APGD-T, APGD, APGD-DLR, Rand and Cascade-Rand and every other method refuses it')
    parser.add_argument('--square_queries', default=5000, type=int, help='forwards per sample of the Square attack at most (default: 5000); not the defence\'s n_queries')
    parser.add_argument('--fab_iters', default=100, type=int, help='iterations of FAB-T per target class, and of the one run of FAB-U / FAB-L1-U (default: 100)')
    parser.add_argument('--fab_restarts', default=1, type=int, help='runs of every FAB (FAB-T per target class, FAB-U, their L1 forms, the FAB stage of APGD+FAB+Square, APGD-L1+FAB, APGD-L1+FAB+Square and Cascade): the first from the clean point, every later one from a random point at distance min(best norm so far, epsilon) / 2, the best norm kept (default: 1); any other method refuses a value other than 1')
    parser.add_argument('--apgd_restarts', default=1, type=int, help='runs of every APGD (APGD-CE, APGD-DLR, APGD-T per target class, their L1 forms, the APGD stages of the composites, of Rand, Custom, Cascade and Cascade-Rand): the first from the start drawn as before, every later one on the whole batch from a fresh draw of the same distribution made on the device; a sample counts as fooled if any run fooled it (default: 1); any other method refuses a value other than 1')
    parser.add_argument('--no-cuda', action='store_true', default=False, help='disables CUDA training')
    parser.add_argument('--max-epochs', type=int, default=None, help='stop after this many epochs (smoke runs)')
    parser.add_argument('--output-root', default=None, help='where checkpoint_<DS>/ is created (default: cwd, as the reference)')
    if with_local_rank:
        parser.add_argument('--local_rank', type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    return parser


class SyntheticLoader:
    """len() batches of seeded U[0,1) images and uniform labels, generated once on the device."""

    def __init__(self, n_batches, batch_size, shape, num_classes, device, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.batches = []
        for _ in range(n_batches):
            x = torch.rand((batch_size,) + tuple(shape), generator=g)
            y = torch.randint(0, num_classes, (batch_size,), generator=g)
            self.batches.append((x.to(device), y.to(device)))

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


def data_source(data, spec):
    """"synthetic", or the dataset kind of spec["data"] when `data` is a directory of that kind's layout (eeadv.data.LAYOUTS);
    anything else raises before any work is done."""
    if str(data).startswith("synthetic"):
        return "synthetic"
    kind = spec.get("data")
    if kind is None:
        raise NotImplementedError(
            "--data %s: this script supports only --data synthetic[:train_batches[:val_batches]]; real Tiny-ImageNet and MNIST "
            "directories are read by experiments_tinyimagenet.py and experiments_mnist.py" % data)
    from . import data as D
    if not D.recognised(kind, data):
        raise NotImplementedError("--data %s is neither synthetic[:train_batches[:val_batches]] nor a %s directory: expected %s"
                                  % (data, kind, D.LAYOUTS[kind]))
    return kind


def sized(spec, args):
    """`spec` with the keys it lists under "yaml_sizes" taken from the YAML when present: num_classes, crop_size (the side of the
    batches, spec["shape"]) and resize_size (the val split's Resize before its CenterCrop, spec["resize"])."""
    spec = dict(spec)
    allowed = spec.get("yaml_sizes", ())
    if "num_classes" in allowed and args.get("num_classes") is not None:
        spec["num_classes"] = int(args.num_classes)
    if "crop_size" in allowed and args.get("crop_size") is not None:
        spec["shape"] = (spec["shape"][0], int(args.crop_size), int(args.crop_size))
    if "resize_size" in allowed and args.get("resize_size") is not None:
        spec["resize"] = int(args.resize_size)
    return spec


def make_loaders(args, spec, device, batch_size):
    kind = data_source(args.data, spec)
    if kind != "synthetic":
        from . import data as D
        return D.make_loaders(kind, args.data, spec, device, batch_size, args.seed)  # the same seed on every rank
    parts = str(args.data).split(":")
    n_train = int(parts[1]) if len(parts) > 1 else 4
    n_val = int(parts[2]) if len(parts) > 2 else 2
    seed = ddp.rank_seed(args.seed)
    return (SyntheticLoader(n_train, batch_size, spec["shape"], spec["num_classes"], device, 1000 + seed),
            SyntheticLoader(n_val, batch_size, spec["shape"], spec["num_classes"], device, 2000 + seed))


def output_dirs(args, spec):
    """experiments_tinyimagenet.py:146-159: cwd/checkpoint_<DS>/<method>/<arch>/<type_canny>-bs..-lr..-momentum..-wd..-seed../"""
    root = args.output_root or os.getcwd()
    d = (root + '/' + spec["ckpt_dir"] + '/' + str(args.method_name) + '/' + str(args.arch) + '/' + str(args.get("type_canny")) +
         '-bs' + str(args.batch_size) + '-lr' + str(args.lr) + '-momentum' + str(args.momentum) + '-wd' + str(args.weight_decay) +
         '-seed' + str(args.seed) + '/')
    dirs = {"root": d, "model": d + 'model_pth/', "best": d + 'best_model_pth/', "log": d + 'log/'}
    if ddp.rank() == 0:
        for k in ("log", "model", "best"):
            os.makedirs(dirs[k], exist_ok=True)
    return dirs


def checkpoint_names(args, dirs, epoch):
    """experiments_tinyimagenet.py:200-211 (the best-model name really lacks the '_' before 'r')."""
    tail = ('_canny_sigma' + str(args.sigma) + '_alpha' + str(args.alpha) + '-bs' + str(args.batch_size) + '-lr_' + str(args.lr) +
            '-w' + str(args.w) + '-gf' + str(args.gf) + '-l' + str(args.low) + '-h' + str(args.high))
    head = 'at_numstep' + str(args.num_steps_1) + '_epsilon' + str(int(args.epsilon * 255))
    return (dirs["model"] + head + '_r' + str(args.r) + tail + '_' + str(epoch) + '.pth', dirs["best"] + head + 'r' + str(args.r) + tail + '.pth')


def _log(line, log_dir):
    if ddp.rank() != 0:
        return
    print(line)
    with open(log_dir + 'log.txt', 'a') as f:
        print(line, file=f)


class _DeviceMeters:
    """AverageMeter semantics (val = last batch, avg = running mean) kept on the device: the reference calls
    .item() on every batch (experiments_tinyimagenet.py:299), here the host only syncs when it prints."""

    def __init__(self, n, device):
        self.sum = torch.zeros(n, dtype=torch.float64, device=device)
        self.last = torch.zeros(n, dtype=torch.float64, device=device)
        self.count = 0

    def update(self, values, n):
        self.last = torch.stack([v.reshape(()).to(torch.float64) for v in values])
        self.sum += self.last * n
        self.count += n

    def read(self):
        last, avg = self.last.tolist(), (self.sum / max(self.count, 1)).tolist()
        out = []
        for v, a in zip(last, avg):
            m = AverageMeter()
            m.val, m.avg = v, a
            out.append(m)
        return out


def train(train_loader, model, criterion, optimizer, epoch, args, device, log_dir, spec, sync=None):
    """experiments_tinyimagenet.py:215-323."""
    batch_time, data_time = AverageMeter(), AverageMeter()
    meters = _DeviceMeters(3, device)
    model.train()
    avmixup = None
    if args.method_name in ('AVmixup', 'tarAVmixup'):
        avmixup = trainer.A.AVmixup(args, gamma=2.0, lambda1=1.0, lambda2=0.1, step_size=args.step_size_1, num_steps=args.num_steps_1,
                                    num_classes=spec["num_classes"], device=device)
    add_square = None
    if "pre_square" in args.method_name:
        from utils.core import Add_Square
        add_square = Add_Square(channels=spec["shape"][0], size=args.cize, epsilon=args.epsilon, n_queries=args.n_queries)
    end = time.time()
    for i, (input, target) in enumerate(train_loader):
        target, input = target.to(device), input.to(device)
        data_time.update(time.time() - end)
        if add_square is not None:
            input = add_square(input).detach()
        loss, output = trainer.train_batch(model, criterion, optimizer, args, input, target, device, avmixup, sync=sync)
        prec1, prec5 = trainer.accuracy(output, target, topk=(1, min(5, spec["num_classes"])))
        if spec.get("mnist_top5_quirk"):
            prec5 = prec1  # MNIST/experiments_mnist.py:246 logs prec1 as top5 (visible in the shipped MNIST log)
        meters.update([loss, prec1, prec5], input.size(0))
        batch_time.update(time.time() - end)
        end = time.time()
        if i % args.print_freq == 0:
            losses, top1, top5 = meters.read()
            _log('Epoch: [{0}][{1}/{2}]\t'
                 'Time {batch_time.val:.3f} ({batch_time.avg:.3f})\t'
                 'Data {data_time.val:.3f} ({data_time.avg:.3f})\t'
                 'Loss {loss.val:.4f} ({loss.avg:.4f})\t'
                 'Prec@1 {top1.val:.3f} ({top1.avg:.3f})\t'
                 'Prec@5 {top5.val:.3f} ({top5.avg:.3f})\t'.format(epoch, i, len(train_loader), batch_time=batch_time, data_time=data_time,
                                                                  loss=losses, top1=top1, top5=top5), log_dir)


def strip_module_prefix(state):
    """DataParallel / DDP checkpoints (`module.`-prefixed keys, what the reference's MNIST / Tiny / free-AT scripts save) -> bare keys."""
    return {k[len("module."):] if k.startswith("module.") else k: v for k, v in state.items()}


def with_module_prefix(state):
    """Bare keys -> the `module.`-prefixed keys of a wrapped model's state_dict(): the reference's MNIST and Tiny drivers save
    nn.DataParallel(model).state_dict() (experiments_tinyimagenet.py:110,196) and its free-AT script the DDP model's
    (AT_free_imagenet_ddp.py:236); their --resume loads into the wrapped model and needs these names.  The ImageNet driver
    saves model.module.state_dict() (experiments_imagenet.py:206): bare keys."""
    return {("module." + k if not k.startswith("module.") else k): v for k, v in state.items()}


def load_model_checkpoint(model, path, device):
    """The weights of a checkpoint file into `model`: (the checkpoint dict, load_state_dict's report).  `module.`-prefixed keys are read as
    bare ones, and keys the model does not have are ignored - reference EE checkpoints carry dead sobel.* / u2netp.* keys."""
    ckpt = torch.load(path, map_location=device, weights_only=True)
    return ckpt, model.load_state_dict(strip_module_prefix(ckpt['state_dict']), strict=False)


def validate_cascade(val_loader, model, args, device, num_steps, n_class, log):
    """--attack_method Cascade / Cascade-Rand: eeadv.cascade.evaluate over the whole loader in place of the per-batch loop.  log(line) receives the clean
    accuracy and one `robust accuracy after <stage>` line per stage (percent of this rank's samples).  Returns the final robust accuracy
    twice, in the place of validate's (adv top-1, adv top-5), averaged over ranks."""
    from . import cascade
    if "tar" in args.method_name:
        raise NotImplementedError("--attack_method %s evaluates untargeted robustness only" % args.attack_method)
    model.eval()
    start = time.time()
    eot_iter, stages, tag = trainer.eot_iter_for(args), None, trainer.norm_tag(args)
    if trainer.apgd_restarts_for(args):
        log(' * APGD: {0} restarts per run, each on the whole batch of its stage'.format(int(args.apgd_restarts)))
    if trainer.fab_restarts_for(args):
        log(' * FAB-T: {0} restarts per target class, {1} iterations each'.format(int(args.fab_restarts), int(getattr(args, 'fab_iters', 100))))
    if args.attack_method == trainer.CASCADE_RAND_METHOD:
        if n_class < 3:
            raise ValueError("--attack_method Cascade-Rand runs APGD-DLR, which needs at least 3 classes, not %d" % n_class)
        stages = cascade.rand_stages(args, int(num_steps), eot_iter, trainer.norm_for(args))
    res = cascade.evaluate(model, args, val_loader, n_class, num_steps=num_steps, device=device, stages=stages)
    log(' * Cascade: {0} samples, {1} attacked rows per stage {2}, {3:.1f} s'.format(
        res.n, '/'.join(res.stage_names), '/'.join(str(r) for r in res.rows_attacked), time.time() - start) + tag)
    log(' * Cascade clean accuracy {0:.3f}'.format(100.0 * res.clean_correct / res.n))
    for name, left in zip(res.stage_names, res.robust_after):
        log(' * Cascade robust accuracy after {0} {1:.3f}'.format(name, 100.0 * left / res.n))
    last = 100.0 * (res.robust_after[-1] if res.robust_after else res.clean_correct) / res.n
    a1, = ddp.gather_mean(last)
    return a1, a1


def _restarts_tag(args):
    """What the FAB line of a validation log carries after its numbers: nothing for one restart (the line stays as it was)."""
    n = trainer.fab_restarts_for(args).get('n_restarts', 1)
    return '' if n == 1 else ', {0} restarts'.format(n)


def validate(val_loader, model, criterion, args, device, num_steps, step_size, log_dir, spec, local_result=False):
    """experiments_tinyimagenet.py:326-432.  Returns (adv top-1, adv top-5) averaged over ranks (the free-AT script returns
    its rank-local averages, AT_free_imagenet_ddp.py:403: local_result=True)."""
    if args.attack_method in trainer.CASCADE_METHODS:
        return validate_cascade(val_loader, model, args, device, num_steps, spec["num_classes"], lambda line: _log(line, log_dir))
    batch_time = AverageMeter()
    meters = _DeviceMeters(6, device)
    model.eval()
    add_square = None
    if "pre_square" in args.method_name:
        from utils.core import Add_Square
        add_square = Add_Square(channels=spec["shape"][0], size=args.cize, epsilon=args.epsilon, n_queries=args.n_queries)
    if trainer.apgd_restarts_for(args):
        _log(' * {0}: APGD, {1} restarts per run, each on the whole batch'.format(args.attack_method, int(args.apgd_restarts)), log_dir)
    if methods.runs(args.attack_method, methods.FAB_U_MEMBERS):
        # untargeted FAB takes one backward pass per class and iteration: say so before the first batch
        _log(' * {0}: K = {1} classes, {1} backward passes per iteration, {2} iterations'.format(
            args.attack_method, spec["num_classes"], int(getattr(args, 'fab_iters', 100))) + _restarts_tag(args), log_dir)
    elif trainer.fab_restarts_for(args):
        _log(' * {0}: FAB-T, {1} iterations per target class'.format(args.attack_method, int(getattr(args, 'fab_iters', 100))) + _restarts_tag(args), log_dir)
    end = time.time()
    for i, (input, target) in enumerate(val_loader):
        target, input = target.to(device), input.to(device)
        if add_square is not None:
            input = add_square(input).detach()
        vals = trainer.validate_batch(model, criterion, args, input, target, device, num_steps, step_size, spec["num_classes"])
        meters.update(list(vals), input.size(0))
        batch_time.update(time.time() - end)
        end = time.time()
        if i % args.print_freq == 0:
            lc, la, t1c, t5c, t1a, t5a = meters.read()
            fmt = ('{tag}: [{0}/{1}]\tTime {batch_time.val:.3f} ({batch_time.avg:.3f})\tLoss {loss.val:.4f} ({loss.avg:.4f})\t'
                   'Prec@1 {top1.val:.3f} ({top1.avg:.3f})\tPrec@5 {top5.val:.3f} ({top5.avg:.3f})')
            _log(fmt.format(i, len(val_loader), tag='Test_clean', batch_time=batch_time, loss=lc, top1=t1c, top5=t5c), log_dir)
            _log(fmt.format(i, len(val_loader), tag='Test_adv', batch_time=batch_time, loss=la, top1=t1a, top5=t5a), log_dir)
    lc, la, t1c, t5c, t1a, t5a = meters.read()
    c1, c5, a1, a5 = ddp.gather_mean(t1c.avg, t5c.avg, t1a.avg, t5a.avg)  # experiments_imagenet.py:369-384
    _log(' * Clean Prec@1 {0:.3f} Prec@5 {1:.3f}'.format(c1, c5), log_dir)
    _log(' * Adv Prec@1 {0:.3f} Prec@5 {1:.3f}'.format(a1, a5) + trainer.norm_tag(args), log_dir)
    if local_result:
        _log(' * Cl Prec@1 {top1.avg:.3f} Prec@5 {top5.avg:.3f}'.format(top1=t1c, top5=t5c), log_dir)  # AT_free_imagenet_ddp.py:400-401
        _log(' * Ad Prec@1 {top1.avg:.3f} Prec@5 {top5.avg:.3f}'.format(top1=t1a, top5=t5a), log_dir)
        return t1a.avg, t5a.avg
    return a1, a5


def run(spec, build_model, argv=None):
    """main() of the reference drivers (experiments_tinyimagenet.py:50-213)."""
    parser = make_parser(spec["description"], with_local_rank=spec.get("ddp", False))
    args = parse_config_file(parser.parse_args(argv))
    spec = sized(spec, args)
    data_source(args.data, spec)  # an unusable --data fails here, before a model is built
    trainer.eot_iter_for(args)  # so does an --eot_iter the chosen attack cannot honour
    trainer.norm_for(args)  # and a --norm it has no L2 for
    trainer.fab_restarts_for(args)  # and a --fab_restarts on a method that runs no FAB
    trainer.apgd_restarts_for(args)  # and an --apgd_restarts on a method that runs no APGD
    for key, default in (("type_canny", None), ("step_size_3", args.get("step_size_2")), ("num_steps_3", args.get("num_steps_2")),
                         ("n_queries", 1), ("cize", spec["shape"][-1]), ("beta", 1.0)):
        if key not in args:
            args[key] = default  # keys the reference reads unconditionally but several of its YAMLs omit
    args.num_classes = spec["num_classes"]
    args.crop_size = spec["shape"][-1]
    use_cuda = not args.no_cuda and torch.cuda.is_available()
    if use_cuda:
        torch.cuda.set_device(ddp.local_rank())
        device = torch.device("cuda", ddp.local_rank())
        # the attack iteration and the parameter update replay captured HIP graphs unless the user says otherwise: eagerly
        # the loop is bound by the host (one launch per ~10 us of Python + ctypes), 3-4x slower than the device can go
        # ... except under multi-rank SyncBatchNorm (the ImageNet scripts): every train-mode forward of the attack loop would put
        # RCCL all_gathers inside the captured graph, a combination that has not run on a multi-GPU node yet
        os.environ.setdefault("EEADV_GRAPH", "0" if (ddp.world() > 1 and spec.get("sync_bn", False)) else "1")
    else:
        device = torch.device("cpu")
        runtime.allow_cpu_plumbing(True)  # --no-cuda: torch-op plumbing run on the host (BASELINE config 1)
    ddp.setup(device)
    set_seed(ddp.rank_seed(args.seed))

    print("=> creating model '{}'".format(args.arch))
    model = build_model(args).to(device)
    # N > 1: the bare model + one flat gradient buffer all-reduced per step (ddp.FlatGradSync) instead of DistributedDataParallel
    # (experiments_imagenet.py:125-129): same averaged gradients, and the update stays capturable as HIP graphs
    if ddp.world() > 1 and spec.get("sync_bn", False):
        model = ddp.convert_sync_batchnorm(model)
    # (EEADV_GRAD_SYNC=ddp: DistributedDataParallel + the eager update instead - ddp.grad_sync_mode)
    net, sync = ddp.make_grad_sync(model, device if use_cuda else None)
    if use_cuda:
        torch.backends.cudnn.benchmark = False  # experiments_tinyimagenet.py:111-112
        torch.backends.cudnn.deterministic = True
    optimizer = trainer.make_sgd(net.parameters(), lr=args.lr, momentum=args.momentum, weight_decay=args.weight_decay)
    criterion = trainer.make_criterion(args)
    best_prec1 = 0.0
    if args.resume:
        if os.path.isfile(args.resume):
            print("=> loading checkpoint '{}'".format(args.resume))
            ckpt, missing = load_model_checkpoint(model, args.resume, device)
            args.start_epoch, best_prec1 = ckpt['epoch'], ckpt['best_prec1']
            print("=> loaded checkpoint '{}' (epoch {}); ignored keys: {}".format(args.resume, ckpt['epoch'], len(missing.unexpected_keys)))
            optimizer.load_state_dict(ckpt['optimizer'])
        else:
            print("=> no checkpoint found at '{}'".format(args.resume))

    batch = ddp.per_rank_batch(args.batch_size) if spec.get("ddp", False) else args.batch_size
    train_loader, val_loader = make_loaders(args, spec, device, batch)
    dirs = output_dirs(args, spec)
    print("Output dir:" + dirs["root"])
    schedule = spec.get("lr_schedule", "half_three_quarters")

    if args.evaluate:
        if sync is not None:
            sync.broadcast_buffers()
        if hasattr(val_loader, "set_epoch"):
            val_loader.set_epoch(args.start_epoch)
        for k, s in ((args.num_steps_1, args.step_size_1), (args.num_steps_2, args.step_size_2), (args.num_steps_3, args.step_size_3)):
            print("=> evaluate.tar_num_step:{},step_size:{}".format(k, s))
            validate(val_loader, net, criterion, args, device, k, s, dirs["log"], spec)
        ddp.teardown()
        return

    last_epoch = args.epochs if args.max_epochs is None else min(args.epochs, args.start_epoch + args.max_epochs)
    for epoch in range(args.start_epoch, last_epoch):
        if schedule == "step30":
            adjust_learning_rate(optimizer, epoch, args.lr)  # experiments_imagenet.py
        else:
            adjust_learning_rate_1(optimizer, epoch, args.lr, args.epochs)
        for loader in (train_loader, val_loader):
            if hasattr(loader, "set_epoch"):
                loader.set_epoch(epoch)  # the epoch's order and flips (eeadv.data.DeviceLoader): --resume at epoch k replays epoch k's
        train(train_loader, net, criterion, optimizer, epoch, args, device, dirs["log"], spec, sync)
        if sync is not None:
            sync.broadcast_buffers()  # rank 0's BatchNorm statistics are the model's, as under DistributedDataParallel
        prec1, _ = validate(val_loader, net, criterion, args, device, args.num_steps_1, args.step_size_1, dirs["log"], spec)
        is_best = prec1 > best_prec1
        best_prec1 = max(prec1, best_prec1)
        if ddp.rank() == 0:
            fname, best = checkpoint_names(args, dirs, epoch)
            state = with_module_prefix(model.state_dict()) if spec.get("ckpt_module_prefix", False) else model.state_dict()
            save_checkpoint({'epoch': epoch + 1, 'arch': args.arch, 'state_dict': state, 'best_prec1': best_prec1,
                             'optimizer': optimizer.state_dict()}, is_best, fname, best)
    ddp.teardown()
    return best_prec1
