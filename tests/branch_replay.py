"""The ResNet body in fp32 and the stock modules in float64 ON THE SAME PIECEWISE-LINEAR BRANCH (shared by the -m gpu tests).

The gradient of a ReLU network is discontinuous in its pre-activations: of the ~3 M of them in ResNet-18 at batch 16 about one lies within
fp32 rounding of zero, its mask differs between ANY two implementations, and one flipped mask of a late layer moves the whole gradient by
0.2 - 0.7 % of its norm.  A comparison that is to tell a rounding difference from a wrong term therefore records, during the fp32 run, every
ReLU mask and the stem max-pool's argmax, and makes the float64 run take exactly those.  Three recorders cover every way the body forms a
ReLU:

  models.bn_act / models.block_tail   the BatchNorm+ReLU launches and the block ends: the mask is `output > 0`;
  ops.wino3x3_bn_train_pre            the mid-block BatchNorm whose batch statistics cross the kernel boundary inside the attack loop
                                      (functional.TrainConvBnConvFn / TrainPairBnConvFn): relu(bn1(conv1 x)) is never materialised, but
                                      ee_fuse.hpp stages relu((v - mean) * (invstd * gamma) + beta), every operation rounded on its own
                                      (-ffp-contract=off), so the same fp32 torch expression on the kernel's arguments and its saved
                                      statistics gives the mask bit for bit;
  ops.bn_relu_pool_fwd                the one-pass stem: maxpool(relu(z)) == relu(maxpool(z)), so `y > 0` is the ReLU mask at each window's
                                      argmax and the one-byte `code` names its position; the float64 side gathers bn1(conv1 x) there.

The EVAL-mode attack route (Branch(..., eval_route=True)) forms its ReLUs in two more places, inside functional.EvalBasicBlockFn /
EvalDownBlockFn, where models.bn_act and models.block_tail never run:

  functional._eval_conv_fwd           returns relu(bn(conv x) [+ res]): the mask is `output > 0` (bn1's ReLU, or the block's end);
  ops.conv3x3s2_pair_bn_eval_fwd      the first output carries bn1's ReLU (`output > 0`); the second, the shortcut's BatchNorm, has none.

Their forward order is the stock path's - one bn_act behind conv1, one block_tail per block - so replay() consumes them unchanged.
"""
import torch
import torch.nn.functional as F

DEV = "cuda:0"
ALL_STOCK = frozenset(("bn", "pool", "head", "conv", "stem", "dense", "conv3", "conv3s2"))
N_RELU = {18: 17, 50: 49}


def move_batchnorms(net, seed):
    """every BatchNorm away from its initial (mean 0, variance 1, weight 1, bias 0), drawn as test_gpu_evalfuse._resnet draws them: eval mode
    reads the running statistics, and the initial state cannot tell `invstd * gamma` from `gamma` or see a missing beta"""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in net.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                dev, n = mod.weight.device, mod.num_features
                mod.running_mean.copy_((torch.randn(n, generator=gen) * 0.1).to(dev))
                mod.running_var.copy_((torch.rand(n, generator=gen) + 0.5).to(dev))
                mod.weight.copy_((torch.rand(n, generator=gen) + 0.5).to(dev))
                mod.bias.copy_((torch.randn(n, generator=gen) * 0.1).to(dev))
    return net


def make_net(models, depth, stock, dt=torch.float32, monkeypatch=None, train=True):
    """make_resnet(depth, 'tiny') from seed 21 in train mode (train=False: in eval mode, every BatchNorm moved away from its initial state
    first - move_batchnorms, seed 21), with models._STOCK = stock from here on: until the test ends when `monkeypatch` is given, otherwise
    until the caller puts it back"""
    if monkeypatch is not None:
        monkeypatch.setattr(models, "_STOCK", stock)
    else:
        models._STOCK = stock
    torch.manual_seed(21)
    net = models.make_resnet(depth, "tiny").to(DEV)
    if not train:
        move_batchnorms(net, 21)
    net = net.to(dt)
    return net.train() if train else net.eval()


def body_run(models, depth, x, dl, stock, dt=torch.float32, monkeypatch=None):
    """one forward + backward of make_resnet(depth, 'tiny') from seed 21 in train mode -> (names, logits, gradients of input and parameters, net)"""
    net = make_net(models, depth, stock, dt, monkeypatch)
    xi = x.to(dt).requires_grad_(True)
    logits = net(xi)
    grads = torch.autograd.grad(logits, [xi] + list(net.parameters()), dl.to(dt))
    return ["input"] + [n for n, _ in net.named_parameters()], logits.detach(), grads, net


def pool_code_to_index(code, W):
    """flat index (h * W + w) into the [H, W] plane of the position each one-byte argmax code of the 3x3 / stride 2 / padding 1 pool names"""
    OH, OW = code.shape[2], code.shape[3]
    oh, ow = torch.meshgrid(torch.arange(OH, device=code.device), torch.arange(OW, device=code.device), indexing="ij")
    hh = (2 * oh - 1)[None, None] + (code.long() // 3)
    ww = (2 * ow - 1)[None, None] + (code.long() % 3)
    return hh * W + ww


def train_pre_mask(c1, sm, si, gamma, beta):
    """the ReLU mask ee_fuse.hpp's train_bn_apply / train_bn_bwd_apply open, as the fp32 torch expression of the same association"""
    sh = (1, -1, 1, 1)
    scale = si if gamma is None else si * gamma
    z = (c1 - sm.view(sh)) * scale.view(sh)
    return (z if beta is None else z + beta.view(sh)) > 0


class Branch:
    """record() during the fp32 run, replay() during the float64 run, restore() afterwards.  `masks` holds, in forward order, one entry per
    ReLU: an activation or a boolean mask, or ("stem", y > 0, argmax index) for the one-pass stem.  `calls` counts what the recorders saw.
    eval_route: also record the two places where the eval-mode attack route forms a ReLU (`calls` then has "eval_conv" and "eval_pair")."""

    def __init__(self, monkeypatch, models, eval_route=False):
        from eeadv import functional, ops
        self.mp, self.models, self.ops, self.fn, self.eval_route = monkeypatch, models, ops, functional, eval_route
        self.orig = {"bn_act": models.bn_act, "block_tail": models.block_tail, "stem_pool": models.stem_pool, "stem_bn_pool": models.stem_bn_pool,
                     "train_pre": ops.wino3x3_bn_train_pre, "pool_fwd": ops.bn_relu_pool_fwd, "ce_head": ops.ce_pool_linear_bwd}
        self.masks, self.calls = [], {"train_pre": 0, "pool_fwd": 0, "pool_fwd_xa": 0, "ce_head": 0}
        if eval_route:
            self.orig.update(eval_conv=functional._eval_conv_fwd, eval_pair=ops.conv3x3s2_pair_bn_eval_fwd)
            self.calls.update(eval_conv=0, eval_pair=0)

    def record(self):
        masks, calls, nested, o = self.masks, self.calls, [0], self.orig
        first = lambda t: t[0] if isinstance(t, tuple) else t

        def rec_bn_act(bn, x, residual=None, relu=True, fork=False):
            out = o["bn_act"](bn, x, residual, relu, fork)
            if relu and not nested[0]:
                masks.append(first(out).detach().clone())
            return out

        def rec_tail(*a, **k):  # the last ReLU of a block, however block_tail gets there (BnDualFn, or bn_act around the shortcut)
            nested[0] += 1
            try:
                out = o["block_tail"](*a, **k)
            finally:
                nested[0] -= 1
            masks.append(first(out).detach().clone())
            return out

        def rec_train_pre(x, stats, cnt, gamma, beta, eps, momentum, running_mean, running_var, u):
            out = o["train_pre"](x, stats, cnt, gamma, beta, eps, momentum, running_mean, running_var, u)
            masks.append(train_pre_mask(x, out[1], out[2], gamma, beta))
            calls["train_pre"] += 1
            return out

        def rec_pool_fwd(x, *a, **k):
            out = o["pool_fwd"](x, *a, **k)
            masks.append(("stem", out[0] > 0, pool_code_to_index(out[1], x.shape[3])))
            calls["pool_fwd"] += 1
            calls["pool_fwd_xa"] += int(len(out) == 5)
            return out

        def rec_ce_head(*a, **k):
            calls["ce_head"] += 1
            return o["ce_head"](*a, **k)

        def rec_eval_conv(x, w, bn, res):  # relu(bn(conv x) [+ res]): bn1's ReLU, or the block's end
            out = o["eval_conv"](x, w, bn, res)
            masks.append(out.detach().clone())
            calls["eval_conv"] += 1
            return out

        def rec_eval_pair(*a, **k):  # (relu(bn1(conv3x3s2 x)), bn_ds(conv1x1s2 x)): the second output has no ReLU
            out = o["eval_pair"](*a, **k)
            masks.append(out[0].detach().clone())
            calls["eval_pair"] += 1
            return out
        if self.eval_route:
            self.mp.setattr(self.fn, "_eval_conv_fwd", rec_eval_conv)
            self.mp.setattr(self.ops, "conv3x3s2_pair_bn_eval_fwd", rec_eval_pair)
        self.mp.setattr(self.models, "bn_act", rec_bn_act)
        self.mp.setattr(self.models, "block_tail", rec_tail)
        self.mp.setattr(self.ops, "wino3x3_bn_train_pre", rec_train_pre)
        self.mp.setattr(self.ops, "bn_relu_pool_fwd", rec_pool_fwd)
        self.mp.setattr(self.ops, "ce_pool_linear_bwd", rec_ce_head)

    def stop(self):
        """the recorders off, nothing replayed (the kernels' own entry points again)"""
        self.mp.setattr(self.models, "bn_act", self.orig["bn_act"])
        self.mp.setattr(self.models, "block_tail", self.orig["block_tail"])
        self.mp.setattr(self.ops, "wino3x3_bn_train_pre", self.orig["train_pre"])
        self.mp.setattr(self.ops, "bn_relu_pool_fwd", self.orig["pool_fwd"])
        self.mp.setattr(self.ops, "ce_pool_linear_bwd", self.orig["ce_head"])
        if self.eval_route:
            self.mp.setattr(self.fn, "_eval_conv_fwd", self.orig["eval_conv"])
            self.mp.setattr(self.ops, "conv3x3s2_pair_bn_eval_fwd", self.orig["eval_pair"])

    def replay(self):
        """-> the list of masks still to be consumed (empty after a float64 run that met every ReLU of the fp32 one)"""
        self.stop()
        masks, o = self.masks, self.orig
        todo = list(masks)

        def replay_bn_act(bn, x, residual=None, relu=True, fork=False):
            out = bn(x)
            if residual is not None:
                out = out + residual
            return out * (todo.pop(0) > 0).to(out.dtype) if relu else out

        def replay_pool(pool, x64):  # ATen's first-maximum rule on the fp32 activations (ee_pool.hip is bit-identical to it), applied to the float64 ones
            idx = F.max_pool2d(masks[0], 3, 2, 1, return_indices=True)[1]
            return x64.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)

        def replay_stem(bn, pool, x, fork=False, conv_stats=None):
            if todo and isinstance(todo[0], tuple):  # the one-pass stem: bn1's output at the fp32 run's argmax, gated by its pooled ReLU mask
                _, keep, idx = todo.pop(0)
                return bn(x).flatten(2).gather(2, idx.flatten(2)).view(idx.shape) * keep.to(x.dtype)
            return o["stem_bn_pool"](bn, pool, x, fork, conv_stats)
        self.mp.setattr(self.models, "bn_act", replay_bn_act)
        self.mp.setattr(self.models, "stem_pool", replay_pool)
        self.mp.setattr(self.models, "stem_bn_pool", replay_stem)
        return todo

    def restore(self):
        self.stop()
        self.mp.setattr(self.models, "stem_pool", self.orig["stem_pool"])
        self.mp.setattr(self.models, "stem_bn_pool", self.orig["stem_bn_pool"])


def replayed_body_gradients(monkeypatch, depth, B, seed, fp32_stock=frozenset(("bnpool",))):
    """The fused ResNet body in fp32, and the stock modules in float64 ON THE SAME PIECEWISE-LINEAR BRANCH: every ReLU mask and the stem
    max-pool's argmax of the float64 run are the ones the fp32 run took.

    Why: the gradient of a ReLU network is discontinuous in its pre-activations.  Of the ~3 M of them in ResNet-18 at batch 16 about one
    lies within fp32 rounding of zero, its mask differs between ANY two implementations (fp32 stock against float64 too), and one flipped
    mask on a 2x2 map of layer 4 moves the whole gradient by 0.2 - 0.7 % of its norm (scripts/fused_vs_stock_diag.py: the fused path is off
    by 2.4e-6 of the norm on inputs without a flip and by 1.5e-3 ... 3.9e-3 on the others; the all-MIOpen path the same, at random from run
    to run).  Holding the branch fixed leaves the arithmetic of the kernels, which is what this compares.
    The stem runs as its two kernels here by default (BatchNorm+ReLU, then the max-pool); with fp32_stock = frozenset() it is the one-pass
    kernel, whose branch the ops.bn_relu_pool_fwd recorder takes from the pooled output and the argmax code."""
    from eeadv import models
    g = torch.Generator(device="cpu").manual_seed(seed)
    x, dl = torch.rand(B, 3, 64, 64, generator=g).to(DEV), torch.randn(B, 200, generator=g).to(DEV)
    br = Branch(monkeypatch, models)
    br.record()
    names, logits32, g32, _ = body_run(models, depth, x, dl, fp32_stock, monkeypatch=monkeypatch)
    n_relu = len(br.masks)
    todo = br.replay()
    _, logits64, g64, _ = body_run(models, depth, x, dl, ALL_STOCK, torch.float64, monkeypatch)
    assert not todo and n_relu == N_RELU[depth]
    br.restore()
    return names, logits32, g32, logits64, g64


class LogitCotangent:
    """an engine loss spec whose d loss / d logits is a given tensor: its `kind` is no cross-entropy kind, so engine._body_input_grad takes
    the branch APGD's DLR loss and FAB's logit differences take - model(x) under attack_forward(), then PoolLinearFn's backward"""
    kind, payload = "cotangent", None

    def __init__(self, dl):
        self.dl = dl

    def dlogits(self, logits):
        assert logits.shape == self.dl.shape
        return self.dl


def replayed_attack_gradient(monkeypatch, B, seed, kind="ce_sum", fp32_stock=frozenset(), affine_seed=None, mode="train", cotangent=None):
    """ResNet-18's INPUT gradient on the route the attack loop takes - engine.input_gradient in train mode, i.e. body_pre under
    functional.attack_forward() and ResNet.head_grad - and the float64 stock modules on the branch that run took, differentiating
    F.cross_entropy(logits64, y, reduction = sum | mean) with respect to the input.  affine_seed: every BatchNorm's weight drawn from
    U(0.5, 1.5) and its bias from N(0, 0.2^2) first - a freshly initialised model has bias 0, where `invstd * gamma` in a ReLU mask
    (x - mean) * (invstd * gamma) + beta > 0 could be any positive number without a test noticing.
    mode="eval": the model in eval mode (make_net(train=False): every BatchNorm moved away from its initial state), the recorders of the
    eval route on.  cotangent: dl [B, 200] - the gradient of <logits, dl> instead of the cross-entropy's, through LogitCotangent on the fp32
    side and torch.autograd.grad(logits64, x64, dl.double()) on the float64 side (`kind` is then unused).
    models._STOCK is left at fp32_stock until the test ends (monkeypatch restores it).
    -> dict(x, y, net32 (after its one forward), twin (a deep copy of net32 from before it), net64, g32, g64, logits64, calls, n_relu, spec)"""
    import copy
    from eeadv import engine, models
    assert mode in ("train", "eval")
    train = mode == "train"
    g = torch.Generator(device="cpu").manual_seed(seed)
    x, y = torch.rand(B, 3, 64, 64, generator=g).to(DEV), torch.randint(0, 200, (B,), generator=g).to(DEV)
    net32 = make_net(models, 18, fp32_stock, monkeypatch=monkeypatch, train=train)
    if affine_seed is not None:
        ga = torch.Generator(device="cpu").manual_seed(affine_seed)
        with torch.no_grad():
            for m in net32.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.weight.copy_(torch.rand(m.weight.shape, generator=ga) + 0.5)
                    m.bias.copy_(torch.randn(m.bias.shape, generator=ga) * 0.2)
    twin = copy.deepcopy(net32)
    spec = engine.LossSpec(kind, y) if cotangent is None else LogitCotangent(cotangent)
    br = Branch(monkeypatch, models, eval_route=not train)
    br.record()
    g32 = engine.input_gradient(net32, x.clone(), spec).detach()
    n_relu = len(br.masks)
    todo = br.replay()
    net64 = make_net(models, 18, ALL_STOCK, torch.float64, monkeypatch, train=train)
    net64.load_state_dict(twin.state_dict())
    x64 = x.double().requires_grad_(True)
    logits64 = net64(x64)
    if cotangent is None:
        (g64,) = torch.autograd.grad(F.cross_entropy(logits64, y, reduction="sum" if kind == "ce_sum" else "mean"), x64)
    else:
        (g64,) = torch.autograd.grad(logits64, x64, cotangent.double())
    assert not todo and n_relu == N_RELU[18], (len(todo), n_relu)
    br.restore()
    monkeypatch.setattr(models, "_STOCK", fp32_stock)  # what net32 and its twin run under; monkeypatch puts the session's value back
    return dict(x=x, y=y, net32=net32, twin=twin, net64=net64, g32=g32, g64=g64, logits64=logits64.detach(), calls=br.calls, n_relu=n_relu, spec=spec)
