"""Pre-activation ResNets of the AWP sub-project, restated for PyTorch-ROCm on the HIP kernels.

  PreActBlock / PreActBottleneck / PreActResNet : AWP/Tiny_imagenet/models_tiny_awp/preactresnet.py:12-156
  PreActResNet_EE (+ _BPDA, _BPDA_3)             : preactresnet_EE.py:70-187 (the same with CannyFilter_BPDA / CannyFilter_step125_1)

State-dict keys, construction order and initialisation (PyTorch's defaults: the reference's init loop is commented out) are the
reference's, so a seed gives the same weights and checkpoints load both ways.  PreActResNet builds only dataset="Tiny-ImageNet" (7x7 / 2
stem + BatchNorm + ReLU + max-pool, then 16x16, 8x8, 4x4 and 2x2 maps at 64x64 inputs - exactly the map sizes of eeadv.models.ResNet).

  PreActResNetCifar : AWP/Cifar100/models_cifar100_awp/preactresnet.py:67-154 with dataset "CIFAR10" / "CIFAR100" (make_preact_cifar)
The CIFAR stem is a bare 3x3 / 1 convolution into layer1 and the head is AvgPool2d(4, stride=1) + `linear`.  At 32x32 inputs the stem and
layer1 work on 32x32 maps, which no kernel of csrc/ takes: those convolutions are MIOpen's (models.conv3 routes them), and the glue
around them is fused wherever its own predicate accepts the shape.  layer2 - layer4 see 16x16, 8x8 and 4x4 maps and run as the Tiny model's
layers 1 - 3 do; the final 4x4 map makes the pool global, so the head is ee_head.hip's.

A pre-activation block ends with a bare `out += shortcut`; the next block begins with relu(bn1(out)) and takes the raw sum as its identity
input.  Here a block hands its output on UN-ADDED, as the pending pair (conv2 output, shortcut), and whoever consumes it - the next
block's bn1, or the final relu(self.bn(out)) - resolves the pair with ONE launch each way (functional.BnSumActFn, ee_bn_sum_act_*): the
add, the BatchNorm and the ReLU forward, and backward the BatchNorm gradient plus the identity branch's, stored once for both summands.
EEADV_STOCK_GLUE=preact resolves it with the add + bn_act instead (A/B runs).
"""
import torch.nn as nn

from utils.core import CannyFilter, CannyFilter_BPDA, CannyFilter_step125_1

from . import ops
from .functional import BnSumActFn
from .models import (BatchNorm2d, _EEFrontMixin, _HEAD_CE, _STOCK, _bump_bn_counters, _dense_f32, _head_is_fused, _route, bn_act, conv1x1s2, conv3,
                     conv_s2_pair, head, stem_bn_pool, stem_conv, train_conv_bn_conv)


class _Sum(tuple):
    """(x, res) of a block output not added yet: the block's value is x + res"""


def _sum_fused(bn, x, res):
    return ("preact" not in _STOCK and "bn" not in _STOCK and type(bn) is BatchNorm2d and bn.affine and bn.track_running_stats
            and _dense_f32(x) and _dense_f32(res) and x.shape == res.shape and ops.bn_sum_act_supported(x))


def boundary_report(model):
    """{BatchNorm module name: route} of the block boundaries the last forward resolved: "ee_bn.sum_act" (BnSumActFn, one launch each way)
    or "add+bn_act" (EEADV_STOCK_GLUE=preact, or a shape the kernels do not take)"""
    return {name: m.__dict__["_ee_boundary"] for name, m in model.named_modules() if "_ee_boundary" in m.__dict__}


def resolve(bn, p, want_sum):
    """(relu(bn(v)), v) for a block input v: a pending pair (one launch: BnSumActFn), the forked stem output (two tensors over one buffer,
    one per consumer) or a plain tensor.  want_sum=False: the second item may be None (nobody reads the sum)."""
    if isinstance(p, _Sum):
        x, res = p
        fused = _sum_fused(bn, x, res)
        bn.__dict__["_ee_boundary"] = "ee_bn.sum_act" if fused else "add+bn_act"
        if fused:
            out = BnSumActFn.apply(x, res, bn.weight, bn.bias, bn.running_mean, bn.running_var, 0.0 if bn.momentum is None else bn.momentum,
                                   bn.eps, bn.training, True, want_sum)
            return out if want_sum else (out, None)
        s = x + res
        return bn_act(bn, s), s
    if isinstance(p, tuple):
        return bn_act(bn, p[0]), p[1]
    return bn_act(bn, p), p


def _conv1x1s2(cv, x):
    """the 1x1 shortcut convolution: stride 2 on ee_conv.hip where it takes the shape (models.conv1x1s2), MIOpen otherwise"""
    sc = conv1x1s2(cv, x)
    return _route(cv, "miopen")(x) if sc is None else sc


class PreActBlock(nn.Module):
    '''Pre-activation version of the BasicBlock.'''
    expansion = 1

    def __init__(self, in_planes, planes, stride=1):
        super(PreActBlock, self).__init__()
        self.bn1 = BatchNorm2d(in_planes)
        self.conv1 = nn.Conv2d(in_planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=1, padding=1, bias=False)

        if stride != 1 or in_planes != self.expansion*planes:
            self.shortcut = nn.Sequential(
                nn.Conv2d(in_planes, self.expansion*planes, kernel_size=1, stride=stride, bias=False)
            )

    def pending(self, p):
        """this block on a block input p (see resolve) -> the pending pair (conv2 output, shortcut)"""
        sc_conv = self.shortcut[0] if hasattr(self, 'shortcut') else None
        a, s = resolve(self.bn1, p, want_sum=sc_conv is None)
        mid = train_conv_bn_conv(self.training, self.bn2, self.conv1, self.conv2, sc_conv, a)
        if mid is not None:  # the attack loop in train mode: bn2's batch statistics across the kernel boundary (models.train_mid_bn)
            return _Sum((mid[0], s if sc_conv is None else mid[1]))
        both = conv_s2_pair(self.conv1, sc_conv, a) if sc_conv is not None else None
        if both is not None:  # the 3x3 / 2 and the 1x1 / 2 shortcut both read a: one launch each way
            out, sc = both
        else:
            out = conv3(self.conv1, a)
            sc = s if sc_conv is None else _conv1x1s2(sc_conv, a)
        return _Sum((conv3(self.conv2, bn_act(self.bn2, out)), sc))

    def forward(self, x):
        x, res = self.pending(x)
        return x + res


class PreActBottleneck(nn.Module):
    '''Pre-activation version of the original Bottleneck module.'''
    expansion = 4

    def __init__(self, in_planes, planes, stride=1):
        super(PreActBottleneck, self).__init__()
        self.bn1 = BatchNorm2d(in_planes)
        self.conv1 = nn.Conv2d(in_planes, planes, kernel_size=1, bias=False)

        self.bn2 = BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)

        self.bn3 = BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, self.expansion*planes, kernel_size=1, bias=False)

        if stride != 1 or in_planes != self.expansion*planes:
            self.shortcut = nn.Sequential(
                nn.Conv2d(in_planes, self.expansion*planes, kernel_size=1, stride=stride, bias=False)
            )

    def pending(self, p):
        """the bottleneck's 1x1 convolutions stay on MIOpen (models.conv1 routes); its boundaries resolve as PreActBlock's"""
        has_sc = hasattr(self, 'shortcut')
        a, s = resolve(self.bn1, p, want_sum=not has_sc)
        sc = _conv1x1s2(self.shortcut[0], a) if has_sc else s
        out = _route(self.conv1, "miopen")(a)
        out = conv3(self.conv2, bn_act(self.bn2, out))
        out = _route(self.conv3, "miopen")(bn_act(self.bn3, out))
        return _Sum((out, sc))

    def forward(self, x):
        x, res = self.pending(x)
        return x + res


class PreActResNet(nn.Module):
    _linear = "fc"  # the attribute name of the final nn.Linear (a state-dict key of the reference)

    def __init__(self, block, num_blocks, num_classes=10, dataset="Tiny-ImageNet"):
        super(PreActResNet, self).__init__()
        self._build_cnn(block, num_blocks, dataset)

    def _build_cnn(self, block, num_blocks, dataset):
        if dataset != "Tiny-ImageNet":
            raise NotImplementedError("dataset=%r: only the Tiny-ImageNet PreActResNets (7x7 / 2 stem, 200 classes) are built" % (dataset,))
        self.in_planes = 64
        self.dataset = dataset
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        num_classes = 200

        self.layer1 = self._make_layer(block, 64, num_blocks[0], stride=1)
        self.layer2 = self._make_layer(block, 128, num_blocks[1], stride=2)
        self.layer3 = self._make_layer(block, 256, num_blocks[2], stride=2)
        self.layer4 = self._make_layer(block, 512, num_blocks[3], stride=2)
        self.bn = BatchNorm2d(512 * block.expansion)

        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(512 * block.expansion, num_classes)

    def _make_layer(self, block, planes, num_blocks, stride):
        strides = [stride] + [1]*(num_blocks-1)
        layers = []
        for stride in strides:
            layers.append(block(self.in_planes, planes, stride))
            self.in_planes = planes * block.expansion
        return nn.Sequential(*layers)

    def body_pre(self, x):
        """relu(self.bn(layer4 output)): the classifier without its pooled linear head (engine fuses that with the loss gradient)"""
        x, moments = stem_conv(self.conv1, x, want_stats=True)
        # the stem output feeds layer1's first bn1 AND its identity branch: a forked pair, the two gradients added inside the stem's backward
        p = stem_bn_pool(self.bn1, self.maxpool, x, fork=True, conv_stats=moments)
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer:
                p = blk.pending(p)
        feat, _ = resolve(self.bn, p, want_sum=False)
        _bump_bn_counters(self)
        return feat

    def head_from_pre(self, feat):
        return head(self.avgpool, getattr(self, self._linear), feat)

    def head_grad(self, feat, labels, reduction):
        """d CrossEntropyLoss(head(feat), labels) / d feat through ee_head.hip (models.ResNet.head_grad), or None"""
        fc = getattr(self, self._linear)
        if not _HEAD_CE or not _head_is_fused(self.avgpool, fc, feat):
            return None
        feat = feat.contiguous()
        logits, _ = ops.pool_linear_fwd(feat, fc.weight.detach(), None if fc.bias is None else fc.bias.detach())
        return ops.ce_pool_linear_bwd(logits, labels, fc.weight.detach(), tuple(feat.shape), reduction)

    def body(self, x):
        return self.head_from_pre(self.body_pre(x))

    def forward(self, x):
        return self.body(x)


class PreActResNetCifar(PreActResNet):
    """The reference's PreActResNet with dataset "CIFAR10" / "CIFAR100" (AWP/Cifar100/models_cifar100_awp/preactresnet.py:74-81, 103-105,
    128-149): conv1 3x3 / 1 straight into layer1 (no bn1, relu, maxpool), AvgPool2d(4, stride=1), `linear` with 10 / 100 outputs."""
    _linear = "linear"
    _CLASSES = {"CIFAR10": 10, "CIFAR100": 100}

    def _build_cnn(self, block, num_blocks, dataset):
        if dataset not in self._CLASSES:
            raise NotImplementedError("dataset=%r: the CIFAR PreActResNets take CIFAR10 or CIFAR100 (Tiny-ImageNet: make_preact)" % (dataset,))
        self.in_planes = 64
        self.dataset = dataset
        self.conv1 = nn.Conv2d(3, 64, kernel_size=3, stride=1, padding=1, bias=False)

        self.layer1 = self._make_layer(block, 64, num_blocks[0], stride=1)
        self.layer2 = self._make_layer(block, 128, num_blocks[1], stride=2)
        self.layer3 = self._make_layer(block, 256, num_blocks[2], stride=2)
        self.layer4 = self._make_layer(block, 512, num_blocks[3], stride=2)
        self.bn = BatchNorm2d(512 * block.expansion)

        self.avgpool = nn.AvgPool2d(4, stride=1)
        self.linear = nn.Linear(512 * block.expansion, self._CLASSES[dataset])

    def body_pre(self, x):
        """relu(self.bn(layer4 output)); the stem's output is layer1's block input as it is (a plain tensor: resolve's third case)"""
        p = conv3(self.conv1, x)
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer:
                p = blk.pending(p)
        feat, _ = resolve(self.bn, p, want_sum=False)
        _bump_bn_counters(self)
        return feat


class PreActResNet_EE(_EEFrontMixin, PreActResNet):
    """x -> clamp(hfs(x) + w * canny(x), 0, 1) -> PreActResNet (preactresnet_EE.py:70-187) with CannyFilter; the _BPDA and _BPDA_3 classes
    below differ only in the edge filter (preactresnet_EE_BPDA.py: CannyFilter_BPDA, preactresnet_EE_BPDA_3.py: CannyFilter_step125_1)."""
    canny_cls = CannyFilter

    def __init__(self, block, num_blocks, num_classes=10, dataset="Tiny-ImageNet", cize=224, r=16, w=0.5, with_gf=False, low=60.0, high=120.0,
                 alpha=0.0, sigma=1):
        nn.Module.__init__(self)
        if dataset != "Tiny-ImageNet":
            raise NotImplementedError("dataset=%r: only the Tiny-ImageNet PreActResNets (7x7 / 2 stem, 200 classes) are built" % (dataset,))
        self.in_planes = 64
        self.dataset = dataset
        self._build_front(cize, 3, r, w, with_gf, low, high, alpha, sigma, self.canny_cls.__name__, False, 0.05, 1)
        self._build_cnn(block, num_blocks, dataset)

    def forward(self, x, draws=None):
        return self.body(self.front(x, draws))


class PreActResNet_EE_BPDA(PreActResNet_EE):
    canny_cls = CannyFilter_BPDA


class PreActResNet_EE_BPDA_3(PreActResNet_EE):
    canny_cls = CannyFilter_step125_1


_EE_CLASSES = {"EE": PreActResNet_EE, "EE_BPDA": PreActResNet_EE_BPDA, "EE_BPDA_3": PreActResNet_EE_BPDA_3}

_BLOCKS = {18: (PreActBlock, [2, 2, 2, 2]), 34: (PreActBlock, [3, 4, 6, 3]), 50: (PreActBottleneck, [3, 4, 6, 3]),
           101: (PreActBottleneck, [3, 4, 23, 3]), 152: (PreActBottleneck, [3, 8, 36, 3])}


def make_preact(depth, dataset="CIFAR10"):
    block, layers = _BLOCKS[depth]
    return PreActResNet(block, layers, dataset=dataset)


def make_preact_cifar(depth, dataset="CIFAR10"):
    """the CIFAR models have a door of their own: make_preact keeps refusing every dataset but Tiny-ImageNet"""
    block, layers = _BLOCKS[depth]
    return PreActResNetCifar(block, layers, dataset=dataset)


def make_preact_ee(depth, variant, dataset="CIFAR10", **kwargs):
    """variant: "EE", "EE_BPDA" or "EE_BPDA_3" (the reference's three preactresnet_EE*.py files)"""
    block, layers = _BLOCKS[depth]
    return _EE_CLASSES[variant](block, layers, dataset=dataset, **kwargs)
