"""PreActResNet_EE_BPDA (reference: AWP/Tiny_imagenet/models_tiny_awp/preactresnet_EE_BPDA.py): the edge-enhancement front end with CannyFilter_BPDA, then the
pre-activation ResNet, on the HIP kernels (eeadv.preact).  Same factory names and keyword arguments (cize, r, w, with_gf, low, high,
alpha, sigma); dataset="Tiny-ImageNet" is the one that is built."""
from eeadv.preact import PreActBlock, PreActBottleneck, PreActResNet_EE_BPDA, make_preact_ee  # noqa: F401


def PreActResNet18_EE_BPDA(dataset="CIFAR10", **kwargs):
    return make_preact_ee(18, "EE_BPDA", dataset=dataset, **kwargs)


def PreActResNet34_EE_BPDA(dataset="CIFAR10", **kwargs):
    return make_preact_ee(34, "EE_BPDA", dataset=dataset, **kwargs)


def PreActResNet50_EE_BPDA(dataset="CIFAR10", **kwargs):
    return make_preact_ee(50, "EE_BPDA", dataset=dataset, **kwargs)


def PreActResNet101_EE_BPDA(dataset="CIFAR10", **kwargs):
    return make_preact_ee(101, "EE_BPDA", dataset=dataset, **kwargs)


def PreActResNet152_EE_BPDA(dataset="CIFAR10", **kwargs):
    return make_preact_ee(152, "EE_BPDA", dataset=dataset, **kwargs)
