"""PreActResNet_EE (reference: AWP/Tiny_imagenet/models_tiny_awp/preactresnet_EE.py): the edge-enhancement front end with CannyFilter, then the
pre-activation ResNet, on the HIP kernels (eeadv.preact).  Same factory names and keyword arguments (cize, r, w, with_gf, low, high,
alpha, sigma); dataset="Tiny-ImageNet" is the one that is built."""
from eeadv.preact import PreActBlock, PreActBottleneck, PreActResNet_EE, make_preact_ee  # noqa: F401


def PreActResNet18_EE(dataset="CIFAR10", **kwargs):
    return make_preact_ee(18, "EE", dataset=dataset, **kwargs)


def PreActResNet34_EE(dataset="CIFAR10", **kwargs):
    return make_preact_ee(34, "EE", dataset=dataset, **kwargs)


def PreActResNet50_EE(dataset="CIFAR10", **kwargs):
    return make_preact_ee(50, "EE", dataset=dataset, **kwargs)


def PreActResNet101_EE(dataset="CIFAR10", **kwargs):
    return make_preact_ee(101, "EE", dataset=dataset, **kwargs)


def PreActResNet152_EE(dataset="CIFAR10", **kwargs):
    return make_preact_ee(152, "EE", dataset=dataset, **kwargs)
