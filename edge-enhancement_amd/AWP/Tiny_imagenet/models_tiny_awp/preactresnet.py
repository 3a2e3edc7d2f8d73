"""Pre-activation ResNets (reference: AWP/Tiny_imagenet/models_tiny_awp/preactresnet.py) on the HIP kernels: eeadv.preact.
Same factory names and signatures; dataset="Tiny-ImageNet" is the one that is built (the CIFAR / ImageNet branches raise
NotImplementedError)."""
from eeadv.preact import PreActBlock, PreActBottleneck, PreActResNet, make_preact  # noqa: F401


def PreActResNet18(dataset="CIFAR10"):
    return make_preact(18, dataset)


def PreActResNet34(dataset="CIFAR10"):
    return make_preact(34, dataset)


def PreActResNet50(dataset="CIFAR10"):
    return make_preact(50, dataset)


def PreActResNet101(dataset="CIFAR10"):
    return make_preact(101, dataset)


def PreActResNet152(dataset="CIFAR10"):
    return make_preact(152, dataset)
