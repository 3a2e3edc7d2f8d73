"""Pre-activation ResNets for CIFAR (reference: AWP/Cifar100/models_cifar100_awp/preactresnet.py) on the HIP path: eeadv.preact.
Same factory names and signatures; dataset="CIFAR10" (the default) and "CIFAR100" are built - 3x3 / 1 stem, AvgPool2d(4), `linear` -
and the ImageNet / Tiny-ImageNet branches raise NotImplementedError (Tiny-ImageNet: AWP/Tiny_imagenet/models_tiny_awp)."""
from eeadv.preact import PreActBlock, PreActBottleneck, PreActResNetCifar as PreActResNet, make_preact_cifar  # noqa: F401


def PreActResNet18(dataset="CIFAR10"):
    return make_preact_cifar(18, dataset)


def PreActResNet34(dataset="CIFAR10"):
    return make_preact_cifar(34, dataset)


def PreActResNet50(dataset="CIFAR10"):
    return make_preact_cifar(50, dataset)


def PreActResNet101(dataset="CIFAR10"):
    return make_preact_cifar(101, dataset)


def PreActResNet152(dataset="CIFAR10"):
    return make_preact_cifar(152, dataset)
