from .preactresnet import PreActResNet18, PreActResNet34, PreActResNet50, PreActResNet101, PreActResNet152  # noqa: F401
from .utils_awp import AdvWeightPerturb, add_into_weights, diff_in_weights  # noqa: F401
