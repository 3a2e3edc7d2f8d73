from .preactresnet import PreActResNet18, PreActResNet34, PreActResNet50, PreActResNet101, PreActResNet152  # noqa: F401
from .preactresnet_EE import PreActResNet18_EE, PreActResNet34_EE, PreActResNet50_EE, PreActResNet101_EE, PreActResNet152_EE  # noqa: F401
from .preactresnet_EE_BPDA import (PreActResNet18_EE_BPDA, PreActResNet34_EE_BPDA, PreActResNet50_EE_BPDA, PreActResNet101_EE_BPDA,  # noqa: F401
                                   PreActResNet152_EE_BPDA)
from .preactresnet_EE_BPDA_3 import (PreActResNet18_EE_BPDA_3, PreActResNet34_EE_BPDA_3, PreActResNet50_EE_BPDA_3,  # noqa: F401
                                     PreActResNet101_EE_BPDA_3, PreActResNet152_EE_BPDA_3)
from .utils_awp import AdvWeightPerturb, add_into_weights, diff_in_weights  # noqa: F401
