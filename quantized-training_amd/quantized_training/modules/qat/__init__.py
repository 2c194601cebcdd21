from .conv import Conv1d, Conv2d, Conv3d  # noqa: F401
from .conv_fused import ConvBn1d, ConvBn2d, ConvBn3d, freeze_bn_stats, update_bn_stats  # noqa: F401
from .linear import Linear  # noqa: F401
from .lora import LoraLinear, is_lora_linear  # noqa: F401
