"""Convolutions whose weight is fake-quantized on every forward
(upstream src/quantized_training/modules/qat/conv.py:16-270)."""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.ao.nn.intrinsic import _FusedModule
from torch.nn.modules.utils import _pair, _single, _triple

__all__ = ["Conv1d", "Conv2d", "Conv3d"]


class _RoutedConv2d:
    """``_conv_forward`` of the 2-d twins: on the device the in-tree implicit-GEMM kernel (csrc/qt_conv.hip through conv_route) where it
    takes the problem, torch's convolution otherwise.  CPU tensors go straight to torch."""

    def _conv_forward(self, input, weight, bias):
        if input.is_cuda:
            from ...conv_route import conv2d_or_none
            if self.padding_mode != "zeros":
                # what nn.Conv2d._conv_forward does: pad explicitly, then convolve without padding
                padded = F.pad(input, self._reversed_padding_repeated_twice, mode=self.padding_mode)
                out = conv2d_or_none(padded, weight, bias, self.stride, _pair(0), self.dilation, self.groups)
            else:
                out = conv2d_or_none(input, weight, bias, self.stride, self.padding, self.dilation, self.groups)
            if out is not None:
                return out
        return super()._conv_forward(input, weight, bias)


class _ConvNd(nn.modules.conv._ConvNd):
    """``_conv_forward(x, weight_fake_quant(W), b)``; shares ``weight`` / ``bias`` Parameters with the float module it was made from."""

    _FLOAT_MODULE = nn.modules.conv._ConvNd
    _TUPLE = staticmethod(_pair)

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 padding_mode="zeros", qconfig=None, device=None, dtype=None) -> None:
        nd = type(self)._TUPLE
        factory_kwargs = {"device": device, "dtype": dtype}
        nn.modules.conv._ConvNd.__init__(self, in_channels, out_channels, nd(kernel_size), nd(stride),
                                         padding if isinstance(padding, str) else nd(padding), nd(dilation), False, nd(0), groups, bias,
                                         padding_mode, **factory_kwargs)
        assert qconfig, "qconfig must be provided for QAT module"
        self.qconfig = qconfig
        # the fake-quantizer's buffers are real even when the layer itself is built on `meta`
        fq_device = None if device is not None and str(device) == "meta" else device
        self.weight_fake_quant = qconfig.weight(factory_kwargs={"device": fq_device, "dtype": dtype})

    def forward(self, input):
        return self._conv_forward(input, self.weight_fake_quant(self.weight), self.bias)

    @classmethod
    def from_float(cls, mod):
        """The QAT twin of a float convolution that carries a ``qconfig`` (a fused module stands for its first member); weight and bias
        stay the SAME Parameter objects as the float module's."""
        assert type(mod) == cls._FLOAT_MODULE, f"qat.{cls.__name__}.from_float only works for {cls._FLOAT_MODULE.__name__}"
        assert getattr(mod, "qconfig", None), "Input float module must have a valid qconfig"
        qconfig = mod.qconfig
        if isinstance(mod, _FusedModule):
            mod = mod[0]
        twin = cls(mod.in_channels, mod.out_channels, mod.kernel_size, stride=mod.stride, padding=mod.padding, dilation=mod.dilation,
                   groups=mod.groups, bias=mod.bias is not None, padding_mode=mod.padding_mode, qconfig=qconfig,
                   device="meta")                      # parameters are adopted from `mod` right below
        twin.weight = mod.weight
        twin.bias = mod.bias
        return twin

    def to_float(self):
        """A plain float convolution holding detached views of the current parameters."""
        cls = type(self)
        conv = cls._FLOAT_CONV_MODULE(self.in_channels, self.out_channels, self.kernel_size, self.stride, self.padding, self.dilation,
                                      self.groups, self.bias is not None, self.padding_mode, device="meta")
        conv.weight = torch.nn.Parameter(self.weight.detach())
        conv.bias = None if self.bias is None else torch.nn.Parameter(self.bias.detach())
        return conv


class Conv1d(_ConvNd, nn.Conv1d):
    _FLOAT_MODULE = nn.Conv1d
    _FLOAT_CONV_MODULE = nn.Conv1d
    _TUPLE = staticmethod(_single)


class Conv2d(_RoutedConv2d, _ConvNd, nn.Conv2d):
    _FLOAT_MODULE = nn.Conv2d
    _FLOAT_CONV_MODULE = nn.Conv2d
    _TUPLE = staticmethod(_pair)


class Conv3d(_ConvNd, nn.Conv3d):
    _FLOAT_MODULE = nn.Conv3d
    _FLOAT_CONV_MODULE = nn.Conv3d
    _TUPLE = staticmethod(_triple)
