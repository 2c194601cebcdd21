"""Convolution + batch norm fused for QAT: the weight is scaled by the BN's running statistics, fake-quantized, and the
convolution's result is un-scaled again in front of the BN (upstream src/quantized_training/modules/qat/conv_fused.py:25-362,
496-538, 628-694, 819-825).  The ReLU variants are not exported upstream either."""
import math

import torch
import torch.ao.nn.intrinsic as nni
import torch.nn as nn
from torch.nn import init
from torch.nn.modules.utils import _pair, _single, _triple
from torch.nn.utils import fuse_conv_bn_weights

from .conv import _RoutedConv2d

__all__ = ["ConvBn1d", "ConvBn2d", "ConvBn3d", "update_bn_stats", "freeze_bn_stats"]

# state-dict names of serialization version 1 (BN tensors on the module itself) -> version 2 (inside the `bn` child)
_V1_NAMES = {
    "bn.weight": "gamma",
    "bn.bias": "beta",
    "bn.running_mean": "running_mean",
    "bn.running_var": "running_var",
    "bn.num_batches_tracked": "num_batches_tracked",
}


class _ConvBnNd(nn.modules.conv._ConvNd, nni._FusedModule):
    _version = 2
    _FLOAT_MODULE = nn.modules.conv._ConvNd
    _FLOAT_RELU_MODULE = None
    _TUPLE = staticmethod(_pair)
    _BN = nn.BatchNorm2d

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=None,
                 padding_mode="zeros", eps=1e-05, momentum=0.1, freeze_bn=False, qconfig=None) -> None:
        nd = type(self)._TUPLE
        nn.modules.conv._ConvNd.__init__(self, in_channels, out_channels, nd(kernel_size), nd(stride), nd(padding), nd(dilation), False,
                                         nd(0), groups, False, padding_mode)
        assert qconfig, "qconfig must be provided for QAT module"
        self.qconfig = qconfig
        self.freeze_bn = freeze_bn if self.training else True
        self.bn = type(self)._BN(out_channels, eps, momentum, True, True)
        self.weight_fake_quant = self.qconfig.weight()
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_bn_parameters()
        # after reset_bn_parameters: both touch the BN's state
        if self.training and not freeze_bn:
            self.update_bn_stats()
        else:
            self.freeze_bn_stats()
        self._enable_slow_path_for_better_numerical_stability = False

    def reset_running_stats(self):
        self.bn.reset_running_stats()

    def reset_bn_parameters(self):
        self.bn.reset_running_stats()
        init.uniform_(self.bn.weight)
        init.zeros_(self.bn.bias)
        if self.bias is not None:                         # (the convolution's bias)
            fan_in, _ = init._calculate_fan_in_and_fan_out(self.weight)
            bound = 1 / math.sqrt(fan_in)
            init.uniform_(self.bias, -bound, bound)

    def update_bn_stats(self):
        self.freeze_bn = False
        self.bn.training = True
        return self

    def freeze_bn_stats(self):
        self.freeze_bn = True
        self.bn.training = False
        return self

    def _shapes(self):
        per_out = [1] * self.weight.dim()
        per_out[0] = -1                                   # broadcast over a weight's output channels
        per_ch = [1] * self.weight.dim()
        per_ch[1] = -1                                    # broadcast over an activation's channels
        return per_out, per_ch

    def _forward(self, input):
        if self._enable_slow_path_for_better_numerical_stability:
            return self._forward_slow(input)
        return self._forward_approximate(input)

    def _forward_approximate(self, input):
        """One pass: convolve with fq(W * scale_factor), scale_factor = bn.weight / running_std, divide the result by scale_factor again
        and hand it (+ the convolution's bias) to the BN."""
        assert self.bn.running_var is not None
        per_out, per_ch = self._shapes()
        running_std = torch.sqrt(self.bn.running_var + self.bn.eps)
        scale_factor = self.bn.weight / running_std
        scaled_weight = self.weight_fake_quant(self.weight * scale_factor.reshape(per_out))
        # a zero bias: the convolution's own bias is added behind the un-scaling
        if self.bias is not None:
            zero_bias = torch.zeros_like(self.bias, dtype=input.dtype)
        else:
            zero_bias = torch.zeros(self.out_channels, device=scaled_weight.device, dtype=input.dtype)
        conv = self._conv_forward(input, scaled_weight, zero_bias)
        conv_orig = conv / scale_factor.reshape(per_ch)
        if self.bias is not None:
            conv_orig = conv_orig + self.bias.reshape(per_ch)
        return self.bn(conv_orig)

    def _forward_slow(self, input):
        """Two passes (arXiv:1806.08342), exact also where bn.weight == 0.  With Y0 = conv(X, W) and the batch statistics of Y0:
            training:   conv(X, fq(r W / running_std)) * (running_std / batch_std) + beta - r * batch_mean / batch_std
            inference:  conv(X, fq(r W / running_std))                             + beta - r * (running_mean - B_c) / running_std"""
        assert self.bn.running_var is not None and self.bn.running_mean is not None
        per_out, per_ch = self._shapes()
        zero_bias = torch.zeros(self.out_channels, device=self.weight.device, dtype=input.dtype)

        if self.bn.training:
            conv_out = self._conv_forward(input, self.weight, zero_bias)          # for the batch mean / std
            with torch.no_grad():                                                 # updates the BN's running statistics
                self.bn(conv_out if self.bias is None else conv_out + self.bias.reshape(per_ch))

        running_std = torch.sqrt(self.bn.running_var + self.bn.eps)
        scale_factor = self.bn.weight / running_std
        scaled_weight = self.weight_fake_quant(self.weight * scale_factor.reshape(per_out))
        conv_bn = self._conv_forward(input, scaled_weight, zero_bias)

        if self.bn.training:
            avg_dims = [0] + list(range(2, self.weight.dim()))
            batch_mean = conv_out.mean(avg_dims)
            batch_var = torch.square(conv_out - batch_mean.reshape(per_ch)).mean(avg_dims)
            batch_std = torch.sqrt(batch_var + self.bn.eps)
            conv_bn *= (running_std / batch_std).reshape(per_ch)
            fused_mean, fused_std = batch_mean, batch_std
        else:
            fused_mean = self.bn.running_mean - (self.bias if self.bias is not None else 0)
            fused_std = running_std

        fused_bias = self.bn.bias - self.bn.weight * fused_mean / fused_std
        conv_bn += fused_bias.reshape(per_ch)
        if self.bias is not None:
            # keeps the convolution's bias in the autograd graph (DDP rejects parameters that take no part in the loss)
            conv_bn += (self.bias - self.bias).reshape(per_ch)
        return conv_bn

    def forward(self, input):
        return self._forward(input)

    def train(self, mode=True):
        """A frozen BN keeps its mode: ``model.train()`` must not switch its statistics back on."""
        self.training = mode
        if not self.freeze_bn:
            for module in self.children():
                module.train(mode)
        return self

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        version = local_metadata.get("version", None)
        if version is None or version == 1:
            # version 1 kept gamma / beta / running_* on the module itself; version 2 holds them in `bn`
            for v2, v1 in _V1_NAMES.items():
                if prefix + v1 in state_dict:
                    state_dict[prefix + v2] = state_dict.pop(prefix + v1)
                elif prefix + v2 in state_dict:
                    pass                                  # (files that carry version 1 but already use the new names)
                elif strict:
                    missing_keys.append(prefix + v2)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    @classmethod
    def from_float(cls, mod):
        """The QAT twin of a fused float ``ConvBnNd`` that carries a ``qconfig``: the convolution's Parameters and the BN's parameters and
        buffers stay the SAME objects."""
        assert type(mod) == cls._FLOAT_MODULE, f"qat.{cls.__name__}.from_float only works for {cls._FLOAT_MODULE.__name__}"
        assert getattr(mod, "qconfig", None), "Input float module must have a valid qconfig"
        conv, bn = mod[0], mod[1]
        twin = cls(conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding, conv.dilation, conv.groups,
                   conv.bias is not None, conv.padding_mode, bn.eps, bn.momentum, False, mod.qconfig)
        twin.weight = conv.weight
        twin.bias = conv.bias
        twin.bn.weight = bn.weight
        twin.bn.bias = bn.bias
        twin.bn.running_mean = bn.running_mean
        twin.bn.running_var = bn.running_var
        twin.bn.num_batches_tracked = bn.num_batches_tracked
        return twin

    def to_float(self):
        """A float convolution with the BN folded into its weight and bias (``fuse_conv_bn_weights``)."""
        cls = type(self)
        conv = cls._FLOAT_CONV_MODULE(self.in_channels, self.out_channels, self.kernel_size, self.stride, self.padding, self.dilation,
                                      self.groups, self.bias is not None, self.padding_mode)
        conv.weight = torch.nn.Parameter(self.weight.detach())
        if self.bias is not None:
            conv.bias = torch.nn.Parameter(self.bias.detach())
        if cls._FLOAT_BN_MODULE:
            assert self.bn.running_var is not None and self.bn.running_mean is not None
            conv.weight, conv.bias = fuse_conv_bn_weights(conv.weight, conv.bias, self.bn.running_mean, self.bn.running_var, self.bn.eps,
                                                          self.bn.weight, self.bn.bias)
        conv.train(self.training)
        return conv


class ConvBn1d(_ConvBnNd, nn.Conv1d):
    _FLOAT_MODULE = nni.ConvBn1d
    _FLOAT_CONV_MODULE = nn.Conv1d
    _FLOAT_BN_MODULE = nn.BatchNorm1d
    _TUPLE = staticmethod(_single)
    _BN = nn.BatchNorm1d


class ConvBn2d(_RoutedConv2d, _ConvBnNd, nn.Conv2d):
    _FLOAT_MODULE = nni.ConvBn2d
    _FLOAT_CONV_MODULE = nn.Conv2d
    _FLOAT_BN_MODULE = nn.BatchNorm2d
    _TUPLE = staticmethod(_pair)
    _BN = nn.BatchNorm2d


class ConvBn3d(_ConvBnNd, nn.Conv3d):
    _FLOAT_MODULE = nni.ConvBn3d
    _FLOAT_CONV_MODULE = nn.Conv3d
    _FLOAT_BN_MODULE = nn.BatchNorm3d
    _TUPLE = staticmethod(_triple)
    _BN = nn.BatchNorm3d


_TWINS = (ConvBn1d, ConvBn2d, ConvBn3d)


def update_bn_stats(mod):
    """For ``model.apply``: let the BN of a fused conv twin update its running statistics again."""
    if type(mod) in _TWINS:
        mod.update_bn_stats()


def freeze_bn_stats(mod):
    """For ``model.apply``: freeze the BN statistics of a fused conv twin."""
    if type(mod) in _TWINS:
        mod.freeze_bn_stats()
