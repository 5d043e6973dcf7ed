"""Layer blocks of the FarSeg and DeepLabv3+ paths (reference ever/module/ops.py:25-100,152-181), HIP-backed.
Child indices ('0' conv, '1' bn/identity, '2' relu/identity) match the reference so state-dict keys
such as `fpn.fpn_inner1.0.weight` are identical."""
import torch.nn as nn

from ..hip import functional as HF
from .layers import AdaptiveAvgPool2d, BatchNorm2d, Conv2d, HipSequential, ReLU, UpsamplingBilinear2d, run_sequence

__all__ = ['ConvBlock', 'Bf16compatible', 'ConvUpsampling', 'DepthwiseConv2d', 'SeparableConv2d', 'SeparableConvBlock',
           'PoolBlock']


class DepthwiseConv2d(Conv2d):
    """nn.Conv2d with groups = in_channels = out_channels (reference ops.py:25-31), on the depthwise kernels."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, bias=True,
                 padding_mode='zeros'):
        assert in_channels == out_channels
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, in_channels, bias, padding_mode)


class SeparableConv2d(HipSequential):
    """depthwise conv -> (activation) -> 1x1 conv (+bias); reference ops.py:34-42."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, bias=True,
                 padding_mode='zeros', activation=None):
        super().__init__(
            Conv2d(in_channels, in_channels, kernel_size, stride, padding, dilation, groups=in_channels, bias=False,
                   padding_mode=padding_mode),
            activation if activation else nn.Identity(),
            Conv2d(in_channels, out_channels, 1, bias=bias),
        )


class ConvBlock(HipSequential):
    """conv -> (BN) -> (ReLU); reference ops.py:45-64."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                 bias=False, bn=True, relu=True, init_fn=None):
        super().__init__(
            Conv2d(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias),
            BatchNorm2d(out_channels) if bn else nn.Identity(),
            ReLU(True) if relu else nn.Identity(),
        )
        if init_fn:
            self.apply(init_fn)

    @staticmethod
    def same_padding(kernel_size, dilation):
        return dilation * (kernel_size - 1) // 2


class SeparableConvBlock(HipSequential):
    """SeparableConv2d -> (BN) -> (ReLU); reference ops.py:67-86.  State-dict keys `0.0.weight` (depthwise), `0.2.weight`
    (pointwise), `1.*` (BatchNorm)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, bias=False, bn=True,
                 relu=True, init_fn=None):
        super().__init__(
            SeparableConv2d(in_channels, out_channels, kernel_size, stride, padding, dilation, bias),
            BatchNorm2d(out_channels) if bn else nn.Identity(),
            ReLU(True) if relu else nn.Identity(),
        )
        if init_fn:
            self.apply(init_fn)

    def forward(self, x):
        # one sequence, so that the pointwise convolution sees the BatchNorm after it (statistics from its epilogue)
        sep = self[0]
        mods = (list(sep) if type(sep) is SeparableConv2d else [sep]) + list(self)[1:]
        return run_sequence(mods, x)

    @staticmethod
    def same_padding(kernel_size, dilation):
        return dilation * (kernel_size - 1) // 2


class PoolBlock(HipSequential):
    """global average pool -> ConvBlock 1x1 -> resize back to the input's size; reference ops.py:89-100.  The resize of
    the 1x1 map (bilinear, align_corners=False) is an exact broadcast (HF.broadcast_hw).  Only output_size 1 (ASPP's
    image-level branch) is implemented."""

    def __init__(self, output_size, in_channels, out_channels):
        if output_size not in (1, (1, 1), [1, 1]):
            raise NotImplementedError('ever_amd PoolBlock: only output_size=1 is implemented (pyramid pooling is not)')
        super().__init__(
            AdaptiveAvgPool2d(output_size),
            ConvBlock(in_channels, out_channels, 1),
        )

    def forward(self, x):
        size = x.shape[-2:]
        y = run_sequence(list(self), x)
        return HF.broadcast_hw(y, size)


class Bf16compatible(nn.Module):
    """Reference ops.py:152-166 runs the wrapped (upsampling) module in fp32 under bf16 autocast.  The
    HIP path computes in fp32 throughout, so this only preserves the `_inner_module` key structure."""

    def __init__(self, module):
        super().__init__()
        self._inner_module = module

    def forward(self, x):
        return self._inner_module(x)


class ConvUpsampling(HipSequential):
    """conv (+bias) -> bilinear(align_corners=True) ; reference ops.py:169-181."""

    def __init__(self, in_channels, out_channels, scale_factor, kernel_size, stride=1, padding=0, dilation=1):
        super().__init__(
            Conv2d(in_channels, out_channels, kernel_size, stride, padding, dilation),
            Bf16compatible(UpsamplingBilinear2d(scale_factor=scale_factor)),
        )
