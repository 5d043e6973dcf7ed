"""DeepLabv3+ decoder and head (reference ever/module/deeplabv3p_head.py:8-86), HIP-backed.  Constructor signatures,
defaults, child indices and state-dict keys follow the reference; `Deeplabv3pHead` is registered in registry.MODEL."""
import torch.nn as nn

from ..core import registry
from ..interface import ERModule
from .aspp import AtrousSpatialPyramidPool, concat_list
from .layers import Conv2d, HipSequential, UpsamplingBilinear2d
from .ops import ConvBlock, SeparableConvBlock

__all__ = ['Deeplabv3pDecoder', 'Deeplabv3pHead']


class Deeplabv3pDecoder(nn.Module):
    """Chen et al., encoder-decoder with atrous separable convolution: the os16 feature through ASPP + 3x3, upsampled
    x4 (align_corners=True) and concatenated with the reduced os4 feature, then separable 3x3 blocks."""

    def __init__(self,
                 os4_feature_channels=256,
                 os16_feature_channels=2048,
                 aspp_channels=256,
                 aspp_atrous=(6, 12, 18),
                 reduction_dim=48,
                 out_channels=256,
                 num_3x3_convs=2,
                 scale_factor=4.0,
                 ):
        super().__init__()
        self.scale_factor = scale_factor
        self.os4_transform = ConvBlock(os4_feature_channels, reduction_dim, 3, 1, 1, bias=False)
        self.os16_transform = HipSequential(
            AtrousSpatialPyramidPool(os16_feature_channels, aspp_channels, aspp_atrous),
            ConvBlock(aspp_channels, aspp_channels, 3, 1, 1, bias=False)
        )
        layers = [SeparableConvBlock(aspp_channels + reduction_dim, out_channels, 3, 1, 1, bias=False)]
        for _ in range(num_3x3_convs - 1):
            layers.append(SeparableConvBlock(out_channels, out_channels, 3, 1, 1, bias=False))
        self.upsample = UpsamplingBilinear2d(scale_factor=scale_factor)
        self.stack_conv3x3 = HipSequential(*layers)

    def forward(self, feat_list):
        os4_feat, os16_feat = feat_list
        os4_feat = self.os4_transform(os4_feat)
        os16_feat = self.os16_transform(os16_feat)
        feat_upx = self.upsample(os16_feat)
        return self.stack_conv3x3(concat_list([os4_feat, feat_upx]))


@registry.MODEL.register(verbose=False)
class Deeplabv3pHead(ERModule):
    """decoder -> 1x1 classifier (+bias) -> bilinear (align_corners=True) upsampling; input [os4 feature, os16 feature]."""

    def __init__(self, config):
        super().__init__(config)
        self.head = HipSequential(
            Deeplabv3pDecoder(**self.config.deeplabv3p_decoder),
            Conv2d(self.config.deeplabv3p_decoder.out_channels, self.config.num_classes, 1),
            UpsamplingBilinear2d(scale_factor=self.config.upsample_scale)
        )

    def forward(self, x):
        return self.head(x)

    def set_default_config(self):
        self.config.update(dict(
            deeplabv3p_decoder=dict(
                os4_feature_channels=256,
                os16_feature_channels=2048,
                aspp_channels=256,
                aspp_atrous=(6, 12, 18),
                reduction_dim=48,
                out_channels=256,
                num_3x3_convs=2,
                scale_factor=4.0,
            ),
            num_classes=3,
            upsample_scale=4.0
        ))
