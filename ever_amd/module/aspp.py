"""Atrous spatial pyramid pooling and the ASPP head (reference ever/module/aspp.py:8-55), HIP-backed.  Constructor
signatures, defaults, child indices and state-dict keys follow the reference; `ASPPHead` stays unregistered, as there."""
import torch.nn as nn

from ..hip import functional_next as HN
from ..interface import ERModule
from .layers import Conv2d, Dropout, HipSequential, UpsamplingBilinear2d
from .ops import ConvBlock, PoolBlock

__all__ = ['AtrousSpatialPyramidPool', 'ASPPHead', 'concat_list']


def concat_list(feats):
    """torch.cat(feats, dim=1) as a chain of two-way channel concatenations (evk_concat_channels)."""
    out = feats[0]
    for f in feats[1:]:
        out = HN.concat_channels(out, f)
    return out


class AtrousSpatialPyramidPool(nn.Module):
    """1x1 branch, one dilated 3x3 branch per rate, the image-level pool branch; concatenated and projected
    (ConvBlock 1x1 + Dropout(0.5)).  Reference aspp.py:8-30."""

    def __init__(self, in_channels, out_channels, atrous_rates, conv_block=ConvBlock):
        super().__init__()
        modules = [conv_block(in_channels, out_channels, 1, bias=False)]
        for rate in atrous_rates:
            modules.append(conv_block(in_channels, out_channels, 3, 1, rate, rate, bias=False))
        modules.append(PoolBlock(1, in_channels, out_channels))
        self.convs = nn.ModuleList(modules)
        self.project = HipSequential(
            conv_block(len(self.convs) * out_channels, out_channels, 1, bias=False),
            Dropout(0.5))

    def forward(self, x):
        return self.project(concat_list([conv(x) for conv in self.convs]))


class ASPPHead(ERModule):
    """ASPP -> 1x1 classifier (+bias) -> bilinear (align_corners=True) upsampling; reference aspp.py:33-55."""

    def __init__(self, config):
        super().__init__(config)
        self.head = HipSequential(
            AtrousSpatialPyramidPool(**self.config.aspp),
            Conv2d(self.config.aspp.out_channels, self.config.num_classes, 1),
            UpsamplingBilinear2d(scale_factor=self.config.upsample_scale),
        )

    def forward(self, x):
        return self.head(x)

    def set_default_config(self):
        self.config.update(dict(
            aspp=dict(
                in_channels=2048,
                out_channels=256,
                atrous_rates=[6, 12, 18]
            ),
            num_classes=3,
            upsample_scale=8.0
        ))
