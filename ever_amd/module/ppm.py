"""Pyramid pooling module and head (reference ever/module/ppm.py:8-62), HIP-backed.  Constructor signatures, defaults, asserts,
child order and state-dict keys follow the reference; `PPMHead` is registered in registry.MODEL.

The reference runs its PoolBlocks one after the other (K adaptive pools of the same map, K up-sampled maps, torch.cat).
Here the module runs their children itself: one pass pools the map for every bin (HF.pyramid_pool), the K ConvBlocks work
on the tiny pooled maps, and one pass writes the input and the K bilinear up-samplings into the concat map
(HF.pyramid_concat)."""
import torch.nn as nn

from ..core import registry
from ..hip import functional as HF
from ..interface import ERModule
from .layers import AdaptiveAvgPool2d, Conv2d, Dropout2d, HipSequential, UpsamplingBilinear2d, run_sequence
from .ops import ConvBlock, PoolBlock

__all__ = ['PyramidPoolModule', 'PPMHead']


class PyramidPoolBlock(PoolBlock):
    """The reference's PoolBlock (ops.py:89-100) for a square output size 1..8: adaptive average pool -> ConvBlock 1x1 ->
    bilinear (align_corners=False) resize back, same children and state-dict keys.  `ops.PoolBlock` itself stays what it
    was, the size-1 block of ASPP (it refuses other sizes); this subclass adds the one-bin calls of the pyramid kernels.
    PyramidPoolModule runs its blocks' children itself, all bins in one pool and one expand pass."""

    def __init__(self, output_size, in_channels, out_channels):
        size = HF.check_bins([output_size], 'PyramidPoolBlock')[0]      # NotImplementedError outside the kernels' bins
        HipSequential.__init__(self, AdaptiveAvgPool2d(output_size), ConvBlock(in_channels, out_channels, 1))
        self._bin = size

    def forward(self, x):
        if self._bin == 1:
            return PoolBlock.forward(self, x)
        return HF.pyramid_expand(run_sequence(list(self), x), x.shape[-2:])


class PyramidPoolModule(nn.Module):
    def __init__(self,
                 in_channels,
                 pool_channels,
                 out_channels,
                 bins,
                 bottleneck_conv='3x3',
                 dropout=0):
        assert out_channels % len(bins) == 0
        super().__init__()
        self.bins = HF.check_bins(bins, 'PyramidPoolModule')       # NotImplementedError outside the kernels' scope
        self.pools = nn.ModuleList([
            PyramidPoolBlock(size, in_channels, pool_channels) for size in bins
        ])
        if bottleneck_conv == '3x3':
            self.conv = ConvBlock(pool_channels * len(bins) + in_channels, out_channels, 3, 1, 1, bias=False)
        elif bottleneck_conv == '1x1':
            self.conv = ConvBlock(pool_channels * len(bins) + in_channels, out_channels, 1, bias=False)
        else:
            self.conv = nn.Identity()

        self.dropout = Dropout2d(p=dropout) if dropout > 0 else nn.Identity()

    def _fusable(self):
        """every block is the stock pair (pool, ConvBlock) without hooks that expect to see a block's own output"""
        return all(type(p) is PyramidPoolBlock and len(p) == 2 and not (p._forward_hooks or p._forward_pre_hooks or p[0]._forward_hooks
                                                                 or p[0]._forward_pre_hooks) for p in self.pools)

    def forward(self, x):
        if self._fusable():
            x_pass, *pooled = HF.pyramid_pool(x, self.bins)
            zs = [p[1](t) for p, t in zip(self.pools, pooled)]
            out = HF.pyramid_concat(x_pass, zs, self.bins)
        else:       # layer by layer: every block's own forward (and hooks)
            from .aspp import concat_list
            out = concat_list([x] + [p(x) for p in self.pools])
        out = self.conv(out)
        return self.dropout(out)


@registry.MODEL.register(verbose=False)
class PPMHead(ERModule):
    """PyramidPoolModule -> 1x1 classifier (+bias) -> bilinear (align_corners=True) upsampling."""

    def __init__(self, config):
        super().__init__(config)
        self.head = HipSequential(
            PyramidPoolModule(**self.config.ppm),
            Conv2d(self.config.ppm.out_channels, self.config.num_classes, 1),
            UpsamplingBilinear2d(scale_factor=self.config.upsample_scale)
        )

    def forward(self, x):
        x = self.head(x)
        return x

    def set_default_config(self):
        self.config.update(dict(
            ppm=dict(
                in_channels=2048,
                pool_channels=512,
                out_channels=512,
                bins=(1, 2, 3, 6)
            ),
            num_classes=3,
            upsample_scale=8.0
        ))
