"""HRNetV2 segmentation head (reference ever/module/hrnet_head.py:8-49), HIP-backed: the four branch maps up-sampled
(bilinear, align_corners=True) to the first one's size and concatenated, 1x1 convolution (+bias) -> BatchNorm -> ReLU, 1x1
classifier (+bias), bilinear up-sampling.  Constructor signatures, defaults, child indices and state-dict keys follow the
reference; `HRNetHead` is registered in registry.MODEL."""
import os

import torch
import torch.nn as nn

from ..core import registry
from ..hip import functional as HF
from ..interface import ERModule
from .fold import _takes_epilogue_stats
from .layers import BatchNorm2d, Conv2d, HipSequential, ReLU, UpsamplingBilinear2d, run_sequence

__all__ = ['SimpleFusion', 'HRNetHead']


class SimpleFusion(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.fuse_conv = HipSequential(
            Conv2d(in_channels, in_channels, 1),
            BatchNorm2d(in_channels),
            ReLU(True),
        )

    def concat(self, feat_list):
        """every source written straight into its channel slice of the concat buffer (HF.bilinear_concat): no up-sampled
        intermediate tensor exists, in either direction"""
        return HF.bilinear_concat(list(feat_list), size=feat_list[0].shape[2:])

    def forward(self, feat_list):
        return self.fuse_conv(self.concat(feat_list))


@registry.MODEL.register(verbose=False)
class HRNetHead(ERModule):
    def __init__(self, config):
        super().__init__(config)
        self.head = HipSequential(
            SimpleFusion(**self.config.hrnet_decoder),
            Conv2d(self.config.hrnet_decoder.in_channels, self.config.num_classes, 1),
            UpsamplingBilinear2d(scale_factor=self.config.upsample_scale),
        )

    def _bn_relu_classifier(self, fusion, x, classifier):
        """`classifier(relu(bn(conv1x1(x))))` with BatchNorm + ReLU + classifier as ONE consumer of the fuse convolution's
        output (HF.bn_relu_dot, as the FPN decoder's branches: module/fpn.py); None = run the layers one by one (eval or
        folded BatchNorm, another norm, hooks, EVK_BN_DOT=0)."""
        if os.environ.get('EVK_BN_DOT', '1') == '0' or not torch.is_grad_enabled() or type(fusion) is not SimpleFusion:
            return None
        seq = fusion.fuse_conv
        if len(seq) != 3 or type(seq[0]) is not Conv2d or not isinstance(seq[2], nn.ReLU) or type(classifier) is not Conv2d:
            return None
        conv, bn = seq[0], seq[1]
        if not (_takes_epilogue_stats(bn) and bn.training and bn.momentum is not None):
            return None
        if any(m._forward_hooks or m._forward_pre_hooks for m in (self.head, fusion, seq, conv, bn, seq[2], classifier)):
            return None
        z = conv(x, bn_stats=True)
        out = HF.bn_relu_dot(z, bn, classifier)
        if out is None:      # wider than the fused form takes (hrnetv2_w48: 720 channels), or no statistics records on z
            return classifier(run_sequence(list(seq)[1:], z))
        if bn.track_running_stats and bn.num_batches_tracked is not None:
            bn._nbt_pending = getattr(bn, '_nbt_pending', 0) + 1
        return out

    def forward(self, x):
        fusion, classifier, upsample = self.head[0], self.head[1], self.head[2]
        if type(fusion) is not SimpleFusion:
            return self.head(x)
        cat = fusion.concat(x)
        logits = self._bn_relu_classifier(fusion, cat, classifier)
        if logits is None:
            logits = classifier(fusion.fuse_conv(cat))
        return upsample(logits)

    def set_default_config(self):
        self.config.update(dict(
            hrnet_decoder=dict(
                in_channels=480,
            ),
            num_classes=3,
            upsample_scale=4.0
        ))
