"""ConvNeXt on the HIP path (API, child order and state-dict keys of reference ever/module/dinov3/models/convnext.py; the
architecture is "A ConvNet for the 2020s", arXiv:2201.03545, with the DINOv3 token outputs).

A block is depthwise 7x7 -> LayerNorm over channels -> 1x1 (C -> 4C) -> GELU -> 1x1 (4C -> C) -> input + drop_path(gamma *
x).  Maps are logical NCHW over NHWC memory, so the channels of a pixel are one contiguous row: the LayerNorm of either
data format is HF.layer_norm on the map, a Linear on the channels is a 1x1 convolution with the [out, in] matrix viewed as
[out, in, 1, 1] (already OHWI memory; the parameter stays 2-D, reference checkpoints load strictly), the block tail is
HF.scale_residual, and none of the reference's permutes is ever materialised."""
import logging
from functools import partial

import numpy as np
import torch
import torch.nn as nn

from ...hip import functional as HF
from ...hip import functional_next as HN
from ..layers import Conv2d, HipSequential
from ..layers import LayerNorm as _TokenLayerNorm

__all__ = ['DropPath', 'Block', 'LayerNorm', 'ConvNeXt', 'convnext_sizes', 'get_convnext_arch']

logger = logging.getLogger('dinov3')


class DropPath(nn.Module):
    """Stochastic depth per sample: x * floor(keep + u) / keep with one uniform draw per sample, identity in eval mode and
    at rate 0.  Inside a Block the factors go into the fused tail instead (Block.forward); called on its own it scales a
    map with the channel-scale kernel."""

    def __init__(self, drop_prob=None):
        super().__init__()
        self.drop_prob = drop_prob

    def forward(self, x):
        if not self.drop_prob or not self.training:
            return x
        scale = HF.drop_path_scale(x, self.drop_prob)
        if x.dim() != 4:
            raise NotImplementedError('ever_amd DropPath: only maps have a kernel outside a Block')
        return HN._ChannelScaleFn.apply(HF.as_nhwc(x, 'drop_path'), scale.view(-1, 1).expand(-1, x.shape[1]).contiguous())


class LayerNorm(nn.Module):
    """LayerNorm over the channels in either data format: "channels_last" takes [..., C] and normalises the last axis,
    "channels_first" takes a logical [N, C, H, W] map.  Both are the same rows of C floats to HF.layer_norm."""

    def __init__(self, normalized_shape, eps=1e-6, data_format='channels_last'):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(normalized_shape))
        self.bias = nn.Parameter(torch.zeros(normalized_shape))
        self.eps = eps
        self.data_format = data_format
        if self.data_format not in ('channels_last', 'channels_first'):
            raise NotImplementedError
        self.normalized_shape = (normalized_shape,)

    def forward(self, x):
        if self.data_format == 'channels_first':
            if x.dim() != 4:
                raise ValueError(f'LayerNorm(channels_first): a [N, C, H, W] map is required, got {tuple(x.shape)}')
            return HF.layer_norm(x, self.weight, self.bias, self.eps, channel_dim=1)
        return HF.layer_norm(x, self.weight, self.bias, self.eps, channel_dim=-1)

    def forward_map(self, x):
        """the normalisation over the channels of a logical-NCHW map, whatever the data format says about tensors"""
        return HF.layer_norm(x, self.weight, self.bias, self.eps, channel_dim=1)


class _MapLinear(nn.Linear):
    """nn.Linear (2-D weight, same keys) that also takes a logical-NCHW map and acts on its channels: a 1x1 convolution."""

    def forward(self, x):
        if x.dim() == 4:
            return HF.conv2d(x, self.weight.view(self.out_features, self.in_features, 1, 1), self.bias)
        raise NotImplementedError('ever_amd ConvNeXt Linear: only maps ([N, C, H, W]) have a kernel')


class Block(nn.Module):
    def __init__(self, dim, drop_path=0.0, layer_scale_init_value=1e-6):
        super().__init__()
        self.dwconv = Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim)
        self.norm = LayerNorm(dim, eps=1e-6)
        self.pwconv1 = _MapLinear(dim, 4 * dim)
        self.act = nn.GELU()
        self.pwconv2 = _MapLinear(4 * dim, dim)
        self.gamma = (nn.Parameter(layer_scale_init_value * torch.ones((dim)), requires_grad=True)
                      if layer_scale_init_value > 0 else None)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()

    def forward(self, x):
        y = self.dwconv(x)
        y = self.norm.forward_map(y)
        y = self.pwconv1(y)
        y = HN.gelu(y)
        y = self.pwconv2(y)
        rate = getattr(self.drop_path, 'drop_prob', None)
        scale = HF.drop_path_scale(y, rate) if (rate and self.training) else None
        return HF.scale_residual(x, y, self.gamma, scale)


def _tokens(x):
    """[N, C, H, W] map -> [N, HW, C] tokens: a view of NHWC memory"""
    return HF.as_nhwc(x, 'convnext').flatten(2).transpose(1, 2)


class ConvNeXt(nn.Module):
    def __init__(self, in_chans=3, depths=[3, 3, 9, 3], dims=[96, 192, 384, 768], drop_path_rate=0.0,
                 layer_scale_init_value=1e-6, patch_size=None, **ignored_kwargs):
        super().__init__()
        if ignored_kwargs:
            logger.warning('ConvNeXt: arguments without a meaning here were dropped: %s', sorted(ignored_kwargs))
        self.downsample_layers = nn.ModuleList()
        self.downsample_layers.append(HipSequential(
            Conv2d(in_chans, dims[0], kernel_size=4, stride=4),
            LayerNorm(dims[0], eps=1e-6, data_format='channels_first')))
        for i in range(3):
            self.downsample_layers.append(HipSequential(
                LayerNorm(dims[i], eps=1e-6, data_format='channels_first'),
                Conv2d(dims[i], dims[i + 1], kernel_size=2, stride=2)))
        self.stages = nn.ModuleList()
        rates = [float(r) for r in np.linspace(0, drop_path_rate, sum(depths))]
        cur = 0
        for i in range(4):
            self.stages.append(nn.Sequential(*[
                Block(dim=dims[i], drop_path=rates[cur + j], layer_scale_init_value=layer_scale_init_value)
                for j in range(depths[i])]))
            cur += depths[i]
        self.norm = _TokenLayerNorm(dims[-1], eps=1e-6)
        self.head = nn.Identity()
        self.embed_dim = dims[-1]
        self.embed_dims = dims
        self.n_blocks = len(self.downsample_layers)
        self.chunked_blocks = False
        self.n_storage_tokens = 0
        self.norms = nn.ModuleList([nn.Identity() for _ in range(3)])
        self.norms.append(self.norm)
        self.patch_size = patch_size
        self.input_pad_size = 4

    def init_weights(self):
        self.apply(self._init_weights)

    def _init_weights(self, module):
        if isinstance(module, nn.LayerNorm):
            module.reset_parameters()
        if isinstance(module, LayerNorm):
            with torch.no_grad():
                module.weight.fill_(1.0)
                module.bias.zero_()
        if isinstance(module, (nn.Conv2d, nn.Linear)):
            nn.init.trunc_normal_(module.weight, std=0.02)
            nn.init.constant_(module.bias, 0)

    def stage_maps(self, x):
        """the four stage outputs (strides 4 / 8 / 16 / 32), un-normalised"""
        outs = []
        for down, stage in zip(self.downsample_layers, self.stages):
            x = stage(down(x))
            outs.append(x)
        return outs

    def forward_features(self, x, masks=None):
        if isinstance(x, torch.Tensor):
            return self.forward_features_list([x], [masks])[0]
        return self.forward_features_list(x, masks)

    def forward_features_list(self, x_list, masks_list):
        output = []
        for x, masks in zip(x_list, masks_list):
            x = self.stage_maps(x)[-1]
            n, c = x.shape[:2]
            x_pool = HF.global_avg_pool(x).reshape(n, 1, c)
            x = _tokens(x)
            # [CLS] and the patch tokens as [N, HW + 1, C]: one LayerNorm over the rows
            x_norm = self.norm(torch.cat([x_pool, x], dim=1))
            output.append({
                'x_norm_clstoken': x_norm[:, 0],
                'x_storage_tokens': x_norm[:, 1:self.n_storage_tokens + 1],
                'x_norm_patchtokens': x_norm[:, self.n_storage_tokens + 1:],
                'x_prenorm': x,
                'masks': masks,
            })
        return output

    def forward(self, *args, is_training=False, **kwargs):
        ret = self.forward_features(*args, **kwargs)
        if is_training:
            return ret
        return self.head(ret['x_norm_clstoken'])

    def _get_intermediate_layers(self, x, n=1):
        if self.patch_size is not None:
            raise NotImplementedError('ever_amd ConvNeXt: patch_size resizing (anti-aliased bilinear interpolation of the '
                                      'feature maps) has no HIP kernel; build the model with patch_size=None')
        total = len(self.downsample_layers)
        take = range(total - n, total) if isinstance(n, int) else n
        maps = self.stage_maps(x)
        output = [[HF.global_avg_pool(m).reshape(m.shape[0], m.shape[1]), m] for i, m in enumerate(maps) if i in take]
        if len(output) != len(take):
            raise ValueError(f'get_intermediate_layers: stages {list(take)} requested, the model has {total}')
        return output

    def get_intermediate_layers(self, x, n=1, reshape=False, return_class_token=False, norm=True):
        outputs = self._get_intermediate_layers(x, n)
        norms = (self.norms[-n:] if isinstance(n, int) else [self.norms[i] for i in n]) if norm else [None] * len(outputs)
        result = []
        for (cls_token, patches), nm in zip(outputs, norms):
            if isinstance(nm, nn.LayerNorm):
                cls_token = nm(cls_token)
                # the rows of the map ARE the tokens: normalise in place of the reference's flatten / permute / reshape
                patches = HF.layer_norm(patches, nm.weight, nm.bias, nm.eps, channel_dim=1)
            if not reshape:
                patches = _tokens(patches)
            result.append((cls_token, patches))
        class_tokens = [out[0] for out in result]
        patch_outs = [out[1] for out in result]
        if return_class_token:
            return tuple(zip(patch_outs, class_tokens))
        return tuple(patch_outs)


convnext_sizes = {
    'tiny': dict(depths=[3, 3, 9, 3], dims=[96, 192, 384, 768]),
    'small': dict(depths=[3, 3, 27, 3], dims=[96, 192, 384, 768]),
    'base': dict(depths=[3, 3, 27, 3], dims=[128, 256, 512, 1024]),
    'large': dict(depths=[3, 3, 27, 3], dims=[192, 384, 768, 1536]),
}


def get_convnext_arch(arch_name):
    try:
        size = convnext_sizes[arch_name.split('_')[1]]
    except KeyError:
        raise NotImplementedError(f'unknown ConvNeXt size in {arch_name!r}: one of {sorted(convnext_sizes)}') from None
    return partial(ConvNeXt, **size)
