"""The layers of the DINOv3 vision transformer on the HIP path (names, constructor signatures, child order and state-dict
keys of reference ever/module/dinov3/layers/{patch_embed,rope_position_encoding,attention,ffn_layers,layer_scale,block}.py).

Tokens [B, N, C] are the NHWC memory of a logical [B, C, N, 1] map, so a Linear on the channels is a 1x1 convolution with the
2-D weight viewed [out, in, 1, 1] (the parameter stays 2-D: reference checkpoints load strictly), the norms are
HF.layer_norm on the last axis, GELU is HN.gelu, both residual tails of a block are HF.scale_residual through the map view,
and attention is ONE HF.attention call on the QKV Linear's output: none of the reference's reshapes, unbinds and transposes is
materialised.  Not ported: CausalSelfAttention, fp8_linear, sparse_linear, dino_head, RMSNorm, SwiGLU."""
import math

import numpy as np
import torch
import torch.nn as nn

from ...hip import functional as HF
from ...hip import functional_next as HN
from ..layers import Conv2d

__all__ = ['PatchEmbed', 'RopePositionEmbedding', 'LinearKMaskedBias', 'SelfAttention', 'Mlp', 'LayerScale',
           'SelfAttentionBlock', 'token_linear']


def _token_map(x):
    """[B, N, C] tokens -> the logical [B, C, N, 1] map over the same (NHWC) memory"""
    if not x.is_contiguous():
        x = x.contiguous()
    b, n, c = x.shape
    return x.view(b, n, 1, c).permute(0, 3, 1, 2)


def _map_tokens(y):
    """logical [B, C, N, 1] map over NHWC memory -> [B, N, C] tokens, a view"""
    y = HF.as_nhwc(y, 'vit')
    b, c, n, w = y.shape
    return y.permute(0, 2, 3, 1).reshape(b, n * w, c)


def token_linear(x, weight, bias):
    """F.linear on the channels of [B, N, C] tokens as a 1x1 convolution of the convolution planner"""
    if x.dim() != 3:
        raise NotImplementedError(f'ever_amd ViT Linear: only [B, N, C] tokens have a kernel, got {tuple(x.shape)}')
    return _map_tokens(HF.conv2d(_token_map(x), weight.view(weight.shape[0], weight.shape[1], 1, 1), bias))


class _TokenLinear(nn.Linear):
    """nn.Linear (2-D weight, same keys) on [B, N, C] tokens."""

    def forward(self, x):
        return token_linear(x, self.weight, self.bias)


def _pair(v):
    if isinstance(v, tuple):
        if len(v) != 2:
            raise ValueError(f'a size is an int or a pair, got {v}')
        return v
    if not isinstance(v, int):
        raise ValueError(f'a size is an int or a pair, got {v!r}')
    return (v, v)


class PatchEmbed(nn.Module):
    """(B, C, H, W) image -> patch tokens: one strided convolution, whose NHWC output already is [B, h, w, D]."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, norm_layer=None, flatten_embedding=True):
        super().__init__()
        self.img_size = _pair(img_size)
        self.patch_size = _pair(patch_size)
        self.patches_resolution = (self.img_size[0] // self.patch_size[0], self.img_size[1] // self.patch_size[1])
        self.num_patches = self.patches_resolution[0] * self.patches_resolution[1]
        self.in_chans = in_chans
        self.embed_dim = embed_dim
        self.flatten_embedding = flatten_embedding
        self.proj = Conv2d(in_chans, embed_dim, kernel_size=self.patch_size, stride=self.patch_size)
        self.norm = norm_layer(embed_dim) if norm_layer else nn.Identity()

    def forward(self, x):
        y = HF.as_nhwc(self.proj(x), 'patch_embed')
        b, c, h, w = y.shape
        y = self.norm(y.permute(0, 2, 3, 1).reshape(b, h * w, c))
        return y if self.flatten_embedding else y.reshape(b, h, w, c)

    def flops(self):
        h, w = self.patches_resolution
        return h * w * self.embed_dim * (self.in_chans * self.patch_size[0] * self.patch_size[1] + (self.norm is not None))

    def reset_parameters(self):
        bound = math.sqrt(1 / (self.in_chans * (self.patch_size[0] ** 2)))
        nn.init.uniform_(self.proj.weight, -bound, bound)
        if self.proj.bias is not None:
            nn.init.uniform_(self.proj.bias, -bound, bound)


class RopePositionEmbedding(nn.Module):
    """Axial RoPE tables without learnable weights: (sin, cos) of [H W, D_head] for an H x W patch grid.  The tables are tiny
    and are evaluated with the reference's torch expressions, in its order, on the buffer's device — the training-time
    shift / jitter / rescale draws included, so the same seed gives the reference's tables.  `periods` keeps the
    constructor's dtype."""

    def __init__(self, embed_dim, *, num_heads, base=100.0, min_period=None, max_period=None, normalize_coords='separate',
                 shift_coords=None, jitter_coords=None, rescale_coords=None, dtype=None, device=None):
        super().__init__()
        if embed_dim % (4 * num_heads) != 0:
            raise AssertionError(f'embed_dim {embed_dim} is not a multiple of 4 x {num_heads} heads')
        both = min_period is not None and max_period is not None
        if (base is None) != both:
            raise ValueError('Either `base` or `min_period`+`max_period` must be provided.')
        self.base = base
        self.min_period = min_period
        self.max_period = max_period
        self.D_head = embed_dim // num_heads
        self.normalize_coords = normalize_coords
        self.shift_coords = shift_coords
        self.jitter_coords = jitter_coords
        self.rescale_coords = rescale_coords
        self.dtype = dtype
        self.register_buffer('periods', torch.empty(self.D_head // 4, device=device, dtype=dtype), persistent=True)
        self._init_weights()

    def augments(self):
        """True where a training-mode forward draws random numbers (so every call gives another table)"""
        return self.training and not (self.shift_coords is None and self.jitter_coords is None and self.rescale_coords is None)

    def forward(self, *, H, W):
        kw = dict(device=self.periods.device, dtype=self.dtype)
        if self.normalize_coords == 'separate':
            div_h, div_w = H, W
        elif self.normalize_coords == 'max':
            div_h = div_w = max(H, W)
        elif self.normalize_coords == 'min':
            div_h = div_w = min(H, W)
        else:
            raise ValueError(f'Unknown normalize_coords: {self.normalize_coords}')
        ch = torch.arange(0.5, H, **kw) / div_h
        cw = torch.arange(0.5, W, **kw) / div_w
        coords = torch.stack(torch.meshgrid(ch, cw, indexing='ij'), dim=-1).flatten(0, 1)    # [HW, 2] in [0, 1]
        coords = 2.0 * coords - 1.0
        if self.training and self.shift_coords is not None:
            coords += torch.empty(2, **kw).uniform_(-self.shift_coords, self.shift_coords)[None, :]
        if self.training and self.jitter_coords is not None:
            top = np.log(self.jitter_coords)
            coords *= torch.empty(2, **kw).uniform_(-top, top).exp()[None, :]
        if self.training and self.rescale_coords is not None:
            top = np.log(self.rescale_coords)
            coords *= torch.empty(1, **kw).uniform_(-top, top).exp()
        angles = 2 * math.pi * coords[:, :, None] / self.periods[None, None, :]     # [HW, 2, D / 4]
        angles = angles.flatten(1, 2).tile(2)                                        # [HW, D]
        return torch.sin(angles), torch.cos(angles)

    def _init_weights(self):
        kw = dict(device=self.periods.device, dtype=self.dtype)
        quarter = self.D_head // 4
        if self.base is not None:
            periods = self.base ** (2 * torch.arange(quarter, **kw) / (self.D_head // 2))
        else:
            ratio = self.max_period / self.min_period
            periods = ratio ** torch.linspace(0, 1, quarter, **kw)
            periods = periods / ratio
            periods = periods * self.max_period
        self.periods.data = periods


class LinearKMaskedBias(_TokenLinear):
    """The QKV Linear whose bias is multiplied by a `bias_mask` buffer (ones / zeros / ones over the q / k / v thirds in the
    released checkpoints).  As in the reference a fresh instance holds NaN in the mask: its output is NaN until a checkpoint is
    loaded.  The product is 3 C floats and is evaluated as written."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if self.out_features % 3 != 0:
            raise AssertionError(f'{self.out_features} output features are not q, k and v thirds')
        if self.bias is not None:
            self.register_buffer('bias_mask', torch.full_like(self.bias, fill_value=math.nan))

    def forward(self, x):
        bias = self.bias * self.bias_mask.to(self.bias.dtype) if self.bias is not None else None
        return token_linear(x, self.weight, bias)


class SelfAttention(nn.Module):
    def __init__(self, dim, num_heads=8, qkv_bias=False, proj_bias=True, attn_drop=0.0, proj_drop=0.0, mask_k_bias=False,
                 device=None):
        super().__init__()
        if attn_drop or proj_drop:
            raise NotImplementedError('ever_amd SelfAttention: dropout inside the attention is out of scope (attn_drop, proj_drop)')
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = (LinearKMaskedBias if mask_k_bias else _TokenLinear)(dim, dim * 3, bias=qkv_bias, device=device)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = _TokenLinear(dim, dim, bias=proj_bias, device=device)
        self.proj_drop = nn.Dropout(proj_drop)

    def compute_attention(self, qkv, attn_bias=None, rope=None):
        if attn_bias is not None:
            raise NotImplementedError('ever_amd SelfAttention: attention masks or bias are out of scope')
        return HF.attention(qkv, self.num_heads, rope)

    def forward(self, x, attn_bias=None, rope=None):
        return self.proj(self.compute_attention(self.qkv(x), attn_bias=attn_bias, rope=rope))

    def forward_list(self, x_list, attn_bias=None, rope_list=None):
        if len(x_list) != len(rope_list):
            raise AssertionError('one rope per tensor')
        return [self.forward(x, attn_bias=attn_bias, rope=rope) for x, rope in zip(x_list, rope_list)]


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.0, bias=True, device=None):
        super().__init__()
        if drop:
            raise NotImplementedError('ever_amd Mlp: dropout is out of scope (drop)')
        if act_layer is not nn.GELU:
            raise NotImplementedError('ever_amd Mlp: only nn.GELU has a kernel here')
        self.fc1 = _TokenLinear(in_features, hidden_features or in_features, bias=bias, device=device)
        self.act = act_layer()
        self.fc2 = _TokenLinear(hidden_features or in_features, out_features or in_features, bias=bias, device=device)
        self.drop = nn.Dropout(drop)

    def forward(self, x):
        return self.fc2(HN.gelu(self.fc1(x)))

    def forward_list(self, x_list):
        return [self.forward(x) for x in x_list]


class LayerScale(nn.Module):
    """x * gamma.  Inside a SelfAttentionBlock gamma goes into the fused residual tail (HF.scale_residual); called on its own it
    is that tail on a zero base, 0 + gamma * x, which gives gamma its gradient."""

    def __init__(self, dim, init_values=1e-5, inplace=False, device=None):
        super().__init__()
        self.inplace = inplace
        self.gamma = nn.Parameter(torch.empty(dim, device=device))
        self.init_values = init_values

    def reset_parameters(self):
        nn.init.constant_(self.gamma, self.init_values)

    def forward(self, x):
        if x.dim() != 3:
            raise NotImplementedError('ever_amd LayerScale: only [B, N, C] tokens have a kernel outside a block')
        if self.inplace and torch.is_grad_enabled() and x.requires_grad:
            raise NotImplementedError('ever_amd LayerScale: inplace=True under autograd is out of scope')
        m = _token_map(x)
        y = _map_tokens(HF.scale_residual(torch.zeros_like(m), m, self.gamma))
        return x.copy_(y) if self.inplace else y


class SelfAttentionBlock(nn.Module):
    """x + ls1(attn(norm1(x))), then x + ls2(mlp(norm2(x))).  drop_path > 0 in training mode is the reference's batch-subset
    form (randperm, index_add) and raises NotImplementedError on use; eval mode is fine."""

    def __init__(self, dim, num_heads, ffn_ratio=4.0, qkv_bias=False, proj_bias=True, ffn_bias=True, drop=0.0, attn_drop=0.0,
                 init_values=None, drop_path=0.0, act_layer=nn.GELU, norm_layer=None, attn_class=SelfAttention, ffn_layer=Mlp,
                 mask_k_bias=False, device=None):
        super().__init__()
        if norm_layer is None:
            from ..layers import LayerNorm as norm_layer
        self.norm1 = norm_layer(dim)
        self.attn = attn_class(dim, num_heads=num_heads, qkv_bias=qkv_bias, proj_bias=proj_bias, attn_drop=attn_drop,
                               proj_drop=drop, mask_k_bias=mask_k_bias, device=device)
        self.ls1 = LayerScale(dim, init_values=init_values, device=device) if init_values else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = ffn_layer(in_features=dim, hidden_features=int(dim * ffn_ratio), act_layer=act_layer, drop=drop,
                             bias=ffn_bias, device=device)
        self.ls2 = LayerScale(dim, init_values=init_values, device=device) if init_values else nn.Identity()
        self.sample_drop_ratio = drop_path

    @staticmethod
    def _tail(x, z, ls):
        """x + gamma * z in one pass (gamma None without a layer scale)"""
        y = HF.scale_residual(_token_map(x), _token_map(z), getattr(ls, 'gamma', None))
        return _map_tokens(y)

    def _forward(self, x, rope=None):
        if self.training and self.sample_drop_ratio > 0.0:
            raise NotImplementedError('ever_amd SelfAttentionBlock: drop_path_rate > 0 in training mode (batch-subset stochastic '
                                      'depth) is out of scope; build the model with drop_path_rate=0 or run it in eval mode')
        x = self._tail(x, self.attn(self.norm1(x), rope=rope), self.ls1)
        return self._tail(x, self.mlp(self.norm2(x)), self.ls2)

    def forward(self, x_or_x_list, rope_or_rope_list=None):
        if isinstance(x_or_x_list, torch.Tensor):
            return self._forward(x_or_x_list, rope=rope_or_rope_list)
        if isinstance(x_or_x_list, list):
            ropes = rope_or_rope_list if rope_or_rope_list is not None else [None] * len(x_or_x_list)
            return [self._forward(x, rope=r) for x, r in zip(x_or_x_list, ropes)]
        raise AssertionError('a tensor or a list of tensors')
