"""The DINOv3 vision transformer on the HIP path (API, child order and state-dict keys of reference
ever/module/dinov3/models/vision_transformer.py; layers in vit_layers.py).  The hot path of a block is the fused RoPE attention
kernel (HF.attention); the token prefix is HF.prepend_tokens.

Out of scope, raising NotImplementedError at construction or on use: norm_layer='rmsnorm', ffn_layer='swiglu*' (vit_7b,
vit7b16_sat493m), masks, drop_path_rate > 0 in training mode, RoPE tables of a dtype other than fp32.  Pretrained weights come
from a local file only; nothing is ever fetched."""
import logging
from functools import partial

import torch
import torch.nn as nn

from ...hip import functional as HF
from ..layers import LayerNorm
from .vit_layers import LayerScale, Mlp, PatchEmbed, RopePositionEmbedding, SelfAttentionBlock

__all__ = ['init_weights_vit', 'DinoVisionTransformer', 'vit_small', 'vit_base', 'vit_large', 'vit_so400m', 'vit_huge2',
           'vit_giant2', 'vitl16_sat493m']

logger = logging.getLogger('dinov3')

ffn_layer_dict = {'mlp': Mlp}
norm_layer_dict = {
    'layernorm': partial(LayerNorm, eps=1e-6),
    'layernormbf16': partial(LayerNorm, eps=1e-5),
}
dtype_dict = {'fp32': torch.float32, 'fp16': torch.float16, 'bf16': torch.bfloat16}


def init_weights_vit(module, name=''):
    if isinstance(module, nn.Linear):
        nn.init.trunc_normal_(module.weight, std=0.02)
        if module.bias is not None:
            nn.init.zeros_(module.bias)
    if isinstance(module, (nn.LayerNorm, LayerScale, PatchEmbed)):
        module.reset_parameters()


def _named_apply(fn, module, name=''):
    """fn(module, name) on every descendant, children first"""
    for child_name, child in module.named_children():
        _named_apply(fn, child, f'{name}.{child_name}' if name else child_name)
    fn(module, name)


class DinoVisionTransformer(nn.Module):
    def __init__(self, *, img_size=224, patch_size=16, in_chans=3, pos_embed_rope_base=100.0, pos_embed_rope_min_period=None,
                 pos_embed_rope_max_period=None, pos_embed_rope_normalize_coords='separate', pos_embed_rope_shift_coords=None,
                 pos_embed_rope_jitter_coords=None, pos_embed_rope_rescale_coords=None, pos_embed_rope_dtype='bf16',
                 embed_dim=768, depth=12, num_heads=12, ffn_ratio=4.0, qkv_bias=True, drop_path_rate=0.0, layerscale_init=None,
                 norm_layer='layernorm', ffn_layer='mlp', ffn_bias=True, proj_bias=True, n_storage_tokens=0, mask_k_bias=False,
                 untie_cls_and_patch_norms=False, untie_global_and_local_cls_norm=False, device=None, **ignored_kwargs):
        super().__init__()
        if ignored_kwargs:
            logger.warning(f'Ignored kwargs: {ignored_kwargs}')
        if norm_layer not in norm_layer_dict:
            raise NotImplementedError(f'ever_amd DinoVisionTransformer: norm_layer={norm_layer!r} has no kernel here '
                                      f'(one of {sorted(norm_layer_dict)}; rmsnorm is out of scope)')
        if ffn_layer not in ffn_layer_dict:
            raise NotImplementedError(f'ever_amd DinoVisionTransformer: ffn_layer={ffn_layer!r} has no kernel here '
                                      f'(one of {sorted(ffn_layer_dict)}; swiglu is out of scope)')
        norm_cls = norm_layer_dict[norm_layer]
        self.num_features = self.embed_dim = embed_dim
        self.n_blocks = depth
        self.num_heads = num_heads
        self.patch_size = patch_size
        self.pos_embed_rope_dtype = pos_embed_rope_dtype
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim,
                                      flatten_embedding=False)
        self.cls_token = nn.Parameter(torch.empty(1, 1, embed_dim, device=device))
        self.n_storage_tokens = n_storage_tokens
        if n_storage_tokens > 0:
            self.storage_tokens = nn.Parameter(torch.empty(1, n_storage_tokens, embed_dim, device=device))
        self.rope_embed = RopePositionEmbedding(
            embed_dim=embed_dim, num_heads=num_heads, base=pos_embed_rope_base, min_period=pos_embed_rope_min_period,
            max_period=pos_embed_rope_max_period, normalize_coords=pos_embed_rope_normalize_coords,
            shift_coords=pos_embed_rope_shift_coords, jitter_coords=pos_embed_rope_jitter_coords,
            rescale_coords=pos_embed_rope_rescale_coords, dtype=dtype_dict[pos_embed_rope_dtype], device=device)
        self.chunked_blocks = False
        self.blocks = nn.ModuleList([
            SelfAttentionBlock(dim=embed_dim, num_heads=num_heads, ffn_ratio=ffn_ratio, qkv_bias=qkv_bias, proj_bias=proj_bias,
                               ffn_bias=ffn_bias, drop_path=drop_path_rate, norm_layer=norm_cls, act_layer=nn.GELU,
                               ffn_layer=ffn_layer_dict[ffn_layer], init_values=layerscale_init, mask_k_bias=mask_k_bias,
                               device=device)
            for _ in range(depth)])
        self.norm = norm_cls(embed_dim)             # everything, or the patch tokens when a norm below is untied
        self.untie_cls_and_patch_norms = untie_cls_and_patch_norms
        self.cls_norm = norm_cls(embed_dim) if untie_cls_and_patch_norms else None
        self.untie_global_and_local_cls_norm = untie_global_and_local_cls_norm
        self.local_cls_norm = norm_cls(embed_dim) if untie_global_and_local_cls_norm else None   # training, second crop list only
        self.head = nn.Identity()
        self.mask_token = nn.Parameter(torch.empty(1, embed_dim, device=device))

    def init_weights(self):
        self.rope_embed._init_weights()
        nn.init.normal_(self.cls_token, std=0.02)
        if self.n_storage_tokens > 0:
            nn.init.normal_(self.storage_tokens, std=0.02)
        nn.init.zeros_(self.mask_token)
        _named_apply(init_weights_vit, self)

    def prepare_tokens_with_masks(self, x, masks=None):
        if masks is not None:
            raise NotImplementedError('ever_amd DinoVisionTransformer: masks (iBOT mask tokens) are out of scope')
        x = self.patch_embed(x)
        _, h, w, _ = x.shape
        # parameter-sized, as written in the reference: mask_token takes its zero gradient
        prefix = self.cls_token + 0 * self.mask_token
        if self.n_storage_tokens > 0:
            prefix = torch.cat([prefix, self.storage_tokens], dim=1)
        return HF.prepend_tokens(x.flatten(1, 2), prefix[0]), (h, w)

    def _rope_source(self, hw):
        """A callable giving the (sin, cos) of a block.  In eval mode or without augmentation every block of the reference
        computes the same table: it is computed once per forward here.  With augmentation in training mode every block draws
        its own, as the reference's does."""
        if self.rope_embed is None:
            return lambda: None
        if self.pos_embed_rope_dtype != 'fp32':
            raise NotImplementedError(f'ever_amd DinoVisionTransformer: pos_embed_rope_dtype={self.pos_embed_rope_dtype!r}: the '
                                      'attention kernel takes fp32 RoPE tables only; build the model with pos_embed_rope_dtype="fp32"')
        if self.rope_embed.augments():
            return lambda: self.rope_embed(H=hw[0], W=hw[1])
        table = self.rope_embed(H=hw[0], W=hw[1])
        return lambda: table

    def _split_norm(self, x, cls_norm):
        """the prefix rows and the patch rows under their own norms; the slices are copied into dense tensors of their own"""
        p = self.n_storage_tokens + 1
        dense = torch.contiguous_format
        return cls_norm(x[:, :p].clone(memory_format=dense)), self.norm(x[:, p:].clone(memory_format=dense))

    def forward_features_list(self, x_list, masks_list):
        xs, ropes = [], []
        for x, masks in zip(x_list, masks_list):
            t, hw = self.prepare_tokens_with_masks(x, masks)
            xs.append(t)
            ropes.append(self._rope_source(hw))
        for blk in self.blocks:
            xs = blk(xs, [r() for r in ropes])
        output = []
        p = self.n_storage_tokens + 1
        for idx, (x, masks) in enumerate(zip(xs, masks_list)):
            if self.untie_cls_and_patch_norms or self.untie_global_and_local_cls_norm:
                if self.untie_global_and_local_cls_norm and self.training and idx == 1:
                    cls_reg, patch = self._split_norm(x, self.local_cls_norm)     # the second entry: local crops
                elif self.untie_cls_and_patch_norms:
                    cls_reg, patch = self._split_norm(x, self.cls_norm)
                else:
                    cls_reg, patch = self._split_norm(x, self.norm)
            else:
                x_norm = self.norm(x)
                cls_reg, patch = x_norm[:, :p], x_norm[:, p:]
            output.append({
                'x_norm_clstoken': cls_reg[:, 0],
                'x_storage_tokens': cls_reg[:, 1:],
                'x_norm_patchtokens': patch,
                'x_prenorm': x,
                'masks': masks,
            })
        return output

    def forward_features(self, x, masks=None):
        if isinstance(x, torch.Tensor):
            return self.forward_features_list([x], [masks])[0]
        return self.forward_features_list(x, masks)

    def _get_intermediate_layers_not_chunked(self, x, n=1):
        x, hw = self.prepare_tokens_with_masks(x)
        total = len(self.blocks)
        take = range(total - n, total) if isinstance(n, int) else n
        rope = self._rope_source(hw)
        output = []
        for i, blk in enumerate(self.blocks):
            x = blk(x, rope())
            if i in take:
                output.append(x)
        if len(output) != len(take):
            raise AssertionError(f'only {len(output)} / {len(take)} blocks found')
        return output

    def get_intermediate_layers(self, x, *, n=1, reshape=False, return_class_token=False, return_extra_tokens=False, norm=True):
        outputs = self._get_intermediate_layers_not_chunked(x, n)
        p = self.n_storage_tokens + 1
        if norm:
            if self.untie_cls_and_patch_norms:
                outputs = [torch.cat(self._split_norm(out, self.cls_norm), dim=1) for out in outputs]
            else:
                outputs = [self.norm(out) for out in outputs]
        class_tokens = [out[:, 0] for out in outputs]
        extra_tokens = [out[:, 1:p] for out in outputs]
        outputs = [out[:, p:] for out in outputs]
        if reshape:
            b, _, h, w = x.shape
            # One dense copy of the patch rows (the slice keeps the batch stride of all N tokens): its [B, h, w, C] memory IS
            # the logical [B, C, h, w] map of the HIP path, so the reference's permute is a view of it and the consumers take
            # it without a layout pass.
            dense = torch.contiguous_format
            outputs = [out.clone(memory_format=dense).view(b, h // self.patch_size, w // self.patch_size, -1).permute(0, 3, 1, 2)
                       for out in outputs]
        if return_class_token and return_extra_tokens:
            return tuple(zip(outputs, class_tokens, extra_tokens))
        if return_class_token:
            return tuple(zip(outputs, class_tokens))
        if return_extra_tokens:
            return tuple(zip(outputs, extra_tokens))
        return tuple(outputs)

    def forward(self, *args, is_training=False, **kwargs):
        ret = self.forward_features(*args, **kwargs)
        if is_training:
            return ret
        return self.head(ret['x_norm_clstoken'])


def _sized(patch_size, kwargs, **size):
    """the named size; a keyword of the caller's wins over it (a reduced model of the same constructor)"""
    return DinoVisionTransformer(**{**size, 'patch_size': patch_size, **kwargs})


def vit_small(patch_size=16, **kwargs):
    return _sized(patch_size, kwargs, embed_dim=384, depth=12, num_heads=6, ffn_ratio=4)


def vit_base(patch_size=16, **kwargs):
    return _sized(patch_size, kwargs, embed_dim=768, depth=12, num_heads=12, ffn_ratio=4)


def vit_large(patch_size=16, **kwargs):
    return _sized(patch_size, kwargs, embed_dim=1024, depth=24, num_heads=16, ffn_ratio=4)


def vit_so400m(patch_size=16, **kwargs):
    return _sized(patch_size, kwargs, embed_dim=1152, depth=27, num_heads=18, ffn_ratio=3.777777778)


def vit_huge2(patch_size=16, **kwargs):
    return _sized(patch_size, kwargs, embed_dim=1280, depth=32, num_heads=20, ffn_ratio=4)


def vit_giant2(patch_size=16, **kwargs):
    """embed_dim 1536 over 24 heads: 64 per head"""
    return _sized(patch_size, kwargs, embed_dim=1536, depth=40, num_heads=24, ffn_ratio=4)


def vitl16_sat493m(pretrained=None, drop_path_rate=0., **kwargs):
    """The satellite-pretrained ViT-L/16.  pretrained: a LOCAL state-dict file, loaded strictly (370 keys)."""
    model = vit_large(pos_embed_rope_base=100, pos_embed_rope_normalize_coords='separate', pos_embed_rope_rescale_coords=2,
                      pos_embed_rope_dtype='fp32', qkv_bias=True, drop_path_rate=drop_path_rate, layerscale_init=1.0e-05,
                      norm_layer='layernormbf16', ffn_layer='mlp', ffn_bias=True, proj_bias=True, n_storage_tokens=4,
                      mask_k_bias=True, untie_global_and_local_cls_norm=True, **kwargs)
    if pretrained is not None:
        msg = model.load_state_dict(torch.load(pretrained, map_location='cpu', weights_only=False))
        logger.info(f'load checkpoint from {pretrained}: {msg}')
    return model
