"""The reference's `ever.module.dinov3` on the HIP path: the convolutional half (models/convnext.py) and the transformer half
(models/vision_transformer.py with the layers of vit_layers.py: patch embedding, axial RoPE, self-attention on the fused RoPE
attention kernel, Mlp, layer scale).  Not ported: RMSNorm, SwiGLU (vit_7b, vit7b16_sat493m), CausalSelfAttention, fp8_linear,
sparse_linear, dino_head."""
from . import convnext, vision_transformer, vit_layers
from .convnext import Block, ConvNeXt, DropPath, LayerNorm, convnext_sizes, get_convnext_arch
from .vision_transformer import (DinoVisionTransformer, init_weights_vit, vit_base, vit_giant2, vit_huge2, vit_large, vit_small,
                                 vit_so400m, vitl16_sat493m)
from .vit_layers import LayerScale, LinearKMaskedBias, Mlp, PatchEmbed, RopePositionEmbedding, SelfAttention, SelfAttentionBlock

__all__ = ['convnext', 'Block', 'ConvNeXt', 'DropPath', 'LayerNorm', 'convnext_sizes', 'get_convnext_arch',
           'vision_transformer', 'vit_layers', 'PatchEmbed', 'RopePositionEmbedding', 'LinearKMaskedBias', 'SelfAttention', 'Mlp',
           'LayerScale', 'SelfAttentionBlock', 'DinoVisionTransformer', 'init_weights_vit', 'vit_small', 'vit_base', 'vit_large',
           'vit_so400m', 'vit_huge2', 'vit_giant2', 'vitl16_sat493m']
