"""The convolutional half of the reference's `ever.module.dinov3` (models/convnext.py) on the HIP path.  The transformer
half (vision_transformer.py: attention, RoPE, RMSNorm) has no kernels here."""
from . import convnext
from .convnext import Block, ConvNeXt, DropPath, LayerNorm, convnext_sizes, get_convnext_arch

__all__ = ['convnext', 'Block', 'ConvNeXt', 'DropPath', 'LayerNorm', 'convnext_sizes', 'get_convnext_arch']
