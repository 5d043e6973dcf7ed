"""ViTEncoder ERModule: the DINOv3 vision transformer of module/dinov3/vision_transformer.py as a segmentation backbone.  Four
blocks' normalised patch tokens, taken as stride-16 maps, are returned either as they are (`pyramid=False`) or resampled to
output strides 4 / 8 / 16 / 32 by parameter-free layers that already have kernels (bilinear x4, bilinear x2, identity,
max-pool 3x3 / 2) — the list FPN takes from ResNetEncoder.  Pretrained weights come from a local `weight_path` only; nothing is
ever fetched."""
import torch
import torch.nn as nn

from ..core import logger, registry
from ..interface import ERModule
from .dinov3 import vision_transformer as vits
from .layers import MaxPool2d, UpsamplingBilinear2d

_logger = logger.get_logger()
__all__ = ['ViTEncoder']

VIT_TYPES = ('vit_small', 'vit_base', 'vit_large', 'vitl16_sat493m')

default_config = dict(
    vit_type='vit_small',
    vit_kwargs=dict(),
    in_channels=3,
    out_indices=None,
    pyramid=True,
    pretrained=False,
    weight_path=None,
    frozen_blocks=-1,
)


@registry.MODEL.register(verbose=False)
class ViTEncoder(ERModule):
    def __init__(self, config=default_config):
        super().__init__(config)
        cfg = self.config
        if cfg.vit_type not in VIT_TYPES:
            raise NotImplementedError(f'ever_amd ViTEncoder: unknown vit_type {cfg.vit_type!r}: one of {VIT_TYPES}')
        kwargs = dict(cfg.vit_kwargs)
        if cfg.vit_type != 'vitl16_sat493m':       # (the released configuration fixes fp32 itself)
            kwargs.setdefault('pos_embed_rope_dtype', 'fp32')
        self.vit = getattr(vits, cfg.vit_type)(in_chans=cfg.in_channels, **kwargs)
        depth = len(self.vit.blocks)
        self.out_indices = (list(cfg.out_indices) if cfg.out_indices is not None
                            else [depth // 4 * (i + 1) - 1 for i in range(4)])
        if len(self.out_indices) != 4 or not all(0 <= i < depth for i in self.out_indices):
            raise ValueError(f'ever_amd ViTEncoder: out_indices {self.out_indices}: four blocks of 0..{depth - 1}')
        if cfg.pretrained:
            if cfg.weight_path is None:
                raise ValueError(f'ever_amd ViTEncoder: pretrained=True needs weight_path (a local state dict of {cfg.vit_type}); '
                                 'nothing is downloaded')
            state = torch.load(cfg.weight_path, map_location=torch.device('cpu'))
            res = self.vit.load_state_dict(state, strict=False)
            _logger.info(f'ViTEncoder: missing_keys {res.missing_keys}, unexpected_keys {res.unexpected_keys}')
        else:
            self.vit.init_weights()
        self.resample = nn.ModuleList([UpsamplingBilinear2d(scale_factor=4), UpsamplingBilinear2d(scale_factor=2), nn.Identity(),
                                       MaxPool2d(kernel_size=3, stride=2, padding=1)]) if cfg.pyramid else None
        self._freeze_blocks()
        _logger.info('ViTEncoder: pretrained = {}'.format(cfg.pretrained))

    def _frozen(self):
        """with frozen_blocks = k > 0: the patch embedding and the first k blocks"""
        k = max(0, int(self.config.frozen_blocks))
        return ([self.vit.patch_embed] + list(self.vit.blocks[:k])) if k > 0 else []

    def _freeze_blocks(self):
        frozen = self._frozen()
        for m in frozen:
            m.eval()
            for p in m.parameters():
                p.requires_grad = False
        if frozen:
            for name in ('cls_token', 'storage_tokens', 'mask_token'):
                if hasattr(self.vit, name):
                    getattr(self.vit, name).requires_grad = False

    def train(self, mode=True):
        super().train(mode)
        for m in self._frozen():
            m.eval()
        return self

    def forward(self, x):
        maps = self.vit.get_intermediate_layers(x, n=self.out_indices, reshape=True, norm=True)
        if self.resample is None:
            return list(maps)
        return [op(m) for op, m in zip(self.resample, maps)]

    def output_channels(self):
        """(384,) * 4 for vit_small, (768,) * 4 for vit_base, (1024,) * 4 for vit_large and vitl16_sat493m"""
        return (self.vit.embed_dim,) * 4

    def set_default_config(self):
        self.config.update(default_config)
