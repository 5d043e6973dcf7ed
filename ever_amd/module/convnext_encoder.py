"""ConvNeXtEncoder ERModule: the ConvNeXt of module/dinov3/convnext.py as a segmentation backbone.  Returns the four stage
maps at output strides 4 / 8 / 16 / 32 with `dims` channels as a list — what FPN takes from ResNetEncoder.  Pretrained
weights come from a local `weight_path` only; nothing is ever fetched."""
import torch

from ..core import logger, registry
from ..interface import ERModule
from .dinov3.convnext import convnext_sizes, get_convnext_arch

_logger = logger.get_logger()
__all__ = ['ConvNeXtEncoder']

default_config = dict(
    convnext_type='convnext_tiny',
    in_channels=3,
    drop_path_rate=0.0,
    layer_scale_init_value=1e-6,
    pretrained=False,
    weight_path=None,
    frozen_stages=-1,
)


@registry.MODEL.register(verbose=False)
class ConvNeXtEncoder(ERModule):
    def __init__(self, config=default_config):
        super().__init__(config)
        cfg = self.config
        self.convnext = get_convnext_arch(cfg.convnext_type)(in_chans=cfg.in_channels, drop_path_rate=cfg.drop_path_rate,
                                                             layer_scale_init_value=cfg.layer_scale_init_value)
        if cfg.pretrained:
            if cfg.weight_path is None:
                raise ValueError(f'ever_amd ConvNeXtEncoder: pretrained=True needs weight_path (a local state dict of '
                                 f'{cfg.convnext_type}); nothing is downloaded')
            state = torch.load(cfg.weight_path, map_location=torch.device('cpu'))
            res = self.convnext.load_state_dict(state, strict=False)
            _logger.info(f'ConvNeXtEncoder: missing_keys {res.missing_keys}, unexpected_keys {res.unexpected_keys}')
        else:
            self.convnext.init_weights()
        self._freeze_stages()
        _logger.info('ConvNeXtEncoder: pretrained = {}'.format(cfg.pretrained))

    def _frozen(self):
        """modules of the first `frozen_stages` (down-sampling layer, stage) pairs"""
        k = max(0, int(self.config.frozen_stages))
        return [m for i in range(min(k, 4)) for m in (self.convnext.downsample_layers[i], self.convnext.stages[i])]

    def _freeze_stages(self):
        for m in self._frozen():
            m.eval()
            for p in m.parameters():
                p.requires_grad = False

    def train(self, mode=True):
        super().train(mode)
        for m in self._frozen():
            m.eval()
        return self

    def forward(self, x):
        return self.convnext.stage_maps(x)

    def output_channels(self):
        """(96, 192, 384, 768) for convnext_tiny / small, (128, ..., 1024) for base, (192, ..., 1536) for large"""
        return tuple(convnext_sizes[self.config.convnext_type.split('_')[1]]['dims'])

    def set_default_config(self):
        self.config.update(default_config)
