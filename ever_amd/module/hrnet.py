"""HRNetEncoder ERModule (API of reference ever/module/hrnet.py:14-108): returns the four branch maps of HRNetV2 at output
strides 4 / 8 / 16 / 32.  Config keys are the reference's: hrnet_type, pretrained, weight_path, norm_eval, frozen_stages,
with_cp.  The factories are registered in registry.MODEL under their names; pretrained weights come from a local
`weight_path` only."""
import torch
from torch.utils import checkpoint as cp

from ..core import logger, registry
from ..interface import ERModule
from . import _hrnet
from .layers import Conv2d

_logger = logger.get_logger()
__all__ = ['HRNetEncoder']

for _name in ('hrnetv2_w18', 'hrnetv2_w32', 'hrnetv2_w40', 'hrnetv2_w48'):
    registry.MODEL.register(_name, getattr(_hrnet, _name), verbose=False)

default_config = dict(
    hrnet_type='hrnetv2_w18',
    pretrained=False,
    weight_path=None,
    norm_eval=False,
    frozen_stages=-1,
    with_cp=False,
)


@registry.MODEL.register(verbose=False)
class HRNetEncoder(ERModule):
    def __init__(self, config=default_config):
        super().__init__(config)
        self.hrnet = registry.MODEL[self.config.hrnet_type](pretrained=self.config.pretrained,
                                                            weight_path=self.config.weight_path,
                                                            norm_eval=self.config.norm_eval,
                                                            frozen_stages=self.config.frozen_stages)
        _logger.info('HRNetEncoder: pretrained = {}'.format(self.config.pretrained))

    def forward(self, x):
        self.hrnet.check_channels()      # hrnetv2_w18 builds and cannot run (C % 4): said before anything else is looked at
        if self.config.with_cp and torch.is_grad_enabled():
            # activation checkpointing of the whole body, non-reentrant as in ResNetEncoder._run_stage
            return cp.checkpoint(self.hrnet, x, use_reentrant=False)
        return self.hrnet(x)

    def reset_in_channels(self, in_channels):
        if in_channels == 3:
            return
        self.hrnet.add_module('conv1', Conv2d(in_channels, 64, kernel_size=3, stride=2, padding=1, bias=False))

    # stage2..stage4 are exposed read/write so plug-ins can wrap stages (reference hrnet.py:51-79)
    def _stage(name):  # noqa: N805
        def getter(self):
            return getattr(self.hrnet, name)

        def setter(self, value):
            delattr(self.hrnet, name)
            setattr(self.hrnet, name, value)

        return property(getter, setter)

    stage2, stage3, stage4 = _stage('stage2'), _stage('stage3'), _stage('stage4')
    del _stage

    def set_default_config(self):
        self.config.update(default_config)

    def output_channels(self):
        """(18, 36, 72, 144) for hrnetv2_w18, ... (48, 96, 192, 384) for hrnetv2_w48: the last stage's branch widths"""
        cfg = self.hrnet.stage4_cfg
        e = _hrnet.blocks_dict[cfg['block']].expansion
        return tuple(c * e for c in cfg['num_channels'])

    def with_context_block(self, ratio):
        raise NotImplementedError('ever_amd HRNetEncoder: the global-context block plug-in has no HIP kernels')

    def with_squeeze_excitation(self, inv_ratio):
        raise NotImplementedError('ever_amd HRNetEncoder: the squeeze-and-excitation plug-in has no HIP kernels')
