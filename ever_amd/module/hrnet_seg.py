"""HRNetV2 segmentation model = HRNetEncoder + HRNetHead + pixel loss, as an ERModule.

The reference ships the encoder (ever/module/hrnet.py) and the head (hrnet_head.py) and leaves the composition to user
projects, as for FarSeg and DeepLabv3+ (module/farseg.py, module/deeplab.py): `forward(x, y)` returns a dict of `*_loss` in
training and the prediction in eval.  State-dict prefixes are `en.` and `head.`; the head's `in_channels` defaults to the
sum of the encoder's output channels."""
from ..core import registry
from ..hip import functional as HF
from ..hip import timing
from ..interface import ERModule
from .farseg import FarSeg, _SigmoidNoGrad
from .hrnet import HRNetEncoder
from .hrnet_head import HRNetHead

__all__ = ['HRNetSeg']


@registry.MODEL.register(verbose=False)
class HRNetSeg(ERModule):
    def __init__(self, config):
        super().__init__(config)
        self.en = HRNetEncoder(self.config.encoder)
        head = dict(self.config.head)
        decoder = dict(head.get('hrnet_decoder', dict()))
        decoder.setdefault('in_channels', sum(self.en.output_channels()))
        head['hrnet_decoder'] = decoder
        self.head = HRNetHead(head)
        if self.config.encoder.get('in_channels', 3) != 3:
            self.en.reset_in_channels(self.config.encoder.in_channels)

    def forward(self, x, y=None):
        self.en.hrnet.check_channels()
        HF._require_cuda(x, 'HRNetSeg input')
        with timing.scope('encoder'):
            feats = self.en(x)
        logits = self.head(feats)
        if self.training:
            if isinstance(y, dict):
                y = y[self.config.loss.get('label_key', 'cls')]
            return self.loss(logits, y)
        if logits.shape[1] == 1:
            return _SigmoidNoGrad(logits)
        return logits

    # cross-entropy with ignore_index for several classes, BCE + dice for one: FarSeg's conventions
    loss = FarSeg.loss

    def set_default_config(self):
        self.config.update(dict(
            encoder=dict(hrnet_type='hrnetv2_w48', pretrained=False, weight_path=None, norm_eval=False, frozen_stages=-1,
                         with_cp=False, in_channels=3),
            head=dict(),
            loss=dict(ignore_index=255, bce=True, dice=True),
        ))
