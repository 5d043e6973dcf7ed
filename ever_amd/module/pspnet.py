"""PSPNet segmentation model = ResNetEncoder (output stride 8) + PPMHead on c5 + pixel loss, as an ERModule.

The reference ships the head (ever/module/ppm.py) and the encoder and leaves the composition to user projects, as for
FarSeg and DeepLabv3+ (module/deeplab.py): `forward(x, y)` returns a dict of `*_loss` in training and the prediction in
eval.  No auxiliary head.  State-dict prefixes are `en.` and `head.`."""
from ..core import registry
from ..hip import functional as HF
from ..hip import timing
from ..interface import ERModule
from .farseg import FarSeg, _SigmoidNoGrad
from .ppm import PPMHead
from .resnet import ResNetEncoder

__all__ = ['PSPNet']


@registry.MODEL.register(verbose=False)
class PSPNet(ERModule):
    def __init__(self, config):
        super().__init__(config)
        self.en = ResNetEncoder(self.config.encoder)
        self.head = PPMHead(self.config.head)

    def forward(self, x, y=None):
        HF._require_cuda(x, 'PSPNet input')
        with timing.scope('encoder'):
            feats = self.en(x)
        logits = self.head(feats[-1])
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
            encoder=dict(resnet_type='resnet50', include_conv5=True, batchnorm_trainable=True, pretrained=False,
                         freeze_at=0, output_stride=8, with_cp=(False, False, False, False), in_channels=3),
            head=dict(),
            loss=dict(ignore_index=255, bce=True, dice=True),
        ))
