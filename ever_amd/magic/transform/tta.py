"""Test-time augmentation (reference ever/magic/transform/tta.py): the model runs once per transformed copy of the image (one
call each, as the reference: batching the copies would change the convolutions' per-tensor operand scale) and the outputs,
taken back by the inverse transforms, are averaged.

On fp32 CUDA outputs the inverse transforms and `sum(outs) / len(outs)` are ONE pass (`hip.transform.d4_mean`, bit for bit the
reference expression): a symmetry of the square enters as its raw model output with the inverse op, a `Scale` output after its
bilinear inverse and any other `Transform` after its own `inv_transform`, both with op 0."""
import torch
import torch.nn as nn

from ...hip.transform import d4_inverse, d4_mean
from ...interface.transform_base import MultiTransform
from . import segm

__all__ = [
    'tta',
    'TestTimeAugmentation'
]

_D4_TYPES = (segm.Identity, segm.Rotate90k, segm.HorizontalFlip, segm.VerticalFlip, segm.Transpose)   # exact types only


def _fusable(ts):
    return (all(segm.on_kernels(t) for t in ts) and len({tuple(t.shape[:2]) for t in ts}) == 1
            and not (torch.is_grad_enabled() and any(t.requires_grad for t in ts)))


def _merge(trans, outs):
    """sum(trans.inv_transform(outs)) / len(outs)"""
    ts = trans._trans_list
    if not (len(outs) and len(outs) == len(ts) and _fusable(outs)):
        outs = trans.inv_transform(outs)
        return sum(outs) / len(outs)
    known = [type(t) in _D4_TYPES for t in ts]
    terms = [o if k else t.inv_transform(o) for t, o, k in zip(ts, outs, known)]
    ops = [d4_inverse(t.d4_op) if k else 0 for t, k in zip(ts, known)]
    sizes = {(o.shape[3], o.shape[2]) if op & 1 else (o.shape[2], o.shape[3]) for o, op in zip(terms, ops)
             if isinstance(o, torch.Tensor) and o.dim() == 4}
    if _fusable(terms) and len(sizes) == 1:
        return d4_mean(terms, ops)
    outs = [t.inv_transform(o) if k else o for t, o, k in zip(ts, terms, known)]
    return sum(outs) / len(outs)


def tta(model, image, tta_config):
    trans = MultiTransform(*tta_config)
    images = trans.transform(image)
    with torch.no_grad():
        outs = [model(im) for im in images]
    return _merge(trans, outs)


class TestTimeAugmentation(nn.Module):
    __test__ = False        # (not a test class, whatever its name says to a collector)

    def __init__(self, module, tta_config):
        super(TestTimeAugmentation, self).__init__()
        self.module = module
        self.trans = MultiTransform(*tta_config)

    @torch.no_grad()
    def forward(self, image):
        images = self.trans.transform(image)
        outs = [self.module(im) for im in images]
        return _merge(self.trans, outs)
