"""The segmentation transforms of test-time augmentation (reference ever/magic/transform/segm.py): the symmetries of the
square and bilinear rescaling, each with its inverse.

An fp32 CUDA tensor goes through the HIP kernels: `hip.transform.d4` (one copy kernel for all eight symmetries) and the
bilinear kernels.  Every other tensor (CPU, another dtype such as an int64 label map, anything while a trace is being
recorded) is an index permutation at the API boundary and evaluates the reference's torch expression."""
import math

import torch
import torch.nn.functional as F

from ...hip import oplib
from ...hip.pointwise import _BilinearFn
from ...hip.transform import D4_HFLIP, D4_IDENTITY, D4_ROT90, D4_TRANSPOSE, D4_VFLIP, d4, d4_inverse
from ...hip._base import as_nhwc
from ...interface.transform_base import Transform

__all__ = ['Identity', 'Rotate90k', 'HorizontalFlip', 'VerticalFlip', 'Transpose', 'Scale', 'on_kernels', 'd4_torch']


def on_kernels(x):
    """the HIP kernels take this tensor"""
    return (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
            and not oplib.tracing())


def d4_torch(x, op):
    """dihedral op `op` as the reference's torch expression"""
    if op == D4_IDENTITY:
        return x
    if op == D4_TRANSPOSE:
        return torch.transpose(x, 2, 3)
    if op == D4_VFLIP:
        return torch.flip(x, [2])
    if op == D4_HFLIP:
        return torch.flip(x, [3])
    if op == 7:
        return torch.flip(torch.transpose(x, 2, 3), [2, 3])
    return torch.rot90(x, {3: 1, 6: 2, 5: 3}[op], [2, 3])


def _apply(x, op):
    if op == D4_IDENTITY:
        return x
    return d4(x, op) if on_kernels(x) else d4_torch(x, op)


class _Dihedral(Transform):
    d4_op = D4_IDENTITY

    def transform(self, inputs):
        return _apply(inputs, self.d4_op)

    def inv_transform(self, transformed_inputs):
        return _apply(transformed_inputs, d4_inverse(self.d4_op))


class Identity(_Dihedral):
    pass


class Rotate90k(_Dihedral):
    def __init__(self, k=1):
        super(Rotate90k, self).__init__()
        assert k in [1, 2, 3]
        self.k = k
        self.d4_op = D4_ROT90[k]


class HorizontalFlip(_Dihedral):
    d4_op = D4_HFLIP


class VerticalFlip(_Dihedral):
    d4_op = D4_VFLIP


class Transpose(_Dihedral):
    d4_op = D4_TRANSPOSE


def _resize(x, size=None, scale_factor=None):
    """F.interpolate(x, size, scale_factor, mode='bilinear', align_corners=True)"""
    if not on_kernels(x) or (size is None) == (scale_factor is None):     # (neither or both: aten's own error)
        return F.interpolate(x, size=size, scale_factor=scale_factor, mode='bilinear', align_corners=True)
    h, w = x.shape[2], x.shape[3]
    if size is not None:
        ho, wo = (size, size) if isinstance(size, int) else size
    else:
        sh, sw = scale_factor if isinstance(scale_factor, (tuple, list)) else (scale_factor, scale_factor)
        ho, wo = math.floor(h * sh), math.floor(w * sw)       # floor(in * scale), as aten
    return _BilinearFn.apply(as_nhwc(x, 'Scale'), int(ho), int(wo))


class Scale(Transform):
    def __init__(self, size=None, scale_factor=None):
        super(Scale, self).__init__()
        self.size = size
        self.scale_factor = scale_factor
        self.input_shape = None

    def transform(self, inputs):
        self.input_shape = inputs.shape
        return _resize(inputs, size=self.size, scale_factor=self.scale_factor)

    def inv_transform(self, transformed_inputs):
        return _resize(transformed_inputs, size=(self.input_shape[2], self.input_shape[3]))


if __name__ == '__main__':
    import numpy as np

    for k in (1, 2, 3):
        Transform.unit_test(Rotate90k(k=k))
    for t in (HorizontalFlip(), VerticalFlip(), Transpose()):
        Transform.unit_test(t)
    for s in np.linspace(0.25, 2.0, num=8):
        Transform.unit_test(Scale(scale_factor=float(s)))
    Transform.unit_test(Scale(scale_factor=0.49))
    Transform.unit_test(Scale(size=(894, 896)))
