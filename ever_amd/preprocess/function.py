"""Tensor preparation functions of the reference (preprocess/function.py): normalisation and zero padding to a size or to a
multiple.  Torch expressions on whatever device the tensor is on; the fused batch pass is hip/augment.py."""
import math

import torch
import torch.nn.functional as F

__all__ = ['th_mean_std_normalize', 'th_divisible_pad', 'th_pad_to_size']


def _bad_dim():
    return ValueError('image dim should be 3 or 4.')


def th_mean_std_normalize(image, mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375)):
    """(image - mean) / std over the channel axis of a [C, H, W] or [N, C, H, W] tensor: `image.sub(mean).div(std)`.
    A superset of the reference: mean and std are built on the image's device (the reference builds them on the CPU and so
    takes CPU images only)."""
    if image.dim() not in (3, 4):
        raise _bad_dim()
    shape = [1] * image.dim()
    shape[image.dim() - 3] = -1
    m = torch.tensor(mean, requires_grad=False, device=image.device).reshape(*shape)
    s = torch.tensor(std, requires_grad=False, device=image.device).reshape(*shape)
    return image.sub(m).div(s)


def _hw_and_tail(tensor):
    """(height, width, pad entries of the leading axes) of a [H, W], [C, H, W] or [N, C, H, W] tensor"""
    if tensor.dim() not in (2, 3, 4):
        raise _bad_dim()
    return tensor.size(-2), tensor.size(-1), [0, 0] * (tensor.dim() - 2)


def th_divisible_pad(tensor, size_divisor: int, mode='constant', value=0):
    """pad the bottom and the right of the last two axes up to the next multiple of `size_divisor`"""
    height, width, tail = _hw_and_tail(tensor)
    nheight = math.ceil(height / size_divisor) * size_divisor
    nwidth = math.ceil(width / size_divisor) * size_divisor
    return F.pad(tensor, pad=[0, nwidth - width, 0, nheight - height] + tail, mode=mode, value=value)


def th_pad_to_size(tensor, size, mode='constant', value=0):
    """pad the bottom and the right of the last two axes up to `size` = (height, width), which may not be smaller"""
    height, width, tail = _hw_and_tail(tensor)
    ph, pw = size[0] - height, size[1] - width
    assert ph >= 0 and pw >= 0
    return F.pad(tensor, pad=[0, pw, 0, ph] + tail, mode=mode, value=value)
