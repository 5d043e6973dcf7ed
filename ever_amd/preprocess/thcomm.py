"""Per-image tensor transforms of the reference (preprocess/thcomm.py) with its names, defaults and return conventions: a
`Pipeline` that splats tuples from stage to stage, layout, normalisation and padding stages.  The `...2` classes carry a
second value (the mask) through untouched."""
import torch.nn as nn

from ..core.to import to_tensor
from . import function as pF

__all__ = ['Pipeline', 'FuncWrapper', 'ToTensor', 'THChannelFirst', 'THChannelFirst2', 'THMeanStdNormalize',
           'THMeanStdNormalize2', 'THDivisiblePad']


class Pipeline(nn.Sequential):
    """stages in order; a stage that returns a tuple feeds it to the next as positional arguments"""

    def __call__(self, *inputs):
        for stage in self._modules.values():
            inputs = stage(*inputs) if isinstance(inputs, tuple) else stage(inputs)
        return inputs


class FuncWrapper(nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def __call__(self, *input):
        return self.fn(*input)


class ToTensor(nn.Module):
    def __call__(self, *input):
        return to_tensor(input)


class THChannelFirst(nn.Module):
    """[H, W, C] -> [C, H, W]; a tensor whose first axis has at most 8 entries is taken to be channel-first already"""

    @staticmethod
    def _is_channel_first(tensor):
        return tensor.size(0) <= 8

    def __call__(self, image):
        return image if THChannelFirst._is_channel_first(image) else image.permute(2, 0, 1)


class THChannelFirst2(THChannelFirst):
    def __call__(self, image, other):
        return THChannelFirst.__call__(self, image), other


class THMeanStdNormalize(nn.Module):
    def __init__(self, mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375)):
        super().__init__()
        self._m = mean
        self._s = std

    def __call__(self, image):
        return pF.th_mean_std_normalize(image.float(), self._m, self._s)


class THMeanStdNormalize2(THMeanStdNormalize):
    def __call__(self, image, other):
        return THMeanStdNormalize.__call__(self, image), other


class THDivisiblePad(nn.Module):
    """pad image (with 0) and mask (with `mask_pad_value`) to a multiple of `size_divisor`; with `pad_to_size` the result is
    the ORIGINAL image padded to that size (as the reference), the mask the divisibly padded one padded on"""

    def __init__(self, size_divisor, mask_pad_value=255, pad_to_size=None):
        super().__init__()
        self.size_divisor = size_divisor
        self.mask_pad_value = mask_pad_value
        self.pad_to_size = pad_to_size

    def __call__(self, image, mask=None):
        pimage = pF.th_divisible_pad(image, self.size_divisor)
        if self.pad_to_size is not None:
            pimage = pF.th_pad_to_size(image, self.pad_to_size)
        pmask = mask
        if mask is not None:
            pmask = pF.th_divisible_pad(mask, self.size_divisor, value=self.mask_pad_value)
            if self.pad_to_size:
                pmask = pF.th_pad_to_size(pmask, self.pad_to_size, value=self.mask_pad_value)
        return pimage, pmask
