"""Random per-image augmentations of the reference (preprocess/thsegm.py) on [H, W, C] images and [H, W] masks, with the
reference's `np.random` calls in its order (the same seed yields the same parameters), and `THBatchAugment`, the one name the
reference does not have: the whole chain for a list of images, on the GPU as ONE kernel launch (hip/augment.py).

The per-image classes evaluate torch expressions on whatever device their tensors are on; they are the compatibility surface,
not the hot path.  `THBatchAugment(scale_range=...)` puts `THRandomScale` in front of the chain and inside the fused pass,
with its arithmetic written out (include/ever_hip.h) and held to aten's within a derived bound, not bit for bit."""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..hip._base import nhwc_copy
from . import thcomm

__all__ = ['THRandomRotate90k', 'THRandomHorizontalFlip', 'THRandomVerticalFlip', 'THRandomCrop', 'THRandomScale',
           'THBatchAugment']


def _pack(image, masks):
    """the reference's return convention: (image, mask) with a mask, the bare image without"""
    return image if masks is None else (image, masks)


def _draw_k(k):
    return int(np.random.choice([0, 1, 2, 3], 1)[0]) if k is None else k


def _draw_flip(p):
    """True = flip.  `p < uniform()` means "leave as is", as the reference writes it"""
    return not (p < np.random.uniform())


def _scale_factors(scale_range, scale_step):
    """the reference's list of factors (THRandomScale.__init__)"""
    return np.linspace(scale_range[0], scale_range[1], int((scale_range[1] - scale_range[0]) / scale_step) + 1)


def _draw_scale(factors):
    return np.random.choice(factors, size=1)[0]


def _rescale(images, masks, factor):
    """THRandomScale's expression at a given factor: (image,) or (image, mask)"""
    nchw = images.permute(2, 0, 1)[None]
    out = (F.interpolate(nchw, scale_factor=factor, mode='bilinear', align_corners=True)[0].permute(1, 2, 0),)
    if masks is not None:
        out += (F.interpolate(masks[None, None], scale_factor=factor, mode='nearest')[0][0],)
    return out


def _draw_origin(h, w, crop_size):
    """(ymin, xmin) for an image already padded up to the crop: y first, then x"""
    ymin = int(np.random.randint(0, max(h, crop_size[0]) - crop_size[0] + 1, 1)[0])
    xmin = int(np.random.randint(0, max(w, crop_size[1]) - crop_size[1] + 1, 1)[0])
    return ymin, xmin


class THRandomRotate90k(nn.Module):
    """rotate image and mask by 90 * k degrees counter-clockwise; k is drawn per call unless fixed"""

    def __init__(self, k=None):
        super().__init__()
        self.k = k

    def __call__(self, images, masks=None):
        k = _draw_k(self.k)
        if k == 0:
            return _pack(images, masks)
        return _pack(torch.rot90(images, k, [0, 1]), None if masks is None else torch.rot90(masks, k, [0, 1]))


class _RandomFlip(nn.Module):
    axis = None

    def __init__(self, p=0.5):
        super().__init__()
        self.p = p

    def __call__(self, images, masks=None):
        if not _draw_flip(self.p):
            return _pack(images, masks)
        return _pack(torch.flip(images, [self.axis]), None if masks is None else torch.flip(masks, [self.axis]))


class THRandomHorizontalFlip(_RandomFlip):
    axis = 1


class THRandomVerticalFlip(_RandomFlip):
    axis = 0


class THRandomCrop(nn.Module):
    """a random `crop_size` window; an image smaller than the crop is first padded with 0 at the bottom and the right, and so
    is its mask (without one that is an error, as in the reference).  Always returns a tuple."""

    def __init__(self, crop_size=(512, 512)):
        super().__init__()
        self.crop_size = crop_size

    def __call__(self, images, masks=None):
        c_h, c_w = self.crop_size
        pad_h, pad_w = max(c_h - images.shape[0], 0), max(c_w - images.shape[1], 0)
        if pad_h or pad_w:
            images = F.pad(images, [0, 0, 0, pad_w, 0, pad_h], mode='constant', value=0)
            masks = F.pad(masks, [0, pad_w, 0, pad_h], mode='constant', value=0)
        ymin, xmin = _draw_origin(images.shape[0], images.shape[1], self.crop_size)
        out = (images[ymin:ymin + c_h, xmin:xmin + c_w, :],)
        if masks is not None:
            out += (masks[ymin:ymin + c_h, xmin:xmin + c_w],)
        return out


class THRandomScale(nn.Module):
    """bilinear (image, align_corners) / nearest (mask) rescale by a factor drawn ONCE, at construction"""

    def __init__(self, scale_range=(0.5, 2.0), scale_step=0.25):
        super().__init__()
        self.scale_factor = _draw_scale(_scale_factors(scale_range, scale_step))

    def __call__(self, images, masks=None):
        return _rescale(images, masks, self.scale_factor)


class THBatchAugment(nn.Module):
    """[THRandomScale(scale_range, scale_step) ->] THRandomRotate90k(rotate_k) -> THRandomHorizontalFlip(hflip_p) ->
    THRandomVerticalFlip(vflip_p) -> THRandomCrop(crop_size) -> THChannelFirst2 -> THMeanStdNormalize2(mean, std) ->
    THDivisiblePad(size_divisor, mask_pad_value) for every image of a list, then `torch.stack`.

    Called with a list of [H, W, C] images (uint8 or fp32, any sizes) and an optional list of [H, W] masks (uint8 or int64).
    For each image in list order it draws k, hflip, vflip, ymin, xmin exactly as that pipeline would when run image by image.
    CUDA inputs: the draws are composed into one dihedral op and one origin per image and the batch is ONE launch of
    `HF.augment_batch`.  CPU inputs: the per-image classes above and `torch.stack` — the same function by construction.

    Returns (images, masks or None).  `channels_last=True`: a logical [N, C, Ho, Wo] tensor over NHWC memory, which the
    models take without their boundary transpose; False: the reference's NCHW-contiguous tensor; the values are identical.
    `mask_dtype`: None keeps the masks' dtype, torch.int64 gives the label maps the losses take.  `mean=None` (with
    `std=None`) only casts to fp32.  `size_divisor=None` leaves the crop size.

    `scale_range=(lo, hi)` adds the rescale step in front: bilinear with align_corners=True for the image, nearest for the
    mask, by one of the reference's factors `np.linspace(lo, hi, int((hi - lo) / scale_step) + 1)`.  `scale_each=True` draws
    the factor per image, before that image's k, hflip, vflip, ymin, xmin.  `scale_each=False` draws ONE factor when the
    object is built, as `THRandomScale` does: under one seed the object then equals the reference pipeline THRandomScale ->
    THRandomRotate90k -> ... built and then run.  The crop origin is drawn on the rescaled, rotated size.  `scale_range=None`
    consumes the random stream exactly as without the keyword.
    The rescale works on the image cast to fp32 first, on both paths: a uint8 image is NOT rounded back to uint8 after the
    interpolation (aten's CPU kernel would, given a uint8 tensor).  CUDA inputs: still ONE launch, with the arithmetic of
    include/ever_hip.h (evk_augment_scale_batch), within 8 * 2^-23 * max|image| of aten before normalisation; its labels are
    `M[min(int(a * float(1 / f)), H - 1), ...]`.  CPU inputs: aten's own `F.interpolate`, whose labels follow a shortcut of
    aten's where a rescaled side equals the source side or twice it, and which has no nearest kernel for int64: int64 masks
    need the device path or a uint8 mask (with mask_dtype=torch.int64)."""

    def __init__(self, crop_size, size_divisor=None, mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375), rotate_k=None,
                 hflip_p=0.5, vflip_p=0.5, mask_pad_value=255, channels_last=True, mask_dtype=None, scale_range=None,
                 scale_step=0.25, scale_each=True):
        super().__init__()
        if (mean is None) != (std is None):
            raise ValueError('THBatchAugment: mean and std come together or not at all')
        self.crop_size = (int(crop_size[0]), int(crop_size[1]))
        self.size_divisor = size_divisor
        self.mean, self.std = mean, std
        self.rotate_k, self.hflip_p, self.vflip_p = rotate_k, hflip_p, vflip_p
        self.mask_pad_value = mask_pad_value
        self.channels_last = channels_last
        self.mask_dtype = mask_dtype
        self.scale_factors = None if scale_range is None else _scale_factors(scale_range, scale_step)
        self.scale_each = bool(scale_each)
        self.scale_factor = None      # scale_each=False: the one factor, drawn now
        if self.scale_factors is not None and not self.scale_each:
            self.scale_factor = _draw_scale(self.scale_factors)

    def _next_scale(self):
        """the factor of the next image (a draw when scale_each), or None without a scale step"""
        if self.scale_factors is None:
            return None
        return float(_draw_scale(self.scale_factors) if self.scale_each else self.scale_factor)

    @property
    def out_size(self):
        d = self.size_divisor
        return self.crop_size if d is None else tuple(math.ceil(s / d) * d for s in self.crop_size)

    def __call__(self, images, masks=None):
        images = list(images)
        masks = None if masks is None else list(masks)
        if not images or (masks is not None and len(masks) != len(images)):
            raise ValueError(f'THBatchAugment: {len(images)} images, {None if masks is None else len(masks)} masks')
        if images[0].is_cuda:
            return self._fused(images, masks)
        return self._per_image(images, masks)

    # ---- the per-image classes: CPU inputs
    def _per_image(self, images, masks):
        random_part = (THRandomRotate90k(self.rotate_k), THRandomHorizontalFlip(self.hflip_p),
                       THRandomVerticalFlip(self.vflip_p), THRandomCrop(self.crop_size))
        outs, mouts = [], []
        for i, image in enumerate(images):
            factor = self._next_scale()
            if factor is None:
                cur = image if masks is None else (image, masks[i])
            else:
                cur = _rescale(image.float(), None if masks is None else masks[i], factor)
            for stage in random_part:
                cur = stage(*cur) if isinstance(cur, tuple) else stage(cur)
            image, mask = cur[0], (cur[1] if len(cur) > 1 else None)
            image = image.permute(2, 0, 1)           # THChannelFirst without its size(0) <= 8 guess: the input IS [H, W, C]
            image = image.float() if self.mean is None else thcomm.THMeanStdNormalize(self.mean, self.std)(image)
            if self.size_divisor is not None:
                image, mask = thcomm.THDivisiblePad(self.size_divisor, self.mask_pad_value)(image, mask)
            outs.append(image)
            mouts.append(mask)
        out = torch.stack(outs)
        if self.channels_last:
            out = nhwc_copy(out)
        if masks is None:
            return out, None
        mout = torch.stack(mouts)
        return out, (mout if self.mask_dtype is None else mout.to(self.mask_dtype))

    # ---- one launch: CUDA inputs
    def _fused(self, images, masks):
        from ..hip import functional as HF
        ops, origins, scales = [], [], []
        for image in images:
            factor = self._next_scale()
            h, w = image.shape[0], image.shape[1]
            if factor is not None:
                h, w = HF.scaled_hw(h, w, factor)
                if h < 1 or w < 1:
                    raise ValueError(f'THBatchAugment: a {image.shape[0]} x {image.shape[1]} image rescaled by {factor} is empty')
                scales.append(factor)
            k, hflip, vflip = _draw_k(self.rotate_k), _draw_flip(self.hflip_p), _draw_flip(self.vflip_p)
            op = HF.D4_ROT90.get(k, HF.D4_IDENTITY)
            if hflip:
                op = HF.d4_compose(op, HF.D4_HFLIP)
            if vflip:
                op = HF.d4_compose(op, HF.D4_VFLIP)
            ht, wt = HF.d4_out_hw(h, w, op)
            if masks is None and (ht < self.crop_size[0] or wt < self.crop_size[1]):
                raise TypeError('THBatchAugment: an image smaller than the crop needs its mask (THRandomCrop pads both)')
            ops.append(op)
            origins.append(_draw_origin(ht, wt, self.crop_size))
        return HF.augment_batch(images, masks, ops, origins, self.crop_size, self.out_size, self.mean, self.std,
                                mask_pad_value=self.mask_pad_value, channels_last=self.channels_last,
                                mask_dtype=self.mask_dtype, scales=scales or None)
