"""Input-preparation family of the host wrappers (include/ever_hip.h: evk_augment_batch, evk_augment_scale_batch;
csrc/augment.hip): the reference's per-image chain [scale /] rotate / flip / crop / channel-first / normalise / pad
(preprocess/thsegm.py, thcomm.py) and `torch.stack` for a whole batch as ONE launch.  Part of the hip/functional.py facade;
`ever_amd.preprocess.thsegm.THBatchAugment` draws the random parameters and calls it."""
import math
import struct

import torch

from . import oplib
from ._base import HipPathError, _stream, _timed_call, empty_nhwc
from .ptr_table import PtrTable
from .transform import d4_out_hw

__all__ = ['augment_batch', 'augment_stats', 'scaled_hw']

_REC = 8                     # int64 words per sample (csrc/augment.hip: kAugRecWords)
_REC_SCALE = 12              # with a scale step (kAugScaleRecWords)
_MASK_MODES = {(torch.uint8, torch.uint8): 1, (torch.uint8, torch.int64): 2, (torch.int64, torch.int64): 3}
_TABLES = {}                 # (words, device) -> PtrTable
_CONSTS = {}                 # (mean, std, device) -> (mean tensor, std tensor)
augment_stats = {'calls': 0, 'samples': 0}      # tests / tools


def _mean_std(mean, std, c, dev):
    if mean is None and std is None:
        return None, None
    if mean is None or std is None:
        raise ValueError('augment_batch: mean and std come together or not at all')
    key = (tuple(float(v) for v in mean), tuple(float(v) for v in std), dev)
    if len(key[0]) != c or len(key[1]) != c:
        raise ValueError(f'augment_batch: {len(key[0])} means and {len(key[1])} stds for {c} channels')
    hit = _CONSTS.get(key)
    if hit is None:
        # as the reference's torch.tensor(mean): fp32 values
        hit = _CONSTS[key] = (torch.tensor(key[0], dtype=torch.float32, device=dev), torch.tensor(key[1], dtype=torch.float32, device=dev))
    return hit


def scaled_hw(h, w, factor):
    """(Hz, Wz) of an [h, w] map rescaled by `factor`: aten's output sizes, floor of the double product"""
    return int(math.floor(float(h) * factor)), int(math.floor(float(w) * factor))


def _f32_bits(v):
    """bit image of float(v) rounded to fp32"""
    return struct.unpack('<I', struct.pack('<f', v))[0]


def augment_batch(images, masks, ops, origins, crop_size, out_size, mean, std, mask_pad_value=255, channels_last=True,
                  mask_dtype=None, scales=None):
    """For each sample i: T = d4(images[i], ops[i]) on the two spatial axes of the [H, W, C] image (and of the [H, W] mask),
    the `crop_size` window at origins[i] = (y0, x0) of T zero-padded up to the crop, `(float(v) - mean) / std` per channel
    (`sub().div()`, bit for bit; only the cast when mean and std are None), zero-padded to `out_size` with the labels padded
    with `mask_pad_value`; stacked.  One launch for the list.

    images: CUDA tensors [H_i, W_i, C], all uint8 or all fp32; masks: None or CUDA tensors [H_i, W_i], all uint8 or all int64;
    mask_dtype: None (the masks' own) or torch.int64.

    scales: None, or one positive float per image.  None, or all exactly 1.0, is the call above, record for record.  Otherwise
    image i is first rescaled by scales[i] as the reference's THRandomScale does it, to [floor(H_i * f), floor(W_i * f)]:
    bilinear with align_corners=True for the image, nearest for the mask, inside the same single launch
    (evk_augment_scale_batch), and ops / origins refer to the rescaled image.  The arithmetic is the one written out in
    include/ever_hip.h (numpy: tests/augment_scale_common.py).  A uint8 image is interpolated in fp32 and NOT rounded back
    to uint8, as aten's CPU kernel would for a uint8 tensor: the result is the chain applied to the image cast to fp32 first,
    within 8 * 2^-23 * max|source| of aten's before normalisation (aten adds the same terms in another order).  The labels
    equal aten's CPU nearest wherever a scaled side is neither the source side nor twice it (there aten takes a shortcut of
    its own); int64 masks, for which aten has no nearest kernel, are scaled all the same.

    Returns (image, labels or None): image is logical [N, C, Ho, Wo] over
    dense NHWC memory (channels_last) or NCHW-contiguous, labels [N, Ho, Wo].  No autograd; not traceable."""
    if oplib.tracing():
        raise HipPathError('augment_batch: not traceable (trace the model, not its input path)')
    n = len(images)
    if n == 0 or len(ops) != n or len(origins) != n or (masks is not None and len(masks) != n):
        raise ValueError(f'augment_batch: {n} images, {len(ops)} ops, {len(origins)} origins'
                         + ('' if masks is None else f', {len(masks)} masks'))
    first = images[0]
    dev, c = first.device, first.shape[-1] if first.dim() == 3 else -1
    if first.dtype not in (torch.uint8, torch.float32):
        raise HipPathError(f'augment_batch: uint8 or fp32 sources required, got {first.dtype}')
    mode = 0
    if masks is not None:
        mode = _MASK_MODES.get((masks[0].dtype, mask_dtype or masks[0].dtype))
        if mode is None:
            raise HipPathError(f'augment_batch: masks {masks[0].dtype} -> {mask_dtype} (uint8 -> uint8, uint8 -> int64 and '
                               f'int64 -> int64 are implemented)')
    if scales is not None:
        if len(scales) != n:
            raise ValueError(f'augment_batch: {n} images, {len(scales)} scales')
        scales = [float(f) for f in scales]
        if not all(f > 0.0 and math.isfinite(f) for f in scales):
            raise ValueError(f'augment_batch: scales must be positive and finite, got {scales}')
        if all(f == 1.0 for f in scales):
            scales = None
    keep, vals = [], []
    nread = 0
    for i, im in enumerate(images):
        if not im.is_cuda or im.device != dev:
            raise HipPathError(f'augment_batch: image {i} is on {im.device}; there is no CPU path here (THBatchAugment has one)')
        if im.dim() != 3 or im.shape[2] != c or im.dtype != first.dtype:
            raise ValueError(f'augment_batch: image {i} is {tuple(im.shape)} {im.dtype}, expected [H, W, {c}] {first.dtype}')
        im = im if im.is_contiguous() else im.contiguous()
        keep.append(im)
        mptr = 0
        if masks is not None:
            m = masks[i]
            if m.device != dev or m.dtype != masks[0].dtype or tuple(m.shape) != tuple(im.shape[:2]):
                raise ValueError(f'augment_batch: mask {i} is {tuple(m.shape)} {m.dtype} on {m.device} for image {tuple(im.shape)}')
            m = m if m.is_contiguous() else m.contiguous()
            keep.append(m)
            mptr = m.data_ptr()
        op, (y0, x0) = int(ops[i]), origins[i]
        vals += [im.data_ptr(), mptr, im.shape[0], im.shape[1], op, int(y0), int(x0), 0]
        hz, wz, taps = im.shape[0], im.shape[1], 1
        if scales is not None:
            hz, wz = scaled_hw(hz, wz, scales[i])
            vals += [hz, wz, _f32_bits(1.0 / scales[i]), 0]
            taps = 1 if scales[i] == 1.0 else 4
        ht, wt = d4_out_hw(hz, wz, op & 7)
        px = max(min(ht, crop_size[0]), 0) * max(min(wt, crop_size[1]), 0) * taps
        nread += px * c * im.element_size() + (px // taps) * (masks[i].element_size() if masks is not None else 0)
    if torch.cuda.is_current_stream_capturing():
        raise HipPathError('augment_batch: not capturable (its record table is validated on the host at every call)')
    ho, wo = int(out_size[0]), int(out_size[1])
    mean_t, std_t = _mean_std(mean, std, c, dev)
    words = n * (_REC if scales is None else _REC_SCALE)
    table = _TABLES.get((words, dev))
    if table is None:
        table = _TABLES[(words, dev)] = PtrTable(words, dev)
    tab = table.upload(vals)          # pinned, non-blocking, in stream order before the launch
    out = empty_nhwc(n, c, ho, wo, dev) if channels_last else torch.empty((n, c, ho, wo), device=dev, dtype=torch.float32)
    labels = None
    if mode:
        labels = torch.empty((n, ho, wo), device=dev, dtype=torch.uint8 if mode == 1 else torch.int64)
    nwritten = out.numel() * 4 + (labels.numel() * labels.element_size() if mode else 0)
    entry = 'evk_augment_batch' if scales is None else 'evk_augment_scale_batch'
    _timed_call('resample_loss', float(nread + nwritten), entry, table.host.data_ptr(), tab.data_ptr(), n, c,
                int(crop_size[0]), int(crop_size[1]), ho, wo, None if mean_t is None else mean_t.data_ptr(),
                None if std_t is None else std_t.data_ptr(), int(mask_pad_value), 0 if channels_last else 1,
                1 if first.dtype == torch.float32 else 0, mode, out.data_ptr(), None if labels is None else labels.data_ptr(),
                _stream())
    augment_stats['calls'] += 1
    augment_stats['samples'] += n
    return out, labels
