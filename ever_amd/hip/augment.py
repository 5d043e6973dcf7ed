"""Input-preparation family of the host wrappers (include/ever_hip.h: evk_augment_batch; csrc/augment.hip): the reference's
per-image chain rotate / flip / crop / channel-first / normalise / pad (preprocess/thsegm.py, thcomm.py) and `torch.stack`
for a whole batch as ONE launch.  Part of the hip/functional.py facade; `ever_amd.preprocess.thsegm.THBatchAugment` draws the
random parameters and calls it."""
import torch

from . import oplib
from ._base import HipPathError, _stream, _timed_call, empty_nhwc
from .ptr_table import PtrTable
from .transform import d4_out_hw

__all__ = ['augment_batch', 'augment_stats']

_REC = 8                     # int64 words per sample (csrc/augment.hip: kAugRecWords)
_MASK_MODES = {(torch.uint8, torch.uint8): 1, (torch.uint8, torch.int64): 2, (torch.int64, torch.int64): 3}
_TABLES = {}                 # (samples, device) -> PtrTable
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


def augment_batch(images, masks, ops, origins, crop_size, out_size, mean, std, mask_pad_value=255, channels_last=True,
                  mask_dtype=None):
    """For each sample i: T = d4(images[i], ops[i]) on the two spatial axes of the [H, W, C] image (and of the [H, W] mask),
    the `crop_size` window at origins[i] = (y0, x0) of T zero-padded up to the crop, `(float(v) - mean) / std` per channel
    (`sub().div()`, bit for bit; only the cast when mean and std are None), zero-padded to `out_size` with the labels padded
    with `mask_pad_value`; stacked.  One launch for the list.

    images: CUDA tensors [H_i, W_i, C], all uint8 or all fp32; masks: None or CUDA tensors [H_i, W_i], all uint8 or all int64;
    mask_dtype: None (the masks' own) or torch.int64.  Returns (image, labels or None): image is logical [N, C, Ho, Wo] over
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
        ht, wt = d4_out_hw(im.shape[0], im.shape[1], op & 7)
        px = min(ht, crop_size[0]) * min(wt, crop_size[1])
        nread += px * (c * im.element_size() + (masks[i].element_size() if masks is not None else 0))
    if torch.cuda.is_current_stream_capturing():
        raise HipPathError('augment_batch: not capturable (its record table is validated on the host at every call)')
    ho, wo = int(out_size[0]), int(out_size[1])
    mean_t, std_t = _mean_std(mean, std, c, dev)
    table = _TABLES.get((n, dev))
    if table is None:
        table = _TABLES[(n, dev)] = PtrTable(n * _REC, dev)
    tab = table.upload(vals)          # pinned, non-blocking, in stream order before the launch
    out = empty_nhwc(n, c, ho, wo, dev) if channels_last else torch.empty((n, c, ho, wo), device=dev, dtype=torch.float32)
    labels = None
    if mode:
        labels = torch.empty((n, ho, wo), device=dev, dtype=torch.uint8 if mode == 1 else torch.int64)
    nwritten = out.numel() * 4 + (labels.numel() * labels.element_size() if mode else 0)
    _timed_call('resample_loss', float(nread + nwritten), 'evk_augment_batch', table.host.data_ptr(), tab.data_ptr(), n, c,
                int(crop_size[0]), int(crop_size[1]), ho, wo, None if mean_t is None else mean_t.data_ptr(),
                None if std_t is None else std_t.data_ptr(), int(mask_pad_value), 0 if channels_last else 1,
                1 if first.dtype == torch.float32 else 0, mode, out.data_ptr(), None if labels is None else labels.data_ptr(),
                _stream())
    augment_stats['calls'] += 1
    augment_stats['samples'] += n
    return out, labels
