"""Scene-stitching family of the host wrappers (include/ever_hip.h: evk_stitch_add, evk_stitch_finalize; csrc/stitch.hip): a
batch of window score maps added into a scene accumulator and its coverage plane, and the accumulator turned into mean scores
or a class map — the `out[..] += s; count[..] += 1` per window and the `out / count` per scene of
magic/bigimage/sliding_window.py.  Part of the hip/functional.py facade; `ever_amd.magic.bigimage.scene` drives it.

The accumulator is a 3-D logical [C, H, W] tensor in one of the two dense layouts, NHWC memory (`acc.permute(1, 2, 0)` is
contiguous) or contiguous; window scores are [M, C, h, w] and are brought to the accumulator's layout if they are in the other."""
import torch

from ._base import HipPathError, _check_map, _inference_only, _stream, _timed_call, nhwc_copy
from .ptr_table import PtrTable

__all__ = ['stitch_add', 'stitch_finalize', 'stitch_stats']

_REC = 2                     # int64 words per window (csrc/stitch.hip: kStitchRecWords)
_MAX_WINDOWS = 64            # per launch (kStitchMaxWindows); evk_stitch_add chains a longer table itself
_RING = 4                    # origin tables per (windows, device), used in turn: an upload waits for the one four uploads back,
                             # not for the launch in front of it, so the host keeps running ahead of the device
_TABLES = {}                 # (windows, device) -> [next, PtrTable x _RING]
stitch_stats = {'add': 0, 'windows': 0, 'launches': 0, 'finalize': 0}      # tests / tools


def _check(t, what, dim):
    _check_map(t, what, dim, f'{dim}-D', 'trace the model, not the tiling around it', 'stitched')


def _acc_layout(acc, what):
    """True: NCHW-contiguous, False: NHWC memory.  One class is both; it is passed as NHWC."""
    if acc.permute(1, 2, 0).is_contiguous():
        return False
    if acc.is_contiguous():
        return True
    raise HipPathError(f'{what}: the accumulator must be dense ([C, H, W] contiguous, or NHWC memory), strides {acc.stride()}')


def _check_count(count, acc, what):
    _check(count, what, 2)
    if tuple(count.shape) != tuple(acc.shape[1:]) or not count.is_contiguous() or count.device != acc.device:
        raise ValueError(f'{what}: the coverage plane must be a contiguous {tuple(acc.shape[1:])} tensor on {acc.device}, got '
                         f'{tuple(count.shape)} with strides {count.stride()} on {count.device}')


def stitch_add(acc, count, scores, origins):
    """For each window m, in order: `acc[:, y0:y0+h, x0:x0+w] += scores[m]; count[y0:y0+h, x0:x0+w] += 1` with
    (y0, x0) = origins[m], bit for bit (every element is added to by one thread, in window order), in one launch per 64
    windows over the bounding box of their origins.  acc: [C, H, W] fp32 in either dense layout, count: [H, W] fp32, scores:
    [M, C, h, w] fp32.  In place; returns None.  No autograd; not traceable."""
    _check(acc, 'stitch_add', 3)
    _check(scores, 'stitch_add', 4)
    _check_count(count, acc, 'stitch_add')
    _inference_only('stitch_add', acc, count, scores)
    m, c, h, w = scores.shape
    if m == 0 or len(origins) != m or c != acc.shape[0] or scores.device != acc.device:
        raise ValueError(f'stitch_add: scores {tuple(scores.shape)} on {scores.device} with {len(origins)} origins for an '
                         f'accumulator {tuple(acc.shape)} on {acc.device}')
    nchw = _acc_layout(acc, 'stitch_add')
    if nchw:
        scores = scores if scores.is_contiguous() else scores.contiguous()
    elif not scores.permute(0, 2, 3, 1).is_contiguous():
        scores = nhwc_copy(scores)
    vals = []
    for y0, x0 in origins:
        vals += [int(y0), int(x0)]
    if torch.cuda.is_current_stream_capturing():
        raise HipPathError('stitch_add: not capturable (its origin table is validated on the host at every call)')
    ring = _TABLES.get((m, acc.device))
    if ring is None:
        ring = _TABLES[(m, acc.device)] = [0] + [PtrTable(m * _REC, acc.device) for _ in range(_RING)]
    table = ring[1 + ring[0]]
    ring[0] = (ring[0] + 1) % _RING
    tab = table.upload(vals)          # pinned, non-blocking, in stream order before the launch
    # algorithmic bytes: the scores once, the covered accumulator elements and their coverage read and written (at most
    # every window's own footprint)
    nb = 4.0 * scores.numel() * 3 + 8.0 * m * h * w
    _timed_call('resample_loss', nb, 'evk_stitch_add', table.host.data_ptr(), tab.data_ptr(), m, scores.data_ptr(),
                acc.data_ptr(), count.data_ptr(), c, acc.shape[1], acc.shape[2], h, w, 1 if nchw else 0, _stream())
    stitch_stats['add'] += 1
    stitch_stats['windows'] += m
    stitch_stats['launches'] += (m + _MAX_WINDOWS - 1) // _MAX_WINDOWS


def stitch_finalize(acc, count, mode='scores', out=None, label_dtype=torch.uint8, threshold=None, fill_label=255):
    """mode 'scores': `acc / count` (one true division per element; NaN where the coverage is 0) into `out` (a tensor of acc's
    shape and strides; None: a new one; `acc` itself: in place).  mode 'labels': a [H, W] map of `label_dtype` (uint8 or
    int64): with two classes or more the index of the first maximal quotient (`argmax(acc / count, 0)`, a NaN maximal), with
    one class `acc / count > threshold`; `fill_label` where the coverage is 0.  The normalised scores are never stored in
    labels mode.  Returns the output.  No autograd; not traceable."""
    _check(acc, 'stitch_finalize', 3)
    _check_count(count, acc, 'stitch_finalize')
    _inference_only('stitch_finalize', acc, count)
    c, h, w = acc.shape
    nchw = _acc_layout(acc, 'stitch_finalize')
    if mode == 'scores':
        if threshold is not None:
            raise ValueError('stitch_finalize: a threshold belongs to mode=\'labels\'')
        if out is None:
            out = torch.empty_like(acc)       # preserve_format: acc's dense strides
        if out.dtype != torch.float32 or out.shape != acc.shape or out.stride() != acc.stride() or out.device != acc.device:
            raise ValueError(f'stitch_finalize: out must have the accumulator\'s shape {tuple(acc.shape)}, strides '
                             f'{acc.stride()}, dtype and device; got {tuple(out.shape)} {out.stride()} {out.dtype} {out.device}')
        _timed_call('resample_loss', 8.0 * acc.numel() + 4.0 * count.numel(), 'evk_stitch_finalize', acc.data_ptr(),
                    count.data_ptr(), c, h, w, 1 if nchw else 0, 0, out.data_ptr(), 0, 0.0, 0, _stream())
    elif mode == 'labels':
        if label_dtype not in (torch.uint8, torch.int64):
            raise HipPathError(f'stitch_finalize: uint8 or int64 labels, got {label_dtype}')
        if (c == 1) != (threshold is not None):
            raise ValueError(f'stitch_finalize: {c} class(es) with threshold={threshold} (one class needs a threshold, more '
                             f'take the argmax)')
        if label_dtype == torch.uint8 and c > 256:
            raise HipPathError(f'stitch_finalize: {c} classes do not fit uint8 labels')
        if out is None:
            out = torch.empty((h, w), device=acc.device, dtype=label_dtype)
        if out.dtype != label_dtype or tuple(out.shape) != (h, w) or not out.is_contiguous() or out.device != acc.device:
            raise ValueError(f'stitch_finalize: out must be a contiguous {(h, w)} {label_dtype} tensor on {acc.device}')
        _timed_call('resample_loss', 4.0 * acc.numel() + 4.0 * count.numel() + float(out.numel() * out.element_size()),
                    'evk_stitch_finalize', acc.data_ptr(), count.data_ptr(), c, h, w, 1 if nchw else 0, 1, out.data_ptr(),
                    1 if label_dtype == torch.int64 else 0, float(threshold) if threshold is not None else 0.0,
                    int(fill_label), _stream())
    else:
        raise ValueError(f'stitch_finalize: mode must be \'scores\' or \'labels\', got {mode!r}')
    stitch_stats['finalize'] += 1
    return out
