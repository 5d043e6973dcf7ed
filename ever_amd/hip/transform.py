"""Test-time-augmentation family of the host wrappers (include/ever_hip.h: evk_d4_apply, evk_d4_merge; csrc/d4.hip): the eight
symmetries of the square as one copy kernel, and `sum(outs) / len(outs)` of the reference's tta (magic/transform/tta.py:11-23)
fused with the inverse transforms into one pass.  Part of the hip/functional.py facade.

An op is 3 bits, `swap | flip_rows << 1 | flip_cols << 2`: transpose first, then flip.  Both wrappers take a tensor in
either dense layout with no conversion: dense NHWC as it is, NCHW-contiguous as [N*C, H, W, 1] (the same memory)."""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ._base import (
    _check_map, _inference_only, _ptr, _stream, _timed_call, empty_nhwc, i32_array, is_nhwc, materialize_lazy, nhwc_copy, ptr_array,
)

__all__ = ['d4', 'd4_mean', 'd4_inverse', 'd4_compose', 'd4_out_hw', 'd4_stats', 'D4_IDENTITY', 'D4_TRANSPOSE', 'D4_VFLIP', 'D4_HFLIP',
           'D4_ROT90']

D4_IDENTITY, D4_TRANSPOSE, D4_VFLIP, D4_HFLIP = 0, 1, 2, 4       # flip(x, [2]) reverses rows, flip(x, [3]) columns
D4_ROT90 = {1: 3, 2: 6, 3: 5}                                    # torch.rot90(x, k, [2, 3])
_MAX_TERMS = 16                                                  # per launch (csrc/d4.hip: kD4MaxTerms)
d4_stats = {'apply': 0, 'mean': 0, 'mean_terms': 0, 'mean_launches': 0}     # tests / tools


def d4_inverse(op):
    """the op that undoes `op`: the two quarter turns undo each other, every other element is an involution"""
    return {3: 5, 5: 3}.get(op, op)


def d4_compose(a, b):
    """the one op that applies `a`, then `b`.  With an op written F(rows, cols) . T^swap (transpose first, then flip), moving
    b's transpose left past a's flips exchanges them (T . F(r, c) = F(c, r) . T); flips commute and cancel in pairs."""
    fr, fc = (a >> 1) & 1, (a >> 2) & 1
    if b & 1:
        fr, fc = fc, fr
    return ((a ^ b) & 1) | ((fr ^ (b >> 1) & 1) << 1) | ((fc ^ (b >> 2) & 1) << 2)


def d4_out_hw(h, w, op):
    return (w, h) if op & 1 else (h, w)


def _check(t, what):
    _check_map(t, what, 4, '4-D [N, C, H, W]', 'a traced TestTimeAugmentation holds the reference\'s aten ops', 'transformed')


def _dense(t):
    """(t in one of the two dense layouts, it is NHWC)"""
    if is_nhwc(t):
        return t, True
    return (t if t.is_contiguous() else t.contiguous()), False


def _alloc(n, c, h, w, nhwc, dev):
    return empty_nhwc(n, c, h, w, dev) if nhwc else torch.empty((n, c, h, w), device=dev, dtype=torch.float32)


def _abi_dims(n, c, nhwc):
    """(N, C) of the C-ABI call: an NCHW-contiguous map is N*C one-channel images"""
    return (n, c) if nhwc else (n * c, 1)


class _D4Fn(Function):
    @staticmethod
    def forward(ctx, x, op):
        x, nhwc = _dense(x)
        n, c, h, w = x.shape
        ho, wo = d4_out_hw(h, w, op)
        y = _alloc(n, c, ho, wo, nhwc, x.device)
        nn, cc = _abi_dims(n, c, nhwc)
        _timed_call('resample_loss', 8.0 * x.numel(), 'evk_d4_apply', x.data_ptr(), y.data_ptr(), nn, h, w, cc, op, _stream())
        ctx.op = op
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        # a permutation's adjoint is its inverse: the same kernel
        return _D4Fn.apply(materialize_lazy(dy), d4_inverse(ctx.op)), None


def d4(x, op):
    """The dihedral op `op` (0..7) on the two spatial axes of x [N, C, H, W]: torch.flip / transpose / rot90 of the reference's
    transforms (magic/transform/segm.py:16-68) as one copy, bit for bit.  The result keeps x's layout (dense NHWC, else
    NCHW-contiguous).  Backward: d4(dy, d4_inverse(op))."""
    _check(x, 'd4')
    op = int(op)
    if not 0 <= op <= 7:
        raise ValueError(f'd4: op must be 0..7, got {op}')
    d4_stats['apply'] += 1
    return _D4Fn.apply(x, op)


def d4_mean(terms, ops):
    """`sum(T_k(terms[k])) / len(terms)` with T_k = d4(., ops[k]), added in list order from 0 and divided once: bit for bit
    `sum(outs) / len(outs)` over the transformed terms (reference tta.py:19-21), in one pass over every term (a list longer
    than 16 is chained through the accumulator, which keeps the order).  No autograd: raises unless gradients are disabled or
    no term requires one.  The result is a new tensor in the first term's layout; a term in the other layout is brought to it."""
    if len(terms) == 0 or len(terms) != len(ops):
        raise ValueError(f'd4_mean: {len(terms)} terms, {len(ops)} ops')
    ops = [int(o) for o in ops]
    if any(not 0 <= o <= 7 for o in ops):
        raise ValueError(f'd4_mean: ops must be 0..7, got {ops}')
    for t in terms:
        _check(t, 'd4_mean')
    _inference_only('d4_mean', *terms)
    first, nhwc = _dense(terms[0])
    n, c = first.shape[0], first.shape[1]
    ho, wo = d4_out_hw(first.shape[2], first.shape[3], ops[0])
    ts = []
    for t, o in zip(terms, ops):
        if tuple(t.shape) != (n, c) + d4_out_hw(ho, wo, o):
            raise ValueError(f'd4_mean: a term of shape {tuple(t.shape)} under op {o} does not give {(n, c, ho, wo)}')
        if nhwc:
            t = t if is_nhwc(t) else nhwc_copy(t)
        else:
            t = t.contiguous()
        ts.append(t)
    dev, st = first.device, _stream()
    y = _alloc(n, c, ho, wo, nhwc, dev)
    nn, cc = _abi_dims(n, c, nhwc)
    d4_stats['mean'] += 1
    d4_stats['mean_terms'] += len(ts)
    with torch.no_grad():
        for i in range(0, len(ts), _MAX_TERMS):
            part, last = ts[i:i + _MAX_TERMS], i + _MAX_TERMS >= len(ts)
            tp, op = ptr_array(part), i32_array(ops[i:i + _MAX_TERMS])
            # algorithmic bytes: every term once, y once (and the accumulator when the list is chained)
            nb = 4.0 * y.numel() * (len(part) + 1 + (1 if i else 0))
            _timed_call('resample_loss', nb, 'evk_d4_merge', tp, op, len(part), _ptr(y) if i else None, y.data_ptr(), nn, ho, wo,
                        cc, len(ts) if last else 0, st)
            d4_stats['mean_launches'] += 1
    return y
