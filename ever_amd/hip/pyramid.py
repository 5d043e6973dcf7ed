"""Pyramid-pooling family of the host wrappers (include/ever_hip.h: evk_ppm_*; csrc/ppm.hip): the K adaptive average pools of
reference ppm.py:30-33 / ops.py:89-100 from one read of the map, and the K bilinear (align_corners=False) up-samplings
with the channel concat as one write, each one autograd node whose backward is one gather-form call.  Part of the
hip/functional.py facade."""
import torch
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _C
from . import oplib
from .workspace import workspace
from ._base import (
    HipPathError, _check_4d, _ptr, _refuse_packed, _stream, _timed_call, as_nhwc, empty_nhwc, i32_array, materialize_lazy,
    ptr_array,
)

__all__ = ['pyramid_pool', 'pyramid_concat', 'pyramid_expand', 'adaptive_avg_pool2d', 'check_bins', 'pyramid_stats', 'PPM_MAX_BINS', 'PPM_MAX_BIN']

PPM_MAX_BINS, PPM_MAX_BIN = 4, 8                      # the scope of the kernels (include/ever_hip.h)
pyramid_stats = {'pool': 0, 'concat': 0, 'skip_views': 0, 'aten': 0}      # tests / tools


def _skip_stride(g, c):
    """pixel stride of `g` [N, C, H, W] if it is a channel slice of a dense NHWC map the kernels can read in place, else 0"""
    n, _, h, w = g.shape
    sn, sc, sh, sw = g.stride()
    ld = sw if w > 1 else (sh if h > 1 else (sn if n > 1 else c))      # (the stride of an axis of one element says nothing)
    if ((c == 1 or sc == 1) and ld >= c and ld % 4 == 0 and (h == 1 or sh == w * ld) and (n == 1 or sn == h * w * ld)
            and g.data_ptr() % 16 == 0):
        return ld
    return 0


class _PyramidPoolFn(Function):
    """(x, p_1 .. p_K): x itself and its K adaptive average pools from one read.  Backward: the gradient that arrives for the
    pass-through output (the concat's channel slice, read in place through its pixel stride) plus every dp_k / count, one
    write of dx."""

    @staticmethod
    def forward(ctx, bins, x):
        n, c, h, w = x.shape
        dev, st, k = x.device, _stream(), len(bins)
        ps = [empty_nhwc(n, c, b, b, dev) for b in bins]
        ba = i32_array(bins)
        ws_bytes = _C.load().evk_ppm_pool_workspace_bytes(n, h, w, c, ba, k)
        ws = workspace(dev, ws_bytes)
        # algorithmic bytes: x once, the pools once
        nb = 4.0 * (x.numel() + sum(p.numel() for p in ps))
        _timed_call('ppm', nb, 'evk_ppm_pool_fwd', x.data_ptr(), ptr_array(ps), ba, k, n, h, w, c, ws.data_ptr(), ws_bytes, st)
        ctx.bins = bins
        ctx.dims = (n, c, h, w)
        return (x, *ps)

    @staticmethod
    @once_differentiable
    def backward(ctx, dskip, *dps):
        if not ctx.needs_input_grad[1]:
            return None, None
        bins = ctx.bins
        n, c, h, w = ctx.dims
        k = len(bins)
        dev = next(g for g in (dskip, *dps) if g is not None).device
        st = _stream()
        dps = [as_nhwc(materialize_lazy(g), 'pyramid_pool.backward') if g is not None
               else torch.zeros((n, b, b, c), device=dev, dtype=torch.float32).permute(0, 3, 1, 2) for g, b in zip(dps, bins)]
        ld = 0
        if dskip is not None:
            dskip = materialize_lazy(dskip)
            ld = _skip_stride(dskip, c)
            if ld:
                pyramid_stats['skip_views'] += 1
            else:
                dskip = as_nhwc(dskip.contiguous(), 'pyramid_pool.backward')
                ld = c
        dx = empty_nhwc(n, c, h, w, dev)
        nb = 4.0 * (dx.numel() * (2 if dskip is not None else 1) + sum(g.numel() for g in dps))
        _timed_call('ppm', nb, 'evk_ppm_pool_bwd', ptr_array(dps), i32_array(bins), k, None if dskip is None else dskip.data_ptr(), ld,
                    dx.data_ptr(), n, h, w, c, st)
        return None, dx


class _PyramidConcatFn(Function):
    """cat([x] + [bilinear(z_k, (H, W), align_corners=False)]) in one write.  Backward: x's gradient is the channel slice of
    dcat, a view; the dz_k come from one call that reads dcat's pooled slices once."""

    @staticmethod
    def forward(ctx, bins, size, x, *zs):
        h, w = size
        n, cp, k = zs[0].shape[0], zs[0].shape[1], len(bins)
        c = 0 if x is None else x.shape[1]          # (no x: the up-sampled maps alone, PoolBlock on its own)
        dev, st = zs[0].device, _stream()
        cat = empty_nhwc(n, c + k * cp, h, w, dev)
        nb = 4.0 * (n * h * w * c + sum(z.numel() for z in zs) + cat.numel())
        _timed_call('ppm', nb, 'evk_ppm_expand_fwd', _ptr(x), ptr_array(zs), i32_array(bins), k, cat.data_ptr(), n, h, w, c, cp, st)
        ctx.bins = bins
        ctx.dims = (n, c, h, w, cp)
        return cat

    @staticmethod
    @once_differentiable
    def backward(ctx, dcat):
        bins = ctx.bins
        n, c, h, w, cp = ctx.dims
        k = len(bins)
        dev, st = dcat.device, _stream()
        dcat = as_nhwc(materialize_lazy(dcat), 'pyramid_concat.backward')
        dx = dcat[:, :c] if c and ctx.needs_input_grad[2] else None
        dzs = [None] * k
        if any(ctx.needs_input_grad[3:]):
            dzs = [empty_nhwc(n, cp, b, b, dev) for b in bins]
            ba = i32_array(bins)
            ws_bytes = _C.load().evk_ppm_expand_bwd_workspace_bytes(n, h, w, c, cp, ba, k)
            ws = workspace(dev, ws_bytes)
            nb = 4.0 * (n * h * w * k * cp + sum(z.numel() for z in dzs))
            _timed_call('ppm', nb, 'evk_ppm_expand_bwd', dcat.data_ptr(), ptr_array(dzs), ba, k, n, h, w, c, cp, ws.data_ptr(), ws_bytes,
                        st)
            dzs = [z if need else None for z, need in zip(dzs, ctx.needs_input_grad[3:])]
        return (None, None, dx, *dzs)


def check_bins(bins, what='pyramid_pool'):
    """the bins as a tuple of ints inside the kernels' scope, else NotImplementedError"""
    out = []
    for b in bins:
        if isinstance(b, (tuple, list)):
            if len(set(b)) != 1:
                raise NotImplementedError(f'ever_amd {what}: only square pooled sizes are implemented, got {tuple(b)}')
            b = b[0]
        out.append(int(b))
    if not 1 <= len(out) <= PPM_MAX_BINS or any(not 1 <= b <= PPM_MAX_BIN for b in out):
        raise NotImplementedError(f'ever_amd {what}: 1 to {PPM_MAX_BINS} bins of size 1 to {PPM_MAX_BIN} are implemented, '
                                  f'got {tuple(out)}')
    return tuple(out)


def _in_scope(what, n, h, w, c, cp, k):
    if c % 4 or cp % 4:
        raise HipPathError(f'{what}: {c} and {cp} channels: the pyramid kernels move 16 bytes along the channel axis, channel '
                           f'counts must be multiples of 4')
    if n * h * w * (c + k * cp) >= 2 ** 31:
        raise HipPathError(f'{what}: a concat map of {n * h * w * (c + k * cp)} elements (fewer than 2^31 are implemented)')


def pyramid_pool(x, bins):
    """`(x, *[F.adaptive_avg_pool2d(x, b) for b in bins])` (reference ppm.py:31-32 with ops.py:92) as one autograd node that
    reads x once.  The first output is x passed through: feed it to pyramid_concat, so that the gradient of the concat's own
    channel slice reaches this node's single backward call instead of an autograd sum.  While a trace is being recorded the
    aten expression is evaluated."""
    bins = check_bins(bins)
    _check_4d(x, 'pyramid_pool')
    if oplib.tracing():
        pyramid_stats['aten'] += 1
        return (x, *[F.adaptive_avg_pool2d(x, b) for b in bins])
    n, c, h, w = x.shape
    _in_scope('pyramid_pool', n, h, w, c, 0, len(bins))
    x = as_nhwc(x, 'pyramid_pool')
    _refuse_packed('pyramid_pool', 'pooled', x)
    pyramid_stats['pool'] += 1
    return _PyramidPoolFn.apply(bins, x)


def pyramid_concat(x_pass, zs, bins=None):
    """`torch.cat([x] + [F.interpolate(z, x.shape[-2:], mode='bilinear', align_corners=False) for z in zs], dim=1)`
    (reference ops.py:96-100, ppm.py:33): one write of the concat map, logical NCHW over NHWC memory; no up-sampled
    intermediate exists.  zs: the K maps [N, Cp, b_k, b_k] (bins default to their sizes)."""
    _check_4d(x_pass, 'pyramid_concat')
    zs = list(zs)
    for z in zs:
        _check_4d(z, 'pyramid_concat')
    bins = check_bins([z.shape[2] for z in zs] if bins is None else bins, 'pyramid_concat')
    n, c, h, w = x_pass.shape
    cp = zs[0].shape[1]
    for z, b in zip(zs, bins):
        if len(zs) != len(bins) or tuple(z.shape) != (n, cp, b, b):
            raise ValueError(f'pyramid_concat: a pooled map of shape {tuple(z.shape)} where {(n, cp, b, b)} is expected')
    if oplib.tracing():
        pyramid_stats['aten'] += 1
        return torch.cat([x_pass] + [F.interpolate(z, (h, w), mode='bilinear', align_corners=False) for z in zs], dim=1)
    _in_scope('pyramid_concat', n, h, w, c, cp, len(bins))
    x_pass = as_nhwc(x_pass, 'pyramid_concat')
    zs = [as_nhwc(z, 'pyramid_concat') for z in zs]
    _refuse_packed('pyramid_concat', 'resampled', x_pass, *zs)
    pyramid_stats['concat'] += 1
    return _PyramidConcatFn.apply(bins, (h, w), x_pass, *zs)


def pyramid_expand(z, size):
    """`F.interpolate(z, size, mode='bilinear', align_corners=False)` of a square map of side 1..8 (reference ops.py:100):
    the one-bin expand without a concat partner."""
    _check_4d(z, 'pyramid_expand')
    if z.shape[2] != z.shape[3]:
        raise NotImplementedError(f'ever_amd pyramid_expand: a square source map is required, got {tuple(z.shape)}')
    bins = check_bins([z.shape[2]], 'pyramid_expand')
    h, w = (int(v) for v in size)
    if oplib.tracing():
        pyramid_stats['aten'] += 1
        return F.interpolate(z, (h, w), mode='bilinear', align_corners=False)
    _in_scope('pyramid_expand', z.shape[0], h, w, 0, z.shape[1], 1)
    z = as_nhwc(z, 'pyramid_expand')
    _refuse_packed('pyramid_expand', 'resampled', z)
    return _PyramidConcatFn.apply(bins, (h, w), None, z)


def adaptive_avg_pool2d(x, size):
    """`F.adaptive_avg_pool2d(x, size)` for a square size 1..8 (reference ops.py:92): the one-bin call of the pyramid
    kernels, without a skip gradient."""
    bins = check_bins([size], 'adaptive_avg_pool2d')
    return pyramid_pool(x, bins)[1]
