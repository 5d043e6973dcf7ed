"""Depthwise convolution family of the host wrappers (reference ops.py:25-42: DepthwiseConv2d and the first convolution of
SeparableConv2d; include/ever_hip.h: evk_depthwise_*), and the broadcast of a 1x1 map with its adjoint (ops.py:89-100,
PoolBlock's interpolate).  Part of the hip/functional.py facade.

The kernels compute in exact fp32 FMA under every conv-math mode: a 3x3 depthwise convolution moves 8 bytes per 9 MACs
and has nothing to gain from the split-MFMA arithmetics, so its results are the same bits in all of them."""
import ctypes

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _C
from . import timing
from ._base import HipPathError, _is_packed, _ptr, _require_cuda, _stream, as_nhwc, empty_nhwc
from .conv import _conv_desc, _pair
from .workspace import workspace

__all__ = ['depthwise_conv2d', 'depthwise_in_scope', 'broadcast_hw']


def depthwise_in_scope(channels, out_channels, groups, kernel_size, stride, dilation=1):
    """True when a convolution is one the depthwise kernels implement: groups == in == out channels (multiplier 1),
    channels % 4 == 0, kernel 1..7 on each axis, stride 1 or 2 on each axis (any dilation, any zero padding)."""
    kh, kw = _pair(kernel_size)
    sh, sw = _pair(stride)
    dh, dw = _pair(dilation)
    return (groups == channels == out_channels and channels % 4 == 0 and 1 <= kh <= 7 and 1 <= kw <= 7
            and sh in (1, 2) and sw in (1, 2) and dh >= 1 and dw >= 1)


def _weight_ckk(weight):
    """The [C][1][kh][kw] weight as dense [C][kh][kw] memory (contiguous and channels_last are both that already)."""
    c, _, kh, kw = weight.shape
    w = weight.detach()
    if w.is_contiguous() or w.is_contiguous(memory_format=torch.channels_last):
        return w
    return w.contiguous()


class _DepthwiseFn(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, dilation, relu):
        n, c, h, w = x.shape
        kh, kw = weight.shape[2], weight.shape[3]
        d = _conv_desc(n, h, w, c, c, kh, kw, stride, padding, dilation)
        wk = _weight_ckk(weight)
        y = empty_nhwc(n, c, d.Ho, d.Wo, x.device)
        flops = 2.0 * n * d.Ho * d.Wo * c * kh * kw
        nbytes = 4.0 * (x.numel() + y.numel() + weight.numel())
        sp = timing.span('depthwise', flops, nbytes)
        _C.call('evk_depthwise_fwd', ctypes.byref(d), x.data_ptr(), wk.data_ptr(), _ptr(bias), y.data_ptr(),
                1 if relu else 0, _stream())
        if sp is not None:
            sp.stop()
        ctx.desc, ctx.relu, ctx.has_bias, ctx.flops, ctx.scope = d, relu, bias is not None, flops, timing.current_scope()
        ctx.w_stride = tuple(weight.stride())
        # x is only read by the weight gradient; y only for the ReLU mask
        ctx.save_for_backward(x if ctx.needs_input_grad[1] or ctx.needs_input_grad[2] else None, weight,
                              y if relu else None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        d = ctx.desc
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_db = ctx.has_bias and ctx.needs_input_grad[2]
        if not (need_dx or need_dw or need_db):
            return None, None, None, None, None, None, None
        dy = as_nhwc(dy, 'depthwise_conv2d.backward')
        if _is_packed(dy):
            raise HipPathError('depthwise_conv2d.backward: a packed output gradient reached the depthwise convolution')
        dev, st = dy.device, _stream()
        c, kh, kw = d.Cin, d.kh, d.kw
        dx = empty_nhwc(d.N, c, d.H, d.W, dev) if need_dx else None
        dw = None
        if need_dw:
            ws = tuple(ctx.w_stride)
            dense = ws == (kh * kw, kh * kw, kw, 1) or ws == (kh * kw, 1, kw, 1)
            dw = (torch.empty_strided(weight.shape, ws, device=dev, dtype=torch.float32) if dense
                  else torch.empty(weight.shape, device=dev, dtype=torch.float32))
        db = torch.empty((c,), device=dev, dtype=torch.float32) if need_db else None
        ws_bytes = _C.load().evk_depthwise_bwd_workspace_bytes(ctypes.byref(d)) if (need_dw or need_db) else 0
        buf = workspace(dev, ws_bytes) if ws_bytes else None
        sp = timing.span('depthwise', 2.0 * ctx.flops, 4.0 * (dy.numel() * 2 + (x.numel() if x is not None else 0)),
                         ctx.scope)
        _C.call('evk_depthwise_bwd', ctypes.byref(d), dy.data_ptr(), _ptr(x), _ptr(y), _weight_ckk(weight).data_ptr(),
                _ptr(dx), _ptr(dw), _ptr(db), _ptr(buf), ws_bytes, st)
        if sp is not None:
            sp.stop()
        return dx, dw, db, None, None, None, None


def depthwise_conv2d(x, weight, bias=None, stride=1, padding=0, dilation=1, relu=False):
    """F.conv2d(x, weight, bias, stride, padding, dilation, groups=C) for weight [C, 1, kh, kw] (+ fused ReLU) on the
    depthwise kernels (csrc/depthwise.hip).  A shape outside their scope raises HipPathError."""
    _require_cuda(x, 'depthwise_conv2d')
    x = as_nhwc(x, 'depthwise_conv2d')
    if _is_packed(x):
        raise HipPathError('depthwise_conv2d: a packed activation reached the depthwise convolution')
    c = x.shape[1]
    if weight.dim() != 4 or weight.shape[0] != c or weight.shape[1] != 1:
        raise ValueError(f'depthwise_conv2d: weight {tuple(weight.shape)} is not [{c}, 1, kh, kw]')
    if not depthwise_in_scope(c, c, c, tuple(weight.shape[2:]), stride, dilation):
        raise HipPathError(f'depthwise_conv2d: C {c}, kernel {tuple(weight.shape[2:])}, stride {_pair(stride)} outside '
                           'the kernels\' scope (C % 4 == 0, kernel <= 7, stride 1 or 2)')
    return _DepthwiseFn.apply(x, weight, bias, _pair(stride), _pair(padding), _pair(dilation), bool(relu))


class _BroadcastHWFn(Function):
    @staticmethod
    def forward(ctx, x, h, w):
        n, c = x.shape[:2]
        src = x.reshape(n, c).contiguous()
        y = empty_nhwc(n, c, h, w, x.device)
        _C.call('evk_broadcast_hw', src.data_ptr(), y.data_ptr(), n, h * w, c, _stream())
        ctx.shape = (n, c, h, w)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        n, c, h, w = ctx.shape
        g = as_nhwc(g, 'broadcast_hw.backward')
        dx = empty_nhwc(n, c, 1, 1, g.device)
        _C.call('evk_sum_hw', g.data_ptr(), dx.data_ptr(), n, h * w, c, _stream())
        return dx, None, None


def broadcast_hw(x, size):
    """F.interpolate(x, size, mode='bilinear', align_corners=False) of a 1x1 map (reference ops.py:96-100): an exact
    broadcast.  Its backward sums over the pixels in a fixed order (evk_sum_hw)."""
    _require_cuda(x, 'broadcast_hw')
    if x.dim() != 4 or x.shape[2:] != (1, 1):
        raise HipPathError(f'broadcast_hw: a [N, C, 1, 1] map is required, got {tuple(x.shape)}')
    if x.shape[1] % 4:
        raise HipPathError('broadcast_hw: channel count must be a multiple of 4')
    h, w = (int(s) for s in size)
    return _BroadcastHWFn.apply(x, h, w)
