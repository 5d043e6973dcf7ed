"""Row LayerNorm and the layer-scale residual of the host wrappers (reference ever/module/dinov3/models/convnext.py:20-28,
70-113,177,224: ConvNeXt's LayerNorm in both data formats, nn.LayerNorm on tokens, `input + drop_path(gamma * x)`;
include/ever_hip.h: evk_ln_*, evk_scale_residual_*).  Part of the hip/functional.py facade.

A logical-NCHW map is NHWC memory here: one contiguous row of C floats per pixel, which is what "channels_first" and
"channels_last" both mean to the kernels, so the reference's permutes around the LayerNorm are views that never happen.
Both kernels compute in plain fp32 under every conv-math mode."""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _C
from . import timing
from ._base import HipPathError, _is_packed, _ptr, _require_cuda, _stream, as_nhwc, materialize_lazy
from .workspace import workspace

__all__ = ['layer_norm', 'scale_residual', 'drop_path_scale', 'row_norm_in_scope']

_MAX_C = 2048


def row_norm_in_scope(channels):
    """True for a row length the LayerNorm / layer-scale kernels take: a multiple of 4 in 4..2048."""
    return channels % 4 == 0 and 4 <= channels <= _MAX_C


def _dense_like(t):
    """an uninitialised tensor of t's shape AND strides (t is dense: NHWC map or contiguous)"""
    return torch.empty_strided(t.shape, t.stride(), device=t.device, dtype=torch.float32)


def _rows_view(t, what, channel_dim):
    """`t` with dense [R][C] memory: a 4-D map normalised over dim 1 is taken to NHWC, anything else made contiguous"""
    if channel_dim == 1 and t.dim() == 4:
        return as_nhwc(t, what)
    return t if t.is_contiguous() else t.contiguous()


class _LayerNormFn(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps, channel_dim):
        c = x.shape[channel_dim]
        r = x.numel() // c
        y = _dense_like(x)
        need_grad = any(ctx.needs_input_grad[:3])
        mean = torch.empty((r,), device=x.device, dtype=torch.float32) if need_grad else None
        rstd = torch.empty((r,), device=x.device, dtype=torch.float32) if need_grad else None
        sp = timing.span('layernorm', 0.0, 8.0 * x.numel())
        _C.call('evk_ln_fwd', x.data_ptr(), _ptr(weight), _ptr(bias), eps, y.data_ptr(), _ptr(mean), _ptr(rstd), r, c, _stream())
        if sp is not None:
            sp.stop()
        ctx.shape, ctx.has_bias, ctx.channel_dim, ctx.scope = (r, c), bias is not None, channel_dim, timing.current_scope()
        if need_grad:
            ctx.save_for_backward(x, weight, mean, rstd)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, weight, mean, rstd = ctx.saved_tensors
        r, c = ctx.shape
        need_dx = ctx.needs_input_grad[0]
        need_dg = weight is not None and ctx.needs_input_grad[1]
        need_db = ctx.has_bias and ctx.needs_input_grad[2]
        if not (need_dx or need_dg or need_db):
            return None, None, None, None, None
        dy = _rows_view(materialize_lazy(dy), 'layer_norm.backward', ctx.channel_dim)
        if _is_packed(dy) or dy.stride() != x.stride():
            raise HipPathError('layer_norm.backward: the output gradient is not a dense fp32 tensor of the input\'s layout')
        dev = dy.device
        dx = _dense_like(x) if need_dx else None
        dg = torch.empty((c,), device=dev, dtype=torch.float32) if need_dg else None
        db = torch.empty((c,), device=dev, dtype=torch.float32) if need_db else None
        ws_bytes = _C.load().evk_ln_bwd_workspace_bytes(r, c) if (need_dg or need_db) else 0
        buf = workspace(dev, ws_bytes) if ws_bytes else None
        sp = timing.span('layernorm', 0.0, 12.0 * x.numel(), ctx.scope)
        _C.call('evk_ln_bwd', dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _ptr(weight), _ptr(dx), _ptr(dg),
                _ptr(db), r, c, _ptr(buf), ws_bytes, _stream())
        if sp is not None:
            sp.stop()
        return dx, dg, db, None, None


def layer_norm(x, weight=None, bias=None, eps=1e-6, channel_dim=None):
    """LayerNorm over the channels on the row kernels (csrc/layernorm.hip): biased variance, y = (x - mean) / sqrt(var + eps)
    * weight + bias — F.layer_norm(x, (C,), ...) and the reference's channels_first expression alike.
    channel_dim None: a 4-D tensor is a logical-NCHW / memory-NHWC map normalised over dim 1 (the result is such a map),
    any other tensor is normalised over its last axis.  channel_dim -1 forces the last axis of a 4-D tensor.  A channel
    count outside the kernels' scope (a multiple of 4 in 4..2048) raises HipPathError."""
    _require_cuda(x, 'layer_norm')
    if channel_dim is None:
        channel_dim = 1 if x.dim() == 4 else -1
    channel_dim = channel_dim % x.dim()
    if not (channel_dim == x.dim() - 1 or (channel_dim == 1 and x.dim() == 4)):
        raise HipPathError(f'layer_norm: channel_dim {channel_dim} of a {x.dim()}-D tensor: only dim 1 of a 4-D map or the last axis')
    if _is_packed(x):
        raise HipPathError('layer_norm: a packed activation reached the LayerNorm')
    c = x.shape[channel_dim]
    if not row_norm_in_scope(c):
        raise HipPathError(f'layer_norm: {c} channels outside the kernels\' scope (a multiple of 4 in 4..{_MAX_C})')
    if x.numel() == 0:
        raise HipPathError('layer_norm: empty tensor')
    for p, name in ((weight, 'weight'), (bias, 'bias')):
        if p is not None and (tuple(p.shape) != (c,) or not p.is_cuda or p.dtype != torch.float32):
            raise ValueError(f'layer_norm: {name} must be an fp32 CUDA tensor of shape ({c},), got {tuple(p.shape)} {p.dtype} {p.device}')
    x = _rows_view(x, 'layer_norm', channel_dim)
    return _LayerNormFn.apply(x, weight, bias, float(eps), channel_dim)


def drop_path_scale(x, drop_prob):
    """The per-sample factors of the reference's drop_path (convnext.py:20-28): floor(keep + u) / keep from ONE
    torch.rand((N, 1, 1, 1)) draw on x's device — the reference's draw, so the generator advances as the reference's
    does — as a dense [N] tensor for scale_residual."""
    keep = 1.0 - drop_prob
    u = torch.rand((x.shape[0],) + (1,) * (x.dim() - 1), dtype=x.dtype, device=x.device)
    return (keep + u).floor_().div_(keep).reshape(-1)


class _ScaleResidualFn(Function):
    @staticmethod
    def forward(ctx, a, z, gamma, scale):
        n, c = z.shape[0], z.shape[1]
        hw = z.shape[2] * z.shape[3]
        y = _dense_like(z)
        sp = timing.span('layer_scale', 0.0, 12.0 * z.numel())
        _C.call('evk_scale_residual_fwd', a.data_ptr(), z.data_ptr(), _ptr(gamma), _ptr(scale), y.data_ptr(), n, hw, c, _stream())
        if sp is not None:
            sp.stop()
        ctx.dims, ctx.scope = (n, hw, c), timing.current_scope()
        need_dg = gamma is not None and ctx.needs_input_grad[2]
        ctx.save_for_backward(z if need_dg else None, gamma, scale)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        z, gamma, scale = ctx.saved_tensors
        n, hw, c = ctx.dims
        need_da, need_dz = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_dg = gamma is not None and ctx.needs_input_grad[2]
        if not (need_da or need_dz or need_dg):
            return None, None, None, None
        dy = as_nhwc(materialize_lazy(dy), 'scale_residual.backward')
        if _is_packed(dy):
            raise HipPathError('scale_residual.backward: a packed output gradient reached the layer-scale residual')
        dev = dy.device
        dz = _dense_like(dy) if need_dz else None
        dg = torch.empty((c,), device=dev, dtype=torch.float32) if need_dg else None
        if need_dz or need_dg:
            ws_bytes = _C.load().evk_scale_residual_bwd_workspace_bytes(n, hw, c) if need_dg else 0
            buf = workspace(dev, ws_bytes) if ws_bytes else None
            sp = timing.span('layer_scale', 0.0, 4.0 * dy.numel() * (1 + int(need_dz) + int(need_dg)), ctx.scope)
            _C.call('evk_scale_residual_bwd', dy.data_ptr(), _ptr(z), _ptr(gamma), _ptr(scale), _ptr(dz), _ptr(dg), n, hw, c,
                    _ptr(buf), ws_bytes, _stream())
            if sp is not None:
                sp.stop()
        return (dy if need_da else None), dz, dg, None


def scale_residual(a, z, gamma=None, sample_scale=None):
    """a + sample_scale[n] * gamma[c] * z on maps, in one pass each way (csrc/layer_scale.hip): the tail of a ConvNeXt block,
    `input + drop_path(gamma * x)` (reference convnext.py:78-82).  gamma: the [C] layer scale or None; sample_scale: the [N]
    drop-path factors (drop_path_scale) or None in eval mode and at rate 0; it carries no gradient."""
    _require_cuda(a, 'scale_residual')
    _require_cuda(z, 'scale_residual')
    if a.dim() != 4 or a.shape != z.shape:
        raise ValueError(f'scale_residual: two maps of one shape are required, got {tuple(a.shape)} and {tuple(z.shape)}')
    a, z = as_nhwc(a, 'scale_residual'), as_nhwc(z, 'scale_residual')
    if _is_packed(a) or _is_packed(z):
        raise HipPathError('scale_residual: a packed activation reached the layer-scale residual')
    n, c = z.shape[:2]
    if not row_norm_in_scope(c):
        raise HipPathError(f'scale_residual: {c} channels outside the kernels\' scope (a multiple of 4 in 4..{_MAX_C})')
    if z.numel() == 0:
        raise HipPathError('scale_residual: empty tensor')
    if gamma is not None and (tuple(gamma.shape) != (c,) or not gamma.is_cuda or gamma.dtype != torch.float32):
        raise ValueError(f'scale_residual: gamma must be an fp32 CUDA tensor of shape ({c},), got {tuple(gamma.shape)}')
    if sample_scale is not None:
        if sample_scale.numel() != n or not sample_scale.is_cuda:
            raise ValueError(f'scale_residual: sample_scale must hold one CUDA value per sample ({n}), got {tuple(sample_scale.shape)}')
        sample_scale = sample_scale.detach().to(torch.float32).reshape(-1).contiguous()
    return _ScaleResidualFn.apply(a, z, gamma, sample_scale)
