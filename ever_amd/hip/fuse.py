"""BiFPN family of the host wrappers (include/ever_hip.h: evk_wfuse_*; csrc/wfuse.hip): the learned weighted fusion node
`sum_k w^_k x_k` of reference fpn.py:196-224 as one autograd node, a term that the reference up-samples first
(nn.UpsamplingNearest2d, fpn.py:264-269, 290) entering as an index shift.  Part of the hip/functional.py facade."""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _C
from . import oplib
from .workspace import workspace
from ._base import (
    HipPathError, _check_4d, _ptr, _refuse_packed, _stream, _timed_call, _require_cuda, as_nhwc, empty_nhwc, i32_array,
    materialize_lazy, ptr_array,
)

__all__ = ['weighted_fuse', 'upsample_nearest2x', 'wfuse_stats', 'WFUSE_EPS', 'WFUSE_NORMS']

WFUSE_EPS = 0.0001                                     # reference Fusion.eps (fpn.py:197)
WFUSE_NORMS = {'fast_normalize': 0, 'softmax': 1}      # the `norm` argument of evk_wfuse_fwd
wfuse_stats = {'nodes': 0, 'shifted_terms': 0, 'aten': 0}      # tests / tools


class _WFuseFn(Function):
    """y = ((w^0 t0 + w^1 t1) + w^2 t2) + w^3 t3, the weights normalised on the device; a shifted term is read at
    (y >> 1, x >> 1).  Backward: one pass over dy gives w^ dy (its 2 x 2 block sums for a shifted term) and, if the weights
    want a gradient, the per-term dots through the Jacobian of the normalisation.  weights None: unit weights."""

    @staticmethod
    def forward(ctx, shifts, norm, eps, weights, *terms):
        nt = len(terms)
        n, c = terms[0].shape[0], terms[0].shape[1]
        h, w = terms[0].shape[2] << shifts[0], terms[0].shape[3] << shifts[0]
        dev, st = terms[0].device, _stream()
        y = empty_nhwc(n, c, h, w, dev)
        tp, sh = ptr_array(terms), i32_array(shifts)
        # algorithmic bytes: every term once at its own size, y once
        nb = 4.0 * (sum(t.numel() for t in terms) + y.numel())
        _timed_call('wfuse', nb, 'evk_wfuse_fwd', tp, sh, nt, _ptr(weights), norm, eps, y.data_ptr(), n, h, w, c, st)
        ctx.cfg = (tuple(shifts), norm, eps)
        ctx.dims = (n, c, h, w)
        need_w = weights is not None and ctx.needs_input_grad[3]
        ctx.save_for_backward(weights, *(terms if need_w else ()))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        shifts, norm, eps = ctx.cfg
        nt = len(shifts)
        n, c, h, w = ctx.dims
        weights, terms = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        need = ctx.needs_input_grad                 # [shifts, norm, eps, weights, terms...]
        dev, st = dy.device, _stream()
        dy = as_nhwc(materialize_lazy(dy), 'weighted_fuse.backward')
        want_w = bool(need[3]) and len(terms) == nt
        dts = [empty_nhwc(n, c, h >> s, w >> s, dev) if need[4 + k] else None for k, s in enumerate(shifts)]
        if not want_w and all(d is None for d in dts):
            return (None,) * (4 + nt)
        dw = torch.empty((nt,), device=dev, dtype=torch.float32) if want_w else None
        ws, ws_bytes = None, 0
        if want_w:
            ws_bytes = _C.load().evk_wfuse_workspace_bytes(n, h, w, c, nt)
            ws = workspace(dev, ws_bytes)
        tp = ptr_array(terms) if want_w else None
        sh, dp = i32_array(shifts), ptr_array(dts)
        # algorithmic bytes: dy once, every requested gradient once, every term once if the weights want theirs
        nb = 4.0 * (dy.numel() + sum(d.numel() for d in dts if d is not None) + (sum(t.numel() for t in terms) if want_w else 0))
        _timed_call('wfuse', nb, 'evk_wfuse_bwd', dy.data_ptr(), tp, sh, nt, _ptr(weights), norm, eps, dp, _ptr(dw), _ptr(ws),
                    ws_bytes, n, h, w, c, st)
        return (None, None, None, dw, *dts)


def _aten_fuse(terms, weights, norm_method, eps):
    """the reference's expression (fpn.py:206-218, with its UpsamplingNearest2d), for a trace that is being recorded"""
    import torch.nn.functional as F
    ts = [F.interpolate(t, scale_factor=2.0, mode='nearest') if s else t for t, s in terms]
    if weights is None:
        out = ts[0]
        for t in ts[1:]:
            out = out + t
        return out
    if norm_method == 'softmax':
        wn = F.softmax(weights, dim=0)
    else:
        r = F.relu(weights)
        wn = r / (torch.sum(r, dim=0, keepdim=True) + eps)
    return torch.sum(wn.view(len(ts), 1, 1, 1, 1) * torch.stack(ts, dim=0), dim=0)


def weighted_fuse(terms, weights, norm_method='fast_normalize', eps=WFUSE_EPS):
    """`sum_k w^_k up_k(x_k)` of a BiFPN node (reference fpn.py:217-218 behind fpn.py:290, 304) as one autograd node.
    terms: one to four `(tensor, shift)`, summed in list order; a term is `[N, C, H >> shift, W >> shift]`, shift 0 or 1, and
    enters at output pixel (y, x) as its pixel (y >> shift, x >> shift) — nearest x2 as an index shift.  weights: the RAW
    `[len(terms)]` parameter on the device, normalised inside the kernel (`fast_normalize`: relu(w) / (sum relu(w) + eps);
    `softmax`), or None for unit weights.  While a trace is being recorded the reference's aten expression is evaluated."""
    if not 1 <= len(terms) <= 4:
        raise ValueError(f'weighted_fuse: 1 to 4 terms, got {len(terms)}')
    if norm_method not in WFUSE_NORMS:
        raise ValueError(f'weighted_fuse: norm_method must be one of {sorted(WFUSE_NORMS)}, got {norm_method!r}')
    ts, shifts = [], []
    for t, shift in terms:
        _check_4d(t, 'weighted_fuse')
        ts.append(t)
        shifts.append(int(shift))
    if weights is not None:
        _require_cuda(weights, 'weighted_fuse')
        if tuple(weights.shape) != (len(ts),):
            raise ValueError(f'weighted_fuse: weights of shape {tuple(weights.shape)} for {len(ts)} terms')
    n, c = ts[0].shape[0], ts[0].shape[1]
    if not 0 <= shifts[0] <= 1:
        raise ValueError(f'weighted_fuse: shift {shifts[0]} (0 and 1 are implemented)')
    h, w = ts[0].shape[2] << shifts[0], ts[0].shape[3] << shifts[0]
    for t, shift in zip(ts, shifts):
        if shift not in (0, 1) or h % (1 << shift) or w % (1 << shift) or tuple(t.shape) != (n, c, h >> shift, w >> shift):
            raise ValueError(f'weighted_fuse: a term of shape {tuple(t.shape)} with shift {shift} does not fit the output '
                             f'{(n, c, h, w)} (shift 0 or 1, H and W even for a shifted term)')
    if oplib.tracing():
        wfuse_stats['aten'] += 1
        return _aten_fuse(list(zip(ts, shifts)), weights, norm_method, eps)
    if c % 4:
        raise HipPathError(f'weighted_fuse: {c} channels: the fusion kernels move 16 bytes along the channel axis, the channel '
                           f'count must be a multiple of 4')
    ts = [as_nhwc(t, 'weighted_fuse') for t in ts]
    _refuse_packed('weighted_fuse', 'a term', *ts)
    if weights is not None and not weights.is_contiguous():
        weights = weights.contiguous()
    wfuse_stats['nodes'] += 1
    wfuse_stats['shifted_terms'] += sum(shifts)
    return _WFuseFn.apply(tuple(shifts), WFUSE_NORMS[norm_method], float(eps), weights, *ts)


def upsample_nearest2x(x):
    """`nn.UpsamplingNearest2d(scale_factor=2)(x)` (reference fpn.py:265): the one-term, unit-weight form of the fusion
    kernel; its backward is the 2 x 2 block sum."""
    return weighted_fuse([(x, 1)], None)
