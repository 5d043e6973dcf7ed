"""Self-attention with RoPE and the token prefix of a ViT of the host wrappers (reference ever/module/dinov3/layers/
attention.py:16-27,66-85,106-118: rope_apply, apply_rope, compute_attention; models/vision_transformer.py:201-231:
prepare_tokens_with_masks; include/ever_hip.h: evk_attn_*, evk_tokens_prepend_*).  Part of the hip/functional.py facade.

The kernels read the QKV Linear's output [B, N, 3 C] as it lies and write [B, N, C] as the projection Linear takes it: the
reference's reshape / unbind / transposes never happen.  Plain fp32 (the exact fp32 MFMA) under every conv-math mode."""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _C
from . import timing
from ._base import HipPathError, _is_packed, _ptr, _require_cuda, _stream, materialize_lazy
from .workspace import workspace

__all__ = ['attention', 'prepend_tokens', 'attention_in_scope']

_HEAD_DIMS = (32, 64)


def attention_in_scope(head_dim):
    """True for a head dimension the attention kernels take (32 or 64: every ViT up to vit_giant2 has 64)."""
    return head_dim in _HEAD_DIMS


def _dense(t):
    t = materialize_lazy(t)
    return t if t.is_contiguous() else t.contiguous()


class _AttentionFn(Function):
    @staticmethod
    def forward(ctx, qkv, sin, cos, num_heads, prefix):
        b, n, c3 = qkv.shape
        c = c3 // 3
        d = c // num_heads
        dev = qkv.device
        o = torch.empty((b, n, c), device=dev, dtype=torch.float32)
        need_grad = ctx.needs_input_grad[0]
        lse = torch.empty((b, num_heads, n), device=dev, dtype=torch.float32) if need_grad else None
        sp = timing.span('attention', 4.0 * b * num_heads * n * n * d, 4.0 * (qkv.numel() + o.numel()))
        _C.call('evk_attn_fwd', qkv.data_ptr(), _ptr(sin), _ptr(cos), o.data_ptr(), _ptr(lse), b, n, num_heads, d, prefix, _stream())
        if sp is not None:
            sp.stop()
        ctx.dims, ctx.scope = (b, n, num_heads, d, prefix), timing.current_scope()
        if need_grad:
            ctx.save_for_backward(qkv, sin, cos, o, lse)
        return o

    @staticmethod
    @once_differentiable
    def backward(ctx, d_o):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        qkv, sin, cos, o, lse = ctx.saved_tensors
        b, n, h, d, prefix = ctx.dims
        d_o = _dense(d_o)
        if _is_packed(d_o) or d_o.dtype != torch.float32 or d_o.shape != o.shape:
            raise HipPathError('attention.backward: the output gradient is not a dense fp32 tensor of the output\'s shape')
        dqkv = torch.empty_like(qkv)
        ws_bytes = _C.load().evk_attn_bwd_workspace_bytes(b, n, h, d)
        buf = workspace(qkv.device, ws_bytes)
        sp = timing.span('attention', 14.0 * b * h * n * n * d, 4.0 * (2 * qkv.numel() + 2 * o.numel()), ctx.scope)
        _C.call('evk_attn_bwd', qkv.data_ptr(), _ptr(sin), _ptr(cos), o.data_ptr(), d_o.data_ptr(), lse.data_ptr(), dqkv.data_ptr(),
                b, n, h, d, prefix, _ptr(buf), ws_bytes, _stream())
        if sp is not None:
            sp.stop()
        return dqkv, None, None, None, None


def attention(qkv, num_heads, rope=None):
    """softmax(rope(q) rope(k)^T / sqrt(D)) v over all tokens, per head, in one kernel each way (csrc/attention.hip).
    qkv: [B, N, 3 C], the QKV Linear's output (q, k, v thirds, each H heads of D = C / H); rope: None or (sin, cos), fp32
    [hw, D] tables for the LAST hw tokens (the N - hw tokens in front of them — class and storage tokens — are not rotated);
    returns [B, N, C].  The tables carry no gradient.  A head dimension other than 32 or 64, or a rope of another dtype or with
    a batch or head dimension, raises HipPathError."""
    _require_cuda(qkv, 'attention')
    if _is_packed(qkv):
        raise HipPathError('attention: a packed activation reached the attention')
    if qkv.dim() != 3 or qkv.dtype != torch.float32:
        raise HipPathError(f'attention: qkv must be an fp32 [B, N, 3 C] tensor, got {tuple(qkv.shape)} {qkv.dtype}')
    b, n, c3 = qkv.shape
    if num_heads < 1 or c3 % (3 * num_heads) != 0:
        raise ValueError(f'attention: {c3} columns are not 3 x {num_heads} heads')
    d = c3 // (3 * num_heads)
    if not attention_in_scope(d):
        raise HipPathError(f'attention: head dimension {d} outside the kernels\' scope {_HEAD_DIMS}')
    if b < 1 or n < 1:
        raise HipPathError('attention: empty tensor')
    sin = cos = None
    prefix = n
    if rope is not None:
        sin, cos = rope
        for t, name in ((sin, 'sin'), (cos, 'cos')):
            if not t.is_cuda or t.dtype != torch.float32:
                raise HipPathError(f'attention: rope {name} must be an fp32 CUDA tensor, got {t.dtype} on {t.device} (bf16 tables are out of scope)')
            if t.dim() != 2 or t.shape[1] != d or t.shape != sin.shape:
                raise HipPathError(f'attention: rope {name} must be [hw, {d}] without batch or head dimensions, got {tuple(t.shape)}')
        if sin.shape[0] > n:
            raise HipPathError(f'attention: rope tables of {sin.shape[0]} rows for {n} tokens')
        prefix = n - sin.shape[0]
        sin, cos = sin.detach().contiguous(), cos.detach().contiguous()
    return _AttentionFn.apply(_dense(qkv), sin, cos, int(num_heads), int(prefix))


class _PrependFn(Function):
    @staticmethod
    def forward(ctx, patches, prefix):
        b, hw, c = patches.shape
        p = prefix.shape[0]
        out = torch.empty((b, p + hw, c), device=patches.device, dtype=torch.float32)
        sp = timing.span('attention', 0.0, 8.0 * out.numel())
        _C.call('evk_tokens_prepend_fwd', patches.data_ptr(), prefix.data_ptr(), out.data_ptr(), b, hw, p, c, _stream())
        if sp is not None:
            sp.stop()
        ctx.dims, ctx.scope = (b, hw, p, c), timing.current_scope()
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        b, hw, p, c = ctx.dims
        need_dx, need_dp = ctx.needs_input_grad
        if not (need_dx or need_dp):
            return None, None
        dout = _dense(dout)
        if _is_packed(dout) or dout.dtype != torch.float32:
            raise HipPathError('prepend_tokens.backward: the output gradient is not a dense fp32 tensor')
        dev = dout.device
        dx = torch.empty((b, hw, c), device=dev, dtype=torch.float32) if need_dx else None
        dp = torch.empty((p, c), device=dev, dtype=torch.float32) if need_dp else None
        sp = timing.span('attention', 0.0, 8.0 * dout.numel(), ctx.scope)
        _C.call('evk_tokens_prepend_bwd', dout.data_ptr(), _ptr(dx), _ptr(dp), b, hw, p, c, _stream())
        if sp is not None:
            sp.stop()
        return dx, dp


def prepend_tokens(patches, prefix):
    """cat([prefix.expand(B), patches], dim=1) in one copy (csrc/tokens.hip): patches [B, HW, C], prefix [P, C] (class and
    storage tokens) -> [B, P + HW, C].  The prefix gradient is summed over the batch in order, without atomics."""
    _require_cuda(patches, 'prepend_tokens')
    _require_cuda(prefix, 'prepend_tokens')
    if _is_packed(patches):
        raise HipPathError('prepend_tokens: a packed activation reached the token prefix')
    if patches.dim() != 3 or prefix.dim() != 2 or prefix.shape[1] != patches.shape[2]:
        raise ValueError(f'prepend_tokens: [B, HW, C] patches and a [P, C] prefix are required, got {tuple(patches.shape)} and {tuple(prefix.shape)}')
    if patches.dtype != torch.float32 or prefix.dtype != torch.float32:
        raise HipPathError('prepend_tokens: fp32 only')
    if prefix.shape[0] < 1 or patches.shape[2] % 4 != 0 or patches.numel() == 0:
        raise HipPathError(f'prepend_tokens: {prefix.shape[0]} prefix tokens of {patches.shape[2]} channels on {tuple(patches.shape)}: '
                           'at least one token and one patch, channels a multiple of 4')
    return _PrependFn.apply(_dense(patches), _dense(prefix))
