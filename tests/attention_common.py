"""The reference of the attention tests: RoPE on q and k, scaled-dot-product attention and its gradients, evaluated on the CPU
from qkv [B, N, 3, H, D] as the model lays it out.  float64 with the softmax written out is THE reference; aten's own fp32
evaluation of the same expression (the RoPE chain, the transposes, F.scaled_dot_product_attention) gives the error a correct fp32
implementation has on the same inputs, which is what the tolerance of tests/test_attention_edges_gpu.py is made of."""
import math

import torch
import torch.nn.functional as F


def rotate_half(x):
    """element d of the result is -x[d + D/2] in the first half and x[d - D/2] in the second: a roll by D/2 and a sign"""
    half = x.shape[-1] // 2
    sign = torch.ones(x.shape[-1], dtype=x.dtype, device=x.device)
    sign[:half] = -1
    return torch.roll(x, half, dims=-1) * sign


def apply_rope(t, sin, cos, prefix):
    """t [B, H, N, D]; sin / cos [N - prefix, D]: the first `prefix` tokens pass, the rest are rotated"""
    body = t[:, :, prefix:, :]
    return torch.cat((t[:, :, :prefix, :], body * cos + rotate_half(body) * sin), dim=-2)


def evaluate(qkv, sin, cos, prefix, d_o, dtype, sdpa):
    """o [B, N, H D], lse [B, H, N], dqkv [B, N, 3, H, D] in `dtype` on the CPU.  sdpa: o through aten's fused kernel."""
    qkv = qkv.detach().to(dtype).requires_grad_(True)
    b, n, _, h, d = qkv.shape
    q, k, v = [t.transpose(1, 2) for t in torch.unbind(qkv, 2)]
    if sin is not None:
        sin, cos = sin.to(dtype), cos.to(dtype)
        q, k = apply_rope(q, sin, cos, prefix), apply_rope(k, sin, cos, prefix)
    s = (q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(d))
    lse = torch.logsumexp(s, dim=-1)
    if sdpa:
        o = F.scaled_dot_product_attention(q, k, v)
    else:
        o = torch.exp(s - lse[..., None]) @ v
    o = o.transpose(1, 2).reshape(b, n, h * d)
    o.backward(d_o.to(dtype))
    return dict(o=o.detach(), lse=lse.detach(), dqkv=qkv.grad.detach())


def max_logit(qkv, sin, cos, prefix):
    """the largest scaled logit, in float64"""
    q, k, _ = [t.transpose(1, 2).double() for t in torch.unbind(qkv, 2)]
    if sin is not None:
        q, k = apply_rope(q, sin.double(), cos.double(), prefix), apply_rope(k, sin.double(), cos.double(), prefix)
    return float(((q @ k.transpose(-1, -2)) / math.sqrt(qkv.shape[-1])).max())


def trig_tables(rows, d, gen):
    """tables of the module's form: one angle per column of the first half, tiled twice — sin^2 + cos^2 = 1"""
    ang = (torch.rand(rows, d // 2, generator=gen) * 2 - 1) * (2 * math.pi)
    ang = ang.tile(2)
    return torch.sin(ang).float(), torch.cos(ang).float()


def random_tables(rows, d, gen):
    """untiled, unrelated sin and cos: only the general adjoint of the rotation differentiates these"""
    return torch.randn(rows, d, generator=gen), torch.randn(rows, d, generator=gen)
