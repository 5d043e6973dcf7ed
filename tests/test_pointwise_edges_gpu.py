"""The layout kernels (NCHW <-> NHWC with channel padding, pad / unpad of the channel axis) and the element-wise kernel of
csrc/pointwise.hip, called directly through the C ABI into NaN-filled, sentinel-guarded outputs (tests/guard_common.py).
Layouts are selections: bit-exact against permute / slicing plus zero padding.  The element-wise kernel runs 16-byte chunks
and a scalar tail (n % 4 != 0); relu, relu_bwd, add, scale and mul_scale are bit-exact against torch on the CPU, gelu and its
gradient are held to the fp64 erf formula as closely as aten's fp32 (at most twice its error plus 2 ulp of the largest value)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests.guard_common import guarded, guards_intact

pytestmark = pytest.mark.gpu

INF = float('inf')


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(name, *args):
    from ever_amd import _C
    _C.call(name, *args)


def _fetch(whole, inner, what, nan_ok=False):
    torch.cuda.synchronize()
    assert guards_intact(whole, inner.numel()), f'{what}: wrote outside its output'
    got = inner.cpu()
    assert nan_ok or not bool(torch.isnan(got).any()), f'{what}: left {int(torch.isnan(got).sum())} of {got.numel()} elements unwritten'
    return got


def _same_bits(got, ref, what):
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    bad = got.contiguous().view(torch.int32) != ref.contiguous().view(torch.int32)
    assert not bool(bad.any()), (f'{what}: {int(bad.sum())} of {bad.numel()} elements differ in their bits, first at '
                                 f'{tuple(int(v) for v in bad.nonzero()[0])}: {got[bad][0].item()!r} vs {ref[bad][0].item()!r}')


# ------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize('n,c,h,w,cp', [(1, 1, 1, 1, 1), (2, 3, 5, 7, 4), (2, 3, 5, 7, 8), (1, 5, 300, 1, 5), (3, 4, 2, 129, 4)],
                         ids=lambda v: str(v))
def test_nchw_nhwc_transposes_pad_with_zeros_and_round_trip(cuda, n, c, h, w, cp):
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(c * h + w))
    want = torch.zeros(n, h, w, cp)
    want[..., :c] = x.permute(0, 2, 3, 1)
    xd = x.to(cuda)
    ow, oi = guarded(want.numel(), cuda)
    _call('evk_nchw_to_nhwc', xd.data_ptr(), oi.data_ptr(), n, c, h, w, cp, _stream())
    nhwc = _fetch(ow, oi, 'nchw_to_nhwc').view(n, h, w, cp)
    _same_bits(nhwc, want, 'nchw_to_nhwc')                    # (the padding: +0.0)
    bw, bi = guarded(x.numel(), cuda)
    _call('evk_nhwc_to_nchw', oi.data_ptr(), bi.data_ptr(), n, c, h, w, cp, _stream())
    _same_bits(_fetch(bw, bi, 'nhwc_to_nchw').view(n, c, h, w), x, 'round trip')
    # the way back reads C of the Cp channels only: NaN in the padding must not arrive
    src = want.clone()
    src[..., c:] = float('nan')
    sd = src.to(cuda)
    bw, bi = guarded(x.numel(), cuda)
    _call('evk_nhwc_to_nchw', sd.data_ptr(), bi.data_ptr(), n, c, h, w, cp, _stream())
    _same_bits(_fetch(bw, bi, 'nhwc_to_nchw (NaN padding)').view(n, c, h, w), x, 'nhwc_to_nchw')


@pytest.mark.parametrize('rows', [1, 257])
@pytest.mark.parametrize('c,cp', [(3, 4), (1, 8), (4, 4), (72, 72)], ids=lambda v: str(v))
def test_pad_and_unpad_channels(cuda, rows, c, cp):
    x = torch.randn(rows, c, generator=torch.Generator().manual_seed(rows + c))
    want = torch.zeros(rows, cp)
    want[:, :c] = x
    xd = x.to(cuda)
    ow, oi = guarded(rows * cp, cuda)
    _call('evk_pad_channels', xd.data_ptr(), oi.data_ptr(), rows, c, cp, _stream())
    _same_bits(_fetch(ow, oi, 'pad_channels').view(rows, cp), want, 'pad_channels')
    src = want.clone()
    src[:, c:] = float('nan')
    sd = src.to(cuda)
    bw, bi = guarded(rows * c, cuda)
    _call('evk_unpad_channels', sd.data_ptr(), bi.data_ptr(), rows, cp, c, _stream())
    _same_bits(_fetch(bw, bi, 'unpad_channels').view(rows, c), x, 'unpad_channels')


# ------------------------------------------------------------------------------------------------ element-wise
SIZES = (1, 2, 3, 4, 5, 7, 1024, 1027)
SPECIALS = (0.0, -0.0, INF, -INF)


def _operand(n, seed, shift):
    """normals with +-0.0 and +-inf cycled through them (from element `shift` on: two operands meet in every pairing), the last
    element — the scalar tail's, where there is one — always a special"""
    t = torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 2
    for k, i in enumerate(range(shift % 3, n, 3)):
        t[i] = SPECIALS[(k + shift) % 4]
    t[n - 1] = SPECIALS[(n + shift) % 4]
    return t


def _same_bits_or_both_nan(got, ref, what):
    """(inf - inf and 0 * inf are NaN on both sides; a NaN's sign and payload are not part of the contract)"""
    both = torch.isnan(got) & torch.isnan(ref)
    _same_bits(torch.where(both, torch.zeros_like(got), got), torch.where(both, torch.zeros_like(ref), ref), what)


@pytest.mark.parametrize('n', SIZES)
def test_elementwise_chunks_and_tail_are_bit_exact(cuda, n):
    a, b = _operand(n, n, 0), _operand(n, n + 1, 1)
    ad, bd = a.to(cuda), b.to(cuda)
    alpha = torch.tensor(0.3, dtype=torch.float32)
    y = torch.relu(_operand(n, n + 2, 2))       # a ReLU output, as relu_bwd's second operand: +-0.0, +inf, positives
    yd = y.to(cuda)
    runs = (
        ('relu_fwd', lambda o: _call('evk_relu_fwd', ad.data_ptr(), o, n, _stream()), torch.relu(a)),
        ('relu_bwd', lambda o: _call('evk_relu_bwd', ad.data_ptr(), yd.data_ptr(), o, n, _stream()),
         torch.ops.aten.threshold_backward(a, y, 0)),
        ('add', lambda o: _call('evk_add', ad.data_ptr(), bd.data_ptr(), o, n, _stream()), a + b),
        ('scale', lambda o: _call('evk_scale', ad.data_ptr(), alpha.item(), o, n, _stream()), a * alpha),
        ('mul_scale', lambda o: _call('evk_mul_scale', ad.data_ptr(), bd.data_ptr(), alpha.item(), o, n, _stream()),
         (a * b) * alpha),
    )
    for name, run, ref in runs:
        ow, oi = guarded(n, cuda)
        run(oi.data_ptr())
        got = _fetch(ow, oi, name, nan_ok=True)
        assert bool((torch.isnan(got) == torch.isnan(ref)).all()), f'{name} n={n}: NaN (or an unwritten element) where torch has none'
        _same_bits_or_both_nan(got, ref, f'{name} n={n}')


def _gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def _gelu_grad64(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def _as_close_as_aten(got, ref64, ref32, scale, what):
    """On the finite values of the fp64 formula: max |got - ref| <= 2 max |aten fp32 - ref| + 2 ulp(scale), `scale` the largest
    finite magnitude in play, operands included: the formula's 1 + erf rounds at ulp(1) whatever the size of the result, so
    the result's own ulp is no measure of one element's error, and the sizes below go down to one element.  Elsewhere
    (gelu(-inf) = -inf * 0 and the like): the same infinity, or a NaN, as the formula gives."""
    fin = torch.isfinite(ref64)
    g_nf, r_nf = got[~fin].double(), ref64[~fin]
    assert bool((torch.isnan(g_nf) == torch.isnan(r_nf)).all()), f'{what}: NaN where the formula has none, or the reverse'
    assert bool((g_nf[~torch.isnan(r_nf)] == r_nf[~torch.isnan(r_nf)]).all()), f'{what}: another infinity than the formula'
    assert not bool(torch.isnan(got[fin]).any()), f'{what}: NaN (or an unwritten element) where the formula is finite'
    if not bool(fin.any()):
        return
    yard = (ref32[fin].double() - ref64[fin]).abs().max().item()
    err = (got[fin].double() - ref64[fin]).abs().max().item()
    floor = 2 * float(np.spacing(np.float32(scale)))
    print(f'{what}: kernel err {err:.3e}, aten fp32 err {yard:.3e}, ratio {err / yard if yard else float("nan"):.3f}, '
          f'bound {2 * yard + floor:.3e} (used {err / (2 * yard + floor):.3f})')
    assert err <= 2 * yard + floor, f'{what}: err {err:.3e} > 2 * {yard:.3e} + {floor:.3e}'


def _largest_finite(*tensors):
    return max((t[torch.isfinite(t)].abs().max().item() for t in tensors if bool(torch.isfinite(t).any())), default=0.0)


@pytest.mark.parametrize('n', SIZES)
def test_gelu_chunks_and_tail_match_the_fp64_erf_formula(cuda, n):
    """Measured on an MI355X, kernel error / aten fp32 error (both against the fp64 formula), printed per size: gelu 0.34 ... 1.00,
    its gradient 0.50 ... 2.14 (n = 5, three ordinary values: 5.7e-8 against 2.7e-8); no size uses more than 0.24 of its bound."""
    x, dy = _operand(n, 7 * n, 0), torch.randn(n, generator=torch.Generator().manual_seed(n))
    xd, gd = x.to(cuda), dy.to(cuda)
    x32 = x.clone().requires_grad_()
    y32 = TF.gelu(x32)
    y32.backward(dy)
    ow, oi = guarded(n, cuda)
    _call('evk_gelu_fwd', xd.data_ptr(), oi.data_ptr(), n, _stream())
    ref = _gelu64(x.double())
    _as_close_as_aten(_fetch(ow, oi, 'gelu_fwd', nan_ok=True), ref, y32.detach(), _largest_finite(x, ref), f'gelu_fwd n={n}')
    ow, oi = guarded(n, cuda)
    _call('evk_gelu_bwd', gd.data_ptr(), xd.data_ptr(), oi.data_ptr(), n, _stream())
    ref = dy.double() * _gelu_grad64(x.double())
    _as_close_as_aten(_fetch(ow, oi, 'gelu_bwd', nan_ok=True), ref, x32.grad, _largest_finite(x, dy, ref), f'gelu_bwd n={n}')
