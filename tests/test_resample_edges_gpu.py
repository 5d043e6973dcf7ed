"""The resampling and pooling kernels of csrc/resample.hip and csrc/pool.hip at their dispatch edges: bilinear (four forward kernels, three
backward kernels, dense and channel-slice calls), MaxPool 3x3 s2, the x2 sub-sampling of LastLevelMaxPool, nearest x2 + add and
the global average pool.  Every kernel is called through the C ABI into NaN-filled, sentinel-guarded outputs
(tests/guard_common.py): nothing outside the result may be written, nothing inside it may stay NaN.

Bilinear cases come from tests/resample_common.py; tests/test_resample_plan_cpu.py holds each of them on the kernel it names.
Reference: F.interpolate(x.double(), size, mode='bilinear', align_corners=True) on the CPU and its autograd.  Tolerance: nothing
fixed in advance — aten's own fp32 CPU result is measured against the same fp64 reference, and the kernel may err at most twice
as much plus 4 ulp of the largest |reference| (both sides round scale * o once in float; an equal-size case has a yardstick of 0,
hence the floor; tests/yardstick_common.py).

Pools and selections are compared bit for bit with aten on the CPU (integer-valued gradients make their sums exact)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests.guard_common import guarded, guards_intact
from tests.resample_common import CASES, SLICE_CASES, case_id
from tests.yardstick_common import as_close_as_aten as _as_close_as_aten

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ helpers
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(name, *args):
    from ever_amd import _C
    _C.call(name, *args)


def _fetch(whole, inner, what):
    """the guarded result on the host, after the two checks every case makes"""
    torch.cuda.synchronize()
    assert guards_intact(whole, inner.numel()), f'{what}: wrote outside its output'
    got = inner.cpu()
    assert not bool(torch.isnan(got).any()), f'{what}: left {int(torch.isnan(got).sum())} of {got.numel()} elements unwritten'
    return got


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(got, ref, what):
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    bad = _bits(got) != _bits(ref)
    assert not bool(bad.any()), (f'{what}: {int(bad.sum())} of {bad.numel()} elements differ in their bits, first at '
                                 f'{tuple(int(v) for v in bad.nonzero()[0])}: {got[bad][0].item()!r} vs {ref[bad][0].item()!r}')


# ------------------------------------------------------------------------------------------------ bilinear
@functools.lru_cache(maxsize=None)
def _bilinear_case(n, c, hi, wi, ho, wo):
    """NHWC fp32 x and dy, and y / dx of aten in fp64 and in fp32; shared by the dense and the slice test — never written to"""
    gen = torch.Generator().manual_seed(hi * 1000 + wo * 10 + c)
    x = torch.randn(n, hi, wi, c, generator=gen)
    g = torch.randn(n, ho, wo, c, generator=gen)
    res = []
    for dt in (torch.float64, torch.float32):
        xr = x.permute(0, 3, 1, 2).contiguous().to(dt).requires_grad_()
        y = TF.interpolate(xr, size=(ho, wo), mode='bilinear', align_corners=True)
        y.backward(g.permute(0, 3, 1, 2).to(dt))
        res += [y.detach().permute(0, 2, 3, 1).contiguous(), xr.grad.permute(0, 2, 3, 1).contiguous()]
    return (x, g) + tuple(res)


def _check_bilinear(what, x, g, y, dx, y64, dx64, y32, dx32):
    _as_close_as_aten(y, y64, y32, f'{what} y')
    _as_close_as_aten(dx, dx64, dx32, f'{what} dx')
    # an input pixel that no output reads (aten agrees in both precisions) gets an exact zero, not a small number
    unread = (dx64 == 0) & (dx32 == 0)
    assert bool((dx[unread] == 0).all()), f'{what}: {int((dx[unread] != 0).sum())} unread input pixels got a gradient'
    # <y(x), g> = <x, dx(g)> up to the two fp32 roundings of the kernel's outputs: the backward's weights are the forward's
    yg, xdx = y.double() * g.double(), x.double() * dx.double()
    diff, bound = abs(yg.sum().item() - xdx.sum().item()), 2 * EPS * yg.abs().sum().item() + 2 * EPS * xdx.abs().sum().item()
    print(f'{what}: adjoint |<y,g> - <x,dx>| = {diff:.3e}, bound {bound:.3e} (used {diff / bound:.3f})')
    assert diff <= bound, f'{what}: adjoint identity off by {diff:.3e} > {bound:.3e}'


@pytest.mark.parametrize('case', [c[:6] for c in CASES], ids=case_id)
def test_bilinear_dense_matches_fp64_as_well_as_aten_fp32(cuda, case):
    """Measured on an MI355X, kernel error / aten fp32 error (both against fp64), printed per case: y 0.24 ... 1.15 (worst: 1 x 1024,
    3 x 3 -> 6 x 6, the element kernel), dx 0.32 ... 1.00 (the wave kernel and aten mostly err by the same amount to the last digit:
    the same products in the same order); the slice calls give the dense calls' figures.  No case uses more than 0.37 of its
    bound, the adjoint identity no more than 0.04 of its own."""
    n, c, hi, wi, ho, wo = case
    x, g, y64, dx64, y32, dx32 = _bilinear_case(*case)
    xd, gd = x.to(cuda), g.to(cuda)
    yw, yi = guarded(y64.numel(), cuda)
    _call('evk_upsample_bilinear_fwd', xd.data_ptr(), yi.data_ptr(), n, hi, wi, ho, wo, c, _stream())
    y = _fetch(yw, yi, 'bilinear_fwd').view(n, ho, wo, c)
    dw, di = guarded(x.numel(), cuda)
    _call('evk_upsample_bilinear_bwd', gd.data_ptr(), di.data_ptr(), n, hi, wi, ho, wo, c, _stream())
    dx = _fetch(dw, di, 'bilinear_bwd').view(n, hi, wi, c)
    _check_bilinear(case_id(case), x, g, y, dx, y64, dx64, y32, dx32)
    if (hi, wi) == (ho, wo):        # equal size: a copy, both ways
        _same_bits(y, x, 'equal-size y')
        _same_bits(dx, g, 'equal-size dx')
    if (ho, wo) == (1, 1):          # every weight sits on the first input pixel
        rest = dx.clone()
        rest[:, 0, 0] = 0
        assert bool((rest == 0).all()) and bool((dx[:, 0, 0] == g[:, 0, 0]).all())


@pytest.mark.parametrize('case,c0,ctot', [s[:3] for s in SLICE_CASES], ids=lambda v: case_id(v) if isinstance(v, tuple) else str(v))
def test_bilinear_slice_matches_fp64_and_leaves_the_other_channels(cuda, case, c0, ctot):
    n, c, hi, wi, ho, wo = case
    x, g, y64, dx64, y32, dx32 = _bilinear_case(*case)
    xd = x.to(cuda)
    yw, yi = guarded(n * ho * wo * ctot, cuda)
    _call('evk_upsample_bilinear_slice_fwd', xd.data_ptr(), yi.data_ptr(), n, hi, wi, ho, wo, c, c0, ctot, _stream())
    torch.cuda.synchronize()
    assert guards_intact(yw, yi.numel()), 'slice_fwd wrote outside the concat buffer'
    buf = yi.cpu().view(n, ho, wo, ctot)
    y = buf[..., c0:c0 + c].contiguous()
    assert not bool(torch.isnan(y).any()), 'slice_fwd left part of its slice unwritten'
    others = torch.cat([buf[..., :c0], buf[..., c0 + c:]], dim=-1)
    assert bool(torch.isnan(others).all()), 'slice_fwd touched channels outside its slice'
    # the gradient buffer holds NaN outside the slice: reading a neighbour's channel poisons dx
    gbuf = torch.full((n, ho, wo, ctot), float('nan'))
    gbuf[..., c0:c0 + c] = g
    gd = gbuf.to(cuda)
    dw, di = guarded(x.numel(), cuda)
    _call('evk_upsample_bilinear_slice_bwd', gd.data_ptr(), di.data_ptr(), n, hi, wi, ho, wo, c, c0, ctot, _stream())
    dx = _fetch(dw, di, 'bilinear_slice_bwd').view(n, hi, wi, c)
    _check_bilinear(f'slice {case_id(case)} c0={c0} Ctot={ctot}', x, g, y, dx, y64, dx64, y32, dx32)


# ------------------------------------------------------------------------------------------------ MaxPool 3x3 s2
POOL_MAPS = ((1, 1), (1, 5), (2, 2), (3, 3), (4, 6), (7, 5), (15, 9))
POOL_CHANNELS = (4, 12, 64)


def _pool_input(kind, n, h, w, c, gen):
    x = torch.randn(n, h, w, c, generator=gen)
    if kind == 'ties':
        x = torch.randint(0, 3, (n, h, w, c), generator=gen).float()
    elif kind == 'neg_inf':
        x[torch.rand(n, h, w, c, generator=gen) < 0.1] = float('-inf')
        x[0, :, :, 1] = float('-inf')       # one whole map: every window of it is all -inf
    elif kind == 'nan':
        x[torch.rand(n, h, w, c, generator=gen) < 0.05] = float('nan')
        x[1, h // 2, w // 2, 2] = float('nan')
    return x


def _code_buffer(nelem, cuda):
    whole = torch.full((nelem + 128,), 0xA5, device=cuda, dtype=torch.uint8)
    return whole, whole[64:64 + nelem]


def _maxpool_gpu(cuda, x, dy):
    n, h, w, c = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    xd, gd = x.to(cuda), dy.to(cuda)
    yw, yi = guarded(n * ho * wo * c, cuda)
    cw, ci = _code_buffer(n * ho * wo * c, cuda)
    _call('evk_maxpool3x3s2_fwd', xd.data_ptr(), yi.data_ptr(), ci.data_ptr(), n, h, w, c, _stream())
    dw, di = guarded(x.numel(), cuda)
    _call('evk_maxpool3x3s2_bwd', gd.data_ptr(), ci.data_ptr(), di.data_ptr(), n, h, w, c, _stream())
    torch.cuda.synchronize()
    assert guards_intact(yw, yi.numel()) and guards_intact(dw, di.numel()), 'maxpool wrote outside its outputs'
    assert bool((cw[:64] == 0xA5).all() and (cw[64 + ci.numel():] == 0xA5).all()), 'maxpool wrote outside its tap codes'
    assert bool((ci <= 8).all()), 'maxpool left a tap code unwritten'
    return yi.cpu().view(n, ho, wo, c), di.cpu().view(n, h, w, c)


@pytest.mark.parametrize('h,w', POOL_MAPS, ids=lambda v: str(v))
def test_maxpool_ties_infinities_and_small_maps_match_aten_bit_for_bit(cuda, h, w):
    n = 2
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    for c in POOL_CHANNELS:
        gen = torch.Generator().manual_seed(100 * h + 10 * w + c)
        dy = torch.randint(-3, 4, (n, ho, wo, c), generator=gen).float()
        for kind in ('normal', 'ties', 'neg_inf'):
            what = f'maxpool {kind} C={c} {h}x{w}'
            x = _pool_input(kind, n, h, w, c, gen)
            xr = x.permute(0, 3, 1, 2).contiguous().requires_grad_()
            yr = TF.max_pool2d(xr, 3, 2, 1)
            yr.backward(dy.permute(0, 3, 1, 2).contiguous())
            y, dx = _maxpool_gpu(cuda, x, dy)
            assert not bool(torch.isnan(y).any()) and not bool(torch.isnan(dx).any()), f'{what}: unwritten output'
            _same_bits(y, yr.detach().permute(0, 2, 3, 1).contiguous(), f'{what} y')
            _same_bits(dx, xr.grad.permute(0, 2, 3, 1).contiguous(), f'{what} dx')
        # NaN propagates: the same outputs are NaN as in aten, the rest equal it, and a NaN window's gradient goes to a NaN
        x = _pool_input('nan', n, h, w, c, gen)
        yr = TF.max_pool2d(x.permute(0, 3, 1, 2).contiguous(), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
        nan_out = torch.isnan(yr)
        assert bool(nan_out.any())
        y, dx = _maxpool_gpu(cuda, x, nan_out.float())
        what = f'maxpool nan C={c} {h}x{w}'
        assert bool((torch.isnan(y) == nan_out).all()), f'{what}: NaN at other outputs than aten'
        _same_bits(torch.where(nan_out, torch.zeros_like(y), y), torch.where(nan_out, torch.zeros_like(yr), yr), f'{what} y')
        assert not bool(torch.isnan(dx).any()), f'{what}: unwritten dx'
        assert bool(torch.isnan(x)[dx != 0].all()), f'{what}: a NaN window sent its gradient to a pixel that holds no NaN'
        assert dx.sum().item() == int(nan_out.sum()), f'{what}: {dx.sum().item()} gradients for {int(nan_out.sum())} NaN windows'


# ------------------------------------------------------------------------------------------------ sub-sampling x2
@pytest.mark.parametrize('h,w', [(1, 1), (1, 2), (2, 1), (3, 3), (4, 6), (7, 5)], ids=lambda v: str(v))
def test_subsample2_is_every_second_pixel_and_its_adjoint_writes_its_zeros(cuda, h, w):
    from ever_amd.hip import functional as HF
    n = 2
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    for c in (4, 132):
        gen = torch.Generator().manual_seed(10 * h + w + c)
        x = torch.randn(n, h, w, c, generator=gen)
        dy = torch.randn(n, ho, wo, c, generator=gen)
        y_ref = x[:, ::2, ::2].contiguous()
        dx_ref = torch.zeros(n, h, w, c)
        dx_ref[:, ::2, ::2] = dy
        xd, gd = x.to(cuda), dy.to(cuda)
        yw, yi = guarded(y_ref.numel(), cuda)
        _call('evk_subsample2_fwd', xd.data_ptr(), yi.data_ptr(), n, h, w, c, _stream())
        _same_bits(_fetch(yw, yi, 'subsample2_fwd').view(n, ho, wo, c), y_ref, f'subsample2 y C={c}')
        dw, di = guarded(x.numel(), cuda)
        _call('evk_subsample2_bwd', gd.data_ptr(), di.data_ptr(), n, h, w, c, _stream())
        _same_bits(_fetch(dw, di, 'subsample2_bwd').view(n, h, w, c), dx_ref, f'subsample2 dx C={c}')     # (+0.0 elsewhere)
        # the wrapper the FPN calls, through autograd
        xt = xd.permute(0, 3, 1, 2).requires_grad_()
        yt = HF.max_pool1x1s2(xt)
        yt.backward(gd.permute(0, 3, 1, 2))
        assert tuple(yt.shape) == (n, c, ho, wo)
        _same_bits(yt.detach().permute(0, 2, 3, 1).cpu(), y_ref, f'max_pool1x1s2 y C={c}')
        _same_bits(xt.grad.permute(0, 2, 3, 1).cpu(), dx_ref, f'max_pool1x1s2 dx C={c}')
        _same_bits(y_ref, TF.max_pool2d(x.permute(0, 3, 1, 2), 1, 2, 0).permute(0, 2, 3, 1).contiguous(), 'reference')


# ------------------------------------------------------------------------------------------------ nearest x2 + add
@pytest.mark.parametrize('n,c,h,w', [(1, 4, 2, 2), (2, 12, 2, 6), (3, 132, 6, 4)], ids=lambda v: str(v))
def test_nearest2x_add_equals_aten_and_its_adjoint_sums_four(cuda, n, c, h, w):
    """(n, c, h, w): the lateral (fine) map; the top map is h / 2 x w / 2"""
    gen = torch.Generator().manual_seed(c)
    top = torch.randn(n, h // 2, w // 2, c, generator=gen)
    lat = torch.randn(n, h, w, c, generator=gen)
    dout = torch.randn(n, h, w, c, generator=gen)
    ref = lat.permute(0, 3, 1, 2) + TF.interpolate(top.permute(0, 3, 1, 2), scale_factor=2, mode='nearest')
    td, ld, gd = top.to(cuda), lat.to(cuda), dout.to(cuda)
    ow, oi = guarded(lat.numel(), cuda)
    _call('evk_upsample_nearest2x_add_fwd', td.data_ptr(), ld.data_ptr(), oi.data_ptr(), n, h, w, c, None, _stream())
    _same_bits(_fetch(ow, oi, 'nearest2x_add').view(n, h, w, c), ref.permute(0, 2, 3, 1).contiguous(), 'nearest2x_add')
    dw, di = guarded(top.numel(), cuda)
    _call('evk_upsample_nearest2x_bwd', gd.data_ptr(), di.data_ptr(), n, h, w, c, _stream())
    dtop = _fetch(dw, di, 'nearest2x_bwd').view(n, h // 2, w // 2, c)
    terms = dout.double().view(n, h // 2, 2, w // 2, 2, c)
    err = (dtop.double() - terms.sum(dim=(2, 4))).abs()
    bound = 3 * EPS * terms.abs().sum(dim=(2, 4))      # three fp32 additions
    print(f'nearest2x_bwd: worst err / bound {(err / bound).max().item():.3f}')
    assert bool((err <= bound).all()), f'nearest2x_bwd: err / bound up to {(err / bound).max().item():.3f}'


# ------------------------------------------------------------------------------------------------ global average pool
@pytest.mark.parametrize('n,c,hw', [(1, 4, 1), (2, 4, 300), (3, 12, 7), (2, 260, 50), (2, 256, 1000), (1, 2048, 16)],
                         ids=lambda v: str(v))
def test_gap_at_idle_threads_ragged_blocks_and_short_maps(cuda, n, c, hw):
    """tpc = min(C / 4, 64) threads per pixel row and rl = 256 / tpc rows in flight: C = 12 leaves a thread idle (3 x 85),
    C = 260 a ragged second workgroup, HW < rl most row lanes empty.  Inputs have mean 0.5: cancellation hides nothing."""
    gen = torch.Generator().manual_seed(c + hw)
    x = torch.randn(n, hw, c, generator=gen) + 0.5
    dy = torch.randn(n, c, generator=gen)
    xd, gd = x.to(cuda), dy.to(cuda)
    yw, yi = guarded(n * c, cuda)
    _call('evk_gap_fwd', xd.data_ptr(), yi.data_ptr(), n, hw, c, _stream())
    y = _fetch(yw, yi, 'gap_fwd').view(n, c)
    ref = x.double().mean(dim=1)
    err = (y.double() - ref).abs()
    bound = hw * EPS * x.double().abs().mean(dim=1) + torch.from_numpy(np.spacing(ref.abs().float().numpy())).double()
    print(f'gap_fwd ({n}, {c}, {hw}): worst err / bound {(err / bound).max().item():.3f}')
    assert bool((err <= bound).all()), f'gap_fwd: err / bound up to {(err / bound).max().item():.3f}'
    dw, di = guarded(x.numel(), cuda)
    _call('evk_gap_bwd', gd.data_ptr(), di.data_ptr(), n, hw, c, _stream())
    dx = _fetch(dw, di, 'gap_bwd').view(n, hw, c)
    inv = torch.tensor(1.0 / hw, dtype=torch.float32)
    _same_bits(dx, (dy * inv)[:, None, :].expand(n, hw, c).contiguous(), 'gap_bwd')
