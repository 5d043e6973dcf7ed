"""The HRNet exchange kernels and the bilinear slice kernels through the C-ABI, against float64 on the CPU from the same fp32
inputs.  Every output is a NaN-filled slice inside a sentinel-guarded allocation (tests/guard_common.py).

Bounds (u = 2^-24), derived, not tuned:
  forward   |y - y64| <= 6 u sum_j |t_j|: one rounding per term (the fma), three additions of partial sums that are each at
            most sum |t_j| (1 + 3u) in magnitude, and max(., 0) is 1-Lipschitz — four roundings, 6 leaves room for second order;
  bits      equal (y_gpu > 0) exactly;          dmasked   equals dy where the bit is set, bit for bit;
  dpooled_s within 4^s u sum |masked dy| of its 2^s x 2^s block (a tree of 2s additions; 2s <= 4^s);
  y_absmax  max |y| bit for bit.
An element whose float64 pre-activation lies inside the forward bound has no certain mask: it gets no upstream gradient,
and each case asserts that these are at most 0.1 % of its elements (unit-normal inputs: expected share ~1e-6).  The planted
zeros of the folded case are exact (x + (-x)) and are checked, not left out."""
import ctypes

import numpy as np
import pytest
import torch

from tests.guard_common import guarded, guards_intact

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
NAN_BITS = 0x7fc00000

# (N, H, W, C), terms as (shift, has BatchNorm), what it covers
CASES = [
    ((1, 8, 8, 4), ((0, False), (3, True)), '1x1 low map, one 16-byte chunk per pixel'),
    ((2, 6, 10, 12), ((0, False), (1, True)), 'odd low dims, C/4 odd, a ReLU-bits tail'),
    ((3, 16, 24, 36), ((0, True), (0, False), (1, True), (2, True)), 'a lower output branch, N not a power of two'),
    ((2, 32, 32, 48), ((0, False), (1, True), (2, True), (3, True)), "W48's branch-0 form"),
    ((2, 8, 8, 8), ((0, False), (1, False)), 'the folded form with planted zeros'),
    ((1, 4, 6, 4), ((0, True),), 'one term, less than one ReLU-bits chunk'),
    ((2, 8, 12, 20), ((0, True), (1, False), (2, True)), 'three terms, CW = 5: 12 blocks per pool workgroup'),
]


class Bufs:
    """device outputs of one case: NaN-filled, each inside its own sentinel-guarded allocation"""

    def __init__(self, dev):
        self.dev, self.all = dev, []

    def out(self, n, dtype=torch.float32):
        whole, inner = guarded(n, self.dev)
        self.all.append((whole, n))
        return inner.view(dtype)

    def check(self, what):
        torch.cuda.synchronize()
        for whole, n in self.all:
            assert guards_intact(whole, n), ('a store beside a buffer', what)


def _unpack_bits(words, numel):
    """bool per float: element j = i // 4 (16 bytes), float e = i % 4: word (j >> 6) * 8 + ((j >> 5) & 1) * 4 + e, bit j & 31
    (csrc/common.hpp: relu_bits_store)"""
    w = words.cpu().numpy().view(np.uint32)
    i = np.arange(numel, dtype=np.int64)
    j, e = i // 4, i % 4
    return ((w[(j >> 6) * 8 + ((j >> 5) & 1) * 4 + e] >> (j & 31).astype(np.uint32)) & 1).astype(bool)


def _up(t, s):
    """[N, h, w, C] -> nearest x 2^s"""
    return t.repeat_interleave(1 << s, dim=1).repeat_interleave(1 << s, dim=2)


def _pool(t, s):
    n, h, w, c = t.shape
    b = 1 << s
    return t.reshape(n, h // b, b, w // b, b, c).sum(dim=(2, 4))


def _inputs(shape, terms, seed, planted):
    n, h, w, c = shape
    g = torch.Generator().manual_seed(seed)
    ts, sss = [], []
    for s, has_bn in terms:
        ts.append(torch.randn((n, h >> s, w >> s, c), generator=g))
        sss.append(torch.stack([torch.rand((c,), generator=g) + 0.5, 0.2 * torch.randn((c,), generator=g)]) if has_bn else None)
    mask = torch.zeros((n, h, w, c), dtype=torch.bool)
    if planted:          # -x of the plain low-resolution term at every fine pixel of a few low pixels
        low = torch.zeros((n, h >> 1, w >> 1, 1), dtype=torch.bool)
        low[0, 0, 0] = low[0, 1, 2] = low[n - 1, (h >> 1) - 1, (w >> 1) - 1] = True
        mask = _up(low, 1).expand(n, h, w, c)
        ts[0] = torch.where(mask, -_up(ts[1], 1), ts[0])
    dy = torch.randn((n, h, w, c), generator=g)
    return ts, sss, dy, mask


@pytest.mark.parametrize('shape,terms,what', CASES, ids=[c[2] for c in CASES])
def test_hr_fuse_forward_and_backward(cuda, shape, terms, what):
    from ever_amd import _C
    lib = _C.load()
    n, h, w, c = shape
    numel = n * h * w * c
    planted = what.startswith('the folded')
    ts, sss, dy, pmask = _inputs(shape, terms, 1 + CASES.index((shape, terms, what)), planted)
    # ---- float64 reference
    t64 = []
    for t, ss, (s, _) in zip(ts, sss, terms):
        v = _up(t.double(), s)
        t64.append(v if ss is None else v * ss[0].double() + ss[1].double())
    pre = t64[0]
    for t in t64[1:]:
        pre = pre + t
    bound = 6 * U * sum(t.abs() for t in t64)
    y64 = pre.clamp_min(0)
    uncertain = (pre.abs() <= bound) & ~pmask
    assert int(uncertain.sum()) <= 1e-3 * numel, ('elements without a certain mask', int(uncertain.sum()), numel)
    if planted:
        assert int(pmask.sum()) == 3 * 4 * c and bool((pre[pmask] == 0).all())
    # ---- device
    st = torch.cuda.current_stream().cuda_stream
    bufs = Bufs(cuda)
    dts = [t.to(cuda) for t in ts]
    dss = [None if s is None else s.to(cuda).contiguous() for s in sss]
    y = bufs.out(numel)
    nbits = lib.evk_relu_bits_bytes(numel) // 4
    bits = bufs.out(nbits, torch.int32)
    amax = bufs.out(lib.evk_absmax_words(), torch.int32)
    amax.view(64, -1)[:, 0] = 0
    k = len(terms)
    rc = lib.evk_hr_fuse_fwd((ctypes.c_void_p * k)(*[t.data_ptr() for t in dts]), (ctypes.c_int32 * k)(*[s for s, _ in terms]),
                             (ctypes.c_void_p * k)(*[None if s is None else s.data_ptr() for s in dss]), k, y.data_ptr(),
                             bits.data_ptr(), amax.data_ptr(), n, h, w, c, st)
    assert rc == 0, lib.evk_last_error()
    bufs.check(what)
    yh = y.cpu().reshape(n, h, w, c)
    assert torch.isfinite(yh).all(), 'y holds an element nobody wrote'
    err = (yh.double() - y64).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f'{what:48s} forward error / bound {worst:.3f}, uncertain {int(uncertain.sum())} of {numel}')
    assert bool((err <= bound).all()), ('forward', what, worst)
    gbit = torch.from_numpy(_unpack_bits(bits, numel)).reshape(n, h, w, c)
    assert torch.equal(gbit, yh > 0), 'bits differ from (y > 0)'
    if planted:
        assert bool((yh[pmask] == 0).all()) and not bool(gbit[pmask].any())
    aw = amax.cpu().view(64, -1)
    assert int(aw[:, 0].max()) == int(yh.abs().max().reshape(1).view(torch.int32)), 'y_absmax'
    assert bool((aw[:, 1:] == NAN_BITS).all()), 'a word between the absmax slots was written'
    # ---- backward: everything any term could ask for, from one launch; twice, for run-to-run identity
    dy = torch.where(uncertain, torch.zeros_like(dy), dy)
    ddy = dy.to(cuda)
    smax = max(s for s, _ in terms)
    runs = []
    for _ in range(2):
        b2 = Bufs(cuda)
        dm = b2.out(numel)
        pools = {s: b2.out(numel >> (2 * s)) for s in range(1, smax + 1)}
        rc = lib.evk_hr_fuse_bwd(ddy.data_ptr(), bits.data_ptr(), dm.data_ptr(), *[pools[s].data_ptr() if s in pools else None
                                                                                  for s in (1, 2, 3)], n, h, w, c, st)
        assert rc == 0, lib.evk_last_error()
        b2.check(what)
        runs.append((dm.cpu(), {s: p.cpu() for s, p in pools.items()}))
    (dm, pools), (dm_b, pools_b) = runs
    assert torch.equal(dm.view(torch.int32), dm_b.view(torch.int32))
    assert all(torch.equal(pools[s].view(torch.int32), pools_b[s].view(torch.int32)) for s in pools)
    want = torch.where(gbit, dy, torch.zeros_like(dy))
    assert torch.equal(dm.reshape(n, h, w, c).view(torch.int32), want.view(torch.int32)), 'dmasked is not dy where the bit is set'
    m64 = torch.where(pre > 0, dy.double(), torch.zeros_like(pre))      # (uncertain elements carry dy = 0)
    for s, p in pools.items():
        p = p.reshape(n, h >> s, w >> s, c)
        assert torch.isfinite(p).all(), f'dpooled_{s} holds an element nobody wrote'
        pb = (4 ** s) * U * _pool(m64.abs(), s)
        perr = (p.double() - _pool(m64, s)).abs()
        print(f'{what:48s} dpooled_{s} error / bound {float((perr / pb.clamp_min(1e-300)).max()):.3f}')
        assert bool((perr <= pb).all()), ('dpooled', s, what)
    # a call that asks for the coarsest pool alone writes the same bits as the full call
    if smax >= 2:
        b3 = Bufs(cuda)
        only = b3.out(numel >> (2 * smax))
        args = [None, None, None]
        args[smax - 1] = only.data_ptr()
        assert lib.evk_hr_fuse_bwd(ddy.data_ptr(), bits.data_ptr(), None, *args, n, h, w, c, st) == 0, lib.evk_last_error()
        b3.check(what)
        assert torch.equal(only.cpu().view(torch.int32), pools[smax].view(torch.int32))


def test_hr_fuse_backward_mask_only(cuda):
    """no pool requested: the masked gradient alone (an output whose other terms are all same-resolution BatchNorm terms)"""
    from ever_amd import _C
    lib = _C.load()
    n, h, w, c = 2, 5, 7, 12
    numel = n * h * w * c
    g = torch.Generator().manual_seed(11)
    x = torch.randn((n, h, w, c), generator=g).to(cuda)
    dy = torch.randn((n, h, w, c), generator=g).to(cuda)
    st = torch.cuda.current_stream().cuda_stream
    bufs = Bufs(cuda)
    y, bits, dm = bufs.out(numel), bufs.out(lib.evk_relu_bits_bytes(numel) // 4, torch.int32), bufs.out(numel)
    assert lib.evk_hr_fuse_fwd((ctypes.c_void_p * 1)(x.data_ptr()), (ctypes.c_int32 * 1)(0), (ctypes.c_void_p * 1)(None), 1,
                               y.data_ptr(), bits.data_ptr(), None, n, h, w, c, st) == 0, lib.evk_last_error()
    assert lib.evk_hr_fuse_bwd(dy.data_ptr(), bits.data_ptr(), dm.data_ptr(), None, None, None, n, h, w, c, st) == 0
    bufs.check('mask only')
    assert torch.equal(y.reshape(n, h, w, c), x.clamp_min(0))
    want = torch.where(x > 0, dy, torch.zeros_like(dy))
    assert torch.equal(dm.reshape(n, h, w, c).view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize('hi,wi,ho,wo', [(3, 5, 12, 20), (12, 20, 12, 20)], ids=['3x5 to 12x20', 'equal size'])
def test_bilinear_slice_equals_the_dense_kernels(cuda, hi, wi, ho, wo):
    """the slice [c0, c0 + C) of a [N, Ho, Wo, Ctot] map: bit-identical to the dense kernel's result, the other channels keep
    their NaN; the backward equals the dense backward of the gathered slice"""
    from ever_amd import _C
    lib = _C.load()
    n, c, c0, ctot = 2, 8, 4, 20
    g = torch.Generator().manual_seed(5)
    x = torch.randn((n, hi, wi, c), generator=g).to(cuda)
    st = torch.cuda.current_stream().cuda_stream
    bufs = Bufs(cuda)
    dense, cat = bufs.out(n * ho * wo * c), bufs.out(n * ho * wo * ctot)
    assert lib.evk_upsample_bilinear_fwd(x.data_ptr(), dense.data_ptr(), n, hi, wi, ho, wo, c, st) == 0, lib.evk_last_error()
    assert lib.evk_upsample_bilinear_slice_fwd(x.data_ptr(), cat.data_ptr(), n, hi, wi, ho, wo, c, c0, ctot, st) == 0, \
        lib.evk_last_error()
    bufs.check('slice forward')
    catv = cat.reshape(n, ho, wo, ctot).cpu()
    densev = dense.reshape(n, ho, wo, c).cpu()
    assert torch.isfinite(densev).all()
    assert torch.equal(catv[..., c0:c0 + c].contiguous().view(torch.int32), densev.view(torch.int32))
    assert bool(torch.isnan(catv[..., :c0]).all()) and bool(torch.isnan(catv[..., c0 + c:]).all())
    if (hi, wi) == (ho, wo):
        assert torch.equal(densev, x.cpu())
    else:       # the dense kernel itself against aten on the host
        ref = torch.nn.functional.interpolate(x.cpu().permute(0, 3, 1, 2).double(), size=(ho, wo), mode='bilinear', align_corners=True)
        assert float((densev.double() - ref.permute(0, 2, 3, 1)).abs().max()) < 1e-5
    # backward
    dcat = torch.randn((n, ho, wo, ctot), generator=g).to(cuda)
    dslice = dcat[..., c0:c0 + c].contiguous()
    dx_dense, dx_slice = bufs.out(x.numel()), bufs.out(x.numel())
    assert lib.evk_upsample_bilinear_bwd(dslice.data_ptr(), dx_dense.data_ptr(), n, hi, wi, ho, wo, c, st) == 0, lib.evk_last_error()
    assert lib.evk_upsample_bilinear_slice_bwd(dcat.data_ptr(), dx_slice.data_ptr(), n, hi, wi, ho, wo, c, c0, ctot, st) == 0, \
        lib.evk_last_error()
    bufs.check('slice backward')
    assert torch.isfinite(dx_dense).all()
    assert torch.equal(dx_slice.cpu().view(torch.int32), dx_dense.cpu().view(torch.int32))


def test_bilinear_slice_wide_channels_take_the_tile_and_wave_kernels(cuda):
    """C >= 128 runs the LDS-tile forward and the wave-per-pixel backward: the same bits as the dense calls there too
    (HRNetV2-W48's 192- and 384-channel branches)"""
    from ever_amd import _C
    lib = _C.load()
    n, hi, wi, ho, wo, c, c0, ctot = 1, 4, 6, 16, 24, 192, 48, 256
    g = torch.Generator().manual_seed(6)
    x = torch.randn((n, hi, wi, c), generator=g).to(cuda)
    dcat = torch.randn((n, ho, wo, ctot), generator=g).to(cuda)
    st = torch.cuda.current_stream().cuda_stream
    bufs = Bufs(cuda)
    dense, cat = bufs.out(n * ho * wo * c), bufs.out(n * ho * wo * ctot)
    dx_dense, dx_slice = bufs.out(x.numel()), bufs.out(x.numel())
    dslice = dcat[..., c0:c0 + c].contiguous()
    assert lib.evk_upsample_bilinear_fwd(x.data_ptr(), dense.data_ptr(), n, hi, wi, ho, wo, c, st) == 0
    assert lib.evk_upsample_bilinear_slice_fwd(x.data_ptr(), cat.data_ptr(), n, hi, wi, ho, wo, c, c0, ctot, st) == 0
    assert lib.evk_upsample_bilinear_bwd(dslice.data_ptr(), dx_dense.data_ptr(), n, hi, wi, ho, wo, c, st) == 0
    assert lib.evk_upsample_bilinear_slice_bwd(dcat.data_ptr(), dx_slice.data_ptr(), n, hi, wi, ho, wo, c, c0, ctot, st) == 0
    bufs.check('wide slice')
    catv = cat.reshape(n, ho, wo, ctot).cpu()
    assert torch.isfinite(dense).all() and torch.isfinite(dx_dense).all()
    assert torch.equal(catv[..., c0:c0 + c].contiguous().view(torch.int32), dense.reshape(n, ho, wo, c).cpu().view(torch.int32))
    assert bool(torch.isnan(catv[..., :c0]).all()) and bool(torch.isnan(catv[..., c0 + c:]).all())
    assert torch.equal(dx_slice.cpu().view(torch.int32), dx_dense.cpu().view(torch.int32))
