"""The four pyramid-pooling launches (include/ever_hip.h: evk_ppm_*) through the C ABI over the case table of
tests/ppm_common.py: maps 1x1 to 33x20 (b > H among them), C 4 to 260, every kind of bin list, a second channel chunk in
both chunked passes.  Outputs and workspaces are NaN-filled slices of exactly the stated sizes inside sentinel-guarded
allocations (tests/guard_common.py); every call is made twice and must give the same bits.  The bounds are those of the
numpy statement: exact where the arithmetic is exact (integer sums, copies, a bin of 1, the quotient sums of the pool
backward), rounding bounds in terms of the operands elsewhere."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ever_amd import _C
from tests import ppm_common as pc
from tests.guard_common import guarded, guards_intact

pytestmark = pytest.mark.gpu
U24 = pc.U24


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(cuda)


def _bins(bins):
    return (ctypes.c_int32 * len(bins))(*bins)


def _tab(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _twice(run):
    """run() -> list of arrays; called twice on fresh allocations: the same bits"""
    a, b = run(), run()
    for u, v in zip(a, b):
        assert np.array_equal(_bits(u), _bits(v)), 'two runs differ'
    return a


def _collect(pairs, shapes, extra=()):
    """after the launch: guards intact, every element written; the outputs as host arrays"""
    torch.cuda.synchronize()
    outs = []
    for (whole, inner), shape in zip(pairs, shapes):
        assert guards_intact(whole, inner.numel()), 'a store outside an output'
        assert not torch.isnan(inner).any(), 'an output element nobody wrote'
        outs.append(inner.cpu().numpy().reshape(shape))
    for whole, inner in extra:
        assert guards_intact(whole, inner.numel()), 'a store outside the workspace'
    return outs


def _pool_fwd(x, bins, cuda):
    n, h, w, c = x.shape
    lib, k = _C.load(), len(bins)
    xd = _dev(x, cuda)

    def run():
        ws_bytes = lib.evk_ppm_pool_workspace_bytes(n, h, w, c, _bins(bins), k)
        assert ws_bytes > 0 and ws_bytes % 16 == 0
        ws = guarded(ws_bytes // 4, cuda)
        outs = [guarded(n * b * b * c, cuda) for b in bins]
        _C.call('evk_ppm_pool_fwd', xd.data_ptr(), _tab([o[1] for o in outs]), _bins(bins), k, n, h, w, c, ws[1].data_ptr(),
                ws_bytes, _stream())
        res = _collect(outs, [(n, b, b, c) for b in bins], [ws])
        assert not torch.isnan(ws[1]).any()          # the cells partition the map: every cell sum is written
        return res
    return _twice(run)


@pytest.mark.parametrize('case', pc.CASES, ids=pc.case_id)
def test_pool_forward(case, cuda):
    h, w, c, _, bins = case
    rng = np.random.default_rng(hash(case) % 2 ** 32)
    xi = rng.integers(-15, 16, size=(pc.N, h, w, c)).astype(np.float32)
    for got, b in zip(_pool_fwd(xi, bins, cuda), bins):      # integer sums are exact in any order: one division is left
        s, _, cnt = pc.pool_fwd64(xi, b)
        ref = s.astype(np.float32) / cnt.astype(np.float32)[None, :, :, None]
        assert np.array_equal(_bits(got), _bits(ref)), b
    xn = rng.standard_normal((pc.N, h, w, c)).astype(np.float32)
    for got, b in zip(_pool_fwd(xn, bins, cuda), bins):
        s, a, cnt = pc.pool_fwd64(xn, b)
        cnt = cnt[None, :, :, None]
        ref = s / cnt
        bound = (cnt - 1) * U24 * a / cnt + U24 * np.abs(ref)
        err = np.abs(got.astype(np.float64) - ref)
        print(f'bin {b}: worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}')
        assert (err <= bound).all(), b


def _expand_fwd(x, zs, bins, cuda):
    n, h, w, c = x.shape
    cp, k = zs[0].shape[3], len(bins)
    xd, zd = _dev(x, cuda), [_dev(z, cuda) for z in zs]

    def run():
        cat = guarded(n * h * w * (c + k * cp), cuda)
        _C.call('evk_ppm_expand_fwd', xd.data_ptr(), _tab(zd), _bins(bins), k, cat[1].data_ptr(), n, h, w, c, cp, _stream())
        return _collect([cat], [(n, h, w, c + k * cp)])
    return _twice(run)[0]


@pytest.mark.parametrize('case', pc.CASES, ids=pc.case_id)
def test_expand_forward(case, cuda):
    h, w, c, cp, bins = case
    rng = np.random.default_rng(hash(case) % 2 ** 32 + 1)
    x = rng.standard_normal((pc.N, h, w, c)).astype(np.float32)
    zs = [rng.standard_normal((pc.N, b, b, cp)).astype(np.float32) for b in bins]
    cat = _expand_fwd(x, zs, bins, cuda)
    assert np.array_equal(_bits(cat[..., :c]), _bits(x))
    for k, (z, b) in enumerate(zip(zs, bins)):
        got = cat[..., c + k * cp:c + (k + 1) * cp]
        if b == 1:
            assert np.array_equal(_bits(got), _bits(np.broadcast_to(z, got.shape))), 'a bin of 1 is a broadcast'
        bound = 8 * 2.0 ** -23 * np.abs(z).max()
        ref64 = pc.expand_fwd(z, h, w, np.float64)
        err = np.abs(got.astype(np.float64) - ref64).max()
        zt = torch.from_numpy(z).permute(0, 3, 1, 2)
        at32 = F.interpolate(zt, (h, w), mode='bilinear', align_corners=False).permute(0, 2, 3, 1).numpy()
        at64 = F.interpolate(zt.double(), (h, w), mode='bilinear', align_corners=False).permute(0, 2, 3, 1).numpy()
        e_aten = np.abs(at32 - at64).max()
        err_aten = np.abs(got.astype(np.float64) - at64).max()
        print(f'bin {b}: error / bound {err / bound:.3f}, against aten {err_aten / max(3 * e_aten, bound):.3f}')
        assert err <= bound, b
        assert err_aten <= max(3 * e_aten, bound), b
        # the header states the blend operation by operation: the fp32 statement gives the same bits
        assert np.array_equal(_bits(got), _bits(pc.expand_fwd(z, h, w, np.float32))), b


def _expand_bwd(dcat, c, cp, bins, cuda):
    n, h, w, _ = dcat.shape
    lib, k = _C.load(), len(bins)
    dd = _dev(dcat, cuda)

    def run():
        ws_bytes = lib.evk_ppm_expand_bwd_workspace_bytes(n, h, w, c, cp, _bins(bins), k)
        assert ws_bytes > 0 and ws_bytes % 16 == 0
        ws = guarded(ws_bytes // 4, cuda)
        outs = [guarded(n * b * b * cp, cuda) for b in bins]
        _C.call('evk_ppm_expand_bwd', dd.data_ptr(), _tab([o[1] for o in outs]), _bins(bins), k, n, h, w, c, cp,
                ws[1].data_ptr(), ws_bytes, _stream())
        res = _collect(outs, [(n, b, b, cp) for b in bins], [ws])
        assert not torch.isnan(ws[1]).any()
        return res
    return _twice(run)


@pytest.mark.parametrize('case', pc.CASES, ids=pc.case_id)
def test_expand_backward(case, cuda):
    h, w, c, cp, bins = case
    rng = np.random.default_rng(hash(case) % 2 ** 32 + 2)
    dcat = rng.standard_normal((pc.N, h, w, c + len(bins) * cp)).astype(np.float32)
    for k, (got, b) in enumerate(zip(_expand_bwd(dcat, c, cp, bins, cuda), bins)):
        dz, mag, support = pc.expand_bwd64(dcat[..., c + k * cp:c + (k + 1) * cp], b)
        bound = (support[None, :, :, None] + 4) * U24 * mag
        err = np.abs(got.astype(np.float64) - dz)
        print(f'bin {b}: worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}')
        assert (err <= bound).all(), b
    if 1 in bins:       # unit weights: integer gradients sum exactly
        di = rng.integers(-15, 16, size=dcat.shape).astype(np.float32)
        for k, (got, b) in enumerate(zip(_expand_bwd(di, c, cp, bins, cuda), bins)):
            if b == 1:
                ref = di[..., c + k * cp:c + (k + 1) * cp].astype(np.float64).sum(axis=(1, 2)).astype(np.float32)
                assert np.array_equal(_bits(got.reshape(ref.shape)), _bits(ref))


def _pool_bwd(dps, bins, h, w, skip, ld, cuda):
    """skip: None, or the [N,h,w,ld] array whose channels [4, 4 + C) (ld > C) or [0, C) (ld == C) are the skip gradient"""
    n, c = dps[0].shape[0], dps[0].shape[3]
    k = len(bins)
    dd = [_dev(d, cuda) for d in dps]
    sd = None if skip is None else _dev(skip, cuda)
    sp = None if sd is None else sd.data_ptr() + (16 if ld > c else 0)

    def run():
        dx = guarded(n * h * w * c, cuda)
        _C.call('evk_ppm_pool_bwd', _tab(dd), _bins(bins), k, sp, ld, dx[1].data_ptr(), n, h, w, c, _stream())
        return _collect([dx], [(n, h, w, c)])
    return _twice(run)[0]


@pytest.mark.parametrize('case', pc.CASES, ids=pc.case_id)
def test_pool_backward(case, cuda):
    h, w, c, _, bins = case
    rng = np.random.default_rng(hash(case) % 2 ** 32 + 3)
    dps = [rng.standard_normal((pc.N, b, b, c)).astype(np.float32) for b in bins]
    got = _pool_bwd(dps, bins, h, w, None, 0, cuda)
    assert np.array_equal(_bits(got), _bits(pc.pool_bwd32(dps, bins, h, w, None))), 'without a skip gradient'
    for ld in (c, c + 8):
        skip = rng.standard_normal((pc.N, h, w, ld)).astype(np.float32)
        own = skip[..., 4:4 + c] if ld > c else skip
        got = _pool_bwd(dps, bins, h, w, skip, ld, cuda)
        assert np.array_equal(_bits(got), _bits(pc.pool_bwd32(dps, bins, h, w, own))), f'skip gradient with ld = {ld}'
