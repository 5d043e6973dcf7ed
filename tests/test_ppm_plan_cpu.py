"""The host side of the pyramid-pooling kernels (include/ever_hip.h: evk_ppm_*), without a GPU: evk_ppm_plan and the
workspace queries over the case table of tests/ppm_common.py, every refusal (each returns before any launch, so none needs
a device), and the numpy statement of the four functions against aten's CPU adaptive_avg_pool2d and bilinear
align_corners=False interpolation."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ever_amd import _C
from tests import ppm_common as pc

FAKE = 0x10000          # an address on the 16-byte grid that nothing dereferences: every call below is refused first


def _bins(bins):
    return (ctypes.c_int32 * max(len(bins), 1))(*bins)


def _tab(k, addr=FAKE):
    return (ctypes.c_void_p * max(k, 1))(*([addr] * max(k, 1)))


def _plan(n, h, w, c, cp, bins):
    out = (ctypes.c_int32 * 16)()
    rc = _C.load().evk_ppm_plan(n, h, w, c, cp, _bins(bins), len(bins), out)
    return rc, list(out)


@pytest.mark.parametrize('case', pc.CASES, ids=pc.case_id)
def test_plan_and_workspaces_over_the_table(case):
    h, w, c, cp, bins = case
    lib = _C.load()
    rc, out = _plan(pc.N, h, w, c, cp, bins)
    assert rc == 0
    assert out == pc.expected_plan(pc.N, h, w, c, cp, bins)
    assert out[2] <= min(h, 63) and out[3] <= min(w, 63)
    assert lib.evk_ppm_pool_workspace_bytes(pc.N, h, w, c, _bins(bins), len(bins)) == out[12]
    assert lib.evk_ppm_expand_bwd_workspace_bytes(pc.N, h, w, c, cp, _bins(bins), len(bins)) == out[13]


def test_the_table_reaches_a_second_chunk_in_both_chunked_passes():
    plans = [_plan(pc.N, *case[:4], case[4])[1] for case in pc.CASES]
    assert {p[5] for p in plans} >= {1, 2} and {p[9] for p in plans} >= {1, 2}
    # the flagship case: ten cells per axis for bins (1, 2, 3, 6) on 64 rows, eight channel chunks of 2048 channels
    rc, out = _plan(16, 64, 64, 2048, 512, (1, 2, 3, 6))
    assert rc == 0 and out[2:6] == [10, 10, 16 * 10 * 8, 8] and out[14:] == [12, 50]
    # the most cells an axis can have: four bins whose window edges never coincide
    rc, out = _plan(1, 840, 840, 4, 4, (8, 7, 5, 3))
    assert rc == 0 and out[2] == len(pc.cells(840, (8, 7, 5, 3))) - 1 <= 63


ALL = ('pool_fwd', 'pool_bwd', 'expand_fwd', 'expand_bwd')
POOL, EXPAND = ALL[:2], ALL[2:]


def _calls(which, n, h, w, c, cp, bins, x=FAKE, tab=None, out=FAKE, ws=FAKE, ws_bytes=1 << 40, dskip=None, ld=0):
    """the launches named in `which` on fake addresses: {name: return code}.  Only calls that the arguments make a launcher
    refuse may be named: nothing here may reach a launch."""
    lib, k = _C.load(), len(bins)
    tab = _tab(k) if tab is None else tab
    b = _bins(bins)
    fns = {
        'pool_fwd': lambda: lib.evk_ppm_pool_fwd(x, tab, b, k, n, h, w, c, ws, ws_bytes, None),
        'pool_bwd': lambda: lib.evk_ppm_pool_bwd(tab, b, k, dskip, ld, out, n, h, w, c, None),
        'expand_fwd': lambda: lib.evk_ppm_expand_fwd(x, tab, b, k, out, n, h, w, c, cp, None),
        'expand_bwd': lambda: lib.evk_ppm_expand_bwd(x, tab, b, k, n, h, w, c, cp, ws, ws_bytes, None),
    }
    return {name: fns[name]() for name in which}


def _all(rcs, code):
    return all(rc == code for rc in rcs.values())


@pytest.mark.parametrize('bins, code, text', [
    ((), -2, b'0 bins'), ((1, 2, 3, 6, 8), -2, b'5 bins'), ((2, 0), -2, b'bin 1 is 0'), ((9,), -2, b'bin 0 is 9'),
])
def test_bins_outside_the_scope_are_refused_everywhere(bins, code, text):
    lib = _C.load()
    rc, _ = _plan(2, 12, 12, 8, 4, bins)
    assert rc == code and text in lib.evk_last_error()
    assert _all(_calls(ALL, 2, 12, 12, 8, 4, bins), code)
    assert lib.evk_ppm_pool_workspace_bytes(2, 12, 12, 8, _bins(bins), len(bins)) == 0
    assert lib.evk_ppm_expand_bwd_workspace_bytes(2, 12, 12, 8, 4, _bins(bins), len(bins)) == 0


def test_channel_counts_sizes_and_the_index_limit_are_refused():
    lib = _C.load()
    for c, cp in ((6, 4), (8, 6), (2, 4)):
        assert _plan(2, 12, 12, c, cp, (1, 2))[0] == -2 and b'multiples of 4' in lib.evk_last_error()
        assert _all(_calls(EXPAND if c % 4 == 0 else ALL, 2, 12, 12, c, cp, (1, 2)), -2)      # (the pools never see Cp)
    for n, h, w in ((0, 12, 12), (2, 0, 12), (2, 12, -1)):
        assert _plan(n, h, w, 8, 4, (2,))[0] == -1
        assert _all(_calls(ALL, n, h, w, 8, 4, (2,)), -1)
    # N H W (C + K Cp) = 2^31 exactly is refused, the flagship case a quarter of it is not
    assert _plan(16, 128, 256, 2048, 512, (1, 2, 3, 6))[0] == -2 and b'2^31' in lib.evk_last_error()
    assert _all(_calls(EXPAND, 16, 128, 256, 2048, 512, (1, 2, 3, 6)), -2)
    assert _plan(16, 128, 256, 4096, 0, (1, 2, 3, 6))[0] == -2
    assert _all(_calls(POOL, 16, 128, 256, 4096, 0, (1, 2, 3, 6)), -2)
    assert _plan(16, 64, 64, 2048, 512, (1, 2, 3, 6))[0] == 0


def test_null_and_misaligned_pointers_small_workspaces_and_the_skip_stride_are_refused():
    lib = _C.load()
    geo = (2, 12, 12, 8, 4, (1, 2))
    assert _all(_calls(ALL, *geo, x=None, out=None), -1)
    assert _all(_calls(ALL, *geo, tab=_tab(2, None)), -1)                  # a null entry of the pointer table
    assert _all(_calls(ALL, *geo, tab=_tab(2, FAKE + 4)), -1)              # an entry off the 16-byte grid
    assert _all(_calls(('pool_fwd', 'expand_fwd', 'expand_bwd'), *geo, x=FAKE + 8), -1)
    assert _all(_calls(('pool_bwd', 'expand_fwd'), *geo, out=FAKE + 8), -1)
    assert _all(_calls(('pool_fwd', 'expand_bwd'), *geo, ws=None), -1)
    assert _all(_calls(('pool_fwd', 'expand_bwd'), *geo, ws=FAKE + 4), -1)
    plan = _plan(*geo)[1]
    assert _calls(('pool_fwd',), *geo, ws_bytes=plan[12] - 1) == {'pool_fwd': -4}
    assert b'evk_ppm_pool_workspace_bytes' in lib.evk_last_error()
    assert _calls(('expand_bwd',), *geo, ws_bytes=plan[13] - 1) == {'expand_bwd': -4}
    assert lib.evk_ppm_plan(*geo[:5], None, 2, (ctypes.c_int32 * 16)()) == -1
    assert lib.evk_ppm_plan(*geo[:5], _bins(geo[5]), 2, None) == -1
    # the skip gradient: pixel stride below C, off the 4-float grid, a pointer off the 16-byte grid
    for dskip, ld in ((FAKE, 4), (FAKE, 7), (FAKE, 10), (FAKE + 4, 16)):
        assert _calls(('pool_bwd',), *geo, dskip=dskip, ld=ld) == {'pool_bwd': -1}, (dskip, ld)
    # an expand without pooled maps, a pool without the map
    assert _all(_calls(EXPAND, 2, 12, 12, 8, 0, (1, 2)), -1)
    assert _all(_calls(POOL, 2, 12, 12, 0, 4, (1, 2)), -1)


MAPS = [(1, 1), (2, 3), (5, 7), (6, 6), (12, 12), (13, 9), (33, 20), (64, 64), (128, 96)]


@pytest.mark.parametrize('hw', MAPS, ids=lambda m: f'{m[0]}x{m[1]}')
def test_statement_against_aten_on_the_cpu(hw):
    """windows to 1e-12 of aten's float64 pool; the fp32 blend within 8 * 2^-23 max|z| of its own float64 evaluation (nine
    roundings of terms below max|z|) and within max(3 e_aten, that) of aten's float64, e_aten being the distance of aten's
    own fp32 result from it (aten's float64 taps differ from the fp32 taps, as aten's fp32 taps do)"""
    h, w = hw
    rng = np.random.default_rng(h * 1000 + w)
    x = rng.standard_normal((2, h, w, 4))
    for b in range(1, 9):
        s, _, cnt = pc.pool_fwd64(x, b)
        ref = F.adaptive_avg_pool2d(torch.from_numpy(x).permute(0, 3, 1, 2), b).permute(0, 2, 3, 1).numpy()
        assert np.abs(s / cnt[None, :, :, None] - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1.0)
        z = rng.standard_normal((2, b, b, 4)).astype(np.float32)
        got32, got64 = pc.expand_fwd(z, h, w, np.float32), pc.expand_fwd(z, h, w, np.float64)
        assert got32.dtype == np.float32
        zt = torch.from_numpy(z).permute(0, 3, 1, 2)
        at32 = F.interpolate(zt, (h, w), mode='bilinear', align_corners=False).permute(0, 2, 3, 1).numpy()
        at64 = F.interpolate(zt.double(), (h, w), mode='bilinear', align_corners=False).permute(0, 2, 3, 1).numpy()
        bound = 8 * 2.0 ** -23 * np.abs(z).max()
        assert np.abs(got32 - got64).max() <= bound, b
        e_aten = np.abs(at32 - at64).max()
        assert np.abs(got32 - at64).max() <= max(3 * e_aten, bound), b
        if b == 1:
            assert np.array_equal(got32, np.broadcast_to(z, got32.shape))


def test_backward_statements_are_the_adjoints():
    """expand_bwd64 is the transpose of expand_fwd (float64), pool_bwd32 of the window mean; the support sizes count taps"""
    rng = np.random.default_rng(7)
    for (h, w), b in (((13, 9), 3), ((2, 3), 8), ((12, 12), 6), ((5, 7), 1)):
        z = rng.standard_normal((2, b, b, 4)).astype(np.float32)
        dy = rng.standard_normal((2, h, w, 4)).astype(np.float32)
        dz, mag, support = pc.expand_bwd64(dy, b)
        lhs = (pc.expand_fwd(z, h, w, np.float64) * dy).sum()
        assert abs(lhs - (dz * z).sum()) <= 1e-10 * mag.sum()
        assert support.max() <= h * w and (np.abs(dz) <= mag + 1e-300).all()
        x = rng.standard_normal((2, h, w, 4)).astype(np.float32)
        dp = rng.standard_normal((2, b, b, 4)).astype(np.float32)
        s, _, cnt = pc.pool_fwd64(x, b)
        lhs = ((s / cnt[None, :, :, None]) * dp).sum()
        dx = pc.pool_bwd32([dp], (b,), h, w, None)
        assert dx.dtype == np.float32
        assert abs(lhs - (dx.astype(np.float64) * x).sum()) <= 1e-5 * np.abs(x).sum()
