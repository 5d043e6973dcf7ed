"""GPU: the stitching kernels of csrc/stitch.hip through the C-ABI, at their edges.  Accumulator, coverage plane and outputs sit
inside the sentinel-guarded allocations of tests/guard_common.py.  The reference is the sequential loop
`acc[:, y0:y0+h, x0:x0+w] += s; count[y0:y0+h, x0:x0+w] += 1` in numpy fp32 and one fp32 division; adds and one correctly
rounded division are the only arithmetic, so every comparison is bit for bit (a NaN quotient is compared as "is a NaN": the
sign of the NaN that 0/0 produces is the processor's choice)."""
import ctypes

import numpy as np
import pytest
import torch

from ever_amd import _C
from ever_amd.magic.bigimage import sliding_window
from tests.guard_common import PAD, guarded, guards_intact

pytestmark = pytest.mark.gpu

LABEL_SENTINEL = 171


def _stream():
    from ever_amd.hip import functional as HF
    return HF._stream()


def _to_mem(a, nchw):
    """logical [.., C, H, W] numpy -> the memory order of the layout"""
    return np.ascontiguousarray(a if nchw else np.moveaxis(a, -3, -1))


def _from_mem(t, shape, nchw):
    """flat device tensor -> logical numpy array of `shape` = (.., C, H, W)"""
    a = t.cpu().numpy()
    if nchw:
        return a.reshape(shape)
    return np.moveaxis(a.reshape(shape[:-3] + (shape[-2], shape[-1], shape[-3])), -1, -3)


def _guarded_from(a, cuda):
    whole, inner = guarded(a.size, cuda)
    inner.copy_(torch.from_numpy(a.reshape(-1)))
    return whole, inner


def _guarded_labels(n, cuda, dtype):
    whole = torch.full((n + 2 * PAD,), LABEL_SENTINEL, device=cuda, dtype=dtype)
    return whole, whole[PAD:PAD + n]


def _label_guards_intact(whole, n):
    return bool((whole[:PAD] == LABEL_SENTINEL).all() and (whole[PAD + n:] == LABEL_SENTINEL).all())


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _reference_add(acc, cnt, scores, origins):
    acc, cnt = acc.copy(), cnt.copy()
    h, w = scores.shape[2:]
    for s, (y0, x0) in zip(scores, origins):
        acc[:, y0:y0 + h, x0:x0 + w] += s
        cnt[y0:y0 + h, x0:x0 + w] += np.float32(1)
    return acc, cnt


def _device_add(cuda, acc0, cnt0, scores, origins, nchw):
    """(acc, count) after evk_stitch_add on guarded copies of acc0 / cnt0; asserts the guards"""
    lib = _C.load()
    c, hs, ws = acc0.shape
    m, _, h, w = scores.shape
    wa, a = _guarded_from(_to_mem(acc0, nchw), cuda)
    wc, cn = _guarded_from(cnt0, cuda)
    s = torch.from_numpy(_to_mem(scores, nchw)).to(cuda)
    flat = [int(v) for yx in origins for v in yx]
    rec = (ctypes.c_int64 * len(flat))(*flat)
    tab = torch.tensor(flat, dtype=torch.int64, device=cuda)
    rc = lib.evk_stitch_add(rec, tab.data_ptr(), m, s.data_ptr(), a.data_ptr(), cn.data_ptr(), c, hs, ws, h, w, int(nchw), _stream())
    assert rc == 0, lib.evk_last_error()
    torch.cuda.synchronize()
    assert guards_intact(wa, acc0.size) and guards_intact(wc, cnt0.size), 'a store beside the accumulator or the coverage plane'
    return _from_mem(a, acc0.shape, nchw), cn.cpu().numpy().reshape(cnt0.shape)


def _plan(origins, c, hs, ws, h, w, nchw):
    flat = [int(v) for yx in origins for v in yx]
    out = (ctypes.c_int32 * 12)()
    assert _C.load().evk_stitch_plan((ctypes.c_int64 * len(flat))(*flat), len(origins), c, hs, ws, h, w, int(nchw), out) == 0
    return list(out)


def _grid_origins(hs, ws, k, s):
    return [(int(b[1]), int(b[0])) for b in np.unique(sliding_window((hs, ws), k, s), axis=0)]


def _random_origins(rng, m, hs, ws, h, w, step=1):
    return [(int(rng.integers(0, hs - h + 1)), int(rng.integers(0, (ws - w) // step + 1)) * step) for _ in range(m)]


_rng = np.random.default_rng(7)
# name -> (C, H, W, h, w, origins)
ADD_CASES = {
    'one-window-is-the-scene': (3, 5, 7, 5, 7, [(0, 0)]),
    '3x3-on-5x7-stride-2': (3, 5, 7, 3, 3, _grid_origins(5, 7, 3, 2)),
    '3x3-on-6x8-stride-2-pulled-back': (3, 6, 8, 3, 3, _grid_origins(6, 8, 3, 2)),
    'coverage-4': (4, 24, 24, 8, 8, _grid_origins(24, 24, 8, 4)),
    'coverage-16': (4, 16, 16, 8, 8, _grid_origins(16, 16, 8, 2)),
    'odd-x0': (4, 9, 24, 4, 8, [(0, 1), (2, 5), (5, 15)]),
    'odd-x0-odd-pixel': (6, 9, 24, 4, 8, [(0, 1), (2, 5), (5, 15)]),
    'W-not-a-multiple-of-4': (8, 9, 21, 4, 8, [(0, 0), (2, 4), (5, 12)]),
    'W-and-pixel-odd': (3, 9, 21, 4, 8, [(0, 0), (2, 4), (5, 12)]),
    'M-1': (4, 20, 24, 4, 8, [(16, 16)]),
    'M-64': (4, 20, 24, 4, 8, _random_origins(_rng, 64, 20, 24, 4, 8, 4)),
    'M-65-chained': (4, 20, 24, 4, 8, _random_origins(_rng, 65, 20, 24, 4, 8, 4)),
    'M-65-chained-scalar': (3, 20, 23, 4, 7, _random_origins(_rng, 65, 20, 23, 4, 7)),
    'two-workgroups-along-a-row': (8, 6, 300, 5, 140, [(0, 0), (1, 160), (0, 80)]),
    'uncovered-pixels-in-the-box': (4, 12, 24, 4, 8, [(0, 0), (8, 16)]),
}
for _c in (1, 3, 4, 6, 8, 64):
    ADD_CASES[f'C-{_c}'] = (_c, 9, 20, 4, 8, [(0, 0), (2, 4), (5, 12), (3, 8)])
# the cases that must take the scalar form, per layout (every other case here takes the 16-byte one)
SCALAR = {0: {'one-window-is-the-scene', '3x3-on-5x7-stride-2', '3x3-on-6x8-stride-2-pulled-back', 'odd-x0-odd-pixel',
              'W-and-pixel-odd', 'M-65-chained-scalar'},
          1: {'one-window-is-the-scene', '3x3-on-5x7-stride-2', '3x3-on-6x8-stride-2-pulled-back', 'coverage-16', 'odd-x0',
              'odd-x0-odd-pixel', 'W-not-a-multiple-of-4', 'W-and-pixel-odd', 'M-65-chained-scalar'}}


@pytest.mark.parametrize('nchw', [0, 1], ids=['nhwc', 'nchw'])
@pytest.mark.parametrize('name', list(ADD_CASES))
def test_stitch_add_equals_the_sequential_loop_bit_for_bit(cuda, name, nchw):
    c, hs, ws, h, w, origins = ADD_CASES[name]
    plan = _plan(origins, c, hs, ws, h, w, nchw)
    cpp = 1 if nchw else c
    assert plan[0] == int((ws * cpp) % 4 == 0 and (w * cpp) % 4 == 0 and all((x0 * cpp) % 4 == 0 for _, x0 in origins))
    assert plan[0] == int(name not in SCALAR[nchw]), (name, plan)
    assert plan[4] == -(-len(origins) // 64)
    rng = np.random.default_rng(len(origins) * 1000 + c)
    scores = rng.standard_normal((len(origins), c, h, w), dtype=np.float32)
    acc0 = rng.standard_normal((c, hs, ws), dtype=np.float32)         # a used accumulator: the kernel adds, it does not set
    cnt0 = rng.integers(0, 3, (hs, ws)).astype(np.float32)
    acc_ref, cnt_ref = _reference_add(acc0, cnt0, scores, origins)
    acc, cnt = _device_add(cuda, acc0, cnt0, scores, origins, nchw)
    bad = _bits(acc) != _bits(acc_ref)
    assert not bad.any(), f'{name}: {int(bad.sum())} accumulator elements differ, first at {tuple(np.argwhere(bad)[0])}'
    assert np.array_equal(_bits(cnt), _bits(cnt_ref)), f'{name}: coverage differs'
    if name.startswith('coverage-'):
        assert int((cnt_ref - cnt0).max()) == int(name.split('-')[1])
    if name == 'uncovered-pixels-in-the-box':
        untouched = (cnt_ref - cnt0) == 0
        assert untouched[:, 8:16].all() and plan[5:9] == [0, 0, 12, 24]       # inside the launch's box, and left as it was
        assert np.array_equal(_bits(acc[:, untouched]), _bits(acc0[:, untouched])) and np.array_equal(cnt[untouched], cnt0[untouched])
    again, cnt_again = _device_add(cuda, acc0, cnt0, scores, origins, nchw)
    assert np.array_equal(_bits(again), _bits(acc)) and np.array_equal(_bits(cnt_again), _bits(cnt)), 'a second run differs'


def _tie_by_rounding():
    """(a, b, n): a < b are neighbouring floats whose quotients by n round to the same float"""
    n = np.float32(3)
    for i in range(1, 1000):
        a = np.float32(3.0) + np.float32(i) * np.float32(2.0 ** -22)        # in [3, 4) the quotients by 3 are 2/3 ulp apart
        b = np.nextafter(a, np.float32(4))
        if a / n == b / n:
            return a, b, n
    raise AssertionError('no rounding tie found')


def _finalize_inputs(c, hs, ws, seed):
    rng = np.random.default_rng(seed)
    acc = rng.standard_normal((c, hs, ws), dtype=np.float32)
    cnt = rng.integers(1, 5, (hs, ws)).astype(np.float32)
    cnt[0, 0] = cnt[hs - 1, ws - 1] = cnt[2, 3:6] = 0                      # never covered (acc stays what add left: 0)
    acc[:, cnt == 0] = 0
    if c >= 2:
        acc[:, 1, 1] = -5
        acc[c - 2:, 1, 1] = 9                                               # the last two classes tie: the first of them
        a, b, n = _tie_by_rounding()
        acc[:, 1, 2] = -5
        acc[0, 1, 2], acc[c - 1, 1, 2], cnt[1, 2] = a, b, n                 # sums differ, quotients do not: class 0
        acc[c - 1, 3, 1] = np.nan                                           # a NaN is maximal
        acc[0, 3, 2] = acc[c - 1, 3, 2] = np.nan                            # two NaNs: the first
        acc[:, 4, 4] = 2.5                                                  # all equal: class 0
    else:
        acc[0, 3, 1] = np.nan
    return acc, cnt


def _device_finalize(cuda, acc, cnt, nchw, mode, in_place=False, i64=False, threshold=0.0, fill=255):
    lib = _C.load()
    c, hs, ws = acc.shape
    wa, a = _guarded_from(_to_mem(acc, nchw), cuda)
    wc, cn = _guarded_from(cnt, cuda)
    if mode == 0:
        wo, o = (wa, a) if in_place else guarded(acc.size, cuda)
    else:
        wo, o = _guarded_labels(hs * ws, cuda, torch.int64 if i64 else torch.uint8)
    rc = lib.evk_stitch_finalize(a.data_ptr(), cn.data_ptr(), c, hs, ws, int(nchw), mode, None if in_place else o.data_ptr(),
                                 int(i64), threshold, fill, _stream())
    assert rc == 0, lib.evk_last_error()
    torch.cuda.synchronize()
    assert guards_intact(wa, acc.size) and guards_intact(wc, cnt.size)
    assert np.array_equal(cn.cpu().numpy().reshape(cnt.shape), cnt), 'the coverage plane was written'
    if mode == 0:
        assert guards_intact(wo, acc.size)
        if not in_place:
            assert np.array_equal(_bits(_from_mem(a, acc.shape, nchw)), _bits(acc)), 'the accumulator was written'
        return _from_mem(o, acc.shape, nchw)
    assert _label_guards_intact(wo, hs * ws)
    assert np.array_equal(_bits(_from_mem(a, acc.shape, nchw)), _bits(acc)), 'the accumulator was written'
    return o.cpu().numpy().reshape(hs, ws)


@pytest.mark.parametrize('nchw', [0, 1], ids=['nhwc', 'nchw'])
@pytest.mark.parametrize('c,ws', [(c, ws) for c in (1, 2, 3, 4, 6, 8, 64) for ws in (12, 13)]
                         + [(1, 1100), (3, 1100), (8, 1100)])       # wide maps: more than one workgroup per row
def test_stitch_finalize_scores_and_labels(cuda, c, ws, nchw):
    hs = 7
    acc, cnt = _finalize_inputs(c, hs, ws, c * 100 + ws)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = acc / cnt
    for in_place in (False, True):
        got = _device_finalize(cuda, acc, cnt, nchw, 0, in_place=in_place)
        nan = np.isnan(q)
        assert np.array_equal(np.isnan(got), nan), 'NaNs (0/0 where nothing was added, and the NaN scores) in other places'
        assert nan[:, cnt == 0].all()
        assert np.array_equal(_bits(got)[~nan], _bits(q)[~nan]), f'scores, in_place={in_place}'
    if c == 1:
        want = (q[0] > np.float32(0.125)).astype(np.int64)
        kw = dict(threshold=0.125)
    else:
        want = torch.from_numpy(q).argmax(dim=0).numpy()
        assert want[1, 1] == c - 2 and want[1, 2] == 0 and want[3, 1] == c - 1 and want[3, 2] == 0 and want[4, 4] == 0
        kw = {}
    for i64, fill in ((False, 255), (True, 255), (False, 9), (True, 100000)):
        w = want.copy()
        w[cnt == 0] = fill
        got = _device_finalize(cuda, acc, cnt, nchw, 1, i64=i64, fill=fill, **kw)
        assert got.dtype == (np.int64 if i64 else np.uint8)
        bad = got.astype(np.int64) != w
        assert not bad.any(), f'labels i64={i64}: {int(bad.sum())} differ, first at {tuple(np.argwhere(bad)[0])}'
        again = _device_finalize(cuda, acc, cnt, nchw, 1, i64=i64, fill=fill, **kw)
        assert np.array_equal(got, again), 'a second run differs'


def test_accumulator_of_more_than_2_to_31_elements(cuda):
    """C = 1, H = W = 46400: element offsets in the far corner are past 2^31 (about 8.6 GB each for the accumulator and the
    coverage plane, 2 GB of labels).  Two overlapping 64 x 64 windows there; the corner exactly, the rest on the device."""
    lib = _C.load()
    hs = ws = 46400
    n = hs * ws
    assert n > 2 ** 31
    k, edge = 64, 128
    origins = [(hs - k, ws - k), (hs - 96, ws - 68)]
    rng = np.random.default_rng(46400)
    scores = rng.standard_normal((2, 1, k, k), dtype=np.float32)
    wa, a = guarded(n, cuda)
    wc, cn = guarded(n, cuda)
    a.zero_()
    cn.zero_()
    s = torch.from_numpy(scores).to(cuda)
    flat = [v for yx in origins for v in yx]
    tab = torch.tensor(flat, dtype=torch.int64, device=cuda)
    rc = lib.evk_stitch_add((ctypes.c_int64 * 4)(*flat), tab.data_ptr(), 2, s.data_ptr(), a.data_ptr(), cn.data_ptr(), 1, hs, ws,
                            k, k, 0, _stream())
    assert rc == 0, lib.evk_last_error()
    wl, lab = _guarded_labels(n, cuda, torch.uint8)
    rc = lib.evk_stitch_finalize(a.data_ptr(), cn.data_ptr(), 1, hs, ws, 0, 1, lab.data_ptr(), 0, 0.25, 255, _stream())
    assert rc == 0, lib.evk_last_error()
    torch.cuda.synchronize()
    assert guards_intact(wa, n) and guards_intact(wc, n) and _label_guards_intact(wl, n)
    acc_ref, cnt_ref = _reference_add(np.zeros((1, edge, edge), np.float32), np.zeros((edge, edge), np.float32), scores,
                                      [(y - (hs - edge), x - (ws - edge)) for y, x in origins])
    a2, c2, l2 = a.view(hs, ws), cn.view(hs, ws), lab.view(hs, ws)
    corner = (slice(hs - edge, hs), slice(ws - edge, ws))
    assert np.array_equal(_bits(a2[corner].cpu().numpy()), _bits(acc_ref[0]))
    assert np.array_equal(_bits(c2[corner].cpu().numpy()), _bits(cnt_ref))
    with np.errstate(invalid='ignore'):
        want = np.where(cnt_ref == 0, 255, acc_ref[0] / cnt_ref > np.float32(0.25)).astype(np.uint8)
    assert np.array_equal(l2[corner].cpu().numpy(), want) and set(np.unique(want)) == {0, 1, 255}
    # the rest: blank the corner, then the whole planes must be zero / the fill label
    a2[corner] = 0
    c2[corner] = 0
    l2[corner] = 255
    assert not bool(a.any()) and not bool(cn.any())
    assert int(lab.min()) == 255


def test_refusals_leave_the_buffers_unwritten(cuda):
    lib = _C.load()
    c, hs, ws, h, w = 3, 8, 12, 4, 8
    wa, a = guarded(c * hs * ws, cuda)
    wc, cn = guarded(hs * ws, cuda)
    wo, o = guarded(c * hs * ws, cuda)
    wl, lab = _guarded_labels(hs * ws, cuda, torch.uint8)
    s = torch.zeros(65 * c * h * w, device=cuda)
    good = [0, 0, 2, 4]
    tab = torch.tensor(good + [0] * 128, dtype=torch.int64, device=cuda)

    def add(records=good, m=2, scores=s.data_ptr(), acc=a.data_ptr(), count=cn.data_ptr(), table=tab.data_ptr(), c_=c, hs_=hs,
            ws_=ws, h_=h, w_=w):
        rec = None if records is None else (ctypes.c_int64 * len(records))(*records)
        return lib.evk_stitch_add(rec, table, m, scores, acc, count, c_, hs_, ws_, h_, w_, 0, _stream())

    assert add(records=None) == -1 and add(table=None) == -1 and add(scores=None) == -1 and add(acc=None) == -1
    assert add(count=None) == -1 and add(m=0) == -1 and add(h_=0) == -1 and add(w_=0) == -1 and add(c_=0) == -1
    assert add(records=[0, 0, 5, 4]) == -1 and add(records=[0, 0, 0, 5]) == -1 and add(records=[-1, 0, 0, 0]) == -1
    assert add(records=[0, 0] * 64 + [7, 0], m=65) == -1            # the bad window is in the second launch: nothing is launched
    assert add(c_=65536) == -2

    def fin(acc=a.data_ptr(), count=cn.data_ptr(), c_=c, mode=0, dst=o.data_ptr(), i64=0, fill=255):
        return lib.evk_stitch_finalize(acc, count, c_, hs, ws, 0, mode, dst, i64, 0.0, fill, _stream())

    assert fin(acc=None) == -1 and fin(count=None) == -1 and fin(mode=2) == -1 and fin(c_=0) == -1
    assert fin(mode=1, dst=None) == -1 and fin(mode=1, dst=lab.data_ptr(), c_=257) == -2
    assert fin(mode=1, dst=lab.data_ptr(), fill=256) == -1
    torch.cuda.synchronize()
    for whole, inner in ((wa, a), (wc, cn), (wo, o)):
        assert bool(torch.isnan(inner).all()) and guards_intact(whole, inner.numel()), 'a refused call wrote something'
    assert bool((lab == LABEL_SENTINEL).all()) and _label_guards_intact(wl, hs * ws)
