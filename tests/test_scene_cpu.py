"""CPU: whole-scene tiled inference (magic/bigimage/scene.py) evaluated with torch ops against `sliding_window_inference`, bit
for bit; `SceneStitcher`'s argument checks and its never-covered pixels; and the host side of csrc/stitch.hip: the form
`evk_stitch_plan` names for a table, and the refusals of the three entry points, which return before any launch."""
import ctypes
import itertools

import pytest
import torch

from ever_amd import _C
from ever_amd.magic.bigimage import SceneStitcher, scene_inference, sliding_window_inference

CASES = [(5, 7, 3, 2), (8, 8, 8, 4), (6, 9, 16, 4), (12, 10, 4, 1), (17, 13, 5, 3)]      # (H, W, kernel, stride)


def _first_channels(c):
    """a deterministic element-wise function of the tile: its first c channels (plus a per-channel shift)"""
    return lambda tiles: tiles[:, :c] + torch.arange(c, dtype=torch.float32).view(1, c, 1, 1)


def _same_bits(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    assert torch.equal(got.contiguous().view(torch.int32), ref.contiguous().view(torch.int32)), what


@pytest.mark.parametrize('n', [1, 2])
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_cpu_scene_inference_equals_sliding_window_inference(case, n):
    ih, iw, k, s = case
    image = torch.randn(n, 4, ih, iw, generator=torch.Generator().manual_seed(ih * 100 + iw))
    model = _first_channels(3)
    for bs in (1, 3, 1000):
        ref = sliding_window_inference(model, image, k, s, batch_size=bs)
        got = scene_inference(model, image, k, s, batch_size=bs)
        _same_bits(got, ref, f'{case} n={n} batch={bs}')
        assert torch.equal(scene_inference(model, image, k, s, batch_size=bs, output='labels', label_dtype=torch.int64),
                           ref.argmax(dim=1))
    # an activation is applied to the window scores, as there
    _same_bits(scene_inference(model, image, k, s, activation=torch.sigmoid),
               sliding_window_inference(model, image, k, s, activation=torch.sigmoid), f'{case} activation')


def test_cpu_rasters_are_normalised_as_sub_div():
    g = torch.Generator().manual_seed(3)
    raster = torch.randint(0, 256, (2, 17, 13, 3), generator=g, dtype=torch.uint8)
    mean, std = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
    image = ((raster.float() - torch.tensor(mean)) / torch.tensor(std)).permute(0, 3, 1, 2)
    model = _first_channels(2)
    ref = sliding_window_inference(model, image, 5, 3, batch_size=4)
    _same_bits(scene_inference(model, raster, 5, 3, batch_size=4, mean=mean, std=std), ref, 'uint8 NHWC raster')
    _same_bits(scene_inference(model, raster[0], 5, 3, mean=mean, std=std), ref[:1], 'uint8 HWC raster')
    _same_bits(scene_inference(model, raster.float(), 5, 3, mean=mean, std=std), ref, 'fp32 raster')
    with pytest.raises(ValueError):
        scene_inference(model, raster, 5, 3, mean=mean)
    with pytest.raises(ValueError):
        scene_inference(model, image, 5, 3, output='classes')
    with pytest.raises(ValueError, match='output stride'):
        scene_inference(lambda t: t[:, :, ::2, ::2], image, 4, 2)


def test_labels_resolve_ties_to_the_first_index_and_treat_nan_as_maximal():
    image = torch.randn(1, 3, 6, 6, generator=torch.Generator().manual_seed(1))
    image[0, 1, 2, 3] = image[0, 2, 2, 3] = 7.0          # classes 1 and 2 tie above class 0
    image[0, 0, 2, 3] = -1.0
    image[0, 2, 4, 1] = float('nan')
    image[0, 0, 5, 5] = float('nan')
    image[0, 2, 5, 5] = float('nan')                      # two NaNs: the first one
    ident = lambda t: t
    ref = sliding_window_inference(ident, image, 6, 6)
    lab = scene_inference(ident, image, 6, 6, output='labels')
    assert lab.dtype == torch.uint8 and lab.shape == (1, 6, 6)
    assert torch.equal(lab.long(), ref.argmax(dim=1))
    assert lab[0, 2, 3] == 1 and lab[0, 4, 1] == 2 and lab[0, 5, 5] == 0
    one = image[:, :1]
    ref1 = sliding_window_inference(ident, one, 4, 2)
    lab1 = scene_inference(ident, one, 4, 2, output='labels', label_dtype=torch.int64, threshold=0.25)
    assert lab1.dtype == torch.int64 and torch.equal(lab1, (ref1[:, 0] > 0.25).long())
    assert lab1[0, 5, 5] == 0                             # NaN > threshold is false
    with pytest.raises(ValueError):
        scene_inference(ident, one, 4, 2, output='labels')                     # one class needs a threshold
    with pytest.raises(ValueError):
        scene_inference(ident, image, 4, 2, output='labels', threshold=0.5)     # more classes take the argmax


def test_scene_stitcher_checks_its_arguments():
    for bad in (dict(num_classes=0), dict(height=-1), dict(width=0), dict(num_classes=2.0), dict(height=True)):
        kw = dict(num_classes=2, height=6, width=8, device='cpu')
        kw.update(bad)
        with pytest.raises(ValueError):
            SceneStitcher(**kw)
    st = SceneStitcher(2, 6, 8, 'cpu')
    assert st.acc.shape == (2, 6, 8) and st.acc.permute(1, 2, 0).is_contiguous() and st.count.shape == (6, 8)
    assert SceneStitcher(2, 6, 8, 'cpu', channels_last=False).acc.is_contiguous()
    s = torch.ones(2, 2, 3, 4)
    for boxes in ([[0, 0, 4, 3]],                                  # one box for two windows
                  [[0, 0, 4, 3], [1, 1, 4, 4]],                    # a box of another size
                  [[0, 0, 4, 3], [5, 0, 9, 3]],                    # past the right border
                  [[0, 0, 4, 3], [0, 4, 4, 7]],                    # past the bottom border
                  [[0, 0, 4, 3], [-1, 0, 3, 3]],                   # negative origin
                  [0, 0, 4, 3]):                                   # not [M, 4]
        with pytest.raises(ValueError):
            st.add(s, boxes)
    with pytest.raises(ValueError):
        st.add(torch.ones(2, 3, 3, 4), [[0, 0, 4, 3], [1, 1, 5, 4]])          # three classes into two
    with pytest.raises(ValueError):
        st.add(s.double(), [[0, 0, 4, 3], [1, 1, 5, 4]])
    assert float(st.count.sum()) == 0 and float(st.acc.abs().sum()) == 0, 'a refused add wrote something'
    with pytest.raises(ValueError):
        st.labels(dtype=torch.int32)
    with pytest.raises(ValueError):
        st.labels(threshold=0.5)
    with pytest.raises(ValueError):
        st.labels(fill_label=256)
    with pytest.raises(ValueError):
        SceneStitcher(1, 4, 4, 'cpu').labels()


def test_never_covered_pixels_give_nan_scores_and_the_fill_label():
    st = SceneStitcher(3, 6, 8, 'cpu')
    s = torch.randn(2, 3, 3, 4, generator=torch.Generator().manual_seed(2))
    st.add(s, [[0, 0, 4, 3], [2, 1, 6, 4]])
    acc = torch.zeros(3, 6, 8)
    acc[:, 0:3, 0:4] += s[0]
    acc[:, 1:4, 2:6] += s[1]
    cnt = torch.zeros(6, 8)
    cnt[0:3, 0:4] += 1
    cnt[1:4, 2:6] += 1
    q = st.scores()
    covered = cnt > 0
    assert torch.equal(st.count, cnt) and bool(torch.isnan(q[:, ~covered]).all())
    _same_bits(q[:, covered], (acc / cnt)[:, covered], 'covered scores')
    for dtype, fill in ((torch.uint8, 255), (torch.int64, 255), (torch.uint8, 7), (torch.int64, -1)):
        lab = st.labels(dtype=dtype, fill_label=fill)
        assert lab.dtype == dtype and bool((lab[~covered] == fill).all())
        assert torch.equal(lab[covered].long(), (acc / cnt).argmax(0)[covered])
    st.reset()
    assert float(st.count.sum()) == 0 and float(st.acc.abs().sum()) == 0
    one = SceneStitcher(1, 6, 8, 'cpu', channels_last=False)
    one.add(s[:, :1], [[0, 0, 4, 3], [2, 1, 6, 4]])
    lab = one.labels(threshold=0.0, fill_label=9)
    assert bool((lab[~covered] == 9).all()) and torch.equal(lab[covered].bool(), ((acc / cnt)[0] > 0.0)[covered])


# ------------------------------------------------------------------ the host side of csrc/stitch.hip
def _records(origins):
    flat = [v for yx in origins for v in yx]
    return (ctypes.c_int64 * len(flat))(*flat)


def _plan(origins, c, h_scene, w_scene, h, w, nchw):
    out = (ctypes.c_int32 * 12)()
    rc = _C.load().evk_stitch_plan(_records(origins), len(origins), c, h_scene, w_scene, h, w, nchw, out)
    return rc, list(out)


def test_plan_names_the_16_byte_form_exactly_where_alignment_allows():
    h_scene, h, w = 12, 4, 8
    seen = set()
    for nchw, c, x0, w_scene in itertools.product((0, 1), (1, 3, 4, 6, 8), (0, 4, 1, 2, 3), (24, 25, 26, 27)):
        cpp = 1 if nchw else c
        rc, out = _plan([(0, 0), (2, x0)], c, h_scene, w_scene, h, w, nchw)
        assert rc == 0
        want = (w_scene * cpp) % 4 == 0 and (w * cpp) % 4 == 0 and (x0 * cpp) % 4 == 0
        assert out[0] == int(want), (nchw, c, x0, w_scene, out)
        seen.add((nchw, c, bool(want)))
        v = 4 if want else 1
        assert out[1] == -(-(x0 + w) * cpp // v // 64) and out[2] == -(-(2 + h) // 4)      # 64 items and 4 rows per workgroup
        assert out[3] == (c if nchw else 1) and out[4] == 1 and out[5:9] == [0, 0, 2 + h, x0 + w]
        assert out[9] == int((w_scene * cpp) % 4 == 0)
        assert out[10] == int(w_scene % 4 == 0 if (nchw or c == 1) else c % 4 == 0)
    # NHWC pixels of 4 or 8 floats put every window edge on the 4-float grid: there is no scalar case to find
    assert {(n, c, f) for n in (0, 1) for c in (1, 3, 4, 6, 8) for f in (False, True)} - {(0, 4, False), (0, 8, False)} == seen
    # an odd window width forces the scalar form wherever a pixel is not a multiple of 4 floats
    assert _plan([(0, 0)], 4, 12, 24, 4, 7, 0)[1][0] == 1 and _plan([(0, 0)], 4, 12, 24, 4, 7, 1)[1][0] == 0
    assert _plan([(0, 0)], 6, 12, 24, 4, 7, 0)[1][0] == 0 and _plan([(0, 0)], 6, 12, 24, 4, 6, 0)[1][0] == 1
    # chained tables: 64 windows per launch, the box is the first launch's
    rc, out = _plan([(i % 5, 0) for i in range(65)], 4, 12, 24, 4, 8, 0)
    assert rc == 0 and out[4] == 2 and out[5:9] == [0, 0, 8, 8]
    assert _plan([(0, 0)] * 64, 4, 12, 24, 4, 8, 0)[1][4] == 1 and _plan([(0, 0)] * 129, 4, 12, 24, 4, 8, 0)[1][4] == 3


def test_refusals_return_their_codes_without_a_device():
    lib = _C.load()
    out = (ctypes.c_int32 * 12)()
    rec = _records([(0, 0), (2, 4)])
    ok = lambda **kw: dict(dict(M=2, C=3, H=8, W=12, h=4, w=8, nchw=0), **kw)

    def plan(records=rec, dst=out, **kw):
        a = ok(**kw)
        return lib.evk_stitch_plan(records, a['M'], a['C'], a['H'], a['W'], a['h'], a['w'], a['nchw'], dst)

    def add(records=rec, table=1, scores=1, acc=1, count=1, **kw):      # pointers are never followed before the checks pass
        a = ok(**kw)
        return lib.evk_stitch_add(records, table, a['M'], scores, acc, count, a['C'], a['H'], a['W'], a['h'], a['w'], a['nchw'], None)

    assert plan() == 0
    for fn in (plan, add):
        assert fn(M=0) == -1 and fn(M=-3) == -1
        assert fn(h=0) == -1 and fn(w=-1) == -1 and fn(C=0) == -1 and fn(H=0) == -1 and fn(W=0) == -1
        assert fn(records=None) == -1
        assert fn(records=_records([(0, 0), (5, 4)])) == -1 and b'not inside' in lib.evk_last_error()     # 5 + 4 > 8 rows
        assert fn(records=_records([(0, 0), (0, 5)])) == -1                                               # 5 + 8 > 12 columns
        assert fn(records=_records([(-1, 0), (0, 0)])) == -1 and fn(records=_records([(0, 0), (0, -4)])) == -1
        assert fn(h=9) == -1 and fn(w=13) == -1                      # a window larger than the scene
        assert fn(C=65536) == -2
        assert fn(C=4096, W=1 << 19, w=8) == -2                      # a row of 2^31 floats
    assert plan(dst=None) == -1
    assert add(table=None) == -1 and add(scores=None) == -1 and add(acc=None) == -1 and add(count=None) == -1
    # a bad window anywhere in a chained table is refused before the first launch
    assert add(records=_records([(0, 0)] * 64 + [(7, 0)]), M=65) == -1

    def fin(acc=1, count=1, C=3, H=8, W=12, nchw=0, mode=0, dst=1, i64=0, fill=255):
        return lib.evk_stitch_finalize(acc, count, C, H, W, nchw, mode, dst, i64, 0.0, fill, None)

    assert fin(acc=None) == -1 and fin(count=None) == -1 and fin(mode=2) == -1 and fin(mode=-1) == -1
    assert fin(mode=1, dst=None) == -1 and b'output' in lib.evk_last_error()
    assert fin(C=0) == -1 and fin(H=0) == -1 and fin(W=-2) == -1
    assert fin(mode=1, C=257) == -2 and b'uint8' in lib.evk_last_error()
    assert fin(mode=1, fill=256) == -1 and fin(mode=1, fill=-1) == -1
    assert fin(C=65536) == -2 and fin(C=4096, W=1 << 19) == -2
