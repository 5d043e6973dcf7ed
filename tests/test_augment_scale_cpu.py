"""The rescale step of THBatchAugment without a device: the random draws, the CPU path against the hand-composed per-image
chain, the host plan of the scaled pass (evk_augment_scale_plan: ratios, refusals, origin limits; no launch), and the numpy
statement of its arithmetic (tests/augment_scale_common.py) held to aten's CPU kernels."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from ever_amd import _C
from ever_amd.hip import functional as HF
from ever_amd.preprocess import thcomm, thsegm
from tests import augment_scale_common as sc
from tests import preprocess_common as pc

RANGE, STEP = (0.5, 2.0), 0.25
FACTORS = np.linspace(0.5, 2.0, 7)


def _images(c=3):
    src = pc.make_sources()
    return ([torch.from_numpy(src[f'img{c}_{i}']) for i in range(len(pc.SOURCE_SIZES))],
            [torch.from_numpy(src[f'mask_{i}']) for i in range(len(pc.SOURCE_SIZES))])


def _record_draws(monkeypatch):
    """every np.random call THBatchAugment makes, in order, as (name, result)"""
    log = []
    for name in ('choice', 'uniform', 'randint'):
        real = getattr(np.random, name)

        def spy(*a, _real=real, _name=name, **kw):
            v = _real(*a, **kw)
            log.append((_name, len(a[0]) if _name == 'choice' else None, float(np.asarray(v).reshape(-1)[0])))
            return v
        monkeypatch.setattr(np.random, name, spy)
    return log


def test_the_keywords_exist_and_default_to_no_scale_step():
    aug = thsegm.THBatchAugment((16, 16), scale_range=RANGE, scale_step=STEP, scale_each=True)
    assert np.array_equal(aug.scale_factors, FACTORS) and aug.scale_each and aug.scale_factor is None
    assert thsegm.THBatchAugment((16, 16)).scale_factors is None
    # the reference's expression, not a rounded count: (1.3 - 0.5) / 0.2 is 4.000000000000001 -> 5 factors
    assert len(thsegm.THBatchAugment((16, 16), scale_range=(0.5, 1.3), scale_step=0.2).scale_factors) == int((1.3 - 0.5) / 0.2) + 1


def test_scale_each_draws_the_factor_first_then_k_flips_and_origin_per_image(monkeypatch):
    images, masks = _images()
    aug = thsegm.THBatchAugment((16, 16), 32, pc.MEAN3, pc.STD3, scale_range=RANGE, scale_step=STEP)
    np.random.seed(21)
    want = []
    for im in images:
        f = float(np.random.choice(FACTORS, size=1)[0])
        k = int(np.random.choice([0, 1, 2, 3], 1)[0])
        u1, u2 = np.random.uniform(), np.random.uniform()
        hz, wz = sc.scaled_hw(im.shape[0], im.shape[1], f)
        ht, wt = (wz, hz) if k % 2 else (hz, wz)
        y = int(np.random.randint(0, max(ht, 16) - 16 + 1, 1)[0])
        x = int(np.random.randint(0, max(wt, 16) - 16 + 1, 1)[0])
        want += [('choice', 7, f), ('choice', 4, float(k)), ('uniform', None, u1), ('uniform', None, u2), ('randint', None, float(y)),
                 ('randint', None, float(x))]
    log = _record_draws(monkeypatch)
    np.random.seed(21)
    aug(images, masks)
    assert log == want and len(log) == 6 * len(images)


def test_scale_once_draws_one_factor_at_construction_as_THRandomScale_does(monkeypatch):
    images, masks = _images()
    np.random.seed(8)
    want = thsegm.THRandomScale(RANGE, STEP).scale_factor
    after = np.random.uniform()
    np.random.seed(8)
    log = _record_draws(monkeypatch)
    aug = thsegm.THBatchAugment((16, 16), 32, pc.MEAN3, pc.STD3, scale_range=RANGE, scale_step=STEP, scale_each=False)
    assert aug.scale_factor == want and log == [('choice', 7, float(want))]
    assert np.random.uniform() == after
    del log[:]
    aug(images, masks)
    assert [e[:2] for e in log] == [('choice', 4), ('uniform', None), ('uniform', None), ('randint', None), ('randint', None)] * len(images)


def test_without_scale_range_the_random_stream_is_todays(monkeypatch):
    images, masks = _images()
    want_i, want_m = pc.run_batch_per_image(pc.namespace(None, thcomm, thsegm), pc.make_sources(), 'batch_pad_ring')
    c, crop, div, mean, std, pad, _, seed = pc.BATCHES['batch_pad_ring']
    tail = np.random.uniform()
    log = _record_draws(monkeypatch)
    np.random.seed(seed)
    aug = thsegm.THBatchAugment(crop, div, mean, std, mask_pad_value=pad, channels_last=False, scale_range=None, scale_step=0.5,
                                scale_each=False)
    assert log == []
    image, mask = aug(images, masks)
    assert len(log) == 5 * len(images) and np.random.uniform() == tail
    assert torch.equal(image.view(torch.int32), want_i.view(torch.int32)) and torch.equal(mask, want_m)


@pytest.mark.parametrize('each', (True, False), ids=('each', 'once'))
@pytest.mark.parametrize('c,f32', ((3, False), (4, True)), ids=('c3_u8', 'c4_f32'))
def test_cpu_path_equals_the_hand_composed_per_image_chain(each, c, f32):
    """THRandomScale's expression at the drawn factor on the image cast to fp32, then the existing classes; scale_each=False
    is the reference pipeline THRandomScale -> ... built and then run under one seed"""
    images, masks = _images(c)
    images = [im.float() * 0.37 for im in images] if f32 else images
    mean, std = (pc.MEAN3, pc.STD3) if c == 3 else (pc.MEAN4, pc.STD4)
    crop, div, pad = (20, 24), 32, 7
    np.random.seed(33)
    scale = None if each else thsegm.THRandomScale(RANGE, STEP)
    tail = (thsegm.THRandomRotate90k(), thsegm.THRandomHorizontalFlip(), thsegm.THRandomVerticalFlip(), thsegm.THRandomCrop(crop),
            thcomm.THChannelFirst2(), thcomm.THMeanStdNormalize2(mean, std), thcomm.THDivisiblePad(div, pad))
    outs = []
    for im, m in zip(images, masks):
        if each:
            f = np.random.choice(FACTORS, size=1)[0]
            cur = thsegm._rescale(im.float(), m, f)
        else:
            cur = scale(im.float(), m)
        assert cur[0].dtype == torch.float32 and cur[1].dtype == torch.uint8
        outs.append(thcomm.Pipeline(*tail)(*cur))
    want_i, want_m = torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])
    for channels_last in (False, True):
        np.random.seed(33)
        aug = thsegm.THBatchAugment(crop, div, mean, std, mask_pad_value=pad, channels_last=channels_last, scale_range=RANGE,
                                    scale_step=STEP, scale_each=each, mask_dtype=torch.int64)
        image, mask = aug(images, masks)
        assert tuple(image.shape) == (len(images), c, 32, 32) and HF.is_nhwc(image) == channels_last
        assert torch.equal(image.contiguous().view(torch.int32), want_i.view(torch.int32))
        assert mask.dtype == torch.int64 and torch.equal(mask, want_m.long())
    # an image smaller than the crop after scaling needs its mask, as in THRandomCrop
    with pytest.raises(TypeError):
        np.random.seed(33)
        thsegm.THBatchAugment((64, 64), scale_range=(0.5, 0.5))(images)


# ------------------------------------------------------------------------------------------------------------ the host plan
def _plan(lib, hs, ws, c, op, y0, x0, ch, cw, ho, wo, hz, wz, sbits, f32=0, nchw=0):
    out = (ctypes.c_int32 * 5)()
    rc = lib.evk_augment_scale_plan(hs, ws, c, op, y0, x0, ch, cw, ho, wo, f32, nchw, hz, wz, sbits, out)
    return rc, tuple(out)


def _bits(v):
    return int(np.array(v, dtype=np.float32).view(np.int32))


ONE = 0x3f800000


def test_plan_gives_the_ratios_of_the_statement_bit_for_bit():
    lib = _C.load()
    assert lib.evk_abi_version() == 21
    # Hz = 1 (ratio 0), Hz = 2 (ratio Hs - 1), Hz = Hs (ratio 1), and inexact ratios
    for (hs, ws), scaled in itertools.product(((3, 5), (13, 9), (16, 16), (1000, 37)), ((1, 1), (2, 1), (1, 2), (2, 2), None, (7, 11), (14, 9), (33, 1999))):
        hz, wz = scaled or (hs, ws)
        rc, (kernel, per, vec, ry, rx) = _plan(lib, hs, ws, 3, 0, 0, 0, 8, 8, 8, 8, hz, wz, ONE)
        assert rc == 0, lib.evk_last_error()
        assert (ry, rx) == (_bits(sc.ratio(hs, hz)), _bits(sc.ratio(ws, wz))), (hs, ws, hz, wz)
        assert (kernel, per, vec) == (0, 12, 1)
    assert _plan(lib, 3, 5, 3, 0, 0, 0, 8, 8, 8, 8, 1, 1, ONE)[1][3:] == (0, 0)
    assert _plan(lib, 3, 5, 3, 0, 0, 0, 8, 8, 8, 8, 2, 2, ONE)[1][3:] == (_bits(2.0), _bits(4.0))
    assert _plan(lib, 3, 5, 3, 0, 0, 0, 8, 8, 8, 8, 3, 5, ONE)[1][3:] == (ONE, ONE)
    # a thread owns whole pixels: four with 16-byte stores (Ho * Wo % 4 == 0), else one
    assert [_plan(lib, 13, 9, c, 1, 0, 0, 8, 8, ho, wo, 6, 4, _bits(2.0))[1][1:3] for c, ho, wo in ((1, 8, 8), (4, 9, 12), (3, 10, 10), (64, 9, 9))] \
        == [(4, 1), (16, 1), (12, 1), (64, 0)]
    before = lib.evk_augment_force_kernel(2)
    try:
        assert _plan(lib, 13, 9, 3, 0, 0, 0, 8, 8, 8, 8, 6, 4, _bits(2.0))[1][1:3] == (3, 0)
    finally:
        lib.evk_augment_force_kernel(before)


def test_plan_refusals_and_origin_limits_on_the_scaled_swapped_size():
    lib = _C.load()
    ok = dict(hs=13, ws=21, c=3, op=0, y0=0, x0=0, ch=8, cw=8, ho=8, wo=8, hz=26, wz=42, sbits=_bits(0.5))

    def rc(**kw):
        return _plan(lib, **{**ok, **kw})[0]

    assert rc() == 0
    assert rc(c=65) == -2 and b'channels' in lib.evk_last_error()
    assert rc(cw=9) == -1 and b'larger than the output' in lib.evk_last_error()
    assert rc(op=8) == -1 and rc(op=-1) == -1 and rc(hs=0) == -1 and rc(c=0) == -1
    assert rc(hs=32768, ws=32768, c=2) == -2 and b'source' in lib.evk_last_error()
    assert rc(hz=0) == -1 and b'scaled size' in lib.evk_last_error()
    assert rc(wz=0) == -1 and rc(hz=-3) == -1
    assert rc(hz=32768, wz=32768, c=2) == -2 and b'scaled image' in lib.evk_last_error()
    assert rc(hz=32768, wz=32767, c=2) == 0
    for bad in (0.0, -0.5, np.inf, -np.inf, np.nan):
        assert rc(sbits=_bits(bad)) == -1 and b'not finite and positive' in lib.evk_last_error(), bad
    assert rc(sbits=_bits(-0.0)) == -1 and rc(sbits=1) == 0 and rc(sbits=0x7f7fffff) == 0
    # origins against d4 of (Hz, Wz) = (26, 42), not of the source (13, 21)
    assert rc(y0=18, x0=34) == 0 and rc(y0=19) == -1 and b'origin' in lib.evk_last_error()
    assert rc(x0=35) == -1 and rc(y0=-1) == -1
    assert rc(op=1, y0=34, x0=18) == 0 and rc(op=1, y0=18, x0=19) == -1 and rc(op=1, y0=35) == -1
    # a scaled image smaller than the crop leaves only origin 0 on that axis
    assert rc(hz=6, wz=10, sbits=_bits(2.0), x0=2) == 0 and rc(hz=6, wz=10, sbits=_bits(2.0), y0=1) == -1
    assert rc(op=3, hz=6, wz=10, sbits=_bits(2.0), y0=2) == 0 and rc(op=3, hz=6, wz=10, sbits=_bits(2.0), x0=1) == -1
    out = (ctypes.c_int32 * 5)()
    assert lib.evk_augment_scale_plan(13, 21, 3, 0, 0, 0, 8, 8, 8, 8, 0, 0, 26, 42, ONE, None) == -1
    # the launcher's refusals come before any launch, so they are safe without a GPU
    rec = (ctypes.c_int64 * 12)(1, 0, 13, 21, 0, 0, 0, 0, 26, 42, _bits(0.5), 0)
    args = (1, 3, 8, 8, 8, 8, None, None, 255, 0, 0, 0)
    assert lib.evk_augment_scale_batch(None, None, *args, 1, None, None) == -1 and b'null record table' in lib.evk_last_error()
    assert lib.evk_augment_scale_batch(rec, 1, *args, None, None, None) == -1
    for word, value in ((8, 0), (9, 0), (10, 0), (10, 1 << 32), (10, _bits(np.inf)), (5, 19), (4, 8), (0, 0)):
        bad = (ctypes.c_int64 * 12)(*rec)
        bad[word] = value
        assert lib.evk_augment_scale_batch(bad, 1, *args, 1, None, None) == -1, (word, value)
    big = (ctypes.c_int64 * 12)(1, 0, 13, 21, 0, 0, 0, 0, 32768, 32768, _bits(0.5), 0)
    assert lib.evk_augment_scale_batch(big, 1, 1, 2, 8, 8, 8, 8, None, None, 255, 0, 0, 0, 1, None, None) == -2
    assert lib.evk_augment_scale_batch(rec, 1, 1, 3, 8, 8, 32768, 32768, None, None, 255, 0, 0, 0, 1, None, None) == -2 \
        and b'output' in lib.evk_last_error()


# ------------------------------------------------------------------------------------------ the statement against aten's CPU
ATEN_SIZES = ((13, 9), (9, 13), (16, 16), (7, 31), (32, 20), (4, 4), (5, 8))
ATEN_FACTORS = (0.5, 0.75, 1.25, 1.5, 1.75)


def test_statement_labels_equal_atens_cpu_nearest_on_every_chosen_case():
    """sizes >= 4 and factors that never give Hz in {Hs, 2 Hs}: aten's same-size / double-size shortcut is not taken"""
    g = np.random.default_rng(1)
    n = 0
    for (h, w), f in itertools.product(ATEN_SIZES, ATEN_FACTORS):
        hz, wz = sc.scaled_hw(h, w, f)
        assert min(h, w) >= 4 and hz >= 1 and wz >= 1 and hz not in (h, 2 * h) and wz not in (w, 2 * w)
        m = g.integers(0, 256, (h, w)).astype(np.uint8)
        got, want = sc.nearest(m, f), sc.aten_nearest(m, f)
        assert got.shape == want.shape == (hz, wz) and np.array_equal(got, want), (h, w, f)
        n += 1
    assert n == len(ATEN_SIZES) * len(ATEN_FACTORS)
    # int64 labels go through the same formula (aten has no such kernel on the CPU)
    wide = g.integers(0, 256, (9, 13)).astype(np.int64) + (1 << 33)
    assert np.array_equal(sc.nearest(wide, 1.5) - (1 << 33), sc.aten_nearest((wide - (1 << 33)).astype(np.uint8), 1.5))


def test_statement_image_is_within_the_derived_bound_of_atens_cpu_bilinear():
    g = np.random.default_rng(2)
    worst = 0.0
    for (h, w), f, kind in itertools.product(ATEN_SIZES + ((3, 5),), ATEN_FACTORS + (0.34, 1.1, 2.0, 1.0), ('u8', 'f32')):
        if min(sc.scaled_hw(h, w, f)) < 1:
            continue
        src = g.integers(0, 256, (h, w, 3)).astype(np.uint8) if kind == 'u8' else (g.standard_normal((h, w, 3)) * 40).astype(np.float32)
        got, want = sc.bilinear(src, f), sc.aten_bilinear(src, f)
        assert got.shape == want.shape and got.dtype == np.float32
        d = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
        assert d <= sc.image_bound(src), (h, w, f, kind, d, sc.image_bound(src))
        worst = max(worst, d / sc.image_bound(src))
    print(f'worst |statement - aten| / bound: {worst:.3f}')
    # f == 1: the source itself, whatever its bits
    odd = np.array([[[-0.0], [np.inf]], [[1e-40], [3.5]]], dtype=np.float32)
    assert sc.bilinear(odd, 1.0).tobytes() == odd.tobytes()
    m = g.integers(0, 7, (5, 8)).astype(np.uint8)
    assert np.array_equal(sc.nearest(m, 1.0), m)
