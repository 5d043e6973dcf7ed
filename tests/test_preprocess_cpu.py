"""CPU: `er.preprocess` against the reference's own results (tests/golden/preprocess_ref.npz, written by
tools/gen_golden_preprocess.py), the composition of dihedral ops, and the host plan of the fused batch pass
(evk_augment_plan: no launch, no GPU)."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import ever_amd as er
from ever_amd import _C
from ever_amd.hip import functional as HF
from ever_amd.preprocess import function as pF, thcomm, thsegm
from tests import preprocess_common as pc
from tests.tta_common import d4_ref

DIRECT, TILE = 0, 1
PP = pc.namespace(pF, thcomm, thsegm)


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(pc.GOLDEN))


# ------------------------------------------------------------------------------------------------ dihedral composition
def test_d4_compose_equals_applying_both_for_all_64_pairs():
    x = torch.arange(2 * 3 * 5 * 7).view(2, 3, 5, 7)
    for a, b in itertools.product(range(8), repeat=2):
        assert torch.equal(d4_ref(d4_ref(x, a), b), d4_ref(x, HF.d4_compose(a, b))), (a, b)
    assert all(HF.d4_compose(op, HF.d4_inverse(op)) == 0 for op in range(8))


def test_rotate_flip_sequence_composes_into_one_op():
    """rot90 k x hflip x vflip as THBatchAugment composes them == the torch expressions of the per-image classes in sequence"""
    x = torch.arange(5 * 7 * 3).view(5, 7, 3)
    for k, h, v in itertools.product(range(4), (False, True), (False, True)):
        seq = torch.rot90(x, k, [0, 1]) if k else x
        seq = torch.flip(seq, [1]) if h else seq
        seq = torch.flip(seq, [0]) if v else seq
        op = HF.D4_ROT90.get(k, HF.D4_IDENTITY)
        op = HF.d4_compose(op, HF.D4_HFLIP) if h else op
        op = HF.d4_compose(op, HF.D4_VFLIP) if v else op
        assert torch.equal(pc.d4_hw(x, op), seq), (k, h, v, op)
        assert tuple(seq.shape[:2]) == HF.d4_out_hw(5, 7, op)


# ------------------------------------------------------------------------------------------------ the reference's API
def test_package_is_exported_under_both_names():
    assert er.preprocess.thsegm is thsegm and er.preprocess.thcomm is thcomm and er.preprocess.function is pF
    import sys
    er.install_as_ever()
    assert sys.modules['ever.preprocess.thsegm'] is thsegm and sys.modules['ever.preprocess'] is er.preprocess
    for mod, names in ((pF, ('th_mean_std_normalize', 'th_divisible_pad', 'th_pad_to_size')),
                       (thcomm, ('Pipeline', 'FuncWrapper', 'ToTensor', 'THChannelFirst', 'THChannelFirst2', 'THMeanStdNormalize',
                                 'THMeanStdNormalize2', 'THDivisiblePad')),
                       (thsegm, ('THRandomRotate90k', 'THRandomHorizontalFlip', 'THRandomVerticalFlip', 'THRandomCrop',
                                 'THRandomScale', 'THBatchAugment'))):
        assert all(hasattr(mod, n) for n in names)


CASES = sorted(pc.per_image_cases(PP, pc.make_sources()))


@pytest.mark.parametrize('name', CASES)
def test_per_image_class_equals_the_reference_fixture(golden, name):
    """values, shapes, dtypes, tuple arity and None entries, bit for bit, under the fixture's seed"""
    src = {k: golden[k] for k in pc.make_sources()}
    arity, kinds, arrays = pc.flatten(pc.per_image_cases(PP, src)[name]())
    assert arity == int(golden[f'{name}/arity']) and kinds == golden[f'{name}/kinds'].tolist()
    for j, a in enumerate(arrays):
        want = golden[f'{name}/{j}']
        assert a.dtype == want.dtype and a.shape == want.shape, (name, j, a.dtype, a.shape, want.dtype, want.shape)
        assert a.tobytes() == want.tobytes(), (name, j)


def test_fixture_sources_are_what_the_tests_build(golden):
    for k, v in pc.make_sources().items():
        assert np.array_equal(golden[k], v) and golden[k].dtype == v.dtype, k


@pytest.mark.parametrize('name', sorted(pc.BATCHES))
def test_batch_pipeline_and_batch_augment_equal_the_reference_fixture(golden, name):
    src = pc.make_sources()
    want_i, want_m = golden[f'{name}/image'], golden[f'{name}/mask']
    image, mask = pc.run_batch_per_image(PP, src, name)
    assert image.numpy().tobytes() == want_i.tobytes() and mask.numpy().tobytes() == want_m.tobytes()
    c, crop, div, mean, std, pad, wide, seed = pc.BATCHES[name]
    images, masks = pc.batch_inputs(src, name)
    for channels_last in (True, False):
        aug = thsegm.THBatchAugment(crop, div, mean, std, mask_pad_value=pad, channels_last=channels_last)
        np.random.seed(seed)
        image, mask = aug(images, masks)
        assert tuple(image.shape) == want_i.shape and image.dtype == torch.float32
        assert image.permute(0, 2, 3, 1).is_contiguous() if channels_last else image.is_contiguous()
        assert image.contiguous().numpy().tobytes() == want_i.tobytes()
        assert mask.numpy().dtype == want_m.dtype and mask.numpy().tobytes() == want_m.tobytes()
    if not wide:
        np.random.seed(seed)
        _, mask = thsegm.THBatchAugment(crop, div, mean, std, mask_pad_value=pad, mask_dtype=torch.int64)(images, masks)
        assert mask.dtype == torch.int64 and np.array_equal(mask.numpy(), want_m.astype(np.int64))


def test_batch_augment_draws_follow_the_reference_order():
    """the fused path's draws (no GPU needed to make them): k, hflip, vflip, then ymin, xmin per image, in list order"""
    src = pc.make_sources()
    images, _ = pc.batch_inputs(src, 'batch_pad_ring')
    np.random.seed(5)
    want = []
    for im in images:
        k = int(np.random.choice([0, 1, 2, 3], 1)[0])
        h, v = not (0.5 < np.random.uniform()), not (0.5 < np.random.uniform())
        ht, wt = (im.shape[1], im.shape[0]) if k % 2 else (im.shape[0], im.shape[1])
        y = int(np.random.randint(0, max(ht, 16) - 16 + 1, 1)[0])
        x = int(np.random.randint(0, max(wt, 16) - 16 + 1, 1)[0])
        want.append((k, h, v, y, x))
    np.random.seed(5)
    got = []
    for im in images:
        k, h, v = thsegm._draw_k(None), thsegm._draw_flip(0.5), thsegm._draw_flip(0.5)
        ht, wt = (im.shape[1], im.shape[0]) if k % 2 else (im.shape[0], im.shape[1])
        got.append((k, h, v) + thsegm._draw_origin(ht, wt, (16, 16)))
    assert got == want


@pytest.mark.parametrize('name', sorted(pc.BATCHES))
def test_fused_semantics_equal_the_reference_fixture(golden, name):
    """what the GPU tests compare the kernel with (preprocess_common.augment_ref: one op, one origin, window, normalise, pad)
    is the reference's per-image pipeline: under the fixture's seed it reproduces the fixture bit for bit"""
    c, crop, div, mean, std, pad, wide, seed = pc.BATCHES[name]
    images, masks = pc.batch_inputs(pc.make_sources(), name)
    np.random.seed(seed)
    ops, origins = [], []
    for im in images:
        k, h, v = thsegm._draw_k(None), thsegm._draw_flip(0.5), thsegm._draw_flip(0.5)
        op = HF.D4_ROT90.get(k, HF.D4_IDENTITY)
        op = HF.d4_compose(op, HF.D4_HFLIP) if h else op
        op = HF.d4_compose(op, HF.D4_VFLIP) if v else op
        ops.append(op)
        origins.append(thsegm._draw_origin(*HF.d4_out_hw(im.shape[0], im.shape[1], op), crop))
    out_size = thsegm.THBatchAugment(crop, div).out_size
    image, mask = pc.augment_ref(images, masks, ops, origins, crop, out_size, mean, std, pad)
    assert image.numpy().tobytes() == golden[f'{name}/image'].tobytes()
    assert mask.numpy().dtype == golden[f'{name}/mask'].dtype and mask.numpy().tobytes() == golden[f'{name}/mask'].tobytes()


def test_observable_behaviours_of_the_reference():
    img, mask = torch.zeros(13, 21, 3, dtype=torch.uint8), torch.zeros(13, 21, dtype=torch.uint8)
    out = thsegm.THRandomCrop((9, 9))(img)
    assert isinstance(out, tuple) and len(out) == 1                       # a tuple even without a mask
    with pytest.raises(TypeError):
        thsegm.THRandomCrop((16, 16))(img)                               # padding needs the mask
    im, m = thsegm.THRandomCrop((16, 16))(img + 9, mask + 9)
    assert int(im[13:].max()) == 0 and int(m[13:].max()) == 0 and m.dtype == torch.uint8     # both padded with 0
    # THChannelFirst's guess: a first axis of at most 8 entries is taken for channels
    assert thcomm.THChannelFirst()(torch.zeros(8, 10, 3)).shape == (8, 10, 3)
    assert thcomm.THChannelFirst()(torch.zeros(9, 10, 3)).shape == (3, 9, 10)
    # pad_to_size pads the original image, not the divisibly padded one; the mask goes through both
    pi, pm = thcomm.THDivisiblePad(32, 255, (40, 40))(torch.ones(3, 13, 21), mask.long())
    assert pi.shape == (3, 40, 40) and pm.shape == (40, 40) and pm.dtype == torch.int64
    assert int(pm[13:].min()) == 255 and float(pi[:, 13:].abs().max()) == 0.0
    with pytest.raises(AssertionError):
        thcomm.THDivisiblePad(32, 255, (20, 20))(torch.ones(3, 13, 21), mask)         # mask already 32 x 32
    np.random.seed(0)
    a = thsegm.THRandomScale().scale_factor
    np.random.seed(0)
    assert a == np.random.choice(np.linspace(0.5, 2.0, 7), size=1)[0]                # drawn at construction


# ------------------------------------------------------------------------------------------------ the host plan
def _plan(lib, hs, ws, c, op, y0, x0, ch, cw, ho, wo, f32, nchw):
    out = (ctypes.c_int32 * 6)()
    rc = lib.evk_augment_plan(hs, ws, c, op, y0, x0, ch, cw, ho, wo, int(f32), int(nchw), out)
    return rc, tuple(out)


def test_augment_plan_names_the_form_of_every_gpu_case():
    """the rule: a swap op on a narrow pixel goes through the LDS tile, whose edge follows the pixel width; everything else is
    direct"""
    lib = _C.load()
    for (hs, ws), c, f32, nchw, op in itertools.product(((13, 21), (37, 33)), (1, 3, 4, 6), (0, 1), (0, 1), range(8)):
        rc, (kernel, t, stride, lds, per, vec) = _plan(lib, hs, ws, c, op, 0, 0, 16, 16, 32, 32, f32, nchw)
        assert rc == 0, lib.evk_last_error()
        if op & 1:
            assert kernel == TILE and t == (32 if c <= 4 else 16)
            assert stride >= t * c and stride % 32 == (1 if nchw else c % 32) and stride - t * c < 32
            assert lds == t * stride * 4 + 32 * 33 * 8 and lds <= 64 * 1024
            assert per == -(-t * t * c // 256) and per <= 16 and vec == 1
        else:
            assert (kernel, t, stride, lds, per, vec) == (DIRECT, 0, 0, 0, 0, 1)
    # the measured crossover: the tile up to C = 6 (NHWC output) and C = 8 (NCHW output), whatever the source type
    for f32 in (0, 1):
        assert [_plan(lib, 37, 33, c, 5, 0, 0, 16, 16, 32, 32, f32, 0)[1][0] for c in (6, 7, 8, 16, 64)] == [TILE, DIRECT, DIRECT, DIRECT, DIRECT]
        assert [_plan(lib, 37, 33, c, 5, 0, 0, 16, 16, 32, 32, f32, 1)[1][0] for c in (6, 8, 9, 16, 64)] == [TILE, TILE, DIRECT, DIRECT, DIRECT]
    lib.evk_augment_force_kernel(TILE)
    assert _plan(lib, 9, 7, 64, 1, 0, 0, 4, 4, 4, 4, 0, 0)[1][:2] == (TILE, 8)
    lib.evk_augment_force_kernel(-1)
    # 16-byte stores need Ho * Wo % 4 == 0 (direct) or Wo % 4 == 0 (tile)
    assert [_plan(lib, 13, 21, 3, 1, 0, 0, 8, 8, ho, wo, 0, 0)[1][5] for ho, wo in ((8, 8), (9, 12), (10, 10), (12, 9))] == [1, 1, 0, 0]
    assert [_plan(lib, 13, 21, 3, 0, 0, 0, 8, 8, ho, wo, 0, 0)[1][5] for ho, wo in ((8, 8), (9, 12), (10, 10), (9, 9), (17, 23))] == [1, 1, 1, 0, 0]
    before = lib.evk_augment_force_kernel(DIRECT)
    try:
        assert before == -1 and _plan(lib, 37, 33, 3, 3, 0, 0, 16, 16, 32, 32, 0, 0)[1][0] == DIRECT
        lib.evk_augment_force_kernel(TILE)
        assert _plan(lib, 37, 33, 3, 3, 0, 0, 16, 16, 32, 32, 0, 0)[1][0] == TILE
        assert _plan(lib, 37, 33, 3, 2, 0, 0, 16, 16, 32, 32, 0, 0)[1][0] == DIRECT      # no swap: nothing to stage
        lib.evk_augment_force_kernel(2)                                                     # direct, 4-byte stores only
        assert _plan(lib, 37, 33, 3, 3, 0, 0, 16, 16, 32, 32, 0, 0)[1][::5] == (DIRECT, 0)
    finally:
        lib.evk_augment_force_kernel(-1)


def test_augment_plan_refusals():
    lib = _C.load()
    assert _plan(lib, 13, 21, 65, 0, 0, 0, 8, 8, 8, 8, 0, 0)[0] == -2 and b'channels' in lib.evk_last_error()
    assert _plan(lib, 13, 21, 3, 0, 0, 0, 16, 16, 16, 15, 0, 0)[0] == -1 and b'larger than the output' in lib.evk_last_error()
    assert _plan(lib, 13, 21, 3, 8, 0, 0, 8, 8, 8, 8, 0, 0)[0] == -1
    # origins: 0 <= y0 <= max(Ht, ch) - ch; a swap op exchanges the limits; a crop past the source leaves only 0
    assert _plan(lib, 13, 21, 3, 0, 5, 13, 8, 8, 8, 8, 0, 0)[0] == 0
    assert _plan(lib, 13, 21, 3, 0, 6, 13, 8, 8, 8, 8, 0, 0)[0] == -1 and b'origin' in lib.evk_last_error()
    assert _plan(lib, 13, 21, 3, 0, 5, 14, 8, 8, 8, 8, 0, 0)[0] == -1
    assert _plan(lib, 13, 21, 3, 1, 13, 5, 8, 8, 8, 8, 0, 0)[0] == 0
    assert _plan(lib, 13, 21, 3, 1, 5, 13, 8, 8, 8, 8, 0, 0)[0] == -1
    assert _plan(lib, 13, 21, 3, 0, 0, 5, 16, 16, 16, 16, 0, 0)[0] == 0
    assert _plan(lib, 13, 21, 3, 0, 1, 0, 16, 16, 16, 16, 0, 0)[0] == -1
    assert _plan(lib, 13, 21, 3, 0, -1, 0, 8, 8, 8, 8, 0, 0)[0] == -1
    # 2^31 source elements
    assert _plan(lib, 32768, 32768, 2, 0, 0, 0, 8, 8, 8, 8, 0, 0)[0] == -2 and b'2^31' in lib.evk_last_error()
    assert _plan(lib, 32768, 32767, 2, 0, 0, 0, 8, 8, 8, 8, 0, 0)[0] == 0
    # the launcher's own refusals come before any launch, so they are safe without a GPU: null tables, 2^31 outputs
    rec = (ctypes.c_int64 * 8)(1, 0, 13, 21, 0, 0, 0, 0)
    args = (1, 3, 8, 8, 8, 8, None, None, 255, 0, 0, 0)
    assert lib.evk_augment_batch(None, None, *args, 1, None, None) == -1 and b'null record table' in lib.evk_last_error()
    assert lib.evk_augment_batch(rec, None, *args, 1, None, None) == -1
    assert lib.evk_augment_batch(rec, rec, *args, None, None, None) == -1
    assert lib.evk_augment_batch(rec, rec, 1, 3, 8, 8, 8, 8, 1, None, 255, 0, 0, 0, 1, None, None) == -1     # mean without std
    assert lib.evk_augment_batch(rec, rec, 1, 3, 8, 8, 8, 8, None, None, 255, 0, 0, 1, 1, None, None) == -1   # mask mode, no output
    big = (ctypes.c_int64 * 8)(1, 0, 13, 21, 0, 0, 0, 0)
    assert lib.evk_augment_batch(big, big, 1, 2, 8, 8, 32768, 32768, None, None, 255, 0, 0, 0, 1, None, None) == -2
    assert b'2^31' in lib.evk_last_error()
