"""evk_augment_scale_batch (csrc/augment.hip) through the C ABI and through THBatchAugment: the image result is written into a
NaN-filled, sentinel-guarded allocation (tests/guard_common.py), the labels into a larger integer buffer prefilled with a
value no case produces, and both are compared BIT FOR BIT with the numpy statement of the contract
(tests/augment_scale_common.py).  The only tolerance in this file is the second witness at the end: aten's CPU chain, within
the bound derived in include/ever_hip.h."""
import itertools

import numpy as np
import pytest
import torch

from tests import augment_scale_common as sc
from tests import preprocess_common as pc
from tests.guard_common import guarded, guards_intact

pytestmark = pytest.mark.gpu

FILL_NAN = 0x7fc00000
MARGIN = 64
MASK_FILL = {torch.uint8: 201, torch.int64: -77}        # labels are 0..5 and 255 (or above 2^32), pad values 255 and 7
MODES = {1: (torch.uint8, torch.uint8), 2: (torch.uint8, torch.int64), 3: (torch.int64, torch.int64)}


def _lib():
    from ever_amd import _C
    return _C.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _source(gen, h, w, c, f32):
    if f32:
        return torch.randn(h, w, c, generator=gen) * torch.pow(2.0, torch.randint(-6, 7, (h, w, c), generator=gen).float())
    return torch.randint(0, 256, (h, w, c), generator=gen, dtype=torch.uint8)


def _mask(gen, h, w, wide):
    m = torch.from_numpy(pc.LABELS)[torch.randint(0, len(pc.LABELS), (h, w), generator=gen)]
    return m.long() if wide else m.to(torch.uint8)


def _limits(h, w, f, op, crop):
    hz, wz = sc.scaled_hw(h, w, f)
    ht, wt = (wz, hz) if op & 1 else (hz, wz)
    return max(ht, crop[0]) - crop[0], max(wt, crop[1]) - crop[1]


def _records(dev_images, dev_masks, scales, ops, origins, mode, override=None):
    recs = []
    for i, im in enumerate(dev_images):
        hz, wz = sc.scaled_hw(im.shape[0], im.shape[1], scales[i])
        rec = [im.data_ptr(), dev_masks[i].data_ptr() if mode else 0, im.shape[0], im.shape[1], ops[i], origins[i][0], origins[i][1],
               0, hz, wz, sc.s_bits(scales[i]), 0]
        for word, value in (override or {}).items():
            rec[word] = value
        recs += rec
    return recs


def _call(lib, dev_images, dev_masks, scales, ops, origins, crop, out_size, c, mean, std, pad, nchw, f32, mode, expect=0, skew=0,
          override=None, unscaled_entry=False):
    """one call into guarded outputs; returns (image [N, C, Ho, Wo] int32 words, labels or None) on the CPU, or, for a refusal
    (`expect` < 0), asserts that nothing was written.  unscaled_entry: evk_augment_batch on the first 8 words of each record"""
    dev = dev_images[0].device
    n, (ho, wo) = len(dev_images), out_size
    recs = _records(dev_images, dev_masks, scales, ops, origins, mode, override)
    if unscaled_entry:
        recs = [v for i in range(n) for v in recs[12 * i:12 * i + 8]]
    host = torch.tensor(recs, dtype=torch.int64)
    table = host.to(dev)
    mean_d = None if mean is None else torch.tensor(mean, dtype=torch.float32, device=dev)
    std_d = None if std is None else torch.tensor(std, dtype=torch.float32, device=dev)
    whole, inner = guarded(n * c * ho * wo + skew, dev)
    inner = inner[skew:]                 # skew: both outputs start off the 16-byte grid (the guard check covers the skipped words)
    margin = MARGIN + skew
    mwhole = None
    if mode:
        mdt = MODES[mode][1]
        mwhole = torch.full((n * ho * wo + 2 * margin,), MASK_FILL[mdt], dtype=mdt, device=dev)
    entry = lib.evk_augment_batch if unscaled_entry else lib.evk_augment_scale_batch
    rc = entry(host.data_ptr(), table.data_ptr(), n, c, crop[0], crop[1], ho, wo, None if mean_d is None else mean_d.data_ptr(),
               None if std_d is None else std_d.data_ptr(), pad, int(nchw), int(f32), mode, inner.data_ptr(),
               None if mwhole is None else mwhole[margin:].data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.evk_last_error())
    assert guards_intact(whole, inner.numel() + skew), 'wrote outside the image output'
    assert skew == 0 or bool((whole[64:64 + skew].view(torch.int32) == FILL_NAN).all()), 'wrote in front of the image output'
    words = inner.view(torch.int32).cpu()
    labels = None
    if mode:
        m = mwhole.cpu()
        fill = MASK_FILL[MODES[mode][1]]
        assert bool((m[:margin] == fill).all()) and bool((m[margin + n * ho * wo:] == fill).all()), 'wrote outside the label output'
        labels = m[margin:margin + n * ho * wo].view(n, ho, wo)
    if expect != 0:
        assert bool((words == FILL_NAN).all()), 'a refused call wrote image elements'
        assert labels is None or bool((labels == fill).all()), 'a refused call wrote labels'
        return None, None
    left = int((words == FILL_NAN).sum())
    assert left == 0, f'{left} of {words.numel()} image elements unwritten'
    if mode:
        assert not bool((labels == fill).any()), 'labels left unwritten'
    words = words.view(n, ho, wo, c).permute(0, 3, 1, 2) if not nchw else words.view(n, c, ho, wo)
    return words, labels


def _check(lib, images, masks, scales, ops, origins, crop, out_size, mean, std, pad, nchw, mode, what, dev_images=None,
           dev_masks=None, skew=0):
    """images / masks: CPU tensors (masks in the mode's input dtype); compares one call with the numpy statement"""
    dev = torch.device('cuda:0')
    c, f32 = images[0].shape[2], images[0].dtype == torch.float32
    dev_images = dev_images or [im.to(dev) for im in images]
    dev_masks = dev_masks or ([m.to(dev) for m in masks] if mode else None)
    words, labels = _call(lib, dev_images, dev_masks, scales, ops, origins, crop, out_size, c, mean, std, pad, nchw, f32, mode, skew=skew)
    ref, mref = sc.augment_scale_ref(images, masks if mode else None, scales, ops, origins, crop, out_size, mean, std, pad,
                                     MODES[mode][1] if mode else None)
    bad = words != ref.view(torch.int32)
    assert not bool(bad.any()), (f'{what}: {int(bad.sum())} of {bad.numel()} image words differ, first at '
                                 f'{tuple(int(v) for v in bad.nonzero()[0])}')
    if mode:
        assert labels.dtype == mref.dtype and torch.equal(labels, mref), f'{what}: labels differ'
    return words, labels


def _mean_std(c):
    return tuple(100.0 + 7.25 * k for k in range(c)), tuple(50.0 + 3.3 * k for k in range(c))


@pytest.mark.parametrize('f32', (False, True), ids=('u8', 'f32'))
@pytest.mark.parametrize('c', (1, 3, 4))
@pytest.mark.parametrize('op', range(8))
def test_full_product_of_sources_outputs_factors_layouts_and_origin_limits(cuda, op, c, f32):
    """13 x 9 and 9 x 13 sources, crop 8 x 8, output 8 x 8 and 16 x 16, factors 0.5 / 0.75 / 1.25 / 2.0, NHWC and NCHW, the
    origin at 0 and at its upper limit; the three mask dtype pairs and the two pad values cycle through the 64 calls"""
    lib = _lib()
    gen = torch.Generator().manual_seed(1000 * op + 10 * c + f32)
    mean, std = _mean_std(c)
    crop = (8, 8)
    for (h, w) in ((13, 9), (9, 13)):
        image = _source(gen, h, w, c, f32)
        masks = {wide: _mask(gen, h, w, wide) for wide in (False, True)}
        dev_image, dev_masks = image.cuda(), {k: v.cuda() for k, v in masks.items()}
        for idx, (out_size, f, nchw, at_limit) in enumerate(itertools.product(((8, 8), (16, 16)), (0.5, 0.75, 1.25, 2.0), (False, True),
                                                                              (False, True))):
            mode, pad = 1 + idx % 3, (255, 7)[(idx // 3) % 2]
            wide = MODES[mode][0] == torch.int64
            origin = _limits(h, w, f, op, crop) if at_limit else (0, 0)
            _check(lib, [image], [masks[wide]], [f], [op], [origin], crop, out_size, mean, std, pad, nchw, mode,
                   f'{h}x{w}x{c} f {f} op {op} out {out_size} origin {origin} nchw {nchw} mode {mode}',
                   dev_images=[dev_image], dev_masks=[dev_masks[wide]])


@pytest.mark.parametrize('f32', (False, True), ids=('u8', 'f32'))
def test_a_single_scaled_pixel_has_ratio_zero(cuda, f32):
    """3 x 5 at f = 0.34: Hz = Wz = 1, ry = rx = 0, every op reads source pixel (0, 0)"""
    lib = _lib()
    gen = torch.Generator().manual_seed(34)
    assert sc.scaled_hw(3, 5, 0.34) == (1, 1) and sc.ratio(3, 1) == 0
    image, mask = _source(gen, 3, 5, 3, f32), _mask(gen, 3, 5, False)
    for op, nchw in itertools.product(range(8), (False, True)):
        words, labels = _check(lib, [image], [mask], [0.34], [op], [(0, 0)], (4, 4), (8, 8), None, None, 7, nchw, 1, f'ratio 0 op {op}')
        assert torch.equal(words[0, :, 0, 0], image[0, 0].float().view(torch.int32)) and int(labels[0, 0, 0]) == int(mask[0, 0])


@pytest.mark.parametrize('nchw', (False, True), ids=('nhwc', 'nchw'))
def test_a_factor_fp32_does_not_represent(cuda, nchw):
    """f = 1.1: s = float(1 / 1.1) and both ratios are inexact; 37 x 33 -> 40 x 36 into a 48 x 32 output is more than one
    workgroup, with the window past the scaled image on one axis only"""
    lib = _lib()
    gen = torch.Generator().manual_seed(11)
    for (h, w), crop, out_size in (((13, 9), (8, 8), (16, 16)), ((37, 33), (40, 24), (48, 32)), ((37, 33), (16, 17), (17, 23))):
        hz, wz = sc.scaled_hw(h, w, 1.1)
        assert float(sc.inv_scale(1.1)) != 1 / 1.1 and float(sc.ratio(h, hz)) != (h - 1) / (hz - 1)
        for (c, f32, mode), op in itertools.product(((3, False, 1), (4, True, 3)), range(8)):
            image, mask = _source(gen, h, w, c, f32), _mask(gen, h, w, mode == 3)
            _check(lib, [image], [mask], [1.1], [op], [_limits(h, w, 1.1, op, crop)], crop, out_size, *_mean_std(c), 255, nchw, mode,
                   f'f 1.1 {h}x{w} c {c} op {op}')


def test_the_last_row_and_column_land_on_the_last_tap(cuda):
    """f = 2.0 on 16 x 16: sy = (15 / 31) * 31 is Hs - 1 exactly, so y0 = Hs - 1 with y1 == y0 and weight 0; f = 1.5: sy =
    (15 / 23) * 23 rounds ABOVE 15, so y0 = Hs - 1 with a weight of 2^-20 on the clamped second tap.  The source sits at the
    end of its allocation's used part: a tap at y0 + 1 would read the NaN row behind it."""
    lib = _lib()
    gen = torch.Generator().manual_seed(2)
    i0, i1, lo, hi = sc._axis(16, 32)
    assert i0[-1] == 15 and i1[-1] == 15 and lo[-1] == 0 and hi[-1] == 1
    i0, i1, lo, hi = sc._axis(16, 24)
    assert i0[-1] == 15 and i1[-1] == 15 and 0 < lo[-1] < 1e-5
    for f, n in ((2.0, 32), (1.5, 24)):
        for c, f32, nchw, op in ((3, False, False, 0), (3, True, True, 6), (1, False, False, 3), (4, True, True, 5)):
            image, mask = _source(gen, 16, 16, c, f32), _mask(gen, 16, 16, False)
            dev = torch.full((18, 16, c), float('nan') if f32 else 255, dtype=image.dtype, device=cuda)
            dev[:16] = image.to(cuda)
            words, _ = _check(lib, [image], [mask], [f], [op], [(0, 0)], (n, n), (32, 32), None, None, 255, nchw, 2,
                              f'last tap f {f} op {op}', dev_images=[dev[:16]])
            if op == 0 and f == 2.0:
                assert torch.equal(words[0, :, 31, 31], image[15, 15].float().view(torch.int32))


@pytest.mark.parametrize('nchw', (False, True), ids=('nhwc', 'nchw'))
def test_a_scaled_image_smaller_than_the_crop(cuda, nchw):
    """13 x 9 at 0.5 is 6 x 4: raw zeros and label 0 inside the 8 x 8 crop past it, +0.0 and the pad label outside the crop"""
    lib = _lib()
    gen = torch.Generator().manual_seed(6)
    image, mask = _source(gen, 13, 9, 3, False), _mask(gen, 13, 9, False)
    for op in range(8):
        ht, wt = (4, 6) if op & 1 else (6, 4)
        words, labels = _check(lib, [image], [mask], [0.5], [op], [(0, 0)], (8, 8), (16, 16), None, None, 7, nchw, 1, f'small op {op}')
        words[:, :, :ht, :wt] = 0
        labels = labels.clone()
        assert bool((words == 0).all())
        assert bool((labels[0, :8, :8][ht:] == 0).all()) and bool((labels[0, :8, wt:8] == 0).all())
        assert bool((labels[0, 8:] == 7).all()) and bool((labels[0, :, 8:] == 7).all())
        _check(lib, [image], [mask], [0.5], [op], [(0, 0)], (8, 8), (16, 16), *_mean_std(3), 7, nchw, 1, f'small normalised op {op}')


def test_64_channels(cuda):
    lib = _lib()
    gen = torch.Generator().manual_seed(64)
    for f32, nchw, op, out_size, f in ((False, False, 0, (8, 8), 1.5), (True, True, 3, (8, 8), 0.75), (False, True, 5, (9, 9), 1.25),
                                       (True, False, 6, (9, 9), 2.0)):
        image, mask = _source(gen, 9, 7, 64, f32), _mask(gen, 9, 7, False)
        _check(lib, [image], [mask], [f], [op], [(0, 0)], (8, 8), out_size, *_mean_std(64), 255, nchw, 2, f'C 64 op {op} out {out_size}')


@pytest.mark.parametrize('mode', (1, 2, 3))
def test_label_modes(cuda, mode):
    """uint8 -> uint8, uint8 -> int64, int64 -> int64 with values above 2^32 (aten has no nearest kernel for int64)"""
    lib = _lib()
    gen = torch.Generator().manual_seed(40 + mode)
    image = _source(gen, 13, 21, 3, False)
    mask = _mask(gen, 13, 21, mode == 3)
    if mode == 3:
        mask = mask + (1 << 33) + (mask << 34)
    for f, op, out_size, nchw in ((0.75, 0, (16, 16), False), (1.75, 3, (16, 16), True), (1.25, 6, (17, 19), False), (0.5, 5, (17, 19), True)):
        _, labels = _check(lib, [image], [mask], [f], [op], [(0, 0)], (12, 16), out_size, *_mean_std(3), 255, nchw, mode,
                           f'mode {mode} f {f} op {op}')
        assert labels.dtype == MODES[mode][1] and (mode != 3 or int(labels.max()) > (1 << 32))


def test_sources_at_odd_byte_addresses_and_outputs_off_the_16_byte_grid(cuda):
    lib = _lib()
    gen = torch.Generator().manual_seed(9)
    h, w = 13, 21
    for c, off in ((3, 1), (1, 3), (3, 5)):
        image, mask = _source(gen, h, w, c, False), _mask(gen, h, w, False)
        ibuf = torch.zeros(h * w * c + 16, dtype=torch.uint8, device=cuda)
        mbuf = torch.zeros(h * w + 16, dtype=torch.uint8, device=cuda)
        di, dm = ibuf[off:off + h * w * c].view(h, w, c), mbuf[off + 2:off + 2 + h * w].view(h, w)
        di.copy_(image)
        dm.copy_(mask)
        assert di.data_ptr() % 2 == 1 and dm.data_ptr() % 2 == 1 and (w * c) % 4 != 0
        for op, f in ((0, 0.75), (6, 1.25), (3, 1.5), (7, 0.5)):
            _check(lib, [image], [mask], [f], [op], [(0, 0)], (16, 16), (16, 32), *_mean_std(c), 255, False, 1,
                   f'odd address c {c} op {op}', dev_images=[di], dev_masks=[dm])
    # output sizes off the 4 grid take the pixel-per-thread form; Ho * Wo % 4 == 0 but outputs 4 bytes / 1 byte off the grid too
    image, mask = _source(gen, 37, 33, 3, False), _mask(gen, 37, 33, False)
    for nchw, op in itertools.product((False, True), (0, 2, 3, 5)):
        _check(lib, [image, image], [mask, mask], [1.25, 0.75], [op, 7 - op], [(1, 2), (0, 0)], (16, 17), (17, 23), *_mean_std(3), 7,
               nchw, 1, f'out 17x23 op {op}')
        _check(lib, [image], [mask], [1.5], [op], [(1, 2)], (16, 16), (32, 32), pc.MEAN3, pc.STD3, 255, nchw, 1, 'off-grid outputs', skew=1)


@pytest.mark.parametrize('nchw', (False, True), ids=('nhwc', 'nchw'))
def test_a_mixed_batch_with_two_unscaled_samples(cuda, nchw):
    """five samples of different sizes, ops and factors in one launch; the two at f = 1.0 are not scaled"""
    lib = _lib()
    gen = torch.Generator().manual_seed(55)
    sizes, ops, scales = pc.SOURCE_SIZES, (3, 0, 5, 4, 7), (0.75, 1.0, 1.5, 2.0, 1.0)
    crop, out_size = (16, 24), (32, 32)
    for f32, mode in ((False, 1), (True, 2), (False, 3), (True, 0)):
        images = [_source(gen, h, w, 3, f32) for h, w in sizes]
        masks = [_mask(gen, h, w, mode == 3) for h, w in sizes]
        origins = []
        for (h, w), op, f in zip(sizes, ops, scales):
            ymax, xmax = _limits(h, w, f, op, crop)
            origins.append((int(torch.randint(0, ymax + 1, (1,), generator=gen)), int(torch.randint(0, xmax + 1, (1,), generator=gen))))
        words, labels = _check(lib, images, masks, list(scales), list(ops), origins, crop, out_size, pc.MEAN3, pc.STD3, 255, nchw, mode,
                               f'mixed mode {mode}')
        # the unscaled samples alone, through evk_augment_batch
        dev = [im.cuda() for im in images]
        devm = [m.cuda() for m in masks]
        for i in (1, 4):
            w1, l1 = _call(lib, [dev[i]], [devm[i]], [1.0], [ops[i]], [origins[i]], crop, out_size, 3, pc.MEAN3, pc.STD3, 255, nchw, f32,
                           mode, unscaled_entry=True)
            assert torch.equal(w1[0], words[i]) and (mode == 0 or torch.equal(l1[0], labels[i]))


@pytest.mark.parametrize('nchw', (False, True), ids=('nhwc', 'nchw'))
def test_all_factors_one_equals_evk_augment_batch_bit_for_bit(cuda, nchw):
    lib = _lib()
    gen = torch.Generator().manual_seed(1)
    sizes, ops = pc.SOURCE_SIZES, (1, 0, 6, 3, 4)
    for f32, mode, out_size in ((False, 1, (32, 32)), (True, 3, (32, 32)), (True, 2, (17, 25))):
        images = [_source(gen, h, w, 3, f32).cuda() for h, w in sizes]
        if f32:
            images[0][0, 0, 0], images[1][2, 1, 1] = -0.0, float('inf')
        masks = [_mask(gen, h, w, mode == 3).cuda() for h, w in sizes]
        origins = [_limits(h, w, 1.0, op, (16, 17)) for (h, w), op in zip(sizes, ops)]
        args = (lib, images, masks, [1.0] * 5, list(ops), origins, (16, 17), out_size, 3, pc.MEAN3, pc.STD3, 7, nchw, f32, mode)
        a, la = _call(*args)
        b, lb = _call(*args, unscaled_entry=True)
        assert torch.equal(a, b) and torch.equal(la, lb)


def test_two_runs_give_the_same_bits(cuda):
    lib = _lib()
    gen = torch.Generator().manual_seed(8)
    images = [_source(gen, h, w, 4, True).cuda() for h, w in pc.SOURCE_SIZES]
    masks = [_mask(gen, h, w, False).cuda() for h, w in pc.SOURCE_SIZES]
    args = (lib, images, masks, [0.5, 1.25, 1.1, 1.0, 1.75], [0, 1, 2, 3, 4], [(0, 0)] * 5, (16, 16), (32, 32), 4, pc.MEAN4, pc.STD4, 255,
            False, True, 2)
    a, la = _call(*args)
    b, lb = _call(*args)
    assert torch.equal(a, b) and torch.equal(la, lb)


def test_refusals_return_their_code_and_write_nothing(cuda):
    lib = _lib()
    gen = torch.Generator().manual_seed(3)
    image, mask = _source(gen, 13, 21, 3, False).to(cuda), _mask(gen, 13, 21, False).to(cuda)
    wide = torch.zeros(4, 4, 65, dtype=torch.uint8, device=cuda)
    mean, std = _mean_std(3)

    def refuse(code, images=(image,), f=2.0, op=0, origin=(0, 0), crop=(8, 8), out_size=(16, 16), c=3, mode=1, ms=(mean, std), override=None):
        _call(lib, list(images), [mask], [f], [op], [origin], crop, out_size, c, ms[0], ms[1], 255, False, False, mode, expect=code,
              override=override)

    refuse(-2, images=(wide,), c=65, mode=0, ms=(None, None))                     # C = 65
    refuse(-1, crop=(17, 8))                                                      # crop larger than the output
    refuse(-1, origin=(19, 0))                                                    # 26 - 8 = 18 is the last row origin of the scaled image
    refuse(-1, origin=(0, 35))                                                    # 42 - 8 = 34
    refuse(-1, op=1, origin=(35, 0))                                              # a swap op exchanges the limits
    refuse(-1, op=1, origin=(0, 19))
    refuse(-1, op=8)
    refuse(-1, ms=(mean, None))
    refuse(-1, override={8: 0})                                                   # Hz < 1
    refuse(-1, override={9: 0})                                                   # Wz < 1
    refuse(-2, override={8: 32768, 9: 32768}, c=2, mode=0, ms=(None, None))       # Hz * Wz * C = 2^31
    for bits in (0, 0x7f800000, 0x7fc00000, 0xbf000000, 0x80000000):              # s: 0, inf, NaN, -0.5, -0
        refuse(-1, override={10: bits})
    refuse(-1, override={10: 1 << 32})
    refuse(-1, override={0: 0})                                                   # a null image
    # a null table
    whole, inner = guarded(3 * 16 * 16, cuda)
    host = torch.tensor([image.data_ptr(), 0, 13, 21, 0, 0, 0, 0, 26, 42, sc.s_bits(2.0), 0], dtype=torch.int64)
    assert lib.evk_augment_scale_batch(host.data_ptr(), None, 1, 3, 8, 8, 16, 16, None, None, 255, 0, 0, 0, inner.data_ptr(), None,
                                       _stream()) == -1
    torch.cuda.synchronize()
    assert guards_intact(whole, inner.numel()) and bool((inner.view(torch.int32) == FILL_NAN).all())


# ------------------------------------------------------------------------------------------------------------ the Python surface
def _draws(images, factors, crop, each, fixed):
    """the draws THBatchAugment makes, composed as it composes them: (scales, ops, origins)"""
    from ever_amd.hip import functional as HF
    scales, ops, origins = [], [], []
    for im in images:
        f = float(np.random.choice(factors, size=1)[0]) if each else fixed
        k = int(np.random.choice([0, 1, 2, 3], 1)[0])
        hflip, vflip = not (0.5 < np.random.uniform()), not (0.5 < np.random.uniform())
        op = HF.D4_ROT90.get(k, HF.D4_IDENTITY)
        op = HF.d4_compose(op, HF.D4_HFLIP) if hflip else op
        op = HF.d4_compose(op, HF.D4_VFLIP) if vflip else op
        hz, wz = sc.scaled_hw(im.shape[0], im.shape[1], f)
        ht, wt = (wz, hz) if op & 1 else (hz, wz)
        y = int(np.random.randint(0, max(ht, crop[0]) - crop[0] + 1, 1)[0])
        x = int(np.random.randint(0, max(wt, crop[1]) - crop[1] + 1, 1)[0])
        scales.append(f)
        ops.append(op)
        origins.append((y, x))
    return scales, ops, origins


@pytest.mark.parametrize('each', (True, False), ids=('each', 'once'))
@pytest.mark.parametrize('name', sorted(pc.BATCHES))
def test_batch_augment_on_cuda_equals_the_statement_under_the_same_draws(cuda, name, each):
    import ever_amd as er
    from ever_amd.hip import functional as HF
    c, crop, div, mean, std, pad, wide, seed = pc.BATCHES[name]
    images, masks = pc.batch_inputs(pc.make_sources(), name)
    dev_images, dev_masks = [im.to(cuda) for im in images], [m.to(cuda) for m in masks]
    factors = np.linspace(0.5, 2.0, 7)
    results = []
    for channels_last in (True, False):
        np.random.seed(seed)
        aug = er.preprocess.thsegm.THBatchAugment(crop, div, mean, std, mask_pad_value=pad, channels_last=channels_last,
                                                  scale_range=(0.5, 2.0), scale_step=0.25, scale_each=each)
        calls = HF.augment_stats['calls']
        image, mask = aug(dev_images, dev_masks)
        assert HF.augment_stats['calls'] == calls + 1
        assert HF.is_nhwc(image) if channels_last else image.is_contiguous()
        results.append((image.cpu().contiguous(), mask.cpu()))
    np.random.seed(seed)
    fixed = None if each else float(np.random.choice(factors, size=1)[0])
    scales, ops, origins = _draws(images, factors, crop, each, fixed)
    assert each is False or len(set(scales)) > 1
    want_i, want_m = sc.augment_scale_ref(images, masks, scales, ops, origins, crop, aug.out_size, mean, std, pad)
    for image, mask in results:
        assert tuple(image.shape) == tuple(want_i.shape) and torch.equal(image.view(torch.int32), want_i.view(torch.int32))
        assert mask.dtype == want_m.dtype and torch.equal(mask, want_m)
    assert torch.equal(results[0][0].view(torch.int32), results[1][0].view(torch.int32))


def test_wrapper_takes_scales_and_keeps_todays_call_when_all_are_one(cuda):
    from ever_amd.hip import functional as HF
    gen = torch.Generator().manual_seed(13)
    images = [_source(gen, h, w, 3, False).to(cuda) for h, w in pc.SOURCE_SIZES[:3]]
    masks = [_mask(gen, h, w, False).to(cuda) for h, w in pc.SOURCE_SIZES[:3]]
    args = (images, masks, [1, 0, 6], [(0, 0)] * 3, (8, 8), (16, 16), pc.MEAN3, pc.STD3)
    a, la = HF.augment_batch(*args)
    b, lb = HF.augment_batch(*args, scales=[1.0, 1, 1.0])
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(la, lb)
    scales = [0.5, 1.0, 1.25]
    z, lz = HF.augment_batch(*args, scales=scales, mask_dtype=torch.int64)
    want_i, want_m = sc.augment_scale_ref([im.cpu() for im in images], [m.cpu() for m in masks], scales, [1, 0, 6], [(0, 0)] * 3, (8, 8),
                                          (16, 16), pc.MEAN3, pc.STD3, 255, torch.int64)
    assert HF.is_nhwc(z) and torch.equal(z.cpu().contiguous().view(torch.int32), want_i.view(torch.int32)) and torch.equal(lz.cpu(), want_m)
    with pytest.raises(ValueError):
        HF.augment_batch(*args, scales=[1.0, 2.0])
    with pytest.raises(ValueError):
        HF.augment_batch(*args, scales=[1.0, 0.0, 2.0])
    with pytest.raises(HF.HipPathError, match='no CPU path'):
        HF.augment_batch([im.cpu() for im in images], None, [0] * 3, [(0, 0)] * 3, (8, 8), (8, 8), None, None, scales=scales)
    with pytest.raises(HF.HipPathError, match='uint8 or fp32'):
        HF.augment_batch([im.half() for im in images], None, [0] * 3, [(0, 0)] * 3, (8, 8), (8, 8), None, None, scales=scales)
    with pytest.raises(HF.HipPathError, match='not traceable'):
        torch.jit.trace(lambda x: HF.augment_batch([x], None, [0], [(0, 0)], (8, 8), (8, 8), None, None, scales=[0.5])[0], (images[0],))


def test_second_witness_atens_cpu_chain_on_the_fp32_cast_sources(cuda):
    """mean = std = None: the fused image against aten's bilinear (CPU) followed by the exact d4 / crop / pad, within
    8 * 2^-23 * max|source|; labels equal (no case here falls into aten's same-size / double-size shortcut)"""
    lib = _lib()
    gen = torch.Generator().manual_seed(77)
    worst, worst_abs = 0.0, 0.0
    for (h, w), f, f32, op in itertools.product(((13, 9), (16, 16), (7, 31), (32, 20)), (0.5, 0.75, 1.25, 1.5, 1.75), (False, True), (0, 3, 6)):
        image, mask = _source(gen, h, w, 3, f32), _mask(gen, h, w, False)
        hz, wz = sc.scaled_hw(h, w, f)
        assert hz not in (h, 2 * h) and wz not in (w, 2 * w)
        crop = out_size = (max(hz, wz), max(hz, wz))
        words, labels = _call(lib, [image.cuda()], [mask.cuda()], [f], [op], [(0, 0)], crop, out_size, 3, None, None, 255, True, f32, 1)
        z = torch.from_numpy(sc.aten_bilinear(image.numpy(), f).copy())
        zm = torch.from_numpy(sc.aten_nearest(mask.numpy(), f).copy())
        want_i, want_m = pc.augment_ref([z], [zm], [op], [(0, 0)], crop, out_size, None, None, 255)
        d = float((words.view(torch.float32).double() - want_i.double()).abs().max())
        bound = sc.image_bound(image.numpy())
        assert d <= bound, (h, w, f, f32, op, d, bound)
        assert torch.equal(labels, want_m)
        worst, worst_abs = max(worst, d / bound), max(worst_abs, d)
    print(f'worst |fused - aten CPU chain|: {worst_abs:.3e}; as a share of 8 * 2^-23 * max|source|: {worst:.4f}')
