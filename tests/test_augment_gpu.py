"""evk_augment_batch (csrc/augment.hip) through the C ABI: the image result is written into a NaN-filled, sentinel-guarded
allocation (tests/guard_common.py), the labels into a larger integer buffer prefilled with a value no case produces, and both
are compared bit for bit with the CPU evaluation of the entry point's semantics (tests/preprocess_common.augment_ref: torch
ops, `sub().div()`).  No tolerance anywhere in this file."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests import preprocess_common as pc
from tests.guard_common import guarded, guards_intact

pytestmark = pytest.mark.gpu

FILL_NAN = 0x7fc00000
MARGIN = 64
MASK_FILL = {torch.uint8: 201, torch.int64: -77}        # labels are 0..5 and 255, pad values 255 and 7
DIRECT, TILE, DIRECT_SCALAR = 0, 1, 2
MODES = {1: (torch.uint8, torch.uint8), 2: (torch.uint8, torch.int64), 3: (torch.int64, torch.int64)}
SMALL, LARGE = (13, 21), (37, 33)      # the larger one crosses a 32-pixel tile edge in both axes with a ragged remainder


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


def _limits(h, w, op, crop):
    ht, wt = (w, h) if op & 1 else (h, w)
    return max(ht, crop[0]) - crop[0], max(wt, crop[1]) - crop[1]


def _call(lib, dev_images, dev_masks, ops, origins, crop, out_size, c, mean, std, pad, nchw, f32, mode, expect=0, skew=0):
    """one evk_augment_batch call into guarded outputs; returns (image [N, C, Ho, Wo] int32 words, labels or None) on the CPU,
    or, for a refusal (`expect` < 0), asserts that nothing was written"""
    dev = dev_images[0].device
    n, (ho, wo) = len(dev_images), out_size
    recs = []
    for i, im in enumerate(dev_images):
        recs += [im.data_ptr(), dev_masks[i].data_ptr() if mode else 0, im.shape[0], im.shape[1], ops[i], origins[i][0],
                 origins[i][1], 0]
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
    rc = lib.evk_augment_batch(host.data_ptr(), table.data_ptr(), n, c, crop[0], crop[1], ho, wo,
                               None if mean_d is None else mean_d.data_ptr(), None if std_d is None else std_d.data_ptr(), pad,
                               int(nchw), int(f32), mode, inner.data_ptr(),
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


def _check(lib, images, masks, ops, origins, crop, out_size, mean, std, pad, nchw, mode, what, dev_images=None, dev_masks=None, skew=0):
    """images / masks: CPU tensors (masks in the mode's input dtype); compares one call with augment_ref"""
    dev = torch.device('cuda:0')
    c, f32 = images[0].shape[2], images[0].dtype == torch.float32
    dev_images = dev_images or [im.to(dev) for im in images]
    dev_masks = dev_masks or ([m.to(dev) for m in masks] if mode else None)
    words, labels = _call(lib, dev_images, dev_masks, ops, origins, crop, out_size, c, mean, std, pad, nchw, f32, mode, skew=skew)
    ref, mref = pc.augment_ref(images, masks if mode else None, ops, origins, crop, out_size, mean, std, pad,
                               MODES[mode][1] if mode else None)
    bad = words != ref.view(torch.int32)
    assert not bool(bad.any()), (f'{what}: {int(bad.sum())} of {bad.numel()} image words differ, first at '
                                 f'{tuple(int(v) for v in bad.nonzero()[0])}')
    if mode:
        assert labels.dtype == mref.dtype and torch.equal(labels, mref), f'{what}: labels differ'


def _plan_kernel(lib, h, w, c, op, origin, crop, out_size, f32, nchw):
    out = (ctypes.c_int32 * 6)()
    assert lib.evk_augment_plan(h, w, c, op, origin[0], origin[1], crop[0], crop[1], out_size[0], out_size[1], int(f32),
                                int(nchw), out) == 0, lib.evk_last_error()
    return out[0]


def _mean_std(c):
    return tuple(100.0 + 7.25 * k for k in range(c)), tuple(50.0 + 3.3 * k for k in range(c))


# (source, crop, output): a pad ring around a window inside the source; a window inside the larger source; a window past the
# larger source on one axis only (40 > 37 and 33 rows, 24 < 33 and 37 columns), so the raw-zero pad falls inside it
GEOMETRIES = ((SMALL, (16, 16), (32, 32)), (LARGE, (16, 16), (32, 32)), (LARGE, (40, 24), (48, 32)))


@pytest.mark.parametrize('f32', (False, True), ids=('u8', 'f32'))
@pytest.mark.parametrize('c', (1, 3, 4, 6))
@pytest.mark.parametrize('op', range(8))
def test_every_op_width_dtype_at_both_origin_limits_in_both_layouts(cuda, op, c, f32):
    """3 geometries x origin at 0 / at its upper limit x NHWC / NCHW; the three mask dtype pairs and the two pad values cycle
    through the twelve calls"""
    lib = _lib()
    gen = torch.Generator().manual_seed(1000 * op + 10 * c + f32)
    mean, std = _mean_std(c)
    for idx, (((h, w), crop, out_size), at_limit, nchw) in enumerate(itertools.product(GEOMETRIES, (False, True), (False, True))):
        mode, pad = 1 + idx % 3, (255, 7)[(idx // 3) % 2]
        origin = _limits(h, w, op, crop) if at_limit else (0, 0)
        assert _plan_kernel(lib, h, w, c, op, origin, crop, out_size, f32, nchw) == (TILE if op & 1 else DIRECT)
        image, mask = _source(gen, h, w, c, f32), _mask(gen, h, w, MODES[mode][0] == torch.int64)
        _check(lib, [image], [mask], [op], [origin], crop, out_size, mean, std, pad, nchw, mode,
               f'{h}x{w}x{c} op {op} crop {crop} origin {origin} nchw {nchw} mode {mode}')


@pytest.mark.parametrize('nchw', (False, True), ids=('nhwc', 'nchw'))
@pytest.mark.parametrize('ops', ((3, 0, 5, 4, 7), (0, 2, 4, 6, 2), (1,), (6,)), ids=('mixed', 'plain', 'one_swap', 'one_plain'))
def test_batches_whose_samples_differ_in_size_op_and_origin(cuda, ops, nchw):
    """a mixed batch runs the tile kernel, in which the samples without a swap read directly; a plain one the direct kernel"""
    lib = _lib()
    gen = torch.Generator().manual_seed(77 + len(ops))
    sizes = pc.SOURCE_SIZES[:len(ops)]
    crop, out_size = (16, 24), (32, 32)
    for f32, mode in ((False, 1), (True, 2), (False, 3), (True, 0)):
        images = [_source(gen, h, w, 3, f32) for h, w in sizes]
        masks = [_mask(gen, h, w, mode == 3) for h, w in sizes]
        origins = []
        for (h, w), op in zip(sizes, ops):
            ymax, xmax = _limits(h, w, op, crop)
            origins.append((int(torch.randint(0, ymax + 1, (1,), generator=gen)), int(torch.randint(0, xmax + 1, (1,), generator=gen))))
        _check(lib, images, masks, list(ops), origins, crop, out_size, pc.MEAN3, pc.STD3, 255, nchw, mode, f'{ops} mode {mode}')


def test_arithmetic_is_one_subtraction_and_one_true_division(cuda):
    """every uint8 value in every channel under the default mean / std; a reciprocal multiply would differ on a fifth of them"""
    lib = _lib()
    image = torch.arange(256, dtype=torch.uint8).view(16, 16, 1).expand(16, 16, 3).contiguous()
    m, s = torch.tensor(pc.MEAN3).view(1, 1, 3), torch.tensor(pc.STD3).view(1, 1, 3)
    exact, recip = image.float().sub(m).div(s), image.float().sub(m).mul(1.0 / s)
    assert int((exact != recip).sum()) > 100         # the test discriminates
    for op, nchw in ((0, False), (3, False), (5, True), (6, True)):
        _check(lib, [image], None, [op], [(0, 0)], (16, 16), (16, 16), pc.MEAN3, pc.STD3, 255, nchw, 0, f'arithmetic op {op}')


@pytest.mark.parametrize('f32', (False, True), ids=('u8', 'f32'))
def test_without_mean_and_std_the_value_is_the_cast(cuda, f32):
    lib = _lib()
    gen = torch.Generator().manual_seed(5)
    image, mask = _source(gen, 37, 33, 3, f32), _mask(gen, 37, 33, False)
    for op, nchw in ((0, False), (1, False), (7, True), (4, True)):
        _check(lib, [image], [mask], [op], [(2, 3)], (24, 24), (32, 40), None, None, 7, nchw, 2, f'no mean/std op {op}')


def test_sources_at_odd_byte_addresses_with_rows_off_the_word_grid(cuda):
    """slices of larger buffers that start at odd bytes; 21 * 3 = 63 and 21 bytes per row"""
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
        for op in (0, 6, 3, 7):
            _check(lib, [image], [mask], [op], [(0, 0)], (16, 16), (16, 32), *_mean_std(c), 255, False, 1,
                   f'odd address c {c} op {op}', dev_images=[di], dev_masks=[dm])


@pytest.mark.parametrize('nchw', (False, True), ids=('nhwc', 'nchw'))
def test_outputs_off_the_16_byte_grid_and_sizes_off_the_4_grid_take_the_4_byte_stores(cuda, nchw):
    """16 bytes per thread only when Ho * Wo % 4 == 0 (direct) or Wo % 4 == 0 (tile) and both outputs are on the 16-byte grid"""
    lib = _lib()
    gen = torch.Generator().manual_seed(41)
    h, w = LARGE
    for c, f32, mode, out_size in ((3, False, 1, (17, 23)), (1, True, 2, (19, 21)), (4, False, 3, (17, 17)), (3, False, 1, (18, 22))):
        image, mask = _source(gen, h, w, c, f32), _mask(gen, h, w, mode == 3)
        for op in range(8):          # a swap op brings the tile kernel, whose wide stores need Wo % 4 == 0
            _check(lib, [image, image], [mask, mask], [op, 7 - op], [(1, 2), (0, 0)], (16, 17), out_size, *_mean_std(c), 7, nchw, mode,
                   f'out {out_size} c {c} op {op}')
    # Ho * Wo % 4 == 0, but the image output starts 4 bytes, the labels 1 byte off the grid
    image, mask = _source(gen, h, w, 3, False), _mask(gen, h, w, False)
    for op in (2, 3):
        _check(lib, [image], [mask], [op], [(1, 2)], (16, 16), (32, 32), pc.MEAN3, pc.STD3, 255, nchw, 1, 'off-grid outputs', skew=1)


@pytest.mark.parametrize('kernel', (DIRECT, TILE, DIRECT_SCALAR), ids=('direct', 'tile', 'direct_scalar'))
def test_both_forms_forced_on_the_same_transposing_cases(cuda, kernel):
    lib = _lib()
    gen = torch.Generator().manual_seed(31)
    before = lib.evk_augment_force_kernel(kernel)
    try:
        for c, f32, op, nchw, mode in ((3, False, 1, False, 1), (3, False, 3, True, 2), (4, True, 5, False, 3), (6, False, 7, True, 1),
                                       (1, True, 3, False, 0), (20, False, 5, False, 1), (64, True, 1, True, 2)):
            h, w = LARGE
            crop, out_size = (40, 24), (48, 32)
            origin = _limits(h, w, op, crop)
            assert _plan_kernel(lib, h, w, c, op, origin, crop, out_size, f32, nchw) == kernel % 2
            image, mask = _source(gen, h, w, c, f32), _mask(gen, h, w, mode == 3)
            _check(lib, [image], [mask], [op], [origin], crop, out_size, *_mean_std(c), 255, nchw, mode, f'forced {kernel} c {c} op {op}')
    finally:
        lib.evk_augment_force_kernel(before)


def test_refusals_return_their_code_and_write_nothing(cuda):
    lib = _lib()
    gen = torch.Generator().manual_seed(3)
    image, mask = _source(gen, 13, 21, 3, False).to(cuda), _mask(gen, 13, 21, False).to(cuda)
    wide = torch.zeros(4, 4, 65, dtype=torch.uint8, device=cuda)
    mean, std = _mean_std(3)

    def refuse(code, images=(image,), masks=(mask,), op=0, origin=(0, 0), crop=(8, 8), out_size=(16, 16), c=3, mode=1, ms=(mean, std)):
        _call(lib, list(images), list(masks), [op], [origin], crop, out_size, c, ms[0], ms[1], 255, False, False, mode, expect=code)

    refuse(-2, images=(wide,), masks=(mask,), c=65, mode=0, ms=(None, None))     # C = 65
    refuse(-1, crop=(17, 8))                                                      # crop larger than the output
    refuse(-1, origin=(6, 0))                                                     # 13 - 8 = 5 is the last row origin
    refuse(-1, origin=(0, 14))
    refuse(-1, op=1, origin=(14, 0))                                              # a swap op exchanges the limits: 21 - 8 = 13
    refuse(-1, op=8)
    refuse(-1, ms=(mean, None))
    # a null table
    whole, inner = guarded(3 * 16 * 16, cuda)
    host = torch.tensor([image.data_ptr(), 0, 13, 21, 0, 0, 0, 0], dtype=torch.int64)
    assert lib.evk_augment_batch(host.data_ptr(), None, 1, 3, 8, 8, 16, 16, None, None, 255, 0, 0, 0, inner.data_ptr(), None,
                                 _stream()) == -1
    torch.cuda.synchronize()
    assert guards_intact(whole, inner.numel()) and bool((inner.view(torch.int32) == FILL_NAN).all())


@pytest.mark.parametrize('name', sorted(pc.BATCHES))
def test_batch_augment_on_cuda_equals_the_reference_fixture(cuda, name):
    """THBatchAugment on device tensors, one launch, against the reference's own per-image pipeline (the fixture)"""
    import ever_amd as er
    from ever_amd.hip import functional as HF
    golden = np.load(pc.GOLDEN)
    src = {k: golden[k] for k in pc.make_sources()}
    want_i, want_m = torch.from_numpy(golden[f'{name}/image']), torch.from_numpy(golden[f'{name}/mask'])
    c, crop, div, mean, std, pad, wide, seed = pc.BATCHES[name]
    images, masks = pc.batch_inputs(src, name, cuda)
    for channels_last in (True, False):
        aug = er.preprocess.thsegm.THBatchAugment(crop, div, mean, std, mask_pad_value=pad, channels_last=channels_last)
        calls = HF.augment_stats['calls']
        np.random.seed(seed)
        image, mask = aug(images, masks)
        assert HF.augment_stats['calls'] == calls + 1
        assert image.is_cuda and tuple(image.shape) == tuple(want_i.shape)
        assert HF.is_nhwc(image) if channels_last else image.is_contiguous()
        assert torch.equal(image.cpu().contiguous().view(torch.int32), want_i.view(torch.int32))
        assert mask.dtype == want_m.dtype and torch.equal(mask.cpu(), want_m)
    np.random.seed(seed)
    _, labels = er.preprocess.thsegm.THBatchAugment(crop, div, mean, std, mask_pad_value=pad, mask_dtype=torch.int64)(images, masks)
    assert labels.dtype == torch.int64 and torch.equal(labels.cpu(), want_m.long())


def test_farseg_takes_both_layouts_of_one_batch_to_the_same_logits(cuda):
    import ever_amd as er
    from ever_amd.hip import functional as HF
    torch.manual_seed(0)
    model = er.module.FarSeg(dict(encoder=dict(resnet_type='resnet18'),
                                  head=dict(fpn=dict(in_channels_list=(64, 128, 256, 512), out_channels=256),
                                            fs_relation=dict(scene_embedding_channels=512)))).to(cuda).eval()
    gen = torch.Generator().manual_seed(4)
    images = [_source(gen, h, w, 3, False).to(cuda) for h, w in ((70, 90), (64, 64), (100, 66))]
    outs = []
    for channels_last in (True, False):
        np.random.seed(12)
        x, _ = er.preprocess.thsegm.THBatchAugment((60, 64), 32, channels_last=channels_last)(images)
        assert tuple(x.shape) == (3, 3, 64, 64)
        with torch.no_grad():
            outs.append((x, model(x)))
    (xa, la), (xb, lb) = outs
    assert HF.is_nhwc(xa) and xb.is_contiguous() and torch.equal(xa, xb)
    assert torch.equal(la.contiguous().view(torch.int32), lb.contiguous().view(torch.int32))


def test_wrapper_refuses_traces_cpu_tensors_and_other_dtypes(cuda):
    from ever_amd.hip import functional as HF
    image = torch.zeros(16, 16, 3, dtype=torch.uint8, device=cuda)

    def call(x, masks=None, **kw):
        return HF.augment_batch([x], masks, [0], [(0, 0)], (8, 8), (8, 8), None, None, **kw)[0]

    with pytest.raises(HF.HipPathError, match='not traceable'):
        torch.jit.trace(call, (image,))
    with pytest.raises(HF.HipPathError, match='no CPU path'):
        call(image.cpu())
    with pytest.raises(HF.HipPathError, match='uint8 or fp32'):
        call(image.half())
    with pytest.raises(HF.HipPathError, match='int64 -> int64'):
        call(image, [torch.zeros(16, 16, dtype=torch.int64, device=cuda)], mask_dtype=torch.uint8)
    with pytest.raises(ValueError):
        HF.augment_batch([image], None, [0, 1], [(0, 0)], (8, 8), (8, 8), None, None)
    out = call(image.float())
    assert HF.is_nhwc(out) and tuple(out.shape) == (1, 3, 8, 8) and float(out.abs().max()) == 0.0
