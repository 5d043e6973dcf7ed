"""GPU: whole-scene tiled inference (magic/bigimage/scene.py) on the device.  With an element-wise callable the result is
compared bit for bit against `sliding_window_inference` evaluated on the CPU (gather, adds in box order and one division are
the only arithmetic); with a real model against the existing device function at the tolerance of
tests/test_inference_api_gpu.py, because the model's own bits depend on how its input batch is laid out."""
import numpy as np
import pytest
import torch

from tests.test_tta_gpu import _farseg_r18, _reference_expression

pytestmark = pytest.mark.gpu

MEAN, STD = (123.675, 116.28, 103.53, 99.5), (58.395, 57.12, 57.375, 61.25)


def _same_bits(got, ref, what):
    got, ref = got.detach().cpu().contiguous(), ref.detach().cpu().contiguous()
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, tuple(got.shape), tuple(ref.shape), got.dtype)
    bad = got.view(torch.int32) != ref.view(torch.int32)
    assert not bool(bad.any()), (f'{what}: {int(bad.sum())} of {bad.numel()} elements differ in their bits, first at '
                                 f'{tuple(int(v) for v in bad.nonzero()[0])}: {got[bad][0].item()!r} vs {ref[bad][0].item()!r}')


def _first3(t):
    """element-wise, and the same on both devices: the tile's first three channels, the second one doubled (exact)"""
    s = t[:, :3].clone()
    s[:, 1] *= 2
    return s


def _whole(t):
    return t


@pytest.fixture(scope='module')
def farseg(cuda):
    return _farseg_r18(cuda)


@pytest.mark.parametrize('bs', [1, 5, 64])
@pytest.mark.parametrize('shape', [(40, 56, 16, 8), (33, 47, 16, 12)], ids=['40x56-k16-s8', '33x47-k16-s12'])
def test_device_scene_inference_equals_the_cpu_loop_bit_for_bit(cuda, shape, bs):
    from ever_amd.hip import functional as HF
    from ever_amd.magic.bigimage import scene_inference, sliding_window, sliding_window_inference
    ih, iw, k, s = shape
    g = torch.Generator().manual_seed(ih + bs)
    image = torch.randn(2, 4, ih, iw, generator=g)
    raster = torch.randint(0, 256, (2, ih, iw, 4), generator=g, dtype=torch.uint8)
    normalised = ((raster.float() - torch.tensor(MEAN)) / torch.tensor(STD)).permute(0, 3, 1, 2)
    nboxes = len(np.unique(sliding_window((ih, iw), k, s), axis=0))
    for model in (_first3, _whole):
        ref = sliding_window_inference(model, image, k, s, batch_size=bs)
        for name, x in (('fp32 NCHW', image.to(cuda)), ('fp32 NHWC', image.to(cuda).contiguous(memory_format=torch.channels_last))):
            before, added = HF.augment_stats['calls'], HF.stitch_stats['windows']
            got = scene_inference(model, x, k, s, batch_size=bs)
            assert got.is_cuda and HF.augment_stats['calls'] == before + 2 * -(-nboxes // bs), 'one gather launch per chunk'
            assert HF.stitch_stats['windows'] == added + 2 * nboxes
            _same_bits(got, ref, f'{name} {model.__name__} batch {bs}')
        ref = sliding_window_inference(model, normalised, k, s, batch_size=bs)
        _same_bits(scene_inference(model, raster.to(cuda), k, s, batch_size=bs, mean=MEAN, std=STD), ref,
                   f'uint8 raster {model.__name__} batch {bs}')
        _same_bits(scene_inference(model, raster[1].to(cuda), k, s, batch_size=bs, mean=MEAN, std=STD), ref[1:],
                   f'uint8 HWC raster {model.__name__} batch {bs}')
    # labels are the argmax of the scores output, and never go through it
    x = image.to(cuda)
    scores = scene_inference(_whole, x, k, s, batch_size=bs)
    for dtype in (torch.uint8, torch.int64):
        lab = scene_inference(_whole, x, k, s, batch_size=bs, output='labels', label_dtype=dtype)
        assert lab.dtype == dtype and lab.shape == (2, ih, iw) and torch.equal(lab.long(), scores.argmax(dim=1))
    one = scene_inference(lambda t: t[:, 2:3], x, k, s, batch_size=bs, output='labels', threshold=0.1)
    assert torch.equal(one.bool(), scores[:, 2] > 0.1)


def test_farseg_scene_equals_the_existing_device_function(cuda, farseg):
    """FarSeg-R18 in eval mode on 192 x 160, window 128, stride 64: against `sliding_window_inference` on the device with the
    tolerance of tests/test_inference_api_gpu.py.  Whether the bits were equal too is printed (README, scene section): the
    final division there is aten's."""
    from ever_amd.magic.bigimage import scene_inference, sliding_window_inference
    big = torch.randn(1, 3, 192, 160, generator=torch.Generator().manual_seed(9)).to(cuda)
    ref = sliding_window_inference(farseg, big, kernel_size=128, stride=64, batch_size=3)
    got = scene_inference(farseg, big, kernel_size=128, stride=64, batch_size=3)
    assert got.shape == ref.shape == (1, 1, 192, 160)
    diff = float((got - ref).abs().max())
    print(f'\nscene_inference vs sliding_window_inference, FarSeg-R18 192x160 k128 s64: max |diff| {diff:.3e}, '
          f'bits equal: {torch.equal(got, ref)}')
    assert torch.allclose(got, ref, atol=1e-5)
    lab = scene_inference(farseg, big, kernel_size=128, stride=64, batch_size=3, output='labels', threshold=0.0)
    assert lab.dtype == torch.uint8 and torch.equal(lab.bool(), got[:, 0] > 0.0)
    with pytest.raises(ValueError, match='output stride'):
        scene_inference(lambda t: farseg(t)[:, :, ::2, ::2], big, kernel_size=128, stride=64)


def test_scene_inference_composes_with_tta(cuda, farseg):
    from ever_amd.hip import functional as HF
    from ever_amd.magic.bigimage import scene_inference, sliding_window_inference
    from ever_amd.magic.transform import segm
    from ever_amd.magic.transform.tta import TestTimeAugmentation
    cfg = [segm.Identity(), segm.HorizontalFlip()]
    image = torch.randn(1, 3, 96, 128, generator=torch.Generator().manual_seed(6)).to(cuda)
    before = HF.d4_stats['mean']
    got = scene_inference(TestTimeAugmentation(farseg, cfg), image, kernel_size=64, stride=32)
    assert HF.d4_stats['mean'] > before
    ref = sliding_window_inference(lambda tiles: _reference_expression(farseg, tiles, cfg), image, kernel_size=64, stride=32)
    print(f'\nscene_inference over TestTimeAugmentation: max |diff| {float((got - ref).abs().max()):.3e}, '
          f'bits equal: {torch.equal(got, ref)}')
    assert got.shape == ref.shape and torch.allclose(got, ref, atol=1e-5)


def test_wrappers_refuse_autograd_cpu_tensors_and_mixed_shapes(cuda):
    from ever_amd.hip import functional as HF
    from ever_amd.magic.bigimage import SceneStitcher
    st = SceneStitcher(2, 8, 12, cuda)
    s = torch.ones(1, 2, 4, 4, device=cuda)
    with pytest.raises(HF.HipPathError):
        HF.stitch_add(st.acc, st.count, s.clone().requires_grad_(), [(0, 0)])
    with torch.no_grad():
        HF.stitch_add(st.acc, st.count, s.clone().requires_grad_(), [(0, 0)])         # no-grad: fine
    with pytest.raises(HF.HipPathError):
        HF.stitch_add(st.acc.cpu(), st.count, s, [(0, 0)])
    with pytest.raises(HF.HipPathError):
        HF.stitch_add(st.acc.double(), st.count, s, [(0, 0)])
    with pytest.raises(HF.HipPathError):
        HF.stitch_add(st.acc[:, ::2], torch.zeros(4, 12, device=cuda), s, [(0, 0)])     # not dense
    with pytest.raises(ValueError):
        HF.stitch_add(st.acc, st.count, s, [(0, 0), (1, 1)])
    with pytest.raises(HF.HipPathError):
        HF.stitch_finalize(st.acc.clone().requires_grad_(), st.count)
    with pytest.raises(ValueError):
        HF.stitch_finalize(st.acc, st.count, mode='mean')
    with pytest.raises(ValueError):
        HF.stitch_finalize(st.acc, st.count, out=torch.empty(2, 8, 12, device=cuda))  # the other layout
    assert float(st.count.sum()) == 16 and float(st.acc.sum()) == 32
    q = st.scores()
    assert q.stride() == st.acc.stride() and bool(torch.isnan(q[:, 4:]).all()) and bool((q[:, :4, :4] == 1).all())
    assert bool((st.labels(fill_label=7)[4:] == 7).all())
