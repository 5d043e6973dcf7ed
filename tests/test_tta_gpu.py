"""Test-time augmentation on the device: `tta` and `TestTimeAugmentation` against the reference's own results
(tests/golden/tta_ref.npz, written by tools/gen_golden_tta.py) and against the reference expression
`sum(inv_k(model(T_k(image)))) / n` evaluated with torch ops on the same device.  The symmetries of the square are exact and the
fused mean adds in the reference's order and divides once, so everything but the `Scale` set is compared bit for bit; the `Scale`
set has the yardstick of tests/test_resample_edges_gpu.py."""
import numpy as np
import pytest
import torch

from tests import tta_common as tc
from tests.test_resample_edges_gpu import _as_close_as_aten

pytestmark = pytest.mark.gpu


def _golden():
    return {k: torch.from_numpy(v) for k, v in np.load(tc.GOLDEN).items()}


def _same_bits(got, ref, what):
    got, ref = got.detach().cpu().contiguous(), ref.detach().cpu().contiguous()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    bad = got.view(torch.int32) != ref.view(torch.int32)
    assert not bool(bad.any()), (f'{what}: {int(bad.sum())} of {bad.numel()} elements differ in their bits, first at '
                                 f'{tuple(int(v) for v in bad.nonzero()[0])}: {got[bad][0].item()!r} vs {ref[bad][0].item()!r}')


def _layouts(x):
    return (('nchw', x.contiguous()), ('nhwc', x.contiguous(memory_format=torch.channels_last)))


def _reference_expression(model, image, cfg):
    """the reference's tta with every transform evaluated by torch ops on the image's device, from fresh model calls"""
    from ever_amd.magic.transform import segm
    with torch.no_grad():
        outs = []
        for t in cfg:
            if type(t) in (segm.Identity, segm.Rotate90k, segm.HorizontalFlip, segm.VerticalFlip, segm.Transpose):
                o = model(segm.d4_torch(image, t.d4_op).contiguous())
                outs.append(segm.d4_torch(o, tc.INVERSE[t.d4_op]))
            else:
                outs.append(t.inv_transform(model(t.transform(image))))
        return sum(outs) / len(outs)


@pytest.mark.parametrize('name', ['d4', 'no_transpose'])
def test_toy_model_equals_the_reference_fixture_bit_for_bit(cuda, name):
    import ever_amd as er
    from ever_amd.hip import functional as HF
    from ever_amd.magic.transform import segm
    from ever_amd.magic.transform.tta import TestTimeAugmentation, tta
    g = _golden()
    cfg = tc.fixture_sets(segm, er.Transform)[name]
    for layout, x in _layouts(g['input'].to(cuda)):
        for t, im in zip(cfg, er.MultiTransform(*cfg).transform(x)):
            want = g['input'] if type(t).__name__ == 'Identity' else g['in_' + tc.transform_label(t)]
            _same_bits(im, want, f'{name} {layout} {tc.transform_label(t)}')
        before = HF.d4_stats['mean']
        _same_bits(tta(tc.toy_model, x, cfg), g[name], f'tta {name} {layout}')
        _same_bits(TestTimeAugmentation(tc.toy_model, cfg)(x), g[name], f'TestTimeAugmentation {name} {layout}')
        assert HF.d4_stats['mean'] == before + 2, 'the fused mean was not taken'


def test_scale_set_is_as_close_to_fp64_as_aten(cuda):
    """Against the reference expression in fp64 (this package's CPU path on a double input: the same aten calls), the device
    result may err at most twice as much as the reference's own fp32 result plus 4 ulp of the largest |reference|."""
    import ever_amd as er
    from ever_amd.hip import functional as HF
    from ever_amd.magic.transform import segm
    from ever_amd.magic.transform.tta import tta
    g = _golden()
    sets = tc.fixture_sets(segm, er.Transform)
    ref64 = tta(tc.toy_model, g['input'].double(), sets['scale'])
    assert ref64.dtype == torch.float64
    for layout, x in _layouts(g['input'].to(cuda)):
        cfg = tc.fixture_sets(segm, er.Transform)['scale']
        ims = er.MultiTransform(*cfg).transform(x)
        for t, im in zip(cfg, ims):
            if isinstance(t, segm.Scale):
                want = g['in_' + tc.transform_label(t)]
                want64 = t.transform(g['input'].double())
                _as_close_as_aten(im.cpu(), want64, want, f'scale {layout} {tc.transform_label(t)}')
        before = HF.d4_stats['mean']
        got = tta(tc.toy_model, x, cfg)
        assert HF.d4_stats['mean'] == before + 1, 'the fused mean was not taken'
        _as_close_as_aten(got.cpu(), ref64, g['scale'], f'tta scale {layout}')


def _farseg_r18(cuda):
    import ever_amd as er
    torch.manual_seed(11)
    m = er.module.FarSeg(dict(encoder=dict(resnet_type='resnet18', in_channels=3),
                              head=dict(fpn=dict(in_channels_list=(64, 128, 256, 512), out_channels=256),
                                        fs_relation=dict(scene_embedding_channels=512))))
    for mod in m.modules():     # (an eval-mode BatchNorm with the initial 0 / 1 statistics would be a weak model)
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.normal_(0, 0.2)
            mod.running_var.uniform_(0.5, 1.5)
    return m.to(cuda).eval()


@pytest.fixture(scope='module')
def farseg(cuda):
    return _farseg_r18(cuda)


def test_model_tta_equals_the_reference_expression_on_the_device(cuda, farseg):
    import ever_amd as er
    from ever_amd.hip import functional as HF
    from ever_amd.magic.transform import segm
    from ever_amd.magic.transform.tta import TestTimeAugmentation, tta
    cfg = tc.fixture_sets(segm, er.Transform)['d4']
    assert len(cfg) == 8
    image = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(5)).to(cuda)
    for layout, x in _layouts(image):
        ref = _reference_expression(farseg, x, cfg)
        before = dict(HF.d4_stats)
        got = tta(farseg, x, cfg)
        assert HF.d4_stats['mean'] == before['mean'] + 1 and HF.d4_stats['mean_terms'] == before['mean_terms'] + 8
        assert HF.d4_stats['apply'] >= before['apply'] + 6          # the transformed images came from the copy kernel
        assert got.shape == ref.shape == (2, 1, 64, 96)
        _same_bits(got, ref, f'tta FarSeg-R18 {layout}')
        _same_bits(TestTimeAugmentation(farseg, cfg)(x), ref, f'TestTimeAugmentation FarSeg-R18 {layout}')


def test_sliding_window_inference_composes_with_tta(cuda, farseg):
    from ever_amd.hip import functional as HF
    from ever_amd.magic.bigimage import sliding_window_inference
    from ever_amd.magic.transform import segm
    from ever_amd.magic.transform.tta import TestTimeAugmentation
    cfg = [segm.Identity(), segm.HorizontalFlip()]
    image = torch.randn(1, 3, 96, 128, generator=torch.Generator().manual_seed(6)).to(cuda)
    before = HF.d4_stats['mean']
    got = sliding_window_inference(TestTimeAugmentation(farseg, cfg), image, kernel_size=64, stride=32)
    assert HF.d4_stats['mean'] > before
    ref = sliding_window_inference(lambda tiles: _reference_expression(farseg, tiles, cfg), image, kernel_size=64, stride=32)
    _same_bits(got, ref, 'sliding window over TestTimeAugmentation')


def test_user_defined_transform_takes_the_plain_path(cuda):
    """a Transform subclass the fused mean does not know is inverted by its own inv_transform and enters with op 0"""
    import ever_amd as er
    from ever_amd.hip import functional as HF
    from ever_amd.magic.transform import segm
    from ever_amd.magic.transform.tta import tta

    class Roll(er.Transform):
        def transform(self, inputs):
            return torch.roll(inputs, 3, 3)

        def inv_transform(self, transformed_inputs):
            return torch.roll(transformed_inputs, -3, 3)

    class MyFlip(segm.HorizontalFlip):          # a subclass may change anything: not fused either
        def inv_transform(self, transformed_inputs):
            return torch.flip(transformed_inputs, [3]) * 2

    cfg = [segm.Rotate90k(1), Roll(), MyFlip(), segm.VerticalFlip()]
    x = torch.randn(2, 3, 12, 20, generator=torch.Generator().manual_seed(8)).to(cuda)
    before = HF.d4_stats['mean']
    got = tta(tc.toy_model, x, cfg)
    assert HF.d4_stats['mean'] == before + 1
    with torch.no_grad():
        outs = [torch.rot90(tc.toy_model(torch.rot90(x, 1, [2, 3])), 3, [2, 3]),
                torch.roll(tc.toy_model(torch.roll(x, 3, 3)), -3, 3),
                torch.flip(tc.toy_model(torch.flip(x, [3])), [3]) * 2,
                torch.flip(tc.toy_model(torch.flip(x, [2])), [2])]
        ref = sum(outs) / len(outs)
    _same_bits(got, ref, 'user-defined transform')
