"""PyramidPoolModule, PPMHead and PSPNet without a GPU: state-dict keys and shapes against the reference's
(tests/golden/ppm_keys.json, tools/gen_golden_ppm.py), defaults, registration and exports, what construction refuses, and
that PoolBlock(1) is still built from the same children."""
import json
import os

import pytest
import torch

import ever_amd as er
from ever_amd.hip import functional as HF

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _keys(m):
    return {k: list(v.shape) for k, v in m.state_dict().items()}


def test_modules_build_with_reference_keys():
    ref = json.load(open(os.path.join(GOLD, 'ppm_keys.json')))
    ppm = er.module.PyramidPoolModule(2048, 512, 512, (1, 2, 3, 6))
    assert _keys(ppm) == ref['PyramidPoolModule']
    assert list(ppm.state_dict()) == list(ref['PyramidPoolModule'])        # same order as well
    head = er.module.PPMHead(dict())
    assert _keys(head) == ref['PPMHead'] and list(head.state_dict()) == list(ref['PPMHead'])
    assert [n for n, _ in ppm.named_children()] == ['pools', 'conv', 'dropout']
    assert all(isinstance(p, er.module.PoolBlock) for p in ppm.pools)


def test_defaults_and_bottlenecks():
    head = er.module.PPMHead(dict())
    assert dict(head.config.ppm) == dict(in_channels=2048, pool_channels=512, out_channels=512, bins=(1, 2, 3, 6))
    assert head.config.num_classes == 3 and head.config.upsample_scale == 8.0
    ppm, cls, up = head.head
    assert isinstance(ppm, er.module.PyramidPoolModule) and isinstance(up, er.module.UpsamplingBilinear2d)
    assert isinstance(cls, er.module.Conv2d) and cls.out_channels == 3 and cls.kernel_size == (1, 1) and cls.bias is not None
    assert up.scale_factor == 8.0
    assert ppm.conv[0].kernel_size == (3, 3) and ppm.conv[0].padding == (1, 1) and ppm.conv[0].in_channels == 2048 + 4 * 512
    assert isinstance(ppm.dropout, torch.nn.Identity)
    one = er.module.PyramidPoolModule(16, 8, 16, (1, 2), bottleneck_conv='1x1', dropout=0.1)
    assert one.conv[0].kernel_size == (1, 1) and one.conv[0].in_channels == 32 and one.conv[0].bias is None
    assert isinstance(one.dropout, er.module.layers.Dropout2d) and one.dropout.p == 0.1
    none = er.module.PyramidPoolModule(16, 8, 16, (1, 2), bottleneck_conv=None)
    assert isinstance(none.conv, torch.nn.Identity)
    with pytest.raises(AssertionError):
        er.module.PyramidPoolModule(16, 8, 15, (1, 2))                      # out_channels % len(bins), as in the reference


def test_registration_and_exports():
    for name in ('PyramidPoolModule', 'PPMHead', 'PSPNet'):
        assert name in er.module.__all__ and hasattr(er.module, name), name
    assert 'PPMHead' in er.registry.MODEL and 'PSPNet' in er.registry.MODEL
    assert 'PyramidPoolModule' not in er.registry.MODEL                     # unregistered, as in the reference
    m = er.builder.make_model(dict(type='PPMHead', params=dict(num_classes=6)))
    assert isinstance(m, er.module.PPMHead) and m.head[1].out_channels == 6
    for name in ('pyramid_pool', 'pyramid_concat', 'adaptive_avg_pool2d'):
        assert name in HF.__all__ and callable(getattr(HF, name)), name
    net = er.module.PSPNet(dict(encoder=dict(resnet_type='resnet18'),
                                head=dict(ppm=dict(in_channels=512, pool_channels=128, out_channels=128), num_classes=6)))
    assert net.config.encoder.output_stride == 8
    prefixes = {k.split('.')[0] for k in net.state_dict()}
    assert prefixes == {'en', 'head'}
    assert 'head.head.0.pools.3.1.0.weight' in net.state_dict() and 'head.head.1.bias' in net.state_dict()


def test_install_as_ever_exposes_the_names():
    er.install_as_ever()
    import ever
    assert ever.module.PPMHead is er.module.PPMHead and ever.module.PyramidPoolModule is er.module.PyramidPoolModule
    assert ever.module.PSPNet is er.module.PSPNet


def test_construction_refuses_what_the_kernels_do_not_cover():
    for bins in ((1, 2, 3, 6, 8), (9,), (0, 2), (1, 16)):
        with pytest.raises(NotImplementedError):
            er.module.PyramidPoolModule(16, 8, 16 * len(bins), bins)
    from ever_amd.module.ppm import PyramidPoolBlock
    with pytest.raises(NotImplementedError):
        PyramidPoolBlock(9, 16, 8)
    with pytest.raises(NotImplementedError):
        PyramidPoolBlock((2, 3), 16, 8)
    for size in (1, 2, 3, 6, 8, (4, 4)):
        blk = PyramidPoolBlock(size, 16, 8)
        assert isinstance(blk, er.module.PoolBlock)
        assert [type(c) for c in blk] == [er.module.AdaptiveAvgPool2d, er.module.ConvBlock]
        assert list(blk.state_dict()) == list(er.module.PoolBlock(1, 16, 8).state_dict())
    with pytest.raises(NotImplementedError):
        er.module.PoolBlock(2, 16, 8)          # ops.PoolBlock itself is unchanged: ASPP's size-1 block
    x = torch.zeros(1, 4, 4, 4)
    with pytest.raises(NotImplementedError):
        er.module.AdaptiveAvgPool2d(9)(x)
    with pytest.raises(NotImplementedError):
        er.module.AdaptiveAvgPool2d((2, 3))(x)
    with pytest.raises(HF.HipPathError):
        er.module.AdaptiveAvgPool2d(2)(x)                                   # a CPU tensor: no fallback
    with pytest.raises(HF.HipPathError):
        HF.pyramid_pool(x, (1, 2))
    with pytest.raises(NotImplementedError):
        HF.pyramid_pool(x, (1, 2, 3, 4, 5))


def test_pool_block_of_one_keeps_its_children():
    blk = er.module.PoolBlock(1, 32, 16)
    assert list(blk.state_dict()) == ['1.0.weight', '1.1.weight', '1.1.bias', '1.1.running_mean', '1.1.running_var',
                                      '1.1.num_batches_tracked']
    assert type(blk[0]) is er.module.AdaptiveAvgPool2d and blk[0].output_size == 1
    assert type(blk[1]) is er.module.ConvBlock and blk[1][0].kernel_size == (1, 1) and blk[1][0].bias is None
    assert len(blk) == 2
    aspp = er.module.AtrousSpatialPyramidPool(32, 16, (6, 12))
    assert any(type(m) is er.module.PoolBlock for m in aspp.modules())
