"""DeepLabv3+ / ASPP modules and the depthwise C-ABI, host side (no GPU): the modules build with the reference's
state-dict names and shapes (tests/golden/deeplab_keys.json, written from the imported reference by
tools/gen_golden_deeplab.py), the head is registered, a stock depthwise convolution retargets onto `Conv2d`, and the new
entry points check their arguments before any launch."""
import ctypes
import json
import os

import pytest
import torch

import ever_amd as er
from ever_amd import _C

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _keys(m):
    return {k: list(v.shape) for k, v in m.state_dict().items()}


def test_modules_build_with_reference_keys():
    ref = json.load(open(os.path.join(GOLD, 'deeplab_keys.json')))
    head = er.module.Deeplabv3pHead(dict())
    assert _keys(head) == ref['Deeplabv3pHead']
    assert list(head.state_dict()) == list(ref['Deeplabv3pHead'])          # same order as well
    assert _keys(er.module.ASPPHead(dict())) == ref['ASPPHead']
    blk = er.module.SeparableConvBlock(304, 256, 3, 1, 1)
    assert list(_keys(blk)) == ['0.0.weight', '0.2.weight', '1.weight', '1.bias', '1.running_mean', '1.running_var',
                                '1.num_batches_tracked']
    assert blk[0][0].groups == 304 and blk[0][0].weight.shape == (304, 1, 3, 3) and blk[0][2].bias is None
    dw = er.module.DepthwiseConv2d(32, 32, 5, 2, 2)
    assert dw.groups == 32 and dw.bias is not None and isinstance(dw, er.module.Conv2d)
    with pytest.raises(AssertionError):
        er.module.DepthwiseConv2d(32, 64, 3)
    with pytest.raises(NotImplementedError):
        er.module.PoolBlock(2, 64, 64)         # pyramid pooling (PPM) is not implemented
    for name in ('DepthwiseConv2d', 'SeparableConv2d', 'SeparableConvBlock', 'PoolBlock', 'AtrousSpatialPyramidPool',
                 'ASPPHead', 'Deeplabv3pDecoder', 'Deeplabv3pHead', 'DeepLabV3Plus'):
        assert name in er.module.__all__ and hasattr(er.module, name), name


def test_registry_and_builder():
    assert 'Deeplabv3pHead' in er.registry.MODEL and 'DeepLabV3Plus' in er.registry.MODEL
    assert 'ASPPHead' not in er.registry.MODEL           # unregistered, as in the reference
    m = er.builder.make_model(dict(type='Deeplabv3pHead', params=dict(num_classes=6)))
    assert isinstance(m, er.module.Deeplabv3pHead) and m.head[1].out_channels == 6
    net = er.module.DeepLabV3Plus(dict(encoder=dict(resnet_type='resnet18'),
                                       head=dict(deeplabv3p_decoder=dict(os4_feature_channels=64, os16_feature_channels=512),
                                                 num_classes=6)))
    sd = net.state_dict()
    assert all(k.startswith(('en.', 'head.')) for k in sd)
    assert sd['head.head.0.stack_conv3x3.0.0.0.weight'].shape == (304, 1, 3, 3)
    assert net.en.resnet.layer4[0].conv2.dilation == (2, 2)          # output stride 16


def test_to_hip_maps_a_depthwise_convolution():
    net = er.module.to_hip(torch.nn.Sequential(torch.nn.Conv2d(16, 16, 3, groups=16)))
    assert isinstance(net[0], er.module.Conv2d) and net[0].groups == 16
    from ever_amd.hip import functional as HF
    assert HF.depthwise_in_scope(16, 16, 16, 3, 1) and HF.depthwise_in_scope(304, 304, 304, (1, 3), (2, 1), 6)
    # out of scope: ResNeXt groups, channel multiplier 2, C % 4, stride 3, kernel 9
    assert not HF.depthwise_in_scope(128, 128, 32, 3, 1)
    assert not HF.depthwise_in_scope(16, 32, 16, 3, 1)
    assert not HF.depthwise_in_scope(6, 6, 6, 3, 1)
    assert not HF.depthwise_in_scope(16, 16, 16, 3, 3)
    assert not HF.depthwise_in_scope(16, 16, 16, 9, 1)
    assert all(hasattr(HF, n) for n in HF.__all__) and 'depthwise_conv2d' in HF.__all__


def test_depthwise_entry_points_check_before_launch():
    lib = _C.load()
    ok = _C.ConvDesc(2, 16, 16, 32, 16, 16, 32, 3, 3, 1, 1, 1, 1, 1, 1)
    assert lib.evk_depthwise_bwd_workspace_bytes(ctypes.byref(ok)) > 0        # host only
    bad = [
        (_C.ConvDesc(2, 16, 16, 32, 16, 16, 64, 3, 3, 1, 1, 1, 1, 1, 1), b'Cin'),            # multiplier 2
        (_C.ConvDesc(2, 16, 16, 6, 16, 16, 6, 3, 3, 1, 1, 1, 1, 1, 1), b'multiple of 4'),   # C % 4
        (_C.ConvDesc(2, 16, 16, 32, 6, 6, 32, 3, 3, 3, 3, 1, 1, 1, 1), b'stride'),          # stride 3
        (_C.ConvDesc(2, 16, 16, 32, 16, 16, 32, 9, 9, 1, 1, 4, 4, 1, 1), b'kernel'),        # 9x9
    ]
    for d, msg in bad:
        assert lib.evk_depthwise_fwd(ctypes.byref(d), 1, 1, None, 1, 0, None) == -2
        assert msg in lib.evk_last_error()
        assert lib.evk_depthwise_bwd(ctypes.byref(d), 1, 1, None, 1, 1, 1, None, 1, 1 << 20, None) == -2
        assert lib.evk_depthwise_bwd_workspace_bytes(ctypes.byref(d)) == 0
    # an output size that does not follow from the geometry, a null pointer, a short workspace
    d = _C.ConvDesc(2, 16, 16, 32, 15, 16, 32, 3, 3, 1, 1, 1, 1, 1, 1)
    assert lib.evk_depthwise_fwd(ctypes.byref(d), 1, 1, None, 1, 0, None) == -1
    assert lib.evk_depthwise_fwd(ctypes.byref(ok), None, 1, None, 1, 0, None) == -1
    assert lib.evk_depthwise_bwd(ctypes.byref(ok), 1, 1, None, 1, 1, 1, None, 1, 16, None) == -4
    assert b'workspace' in lib.evk_last_error()
    assert lib.evk_broadcast_hw(None, 1, 1, 4, 4, None) == -1 and lib.evk_sum_hw(1, 1, 1, 4, 6, None) == -1


def test_batchnorm_refuses_one_value_per_channel_in_training():
    bn = er.module.BatchNorm2d(8).train()
    with pytest.raises(ValueError, match='more than 1 value per channel'):
        bn(torch.zeros(1, 8, 1, 1))
