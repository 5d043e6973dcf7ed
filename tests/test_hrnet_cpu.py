"""HRNetV2 modules and the exchange / slice C-ABI, host side (no GPU): every encoder type and the head build with the
reference's state-dict names, shapes and ORDER (tests/golden/hrnet_keys.json, written from the imported reference by
tools/gen_golden_hrnet.py), the registry and builder know them, hrnetv2_w18 builds and refuses to run, and the new entry
points check their arguments before any launch."""
import ctypes
import hashlib
import itertools
import json
import os

import pytest
import torch

import ever_amd as er
from ever_amd import _C

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TYPES = ('hrnetv2_w18', 'hrnetv2_w32', 'hrnetv2_w40', 'hrnetv2_w48')


def _ordered(m):
    return [[k, list(v.shape)] for k, v in m.state_dict().items()]


def _key_groups(state_dict):
    """tools/gen_golden_hrnet.py: key_groups — per run of entries sharing their first three name components, the count and the
    sha256 of the "name shape" lines: names, shapes and order"""
    rows = [(k, f'{k} {tuple(v.shape)}') for k, v in state_dict.items()]
    return [[g, len(lines), hashlib.sha256('\n'.join(lines).encode()).hexdigest()[:16]]
            for g, lines in ((g, [r[1] for r in it]) for g, it in itertools.groupby(rows, lambda r: '.'.join(r[0].split('.')[:3])))]


@pytest.mark.parametrize('hrnet_type', TYPES)
def test_encoder_builds_with_reference_keys_in_reference_order(hrnet_type):
    ref = json.load(open(os.path.join(GOLD, 'hrnet_keys.json')))
    en = er.module.HRNetEncoder(dict(hrnet_type=hrnet_type))
    got = _key_groups(en.state_dict())
    assert [g[:2] for g in got] == [g[:2] for g in ref[hrnet_type]]           # sub-modules, their order and entry counts
    assert got == ref[hrnet_type], [a[0] for a, b in zip(got, ref[hrnet_type]) if a != b]
    c = int(hrnet_type[-2:])
    assert en.output_channels() == (c, 2 * c, 4 * c, 8 * c)
    # this package's layers throughout
    assert isinstance(en.hrnet.conv1, er.module.Conv2d) and isinstance(en.hrnet.bn1, er.module.BatchNorm2d)
    assert en.hrnet.bn1.momentum == 0.1
    mod = en.hrnet.stage4[0]
    assert isinstance(mod, er.module.HighResolutionModule) and isinstance(mod.fuse_layers[0][3], er.module.HipSequential)
    assert en.stage4 is en.hrnet.stage4 and en.stage2 is en.hrnet.stage2


def test_head_builds_with_reference_keys_in_reference_order():
    ref = json.load(open(os.path.join(GOLD, 'hrnet_keys.json')))
    head = er.module.HRNetHead(dict())
    assert _ordered(head) == ref['HRNetHead']
    assert head.head[0].fuse_conv[0].bias is not None and head.head[1].out_channels == 3
    assert head.head[2].scale_factor == 4.0


def test_registry_builder_and_composition():
    for name in TYPES + ('HRNetEncoder', 'HRNetHead', 'HRNetSeg'):
        assert name in er.registry.MODEL, name
    for name in ('HighResolutionModule', 'HighResolutionNet', 'HRNetEncoder', 'SimpleFusion', 'HRNetHead', 'HRNetSeg'):
        assert name in er.module.__all__ and hasattr(er.module, name), name
    head = er.builder.make_model(dict(type='HRNetHead', params=dict(num_classes=6)))
    assert isinstance(head, er.module.HRNetHead) and head.head[1].out_channels == 6
    net = er.builder.make_model(dict(type='HRNetSeg', params=dict(encoder=dict(hrnet_type='hrnetv2_w32'),
                                                                 head=dict(num_classes=6))))
    sd = net.state_dict()
    assert all(k.startswith(('en.', 'head.')) for k in sd)
    # the head's width defaults to the sum of the encoder's output channels
    assert sd['head.head.0.fuse_conv.0.weight'].shape == (480, 480, 1, 1) and sd['head.head.1.weight'].shape == (6, 480, 1, 1)
    assert sd['en.hrnet.stage4.2.fuse_layers.3.0.2.0.weight'].shape == (256, 32, 3, 3)


def test_reset_in_channels_replaces_the_first_convolution():
    en = er.module.HRNetEncoder(dict(hrnet_type='hrnetv2_w32'))
    keys = list(en.state_dict())
    old = en.hrnet.conv1
    en.reset_in_channels(3)
    assert en.hrnet.conv1 is old
    en.reset_in_channels(4)
    assert en.hrnet.conv1 is not old and isinstance(en.hrnet.conv1, er.module.Conv2d)
    assert en.hrnet.conv1.weight.shape == (64, 4, 3, 3) and list(en.state_dict()) == keys


def test_plugins_without_kernels_raise():
    en = er.module.HRNetEncoder(dict(hrnet_type='hrnetv2_w32'))
    with pytest.raises(NotImplementedError, match='context'):
        en.with_context_block(1 / 16.)
    with pytest.raises(NotImplementedError, match='squeeze'):
        en.with_squeeze_excitation(16)


def test_w18_builds_and_its_forward_names_the_channel_rule():
    en = er.module.HRNetEncoder(dict(hrnet_type='hrnetv2_w18'))
    x = torch.zeros(1, 3, 64, 64)                     # a CPU tensor: the rule is named before the device is looked at
    with pytest.raises(NotImplementedError, match='multiples of 4'):
        en(x)
    with pytest.raises(NotImplementedError, match='18 channels'):
        en.hrnet(x)
    # a type that can run refuses the CPU tensor instead
    with pytest.raises(er.hip.functional.HipPathError):
        er.module.HRNetEncoder(dict(hrnet_type='hrnetv2_w32'))(x)


def test_pretrained_needs_a_local_weight_path(tmp_path):
    with pytest.raises(ValueError, match='weight_path'):
        er.registry.MODEL['hrnetv2_w32'](pretrained=True)
    src = er.registry.MODEL['hrnetv2_w32']()
    path = str(tmp_path / 'w32.pth')
    torch.save(src.state_dict(), path)
    dst = er.registry.MODEL['hrnetv2_w32'](pretrained=True, weight_path=path)
    assert all(torch.equal(a, b) for a, b in zip(src.state_dict().values(), dst.state_dict().values()))


def test_norm_eval_and_frozen_stages_follow_the_reference():
    net = er.registry.MODEL['hrnetv2_w32'](norm_eval=True, frozen_stages=1).train()
    assert not any(m.training for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d))
    assert net.stage2.training
    assert not any(p.requires_grad for m in (net.conv1, net.bn1, net.conv2, net.bn2, net.layer1) for p in m.parameters())
    assert all(p.requires_grad for p in net.stage2.parameters())


def test_hr_fuse_entry_points_check_before_launch():
    lib = _C.load()
    P, I = ctypes.c_void_p, ctypes.c_int32

    def fwd(nterms=2, shifts=(0, 1), terms=(16, 16), n=1, h=8, w=8, c=8, y=16, bits=16):
        k = max(len(shifts), 1)
        return lib.evk_hr_fuse_fwd((P * k)(*terms[:k]), (I * k)(*shifts), (P * k)(), nterms, y, bits, None, n, h, w, c, None)

    # (the pointers are never dereferenced: every call below returns before a launch)
    assert fwd(y=None) == -1 and fwd(bits=None) == -1 and fwd(h=0) == -1
    assert fwd(terms=(16, None)) == -1 and b'term 1' in lib.evk_last_error()
    assert lib.evk_hr_fuse_fwd(None, None, None, 1, 16, 16, None, 1, 8, 8, 8, None) == -1
    assert fwd(c=6) == -2 and b'multiple of 4' in lib.evk_last_error()
    assert fwd(nterms=0) == -2 and b'terms' in lib.evk_last_error()
    assert fwd(nterms=5) == -2 and b'terms' in lib.evk_last_error()
    assert fwd(shifts=(0, 4)) == -2 and b'shift 4' in lib.evk_last_error()
    assert fwd(shifts=(0, 2), h=6) == -2 and b'multiples of 4' in lib.evk_last_error()
    assert fwd(shifts=(0, 1), w=7) == -2 and b'multiples of 2' in lib.evk_last_error()
    assert fwd(n=1 << 15, h=1 << 10, w=1 << 10, c=4) == -2 and b'2^31' in lib.evk_last_error()

    def bwd(dy=16, bits=16, dm=16, p1=None, p2=None, p3=None, n=1, h=8, w=8, c=8):
        return lib.evk_hr_fuse_bwd(dy, bits, dm, p1, p2, p3, n, h, w, c, None)

    assert bwd(dy=None) == -1 and bwd(bits=None) == -1 and bwd(dm=None) == -1 and bwd(c=0) == -1
    assert bwd(c=10) == -2 and b'multiple of 4' in lib.evk_last_error()
    assert bwd(p3=16, h=12) == -2 and b'multiples of 8' in lib.evk_last_error()
    assert bwd(dm=None, p1=16, w=5) == -2 and b'multiples of 2' in lib.evk_last_error()


def test_bilinear_slice_entry_points_check_before_launch():
    lib = _C.load()
    for fn in (lib.evk_upsample_bilinear_slice_fwd, lib.evk_upsample_bilinear_slice_bwd):
        assert fn(None, 16, 1, 4, 4, 8, 8, 8, 0, 8, None) == -1
        assert fn(16, None, 1, 4, 4, 8, 8, 8, 0, 8, None) == -1
        assert fn(16, 16, 1, 4, 4, 8, 8, 8, 4, 8, None) == -1 and b'c0 + C <= Ctot' in lib.evk_last_error()
        assert fn(16, 16, 1, 4, 4, 8, 8, 8, -4, 16, None) == -1
        assert fn(16, 16, 1, 4, 4, 0, 8, 8, 0, 8, None) == -1


def test_functional_facade_exports_the_new_calls():
    from ever_amd.hip import functional as HF
    assert 'hr_fuse' in HF.__all__ and 'bilinear_concat' in HF.__all__ and all(hasattr(HF, n) for n in HF.__all__)
    with pytest.raises(ValueError, match='1 to 4 terms'):
        HF.hr_fuse([])
    with pytest.raises(HF.HipPathError):
        HF.hr_fuse([(torch.zeros(1, 4, 2, 2), 0, None)])
