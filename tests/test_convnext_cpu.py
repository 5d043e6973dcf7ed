"""ConvNeXt without a GPU: state-dict layout against the reference's (tests/golden/convnext_keys.json, written by
tools/gen_golden_convnext.py), strict loading, the refusals, the registry entry and the LayerNorm swap of to_hip."""
import json
import os

import pytest
import torch

import ever_amd as er
from ever_amd.module.dinov3 import ConvNeXt, convnext_sizes, get_convnext_arch
from tests import convnext_common as cc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def ref_keys():
    with open(os.path.join(GOLDEN, 'convnext_keys.json')) as f:
        return json.load(f)


@pytest.mark.parametrize('size', cc.SIZES)
def test_state_dict_keys_and_shapes_equal_the_reference(ref_keys, size):
    sd = get_convnext_arch('convnext_' + size)().state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == ref_keys['convnext_' + size]
    assert convnext_sizes[size]['dims'][0] * 4 == sd['stages.0.0.pwconv1.weight'].shape[0]


def test_reference_format_state_dict_loads_strictly(ref_keys):
    state = {k: torch.full(shape, 0.25) for k, shape in ref_keys['convnext_tiny']}
    model = get_convnext_arch('convnext_tiny')()
    res = model.load_state_dict(state, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert model.stages[2][1].pwconv1.weight.shape == (4 * 384, 384) and model.stages[2][1].pwconv1.weight.dim() == 2
    assert model.downsample_layers[0][0].weight.flatten()[3].item() == 0.25 and model.stages[0][0].gamma[0].item() == 0.25


def test_constructor_defaults_follow_the_reference():
    m = ConvNeXt()
    assert [len(s) for s in m.stages] == [3, 3, 9, 3] and m.embed_dims == [96, 192, 384, 768] and m.embed_dim == 768
    assert m.patch_size is None and m.n_storage_tokens == 0 and m.n_blocks == 4 and m.input_pad_size == 4
    assert m.stages[0][0].gamma[0].item() == pytest.approx(1e-6) and m.norms[3] is m.norm
    assert ConvNeXt(layer_scale_init_value=0, depths=[1, 1, 1, 1]).stages[0][0].gamma is None
    rates = [getattr(b.drop_path, 'drop_prob', 0.0) for s in ConvNeXt(drop_path_rate=0.3).stages for b in s]
    assert rates[0] == 0.0 and rates[-1] == pytest.approx(0.3) and rates == sorted(rates)


def test_unknown_size_raises_not_implemented():
    with pytest.raises(NotImplementedError):
        get_convnext_arch('convnext_huge')


def test_patch_size_raises_on_use():
    m = ConvNeXt(patch_size=16, **cc.REDUCED)           # building is fine
    with pytest.raises(NotImplementedError, match='patch_size'):
        m.get_intermediate_layers(torch.zeros(1, 3, 64, 64), n=1)


def test_encoder_is_registered_and_builds_from_a_config():
    assert er.registry.MODEL['ConvNeXtEncoder'] is er.module.ConvNeXtEncoder
    enc = er.module.ConvNeXtEncoder(dict(convnext_type='convnext_base', drop_path_rate=0.1, frozen_stages=1))
    assert enc.output_channels() == (128, 256, 512, 1024) and enc.config.in_channels == 3
    assert enc.config.layer_scale_init_value == 1e-6 and enc.config.pretrained is False and enc.config.weight_path is None
    assert not any(p.requires_grad for p in enc.convnext.downsample_layers[0].parameters())
    assert not any(p.requires_grad for p in enc.convnext.stages[0].parameters())
    assert all(p.requires_grad for p in enc.convnext.stages[1].parameters())
    with pytest.raises(ValueError, match='weight_path'):
        er.module.ConvNeXtEncoder(dict(pretrained=True))
    with pytest.raises(NotImplementedError):
        er.module.ConvNeXtEncoder(dict(convnext_type='convnext_nano'))


def test_encoder_loads_a_local_weight_file(tmp_path):
    src = get_convnext_arch('convnext_tiny')()
    path = str(tmp_path / 'w.pt')
    torch.save(src.state_dict(), path)
    enc = er.module.ConvNeXtEncoder(dict(pretrained=True, weight_path=path))
    assert torch.equal(enc.convnext.stages[1][0].pwconv2.weight, src.stages[1][0].pwconv2.weight)


def test_names_are_exported_and_aliased():
    import sys
    for name in ('DropPath', 'Block', 'LayerNorm', 'ConvNeXt', 'convnext_sizes', 'get_convnext_arch'):
        assert hasattr(er.module.dinov3, name)
    er.install_as_ever()
    assert sys.modules['ever.module.dinov3'] is er.module.dinov3


def test_to_hip_swaps_layer_norm_and_refuses_cpu_and_multi_axis():
    from ever_amd.hip.functional import HipPathError
    net = torch.nn.Sequential(torch.nn.LayerNorm(8), torch.nn.LayerNorm((4, 8)))
    keys = list(net.state_dict())
    er.module.to_hip(net)
    assert type(net[0]) is er.module.LayerNorm and isinstance(net[0], torch.nn.LayerNorm) and list(net.state_dict()) == keys
    with pytest.raises(HipPathError):
        net[0](torch.zeros(2, 8))                        # no CPU fallback
    with pytest.raises(NotImplementedError):
        net[1](torch.zeros(2, 4, 8))
