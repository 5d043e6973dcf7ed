"""The DINOv3 ViT without a GPU: state-dict layout against the reference's (tests/golden/vit_keys.json, written by
tools/gen_golden_vit.py), strict loading, the RoPE tables bit for bit against the reference's CPU values, what is refused, the
ViTEncoder configuration and the registry entry."""
import json
import os

import numpy as np
import pytest
import torch

import ever_amd as er
from ever_amd.hip.functional import HipPathError
from ever_amd.module import dinov3
from tests import vit_common as vc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def ref_keys():
    with open(os.path.join(GOLDEN, 'vit_keys.json')) as f:
        return json.load(f)


@pytest.mark.parametrize('size', vc.SIZES)
def test_state_dict_keys_and_shapes_match_the_reference(ref_keys, size):
    with torch.device('meta'):
        sd = getattr(dinov3, size)().state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == ref_keys[size]
    if size == 'vitl16_sat493m':
        assert len(sd) == 370
        for k in ('rope_embed.periods', 'blocks.23.attn.qkv.bias_mask', 'local_cls_norm.weight', 'storage_tokens', 'mask_token'):
            assert k in sd


def test_reference_shaped_state_dict_loads_strictly(ref_keys, tmp_path):
    state = {k: torch.full(shape, 0.25) for k, shape in ref_keys['vit_small']}
    model = dinov3.vit_small()
    res = model.load_state_dict(state, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert float(model.blocks[11].mlp.fc2.weight.detach().min()) == 0.25 and model.blocks[0].attn.qkv.weight.dim() == 2
    with pytest.raises(RuntimeError):
        model.load_state_dict({k: v for k, v in state.items() if k != 'mask_token'}, strict=True)
    # the released constructor loads a local file strictly; two of its 24 blocks keep the file at a few MB (the caller's
    # keyword wins over the named size, and the full 370-key layout is checked under meta above)
    small = {k: torch.full(shape, 0.5) for k, shape in ref_keys['vitl16_sat493m']
             if not k.startswith('blocks.') or int(k.split('.')[1]) < 2}
    path = str(tmp_path / 'vitl.pth')
    torch.save(small, path)
    m = dinov3.vitl16_sat493m(pretrained=path, depth=2)
    assert float(m.blocks[1].attn.qkv.bias_mask[0]) == 0.5 and m.rope_embed.periods.dtype == torch.float32
    assert float(m.local_cls_norm.weight.detach()[0]) == 0.5 and tuple(m.storage_tokens.shape) == (1, 4, 1024)
    torch.save({k: v for k, v in small.items() if k != 'storage_tokens'}, path)
    with pytest.raises(RuntimeError):
        dinov3.vitl16_sat493m(pretrained=path, depth=2)


def test_fresh_masked_bias_is_nan_as_in_the_reference():
    m = dinov3.DinoVisionTransformer(embed_dim=64, depth=1, num_heads=2, mask_k_bias=True)
    assert bool(torch.isnan(m.blocks[0].attn.qkv.bias_mask).all())
    assert m.rope_embed.periods.dtype == torch.bfloat16          # the constructor's default dtype is kept


@pytest.mark.parametrize('name', list(vc.ROPE_TABLES))
def test_rope_tables_equal_the_reference_bit_for_bit(name):
    gold = np.load(os.path.join(GOLDEN, 'vit_ref.npz'))
    sin, cos = vc.rope_table(dinov3.RopePositionEmbedding, name)
    for got, key in ((sin, 'sin'), (cos, 'cos')):
        ref = gold[f'rope/{name}/{key}']
        assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape
        assert np.array_equal(got.numpy().view(np.int32), ref.view(np.int32)), (name, key)
    if name.startswith('train'):
        again = vc.rope_table(dinov3.RopePositionEmbedding, name)
        assert torch.equal(again[0], sin) and torch.equal(again[1], cos)          # the same seed, the same tables


def test_rope_constructor_refusals():
    with pytest.raises(ValueError):
        dinov3.RopePositionEmbedding(64, num_heads=2, base=None)
    with pytest.raises(ValueError):
        dinov3.RopePositionEmbedding(64, num_heads=2, base=100.0, min_period=1.0, max_period=10.0)
    with pytest.raises(AssertionError):
        dinov3.RopePositionEmbedding(60, num_heads=2)
    m = dinov3.RopePositionEmbedding(64, num_heads=2, base=None, min_period=1.0, max_period=10.0, dtype=torch.float32)
    assert tuple(m(H=2, W=3)[0].shape) == (6, 32)


def test_out_of_scope_configurations_raise():
    V = dinov3.DinoVisionTransformer
    small = dict(embed_dim=64, depth=1, num_heads=2)
    with pytest.raises(NotImplementedError, match='rmsnorm'):
        V(norm_layer='rmsnorm', **small)
    for ffn in ('swiglu', 'swiglu32', 'swiglu64', 'swiglu128'):
        with pytest.raises(NotImplementedError, match='swiglu'):
            V(ffn_layer=ffn, **small)
    x = torch.zeros(1, 3, 32, 32)
    with pytest.raises(NotImplementedError, match='masks'):
        V(**small).prepare_tokens_with_masks(x, masks=torch.zeros(1, 4, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match='pos_embed_rope_dtype'):
        V(**small)._rope_source((2, 2))                      # the constructor's default is bf16
    with pytest.raises(NotImplementedError, match='drop_path_rate'):
        V(drop_path_rate=0.1, pos_embed_rope_dtype='fp32', **small).train().blocks[0](torch.zeros(1, 5, 64), None)
    with pytest.raises(NotImplementedError):
        dinov3.SelfAttention(64, num_heads=2, attn_drop=0.1)
    with pytest.raises(NotImplementedError):
        dinov3.SelfAttention(64, num_heads=2).compute_attention(torch.zeros(1, 5, 192), attn_bias=torch.zeros(1))
    for name in ('CausalSelfAttention', 'vit_7b', 'vit7b16_sat493m', 'RMSNorm', 'SwiGLUFFN', 'DINOHead'):
        assert not hasattr(dinov3, name)


def test_cpu_tensors_raise_hip_path_error():
    from ever_amd.hip import functional as HF
    with pytest.raises(HipPathError):
        HF.attention(torch.zeros(1, 5, 192), 2)
    with pytest.raises(HipPathError):
        HF.prepend_tokens(torch.zeros(1, 4, 8), torch.zeros(1, 8))
    with pytest.raises(HipPathError):
        dinov3.DinoVisionTransformer(embed_dim=64, depth=1, num_heads=2, pos_embed_rope_dtype='fp32')(torch.zeros(1, 3, 32, 32))


def test_encoder_config_defaults_output_channels_and_registry():
    from ever_amd.core import registry
    assert registry.MODEL['ViTEncoder'] is er.module.ViTEncoder
    enc = er.module.ViTEncoder(dict(vit_type='vit_base', frozen_blocks=2))
    cfg = enc.config
    assert (cfg.in_channels, cfg.out_indices, cfg.pyramid, cfg.pretrained, cfg.weight_path) == (3, None, True, False, None)
    assert dict(cfg.vit_kwargs) == {} and enc.vit.pos_embed_rope_dtype == 'fp32'
    assert enc.out_indices == [2, 5, 8, 11] and enc.output_channels() == (768,) * 4
    assert not any(p.requires_grad for p in enc.vit.blocks[1].parameters()) and not enc.vit.cls_token.requires_grad
    assert all(p.requires_grad for p in enc.vit.blocks[2].parameters())
    assert not enc.train().vit.blocks[0].training and enc.vit.blocks[2].training
    small = er.module.ViTEncoder(dict(vit_type='vit_small', pyramid=False, out_indices=(0, 1, 2, 3),
                                      vit_kwargs=dict(n_storage_tokens=4)))
    assert small.resample is None and small.out_indices == [0, 1, 2, 3] and small.output_channels() == (384,) * 4
    assert small.vit.n_storage_tokens == 4
    with pytest.raises(NotImplementedError):
        er.module.ViTEncoder(dict(vit_type='vit_7b'))
    with pytest.raises(ValueError):
        er.module.ViTEncoder(dict(vit_type='vit_small', pretrained=True))
    with pytest.raises(ValueError):
        er.module.ViTEncoder(dict(vit_type='vit_small', out_indices=(0, 1, 2)))


def test_exports_after_install_as_ever():
    er.install_as_ever()
    import ever.module.dinov3 as d
    for name in ('PatchEmbed', 'RopePositionEmbedding', 'LinearKMaskedBias', 'SelfAttention', 'Mlp', 'LayerScale',
                 'SelfAttentionBlock', 'DinoVisionTransformer', 'init_weights_vit', 'vit_small', 'vit_base', 'vit_large',
                 'vit_so400m', 'vit_huge2', 'vit_giant2', 'vitl16_sat493m'):
        assert getattr(d, name) is getattr(dinov3, name)
    assert hasattr(er.module, 'ViTEncoder')
