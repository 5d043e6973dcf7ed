"""The DINOv3 ViT on the HIP path against fixtures of the imported reference (tools/gen_golden_vit.py): two reduced models
(depth 2, 2 heads of 32 and of 64, 4 storage tokens, masked K bias, layer scale 1, untied local class norm) on a square input,
on a 3 x 5 grid (only H != W shows a swapped RoPE axis) and on 77 tokens (past one key tile): forward_features,
get_intermediate_layers with class and extra tokens, and the gradients of a fixed linear functional.  Weights and inputs are
regenerated from oracle/portable.py (tests/vit_common.py).  Tolerances are those of tests/test_convnext_gpu.py: outputs to 1e-4
of their range, the input gradient and the stored full gradients to 1e-3, every other parameter's digest to 2e-3 of its norm.
They discriminate: on such a model fp32 against fp64 is 1.5e-6 of the range, dropping RoPE moves the patch tokens by 0.8-1.1 of
it, swapping H and W by 0.7-1.0 on the non-square cases, un-masking the K bias by 0.07-0.09.

Also: eval mode twice gives the same bits; the default residual tail (no layer scale) bit for bit against a unit layer scale; a
stand-alone LayerScale's gradients; what HF.attention refuses; ViTEncoder's pyramid, whose maps are dense NHWC; one
ViTEncoder -> FPN -> AssymetricDecoder training step."""
import os

import numpy as np
import pytest
import torch

from tests import vit_common as vc

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _rel(a, b):
    a = a.detach().double().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


class _OnHost:
    """what oracle.gen_golden.grad_digest reads of a parameter: its gradient (on the host)"""

    def __init__(self, p):
        self.grad = p.grad.detach().cpu()


def _reduced(cuda, tag):
    from ever_amd.module.dinov3 import DinoVisionTransformer
    return vc.load_filled(DinoVisionTransformer(**vc.MODELS[tag]), tag).to(cuda)


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(GOLD, 'vit_ref.npz'))


@pytest.mark.parametrize('tag,case', vc.RUNS)
def test_reduced_model_matches_reference(cuda, gold, tag, case):
    from oracle.gen_golden import grad_digest
    m = _reduced(cuda, tag).train()
    outs, dx = vc.run_case(m, tag, case, vc.case_input(case).to(cuda))
    torch.cuda.synchronize()
    pre = f'{tag}/{case}'
    for k, v in outs.items():
        r = _rel(v, gold[f'{pre}/{k}'])
        print(f'{pre} {k} {tuple(v.shape)}: {r:.2e} of the range')
        assert r < 1e-4, (k, r)
    r = _rel(dx, gold[f'{pre}/dx'])
    print(f'{pre} input gradient: {r:.2e}')
    assert r < 1e-3
    names = [str(k) for k in gold[f'{tag}/param_names']]
    params = dict(vc.named_grads(m))
    assert list(params) == names
    for i, (k, p) in enumerate(params.items()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        if k in vc.FULL_GRADS:
            r = _rel(p.grad, gold[f'{pre}/grad/{k}'])
            print(f'{pre} grad {k}: {r:.2e}')
            assert r < 1e-3, (k, r)
        else:
            got, ref = np.asarray(grad_digest([(k, _OnHost(p))])[k]), gold[f'{pre}/digest'][i]
            assert np.abs(got - ref).max() <= 2e-3 * max(abs(ref[0]), 1e-30), (k, got, ref)
    assert all(p.grad is None for k, p in m.named_parameters() if k.startswith('local_cls_norm.'))


def test_eval_mode_gives_the_same_bits_twice_and_the_forward_forms_agree(cuda):
    m = _reduced(cuda, 'd32').eval()
    x = vc.case_input('odd').to(cuda)
    with torch.no_grad():
        a, b = m.forward_features(x), m.forward_features(x)
        both = m.forward_features([x, vc.case_input('sq').to(cuda)], [None, None])
        assert torch.equal(m(x), a['x_norm_clstoken']) and isinstance(m(x, is_training=True), dict)
        last = m.get_intermediate_layers(x, n=1, reshape=False, norm=True)
        raw = m.get_intermediate_layers(x, n=1, reshape=True, norm=False)
    for k in ('x_norm_clstoken', 'x_storage_tokens', 'x_norm_patchtokens', 'x_prenorm'):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], both[0][k]), k
    assert a['masks'] is None and tuple(a['x_storage_tokens'].shape) == (2, 4, 64)
    assert tuple(both[1]['x_norm_patchtokens'].shape) == (2, 16, 64)
    assert _rel(last[0], a['x_norm_patchtokens'].cpu().numpy()) < 1e-6      # (normalised with, and without, the prefix rows)
    assert tuple(raw[0].shape) == (2, 64, 3, 5)
    assert torch.equal(raw[0].permute(0, 2, 3, 1).reshape(2, 15, 64), a['x_prenorm'][:, 5:])


def test_default_tail_without_layer_scale_equals_a_unit_layer_scale(cuda):
    """layerscale_init=None (the default of vit_small / base / large) runs the gamma=None residual tail; x + z and x + 1 * z are
    the same fp32 numbers, so it must give the bits of the model above with every gamma set to one — outputs and gradients"""
    from ever_amd.module.dinov3 import DinoVisionTransformer
    unit = _reduced(cuda, 'd32')
    state = {k: (torch.ones_like(v) if k.endswith('.gamma') else v) for k, v in unit.state_dict().items()}
    unit.load_state_dict(state, strict=True)
    plain = DinoVisionTransformer(**dict(vc.MODELS['d32'], layerscale_init=None)).to(cuda)
    assert isinstance(plain.blocks[0].ls1, torch.nn.Identity) and not any(k.endswith('.gamma') for k in plain.state_dict())
    plain.load_state_dict({k: v for k, v in state.items() if not k.endswith('.gamma')}, strict=True)
    x = vc.case_input('odd').to(cuda)
    outs_u, dx_u = vc.run_case(unit.train(), 'd32', 'odd', x)
    outs_p, dx_p = vc.run_case(plain.train(), 'd32', 'odd', x)
    from ever_amd.hip import functional as HF
    HF.wait_wgrad_stream()
    torch.cuda.synchronize()
    for k in outs_u:
        assert torch.equal(outs_u[k], outs_p[k]), k
    assert torch.equal(dx_u, dx_p)
    grads_u = dict(vc.named_grads(unit))
    for k, p in vc.named_grads(plain):
        assert torch.equal(p.grad, grads_u[k].grad), k


def test_standalone_layer_scale_gives_gamma_its_gradient(cuda):
    from ever_amd.module.dinov3 import LayerScale
    gen = torch.Generator().manual_seed(4)
    ls = LayerScale(64, init_values=1.0).to(cuda)
    with torch.no_grad():
        ls.gamma.copy_(torch.rand(64, generator=gen) + 0.5)
    x = torch.randn(3, 7, 64, generator=gen).to(cuda).requires_grad_(True)
    w = torch.randn(3, 7, 64, generator=gen).to(cuda)
    y = ls(x)
    (y * w).sum().backward()
    xr = x.detach().double().requires_grad_(True)
    gr = ls.gamma.detach().double().requires_grad_(True)
    yr = xr * gr
    (yr * w.double()).sum().backward()
    assert torch.equal(y.detach(), x.detach() * ls.gamma.detach())           # one rounding per element
    assert ls.gamma.grad is not None and x.grad is not None
    assert torch.equal(x.grad, (w * ls.gamma.detach()))
    # 21 products per channel summed in fp32: a few ulp of the sum of their magnitudes
    bound = 21 * 2.0 ** -23 * float((xr.detach() * w.double()).abs().sum((0, 1)).max())
    assert float((ls.gamma.grad.double() - gr.grad).abs().max()) <= bound
    with torch.no_grad():
        z = x.detach().clone()
        m = LayerScale(64, inplace=True).to(cuda)
        m.gamma.fill_(2.0)
        assert m(z) is z and torch.equal(z, x.detach() * 2)


def test_attention_wrapper_refuses_out_of_scope_operands(cuda):
    from ever_amd.hip import functional as HF
    from ever_amd.hip.functional import HipPathError
    qkv = torch.randn(2, 9, 3 * 2 * 32, device=cuda)
    tab = torch.randn(4, 32, device=cuda)
    assert tuple(HF.attention(qkv, 2, (tab, tab)).shape) == (2, 9, 64)          # 5 prefix tokens, 4 rotated
    with pytest.raises(HipPathError, match='fp32'):
        HF.attention(qkv, 2, (tab.half(), tab.half()))
    with pytest.raises(HipPathError, match='fp32'):
        HF.attention(qkv, 2, (tab, tab.bfloat16()))
    with pytest.raises(HipPathError, match='batch or head'):
        HF.attention(qkv, 2, (tab[None], tab[None]))                            # a head dimension
    with pytest.raises(HipPathError, match='batch or head'):
        HF.attention(qkv, 2, (tab[None, None].expand(2, 2, 4, 32), tab[None, None].expand(2, 2, 4, 32)))
    with pytest.raises(HipPathError, match='batch or head'):
        HF.attention(qkv, 2, (tab, tab[:3]))                                    # sin and cos of different shapes
    with pytest.raises(HipPathError, match='batch or head'):
        HF.attention(qkv, 2, (torch.randn(4, 64, device=cuda),) * 2)            # tables of another head dimension
    with pytest.raises(HipPathError, match='rows'):
        HF.attention(qkv, 2, (torch.randn(10, 32, device=cuda),) * 2)           # more rope rows than tokens
    for heads, d in ((12, 16), (4, 48), (1, 192), (1, 128)):
        with pytest.raises(HipPathError, match='head dimension'):
            HF.attention(torch.randn(2, 9, 3 * heads * d, device=cuda), heads)
    with pytest.raises(HipPathError):
        HF.attention(qkv.half(), 2)
    with pytest.raises(ValueError):
        HF.attention(qkv, 5)
    torch.cuda.synchronize()


def _encoder_kwargs():
    return dict(embed_dim=64, depth=4, num_heads=2, n_storage_tokens=4, layerscale_init=1.0)


def test_encoder_pyramid_strides_and_channels(cuda):
    import ever_amd as er
    torch.manual_seed(2)
    enc = er.module.ViTEncoder(dict(vit_type='vit_small', vit_kwargs=_encoder_kwargs())).to(cuda).eval()
    flat = er.module.ViTEncoder(dict(vit_type='vit_small', vit_kwargs=_encoder_kwargs(), pyramid=False)).to(cuda).eval()
    flat.load_state_dict(enc.state_dict())
    x = vc.case_input('sq').to(cuda)
    with torch.no_grad():
        maps, same = enc(x), flat(x)
    assert enc.out_indices == [0, 1, 2, 3] and enc.output_channels() == (64,) * 4
    assert [tuple(m.shape) for m in maps] == [(2, 64, 16, 16), (2, 64, 8, 8), (2, 64, 4, 4), (2, 64, 2, 2)]
    assert [tuple(m.shape) for m in same] == [(2, 64, 4, 4)] * 4
    assert torch.equal(maps[2], same[2]) and all(bool(torch.isfinite(m).all()) for m in maps)
    from ever_amd.hip import functional as HF
    assert all(HF.is_nhwc(m) for m in same)       # dense maps: no layout pass in front of the resampling layers or FPN


class _Seg(torch.nn.Module):
    def __init__(self, num_classes=6):
        super().__init__()
        import ever_amd as er
        self.en = er.module.ViTEncoder(dict(vit_type='vit_small', vit_kwargs=_encoder_kwargs()))
        self.fpn = er.module.FPN(self.en.output_channels(), 64)
        self.decoder = er.module.AssymetricDecoder(64, 32, classifier_config=dict(num_classes=num_classes, scale_factor=4))

    def forward(self, x):
        return self.decoder(self.fpn(self.en(x)))


def _step(cuda):
    import ever_amd as er
    from ever_amd.hip import functional as HF
    from oracle import portable
    torch.manual_seed(5)
    m = _Seg().to(cuda).train()
    x, y = portable.synthetic_batch('vit_step', 2, 3, 64, 64, 6)
    opt = er.opt.FusedSGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    loss = HF.cross_entropy(m(torch.from_numpy(x).to(cuda)), torch.from_numpy(y).to(cuda), ignore_index=255)
    loss.backward()
    HF.wait_wgrad_stream()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    opt.step()
    torch.cuda.synchronize()
    return m, loss.item(), before, grads


def test_encoder_fpn_decoder_training_step(cuda):
    m, loss, before, grads = _step(cuda)
    assert np.isfinite(loss) and loss > 0
    # every parameter is reached (none of the reduced encoder's norms is untied)
    assert sorted(set(before) - set(grads)) == []
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    same = [k for k, p in m.named_parameters() if torch.equal(p.detach(), before[k]) and k != 'en.vit.mask_token']
    assert not same, f'parameters the step did not change: {same}'
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    _, loss2, _, _ = _step(cuda)
    assert loss2 == loss
