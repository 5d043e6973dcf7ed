"""ConvNeXt on the HIP path against fixtures of the imported reference (tools/gen_golden_convnext.py): two reduced models
(depths 1-1-2-1, dims 8-16-32-64, layer scale 1) on a square and on an odd-sized input, both forward forms and the gradients of
a fixed linear functional; eval against train mode; stochastic depth against the same block in aten ops under the same seed;
one ConvNeXtEncoder -> FPN -> AssymetricDecoder training step with the weight-gradient side stream on and off; a checkpoint
round trip.  Weights and inputs are regenerated from oracle/portable.py (tests/convnext_common.py).  Tolerances are those of
tests/test_hrnet_gpu.py: outputs to 1e-4 of their range, the input gradient and the stored full gradients to 1e-3, every other
parameter's digest to 2e-3 of its norm."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import convnext_common as cc

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


def _reduced(cuda, **kw):
    from ever_amd.module.dinov3 import ConvNeXt
    return cc.load_filled(ConvNeXt(**dict(cc.REDUCED, **kw))).to(cuda)


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(GOLD, 'convnext_ref.npz'))


@pytest.mark.parametrize('case', list(cc.CASES))
def test_reduced_model_matches_reference(cuda, gold, case):
    from oracle.gen_golden import grad_digest
    m = _reduced(cuda).train()
    outs, dx = cc.run_case(m, case, cc.case_input(case).to(cuda))
    torch.cuda.synchronize()
    for k, v in outs.items():
        r = _rel(v, gold[f'{case}/{k}'])
        print(f'{case} {k} {tuple(v.shape)}: {r:.2e} of the range')
        assert r < 1e-4, (k, r)
    r = _rel(dx, gold[f'{case}/dx'])
    print(f'{case} input gradient: {r:.2e}')
    assert r < 1e-3
    names = [str(k) for k in gold['param_names']]
    params = dict(cc.named_grads(m))
    assert list(params) == names
    for i, (k, p) in enumerate(params.items()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        if k in cc.FULL_GRADS:
            r = _rel(p.grad, gold[f'{case}/grad/{k}'])
            print(f'{case} grad {k}: {r:.2e}')
            assert r < 1e-3, (k, r)
        else:
            got, ref = np.asarray(grad_digest([(k, _OnHost(p))])[k]), gold[f'{case}/digest'][i]
            assert np.abs(got - ref).max() <= 2e-3 * max(abs(ref[0]), 1e-30), (k, got, ref)


def test_odd_case_drops_a_row_and_a_column(cuda):
    m = _reduced(cuda).eval()
    with torch.no_grad():
        maps = m.get_intermediate_layers(cc.case_input('odd').to(cuda), n=4, reshape=True)
        toks = m.get_intermediate_layers(cc.case_input('odd').to(cuda), n=[3], return_class_token=True)
    assert [tuple(t.shape[2:]) for t in maps] == [(18, 14), (9, 7), (4, 3), (2, 1)]
    assert tuple(toks[0][0].shape) == (2, 2, 64) and tuple(toks[0][1].shape) == (2, 64)
    assert torch.equal(toks[0][0], maps[3].flatten(2).transpose(1, 2))


def test_eval_equals_train_without_drop_path(cuda):
    m = _reduced(cuda)
    x = cc.case_input('sq').to(cuda)
    with torch.no_grad():
        a = m.train().get_intermediate_layers(x, n=4, reshape=True)
        fa = m.forward_features(x)
        b = m.eval().get_intermediate_layers(x, n=4, reshape=True)
        fb = m.forward_features(x)
        assert torch.equal(m(x), fb['x_norm_clstoken']) and isinstance(m(x, is_training=True), dict)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    for k in ('x_norm_clstoken', 'x_norm_patchtokens', 'x_prenorm'):
        assert torch.equal(fa[k], fb[k])
    assert fa['x_storage_tokens'].shape[1] == 0 and fa['masks'] is None


def _aten_block(blk, x, rate):
    """the block's definition in aten ops on the device (NCHW in, the reference's order of operations and its draw)"""
    c = x.shape[1]
    y = F.conv2d(x, blk.dwconv.weight, blk.dwconv.bias, padding=3, groups=c).permute(0, 2, 3, 1)
    y = F.layer_norm(y, (c,), blk.norm.weight, blk.norm.bias, blk.norm.eps)
    y = F.linear(F.gelu(F.linear(y, blk.pwconv1.weight, blk.pwconv1.bias)), blk.pwconv2.weight, blk.pwconv2.bias)
    y = (blk.gamma * y).permute(0, 3, 1, 2)
    keep = 1 - rate
    mask = (keep + torch.rand((x.shape[0], 1, 1, 1), dtype=x.dtype, device=x.device)).floor_()
    return x + y.div(keep) * mask, mask.reshape(-1)


def test_drop_path_matches_aten_under_the_same_seed(cuda):
    """one draw of N numbers per block: the same samples dropped, the same values (1e-6 of the range; the convolutions in
    the exact-fp32 arithmetic, so that both sides are fp32 dot products) and the same generator state afterwards"""
    from ever_amd.hip import functional as HF
    from ever_amd.module.dinov3 import Block
    rate, n, c = 0.3, 16, 8
    torch.manual_seed(3)
    blk = Block(c, drop_path=rate, layer_scale_init_value=1.0).to(cuda).train()
    with torch.no_grad():
        for p in blk.parameters():
            p.copy_(torch.randn(p.shape, device=cuda) * (0.3 if p.dim() > 1 else 1.0))
    x = torch.randn(n, c, 9, 7, device=cuda)
    prev = HF.set_conv_math('f32')
    try:
        with torch.no_grad():
            torch.manual_seed(11)
            got = blk(x)
            state_hip = torch.cuda.get_rng_state(cuda)
            torch.manual_seed(11)
            ref, mask = _aten_block(blk, x, rate)
            state_aten = torch.cuda.get_rng_state(cuda)
    finally:
        HF.set_conv_math(prev)
    torch.cuda.synchronize()
    assert torch.equal(state_hip, state_aten)
    dropped = mask == 0
    assert 0 < int(dropped.sum()) < n
    assert torch.equal(got[dropped], x[dropped])
    r = _rel(got, ref.cpu().numpy())
    print(f'drop path {rate}: {int(dropped.sum())} of {n} samples dropped, max difference {r:.2e} of the range')
    assert r <= 1e-6
    blk.eval()
    with torch.no_grad():
        state = torch.cuda.get_rng_state(cuda)
        blk(x)
        assert torch.equal(torch.cuda.get_rng_state(cuda), state)          # no draw in eval mode


class _Seg(torch.nn.Module):
    def __init__(self, num_classes=6):
        super().__init__()
        import ever_amd as er
        self.en = er.module.ConvNeXtEncoder(dict(convnext_type='convnext_tiny', drop_path_rate=0.1))
        self.fpn = er.module.FPN(self.en.output_channels(), 64)
        self.decoder = er.module.AssymetricDecoder(64, 32, classifier_config=dict(num_classes=num_classes, scale_factor=4))

    def forward(self, x):
        return self.decoder(self.fpn(self.en(x)))


def _step(cuda, side):
    import ever_amd as er
    from ever_amd.hip import functional as HF
    from oracle import portable
    prev = HF.set_wgrad_stream(side)
    try:
        torch.manual_seed(5)
        m = _Seg().to(cuda).train()
        x, y = portable.synthetic_batch('convnext_step', 2, 3, 64, 64, 6)
        opt = er.opt.FusedSGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
        before = {k: p.detach().clone() for k, p in m.named_parameters()}
        torch.manual_seed(6)
        loss = HF.cross_entropy(m(torch.from_numpy(x).to(cuda)), torch.from_numpy(y).to(cuda), ignore_index=255)
        loss.backward()
        HF.wait_wgrad_stream()
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
        opt.step()
        torch.cuda.synchronize()
    finally:
        HF.set_wgrad_stream(prev)
    return m, loss.item(), before, grads


def test_encoder_fpn_decoder_training_step(cuda):
    m, loss, before, grads = _step(cuda, side=True)
    assert np.isfinite(loss) and loss > 0
    # every parameter is reached but the token norm, which the stage maps do not pass through
    assert sorted(set(before) - set(grads)) == ['en.convnext.norm.bias', 'en.convnext.norm.weight']
    same = [k for k, p in m.named_parameters() if k in grads and torch.equal(p.detach(), before[k])]
    assert not same, f'parameters the step did not change: {same}'
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    _, loss_off, _, grads_off = _step(cuda, side=False)
    assert loss_off == loss
    diff = [k for k in grads if not torch.equal(grads[k], grads_off[k])]
    assert not diff, f'gradients that differ with the weight-gradient side stream off: {diff}'


def test_checkpoint_round_trip_with_strict_keys(cuda, tmp_path):
    m = _reduced(cuda, drop_path_rate=0.2).eval()
    path = str(tmp_path / 'convnext.pth')
    torch.save(m.state_dict(), path)
    from ever_amd.module.dinov3 import ConvNeXt
    m2 = ConvNeXt(**dict(cc.REDUCED, drop_path_rate=0.2))
    res = m2.load_state_dict(torch.load(path, map_location='cpu'), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    m2 = m2.to(cuda).eval()
    x = cc.case_input('odd').to(cuda)
    with torch.no_grad():
        for u, v in zip(m.get_intermediate_layers(x, n=4, reshape=True), m2.get_intermediate_layers(x, n=4, reshape=True)):
            assert torch.equal(u, v)
