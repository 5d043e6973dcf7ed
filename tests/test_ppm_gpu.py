"""Pyramid pooling on the HIP path: PyramidPoolModule (both bottlenecks and none) and PPMHead against fixtures of the
imported reference (tools/gen_golden_ppm.py) in train and eval mode; the fused module against the same module run layer
by layer with aten's pool, interpolate and cat on the device; PoolBlock(1) on the path it had before; dropout under one
seed; one PSPNet-R18 training step; the traced form.  Weights and inputs are regenerated from oracle/portable.py.
Tolerances are those of tests/test_deeplab_gpu.py, whose image-level branch has the same few-sample BatchNorm (here the
bin-1 BatchNorm normalises four values per channel)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')

N, CIN, CPOOL, COUT, BINS = 4, 16, 8, 16, (1, 2, 3, 6)
CASES = {
    'ppm3x3_12x12': ('module', '3x3', (12, 12)),
    'ppm3x3_13x9': ('module', '3x3', (13, 9)),
    'ppm1x1_13x9': ('module', '1x1', (13, 9)),
    'ppmid_12x12': ('module', 'none', (12, 12)),
    'head_13x9': ('head', '3x3', (13, 9)),
}
HEAD_CLASSES, HEAD_SCALE = 3, 4.0


def _rel(a, b):
    a = a.detach().double().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    b = b.detach().double().cpu().numpy() if torch.is_tensor(b) else np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _portable(m):
    from oracle import portable
    filled = portable.fill_state_dict(m.state_dict())
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in filled.items()}, strict=True)
    return m


def _nhwc(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda).contiguous(memory_format=torch.channels_last)


def _args(bottleneck, dropout=0):
    return dict(in_channels=CIN, pool_channels=CPOOL, out_channels=COUT, bins=BINS, bottleneck_conv=bottleneck, dropout=dropout)


def _build(kind, bottleneck, cuda):
    import ever_amd as er
    if kind == 'module':
        m = er.module.PyramidPoolModule(**_args(bottleneck))
    else:
        m = er.module.PPMHead(dict(ppm=_args(bottleneck), num_classes=HEAD_CLASSES, upsample_scale=HEAD_SCALE))
    return _portable(m).to(cuda)


class _OnHost:
    """what oracle.gen_golden.grad_digest reads of a parameter: its gradient (on the host)"""

    def __init__(self, p):
        self.grad = p.grad.detach().cpu()


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(GOLD, 'ppm_ref.npz'))


@pytest.mark.parametrize('name', list(CASES))
def test_matches_reference(name, cuda, gold):
    """train-mode output to 1e-4 of its range, the input gradient to 1e-3, parameter-gradient digests to 2e-3 of the
    gradient's norm, BatchNorm buffers and the eval-mode output to 1e-4"""
    from oracle import portable
    from oracle.gen_golden import grad_digest
    from ever_amd.hip import functional as HF
    kind, bottleneck, (h, w) = CASES[name]
    m = _build(kind, bottleneck, cuda).train()
    x = _nhwc(portable.normalish(name + '/x', (N, CIN, h, w)), cuda).requires_grad_()
    before = dict(HF.pyramid_stats)
    y = m(x)
    g = _nhwc(portable.uniform(name + '/g', tuple(y.shape)), cuda)
    y.backward(g)
    torch.cuda.synchronize()
    assert HF.pyramid_stats['pool'] - before['pool'] == 1 and HF.pyramid_stats['concat'] - before['concat'] == 1
    assert HF.pyramid_stats['skip_views'] - before['skip_views'] == 1       # the concat's slice was read in place
    assert tuple(y.shape) == gold[name + '/out'].shape
    assert _rel(y, gold[name + '/out']) < 1e-4
    assert _rel(x.grad, gold[name + '/dx']) < 1e-3
    for k, p in m.named_parameters():
        got = np.asarray(grad_digest([(k, _OnHost(p))])[k])
        ref = gold[f'{name}/digest/{k}']
        assert np.abs(got - ref).max() <= 2e-3 * max(abs(ref[0]), 1e-30), (k, got, ref)
    for k, v in m.state_dict().items():
        if 'running_' in k:
            assert _rel(v, gold[f'{name}/buffer/{k}']) < 1e-4, k
    m.eval()
    with torch.no_grad():
        ye = m(x.detach())
    assert _rel(ye, gold[name + '/out_eval']) < 1e-4


def _layer_by_layer(m, x):
    """PyramidPoolModule's forward with aten's adaptive pool, bilinear interpolate and cat around the module's own blocks"""
    size = x.shape[-2:]
    out = [x]
    for blk, b in zip(m.pools, m.bins):
        z = blk[1](F.adaptive_avg_pool2d(x, b))
        out.append(F.interpolate(z, size=size, mode='bilinear', align_corners=False))
    return m.dropout(m.conv(torch.cat(out, dim=1)))


@pytest.mark.parametrize('hw', [(12, 12), (13, 9)])
def test_fused_against_layer_by_layer(hw, cuda):
    """the same weights and input through the fused passes and through aten's layer-by-layer chain, both on the device, in
    train mode: output to 1e-4, input and parameter gradients to 1e-3 (the few-sample BatchNorm amplifies the rounding
    differences of the pools alike in both comparisons)"""
    from oracle import portable
    m = _build('module', '3x3', cuda).train()
    xn = portable.normalish('ppm_lbl/x', (N, CIN) + hw)
    gn = portable.uniform('ppm_lbl/g', (N, COUT) + hw)
    res = []
    for fn in (lambda t: m(t), lambda t: _layer_by_layer(m, t)):
        m.zero_grad(set_to_none=True)
        x = _nhwc(xn, cuda).requires_grad_()
        y = fn(x)
        y.backward(_nhwc(gn, cuda))
        torch.cuda.synchronize()
        res.append((y.detach(), x.grad, {k: p.grad.clone() for k, p in m.named_parameters()}))
    (y0, dx0, g0), (y1, dx1, g1) = res
    assert _rel(y0, y1) < 1e-4 and _rel(dx0, dx1) < 1e-3
    for k in g0:
        assert _rel(g0[k], g1[k]) < 1e-3, k


def test_pool_block_of_one_is_on_its_old_path(cuda):
    """PoolBlock(1): global average pool -> ConvBlock -> exact broadcast, bit for bit, and no pyramid kernel runs"""
    import ever_amd as er
    from ever_amd.hip import functional as HF
    from ever_amd.module.layers import run_sequence
    blk = _portable(er.module.PoolBlock(1, 32, 16)).to(cuda).train()
    x = torch.randn(4, 13, 9, 32, device=cuda).permute(0, 3, 1, 2)
    before = dict(HF.pyramid_stats)
    y = blk(x)
    want = HF.broadcast_hw(run_sequence(list(blk), x), x.shape[-2:])
    assert HF.pyramid_stats == before
    assert tuple(y.shape) == (4, 16, 13, 9) and torch.equal(y, want)
    # the pyramid's block at a size above 1 runs the one-bin kernels: against aten on the device
    from ever_amd.module.ppm import PyramidPoolBlock
    blk3 = _portable(PyramidPoolBlock(3, 32, 16)).to(cuda).eval()
    with torch.no_grad():
        y3 = blk3(x)
        ref = F.interpolate(blk3[1](F.adaptive_avg_pool2d(x, 3)), size=(13, 9), mode='bilinear', align_corners=False)
    assert _rel(y3, ref) < 1e-5
    assert _rel(er.module.AdaptiveAvgPool2d(6)(x), F.adaptive_avg_pool2d(x, 6)) < 1e-6


def test_dropout_under_one_seed(cuda):
    """dropout > 0: the module's output is layers.Dropout2d applied by hand, under the same seed, to the output of the same
    module without dropout"""
    import ever_amd as er
    m = _portable(er.module.PyramidPoolModule(**_args('1x1', dropout=0.5))).to(cuda).train()
    m0 = _portable(er.module.PyramidPoolModule(**_args('1x1'))).to(cuda).train()
    assert isinstance(m.dropout, er.module.layers.Dropout2d)
    x = torch.randn(N, 12, 12, CIN, device=cuda).permute(0, 3, 1, 2)
    torch.manual_seed(5)
    y = m(x)
    torch.manual_seed(5)
    want = er.module.layers.Dropout2d(0.5).train()(m0(x))
    assert torch.equal(y, want)
    dropped = (y.abs().amax(dim=(2, 3)) == 0).float().mean().item()
    assert 0.1 < dropped < 0.9


def test_pspnet_r18_training_step(cuda):
    import ever_amd as er
    m = er.module.PSPNet(dict(encoder=dict(resnet_type='resnet18'),
                              head=dict(ppm=dict(in_channels=512, pool_channels=128, out_channels=128), num_classes=6)))
    m = _portable(m).to(cuda).train()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 64, 64, generator=g).to(cuda)
    y = torch.randint(0, 6, (2, 64, 64), generator=g).to(cuda)
    opt = er.opt.FusedSGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    losses = m(x, y)
    assert losses and all(k.endswith('_loss') for k in losses)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    assert all(torch.isfinite(v).all() for v in losses.values())
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    assert any(p.grad.abs().max() > 0 for n, p in m.named_parameters() if n.startswith('en.'))
    opt.step()
    assert all(torch.isfinite(p).all() for p in m.parameters())
    m.eval()
    with torch.no_grad():
        out = m(x)
    assert tuple(out.shape) == (2, 6, 64, 64) and torch.isfinite(out).all()


def test_traced_form(cuda):
    """a TorchScript trace of the eval-mode head records the reference's aten expression for the pyramid (adaptive pools,
    bilinear interpolation, cat); the replay equals the eager forward, which runs the kernels, on a second input too"""
    from ever_amd.hip import functional as HF
    m = _build('head', '3x3', cuda).eval()
    g = torch.Generator().manual_seed(9)
    x1, x2 = (torch.randn(2, 13, 9, CIN, generator=g).to(cuda).permute(0, 3, 1, 2) for _ in range(2))
    with torch.no_grad():
        before = HF.pyramid_stats['aten']
        traced = torch.jit.trace(m, (x1,), check_trace=False)
        assert HF.pyramid_stats['aten'] - before == 2
        kinds = {n.kind() for n in traced.inlined_graph.nodes()}
        assert 'aten::adaptive_avg_pool2d' in kinds and 'aten::cat' in kinds, kinds
        assert any(k.startswith('aten::upsample_bilinear2d') or k == 'aten::__interpolate' for k in kinds), kinds
        for x in (x1, x2):
            assert _rel(traced(x), m(x)) < 1e-5
