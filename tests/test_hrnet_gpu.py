"""HRNetV2 on the HIP path against fixtures of the imported reference (tools/gen_golden_hrnet.py): one 4-branch
HighResolutionModule (train-mode forward + backward, BatchNorm buffers, eval outputs) and a reduced HRNetV2 + HRNetHead end to
end with cross-entropy; the fused exchange against its layer-by-layer fallback; folded inference; Launcher steps with a
checkpoint round trip; the weight-gradient side stream on and off.  Weights and inputs are regenerated from
oracle/portable.py.  Tolerances are those of tests/test_deeplab_gpu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')

MOD_N, MOD_CH, MOD_HW = 2, (8, 16, 32, 64), (32, 16, 8, 4)
W8_EXTRA = dict(
    stage1=dict(num_modules=1, num_branches=1, block='BOTTLENECK', num_blocks=(1,), num_channels=(16,), fuse_method='SUM'),
    stage2=dict(num_modules=1, num_branches=2, block='BASIC', num_blocks=(1, 1), num_channels=(8, 16), fuse_method='SUM'),
    stage3=dict(num_modules=2, num_branches=3, block='BASIC', num_blocks=(1, 1, 1), num_channels=(8, 16, 32),
                fuse_method='SUM'),
    stage4=dict(num_modules=1, num_branches=4, block='BASIC', num_blocks=(1, 1, 1, 1), num_channels=(8, 16, 32, 64),
                fuse_method='SUM'))
# a bias in front of a training-mode BatchNorm: its gradient is zero in exact arithmetic (fp64 norm 6e-17), so only
# finiteness is asserted and it stays out of the relative comparisons
ZERO_GRAD = 'head.head.0.fuse_conv.0.bias'


def _w8(pretrained=False, weight_path=None, norm_eval=False, frozen_stages=-1):
    from ever_amd.module._hrnet import HighResolutionNet
    return HighResolutionNet(W8_EXTRA, norm_eval, frozen_stages=frozen_stages)


def _rel(a, b):
    a = a.detach().double().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _portable(m):
    from oracle import portable
    filled = portable.fill_state_dict(m.state_dict())
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in filled.items()}, strict=True)
    return m


def _nhwc(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda).contiguous(memory_format=torch.channels_last)


def _digest_close(got, ref, what, tol=2e-3):
    """grad_digest entries [norm, sum, 4 samples, projection], each within tol of the tensor's norm"""
    got, ref = np.asarray(got), np.asarray(ref)
    scale = max(abs(ref[0]), 1e-30)
    assert np.abs(got - ref).max() <= tol * scale, (what, got, ref)


class _OnHost:
    """what oracle.gen_golden.grad_digest reads of a parameter: its gradient (on the host)"""

    def __init__(self, p):
        self.grad = p.grad.detach().cpu()


def _module(cuda):
    import ever_amd as er
    from ever_amd.module._resnets import BasicBlock
    return _portable(er.module.HighResolutionModule(4, BasicBlock, (1, 1, 1, 1), list(MOD_CH), list(MOD_CH), 'SUM')).to(cuda)


def _module_io(cuda):
    from oracle import portable
    xs = [_nhwc(portable.normalish(f'hrnet_module/x{i}', (MOD_N, c, s, s)), cuda) for i, (c, s) in enumerate(zip(MOD_CH, MOD_HW))]
    gs = [_nhwc(portable.uniform(f'hrnet_module/g{i}', (MOD_N, c, s, s)), cuda) for i, (c, s) in enumerate(zip(MOD_CH, MOD_HW))]
    return xs, gs


def _check_module_against_fixture(m, cuda):
    """train-mode outputs to 1e-4 of their range; input gradients and the fuse layers' full gradients to 1e-3; the other
    parameters' digests to 2e-3; BatchNorm buffers to 1e-4; eval outputs to 1e-4"""
    from oracle.gen_golden import grad_digest
    gold = np.load(os.path.join(GOLD, 'hrnet_module.npz'))
    xs, gs = _module_io(cuda)
    xs = [x.requires_grad_() for x in xs]
    m.train()
    ys = m(list(xs))
    torch.autograd.backward(ys, gs)
    torch.cuda.synchronize()
    for i, (y, x) in enumerate(zip(ys, xs)):
        assert _rel(y, gold[f'y{i}']) < 1e-4, i
        assert _rel(x.grad, gold[f'dx{i}']) < 1e-3, i
    for k, p in m.named_parameters():
        if 'grad/' + k in gold:
            assert _rel(p.grad, gold['grad/' + k]) < 1e-3, k
        else:
            _digest_close(grad_digest([(k, _OnHost(p))])[k], gold['digest/' + k], k)
    for k, v in m.state_dict().items():
        if 'running_' in k:
            assert _rel(v, gold['buffer/' + k]) < 1e-4, k
    m.eval()
    with torch.no_grad():
        for i, y in enumerate(m([x.detach() for x in xs])):
            assert _rel(y, gold[f'y_eval{i}']) < 1e-4, i


def test_module_matches_reference(cuda):
    from ever_amd.hip import functional as HF
    m = _module(cuda)
    before = dict(HF.hr_fuse_stats)
    _check_module_against_fixture(m, cuda)
    d = {k: HF.hr_fuse_stats[k] - before[k] for k in before}
    # one node per output and pass (train, eval); eval: all twelve BatchNorms enter from their running statistics.  (In
    # training this narrow module's convolutions leave no statistics records — their epilogue writes them for channel counts
    # that fill its 64-column tile — so each BatchNorm runs by itself and its term is plain; the fused training form is
    # test_fused_training_terms_equal_the_layer_by_layer_fallback's.)
    assert d['nodes'] == 8 and d['bn_running'] == 12
    assert d['plain'] + d['bn_batch'] + d['bn_running'] == 32


def test_fused_module_equals_the_layer_by_layer_fallback(cuda):
    """a forward hook on a BatchNorm of an up-sampling fuse layer and on a down-sampling chain sends those terms through the
    modules' own forward (a plain term each): the same fixture within the same tolerances, and the hooks saw their outputs"""
    m = _module(cuda)
    seen = []
    h1 = m.fuse_layers[0][2][1].register_forward_hook(lambda mod, i, o: seen.append(('bn', tuple(o.shape))))
    h2 = m.fuse_layers[3][1].register_forward_hook(lambda mod, i, o: seen.append(('chain', tuple(o.shape))))
    h3 = m.fuse_layers[2][0][1][0].register_forward_hook(lambda mod, i, o: seen.append(('conv', tuple(o.shape))))
    _check_module_against_fixture(m, cuda)
    for h in (h1, h2, h3):
        h.remove()
    assert seen.count(('bn', (MOD_N, 8, 8, 8))) == 2 and seen.count(('chain', (MOD_N, 64, 4, 4))) == 2
    assert seen.count(('conv', (MOD_N, 32, 8, 8))) == 2
    # the nearest up-sampling has no tensor of its own to show to a hook: said, not skipped
    h = m.fuse_layers[0][1].register_forward_hook(lambda mod, i, o: None)
    with pytest.raises(NotImplementedError, match='up-sampling'):
        m([x for x in _module_io(cuda)[0]])
    h.remove()


WIDE_N, WIDE_CH, WIDE_HW = 4, (64, 128, 256), (16, 8, 4)


def _wide_run(cuda, hooked):
    import ever_amd as er
    from ever_amd.hip import functional as HF
    from ever_amd.module._resnets import BasicBlock
    from oracle import portable
    m = _portable(er.module.HighResolutionModule(3, BasicBlock, (1, 1, 1), list(WIDE_CH), list(WIDE_CH), 'SUM')).to(cuda).train()
    if hooked:
        for mod in m.fuse_layers.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.register_forward_hook(lambda mod, i, o: None)
    xs = [_nhwc(portable.normalish(f'hrnet_wide/x{i}', (WIDE_N, c, s, s)), cuda).requires_grad_()
          for i, (c, s) in enumerate(zip(WIDE_CH, WIDE_HW))]
    gs = [_nhwc(portable.uniform(f'hrnet_wide/g{i}', (WIDE_N, c, s, s)), cuda) for i, (c, s) in enumerate(zip(WIDE_CH, WIDE_HW))]
    before = dict(HF.hr_fuse_stats)
    ys = m(list(xs))
    torch.autograd.backward(ys, gs)
    torch.cuda.synchronize()
    d = {k: HF.hr_fuse_stats[k] - before[k] for k in before}
    return (d, [y.detach().cpu().numpy() for y in ys], [x.grad.cpu().numpy() for x in xs],
            {k: p.grad.cpu().numpy() for k, p in m.named_parameters()},
            {k: v.cpu().numpy() for k, v in m.state_dict().items() if 'running_' in k or 'num_batches' in k})


def test_fused_training_terms_equal_the_layer_by_layer_fallback(cuda):
    """channel counts whose convolutions leave statistics records (64 / 128 / 256): all six BatchNorms of the exchange are
    finalised and applied inside the nodes, their backward runs on the node's masked gradient and block sums — against the
    same module with a forward hook on every fuse BatchNorm (each term then runs layer by layer, the path the fixture of
    test_module_matches_reference checks against the reference), within that test's tolerances"""
    d0, y0, dx0, dp0, b0 = _wide_run(cuda, False)
    d1, y1, dx1, dp1, b1 = _wide_run(cuda, True)
    assert d0 == dict(nodes=3, plain=3, bn_batch=6, bn_running=0), d0
    assert d1 == dict(nodes=3, plain=9, bn_batch=0, bn_running=0), d1
    for a, b in zip(y0, y1):
        assert _rel(a, b) < 1e-4
    for a, b in zip(dx0, dx1):
        assert _rel(a, b) < 1e-3
    for k in dp0:
        assert _rel(dp0[k], dp1[k]) < 1e-3, k
    for k in b0:
        assert _rel(b0[k], b1[k]) < 1e-4, k


def test_eval_mode_backward_fused_equals_fallback(cuda):
    """eval mode with autograd on (norm_eval fine-tuning): scale / shift from the running statistics, the BatchNorm backward
    with constant statistics — against the same module run layer by layer (hooks on every fuse BatchNorm)"""
    xs, gs = _module_io(cuda)
    grads = []
    for hooked in (False, True):
        m = _module(cuda).eval()
        if hooked:
            for mod in m.fuse_layers.modules():
                if isinstance(mod, torch.nn.BatchNorm2d):
                    mod.register_forward_hook(lambda mod, i, o: None)
        x = [t.clone().requires_grad_() for t in xs]
        ys = m(list(x))
        torch.autograd.backward(ys, gs)
        torch.cuda.synchronize()
        grads.append(([y.detach() for y in ys], [t.grad for t in x],
                      {k: p.grad for k, p in m.named_parameters() if k.startswith('fuse_layers.')}))
    (y0, dx0, dp0), (y1, dx1, dp1) = grads
    for a, b in zip(y0, y1):
        assert _rel(a, b.cpu().numpy()) < 1e-5
    for a, b in zip(dx0, dx1):
        assert _rel(a, b.cpu().numpy()) < 1e-4
    for k in dp0:
        assert _rel(dp0[k], dp1[k].cpu().numpy()) < 1e-4, k


def _e2e_model(cuda, in_channels=3, num_classes=6):
    import ever_amd as er
    er.registry.MODEL.register('hrnetv2_w8_fixture', _w8, override=True, verbose=False)
    m = er.module.HRNetSeg(dict(encoder=dict(hrnet_type='hrnetv2_w8_fixture', in_channels=in_channels),
                                head=dict(num_classes=num_classes)))
    return _portable(m).to(cuda)


def test_end_to_end_matches_reference(cuda):
    from oracle import portable
    from oracle.gen_golden import grad_digest
    meta = json.load(open(os.path.join(GOLD, 'hrnet_e2e_w8.json')))
    gold = np.load(os.path.join(GOLD, 'hrnet_e2e_w8.npz'))
    x, y = portable.synthetic_batch('hrnet_e2e_w8', meta['n'], 3, meta['hw'], meta['hw'], meta['num_classes'])
    for name in ('grads', 'grads_fp64'):          # digest rows in grad_keys' order
        meta[name] = {str(k): list(v) for k, v in zip(gold['grad_keys'], gold[name])}
    m = _e2e_model(cuda).train()
    assert m.head.head[0].fuse_conv[0].in_channels == 120        # the default: the sum of the encoder's output channels
    lg = m.head(m.en(_nhwc(x, cuda)))
    loss = m.loss(lg, torch.from_numpy(y).to(cuda))['cls_loss']
    loss.backward()
    torch.cuda.synchronize()
    lgn = lg.detach().cpu().numpy()
    assert _rel(lgn[..., ::4, ::4], gold['logits']) < 1e-3
    assert abs(loss.item() - meta['loss']) <= 1e-4 * abs(meta['loss'])
    # digests (test_deeplab_gpu.py's rule): the norm against the fp64 reference within max(2e-2, 6x the case's worst
    # fp32-vs-fp64 norm deviation); samples and projection within max(2e-3, twice the CASE's worst such deviation)
    keys = [k for k in meta['grads'] if k != ZERO_GRAD]
    case = max(float(np.abs(np.asarray(meta['grads'][k]) - np.asarray(meta['grads_fp64'][k]))[[0, 2, 3, 4, 5, 6]].max()
                     / max(abs(meta['grads_fp64'][k][0]), 1e-30)) for k in keys)
    case_norm = max(abs(meta['grads'][k][0] - meta['grads_fp64'][k][0]) / meta['grads_fp64'][k][0] for k in keys)
    assert meta['grads_fp64'][ZERO_GRAD][0] < 1e-12
    params = dict(m.named_parameters())
    assert sorted(params) == sorted(meta['grads'])
    for k, p in params.items():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        if k == ZERO_GRAD:
            continue
        d32, d64 = np.asarray(meta['grads'][k]), np.asarray(meta['grads_fp64'][k])
        got = np.asarray(grad_digest([(k, _OnHost(p))])[k])
        assert abs(got[0] - d64[0]) <= max(2e-2, 6 * case_norm) * abs(d64[0]) + 1e-7, (k, got, d32, d64)
        keep = [0, 2, 3, 4, 5, 6]       # (the sum grows as sqrt(numel) x the norm: compared through the projection instead)
        _digest_close(got[keep], d32[keep], k, tol=max(2e-3, 2 * case))
    # argmax: identical wherever the reference decides by more than 1e-3 of the logit range; inside that band at most as
    # many flips as the band has pixels
    am, margin = gold['argmax'], gold['margin']
    decided = margin > 1e-3 * meta['logit_range']
    got = lgn.argmax(1)
    assert np.array_equal(got[decided], am[decided])
    flips = int((got != am).sum())
    print(f"argmax flips {flips} of {int((~decided).sum())} pixels inside the tie band")
    assert flips <= int((~decided).sum())        # the condition; MI355X: 0 flips of 185 tie-band pixels


def test_activation_checkpointing_gives_the_same_step(cuda):
    """`with_cp`: the body under non-reentrant activation checkpointing (saved-tensor hooks are observers: every exchange term
    then runs layer by layer) — the same loss and gradients as the plain step to fp32 rounding"""
    from oracle import portable
    x, y = portable.synthetic_batch('hrnet_cp', 2, 3, 64, 64, 6)
    res = []
    for with_cp in (False, True):
        m = _e2e_model(cuda).train()
        m.en.config.with_cp = with_cp
        loss = m(_nhwc(x, cuda), torch.from_numpy(y).to(cuda))['cls_loss']
        loss.backward()
        torch.cuda.synchronize()
        res.append((loss.item(), {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}))
    (l0, g0), (l1, g1) = res
    assert abs(l0 - l1) <= 1e-5 * abs(l0)
    for k in g0:
        if k != ZERO_GRAD:
            assert _rel(g1[k], g0[k]) < 2e-3, k


def test_folded_inference_matches_unfolded(cuda):
    from ever_amd.module.fold import fold_batchnorm
    m = _e2e_model(cuda).eval()
    x = torch.randn(2, 3, 128, 128, device=cuda)
    with torch.no_grad():
        y0 = m(x)
        fold_batchnorm(m)
        assert m._folded_pairs >= 40
        y1 = m(x)
    assert _rel(y1, y0.cpu().numpy()) < 1e-5


def test_launcher_steps_and_checkpoint(cuda, tmp_path):
    """three Launcher iterations of HRNetSeg (one class: BCE + dice, a 4-band image) with FusedSGD, then a checkpoint round
    trip"""
    import ever_amd as er
    from tests import plumbing_common as pc
    m = _e2e_model(cuda, in_channels=4, num_classes=1).train()
    loader = torch.utils.data.DataLoader(pc.ToyTiles(), batch_size=2, shuffle=False)
    sched = er.builder.make_learningrate(dict(type='poly', params=dict(base_lr=0.01, power=0.9, max_iters=3)))
    opt = er.opt.FusedSGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    tl = er.Launcher(str(tmp_path), m, opt, sched)
    rec = []
    orig = tl._logger.train_log

    def spy(**kw):
        rec.append({k: float(v) for k, v in kw['loss_dict'].items()})
        return orig(**kw)

    tl._logger.train_log = spy
    tl.train_by_config(loader, config=er.AttrDict.from_dict(dict(num_iters=3, save_ckpt_interval_epoch=1000)))
    assert len(rec) == 3 and all(np.isfinite(r['bce_loss']) and np.isfinite(r['dice_loss']) for r in rec)
    assert all(torch.isfinite(p).all() for p in m.parameters())
    sd = m.state_dict()
    assert int(sd['en.hrnet.stage4.0.fuse_layers.0.1.1.num_batches_tracked']) == 3       # counted inside the exchange as well
    path = os.path.join(str(tmp_path), 'ck.pth')
    torch.save(sd, path)
    m2 = _e2e_model(cuda, in_channels=4, num_classes=1)
    m2.load_state_dict(torch.load(path, map_location=cuda), strict=True)
    m.eval()
    m2.eval()
    x = torch.randn(2, 4, 64, 64, device=cuda)
    with torch.no_grad():
        assert torch.equal(m(x), m2(x))


_SIDE = r'''
import sys, torch
sys.path.insert(0, {root!r})
import ever_amd as er
from ever_amd.hip import functional as HF
from tests.test_hrnet_gpu import _e2e_model
HF.set_wgrad_stream({on})
HF.set_wgrad_shared_split(False)
cuda = torch.device('cuda:0')
m = _e2e_model(cuda).train()
g = torch.Generator().manual_seed(2)
x = torch.randn(2, 3, 128, 128, generator=g).to(cuda)
y = torch.randint(0, 6, (2, 128, 128), generator=g).to(cuda)
sum(m(x, y).values()).backward()
torch.cuda.synchronize()
torch.save({{k: p.grad.cpu() for k, p in m.named_parameters()}}, {out!r})
'''


def test_side_stream_on_and_off_give_the_same_bits(cuda, tmp_path):
    """one training step with the weight-gradient side stream on and off, each in a child process: the same gradients bit
    for bit (the exchange backward has one owner per element and no atomics)"""
    outs = []
    for on in (False, True):
        out = str(tmp_path / f'g{int(on)}.pt')
        code = _SIDE.format(root=ROOT, on=on, out=out)
        r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(torch.load(out))
    g0, g1 = outs
    diff = [k for k in g0 if not torch.equal(g0[k], g1[k])]
    assert not diff, diff[:5]
