"""BiFPN on the HIP path against fixtures of the imported reference (tools/gen_golden_bifpn.py): three module cases (train-mode
forward + backward, BatchNorm buffers, eval outputs) and ResNet-18 -> FPN -> BiFPN -> AssymetricDecoder end to end with
cross entropy, at the tolerances of tests/test_deeplab_gpu.py; the index-shift term against a materialised nearest x2; the
layer-by-layer path under a hook; optimizer steps, the state-dict round trip, a trace.  Weights and inputs are regenerated
from oracle/portable.py (tests/bifpn_common.py)."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from tests import bifpn_common as bc
from tests.test_deeplab_gpu import _OnHost, _digest_close, _nhwc, _rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')


def _module(case, cuda):
    import ever_amd as er
    norm, down, strides, _ = bc.MODULE_CASES[case]
    return bc.load_portable(er.module.BiFPN(bc.MODULE_C, list(strides), norm, down)).to(cuda)


def _bias_before_batchnorm(m, key):
    """the bias of a convolution whose output a training-mode BatchNorm normalises: its gradient is zero in exact arithmetic
    (every convolution bias of a BiFPN is one: `*.1.2.bias` of the fusion blocks, `*.0.bias` of the resampling branches)"""
    if not key.endswith('.bias'):
        return False
    return isinstance(m.get_submodule(key[:-5]), torch.nn.Conv2d)


def _step(m, case, cuda):
    xs_np, gs_np = bc.module_inputs(case)
    xs = [_nhwc(x, cuda).requires_grad_() for x in xs_np]
    ys = m(list(xs))
    torch.autograd.backward(ys, [_nhwc(g, cuda) for g in gs_np])
    torch.cuda.synchronize()
    return xs, ys


@pytest.mark.parametrize('case', list(bc.MODULE_CASES))
def test_module_matches_reference(cuda, case):
    """outputs and eval outputs to 1e-4 of their range; input and parameter gradients, Fusion.weights included, to 1e-3;
    BatchNorm buffers to 1e-4"""
    gold = np.load(os.path.join(GOLD, 'bifpn_module.npz'))
    edges = bc.MODULE_CASES[case][3]
    m = _module(case, cuda).train()
    xs, ys = _step(m, case, cuda)
    assert len(ys) == 4
    for i, e in enumerate(edges):
        s = bc.stored_stride(e)
        assert _rel(ys[i][..., ::s, ::s], gold[f'{case}/out{i}']) < 1e-4, i
        assert _rel(xs[i].grad[..., ::s, ::s], gold[f'{case}/dx{i}']) < 1e-3, i
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        ref = gold[f'{case}/grad/{k}']
        if _bias_before_batchnorm(m, k):
            # zero in exact arithmetic: the reference's value is the rounding residue of a sum that cancels.  Held to 1e-3 of
            # the range of the same convolution's weight gradient, the scale both residues are rounded at.
            scale = float(np.abs(gold[f'{case}/grad/{k[:-4]}weight']).max())
            assert float(np.abs(p.grad.cpu().numpy() - ref).max()) <= 1e-3 * scale, k
        elif np.abs(ref).max() == 0:        # a Fusion weight behind a shut ReLU gate, or in a node whose output nothing reads
            assert float(p.grad.abs().max()) == 0, k
        else:
            assert _rel(p.grad, ref) < 1e-3, k
    for k, v in m.state_dict().items():
        if 'running_' in k:
            assert _rel(v, gold[f'{case}/buffer/{k}']) < 1e-4, k
    m.eval()
    with torch.no_grad():
        ye = m([x.detach() for x in xs])
    for i, e in enumerate(edges):
        s = bc.stored_stride(e)
        assert _rel(ye[i][..., ::s, ::s], gold[f'{case}/eval{i}']) < 1e-4, i


def test_end_to_end_matches_reference(cuda):
    """loss to 1e-4 relative, logits to 1e-3 of their range, gradient digests by the rule of tests/test_deeplab_gpu.py"""
    import ever_amd as er
    from ever_amd.hip import functional as HF
    from oracle import portable
    from oracle.gen_golden import grad_digest
    meta = json.load(open(os.path.join(GOLD, 'bifpn_e2e_r18.json')))
    gold = np.load(os.path.join(GOLD, 'bifpn_e2e_r18.npz'))
    x, y = portable.synthetic_batch(meta['name'], meta['n'], 3, meta['hw'], meta['hw'], meta['num_classes'])
    m = bc.load_portable(bc.BiFPNSeg(er.module), 'bifpn.').to(cuda).train()
    lg = m(_nhwc(x, cuda))
    loss = HF.cross_entropy(lg, torch.from_numpy(y).to(cuda), ignore_index=255)
    loss.backward()
    torch.cuda.synchronize()
    lgn = lg.detach().cpu().numpy()
    st = meta['stride']
    assert _rel(lgn[..., ::st, ::st], gold['logits']) < 1e-3
    assert abs(loss.item() - meta['loss']) <= 1e-4 * abs(meta['loss'])
    # digests (tests/test_deeplab_gpu.py's rules): the norm against the fp64 reference within max(2e-2, 6x the case's worst
    # fp32-vs-fp64 norm deviation); samples and projection within twice the CASE's worst fp32-vs-fp64 deviation.  A convolution
    # bias in front of a training-mode BatchNorm (every one in the BiFPN and the decoder's classifier aside) has a gradient of
    # zero in exact arithmetic — the fp64 reference's norm is below 1e-6 — and is left out of the case's deviation, as the
    # norm rule of that test leaves it out; its own check is the absolute term of the norm rule.
    live = [k for k, v in meta['grads_fp64'].items() if v[0] > 1e-6]
    assert all(k.endswith('.bias') and k.startswith('bifpn.') for k in meta['grads'] if k not in live)
    case = max(float(np.abs(np.asarray(meta['grads'][k]) - np.asarray(meta['grads_fp64'][k]))[[0, 2, 3, 4, 5, 6]].max()
                     / max(abs(meta['grads_fp64'][k][0]), 1e-30)) for k in live)
    case_norm = max(abs(meta['grads'][k][0] - meta['grads_fp64'][k][0]) / meta['grads_fp64'][k][0] for k in live)
    print(f'fp32-vs-fp64 of the reference on this case: digests {case:.2e}, norms {case_norm:.2e}')
    for k, p in m.named_parameters():
        d32, d64 = np.asarray(meta['grads'][k]), np.asarray(meta['grads_fp64'][k])
        got = np.asarray(grad_digest([(k, _OnHost(p))])[k])
        assert abs(got[0] - d64[0]) <= max(2e-2, 6 * case_norm) * abs(d64[0]) + 1e-7, (k, got, d32, d64)
        if k in live:
            keep = [0, 2, 3, 4, 5, 6]       # (the sum grows as sqrt(numel) x the norm: compared through the projection instead)
            _digest_close(got[keep], d32[keep], k, tol=max(2e-3, 2 * case))
    am, margin = gold['argmax'], gold['margin']
    decided = margin > 1e-3 * meta['logit_range']
    assert np.array_equal(lgn.argmax(1)[decided], am[decided])


@pytest.mark.parametrize('norm', ['fast_normalize', 'softmax'])
def test_index_shift_equals_materialised_upsampling(cuda, norm):
    """a shift-1 term against nearest x2 from the unit-weight call followed by shift 0: outputs and all gradients, bit for bit"""
    from ever_amd.hip import functional as HF
    g = torch.Generator().manual_seed(3)
    a = torch.randn((2, 6, 10, 12), generator=g).to(cuda).permute(0, 3, 1, 2)      # [N, C, H, W] over NHWC memory
    b = torch.randn((2, 3, 5, 12), generator=g).to(cuda).permute(0, 3, 1, 2)
    c = torch.randn((2, 6, 10, 12), generator=g).to(cuda).permute(0, 3, 1, 2)
    dy = torch.randn((2, 6, 10, 12), generator=g).to(cuda).permute(0, 3, 1, 2)
    w0 = torch.tensor([0.7, 1.3, -0.2] if norm == 'softmax' else [0.7, 1.3, 0.4])
    runs = []
    for materialise in (False, True):
        ts = [t.clone().requires_grad_() for t in (a, b, c)]
        w = w0.clone().to(cuda).requires_grad_()
        mid = (HF.upsample_nearest2x(ts[1]), 0) if materialise else (ts[1], 1)
        y = HF.weighted_fuse([(ts[0], 0), mid, (ts[2], 0)], w, norm)
        y.backward(dy)
        torch.cuda.synchronize()
        runs.append([y.detach(), w.grad] + [t.grad for t in ts])
    for u, v in zip(*runs):
        assert u.shape == v.shape and torch.equal(u.contiguous().view(torch.int32), v.contiguous().view(torch.int32))
    up = HF.upsample_nearest2x(b)
    assert torch.equal(up, b.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3))


def test_hook_on_an_upsampling_module_sees_its_output_and_changes_no_bit(cuda):
    from ever_amd.hip import functional as HF
    case = 'fast_conv'
    fused = _module(case, cuda).train()
    hooked = copy.deepcopy(fused)
    seen = []
    handle = hooked.upsample_modules[0].register_forward_hook(lambda mod, inp, out: seen.append((inp[0].shape, out.shape)))
    before = dict(HF.wfuse_stats)
    xs_f, ys_f = _step(fused, case, cuda)
    mid = dict(HF.wfuse_stats)
    xs_h, ys_h = _step(hooked, case, cuda)
    after = dict(HF.wfuse_stats)
    handle.remove()
    assert len(seen) == 1 and seen[0][1][-2:] == tuple(2 * e for e in seen[0][0][-2:])
    # fused: three shifted terms in six nodes; hooked: one of them became a node of its own (the unit-weight call)
    assert mid['nodes'] - before['nodes'] == 6 and mid['shifted_terms'] - before['shifted_terms'] == 3
    assert after['nodes'] - mid['nodes'] == 7 and after['shifted_terms'] - mid['shifted_terms'] == 3
    for u, v in zip(ys_f, ys_h):
        assert torch.equal(u, v)
    for u, v in zip(xs_f, xs_h):
        assert torch.equal(u.grad, v.grad)
    for (k, p), (_, q) in zip(fused.named_parameters(), hooked.named_parameters()):
        assert torch.equal(p.grad, q.grad), k
    for (k, u), (_, v) in zip(fused.state_dict().items(), hooked.state_dict().items()):
        assert torch.equal(u, v), k


def test_fused_sgd_steps_move_every_fusion_weight(cuda):
    import ever_amd as er
    torch.manual_seed(5)
    m = er.module.BiFPN(16, [4, 8, 16, 32]).to(cuda).train()
    opt = er.opt.FusedSGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    start = {k: p.detach().clone() for k, p in m.named_parameters() if k.endswith('.weights')}
    assert len(start) == 6
    g = torch.Generator().manual_seed(6)
    for _ in range(3):
        xs = [torch.randn((2, 32 >> i, 32 >> i, 16), generator=g).to(cuda).permute(0, 3, 1, 2) for i in range(4)]
        opt.zero_grad()
        ys = m(xs)
        sum((y * y).mean() for y in ys).backward()
        opt.step()
    torch.cuda.synchronize()
    for k, p in m.named_parameters():
        assert torch.isfinite(p).all(), k
        if k in start:
            assert bool((p.detach() != start[k]).all()), (k, p, start[k])


def test_state_dict_round_trip(cuda):
    import ever_amd as er
    case = 'softmax_maxpool'
    m = _module(case, cuda).train()
    _step(m, case, cuda)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    norm, down, strides, _ = bc.MODULE_CASES[case]
    m2 = er.module.BiFPN(bc.MODULE_C, list(strides), norm, down).to(cuda)
    m2.load_state_dict(sd, strict=True)
    assert list(m2.state_dict()) == list(sd) and all(torch.equal(v, sd[k]) for k, v in m2.state_dict().items())
    m.eval()
    m2.eval()
    xs = [_nhwc(x, cuda) for x in bc.module_inputs(case)[0]]
    with torch.no_grad():
        for u, v in zip(m(list(xs)), m2(list(xs))):
            assert torch.equal(u, v)


def test_channels_off_the_16_byte_grid_raise_with_a_sentence(cuda):
    import ever_amd as er
    from ever_amd.hip import functional as HF
    m = er.module.BiFPN(6, [4, 8, 16, 32]).to(cuda)
    with pytest.raises(HF.HipPathError, match='multiple of 4'):
        m([torch.randn(1, 6, 16 >> i, 16 >> i, device=cuda) for i in range(4)])
    with pytest.raises(ValueError, match='does not fit'):
        HF.weighted_fuse([(torch.zeros(1, 4, 4, 4, device=cuda), 0), (torch.zeros(1, 4, 3, 3, device=cuda), 1)], torch.ones(2, device=cuda))


class _Traceable(torch.nn.Module):
    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, a, b, c, d):
        return tuple(self.m([a, b, c, d]))


def test_trace_of_an_eval_mode_bifpn_replays_the_eager_output(cuda):
    """while the trace is recorded the node evaluates the reference's aten expression (no up-sampling kernel, no fusion kernel
    in the graph); the replay equals the eager forward, which runs the kernels, to fp32 rounding, on a second input too"""
    from ever_amd.hip import functional as HF
    case = 'fast_conv'
    m = _Traceable(_module(case, cuda).eval())
    xs = [_nhwc(x, cuda) for x in bc.module_inputs(case)[0]]
    g = torch.Generator().manual_seed(9)
    xs2 = [torch.randn(tuple(x.permute(0, 2, 3, 1).shape), generator=g).to(cuda).permute(0, 3, 1, 2) for x in xs]
    with torch.no_grad():
        before = HF.wfuse_stats['aten']
        traced = torch.jit.trace(m, tuple(xs), check_trace=False)
        assert HF.wfuse_stats['aten'] - before == 6
        kinds = {n.kind() for n in traced.inlined_graph.nodes()}
        assert 'aten::stack' in kinds and 'aten::upsample_nearest2d' in kinds, kinds
        for inp in (xs, xs2):
            want, got = m(*inp), traced(*inp)
            for u, v in zip(want, got):
                assert _rel(v, u.cpu().numpy()) < 1e-5
