"""The FS-Relation scene MLPs as one node of five launches (csrc/relation_scene.hip, hip/pointwise.py: scene_mlp, module/
fs_relation.py: _scene_embeddings; reference fs_relation.py:23-29,56-60).  The forward is bit-identical to the layer path
(EVK_SCENE_MLP=0: conv1x1_smallm_kernel, whose body it shares); every backward output is held against an fp64 evaluation of its
formula on the kernel's own fp32 inputs under the a-priori bound |got - ref| <= gamma_T sum|a_t b_t|, gamma_T = T u / (1 - T u),
u = 2^-24, T = length of the sum + 2 (any order, with or without FMA); the sums have one order (two runs, another stream: same
bits); the module takes the fused path only for plain MLPs nobody watches, in training, on supported shapes."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _gamma(t):
    return t * U / (1.0 - t * U)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


_MLPS = {}


def _mlps(cuda, k, c, levels):
    """`levels` scene encoders Conv2d(k, c, 1) -> ReLU -> Conv2d(c, c, 1), built once per (k, c) and never written"""
    from ever_amd.module.fs_relation import _mlp
    if (k, c) not in _MLPS:
        torch.manual_seed(1000 * k + c)
        _MLPS[(k, c)] = [_mlp(k, c).to(cuda).train() for _ in range(8)]
    return _MLPS[(k, c)][:levels]


# ------------------------------------------------------------------------------------------ 1. forward bit-identity
@pytest.mark.parametrize('n', [1, 3, 16, 32])
def test_forward_has_the_bits_of_the_layer_path(cuda, n):
    from ever_amd.hip import functional as HF
    g = torch.Generator().manual_seed(n)
    for k in (8, 100, 1028, 2048):         # 1028: K / 4 = 257, one chunk past the 256-thread stride
        s = torch.randn(n, k, 1, 1, generator=g).to(cuda).requires_grad_()
        for c in (4, 96, 256):
            for levels in (1, 4, 8):
                mlps = _mlps(cuda, k, c, levels)
                fused = HF.scene_mlp(s, mlps)
                with torch.no_grad():
                    layer = [m(s) for m in mlps]
                assert len(fused) == levels
                for a, b in zip(fused, layer):
                    assert a.shape == b.shape == (n, c, 1, 1) and HF.is_nhwc(a)
                    assert torch.equal(_bits(a), _bits(b)), (n, k, c, levels)


def test_forward_bits_with_exact_zeros_and_negatives_in_front_of_the_relu(cuda):
    from ever_amd.hip import functional as HF
    from ever_amd.module.fs_relation import _mlp
    g = torch.Generator().manual_seed(77)
    n, k, c = 16, 8, 96
    mlps = [_mlp(k, c).to(cuda).train() for _ in range(4)]
    with torch.no_grad():
        for m in mlps:
            m[0].weight.copy_(torch.randint(-2, 3, (c, k, 1, 1), generator=g).float())
            m[0].bias.zero_()
    s = torch.randint(-3, 4, (n, k, 1, 1), generator=g).float().to(cuda).requires_grad_()
    pre = [s.detach().double().reshape(n, k) @ m[0].weight.detach().double().reshape(c, k).t() for m in mlps]
    assert all(bool((p == 0).any()) and bool((p < 0).any()) and bool((p > 0).any()) for p in pre)
    fused = HF.scene_mlp(s, mlps)
    with torch.no_grad():
        layer = [m(s) for m in mlps]
        hidden = [m[0](s, relu=True) for m in mlps]
    for a, b, hd, p in zip(fused, layer, hidden, pre):
        assert torch.equal(_bits(a), _bits(b))
        assert torch.equal(hd.reshape(n, c).double(), p.clamp_min(0))       # (integers: the hidden layer is exact)


# ------------------------------------------------------------------------------------------ 2. + 3. backward
def _backward_case(cuda, levels, n, k, c, seed, drop_level=None):
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(cuda)
    t = dict(s=rnd(n, k), h=rnd(levels, n, c).clamp_min(0),                 # about half of h is exactly zero
             g=[None if l == drop_level else rnd(n, c) for l in range(levels)],
             w1=[rnd(c, k) * 0.1 for _ in range(levels)], w2=[rnd(c, c) * 0.1 for _ in range(levels)])
    assert bool((t['h'] == 0).any()) and bool((t['h'] > 0).any())
    return t


def _run_backward(t, stream=None):
    from ever_amd import _C
    from ever_amd.hip.pointwise import _scene_ptrs
    levels, n, c = t['h'].shape
    k = t['s'].shape[1]
    dev = t['s'].device
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
        out = dict(dh=torch.full((levels, n, c), float('nan'), device=dev), ds=torch.full((n, k), float('nan'), device=dev),
                   dw1=[torch.full((c, k), float('nan'), device=dev) for _ in range(levels)],
                   db1=[torch.full((c,), float('nan'), device=dev) for _ in range(levels)],
                   dw2=[torch.full((c, c), float('nan'), device=dev) for _ in range(levels)],
                   db2=[torch.full((c,), float('nan'), device=dev) for _ in range(levels)])
        nbytes = _C.load().evk_relation_scene_bwd_workspace_bytes(levels, n, k, c)
        assert nbytes > 0 and nbytes % (n * k * 4) == 0 and nbytes // (n * k * 4) <= 64
        ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
        _C.call('evk_relation_scene_bwd', t['s'].data_ptr(), t['h'].data_ptr(), _scene_ptrs(t['g']), _scene_ptrs(t['w1']),
                _scene_ptrs(t['w2']), out['dh'].data_ptr(), out['ds'].data_ptr(), _scene_ptrs(out['dw1']), _scene_ptrs(out['db1']),
                _scene_ptrs(out['dw2']), _scene_ptrs(out['db2']), levels, n, k, c, ws.data_ptr(), nbytes,
                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out


def _flat(out):
    return [out['dh'], out['ds']] + out['dw1'] + out['db1'] + out['dw2'] + out['db2']


def _within(got, ref, mag, t, what):
    """|got - ref| <= gamma_t * mag elementwise (mag = sum |a b| of that element's sum, fp64)"""
    err = (got.double() - ref).abs()
    bound = _gamma(t) * mag
    worst = float((err - bound).max())
    print(f'{what}: max err {float(err.max()):.3e}, max bound {float(bound.max()):.3e}')
    assert bool((err <= bound).all()), (what, worst)


# (levels, n, k, c): bench-like; the smallest; ragged column / row tiles, K / 4 = 257, slices that cross levels with a short
# last one; a second, ragged half of the 16 rows B2 holds in registers; C = 256 (four column tiles, 64 rows of W2 per wave)
_CASES = [(4, 16, 512, 64), (1, 1, 8, 4), (8, 32, 1028, 96), (2, 17, 12, 8), (3, 3, 100, 256)]


@pytest.mark.parametrize('levels,n,k,c', _CASES)
def test_backward_against_fp64_within_the_a_priori_bound(cuda, levels, n, k, c):
    t = _backward_case(cuda, levels, n, k, c, seed=levels * 100 + n, drop_level=1 if levels > 1 else None)
    out = _run_backward(t)
    assert all(bool(torch.isfinite(x).all()) for x in _flat(out))
    s, h = t['s'].double(), t['h'].double()
    dhl = out['dh'].double()                      # B2 and B3 are fed the dh the library produced
    ds_ref, ds_mag = torch.zeros_like(s), torch.zeros_like(s)
    for l in range(levels):
        g = (t['g'][l] if t['g'][l] is not None else torch.zeros(n, c, device=s.device)).double()
        w1, w2 = t['w1'][l].double(), t['w2'][l].double()
        _within(out['dw2'][l], g.t() @ h[l], g.abs().t() @ h[l].abs(), n + 2, f'dW2[{l}]')
        _within(out['db2'][l], g.sum(0), g.abs().sum(0), n + 2, f'db2[{l}]')
        mask = (h[l] > 0).double()                # h == 0 -> gradient 0, as torch.relu
        _within(out['dh'][l], mask * (g @ w2), g.abs() @ w2.abs(), c + 2, f'dh[{l}]')
        assert bool((out['dh'][l][h[l] == 0] == 0).all())
        _within(out['dw1'][l], dhl[l].t() @ s, dhl[l].abs().t() @ s.abs(), n + 2, f'dW1[{l}]')
        _within(out['db1'][l], dhl[l].sum(0), dhl[l].abs().sum(0), n + 2, f'db1[{l}]')
        ds_ref += dhl[l] @ w1
        ds_mag += dhl[l].abs() @ w1.abs()
    _within(out['ds'], ds_ref, ds_mag, levels * c + 2, 'ds')


def test_backward_has_one_summation_order(cuda):
    t = _backward_case(cuda, 4, 16, 512, 64, seed=5, drop_level=2)
    a, b = _run_backward(t), _run_backward(t)
    other = torch.cuda.Stream(cuda)
    other.wait_stream(torch.cuda.current_stream())
    c = _run_backward(t, stream=other)
    for x, y, z in zip(_flat(a), _flat(b), _flat(c)):
        assert torch.equal(_bits(x), _bits(y)) and torch.equal(_bits(x), _bits(z))


# ------------------------------------------------------------------------------------------ 4. + 5. the module
def _relation(cuda, scale_aware):
    import ever_amd as er
    torch.manual_seed(9)
    m = er.module.fs_relation.FSRelation(512, (64, 64, 64, 64), 64, scale_aware_proj=scale_aware).to(cuda).train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            torch.nn.init.uniform_(mod.weight, 0.5, 1.5)
            torch.nn.init.uniform_(mod.bias, -0.3, 0.3)
    return m


def _inputs(cuda, n=3):
    g = torch.Generator().manual_seed(3)
    scene = (torch.randn(n, 512, 1, 1, generator=g) * 0.1)
    feats = [(torch.randn(n, 64, 24 >> i, 32 >> i, generator=g) + 0.2) for i in range(4)]
    ws = [torch.randn(n, 64, 24 >> i, 32 >> i, generator=g) for i in range(4)]
    return scene, feats, ws


def _step(m, scene, feats, ws, dev, dtype=torch.float32, grad=True):
    for mod in m.modules():
        if hasattr(mod, 'reset_running_stats'):
            mod.reset_running_stats()
            mod._nbt_pending = 0
    m.zero_grad(set_to_none=True)
    sc = scene.to(dev, dtype).requires_grad_(bool(grad))        # grad='scene': only the scene wants one, forward only
    fs = [f.to(dev, dtype).contiguous(memory_format=torch.channels_last).requires_grad_(grad is True) for f in feats]
    outs = m(sc, fs)
    if grad is not True:
        return [o.detach() for o in outs], None, {}
    sum((o * w.to(dev, dtype)).sum() for o, w in zip(outs, ws)).backward()
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    return [o.detach() for o in outs], sc.grad, {k: p.grad.clone() for k, p in m.named_parameters()}


def _spy(monkeypatch):
    from ever_amd.hip import functional as HF
    calls, orig = [], HF.scene_mlp

    def spy(scene, mlps):
        calls.append(len(mlps))
        return orig(scene, mlps)
    monkeypatch.setattr(HF, 'scene_mlp', spy)
    return calls


@pytest.mark.parametrize('scale_aware', [True, False], ids=['scale_aware', 'one_mlp'])
def test_module_same_outputs_and_gradients_no_worse_than_the_layer_path(cuda, monkeypatch, scale_aware):
    """Outputs bit-equal; the scene-input gradient and every parameter gradient against an fp64 torch.nn copy of the module:
    the fused path's error (max |got - ref| / max |ref|) is at most twice the layer path's, the parent behaviour."""
    from oracle import farseg_ref
    m = _relation(cuda, scale_aware)
    scene, feats, ws = _inputs(cuda)
    ref = farseg_ref.FSRelationRef(512, (64, 64, 64, 64), 64, scale_aware_proj=scale_aware).double().train()
    ref.load_state_dict({k: v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()
                         for k, v in m.state_dict().items()})
    _, s_ref, p_ref = _step(ref, scene, feats, ws, torch.device('cpu'), torch.float64)
    calls = _spy(monkeypatch)
    monkeypatch.setenv('EVK_SCENE_MLP', '1')
    o1, s1, p1 = _step(m, scene, feats, ws, cuda)
    assert calls == [4 if scale_aware else 1]
    monkeypatch.setenv('EVK_SCENE_MLP', '0')
    o0, s0, p0 = _step(m, scene, feats, ws, cuda)
    assert calls == [4 if scale_aware else 1]
    for a, b in zip(o1, o0):
        assert torch.equal(_bits(a), _bits(b))
    for k, w in m.named_parameters():         # AccumulateGrad stored the fused gradients as they came: the parameter's strides
        assert p1[k].stride() == w.stride(), k

    def err(got, want):
        want = want.to(got.device)
        return float((got.double() - want).abs().max() / want.abs().max().clamp_min(1e-300))
    rows = [('scene', err(s1, s_ref), err(s0, s_ref))] + [(k, err(p1[k], p_ref[k]), err(p0[k], p_ref[k])) for k in p_ref]
    for k, e1, e0 in rows:
        print(f'parity scale_aware_proj={scale_aware} {k}: fused {e1:.3e} layer {e0:.3e}')
    for k, e1, e0 in rows:
        if k.endswith('.0.bias') and ('content_encoders' in k or 'feature_reencoders' in k):
            continue      # (in front of a training-mode BatchNorm: the true gradient is zero, both paths hold rounding noise)
        assert e1 <= 2.0 * e0, (k, e1, e0)


def test_module_keeps_the_layer_path_where_it_must(cuda, monkeypatch):
    import ever_amd as er
    m = _relation(cuda, True)
    scene, feats, ws = _inputs(cuda)
    calls = _spy(monkeypatch)

    def both(model, sc=scene, fts=feats, wts=ws, grad=True):
        """(as the model routes it, with the switch off): the results of the two runs"""
        monkeypatch.setenv('EVK_SCENE_MLP', '1')
        a = _step(model, sc, fts, wts, cuda, grad=grad)
        monkeypatch.setenv('EVK_SCENE_MLP', '0')
        return a, _step(model, sc, fts, wts, cuda, grad=grad)

    def same(a, b):
        assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a[0], b[0]))
        assert (a[1] is None and b[1] is None) or torch.equal(_bits(a[1]), _bits(b[1]))
        assert a[2].keys() == b[2].keys() and all(torch.equal(_bits(a[2][k]), _bits(b[2][k])) for k in a[2])
    # a forward hook on one encoder
    seen = []
    hook = m.scene_encoder[2].register_forward_hook(lambda mod, i, o: seen.append(tuple(o.shape)))
    same(*both(m))
    hook.remove()
    assert calls == [] and seen == [(3, 64, 1, 1)] * 2
    # more rows than the kernels take
    g = torch.Generator().manual_seed(4)
    sc33 = torch.randn(33, 512, 1, 1, generator=g) * 0.1
    f33 = [torch.randn(33, 64, 4, 4, generator=g) for _ in range(4)]
    same(*both(m, sc33, f33, [torch.ones_like(f) for f in f33]))
    assert calls == []
    # eval mode and no-grad
    m.eval()
    same(*both(m, grad='scene'))
    m.train()
    with torch.no_grad():
        same(*both(m, grad=False))
    assert calls == []
    # a convolution without bias
    nb = _relation(cuda, True)
    nb.scene_encoder[1][0] = er.module.Conv2d(512, 64, 1, bias=False).to(cuda)
    same(*both(nb))
    assert calls == []
    # and the plain module does take it
    both(m)
    assert calls == [4]


# ------------------------------------------------------------------------------------------ 6. captured step
def test_captured_step_equals_the_eager_step_with_the_fused_branch(cuda, monkeypatch):
    from tests.test_graph_gpu import _run
    from ever_amd.hip import functional as F
    monkeypatch.setenv('EVK_SCENE_MLP', '1')
    calls = _spy(monkeypatch)
    prev = F.set_conv_math('f16x2')
    try:
        le, se, be = _run(cuda, False, steps=5)
        eager_calls = len(calls)
        lg, sg, bg = _run(cuda, True, steps=5)       # three eager steps, the capture, replays
    finally:
        F.set_conv_math(prev)
    assert eager_calls == 5 and len(calls) > eager_calls
    assert le == lg, (le, lg)
    assert not [k for k in se if not torch.equal(se[k], sg[k])]
    assert all(torch.equal(a, b) for a, b in zip(be, bg))
