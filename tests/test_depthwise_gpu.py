"""Depthwise convolution on its own kernels (csrc/depthwise.hip; groups == in == out channels, reference ops.py:25-42):
forward, input / weight / bias gradients against torch's grouped convolution in fp64 on the CPU over the kernels' scope,
bit-identity across the conv-math modes and across runs, large maps (16 x 304 x 128^2; an input above 2 GiB), the
dispatch in `Conv2d` (the block-diagonal path only for grouped convolutions outside the scope), and a depthwise
ConvBlock in training mode (the BatchNorm after it computes its own statistics)."""
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def _nhwc(t, cuda):
    return t.to(cuda).contiguous(memory_format=torch.channels_last)


def _reference(x, w, b, stride, padding, dilation, relu, g):
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    br = b.double().requires_grad_() if b is not None else None
    y = F.conv2d(xr, wr, br, stride, padding, dilation, groups=x.shape[1])
    if relu:
        y = y.relu()
    y.backward(g.double())
    return y.detach(), xr.grad, wr.grad, (br.grad if br is not None else None)


def _hip(cuda, x, w, b, stride, padding, dilation, relu, g):
    from ever_amd.hip import functional as HF
    xg = _nhwc(x, cuda).requires_grad_()
    wg = w.to(cuda).requires_grad_()
    bg = b.to(cuda).requires_grad_() if b is not None else None
    y = HF.depthwise_conv2d(xg, wg, bg, stride, padding, dilation, relu=relu)
    y.backward(_nhwc(g, cuda))
    torch.cuda.synchronize()
    return y.detach(), xg.grad, wg.grad, (bg.grad if bg is not None else None)


def _case(c, k, stride, dil, i):
    """one point of the grid; padding / bias / ReLU / batch / odd sizes cycle with the case index"""
    kh, kw = (1, 3) if k == '1x3' else (k, k)
    same = i % 2 == 0
    pad = (dil * (kh - 1) // 2, dil * (kw - 1) // 2) if same else (0, 0)
    h = 11 + (0 if same else dil * (kh - 1))
    w = 13 + (0 if same else dil * (kw - 1))
    n = 1 if i % 3 == 0 else 3
    return dict(c=c, kh=kh, kw=kw, stride=(stride, stride), pad=pad, dil=(dil, dil), n=n, h=h, w=w, bias=i % 4 < 2,
                relu=i % 5 == 1)


GRID = [_case(c, k, s, d, i) for i, (c, k, s, d) in
        enumerate(itertools.product((4, 32, 304), (3, 5, 7, '1x3'), (1, 2), (1, 2, 6)))]


def _tensors(p, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(p['n'], p['c'], p['h'], p['w'], generator=gen)
    wt = torch.randn(p['c'], 1, p['kh'], p['kw'], generator=gen) * 0.3
    b = torch.randn(p['c'], generator=gen) if p['bias'] else None
    ho = (p['h'] + 2 * p['pad'][0] - p['dil'][0] * (p['kh'] - 1) - 1) // p['stride'][0] + 1
    wo = (p['w'] + 2 * p['pad'][1] - p['dil'][1] * (p['kw'] - 1) - 1) // p['stride'][1] + 1
    g = torch.randn(p['n'], p['c'], ho, wo, generator=gen)
    return x, wt, b, g


@pytest.mark.parametrize('p', GRID, ids=[f"c{p['c']}-k{p['kh']}x{p['kw']}-s{p['stride'][0]}-d{p['dil'][0]}-p{p['pad'][0]}"
                                          f"-n{p['n']}{'-b' if p['bias'] else ''}{'-relu' if p['relu'] else ''}" for p in GRID])
def test_depthwise_matches_fp64(cuda, p):
    x, w, b, g = _tensors(p, p['c'] * 7 + p['kh'] * 3 + p['dil'][0])
    args = (p['stride'], p['pad'], p['dil'], p['relu'], g)
    ref = _reference(x, w, b, *args)
    got = _hip(cuda, x, w, b, *args)
    assert got[0].shape == ref[0].shape
    assert _rel(got[0], ref[0]) < 2e-6
    assert _rel(got[1], ref[1]) < 2e-6
    assert got[2].shape == w.shape and _rel(got[2], ref[2]) < 5e-6
    if b is not None:
        assert _rel(got[3], ref[3]) < 5e-6


def test_same_bits_in_every_conv_math_mode_and_run(cuda):
    from ever_amd.hip import functional as HF
    prev = HF.get_conv_math()
    try:
        for p in (GRID[0], GRID[30], GRID[-1], _case(304, 3, 1, 1, 2)):
            x, w, b, g = _tensors(p, 5)
            args = (p['stride'], p['pad'], p['dil'], p['relu'], g)
            first = None
            for mode in ('f16x2', 'bf16x3', 'f32', 'bf16', 'f16x2'):
                HF.set_conv_math(mode)
                out = _hip(cuda, x, w, b, *args)
                if first is None:
                    first = out
                for a, r in zip(out, first):
                    assert (a is None and r is None) or torch.equal(a, r), mode
    finally:
        HF.set_conv_math(prev)


def test_large_map_against_fp64_on_a_slice(cuda):
    """16 x 304 x 128^2, 3x3 (the first separable block of the DeepLabv3+ decoder at 512^2 tiles): y and dx of a two-image
    slice of the full-size run against fp64; dw / db of a run on that slice against fp64"""
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(16, 304, 128, 128, generator=gen)
    w = torch.randn(304, 1, 3, 3, generator=gen) * 0.3
    b = torch.randn(304, generator=gen)
    g = torch.randn(16, 304, 128, 128, generator=gen)
    got = _hip(cuda, x, w, b, 1, 1, 1, False, g)
    sl = slice(5, 7)
    ref = _reference(x[sl], w, b, 1, 1, 1, False, g[sl])
    assert _rel(got[0][sl], ref[0]) < 2e-6 and _rel(got[1][sl], ref[1]) < 2e-6
    part = _hip(cuda, x[sl], w, b, 1, 1, 1, False, g[sl])
    assert _rel(part[2], ref[2]) < 5e-6 and _rel(part[3], ref[3]) < 5e-6


def test_input_above_2gib(cuda):
    """1 x 32 x 4096 x 4160 fp32 (2.18 GB): the output and input-gradient rows past the 2 GiB byte offset of x
    against fp64 on a crop (64-bit element offsets)"""
    from ever_amd.hip import functional as HF
    n, c, h, wd = 1, 32, 4096, 4160
    assert n * c * h * wd * 4 > 2 ** 31
    gen = torch.Generator(device=cuda).manual_seed(11)
    x = torch.randn(n, h, wd, c, device=cuda, generator=gen).permute(0, 3, 1, 2).requires_grad_()
    w = (torch.randn(c, 1, 3, 3, device=cuda, generator=gen) * 0.3).requires_grad_()
    y = HF.depthwise_conv2d(x, w, None, 1, 1, 1)
    g = torch.randn(n, h, wd, c, device=cuda, generator=gen).permute(0, 3, 1, 2)
    y.backward(g)
    torch.cuda.synchronize()
    r0 = (2 ** 31) // (4 * wd * c) - 2          # a few rows before the boundary, through the last row
    wr = w.detach().double().cpu()
    xc = F.pad(x.detach()[:, :, r0 - 1:, :].double().cpu(), (1, 1, 0, 1))
    yref = F.conv2d(xc, wr, groups=c)
    assert yref.shape[2] == h - r0
    assert _rel(y[:, :, r0:, :], yref) < 2e-6
    gc = F.pad(g[:, :, r0 - 1:, :].double().cpu(), (1, 1, 0, 1))
    dxref = F.conv2d(gc, wr.flip(2, 3), groups=c)
    assert _rel(x.grad[:, :, r0:, :], dxref) < 2e-6
    assert bool(torch.isfinite(w.grad).all())


class _Dense(RuntimeError):
    pass


def test_dispatch(cuda, monkeypatch):
    """a depthwise Conv2d never builds the block-diagonal weight; a ResNeXt-style grouped convolution still does"""
    import ever_amd as er
    from ever_amd.hip import functional as HF

    def refuse(weight, groups):
        raise _Dense(groups)

    monkeypatch.setattr(HF, 'grouped_dense_weight', refuse)
    dwc = er.module.Conv2d(32, 32, 3, 1, 1, groups=32).to(cuda)
    x = torch.randn(2, 32, 20, 24, device=cuda).contiguous(memory_format=torch.channels_last).requires_grad_()
    dwc(x).sum().backward()
    assert dwc.weight.grad is not None and x.grad is not None
    for conv in (er.module.Conv2d(128, 128, 3, 1, 1, groups=32), er.module.Conv2d(32, 64, 3, 1, 1, groups=32),
                 er.module.Conv2d(32, 32, 3, 3, 1, groups=32), er.module.Conv2d(32, 32, 9, 1, 4, groups=32)):
        conv = conv.to(cuda)
        with pytest.raises(_Dense):
            conv(torch.randn(2, conv.in_channels, 20, 24, device=cuda))
    odd = er.module.Conv2d(6, 6, 3, 1, 1, groups=6).to(cuda)          # C % 4 != 0
    with pytest.raises(_Dense):
        odd(torch.randn(2, 6, 20, 24, device=cuda))


def test_depthwise_convblock_trains_like_fp64(cuda):
    import ever_amd as er
    torch.manual_seed(4)
    c = 64
    blk = er.module.ConvBlock(c, c, 3, 1, 1, groups=c).to(cuda).train()
    ref = torch.nn.Sequential(torch.nn.Conv2d(c, c, 3, 1, 1, groups=c, bias=False), torch.nn.BatchNorm2d(c),
                              torch.nn.ReLU()).double().train()
    ref.load_state_dict({k: v.double().cpu() for k, v in blk.state_dict().items()})
    x = torch.randn(3, c, 33, 35)
    y = blk(_nhwc(x, cuda))
    yr = ref(x.double())
    torch.cuda.synchronize()
    assert _rel(y, yr.detach()) < 2e-5
    assert _rel(blk[1].running_mean, ref[1].running_mean) < 1e-5
    assert _rel(blk[1].running_var, ref[1].running_var) < 1e-5


@pytest.mark.parametrize('relu', (False, True), ids=['plain', 'relu'])
def test_mixed_requires_grad_gives_the_same_bits_and_none_elsewhere(cuda, relu):
    """x only (no workspace, x not saved), weight only, bias only: each gradient equals the all-gradients call's bit for bit"""
    from ever_amd.hip import functional as HF
    p = dict(c=96, kh=3, kw=5, stride=(2, 1), pad=(1, 3), dil=(1, 2), n=2, h=13, w=18, bias=True, relu=relu)
    x, w, b, g = _tensors(p, 21)
    full = _hip(cuda, x, w, b, p['stride'], p['pad'], p['dil'], relu, g)
    ref = _reference(x, w, b, p['stride'], p['pad'], p['dil'], relu, g)
    for a, r, tol in zip(full, ref, (2e-6, 2e-6, 5e-6, 5e-6)):
        assert _rel(a, r) < tol
    for which in range(3):
        leaves = [_nhwc(x, cuda), w.to(cuda), b.to(cuda)]
        leaves[which].requires_grad_()
        y = HF.depthwise_conv2d(*leaves, p['stride'], p['pad'], p['dil'], relu=relu)
        y.backward(_nhwc(g, cuda))
        torch.cuda.synchronize()
        assert torch.equal(y.detach(), full[0])
        for i, leaf in enumerate(leaves):
            if i == which:
                assert leaf.grad is not None and leaf.grad.shape == leaf.shape and torch.equal(leaf.grad, full[1 + i]), which
            else:
                assert leaf.grad is None
    # no gradient at all: the output does not require one
    assert not HF.depthwise_conv2d(_nhwc(x, cuda), w.to(cuda), b.to(cuda), p['stride'], p['pad'], p['dil'], relu=relu).requires_grad


def test_non_dense_weight_view(cuda):
    """a [C, 1, 3, 3] view with strides (18, 18, 6, 2): as a view of a parameter (the gradient reaches the parameter, zero between
    the taps) and as a leaf of its own (the gradient has the leaf's shape)"""
    from ever_amd.hip import functional as HF
    c = 32
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(2, c, 9, 11, generator=gen)
    base = torch.randn(c, 1, 3, 6, generator=gen) * 0.3
    g = torch.randn(2, c, 9, 11, generator=gen)
    ref = _reference(x, base[..., ::2].contiguous(), None, 1, 1, 1, False, g)
    param = base.to(cuda).requires_grad_()
    view = param[..., ::2]
    assert not view.is_contiguous() and view.shape == (c, 1, 3, 3)
    y = HF.depthwise_conv2d(_nhwc(x, cuda), view, None, 1, 1, 1)
    y.backward(_nhwc(g, cuda))
    torch.cuda.synchronize()
    assert _rel(y.detach(), ref[0]) < 2e-6
    assert param.grad.shape == param.shape and bool((param.grad[..., 1::2] == 0).all())
    assert _rel(param.grad[..., ::2], ref[2]) < 5e-6
    leaf = base.to(cuda)[..., ::2].detach().requires_grad_()
    assert leaf.stride() == (18, 18, 6, 2)
    HF.depthwise_conv2d(_nhwc(x, cuda), leaf, None, 1, 1, 1).backward(_nhwc(g, cuda))
    torch.cuda.synchronize()
    assert leaf.grad.shape == leaf.shape and torch.equal(leaf.grad, param.grad[..., ::2])


def test_broadcast_hw_backward_matches_fp64(cuda):
    """the adjoint of the 1x1-map broadcast: dx[n][c] = sum over the pixels of g; at most ceil(HW / 32) + 32 roundings, each
    relative to a partial sum of magnitude <= sum |g| (sum_hw_kernel: 32 pixel slices per channel group at C / 4 >= 8)"""
    from ever_amd.hip import functional as HF
    n, c, h, w = 3, 36, 17, 23
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(n, c, 1, 1, generator=gen)
    g = torch.randn(n, c, h, w, generator=gen)
    xg = x.to(cuda).requires_grad_()
    y = HF.broadcast_hw(xg, (h, w))
    assert y.shape == (n, c, h, w) and torch.equal(y.detach().cpu(), x.expand(n, c, h, w))
    y.backward(_nhwc(g, cuda))
    torch.cuda.synchronize()
    want = g.double().sum((2, 3), keepdim=True)
    bound = (-(-h * w // 32) + 32) * 2.0 ** -24 * g.double().abs().sum((2, 3), keepdim=True)
    assert xg.grad.shape == x.shape and bool(((xg.grad.double().cpu() - want).abs() <= bound).all())
