"""Convolution geometries the kernels' gathers branch on, through ever_amd.hip.functional.conv2d: y, dx, dw, db against a
float64 convolution in every arithmetic.  The list is that of tests/test_conv_wgrad_gpu.py (odd maps under stride 2, strides
and kernels that differ per axis, padding 0 / beyond "same" / asymmetric, dilation 6 / 12 / 18 with taps wholly in the
padding, stride and dilation together, ragged channel counts) plus what only the Python layer decides: channel padding
(Cin 3 / 5 / 12), narrow outputs (Cout 1 / 6 / 20), the fused ReLU, and one layer that takes the planar weight-gradient path.

Bound (none is new): e = max|hip - ref64| / max|ref64|; y, dx: e <= max(4 e32, 5e-6), dw, db: e <= max(4 e32, 1e-5), e32 being
the same error of torch's fp32 CPU convolution on the same case; the bf16 mode at the grade tests/test_bf16_mode_gpu.py pins."""
import ctypes

import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

BF16_GRADE = 2e-2
PLANES = {'f32': 0, 'bf16': 1, 'f16x2': 2, 'bf16x3': 3}


def _g(name, n, cin, h, w, cout, k, s=1, p=0, dil=1, bias=False, relu=False):
    pair = lambda v: (v, v) if isinstance(v, int) else tuple(v)   # noqa: E731
    return dict(name=name, n=n, cin=cin, h=h, w=w, cout=cout, k=pair(k), s=pair(s), p=pair(p), dil=pair(dil), bias=bias, relu=relu)


CASES = [
    _g('s2_odd', 2, 64, 37, 29, 64, 3, s=2, p=1),
    _g('s2x1', 2, 64, 20, 24, 128, 3, s=(2, 1), p=1, bias=True),
    _g('s1x2', 2, 64, 20, 24, 64, 3, s=(1, 2), p=1),
    _g('k1x7', 2, 64, 16, 24, 64, (1, 7), p=(0, 3)),
    _g('k7x1', 2, 64, 16, 24, 64, (7, 1), p=(3, 0), bias=True),
    _g('k3x1', 1, 64, 257, 1, 128, (3, 1), p=(1, 0)),
    _g('pad0', 2, 128, 18, 18, 128, 3, p=0),
    _g('pad2', 2, 128, 16, 16, 128, 3, p=2, bias=True),
    _g('pad2x0', 2, 64, 16, 16, 64, 3, p=(2, 0)),
    _g('dil6_32', 1, 128, 32, 32, 128, 3, p=6, dil=6),
    _g('dil12_8', 2, 128, 8, 8, 128, 3, p=12, dil=12, bias=True),        # eight of nine taps read nothing but padding
    _g('dil18_4', 2, 128, 4, 4, 128, 3, p=18, dil=18),
    _g('dil18_32', 1, 64, 32, 32, 64, 3, p=18, dil=18),
    _g('aspp_d12', 1, 256, 32, 32, 256, 3, p=12, dil=12),                # the ASPP branch of a 512^2 tile at output stride 16
    _g('dil2_s2', 2, 64, 17, 17, 64, 3, s=2, p=2, dil=2),                # gcd(dil, stride) = 2: the odd residue classes are empty
    _g('dil3_s2', 2, 64, 19, 17, 64, 3, s=2, p=3, dil=3, bias=True),     # gcd 1: every class, taps two apart
    _g('dil2_s4x2', 1, 64, 21, 18, 64, (5, 3), s=(4, 2), p=(4, 2), dil=(2, 2)),
    _g('cin72_cout200', 2, 72, 12, 12, 200, 3, p=1),
    _g('cin200_cout136', 2, 200, 12, 12, 136, 3, p=1, bias=True),
    _g('cout520', 1, 64, 10, 10, 520, 3, p=1, bias=True),
    _g('cout4', 2, 128, 20, 20, 4, 3, p=1, bias=True),
    _g('cin3', 2, 3, 20, 20, 64, 3, p=1),                                # channel padding
    _g('cin5', 2, 5, 20, 20, 32, 3, s=2, p=1, bias=True),
    _g('cin12', 2, 12, 16, 16, 64, 1),
    _g('cout1', 2, 64, 16, 16, 1, 1, bias=True),                         # narrow outputs
    _g('cout6', 2, 64, 16, 16, 6, 3, p=1, bias=True),
    _g('cout20', 2, 64, 16, 16, 20, 3, p=1),
    _g('relu', 2, 64, 16, 16, 64, 3, p=1, bias=True, relu=True),
    _g('relu_dil', 1, 128, 16, 16, 128, 3, p=6, dil=6, relu=True),
    _g('planar_pays', 1, 64, 128, 128, 128, 3, p=1),                     # 128^2 map, Cout >= 128: nine-tap planar weight gradient behind its pack
]
assert len({c['name'] for c in CASES}) == len(CASES)
_REF = {}
WORST = {}


def _rel(a, ref):
    return (a.detach().cpu().double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)


def _inputs(c):
    g = torch.Generator().manual_seed(77 + c['cin'] + 3 * c['cout'] + 5 * c['h'] + 7 * c['k'][0])
    kk = c['cin'] * c['k'][0] * c['k'][1]
    x = torch.randn(c['n'], c['cin'], c['h'], c['w'], generator=g) + 0.5
    wt = (torch.randn(c['cout'], c['cin'], *c['k'], generator=g) + 0.1) / kk ** 0.5
    b = torch.randn(c['cout'], generator=g) if c['bias'] else None
    return g, x, wt, b


def _reference(c, bf16=False):
    """float64 results, the upstream gradient, and the errors of torch's fp32 CPU convolution against them.  With a fused ReLU a
    pre-activation whose sign the arithmetic under test cannot be sure of gets no upstream gradient — one flipped mask moves dx /
    dw / db by a whole term.  fp32-grade arithmetics: |pre| <= 1e-4 max|pre| (twenty times their y bound).  Plain bf16: each
    product carries two operand roundings of 2^-9, so element i is off by at most 2^-8 S_i, S_i = conv(|x|, |w|)_i + |b|: the
    band is |pre_i| <= 2^-8 S_i, per element.  The masked share is printed."""
    if (c['name'], bf16) in _REF:
        return _REF[(c['name'], bf16)]
    g, x, wt, b = _inputs(c)
    res = {}
    gy = None
    for dt in (torch.float64, torch.float32):
        xr, wr = x.to(dt).requires_grad_(), wt.to(dt).requires_grad_()
        br = b.to(dt).requires_grad_() if b is not None else None
        pre = TF.conv2d(xr, wr, br, c['s'], c['p'], c['dil'])
        if gy is None:
            gy = torch.randn(pre.shape, generator=g) + 0.25
            if c['relu']:
                p = pre.detach()
                if bf16:
                    band = 2.0 ** -8 * (TF.conv2d(x.double().abs(), wt.double().abs(), None, c['s'], c['p'], c['dil']) +
                                        (b.double().abs().view(1, -1, 1, 1) if b is not None else 0.0))
                else:
                    band = 1e-4 * p.abs().max()
                keep = p.abs() > band
                print(f"{c['name']}: {1.0 - keep.double().mean().item():.2%} of the pre-activations are too close to the ReLU's kink for {'bf16' if bf16 else 'fp32 grade'}")
                gy = gy * keep.float()
        y = torch.relu(pre) if c['relu'] else pre
        y.backward(gy.to(dt))
        res[dt] = dict(y=y.detach(), dx=xr.grad, dw=wr.grad, db=br.grad if br is not None else None)
    r64, r32 = res[torch.float64], res[torch.float32]
    e32 = {k: _rel(r32[k], r64[k]) for k in r64 if r64[k] is not None}
    _REF[(c['name'], bf16)] = (r64, e32, gy)
    return _REF[(c['name'], bf16)]


def routes(lib, c, planes):
    """(forward kernel, [data-gradient kernel per residue class, '' = no launch]) evk_conv2d_route names for the descriptor
    the Python layer builds: hip/conv.py pads Cin and Cout to multiples of 4 (`_pad4`) and, under the split arithmetics, a Cout
    below 8 to 8 (`narrow8`, which needs an unpadded Cin) — by conv.py's own rule, `conv_channel_padding`"""
    from ever_amd import _C
    from ever_amd.hip.conv import conv_channel_padding
    cin, cout, _ = conv_channel_padding(c['cin'], c['cout'], planes != 0)
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = c['k'], c['s'], c['p'], c['dil']
    ho, wo = (c['h'] + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (c['w'] + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    d = _C.ConvDesc(c['n'], c['h'], c['w'], cin, ho, wo, cout, kh, kw, sh, sw, ph, pw, dh, dw)
    out = []
    for cls in [-1] + list(range(sh * sw)):
        buf = ctypes.create_string_buffer(128)
        assert lib.evk_conv2d_route(ctypes.byref(d), cls, planes, 0, 0, 0, 32, buf, len(buf), None) == 0, lib.evk_last_error()
        out.append(buf.value.decode())
    return out[0], out[1:]


def _run(cuda, c, mode):
    from ever_amd.hip import functional as F
    r64, e32, gy = _reference(c, mode == 'bf16')
    _, x, wt, b = _inputs(c)
    prev = F.set_conv_math(mode)
    try:
        xg = x.to(cuda).requires_grad_(True)
        wg = wt.to(cuda).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        bg = b.to(cuda).requires_grad_(True) if b is not None else None
        yg = F.conv2d(xg, wg, bg, stride=c['s'], padding=c['p'], dilation=c['dil'], relu=c['relu'])
        yg.backward(gy.to(cuda))
        torch.cuda.synchronize()
    finally:
        F.set_conv_math(prev)
    got = dict(y=yg, dx=xg.grad, dw=wg.grad, db=bg.grad if bg is not None else None)
    from ever_amd import _C
    fwd, dgrad = routes(_C.load(), c, PLANES[mode])
    print(f"{c['name']:15s} {mode:6s} fwd {fwd}  dgrad {dgrad}")
    bad = []
    for k in ('y', 'dx', 'dw', 'db'):
        if got[k] is None:
            continue
        assert got[k].shape == r64[k].shape, (k, got[k].shape, r64[k].shape)
        assert torch.isfinite(got[k]).all(), (c['name'], mode, k)
        e = _rel(got[k], r64[k])
        floor = 5e-6 if k in ('y', 'dx') else 1e-5
        bound = BF16_GRADE if (mode == 'bf16' and k != 'db') else max(4 * e32[k], floor)
        print(f"{'':15s} {'':6s} {k:2s} e {e:.2e} / bound {bound:.2e} (e32 {e32[k]:.2e})")
        if e / bound > WORST.get((mode, k), (0.0,))[0]:
            WORST[(mode, k)] = (e / bound, c['name'], f'e {e:.2e} e32 {e32[k]:.2e}')
        if e > bound:
            bad.append((k, e, bound, e32[k]))
    assert not bad, (c['name'], mode, bad)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_conv_geometry_against_fp64(cuda, case, conv_math):
    _run(cuda, case, conv_math)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_conv_geometry_bf16_grade(cuda, case):
    _run(cuda, case, 'bf16')


def test_planar_pays_case_takes_the_production_weight_gradient_path():
    """the one case that is there for the nine-tap planar kernel behind its pack satisfies the Python layer's condition for it"""
    from ever_amd import _C
    from ever_amd.hip import conv as HC
    from ever_amd.hip import functional as F
    c = next(c for c in CASES if c['name'] == 'planar_pays')
    d = _C.ConvDesc(c['n'], c['h'], c['w'], c['cin'], c['h'], c['w'], c['cout'], 3, 3, 1, 1, 1, 1, 1, 1)
    prev = F.set_conv_math('f16x2')
    try:
        assert HC._wgrad_planar_pays(d)
    finally:
        F.set_conv_math(prev)
    buf = ctypes.create_string_buffer(128)
    lib = _C.load()
    assert lib.evk_conv2d_wgrad_route(ctypes.byref(d), 2, 8 | 16 | 32, buf, len(buf), None) == 0 and buf.value == b'conv_wgrad_tr_kernel<9>'


def test_the_cases_cover_the_data_gradient_classes_and_both_3x3_families():
    """Read from evk_conv2d_route for CASES (no launch): a data gradient with stride and dilation together (gcd 1 and gcd > 1),
    an empty residue class, and both families of 3x3 kernels (LDS halo, generic implicit GEMM)."""
    import math
    from ever_amd import _C
    lib = _C.load()
    seen = set()
    for c in CASES:
        for mode, planes in PLANES.items():
            fwd, dgrad = routes(lib, c, planes)
            assert fwd
            strided, dilated = max(c['s']) > 1, max(c['dil']) > 1
            if strided and dilated and any(dgrad):
                seen.add('strided_dilated_gcd1' if all(math.gcd(d_, s_) == 1 for d_, s_ in zip(c['dil'], c['s'])) else 'strided_dilated_gcd>1')
            if '' in dgrad:
                seen.add('empty_class')
            if c['k'] == (3, 3):
                for name in [fwd] + dgrad:
                    if name.startswith('conv3x3_halo_x3_kernel'):
                        seen.add('halo')
                    if name.startswith('conv_igemm_x3'):
                        seen.add('generic')
    assert seen >= {'strided_dilated_gcd1', 'strided_dilated_gcd>1', 'empty_class', 'halo', 'generic'}, seen
    if WORST:
        print('\nworst e / bound per arithmetic and tensor:')
        for (mode, k), (r, name, what) in sorted(WORST.items()):
            print(f'  {mode:7s} {k:2s} {r:5.2f}  ({name}: {what})')
