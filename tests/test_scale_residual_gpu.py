"""The layer-scale residual (csrc/layer_scale.hip: y = a + (s[n] gamma[c]) z, the tail of a ConvNeXt block) through the C ABI,
with every output and the workspace NaN-filled inside sentinel-guarded allocations (tests/guard_common.py).

The kernel rounds each product and the sum on its own, in the documented order, so the forward is compared with the fp32
evaluation of a + (s * gamma) * z in torch on the CPU to 1 ulp and dz = (s * gamma) * dy bit for bit; dgamma = sum s dy z
against float64 to 1e-4 max(1, max|ref|) (the project's tolerance for reduced gradients, tests/test_groupnorm_edges_gpu.py)."""
import ctypes

import numpy as np
import pytest
import torch

from tests.guard_common import guarded, guards_intact

pytestmark = pytest.mark.gpu

TOL_GRAD = 1e-4
# (N, HW, C); HW None: from the plan, a lone row on the second grid trip
CASES = {
    'one': (1, 1, 4),
    'c8': (2, 63, 8),
    'c96': (3, 17 * 13, 96),
    'c100': (2, 4096, 100),
    'second_trip_c96': (3, None, 96),
}


def _lib():
    from ever_amd import _C
    return _C.load()


def _call(name, *args):
    from ever_amd import _C
    _C.call(name, *args)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _plan(r, c):
    out = (ctypes.c_int32 * 4)()
    assert _lib().evk_ln_plan(r, c, out) == 0
    return tuple(out)


def _shape(name):
    n, hw, c = CASES[name]
    if hw is None:
        _, _, rows, _ = _plan(1, c)
        cap = _plan(2 ** 40, c)[3]
        total = rows * cap + 1                       # rows of the whole batch
        hw = -(-total // n)
        while (n * hw - 1) // (rows * cap) != 1:      # the last row sits on the second trip (and no third one exists)
            hw -= 1
    return n, hw, c


def _ptr(t):
    return None if t is None else t.data_ptr()


def _fetch(whole, inner, what):
    torch.cuda.synchronize()
    assert guards_intact(whole, inner.numel()), f'{what}: wrote outside its allocation'
    got = inner.cpu()
    assert not bool(torch.isnan(got).any()), f'{what}: {int(torch.isnan(got).sum())} of {got.numel()} elements unwritten'
    return got


def _same_bits(got, ref, what):
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    bad = got.contiguous().view(torch.int32) != ref.contiguous().view(torch.int32)
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} of {bad.numel()} elements differ in their bits'


def _inputs(n, hw, c, seed, has_gamma=True, has_s=True, zero_sample=None):
    gen = torch.Generator().manual_seed(seed)
    a, z, dy = (torch.randn(n, hw, c, generator=gen) for _ in range(3))
    gamma = torch.randn(c, generator=gen) if has_gamma else None
    s = None
    if has_s:
        keep = 0.7
        s = torch.floor(keep + torch.rand(n, generator=gen)) / keep
        s[0] = 1.0 / keep
        if zero_sample is not None:
            s[zero_sample] = 0.0
    return a, z, dy, gamma, s


def _factor(gamma, s, n, c):
    """the fp32 factor s[n] * gamma[c], [N][1][C]"""
    f = torch.ones(n, 1, c)
    if s is not None:
        f = f * s.view(n, 1, 1)
    if gamma is not None:
        f = f * gamma.view(1, 1, c)
    return f


def _run(cuda, a, z, dy, gamma, s, want=('dz', 'dgamma')):
    n, hw, c = z.shape
    d = {k: (None if v is None else v.to(cuda)) for k, v in dict(a=a, z=z, dy=dy, gamma=gamma, s=s).items()}
    yw, yi = guarded(z.numel(), cuda)
    _call('evk_scale_residual_fwd', d['a'].data_ptr(), d['z'].data_ptr(), _ptr(d['gamma']), _ptr(d['s']), yi.data_ptr(), n, hw, c,
          _stream())
    out = dict(y=_fetch(yw, yi, 'y').view(n, hw, c))
    bufs = {k: guarded(z.numel() if k == 'dz' else c, cuda) for k in want}
    nbytes = _lib().evk_scale_residual_bwd_workspace_bytes(n, hw, c) if 'dgamma' in want else 0
    assert 'dgamma' not in want or nbytes == _plan(n * hw, c)[3] * c * 4
    ww, wi = guarded(nbytes // 4, cuda) if nbytes else (None, None)
    _call('evk_scale_residual_bwd', d['dy'].data_ptr(), d['z'].data_ptr(), _ptr(d['gamma']), _ptr(d['s']),
          _ptr(bufs['dz'][1]) if 'dz' in bufs else None, _ptr(bufs['dgamma'][1]) if 'dgamma' in bufs else None, n, hw, c,
          _ptr(wi), nbytes, _stream())
    for k, (w, i) in bufs.items():
        out[k] = _fetch(w, i, k).view(n, hw, c) if k == 'dz' else _fetch(w, i, k)
    if nbytes:
        _fetch(ww, wi, 'workspace')
    return out


def _check(got, a, z, dy, gamma, s, what):
    n, hw, c = z.shape
    f = _factor(gamma, s, n, c)
    y32 = a + f * z                                   # fp32, each operation rounded on its own, the documented order
    ulp = torch.from_numpy(np.spacing(np.abs(y32.numpy()))).double()
    err = ((got['y'].double() - y32.double()).abs() / ulp).max().item()
    print(f'{what}: y within {err:.2f} ulp of the fp32 expression')
    assert err <= 1.0
    y64 = a.double() + f.double() * z.double()
    assert (got['y'].double() - y64).abs().max().item() <= 2e-6 * max(1.0, y64.abs().max().item())
    if 'dz' in got:
        _same_bits(got['dz'], (f * dy).contiguous(), f'{what} dz')
    if 'dgamma' in got:
        sd = torch.ones(n) if s is None else s
        ref = (sd.double().view(n, 1, 1) * dy.double() * z.double()).sum(dim=(0, 1))
        e, scale = (got['dgamma'].double() - ref).abs().max().item(), max(1.0, ref.abs().max().item())
        print(f'{what}: dgamma max err {e:.3e}, bound {TOL_GRAD:g} * {scale:.3e}')
        assert e <= TOL_GRAD * scale


def test_second_trip_case_has_a_lone_row_on_the_second_trip():
    n, hw, c = _shape('second_trip_c96')
    _, _, rows, wgs = _plan(n * hw, c)
    assert wgs == _plan(2 ** 40, c)[3] and rows * wgs < n * hw <= 2 * rows * wgs and n * hw - rows * wgs <= n


@pytest.mark.parametrize('name', list(CASES))
def test_forward_and_backward(cuda, name):
    n, hw, c = _shape(name)
    a, z, dy, gamma, s = _inputs(n, hw, c, 20 + list(CASES).index(name))
    _check(_run(cuda, a, z, dy, gamma, s), a, z, dy, gamma, s, name)


@pytest.mark.parametrize('has_gamma,has_s', [(False, True), (True, False), (False, False)])
def test_null_gamma_and_null_sample_scale(cuda, has_gamma, has_s):
    n, hw, c = _shape('c96')
    a, z, dy, gamma, s = _inputs(n, hw, c, 31, has_gamma, has_s)
    got = _run(cuda, a, z, dy, gamma, s)
    _check(got, a, z, dy, gamma, s, f'gamma {has_gamma} s {has_s}')
    if not has_gamma and not has_s:
        _same_bits(got['y'], a + z, 'y == a + z')
        _same_bits(got['dz'], dy, 'dz == dy')


def test_dropped_sample_passes_the_input_through(cuda):
    n, hw, c = _shape('c96')
    a, z, dy, gamma, s = _inputs(n, hw, c, 41, zero_sample=1)
    got = _run(cuda, a, z, dy, gamma, s)
    _check(got, a, z, dy, gamma, s, 'dropped sample')
    _same_bits(got['y'][1], a[1], 'y == a on the dropped sample')
    assert bool((got['dz'][1] == 0).all()) and bool((got['dz'][0] != 0).any())


def test_each_backward_output_alone_and_second_run(cuda):
    n, hw, c = _shape('second_trip_c96')
    a, z, dy, gamma, s = _inputs(n, hw, c, 51)
    full = _run(cuda, a, z, dy, gamma, s)
    again = _run(cuda, a, z, dy, gamma, s)
    for k in full:
        _same_bits(again[k], full[k], f'second run {k}')
    _same_bits(_run(cuda, a, z, dy, gamma, s, want=('dz',))['dz'], full['dz'], 'dz alone')
    _same_bits(_run(cuda, a, z, dy, gamma, s, want=('dgamma',))['dgamma'], full['dgamma'], 'dgamma alone')


def test_refusals_launch_nothing(cuda):
    lib = _lib()
    x = torch.randn(4 * 16 * 8, device=cuda)
    outs = {k: guarded(m, cuda) for k, m in (('y', x.numel()), ('dz', x.numel()), ('dg', 2056), ('ws', 1024 * 2056))}
    o = {k: v[1] for k, v in outs.items()}

    def fwd(n, hw, c, ap=None):
        return lib.evk_scale_residual_fwd(ap or x.data_ptr(), x.data_ptr(), None, None, o['y'].data_ptr(), n, hw, c, _stream())

    def bwd(n, hw, c, ws_bytes=None):
        return lib.evk_scale_residual_bwd(x.data_ptr(), x.data_ptr(), None, None, o['dz'].data_ptr(), o['dg'].data_ptr(), n, hw,
                                          c, o['ws'].data_ptr(), o['ws'].numel() * 4 if ws_bytes is None else ws_bytes, _stream())
    for n, hw, c in ((4, 16, 0), (4, 16, 6), (4, 16, 2052), (0, 16, 8), (4, 0, 8), (4, -2, 8)):
        assert fwd(n, hw, c) in (-1, -2) and lib.evk_last_error(), (n, hw, c)
        assert bwd(n, hw, c) in (-1, -2), (n, hw, c)
        assert lib.evk_scale_residual_bwd_workspace_bytes(n, hw, c) == 0
    assert fwd(4, 16, 8, ap=x.data_ptr() + 4) == -1                                          # 16-byte alignment
    assert lib.evk_scale_residual_fwd(None, x.data_ptr(), None, None, o['y'].data_ptr(), 4, 16, 8, _stream()) == -1
    assert bwd(4, 16, 8, ws_bytes=lib.evk_scale_residual_bwd_workspace_bytes(4, 16, 8) - 4) == -4
    assert lib.evk_scale_residual_bwd(x.data_ptr(), x.data_ptr(), None, None, None, None, 4, 16, 8, None, 0, _stream()) == -1
    torch.cuda.synchronize()
    for k, (whole, inner) in outs.items():
        assert guards_intact(whole, inner.numel()) and bool(torch.isnan(inner).all()), f'{k}: a refused call wrote'
