"""Row LayerNorm (csrc/layernorm.hip) at the edges of its thread plan, called directly through the C ABI.  Every output (y,
save_mean, save_rstd, dx, dgamma, dbeta) is a NaN-filled slice of a sentinel-guarded allocation (tests/guard_common.py) and so
is the workspace, at exactly evk_ln_bwd_workspace_bytes: an element nobody wrote stays NaN, a store beside a slice or past the
workspace breaks a sentinel.

Reference: the definition in float64 torch on the CPU from the same fp32 inputs — per-row mean and biased variance,
y = (x - mean) * rstd * gamma + beta — and autograd on it.

Tolerances: the project's own for the normalisation kernels (tests/test_groupnorm_edges_gpu.py): y to 1e-5 max(1, max|ref|),
gradients to 1e-4 max(1, max|ref|), save_mean to 1e-6 max(1, |mean|), save_rstd to 1e-5 relative; inputs zero-mean,
unit-scale, eps = 1e-6 (ConvNeXt's).

Rows with a large common offset (1000 + 2 n(0,1)) are measured against aten's own fp32 F.layer_norm on the CPU, both against
float64: the kernel must stay within 2x aten's error.  Constant rows whose constant has few enough mantissa bits for every
partial sum of the row to be exact (at most 11 bits here, rows of at most 2048) have variance exactly 0: y == beta bit for
bit, save_mean is the constant, save_rstd is 1 / sqrt(eps) to 1 ulp."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.guard_common import guarded, guards_intact

pytestmark = pytest.mark.gpu

EPS = float(np.float32(1e-6))        # the kernels take eps as a float
TOL_Y, TOL_GRAD, TOL_MEAN, TOL_RSTD = 1e-5, 1e-4, 1e-6, 1e-5

# (R, C) — what each is here for; R None: taken from the plan inside the test
CASES = {
    'one_lane': (1, 4),                  # L = 1, one row
    'r3_c8': (3, 8),
    'c96_ragged': (257, 96),             # L < 64, several rows per wave, a ragged last workgroup
    'c100_masked': (65, 100),            # C / 4 = 25: a masked column
    'c1536': (33, 1536),                 # L = 64 x 6 columns
    'c2048': (5, 2048),                  # L = 64 x 8 columns: the cap
    'c384': (1000, 384),
    'second_trip_c8': (None, 8),         # rows-per-trip x workgroups + 1: a lone row on the second grid trip
    'second_trip_c96': (None, 96),
    'wg_minus_1_c96': (None, 96),        # rows-per-workgroup - 1 and + 1
    'wg_plus_1_c96': (None, 96),
    'wg_minus_1_c1536': (None, 1536),
    'wg_plus_1_c1536': (None, 1536),
}
AFFINE = ('both', 'gamma', 'beta', 'none')


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
    return tuple(out)       # lanes, columns, rows per workgroup per trip, workgroups


def _shape(name):
    r, c = CASES[name]
    if r is None:
        _, _, rows, _ = _plan(1, c)
        cap = _plan(2 ** 40, c)[3]
        r = rows * cap + 1 if name.startswith('second_trip') else (rows - 1 if 'minus' in name else rows + 1)
    return r, c


def _ptr(t):
    return None if t is None else t.data_ptr()


def _fetch(whole, inner, what, nan_ok=False):
    torch.cuda.synchronize()
    assert guards_intact(whole, inner.numel()), f'{what}: wrote outside its allocation'
    got = inner.cpu()
    assert nan_ok or not bool(torch.isnan(got).any()), f'{what}: {int(torch.isnan(got).sum())} of {got.numel()} elements unwritten'
    return got


def _same_bits(got, ref, what):
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    bad = got.contiguous().view(torch.int32) != ref.contiguous().view(torch.int32)
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} of {bad.numel()} elements differ in their bits'


def _close(got, ref, tol, what):
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), f'{what}: not finite'
    err, scale = (got - ref).abs().max().item(), max(1.0, ref.abs().max().item())
    print(f'{what}: max err {err:.3e}, bound {tol:g} * {scale:.3e}')
    assert err <= tol * scale, f'{what}: max err {err:.3e} > {tol:g} * {scale:.3e}'


def _inputs(r, c, seed, affine='both'):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(r, c, generator=gen)
    gamma, beta = torch.randn(c, generator=gen), torch.randn(c, generator=gen)
    dy = torch.randn(r, c, generator=gen)
    return x, (gamma if affine in ('both', 'gamma') else None), (beta if affine in ('both', 'beta') else None), dy


_REF = {}


def _reference(key, x, gamma, beta, dy):
    """float64 definition and its gradients (dgamma / dbeta as if gamma = 1 / beta = 0 where absent); computed once per key"""
    if key in _REF:
        return _REF[key]
    c = x.shape[1]
    xd = x.double().requires_grad_(True)
    gm = (torch.ones(c) if gamma is None else gamma).double().requires_grad_(True)
    bt = (torch.zeros(c) if beta is None else beta).double().requires_grad_(True)
    mean = xd.mean(dim=1, keepdim=True)
    var = ((xd - mean) ** 2).mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    y = (xd - mean) * rstd * gm + bt
    y.backward(dy.double())
    _REF[key] = dict(y=y.detach(), mean=mean.detach().reshape(-1), rstd=rstd.detach().reshape(-1), dx=xd.grad, dgamma=gm.grad,
                     dbeta=bt.grad)
    return _REF[key]


def _forward(cuda, x, gamma, beta, stats=True):
    r, c = x.shape
    dev = dict(x=x.to(cuda), gamma=None if gamma is None else gamma.to(cuda), beta=None if beta is None else beta.to(cuda))
    yw, yi = guarded(x.numel(), cuda)
    mw, mi = guarded(r, cuda) if stats else (None, None)
    rw, ri = guarded(r, cuda) if stats else (None, None)
    _call('evk_ln_fwd', dev['x'].data_ptr(), _ptr(dev['gamma']), _ptr(dev['beta']), EPS, yi.data_ptr(), _ptr(mi), _ptr(ri), r, c,
          _stream())
    y = _fetch(yw, yi, 'y').view(r, c)
    mean = _fetch(mw, mi, 'save_mean') if stats else None
    rstd = _fetch(rw, ri, 'save_rstd') if stats else None
    dev.update(mean=mi, rstd=ri)
    return y, mean, rstd, dev


def _backward(cuda, dev, dy, want=('dx', 'dgamma', 'dbeta')):
    r, c = dy.shape
    dyd = dy.to(cuda)
    bufs = {k: guarded(dy.numel() if k == 'dx' else c, cuda) for k in want}
    params = 'dgamma' in want or 'dbeta' in want
    nbytes = _lib().evk_ln_bwd_workspace_bytes(r, c) if params else 0
    assert not params or nbytes == _plan(r, c)[3] * 2 * c * 4
    ww, wi = guarded(nbytes // 4, cuda) if params else (None, None)
    _call('evk_ln_bwd', dyd.data_ptr(), dev['x'].data_ptr(), dev['mean'].data_ptr(), dev['rstd'].data_ptr(), _ptr(dev['gamma']),
          *[_ptr(bufs[k][1]) if k in bufs else None for k in ('dx', 'dgamma', 'dbeta')], r, c, _ptr(wi), nbytes, _stream())
    out = {k: _fetch(w, i, k) for k, (w, i) in bufs.items()}
    if 'dx' in out:
        out['dx'] = out['dx'].view(r, c)
    if params:
        _fetch(ww, wi, 'backward workspace')       # every record fully written, nothing beside them
    return out


def _stats_close(mean, rstd, ref, what):
    m, r = ref['mean'], ref['rstd']
    em = ((mean.double() - m).abs() / m.abs().clamp(min=1.0)).max().item()
    er = ((rstd.double() - r).abs() / r).max().item()
    print(f'{what}: save_mean err {em:.3e} (bound {TOL_MEAN:g}), save_rstd relative err {er:.3e} (bound {TOL_RSTD:g})')
    assert em <= TOL_MEAN and er <= TOL_RSTD, f'{what}: save_mean err {em:.3e}, save_rstd relative err {er:.3e}'


# ------------------------------------------------------------------------------------------------ the plan's edges
def test_case_table_reaches_every_regime():
    plans = {n: _plan(*_shape(n)) for n in CASES}
    assert plans['one_lane'][:2] == (1, 1) and plans['c2048'][:2] == (64, 8) and plans['c1536'][:2] == (64, 6)
    lanes, cols, rows, wgs = plans['c96_ragged']
    assert lanes < 64 and lanes * cols == 24 and wgs > 1 and 257 % rows != 0
    lanes, cols, _, _ = plans['c100_masked']
    assert lanes * cols > 25                                    # a masked column
    for n in ('second_trip_c8', 'second_trip_c96'):
        r, c = _shape(n)
        _, _, rows, wgs = plans[n]
        assert r == rows * wgs + 1 and wgs == _plan(2 ** 40, c)[3]
    assert plans['wg_minus_1_c96'][3] == 1 and plans['wg_plus_1_c96'][3] == 2


@pytest.mark.parametrize('name', list(CASES))
def test_forward_and_backward_match_float64(cuda, name):
    i = list(CASES).index(name)
    r, c = _shape(name)
    affine = AFFINE[i % 4]
    x, gamma, beta, dy = _inputs(r, c, 100 + i, affine)
    ref = _reference(name, x, gamma, beta, dy)
    y, mean, rstd, dev = _forward(cuda, x, gamma, beta)
    got = _backward(cuda, dev, dy)
    _stats_close(mean, rstd, ref, name)
    _close(y, ref['y'], TOL_Y, f'{name} y')
    for k in sorted(got):
        _close(got[k], ref[k], TOL_GRAD, f'{name} {k}')


@pytest.mark.parametrize('name', ['c96_ragged', 'c100_masked', 'c2048'])
def test_null_affine_and_null_outputs(cuda, name):
    """gamma / beta absent in every combination; the forward without statistics; each backward output on its own and each one
    left out: what is computed does not depend on what else is asked for (same bits)"""
    r, c = _shape(name)
    for affine in AFFINE:
        x, gamma, beta, dy = _inputs(r, c, 7, affine)
        ref = _reference((name, affine), x, gamma, beta, dy)
        y, mean, rstd, dev = _forward(cuda, x, gamma, beta)
        _close(y, ref['y'], TOL_Y, f'{name} {affine} y')
        y2 = _forward(cuda, x, gamma, beta, stats=False)[0]
        _same_bits(y2, y, f'{name} {affine} y without statistics')
        full = _backward(cuda, dev, dy)
        for k in sorted(full):
            _close(full[k], ref[k], TOL_GRAD, f'{name} {affine} {k}')
        if affine != 'both':
            continue
        for want in (('dx',), ('dgamma',), ('dbeta',), ('dx', 'dgamma'), ('dx', 'dbeta'), ('dgamma', 'dbeta')):
            part = _backward(cuda, dev, dy, want)
            assert sorted(part) == sorted(want)
            for k in want:
                _same_bits(part[k], full[k], f'{name} {k} alone with {want}')


@pytest.mark.parametrize('name', ['c96_ragged', 'c384', 'second_trip_c96', 'c1536'])
def test_second_run_gives_the_same_bits(cuda, name):
    r, c = _shape(name)
    x, gamma, beta, dy = _inputs(r, c, 11)
    y, mean, rstd, dev = _forward(cuda, x, gamma, beta)
    got = _backward(cuda, dev, dy)
    y2, mean2, rstd2, dev2 = _forward(cuda, x, gamma, beta)
    got2 = _backward(cuda, dev2, dy)
    for a, b, what in ((y, y2, 'y'), (mean, mean2, 'save_mean'), (rstd, rstd2, 'save_rstd')):
        _same_bits(b, a, f'{name} {what}')
    for k in got:
        _same_bits(got2[k], got[k], f'{name} {k}')


# ------------------------------------------------------------------------------------------------ numerics
@pytest.mark.parametrize('c', [96, 100, 1536, 2048])
def test_constant_rows_have_zero_variance(cuda, c):
    consts = torch.tensor([0.0, 1.0, -3.5, 1000.0, 2.0 ** -20, 384.25, -0.0078125])       # <= 11 mantissa bits each
    x = consts.view(-1, 1).expand(-1, c).contiguous()
    gen = torch.Generator().manual_seed(3)
    gamma, beta = torch.randn(c, generator=gen), torch.randn(c, generator=gen)
    y, mean, rstd, _ = _forward(cuda, x, gamma, beta)
    _same_bits(y, beta.view(1, -1).expand(len(consts), -1).contiguous(), f'C={c} y == beta')
    _same_bits(mean + 0.0, consts + 0.0, f'C={c} save_mean')           # (+ 0.0: -0.0 and 0.0 are the same mean)
    want = np.float32(1.0 / np.sqrt(np.float64(EPS)))
    ulp = float(np.spacing(want))
    err = (rstd.double() - 1.0 / np.sqrt(np.float64(EPS))).abs().max().item()
    print(f'C={c}: save_rstd {rstd[0].item()!r}, 1/sqrt(eps) {float(want)!r}, err {err:.3e}, ulp {ulp:.3e}')
    assert err <= ulp


@pytest.mark.parametrize('c', [96, 1536])
def test_large_mean_rows_stay_within_twice_atens_error(cuda, c):
    gen = torch.Generator().manual_seed(5)
    x = 1000.0 + 2.0 * torch.randn(64, c, generator=gen)
    xd = x.double()
    mean = xd.mean(dim=1, keepdim=True)
    var = ((xd - mean) ** 2).mean(dim=1, keepdim=True)
    ref = (xd - mean) / torch.sqrt(var + EPS)
    aten = F.layer_norm(x, (c,), None, None, EPS)
    y, smean, srstd, _ = _forward(cuda, x, None, None)
    scale = ref.abs().max().item()
    e_aten = (aten.double() - ref).abs().max().item()
    e_kernel = (y.double() - ref).abs().max().item()
    print(f'C={c}: kernel err {e_kernel:.3e} ({e_kernel / scale:.2e} of max|y|), aten fp32 err {e_aten:.3e} '
          f'({e_aten / scale:.2e} of max|y|), ratio {e_kernel / e_aten:.3f}')
    assert e_kernel <= 2.0 * e_aten, f'kernel err {e_kernel:.3e} > 2 x aten err {e_aten:.3e}'
    em = ((smean.double() - mean.reshape(-1)).abs() / mean.reshape(-1).abs()).max().item()
    print(f'C={c}: save_mean relative err {em:.3e}')
    assert em <= TOL_MEAN


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing(cuda):
    r, c = 8, 8
    x = torch.randn(r, 2056, device=cuda)
    outs = {k: guarded(n, cuda) for k, n in (('y', r * 2056), ('mean', r), ('rstd', r), ('dx', r * 2056), ('dg', 2056),
                                              ('db', 2056), ('ws', 1024 * 2 * 2056))}
    o = {k: v[1] for k, v in outs.items()}
    lib = _lib()

    def fwd(rr, cc, xp=None, yp=None):
        return lib.evk_ln_fwd(xp or x.data_ptr(), None, None, EPS, yp or o['y'].data_ptr(), o['mean'].data_ptr(),
                              o['rstd'].data_ptr(), rr, cc, _stream())

    def bwd(rr, cc, ws_bytes=None, dxp=-1):
        return lib.evk_ln_bwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), None,
                              o['dx'].data_ptr() if dxp == -1 else dxp, o['dg'].data_ptr(), o['db'].data_ptr(), rr, cc,
                              o['ws'].data_ptr(), o['ws'].numel() * 4 if ws_bytes is None else ws_bytes, _stream())
    for rr, cc in ((r, 0), (r, 6), (r, 2052), (0, c), (-1, c)):
        assert fwd(rr, cc) in (-1, -2) and lib.evk_last_error(), (rr, cc)
        assert bwd(rr, cc) in (-1, -2), (rr, cc)
    assert fwd(r, c, xp=x.data_ptr() + 4) == -1 and fwd(r, c, yp=o['y'].data_ptr() + 8) == -1      # 16-byte alignment
    assert lib.evk_ln_fwd(None, None, None, EPS, o['y'].data_ptr(), None, None, r, c, _stream()) == -1
    assert bwd(r, c, ws_bytes=lib.evk_ln_bwd_workspace_bytes(r, c) - 4) == -4                       # EVK_E_WORKSPACE
    assert lib.evk_ln_bwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), None, None, None, None, r, c, None, 0,
                          _stream()) == -1                                                          # nothing to compute
    torch.cuda.synchronize()
    for k, (whole, inner) in outs.items():
        assert guards_intact(whole, inner.numel()) and bool(torch.isnan(inner).all()), f'{k}: a refused call wrote'
