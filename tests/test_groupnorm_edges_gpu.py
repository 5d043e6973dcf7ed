"""GroupNorm (+ReLU), channel concat / split and the Dropout2d channel scale (csrc/groupnorm.hip) at the edges of the reduce
plan, called directly through the C ABI.  Every output (y, save_mean, save_rstd, dx, dgamma, dbeta) is a NaN-filled slice of
a sentinel-guarded allocation (tests/guard_common.py) and so is the workspace, at exactly evk_gn_workspace_bytes: an element
nobody wrote stays NaN, a store beside a slice or past the workspace breaks a sentinel.

Reference: the definition in float64 torch on the CPU from the same fp32 inputs — per (sample, group) mean and biased
variance, y = (x - mean) * rstd * gamma + beta, optionally ReLU — and autograd on it.  The ReLU gradient is masked on y > 0;
where the float64 pre-activation lies within the forward tolerance of zero the reference takes the sign the kernel's own y
has, since either is a correct forward there and the backward must follow the forward it got.

Tolerances: the project's own (test_next_rows_gpu.py::test_group_norm_matches_torch), y to 1e-5 max(1, max|ref|), gradients
to 1e-4 max(1, max|ref|); save_mean to 1e-6 max(1, |mean|), save_rstd to 1e-5 relative.

Known property of the pivot shift (sums of x - x[n][0][c] in fp32, un-shifted in fp64): its error grows with the square of
the pivot's distance from the mean in standard deviations — about 2e-6 relative in rstd at 8 sigma (tested below), about
2e-5 at 50 sigma (an emulation of the fp32 partial sums; not tested, not a defect this file is after).

Concat, split and channel_scale move or multiply single values: bit-exact against torch.cat, slicing and an fp32 multiply."""
import ctypes

import numpy as np
import pytest
import torch

from tests.guard_common import guarded, guards_intact

pytestmark = pytest.mark.gpu

EPS = float(np.float32(1e-5))        # the kernels take eps as a float
TOL_Y, TOL_GRAD, TOL_MEAN, TOL_RSTD = 1e-5, 1e-4, 1e-6, 1e-5
STREAM_CAP = 2048 * 256              # 16-byte elements one trip of the apply / concat / split / scale grids covers

# (HW, C, G, N) — see test_case_table_reaches_every_regime for what each is here for
CASES = [
    (1, 4, 1, 3),            # tpc 1, rl 256, one row
    (5, 4, 4, 3),            # tpc 1, groups of one channel
    (4099, 12, 3, 3),        # tpc 3, rl 85: thread 255 idle
    (1073, 200, 8, 3),       # tpc 50, rl 5, four chunks, the last short
    (8209, 260, 4, 1),       # tpc 65 (a wave straddles rows), 33 chunks, second trip of the apply grids
    (660, 48, 4, 3),         # tpc 12, rl 21
    (7, 1028, 4, 3),         # c4 257: one thread takes a second column trip
    (5, 1536, 32, 3),        # c4 384: half the threads take a second column trip
    (3, 2052, 4, 3),         # c4 513: three column trips
    (1031, 64, 32, 3),       # two chunks, the last short, groups of two channels
    (2053, 64, 2, 3),        # three chunks, the last short
    (16400, 1024, 32, 1),    # more than 256 chunks' worth: the cap
]
AFFINE = ('both', 'gamma', 'beta', 'none')


def _flags(i):
    """(affine parameters present, dgamma / dbeta requested, ReLU) of case i"""
    return AFFINE[i % 4], i % 3 != 2, bool((i // 4 + i % 4) % 2)


def _lib():
    from ever_amd import _C
    return _C.load()


def _call(name, *args):
    from ever_amd import _C
    _C.call(name, *args)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _plan(hw, c):
    out = (ctypes.c_int32 * 4)()
    assert _lib().evk_gn_plan(hw, c, out) == 0
    return tuple(out)       # nchunk, rows_per_chunk, tpc, rl


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
    assert not bool(bad.any()), (f'{what}: {int(bad.sum())} of {bad.numel()} elements differ in their bits, first at '
                                 f'{tuple(int(v) for v in bad.nonzero()[0])}: {got[bad][0].item()!r} vs {ref[bad][0].item()!r}')


def _close(got, ref, tol, what):
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), f'{what}: not finite'
    err, scale = (got - ref).abs().max().item(), max(1.0, ref.abs().max().item())
    print(f'{what}: max err {err:.3e}, bound {tol:g} * {scale:.3e}')
    assert err <= tol * scale, f'{what}: max err {err:.3e} > {tol:g} * {scale:.3e}'


def _stats_close(mean, rstd, ref, what):
    m, r = ref['mean'], ref['rstd']
    em = ((mean.double() - m).abs() / m.abs().clamp(min=1.0)).max().item()
    er = ((rstd.double() - r).abs() / r).max().item()
    print(f'{what}: save_mean err {em:.3e} (bound {TOL_MEAN:g}), save_rstd relative err {er:.3e} (bound {TOL_RSTD:g})')
    assert em <= TOL_MEAN, f'{what}: save_mean err {em:.3e}'
    assert er <= TOL_RSTD, f'{what}: save_rstd relative err {er:.3e}'


# ------------------------------------------------------------------------------------------------ inputs, reference
def _inputs(hw, c, g, n, seed, affine='both'):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, hw, c, generator=gen) * 2 + 0.7
    gamma, beta = torch.randn(c, generator=gen), torch.randn(c, generator=gen)
    dy = torch.randn(n, hw, c, generator=gen)
    return x, (gamma if affine in ('both', 'gamma') else None), (beta if affine in ('both', 'beta') else None), dy


def _reference(x, gamma, beta, g, relu, dy=None, y_got=None):
    """float64 definition; with dy also the gradients (dgamma / dbeta as if gamma = 1 / beta = 0 where absent)"""
    n, hw, c = x.shape
    xd = x.double().requires_grad_(dy is not None)
    gm = (torch.ones(c) if gamma is None else gamma).double().requires_grad_(dy is not None)
    bt = (torch.zeros(c) if beta is None else beta).double().requires_grad_(dy is not None)
    xg = xd.view(n, hw, g, c // g)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    y = ((xg - mean) * rstd).view(n, hw, c) * gm + bt
    if relu:
        pos = y.detach() > 0
        if y_got is not None:       # (ties within the forward tolerance: the sign the kernel's forward produced)
            band = TOL_Y * max(1.0, y.detach().abs().max().item())
            pos = torch.where(y.detach().abs() <= band, y_got > 0, pos)
        y = y * pos
    ref = dict(y=y.detach(), mean=mean.detach().reshape(n, g), rstd=rstd.detach().reshape(n, g))
    if dy is not None:
        y.backward(dy.double())
        ref.update(dx=xd.grad, dgamma=gm.grad, dbeta=bt.grad)
    return ref


# ------------------------------------------------------------------------------------------------ guarded launches
def _workspace(n, hw, c, g, cuda):
    nbytes = _lib().evk_gn_workspace_bytes(n, hw, c, g)
    nchunk = _plan(hw, c)[0]
    assert nbytes == (n * nchunk * 2 * c + 2 * n * g) * 4
    whole, inner = guarded(nbytes // 4, cuda)
    return whole, inner, nbytes, n * nchunk * 2 * c


def _forward(cuda, x, gamma, beta, g, relu):
    """evk_gn_fwd into guarded outputs and an exactly sized guarded workspace -> (y, mean, rstd on the CPU, device state)"""
    n, hw, c = x.shape
    dev = dict(x=x.to(cuda), gamma=None if gamma is None else gamma.to(cuda), beta=None if beta is None else beta.to(cuda))
    yw, yi = guarded(x.numel(), cuda)
    mw, mi = guarded(n * g, cuda)
    rw, ri = guarded(n * g, cuda)
    ww, wi, nbytes, npartial = _workspace(n, hw, c, g, cuda)
    _call('evk_gn_fwd', dev['x'].data_ptr(), _ptr(dev['gamma']), _ptr(dev['beta']), EPS, yi.data_ptr(), mi.data_ptr(),
          ri.data_ptr(), n, hw, c, g, 1 if relu else 0, wi.data_ptr(), nbytes, _stream())
    y = _fetch(yw, yi, 'y').view(n, hw, c)
    mean, rstd = _fetch(mw, mi, 'save_mean').view(n, g), _fetch(rw, ri, 'save_rstd').view(n, g)
    ws = _fetch(ww, wi, 'forward workspace', nan_ok=True)        # (the coefficients behind the partial sums: backward only)
    assert not bool(torch.isnan(ws[:npartial]).any()), 'forward: a partial sum was never written'
    dev.update(y=yi, mean=mi, rstd=ri)
    return y, mean, rstd, dev


def _backward(cuda, dev, dy, g, relu, want_d):
    n, hw, c = dy.shape
    dyd = dy.to(cuda)
    xw, xi = guarded(dy.numel(), cuda)
    gw, gi = guarded(c, cuda) if want_d else (None, None)
    bw, bi = guarded(c, cuda) if want_d else (None, None)
    ww, wi, nbytes, _ = _workspace(n, hw, c, g, cuda)
    _call('evk_gn_bwd', dyd.data_ptr(), dev['x'].data_ptr(), dev['y'].data_ptr() if relu else None, _ptr(dev['gamma']),
          dev['mean'].data_ptr(), dev['rstd'].data_ptr(), xi.data_ptr(), _ptr(gi), _ptr(bi), n, hw, c, g, 1 if relu else 0,
          wi.data_ptr(), nbytes, _stream())
    out = dict(dx=_fetch(xw, xi, 'dx').view(n, hw, c))
    if want_d:
        out.update(dgamma=_fetch(gw, gi, 'dgamma'), dbeta=_fetch(bw, bi, 'dbeta'))
    _fetch(ww, wi, 'backward workspace')
    return out


def _check_all(cuda, x, gamma, beta, dy, g, relu, want_d, what):
    y, mean, rstd, dev = _forward(cuda, x, gamma, beta, g, relu)
    got = _backward(cuda, dev, dy, g, relu, want_d)
    ref = _reference(x, gamma, beta, g, relu, dy, y_got=y)
    _stats_close(mean, rstd, ref, what)
    _close(y, ref['y'], TOL_Y, f'{what} y')
    for k in sorted(got):
        _close(got[k], ref[k], TOL_GRAD, f'{what} {k}')
    return got, ref


# ------------------------------------------------------------------------------------------------ the case table
def test_case_table_reaches_every_regime():
    """Asked of evk_gn_plan, so that a change to the plan cannot silently empty a regime of the table."""
    rows = []
    for i, (hw, c, g, n) in enumerate(CASES):
        nchunk, rpc, tpc, rl = _plan(hw, c)
        rows.append(dict(i=i, hw=hw, c=c, g=g, n=n, nchunk=nchunk, rpc=rpc, tpc=tpc, rl=rl, c4=c // 4, n4=n * hw * c // 4))

    def count(pred):
        return sum(1 for r in rows if pred(r))

    assert count(lambda r: r['tpc'] == 1 and r['rl'] == 256) >= 2
    assert count(lambda r: 256 % r['tpc'] != 0 and r['tpc'] * r['rl'] < 256) >= 4                  # idle threads
    assert count(lambda r: r['tpc'] % 64 != 0 and r['tpc'] > 64) >= 1                             # a wave straddles rows
    assert count(lambda r: r['c4'] > r['tpc']) >= 3                                               # second column trip ...
    assert count(lambda r: r['c4'] > r['tpc'] and r['c4'] % r['tpc'] == 1) >= 2                   # ... by one thread
    assert count(lambda r: r['c4'] > r['tpc'] and r['c4'] % r['tpc'] == r['tpc'] // 2) >= 1       # ... by half of them
    assert count(lambda r: r['c4'] > 2 * r['tpc']) >= 1                                           # a third trip
    assert count(lambda r: r['nchunk'] > 1 and r['nchunk'] * r['rpc'] > r['hw']) >= 4             # short last chunk
    assert count(lambda r: r['rl'] > 1 and r['nchunk'] > 1 and r['rpc'] > -(-r['hw'] // r['nchunk'])) >= 1   # rounded up to rl
    assert count(lambda r: r['hw'] * r['c'] > 256 * 65536 and r['nchunk'] > 250) == 1             # the request cap
    assert count(lambda r: r['n4'] > STREAM_CAP) >= 2                                             # second apply trip
    assert count(lambda r: r['n'] == 1) >= 2 and count(lambda r: r['n'] == 3) >= 8
    assert count(lambda r: r['c'] // r['g'] == 1) >= 1 and count(lambda r: r['c'] // r['g'] > 64) >= 1
    for relu in (False, True):
        for a in AFFINE:
            assert sum(1 for i in range(len(CASES)) if _flags(i)[0] == a and _flags(i)[2] == relu) >= 1, (a, relu)
        for d in (False, True):
            assert sum(1 for i in range(len(CASES)) if _flags(i)[1] == d and _flags(i)[2] == relu) >= 1, (d, relu)
    for a in AFFINE:
        assert sum(1 for i in range(len(CASES)) if _flags(i)[0] == a) >= 2
    assert sum(1 for i in range(len(CASES)) if not _flags(i)[1]) >= 2


@pytest.mark.parametrize('i', range(len(CASES)), ids=lambda i: 'hw{}-c{}-g{}-n{}'.format(*CASES[i]))
def test_group_norm_at_plan_edges(cuda, i):
    hw, c, g, n = CASES[i]
    affine, want_d, relu = _flags(i)
    x, gamma, beta, dy = _inputs(hw, c, g, n, 100 + i, affine)
    _check_all(cuda, x, gamma, beta, dy, g, relu, want_d, f'{CASES[i]} {affine} relu={relu}')


@pytest.mark.parametrize('hw,c,g', [(4099, 12, 3), (1073, 200, 8), (660, 48, 4)], ids=lambda v: str(v))
def test_group_norm_with_an_outlying_pivot_row(cuda, hw, c, g):
    """row 0 of every sample — the pivot the partial sums are shifted by — lies 8 standard deviations off the rest"""
    x, gamma, beta, dy = _inputs(hw, c, g, 3, 7 * hw + c)
    x[:, 0, :] += 16.0
    _check_all(cuda, x, gamma, beta, dy, g, hw % 2 == 0, True, f'pivot +8 sigma {(hw, c, g)}')


@pytest.mark.parametrize('kind', ['1000+randn', '300+0.01randn'])
@pytest.mark.parametrize('hw,c,g', [(1073, 200, 8), (7, 1028, 4), (1031, 64, 32)], ids=lambda v: str(v))
def test_group_norm_with_a_mean_that_dwarfs_the_spread(cuda, hw, c, g, kind):
    """The rounding of the fp32 mean dominates y here, so no fixed bound applies: the kernel may be at most twice as far from
    float64 as torch's own fp32 CPU group_norm on the same input, plus 4 ulp of max|ref| (an equally valid rounding of the
    mean can land on the other side of the same ulp).  save_rstd stays within 1e-5 relative — sums of raw x and x^2 in fp32
    would miss that by orders of magnitude, which is what the pivot shift is for."""
    n = 3
    gen = torch.Generator().manual_seed(hw + c)
    r = torch.randn(n, hw, c, generator=gen)
    x = 1000.0 + r if kind.startswith('1000') else 300.0 + 0.01 * r
    gamma, beta = torch.randn(c, generator=gen), torch.randn(c, generator=gen)
    y, mean, rstd, _ = _forward(cuda, x, gamma, beta, g, False)
    ref = _reference(x, gamma, beta, g, False)
    t32 = torch.nn.functional.group_norm(x.permute(0, 2, 1).contiguous(), g, gamma, beta, EPS).permute(0, 2, 1)
    top = ref['y'].abs().max().item()
    err = (y.double() - ref['y']).abs().max().item()
    err32 = (t32.double() - ref['y']).abs().max().item()
    allow = 2.0 * err32 + 4.0 * float(np.spacing(np.float32(top)))
    er = ((rstd.double() - ref['rstd']).abs() / ref['rstd']).max().item()
    print(f'large mean {kind} {(hw, c, g)}: kernel err {err:.3e}, torch fp32 err {err32:.3e}, ratio {err / max(err32, 1e-300):.3f}, '
          f'allowance {allow:.3e}, max|ref| {top:.3e}, save_rstd relative err {er:.3e}')
    assert er <= TOL_RSTD, f'save_rstd relative err {er:.3e}'
    assert bool(torch.isfinite(y).all()) and err <= allow, f'y err {err:.3e} > 2 * {err32:.3e} + 4 ulp({top:.3e})'


@pytest.mark.parametrize('relu', [False, True])
def test_group_norm_of_a_constant_group(cuda, relu):
    hw, c, g, n, const = 35, 48, 4, 3, 1.5
    cg = c // g
    x, gamma, beta, dy = _inputs(hw, c, g, n, 11)
    x[1, :, 2 * cg:3 * cg] = const
    y, mean, rstd, dev = _forward(cuda, x, gamma, beta, g, relu)
    assert mean[1, 2].item() == const
    want = np.float32(1.0 / np.sqrt(np.float64(EPS)))
    assert abs(float(rstd[1, 2]) - float(want)) <= float(np.spacing(want)), (float(rstd[1, 2]), float(want))
    want_y = (beta[2 * cg:3 * cg].clamp(min=0) if relu else beta[2 * cg:3 * cg]).expand(hw, cg)
    _same_bits(y[1, :, 2 * cg:3 * cg], want_y, 'y of the constant group')
    got = _backward(cuda, dev, dy, g, relu, True)
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    ref = _reference(x, gamma, beta, g, relu, dy, y_got=y)      # (and everything else as usual)
    _stats_close(mean, rstd, ref, 'constant group')
    _close(y, ref['y'], TOL_Y, 'constant group y')
    for k in sorted(got):
        _close(got[k], ref[k], TOL_GRAD, f'constant group {k}')


def test_relu_mask_silences_a_channel_that_is_zero_everywhere(cuda):
    hw, c, g, n, dead = 70, 48, 4, 3, 17
    x, gamma, beta, dy = _inputs(hw, c, g, n, 13)
    beta[dead] = -100.0
    y, mean, rstd, dev = _forward(cuda, x, gamma, beta, g, True)
    assert bool((y[:, :, dead] == 0).all())
    got = _backward(cuda, dev, dy, g, True, True)
    assert got['dgamma'][dead].item() == 0.0 and got['dbeta'][dead].item() == 0.0
    ref = _reference(x, gamma, beta, g, True, dy, y_got=y)
    assert ref['dgamma'][dead].item() == 0.0
    _close(y, ref['y'], TOL_Y, 'dead channel y')
    for k in sorted(got):
        _close(got[k], ref[k], TOL_GRAD, f'dead channel {k}')
    _close(got['dx'][:, :, dead], ref['dx'][:, :, dead], TOL_GRAD, 'dx of the dead channel')


def test_group_norm_refuses_bad_arguments_before_any_launch(cuda):
    from ever_amd._C import HipKernelError
    t = torch.zeros(4096, device=cuda)
    p = t.data_ptr()

    def fwd(n, hw, c, g, nbytes=1 << 14):
        _call('evk_gn_fwd', p, p, p, EPS, p, p, p, n, hw, c, g, 0, p, nbytes, _stream())

    def bwd(n, hw, c, g, nbytes=1 << 14, y=p, flags=0):
        _call('evk_gn_bwd', p, p, y, p, p, p, p, p, p, n, hw, c, g, flags, p, nbytes, _stream())

    for fn, name in ((fwd, 'gn_fwd'), (bwd, 'gn_bwd')):
        with pytest.raises(HipKernelError, match=f'{name}: C=6 must be a multiple of 4'):
            fn(1, 4, 6, 1)
        with pytest.raises(HipKernelError, match=f'{name}: C=8 must be a multiple of 4 and of G=3'):
            fn(1, 4, 8, 3)
        with pytest.raises(HipKernelError, match=f'{name}: batch 65536 > 65535'):
            fn(65536, 1, 4, 1)
        need = _lib().evk_gn_workspace_bytes(2, 5, 8, 2)
        with pytest.raises(HipKernelError, match=f'{name}: workspace'):
            fn(2, 5, 8, 2, nbytes=need - 1)
    with pytest.raises(HipKernelError, match='gn_bwd: null pointer'):
        bwd(2, 5, 8, 2, y=None, flags=1)
    torch.cuda.synchronize()
    assert bool((t == 0).all())          # (nothing was launched on the way)


# ------------------------------------------------------------------------------------------------ concat / split / scale
def _concat(cuda, a, b):
    rows, ca, cb = a.shape[0], a.shape[1], b.shape[1]
    ad, bd = a.to(cuda), b.to(cuda)
    ow, oi = guarded(rows * (ca + cb), cuda)
    _call('evk_concat_channels', ad.data_ptr(), bd.data_ptr(), oi.data_ptr(), rows, ca, cb, _stream())
    return _fetch(ow, oi, 'concat').view(rows, ca + cb), oi


def _split(cuda, src_dev, rows, ca, cb, want_a=True, want_b=True):
    aw, ai = guarded(rows * ca, cuda)
    bw, bi = guarded(rows * cb, cuda)
    _call('evk_split_channels', src_dev.data_ptr(), ai.data_ptr() if want_a else None, bi.data_ptr() if want_b else None,
          rows, ca, cb, _stream())
    a = _fetch(aw, ai, 'split a', nan_ok=not want_a).view(rows, ca)
    b = _fetch(bw, bi, 'split b', nan_ok=not want_b).view(rows, cb)
    assert want_a or bool(torch.isnan(a).all())
    assert want_b or bool(torch.isnan(b).all())
    return a, b


CONCAT = [(rows, ca, cb) for ca, cb in ((4, 4), (8, 12), (256, 4), (4, 1028)) for rows in (1, 7, 70)] + [(2053, 4, 1028)]


@pytest.mark.parametrize('rows,ca,cb', CONCAT, ids=lambda v: str(v))
def test_concat_and_split_are_selections(cuda, rows, ca, cb):
    """the last case takes the grids past their cap of 2048 workgroups"""
    assert (rows == 2053) == (rows * (ca + cb) // 4 > STREAM_CAP)
    gen = torch.Generator().manual_seed(rows + ca)
    a, b = torch.randn(rows, ca, generator=gen), torch.randn(rows, cb, generator=gen)
    want = torch.cat([a, b], dim=1)
    out, out_dev = _concat(cuda, a, b)
    _same_bits(out, want, 'concat')
    a2, b2 = _split(cuda, out_dev, rows, ca, cb)                 # the round trip
    _same_bits(a2, a, 'split(concat).a')
    _same_bits(b2, b, 'split(concat).b')
    src = torch.randn(rows, ca + cb, generator=gen)
    sd = src.to(cuda)
    a3, _ = _split(cuda, sd, rows, ca, cb, want_b=False)
    _same_bits(a3, src[:, :ca], 'split with b null')
    _, b3 = _split(cuda, sd, rows, ca, cb, want_a=False)
    _same_bits(b3, src[:, ca:], 'split with a null')


def test_concat_split_and_scale_refuse_bad_arguments(cuda):
    from ever_amd._C import HipKernelError
    t = torch.zeros(64, device=cuda)
    p = t.data_ptr()
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        with pytest.raises(HipKernelError, match='concat_channels: null pointer'):
            _call('evk_concat_channels', *args, 2, 4, 4, _stream())
    for args in ((None, p, p), (p, None, None)):
        with pytest.raises(HipKernelError, match='split_channels: null pointer'):
            _call('evk_split_channels', *args, 2, 4, 4, _stream())
    for name in ('concat_channels', 'split_channels'):
        for ca, cb in ((6, 4), (4, 2), (0, 4), (4, 0)):
            with pytest.raises(HipKernelError, match=f'{name}: channel counts'):
                _call('evk_' + name, p, p, p, 2, ca, cb, _stream())
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        with pytest.raises(HipKernelError, match='channel_scale: null pointer'):
            _call('evk_channel_scale', *args, 1, 2, 4, _stream())
    for c in (6, 0):
        with pytest.raises(HipKernelError, match='channel_scale: C='):
            _call('evk_channel_scale', p, p, p, 1, 2, c, _stream())
    torch.cuda.synchronize()
    assert bool((t == 0).all())


@pytest.mark.parametrize('n,hw,c', [(3, 1, 8), (3, 35, 12), (3, 35, 1028), (3, 2731, 260)], ids=lambda v: str(v))
def test_channel_scale_is_an_fp32_multiply(cuda, n, hw, c):
    """the last case takes the grid past its cap; a scale of 0 gives +-0, and NaN where x is NaN, as torch does"""
    assert (n * hw * c // 4 > STREAM_CAP) == (hw == 2731)
    gen = torch.Generator().manual_seed(hw + c)
    x = torch.randn(n, hw, c, generator=gen)
    scale = torch.where(torch.rand(n, c, generator=gen) > 0.3, torch.tensor(1.0 / 0.75), torch.tensor(0.0))
    scale[1] = torch.randn(c, generator=gen)         # (not only the two values of a dropout mask)
    scale[1, 3], scale[n - 1, c - 1] = 0.0, 0.0
    x[1, hw - 1, 3] = float('nan')
    x[n - 1, 0, c - 1] = float('nan')
    x[0, 0, 0] = float('inf')
    scale[0, 0] = 0.0
    want = x * scale[:, None, :]
    assert bool(torch.isnan(want[1, hw - 1, 3])) and bool(torch.isnan(want[0, 0, 0]))
    xd, sd = x.to(cuda), scale.to(cuda)
    ow, oi = guarded(x.numel(), cuda)
    _call('evk_channel_scale', xd.data_ptr(), sd.data_ptr(), oi.data_ptr(), n, hw, c, _stream())
    got = _fetch(ow, oi, 'channel_scale', nan_ok=True).view(n, hw, c)
    both = torch.isnan(got) & torch.isnan(want)
    assert int(both.sum()) == int(torch.isnan(want).sum()) == 3
    _same_bits(torch.where(both, torch.zeros_like(got), got), torch.where(both, torch.zeros_like(want), want), 'channel_scale')
