"""The BatchNorm family (csrc/bn.hip, bn_pool.hip; bn_dot.hip has tests/test_bn_dot_gpu.py) at its plan, channel and map-shape
edges, through the C-ABI, against float64 computed on the CPU from the same fp32 inputs.

Shapes are picked WITH evk_bn_plan: a case names the edges it exists for (`want`) and fails with "no longer covers" when a
retuned plan takes one away; the last test asserts the union.  Every output and the workspace hold NaN before a launch and are
slices of sentinel-guarded allocations (tests/guard_common.py).

Bounds are derived, not tuned (u = 2^-24; DESIGN.md §6b carries the derivation and the measured worst error / bound):
  a fp32 sum of n terms along a chain of L additions errs by at most L u sum|terms|; the plan gives L (`_chains`);
  mean: the shifted sum, divided in fp64, cast;  var: the shifted sum of squares and the mean's error through E[d^2] - E[d]^2;
  invstd: var's error through (var + eps)^-1/2, cast;  scale, shift, running statistics: their fp32 expressions term by term;
  y: |x| e(scale) + e(shift) + 3 u (|x scale| + |shift| + |residual|);
  dbeta, dgamma: L u sum|terms| + the error of xhat under the sums + cast;  dx: k0 (g - k1 - xhat k2) term by term.
An element whose float64 pre-activation lies inside the bound of y has no certain ReLU mask: it gets no upstream gradient, and
every case asserts that this leaves out at most 0.1 % of its elements."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests.bn_ref_common import (LEFT_OUT, NAN_BITS, U, WORST, Bufs, Stats, _amax_holds, _bwd_ref, _data, _given_stats,  # noqa: F401
                                 _hold, _params, _ptr, _stream)

pytestmark = pytest.mark.gpu

EPS = float(np.float32(1e-5))
MOM = float(np.float32(0.1))
RELU = 1

RAN = {}                # test -> set of edges its cases asserted and ran


# ------------------------------------------------------------------------------------------------ plumbing
def _plan(lib, rows, c, kind=0):
    out = (ctypes.c_int32 * 6)()
    assert lib.evk_bn_plan(rows, c, kind, out) == 0, (rows, c, kind, lib.evk_last_error())
    return tuple(out)


def _chains(pl):
    """longest chains of fp32 additions a term passes in the statistics pass (four rows per trip, pairwise inside a trip, a
    tail of up to three, the fold over the rl thread-rows) and in the backward reduce pass (one row at a time)"""
    _, rpb, _, rl = pl[:4]
    n_t = rpb // rl
    return n_t // 4 + 2 + 3 + (rl - 1), n_t + (rl - 1)


# ------------------------------------------------------------------------------------------------ float64 references
def _stats_ref(ranks, chains):
    """float64 batch statistics of the concatenated `ranks` ([rows_r][C] fp32) and the bounds of what the statistics pass
    (pivot = first row of each rank, chain chains[r]) and the fp64 merge make of them"""
    allx = torch.cat(ranks).double()
    n_tot = allx.shape[0]
    st = Stats()
    st.rows = n_tot
    st.mean = allx.mean(0)
    st.var = ((allx - st.mean) ** 2).mean(0)
    st.invstd = (st.var + EPS).rsqrt()
    e_mean64, e_m2, locals_ = 0.0, 0.0, []
    for x, chain in zip(ranks, chains):
        xd = x.double()
        n = xd.shape[0]
        d = xd - xd[0]
        e_s = (chain + 1) * U * d.abs().sum(0)            # (+1: the subtraction of the pivot)
        e_q = (chain + 3) * U * (d * d).sum(0)            # (+3: the subtraction, twice, and the product)
        e_m2 = e_m2 + e_q + 2 * d.sum(0).abs() * e_s / n + e_s ** 2 / n
        e_mean64 = e_mean64 + e_s / n_tot
        locals_.append((n, xd.mean(0), e_s / n))
    for n, m_r, e_mr in locals_:                          # M2 = sum M2_r + sum n_r (mean_r - mean)^2
        e_m2 = e_m2 + n * (2 * (m_r - st.mean).abs() * (e_mr + e_mean64) + (e_mr + e_mean64) ** 2)
    st.e_mean = e_mean64 + U * st.mean.abs()
    st.e_var = e_m2 / n_tot
    st.e_invstd = ((st.var - st.e_var).clamp_min(0) + EPS).rsqrt() - st.invstd + U * st.invstd
    return st


def _affine_ref(st, gamma, beta):
    """scale = gamma invstd, shift = beta - mean scale as the finalisation forms them in fp32, and their bounds"""
    sc = gamma * st.invstd
    e_sc = gamma.abs() * st.e_invstd + U * sc.abs()
    sh = beta - st.mean * sc
    e_sh = sc.abs() * st.e_mean + st.mean.abs() * e_sc + 2 * U * (beta.abs() + (st.mean * sc).abs())
    return sc, e_sc, sh, e_sh


def _pre_ref(x, res, aff):
    sc, e_sc, sh, e_sh = aff
    xd = x.double()
    pre = xd * sc + sh
    e = xd.abs() * e_sc + e_sh + 3 * U * ((xd * sc).abs() + sh.abs())
    if res is not None:
        pre = pre + res.double()
        e = e + 3 * U * res.double().abs()
    return pre, e


def _running_ref(st, rm0, rv0):
    unb = st.rows / (st.rows - 1.0) if st.rows > 1 else 1.0
    rm = (1 - MOM) * rm0 + MOM * st.mean
    rv = (1 - MOM) * rv0 + MOM * st.var * unb
    e_rm = MOM * st.e_mean + 3 * U * (((1 - MOM) * rm0).abs() + (MOM * st.mean).abs())
    e_rv = MOM * unb * (st.e_var + U * st.var) + 3 * U * (((1 - MOM) * rv0).abs() + (MOM * st.var * unb).abs())
    return rm, e_rm, rv, e_rv


def _mask_gradient(gen, pre, e_pre, relu, what):
    """upstream gradient with none where the float64 pre-activation does not decide the mask; (dy, g)"""
    dy = torch.randn(pre.shape, generator=gen) + 0.25
    if not relu:
        return dy, dy.double()
    unsure = pre.abs() <= e_pre
    share = unsure.double().mean().item()
    assert share <= LEFT_OUT, ('elements left without a gradient', what, share)
    dy = torch.where(unsure, torch.zeros_like(dy), dy)
    return dy, (dy * (pre > 0)).double()


# ------------------------------------------------------------------------------------------------ 2. plain forward / backward
def _p(name, rows, c, want, relu=True, res=False, affine=True, running=True, amax=True, mask='x', eval_=False):
    return dict(name=name, rows=rows, c=c, want=set(want), relu=relu, res=res, affine=affine, running=running, amax=amax,
                mask=mask, eval=eval_)


PLAIN = [
    # ---- workgroups
    _p('one_wg', 100, 64, {'nblk=1', 'n=7'}),
    _p('two_short', 1000, 64, {'nblk=2', 'short_last'}, res=True),
    _p('fold31', 15800, 64, {'nblk=31'}, relu=False),
    _p('fold32', 16300, 64, {'nblk=32'}, res=True, amax=False),
    _p('fold33', 16800, 64, {'nblk=33', 'short_last'}, mask='y'),
    _p('fold96', 49100, 64, {'nblk=96'}, affine=False),
    _p('fold97', 49600, 64, {'nblk=97'}, eval_=True),
    _p('fold128', 65500, 64, {'nblk=128'}, running=False),
    _p('fold129', 66000, 64, {'nblk=129', 'short_last'}, relu=False, res=True),
    _p('cap512', 270001, 64, {'nblk=512', 'cap', 'short_last'}),
    # ---- rows per thread-row: the unrolled loop alone (4), the tail alone (1, 3), both (5, 7), neither (0).  (A workgroup of
    # several holds about 32768 elements, 12 to 33 rows per thread-row: the small counts exist in single workgroups only.)
    _p('rows_lt_rl', 5, 4, {'rows<rl', 'n=0', 'n=1', 'C=4'}),
    _p('one_row', 1, 4, {'rows<rl', 'n=0', 'n=1'}, relu=False, amax=False),
    _p('one_row_wide', 1, 2048, {'n=1', 'C=2048'}, res=True),
    _p('n3', 48, 64, {'n=3'}, mask='y'),
    _p('n4', 64, 64, {'n=4'}, eval_=True, res=True),
    _p('n5', 80, 64, {'n=5'}, affine=False, running=False),
    # ---- channels
    _p('c12', 77, 12, {'C=12', 'idle_thread'}, res=True),
    _p('c20', 77, 20, {'C=20', 'idle_thread'}, eval_=True),
    _p('c800', 50, 800, {'C=800', 'idle_thread'}),
    _p('c1028', 40, 1028, {'C=1028', 'second_trip'}, res=True),
    _p('c2048', 33, 2048, {'C=2048'}, relu=False),
    _p('chunk12', 6000, 12, {'chunk_base:12', 'nblk=3'}, res=True),
    _p('chunk20', 3500, 20, {'chunk_base:20'}, mask='y'),
    _p('chunk28', 2500, 28, {'chunk_base:28'}, eval_=True, relu=False),
    _p('chunk2044', 40, 2044, {'chunk_base:2044', 'C=2044', 'second_trip'}),
    # (c4 = 41 is the first chunk count whose fp32 reciprocal rounds DOWN: lane offsets 41, 82, 164 and 287 come out of the
    # multiplication one chunk too high, and only the correction steps of chunk_of bring them back)
    _p('chunk164', 500, 164, {'chunk_base:164'}, res=True),
]
assert len({c['name'] for c in PLAIN}) == len(PLAIN)
PLAIN_EDGES = ({f'nblk={k}' for k in (1, 2, 31, 32, 33, 96, 97, 128, 129, 512)} | {'cap', 'short_last', 'rows<rl', 'idle_thread', 'second_trip'} |
               {f'n={k}' for k in (0, 1, 3, 4, 5, 7)} | {f'C={k}' for k in (4, 12, 20, 800, 1028, 2044, 2048)} |
               {f'chunk_base:{k}' for k in (12, 20, 28, 164, 2044)} |
               {'relu', 'no_relu', 'res', 'no_res', 'no_affine', 'no_running', 'train0', 'eval', 'amax', 'no_amax', 'mask_x', 'mask_y'})


def _plain_tags(lib, case):
    rows, c = case['rows'], case['c']
    nblk, rpb, tpc, rl = _plan(lib, rows, c)[:4]
    c4 = c // 4
    t = {f'nblk={nblk}', f'C={c}'}
    if rows % rpb:
        t.add('short_last')
    if nblk == 512 and _plan(lib, 2 * rows, c)[0] == 512:
        t.add('cap')
    last = rows - (nblk - 1) * rpb
    per_thread_row = {-(-last // rl), last // rl} | ({rpb // rl} if nblk > 1 else set())
    t |= {f'n={k}' for k in per_thread_row}
    if rows < rl:
        t.add('rows<rl')
    if tpc * rl < 256:
        t.add('idle_thread')
    if c4 > tpc:
        t.add('second_trip')
    if 256 % c4 and -(-rows * c4 // 256) >= 64:
        t.add(f'chunk_base:{c}')     # apply workgroups whose first element is not at channel 0
    t |= {'relu' if case['relu'] else 'no_relu', 'res' if case['res'] else 'no_res', 'amax' if case['amax'] else 'no_amax'}
    if not case['affine']:
        t.add('no_affine')
    if case['eval']:
        t |= {'eval', 'train0'}
    elif not case['running']:
        t.add('no_running')
    if case['relu'] and not case['res']:
        t.add('mask_' + case['mask'])
    return t


@pytest.mark.parametrize('case', PLAIN, ids=lambda c: c['name'])
def test_plain_forward_backward_at_plan_edges(cuda, case):
    from ever_amd import _C
    lib = _C.load()
    rows, c, relu, name = case['rows'], case['c'], case['relu'], case['name']
    tags = _plain_tags(lib, case)
    assert case['want'] <= tags, f"{name} no longer covers {sorted(case['want'] - tags)}: plan {_plan(lib, rows, c)}"
    pl = _plan(lib, rows, c)
    chain_f, chain_b = _chains(pl)
    gen = torch.Generator().manual_seed(7000 + rows + c)
    x = _data(gen, rows, c)
    res = torch.randn(rows, c, generator=gen) if case['res'] else None
    gamma, beta, g64, b64 = _params(gen, c, case['affine'])
    b = Bufs(cuda)
    dev = lambda t: None if t is None else t.to(cuda)
    xd, resd, gd, bd = dev(x), dev(res), dev(gamma), dev(beta)
    ws, wsb = b.workspace(lib, rows, c)
    y, smean, sinv = b.out(rows * c), b.out(c), b.out(c)
    yam = b.out(lib.evk_absmax_words(), torch.int32) if case['amax'] else None
    flags = RELU if relu else 0
    st_ = _stream()
    if case['eval']:
        rm0, rv0 = 0.5 * torch.randn(c, generator=gen), 0.5 + torch.rand(c, generator=gen)
        st = _given_stats(rm0.double(), (rv0.double() + EPS).rsqrt(), torch.zeros(c, dtype=torch.float64), None)
        st.e_invstd = U * st.invstd
        rm, rv = dev(rm0), dev(rv0)
        _C.call('evk_bn_fwd_eval', xd.data_ptr(), _ptr(resd), _ptr(gd), _ptr(bd), rm.data_ptr(), rv.data_ptr(), EPS,
                y.data_ptr(), smean.data_ptr(), sinv.data_ptr(), rows, c, flags, ws.data_ptr(), wsb, _ptr(yam), st_)
        b.check((name, 'fwd_eval'))
        assert torch.equal(smean.cpu(), rm0), (name, 'save_mean of the eval forward is the running mean')
        _hold('save_invstd', sinv, st.invstd, st.e_invstd, (name, 'eval'))
        mean_in, inv_in = smean, sinv
    else:
        st = _stats_ref([x], [chain_f])
        rm0, rv0 = 0.5 * torch.randn(c, generator=gen), 0.5 + torch.rand(c, generator=gen)
        rm, rv = (dev(rm0.clone()), dev(rv0.clone())) if case['running'] else (None, None)
        _C.call('evk_bn_fwd_train', xd.data_ptr(), _ptr(resd), _ptr(gd), _ptr(bd), _ptr(rm), _ptr(rv), MOM, EPS, y.data_ptr(),
                smean.data_ptr(), sinv.data_ptr(), rows, c, flags, ws.data_ptr(), wsb, _ptr(yam), st_)
        b.check((name, 'fwd_train'))
        _hold('save_mean', smean, st.mean, st.e_mean, name)
        _hold('save_invstd', sinv, st.invstd, st.e_invstd, name)
        if case['running']:
            rm_ref, e_rm, rv_ref, e_rv = _running_ref(st, rm0.double(), rv0.double())
            _hold('running_mean', rm, rm_ref, e_rm, name)
            _hold('running_var', rv, rv_ref, e_rv, name)
    pre, e_pre = _pre_ref(x, res, _affine_ref(st, g64, b64))
    _hold('y', y.view(rows, c), pre.clamp_min(0) if relu else pre, e_pre, name)
    if case['amax']:
        _amax_holds(yam, y, (name, 'y'))

    # ---- backward.  The training case hands the kernel the float64 statistics rounded to fp32 (their error: the cast), so
    # that its bounds do not inherit the forward's; the eval case what the eval forward saved.
    dy, g = _mask_gradient(gen, pre, e_pre, relu, name)
    if not case['eval']:
        mean_in, inv_in = dev(st.mean.float()), dev(st.invstd.float())
        st = _given_stats(st.mean, st.invstd, U * st.mean.abs(), U * st.invstd)
    train = 0 if case['eval'] else 1
    dbeta_r, e_db, dgamma_r, e_dg, dx_r, e_dx = _bwd_ref(x, g, st, g64, train, chain_b)
    b2 = Bufs(cuda)
    ws2, _ = b2.workspace(lib, rows, c)
    dx = b2.out(rows * c)
    dres = b2.out(rows * c) if case['res'] else None
    dgam, dbet = (b2.out(c), b2.out(c)) if case['affine'] else (None, None)
    dam = b2.out(lib.evk_absmax_words(), torch.int32) if case['amax'] else None
    y_in = y if relu and (case['res'] or case['mask'] == 'y') else None
    dyd = dev(dy)
    _C.call('evk_bn_bwd', dyd.data_ptr(), xd.data_ptr(), _ptr(y_in), _ptr(gd), _ptr(bd), mean_in.data_ptr(), inv_in.data_ptr(),
            dx.data_ptr(), _ptr(dres), _ptr(dgam), _ptr(dbet), rows, c, flags, train, ws2.data_ptr(), wsb, _ptr(dam), st_)
    b2.check((name, 'bwd'))
    b.check((name, 'bwd, the forward buffers'))
    _hold('dx', dx.view(rows, c), dx_r, e_dx, name)
    if case['affine']:
        _hold('dbeta', dbet, dbeta_r, e_db, name)
        _hold('dgamma', dgam, dgamma_r, e_dg, name)
    if case['res']:
        assert torch.equal(dres.cpu().view(rows, c), g.float()), (name, 'd_residual is the masked gradient, bit for bit')
    if case['amax']:
        _amax_holds(dam, dx, (name, 'dx'))
    RAN.setdefault('plain', set()).update(tags)


# ------------------------------------------------------------------------------------------------ 3. no tolerance needed
@pytest.mark.parametrize('rows,c', [(4096, 64), (8192, 20)])
def test_statistics_do_not_move_with_the_data(cuda, rows, c):
    """x = d and x = 1024 + d, d multiples of 2^-10 in [-4, 4] whose channel sums are zero: both exact in fp32, and the sums
    of (x - pivot) are the same numbers in both runs — small enough to be exact, and rows a power of two (the finalisation
    multiplies by 1 / rows), so that the mean is 0 and 1024 exactly and x - mean the same numbers too.
    save_invstd, running_var, dgamma and dbeta must agree bit for bit; a kernel without the pivot loses var to cancellation."""
    from ever_amd import _C
    lib = _C.load()
    nblk, rpb, _, _ = _plan(lib, rows, c)[:4]
    assert nblk >= 4 and rpb * 8 < 2 ** 14 and rows & (rows - 1) == 0      # several workgroups; a workgroup's sum of |d - d0| <= 8 is exact
    gen = torch.Generator().manual_seed(31 + c)
    half = torch.randint(-4096, 4097, (rows // 2, c), generator=gen).float() / 1024
    d = torch.cat([half, -half])[torch.randperm(rows, generator=gen)]
    dy = (torch.randn(rows, c, generator=gen) + 0.25).to(cuda)
    gamma = (0.5 + torch.rand(c, generator=gen)).to(cuda)
    beta = torch.randn(c, generator=gen).to(cuda)
    st_ = _stream()
    got = []
    for shift in (0.0, 1024.0):
        x = d + shift
        assert torch.equal((x.double() - shift).float(), d)
        xd = x.to(cuda)
        b = Bufs(cuda)
        ws, wsb = b.workspace(lib, rows, c)
        y, smean, sinv, dx, dgam, dbet = b.out(rows * c), b.out(c), b.out(c), b.out(rows * c), b.out(c), b.out(c)
        rm, rv = torch.zeros(c, device=cuda), torch.zeros(c, device=cuda)
        _C.call('evk_bn_fwd_train', xd.data_ptr(), None, gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), MOM, EPS,
                y.data_ptr(), smean.data_ptr(), sinv.data_ptr(), rows, c, 0, ws.data_ptr(), wsb, None, st_)
        _C.call('evk_bn_bwd', dy.data_ptr(), xd.data_ptr(), None, gamma.data_ptr(), beta.data_ptr(), smean.data_ptr(), sinv.data_ptr(),
                dx.data_ptr(), None, dgam.data_ptr(), dbet.data_ptr(), rows, c, 0, 1, ws.data_ptr(), wsb, None, st_)
        b.check(('shift', shift))
        assert torch.equal(smean.cpu(), torch.full((c,), shift)), ('the mean of the shifted data is the shift, exactly', shift)
        st = _stats_ref([x], [_chains(_plan(lib, rows, c))[0]])
        _hold('save_invstd', sinv, st.invstd, st.e_invstd, ('shift', shift, rows, c))
        got.append([t.cpu().clone() for t in (sinv, rv, dgam, dbet, dx)])
    for name, a, bb in zip(('save_invstd', 'running_var', 'dgamma', 'dbeta', 'dx'), *got):
        assert torch.isfinite(a).all() and torch.equal(a.view(torch.int32), bb.view(torch.int32)), (name, 'moved with the data', rows, c)


@pytest.mark.parametrize('rows,c', [(4000, 64), (6000, 12)])
def test_mask_from_x_equals_mask_from_y(cuda, rows, c):
    """A tenth of every channel's rows sits within a few ulp of the pre-activation's zero, on either side (beta is placed
    AFTER the statistics of the final x are known, so that the zero falls on the value those rows cluster around); channel 0
    has gamma = beta = 0 (a zero-initialised last BatchNorm of a residual block: every pre-activation is exactly 0).  The
    backward with y and the one that recomputes the mask from x must agree bit for bit, in the reduce pass and the apply pass."""
    from ever_amd import _C
    lib = _C.load()
    assert _plan(lib, rows, c)[0] >= 2
    gen = torch.Generator().manual_seed(77 + c)
    x = torch.randn(rows, c, generator=gen) + 3.0
    v = 2.5 + 0.25 * torch.rand(c, generator=gen)                     # the value a tenth of a channel's rows cluster around
    near = torch.rand(rows, c, generator=gen) < 0.1
    ulps = torch.randint(-6, 7, (rows, c), generator=gen)
    x = torch.where(near, (v.expand(rows, c).contiguous().view(torch.int32) + ulps.int()).view(torch.float32), x)
    xd = x.double()
    mean, invstd = xd.mean(0), (xd.var(0, unbiased=False) + EPS).rsqrt()
    gamma = 0.5 + torch.rand(c, generator=gen)
    beta = ((v.double() - mean) * gamma.double() * invstd * -1.0).float()        # gamma invstd (v - mean) + beta = 0
    gamma[0], beta[0] = 0.0, 0.0
    pre = (xd - mean) * invstd * gamma.double() + beta.double()
    close = pre.abs() <= 16 * U * ((xd * invstd * gamma.double()).abs() + (mean * invstd * gamma.double()).abs() + beta.double().abs())
    assert close[:, 1:].double().mean() >= 0.1 and (pre[close] > 0).any() and (pre[close] < 0).any()
    st_ = _stream()
    xg, gg, bg = x.to(cuda), gamma.to(cuda), beta.to(cuda)
    b = Bufs(cuda)
    ws, wsb = b.workspace(lib, rows, c)
    y, smean, sinv = b.out(rows * c), b.out(c), b.out(c)
    _C.call('evk_bn_fwd_train', xg.data_ptr(), None, gg.data_ptr(), bg.data_ptr(), None, None, MOM, EPS, y.data_ptr(), smean.data_ptr(),
            sinv.data_ptr(), rows, c, RELU, ws.data_ptr(), wsb, None, st_)
    b.check('mask: forward')
    yc = y.cpu().view(rows, c)
    on = yc > 0
    share = on[:, 1:][close[:, 1:]].double().mean().item()
    assert 0.2 < share < 0.8, ('the forward puts the clustered rows on both sides of zero', share)
    assert not on[:, 0].any()

    def backward(dy, y_in, train):
        b2 = Bufs(cuda)
        ws2, _ = b2.workspace(lib, rows, c)
        dx, dgam, dbet = b2.out(rows * c), b2.out(c), b2.out(c)
        _C.call('evk_bn_bwd', dy.data_ptr(), xg.data_ptr(), _ptr(y_in), gg.data_ptr(), bg.data_ptr(), smean.data_ptr(), sinv.data_ptr(),
                dx.data_ptr(), None, dgam.data_ptr(), dbet.data_ptr(), rows, c, RELU, train, ws2.data_ptr(), wsb, None, st_)
        b2.check('mask: backward')
        out = [t.cpu().clone() for t in (dx, dgam, dbet)]
        assert all(torch.isfinite(t).all() for t in out)
        return out

    dy = (torch.randn(rows, c, generator=gen) - 0.25).to(cuda)
    for train in (1, 0):
        for name, a, bb in zip(('dx', 'dgamma', 'dbeta'), backward(dy, y, train), backward(dy, None, train)):
            assert torch.equal(a.view(torch.int32), bb.view(torch.int32)), (name, 'the mask from x is not the mask from y', train)
    # the recomputed signs themselves: with dy = 1 and train = 0, dbeta counts the reduce pass's mask and dx = gamma invstd
    # where the apply pass's mask is set, 0 elsewhere
    dx, _, dbet = backward(torch.ones(rows, c, device=cuda), None, 0)
    assert torch.equal(dbet, on.sum(0).float()), 'reduce pass: the recomputed sign is not the sign of y'
    assert torch.equal(dx.view(rows, c)[:, 1:] != 0, on[:, 1:]), 'apply pass: the recomputed sign is not the sign of y'
    RAN.setdefault('mask', set()).add((rows, c))


# ---- split invariance of the statistics records
NPARTS = (1, 31, 33, 511, 512, 513, 1023, 1024, 1025, 2048)
PARTS_C = (4, 12, 64, 68)


def _records(gen, x, nparts, ragged=True, empty=0.25, first_empty=True):
    """[nparts][3][C] fp32 records (count, mean, M2) of consecutive row ranges of x, some of them empty"""
    rows, c = x.shape
    live = torch.rand(nparts, generator=gen) >= empty
    if first_empty and nparts > 1:
        live[0] = False
    k = int(live.sum())
    if k == 0 or k > rows:
        live[:] = False
        live[-min(nparts, rows):] = True
        k = int(live.sum())
    if ragged and k > 1:
        cuts = torch.sort(torch.randperm(rows - 1, generator=gen)[:k - 1] + 1).values.tolist()
    else:
        cuts = [rows * (i + 1) // k for i in range(k - 1)]
    bounds = [0] + cuts + [rows]
    rec = torch.zeros(nparts, 3, c, dtype=torch.float64)
    xd = x.double()
    for j, i in enumerate(torch.nonzero(live).flatten().tolist()):
        seg = xd[bounds[j]:bounds[j + 1]]
        rec[i, 0] = seg.shape[0]
        rec[i, 1] = seg.mean(0)
        rec[i, 2] = ((seg - seg.mean(0)) ** 2).sum(0)
    return rec.float()


def _merge_ref(rec):
    """Chan's merge of the fp32 records in float64"""
    r = rec.double()
    n, m, m2 = r[:, 0], r[:, 1], r[:, 2]
    tot = n.sum(0)
    mean = (n * m).sum(0) / tot
    return mean, (m2.sum(0) + (n * (m - mean) ** 2).sum(0)) / tot


@pytest.mark.parametrize('nparts', NPARTS)
def test_records_merge_the_same_however_they_are_split(cuda, nparts):
    """The same rows as `nparts` records — equal or ragged counts, empty records, the first among them — through
    evk_bn_finalize_parts and evk_bn_fwd_train_parts, against the float64 merge of the same fp32 records.  The merge runs in
    fp64: what remains is the cast of each output and the fp32 expressions of scale, shift and the running statistics."""
    from ever_amd import _C
    lib = _C.load()
    st_ = _stream()
    for c in PARTS_C:
        fc, fl = _plan(lib, nparts, c, 2)[2:4]
        for ragged, rows in ((True, max(96, 3 * nparts // 2)), (False, max(64, nparts)), (True, 1)):
            if rows == 1 and c != 12:
                continue
            gen = torch.Generator().manual_seed(nparts * 100 + c + ragged)
            x = _data(gen, rows, c) + 3.0
            rec = _records(gen, x, nparts, ragged, first_empty=rows > 1)
            assert int(rec[:, 0, 0].sum()) == rows
            what = (nparts, c, rows, 'ragged' if ragged else 'equal', f'<{fc}, {fl}>')
            mean, var = _merge_ref(rec)
            st = _given_stats(mean, (var + EPS).rsqrt(), 1.001 * U * mean.abs(), None)
            st.e_invstd = 1.001 * U * st.invstd
            st.rows, st.var, st.e_var = rows, var, 1e-12 * var
            gamma, beta, g64, b64 = _params(gen, c, True)
            rm0, rv0 = 0.5 * torch.randn(c, generator=gen), 0.5 + torch.rand(c, generator=gen)
            aff = _affine_ref(st, g64, b64)
            rm_ref, e_rm, rv_ref, e_rv = _running_ref(st, rm0.double(), rv0.double())
            recd, xd, gd, bd = rec.to(cuda), x.to(cuda), gamma.to(cuda), beta.to(cuda)
            for entry in ('finalize', 'fwd'):
                b = Bufs(cuda)
                smean, sinv, rm, rv = b.out(c), b.out(c), rm0.to(cuda), rv0.to(cuda)
                if entry == 'finalize':
                    ss = b.out(2 * c)
                    _C.call('evk_bn_finalize_parts', recd.data_ptr(), nparts, c, rows, gd.data_ptr(), bd.data_ptr(), rm.data_ptr(),
                            rv.data_ptr(), MOM, EPS, smean.data_ptr(), sinv.data_ptr(), ss.data_ptr(), st_)
                else:
                    ws, wsb = b.workspace(lib, rows, c)
                    y = b.out(rows * c)
                    _C.call('evk_bn_fwd_train_parts', xd.data_ptr(), None, gd.data_ptr(), bd.data_ptr(), rm.data_ptr(), rv.data_ptr(),
                            MOM, EPS, y.data_ptr(), smean.data_ptr(), sinv.data_ptr(), rows, c, 0, recd.data_ptr(), nparts,
                            ws.data_ptr(), wsb, None, st_)
                b.check(what + (entry,))
                _hold('parts mean', smean, st.mean, st.e_mean, what)
                _hold('parts invstd', sinv, st.invstd, st.e_invstd, what)
                _hold('parts run_mean', rm, rm_ref, e_rm, what)
                _hold('parts run_var', rv, rv_ref, e_rv, what)
                if entry == 'finalize':
                    _hold('parts scale', ss[:c], aff[0], aff[1], what)
                    _hold('parts shift', ss[c:], aff[2], aff[3], what)
                else:
                    pre, e_pre = _pre_ref(x, None, aff)
                    _hold('parts y', y.view(rows, c), pre, e_pre, what)
            if rows == 1:
                assert var.abs().max() == 0       # (and running_var above took the factor 1, not 1 / 0)
            RAN.setdefault('parts', set()).add((fc, fl))


# ------------------------------------------------------------------------------------------------ 4. the fused stem pass
POOL = [
    ((2, 17, 31, 64), {'odd_hw', 'pixel'}), ((1, 16, 31, 12), {'odd_w', 'pixel'}), ((3, 17, 16, 4), {'odd_h', 'pixel'}),
    ((2, 1, 1, 4), {'1x1', 'pixel'}), ((1, 1, 9, 8), {'h1', 'pixel'}), ((1, 2, 2, 4), {'2x2', 'quad'}), ((2, 3, 3, 20), {'odd_hw', 'pixel'}),
    ((2, 16, 16, 64), {'quad'}), ((1, 30, 34, 12), {'quad'}),
    ((2, 64, 64, 64), {'quad', 'several_wg:quad'}), ((2, 63, 65, 64), {'odd_hw', 'pixel', 'several_wg:pixel'}),
]
POOL_EDGES = {'odd_hw', 'odd_w', 'odd_h', '1x1', 'h1', '2x2', 'quad', 'pixel', 'several_wg:quad', 'several_wg:pixel'}


def _pool_tags(lib, shape):
    n, h, w, c = shape
    pl = _plan(lib, n * h * w, c, 1)
    quad = h % 2 == 0 and w % 2 == 0
    t = {'quad' if quad else 'pixel'}
    if h % 2 and w % 2 and h > 1:
        t.add('odd_hw')
    elif h % 2 and h > 1:
        t.add('odd_h')
    elif w % 2 and w > 1 and h > 1:
        t.add('odd_w')
    if (h, w) == (1, 1):
        t.add('1x1')
    elif h == 1:
        t.add('h1')
    if (h, w) == (2, 2):
        t.add('2x2')
    if (pl[4] if quad else pl[0]) >= 4:
        t.add('several_wg:' + ('quad' if quad else 'pixel'))
    return t, pl


def _pool_chain(pl, quad):
    nblk, rpb, _, rl, qn, qpb = pl
    return (4 * (qpb // rl) if quad else rpb // rl) + (rl - 1)


def _nchw(t, n, h, w, c):
    return t.view(n, h, w, c).permute(0, 3, 1, 2)


def _nhwc_rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _pool_forward(lib, cuda, x, rec, gamma, beta, shape, what):
    from ever_amd import _C
    n, h, w, c = shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    b = Bufs(cuda)
    ws, wsb = b.workspace(lib, n * h * w, c)
    y, code, smean, sinv = b.out(n * ho * wo * c), b.out(n * ho * wo * c, torch.uint8), b.out(c), b.out(c)
    am = b.out(lib.evk_absmax_words(), torch.int32)
    _C.call('evk_bn_relu_pool_fwd_train_parts', x.data_ptr(), _ptr(gamma), _ptr(beta), None, None, MOM, EPS, y.data_ptr(), code.data_ptr(),
            smean.data_ptr(), sinv.data_ptr(), n, h, w, c, rec.data_ptr(), rec.shape[0], ws.data_ptr(), wsb, am.data_ptr(), _stream())
    b.check(what)
    _amax_holds(am, y, what)
    return y, code, smean, sinv, b


def _pool_backward(lib, cuda, dp, code, x, gamma, beta, smean, sinv, shape, train, what):
    from ever_amd import _C
    n, h, w, c = shape
    b = Bufs(cuda)
    ws, wsb = b.workspace(lib, n * h * w, c)
    dx, dgam, dbet = b.out(n * h * w * c), b.out(c), b.out(c)
    am = b.out(lib.evk_absmax_words(), torch.int32)
    _C.call('evk_bn_relu_pool_bwd', dp.data_ptr(), code.data_ptr(), x.data_ptr(), _ptr(gamma), _ptr(beta), smean.data_ptr(), sinv.data_ptr(),
            dx.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), n, h, w, c, train, ws.data_ptr(), wsb, am.data_ptr(), _stream())
    b.check(what)
    _amax_holds(am, dx, what)
    return dx, dgam, dbet, b


def _one_record(x):
    """the rows of x as an empty record and one record (the statistics pass of the producing convolution stands behind them)"""
    xd = x.double()
    rec = torch.zeros(2, 3, x.shape[1], dtype=torch.float64)
    rec[1, 0], rec[1, 1], rec[1, 2] = x.shape[0], xd.mean(0), ((xd - xd.mean(0)) ** 2).sum(0)
    return rec.float()


@pytest.mark.parametrize('shape,want', POOL, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else '')
def test_stem_pass_against_fp64(cuda, shape, want):
    """BatchNorm + ReLU + MaxPool2d(3, 2, 1) forward and backward against float64 max_pool2d(relu(batch_norm(x))) and its
    gradients.  A window whose two best taps are closer than the forward bound, or whose winner is within the bound of zero,
    has no certain winner: it gets dp = 0 (at most 0.1 % of the windows).  Codes equal torch's return_indices on the rest
    wherever the maximum is positive."""
    from ever_amd import _C
    lib = _C.load()
    n, h, w, c = shape
    tags, pl = _pool_tags(lib, shape)
    assert want <= tags, f'{shape} no longer covers {sorted(want - tags)}: plan {pl}'
    quad = 'quad' in tags
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    rows = n * h * w
    gen = torch.Generator().manual_seed(900 + sum(shape))
    x = _data(gen, rows, c)
    gamma, beta, g64, b64 = _params(gen, c, True)
    rec = _one_record(x)
    xd = x.double()
    st = Stats()
    st.rows, st.mean, st.var = rows, xd.mean(0), xd.var(0, unbiased=False)
    st.invstd = (st.var + EPS).rsqrt()
    # the casts of the record's mean and M2 and of the outputs; the merge itself runs in fp64 around the first record's mean,
    # 0 for an empty one: var = (B - A^2 / N) / N cancels mean^2 at 2^-53
    st.e_mean, st.e_var = 2.001 * U * st.mean.abs(), 1.001 * U * st.var + 1e-14 * st.mean ** 2
    st.e_invstd = ((st.var - st.e_var).clamp_min(0) + EPS).rsqrt() - st.invstd + U * st.invstd
    pre, e_pre = _pre_ref(x, None, _affine_ref(st, g64, b64))
    pre4, e4 = _nchw(pre, n, h, w, c), _nchw(e_pre, n, h, w, c)
    z = pre4.clamp_min(0).clone().requires_grad_()
    p_ref, idx = TF.max_pool2d(z, 3, 2, 1, return_indices=True)
    assert p_ref.shape == (n, c, ho, wo)
    # per window: the two best pre-activations (padding never wins) and the largest bound among its taps
    inf = float('inf')
    win = TF.unfold(TF.pad(pre4, (1, 1, 1, 1), value=-inf), 3, stride=2).view(n, c, 9, -1)
    e_win = TF.unfold(TF.pad(e4, (1, 1, 1, 1), value=0.0), 3, stride=2).view(n, c, 9, -1).max(2).values.view(n, c, ho, wo)
    top = win.topk(2, dim=2).values
    top1, top2 = top[:, :, 0].view(n, c, ho, wo), top[:, :, 1].view(n, c, ho, wo)
    unsure = (top1.abs() <= e_win) | ((top1 > e_win) & (top1 - top2 <= 2 * e_win))
    assert unsure.double().mean().item() <= LEFT_OUT, ('windows left without a gradient', shape, unsure.double().mean().item())
    what = ('stem', shape)
    xg, gg, bg = x.to(cuda), gamma.to(cuda), beta.to(cuda)
    y, code, smean, sinv, fb = _pool_forward(lib, cuda, xg, rec.to(cuda), gg, bg, shape, what)
    _hold('pool mean', smean, st.mean, st.e_mean, what)
    _hold('pool invstd', sinv, st.invstd, st.e_invstd, what)
    _hold('pool y', _nchw(y.cpu(), n, ho, wo, c), p_ref.detach(), e_win, what)
    oy, ox = torch.arange(ho).view(1, 1, ho, 1), torch.arange(wo).view(1, 1, 1, wo)
    tap = (idx // w - (2 * oy - 1)) * 3 + (idx % w - (2 * ox - 1))
    decided = ~unsure & (top1 > e_win)
    got_tap = _nchw(code.cpu(), n, ho, wo, c).long()
    assert (got_tap <= 8).all(), ('a code nobody wrote', shape)
    assert torch.equal(got_tap[decided], tap[decided]), ('codes differ from return_indices', shape)

    dp = torch.randn(n, c, ho, wo, generator=gen) + 0.25
    dp = torch.where(unsure, torch.zeros_like(dp), dp)
    p_ref.backward(dp.double())
    live = (pre4 > 0).double()
    g4 = z.grad * live
    z.grad = None
    TF.max_pool2d(z, 3, 2, 1).backward(dp.double().abs())
    e_g = _nhwc_rows(3 * U * z.grad * live)        # a pixel sums the gradients of up to four windows in fp32
    dbeta_r, e_db, dgamma_r, e_dg, dx_r, e_dx = _bwd_ref(x, _nhwc_rows(g4), _given_stats(st.mean, st.invstd, st.e_mean, st.e_invstd),
                                                          g64, 1, _pool_chain(pl, quad), e_g=e_g)
    dpg = dp.permute(0, 2, 3, 1).contiguous().to(cuda)
    dx, dgam, dbet, _ = _pool_backward(lib, cuda, dpg, code, xg, gg, bg, smean, sinv, shape, 1, what)
    fb.check(what + ('the forward buffers',))
    _hold('pool dx', dx.view(rows, c), dx_r, e_dx, what)
    _hold('pool dbeta', dbet, dbeta_r, e_db, what)
    _hold('pool dgamma', dgam, dgamma_r, e_dg, what)
    RAN.setdefault('pool', set()).update(tags)


@pytest.mark.parametrize('crop', ['row', 'col', 'both'])
def test_stem_pass_quad_path_equals_pixel_path_on_shared_windows(cuda, crop):
    """An even map takes the quad kernels, the same map without its last row and / or column the per-pixel kernels.  With the
    same statistics records and train = 0 nothing couples distant pixels: on the windows that do not touch the cropped edge
    the two forwards must agree bit for bit (y and codes), and with dp = 0 on the windows that do touch it, dz of every
    shared pixel — hence its sum over any shared window — within the rounding of a pixel's up to four gradients."""
    from ever_amd import _C
    lib = _C.load()
    n, h, w, c = 2, 18, 22, 12
    gen = torch.Generator().manual_seed(5 + len(crop))
    x = _data(gen, n * h * w, c)
    gamma, beta, g64, _ = _params(gen, c, True)
    rec = _one_record(x).to(cuda)
    hc, wc = h - (crop in ('row', 'both')), w - (crop in ('col', 'both'))
    ho, wo = h // 2, w // 2
    assert ((hc - 1) // 2 + 1, (wc - 1) // 2 + 1) == (ho, wo)
    assert 'pixel' in _pool_tags(lib, (n, hc, wc, c))[0] and 'quad' in _pool_tags(lib, (n, h, w, c))[0]
    xc = x.view(n, h, w, c)[:, :hc, :wc].contiguous()
    dp = torch.randn(n, ho, wo, c, generator=gen) + 0.25
    if hc < h:
        dp[:, ho - 1] = 0
    if wc < w:
        dp[:, :, wo - 1] = 0
    gg, bg, dpg = gamma.to(cuda), beta.to(cuda), dp.to(cuda)
    out = []
    for shape, xs in (((n, h, w, c), x), ((n, hc, wc, c), xc)):
        xg = xs.to(cuda)
        y, code, smean, sinv, _ = _pool_forward(lib, cuda, xg, rec, gg, bg, shape, (crop, shape))
        dx, _, _, _ = _pool_backward(lib, cuda, dpg, code, xg, gg, bg, smean, sinv, shape, 0, (crop, shape))
        out.append((y.cpu().view(n, ho, wo, c), code.cpu().view(n, ho, wo, c), dx.cpu().view(n, shape[1], shape[2], c), sinv.cpu()))
    (y_e, code_e, dx_e, sinv_e), (y_o, code_o, dx_o, sinv_o) = out
    assert torch.equal(sinv_e, sinv_o)
    sy, sx = slice(0, ho - (hc < h)), slice(0, wo - (wc < w))
    assert torch.equal(y_e[:, sy, sx], y_o[:, sy, sx]) and torch.equal(code_e[:, sy, sx], code_o[:, sy, sx])
    assert torch.isfinite(dx_e).all() and torch.isfinite(dx_o).all() and dx_e.abs().max() > 0
    k0 = (g64 * sinv_e.double()).abs()
    iy, ix = torch.arange(hc), torch.arange(wc)
    absdz = 0.0         # sum of |dp| over the (up to four) windows a pixel is a tap of
    for wy in (iy // 2, ((iy + 1) // 2).clamp_max(ho - 1)):
        for wx in (ix // 2, ((ix + 1) // 2).clamp_max(wo - 1)):
            absdz = absdz + dp.abs().double()[:, wy][:, :, wx]
    bound = k0 * 6 * U * absdz + 2 * U * dx_e[:, :hc, :wc].abs().double()
    _hold('quad vs pixel', dx_o, dx_e[:, :hc, :wc].double(), bound, ('crop', crop))
    assert torch.equal(dx_e[:, hc:], torch.zeros_like(dx_e[:, hc:])) and torch.equal(dx_e[:, :, wc:], torch.zeros_like(dx_e[:, :, wc:]))
    RAN.setdefault('crop', set()).add(crop)


# ------------------------------------------------------------------------------------------------ 5. staged / partial-fed
@pytest.mark.parametrize('rows,c,split,relu,res', [(1500, 64, 600, True, False), (3001, 20, 3000, True, True), (700, 12, 350, False, False)])
def test_staged_entry_points_as_two_ranks(cuda, rows, c, split, relu, res):
    """evk_bn_local_stats on two row ranges, merged on the host as module/sync_bn.py merges ranks, then evk_bn_apply_stats,
    evk_bn_bwd_local_sums and evk_bn_bwd_apply_sums per range: the float64 BatchNorm over ALL rows within the bounds of the
    plain path (each range with the chain of its own plan)."""
    from ever_amd import _C
    from ever_amd.module.sync_bn import merge_local_stats
    lib = _C.load()
    st_ = _stream()
    gen = torch.Generator().manual_seed(rows + c)
    x = _data(gen, rows, c)
    resid = torch.randn(rows, c, generator=gen) if res else None
    gamma, beta, g64, b64 = _params(gen, c, True)
    ranks = [(0, split), (split, rows)]
    chains = [_chains(_plan(lib, r1 - r0, c)) for r0, r1 in ranks]
    st = _stats_ref([x[r0:r1] for r0, r1 in ranks], [ch[0] for ch in chains])
    flags = RELU if relu else 0
    gg, bg = gamma.to(cuda), beta.to(cuda)
    xs = [x[r0:r1].contiguous().to(cuda) for r0, r1 in ranks]
    rs = [resid[r0:r1].contiguous().to(cuda) if res else None for r0, r1 in ranks]
    bufs = Bufs(cuda)
    local = []
    for (r0, r1), xr in zip(ranks, xs):
        ws, wsb = bufs.workspace(lib, r1 - r0, c)
        s = bufs.out(2 * c, torch.float64)
        _C.call('evk_bn_local_stats', xr.data_ptr(), s.data_ptr(), r1 - r0, c, ws.data_ptr(), wsb, st_)
        local.append(s)
    bufs.check('local_stats')
    mean64, var64, total = merge_local_stats(torch.stack(local), torch.tensor([float(r1 - r0) for r0, r1 in ranks], device=cuda, dtype=torch.float64))
    assert float(total) == rows
    mean, invstd = mean64.float(), torch.rsqrt(var64 + EPS).float()
    what = ('staged', rows, c)
    _hold('save_mean', mean, st.mean, st.e_mean, what)
    _hold('save_invstd', invstd, st.invstd, st.e_invstd, what)
    pre, e_pre = _pre_ref(x, resid, _affine_ref(st, g64, b64))
    ys = []
    for (r0, r1), xr, rr in zip(ranks, xs, rs):
        ws, wsb = bufs.workspace(lib, r1 - r0, c)
        y = bufs.out((r1 - r0) * c)
        _C.call('evk_bn_apply_stats', xr.data_ptr(), _ptr(rr), gg.data_ptr(), bg.data_ptr(), mean.data_ptr(), invstd.data_ptr(), y.data_ptr(),
                r1 - r0, c, flags, ws.data_ptr(), wsb, st_)
        ys.append(y)
    bufs.check('apply_stats')
    _hold('y', torch.cat(ys).view(rows, c), pre.clamp_min(0) if relu else pre, e_pre, what)
    dy, g = _mask_gradient(gen, pre, e_pre, relu, what)
    chain_b = max(ch[1] for ch in chains)
    dbeta_r, e_db, dgamma_r, e_dg, dx_r, e_dx = _bwd_ref(x, g, st, g64, 1, chain_b)
    sums, dres = [], []
    dys = [dy[r0:r1].contiguous().to(cuda) for r0, r1 in ranks]
    for (r0, r1), xr, y, dyr in zip(ranks, xs, ys, dys):
        ws, wsb = bufs.workspace(lib, r1 - r0, c)
        s = bufs.out(2 * c, torch.float64)
        dr = bufs.out((r1 - r0) * c) if res else None
        _C.call('evk_bn_bwd_local_sums', dyr.data_ptr(), xr.data_ptr(), _ptr(y if res else None), gg.data_ptr(),
                bg.data_ptr(), mean.data_ptr(), invstd.data_ptr(), _ptr(dr), s.data_ptr(), r1 - r0, c, flags, ws.data_ptr(), wsb, st_)
        sums.append(s)
        dres.append(dr)
    bufs.check('bwd_local_sums')
    tot = sums[0] + sums[1]
    assert torch.isfinite(tot).all()
    _hold('dbeta', tot[:c].float(), dbeta_r, e_db, what)
    _hold('dgamma', tot[c:].float(), dgamma_r, e_dg, what)
    means = (tot / total).float()
    mg, mgx = means[:c].contiguous(), means[c:].contiguous()
    dxs = []
    for (r0, r1), xr, dr, dyr in zip(ranks, xs, dres, dys):
        ws, wsb = bufs.workspace(lib, r1 - r0, c)
        dx = bufs.out((r1 - r0) * c)
        gsrc, gflags = (dr, 0) if res else (dyr, flags)
        _C.call('evk_bn_bwd_apply_sums', gsrc.data_ptr(), xr.data_ptr(), None, gg.data_ptr(), bg.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                mg.data_ptr(), mgx.data_ptr(), dx.data_ptr(), r1 - r0, c, gflags, ws.data_ptr(), wsb, st_)
        dxs.append(dx)
    bufs.check('bwd_apply_sums')
    _hold('dx', torch.cat(dxs).view(rows, c), dx_r, e_dx, what)
    if res:
        assert torch.equal(torch.cat(dres).cpu().view(rows, c), g.float())


@pytest.mark.parametrize('nparts', [1, 33, 129])
def test_backward_from_host_partials(cuda, nparts):
    """evk_bn_bwd_from_partials: the (sum g, sum g xhat) records formed on the host in float64 and cast, `nparts` of them
    (one, and both sides of the 32 fold lanes and their 4x unroll); dgamma, dbeta and dx against the float64 backward."""
    from ever_amd import _C
    lib = _C.load()
    rows, c = 1300, 20
    gen = torch.Generator().manual_seed(nparts)
    x = _data(gen, rows, c)
    g = torch.randn(rows, c, generator=gen) * (torch.rand(rows, c, generator=gen) < 0.6)
    gamma, _, g64, _ = _params(gen, c, True)
    xd = x.double()
    mean, invstd = xd.mean(0), (xd.var(0, unbiased=False) + EPS).rsqrt()
    st = _given_stats(mean, invstd, U * mean.abs(), U * invstd)
    xh = (xd - mean) * invstd
    edges = [rows * i // nparts for i in range(nparts + 1)]
    part = torch.stack([torch.stack([g.double()[a:b_].sum(0), (g.double() * xh)[a:b_].sum(0)]) for a, b_ in zip(edges[:-1], edges[1:])]).float()
    e_sums = tuple(U * part.double()[:, i].abs().sum(0) + U * part.double()[:, i].sum(0).abs() for i in (0, 1))
    dbeta_r, e_db, dgamma_r, e_dg, dx_r, e_dx = _bwd_ref(x, g.double(), st, g64, 1, 0, e_sums=e_sums)
    b = Bufs(cuda)
    ws = b.out(16 * c)
    dx, dgam, dbet = b.out(rows * c), b.out(c), b.out(c)
    am = b.out(lib.evk_absmax_words(), torch.int32)
    pg, gg, xg, gam, mu, isd = (t.to(cuda) for t in (part, g, x, gamma, mean.float(), invstd.float()))
    _C.call('evk_bn_bwd_from_partials', gg.data_ptr(), xg.data_ptr(), gam.data_ptr(), mu.data_ptr(), isd.data_ptr(), pg.data_ptr(), None, nparts, dx.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), rows, c, 0, 1,
            ws.data_ptr(), 16 * c * 4, am.data_ptr(), _stream())
    b.check(('from_partials', nparts))
    what = ('from_partials', nparts)
    _hold('dbeta', dbet, dbeta_r, e_db, what)
    _hold('dgamma', dgam, dgamma_r, e_dg, what)
    _hold('dx', dx.view(rows, c), dx_r, e_dx, what)
    _amax_holds(am, dx, what)


# ------------------------------------------------------------------------------------------------ the union
def test_the_cases_cover_every_edge():
    """Read from the plans the library answers (no launch): every edge of the plain path, of the records' merge and of the
    fused stem pass is owned by a case above; whatever ran in this process asserted the same edges."""
    from ever_amd import _C
    lib = _C.load()
    plain = set()
    for case in PLAIN:
        plain |= _plain_tags(lib, case)
    assert PLAIN_EDGES <= plain, sorted(PLAIN_EDGES - plain)
    merges = {_plan(lib, k, c, 2)[2:4] for k in NPARTS for c in PARTS_C}
    assert merges == {(8, 32), (2, 128), (1, 256)}, merges
    pool = set()
    for shape, want in POOL:
        tags, _ = _pool_tags(lib, shape)
        assert want <= tags, (shape, sorted(want - tags))
        pool |= tags
    assert POOL_EDGES <= pool, sorted(POOL_EDGES - pool)
    if 'plain' in RAN and len(RAN) >= 4:
        assert RAN['plain'] <= plain and RAN.get('pool', set()) <= pool and RAN.get('parts', set()) <= merges
    if WORST:
        print('\nworst error / bound per quantity:')
        for name, (r, what) in sorted(WORST.items()):
            print(f'  {name:16s} {r:6.3f}  ({what})')
