"""The two-map BatchNorm passes at the end of a residual block with a shortcut convolution (csrc/bn.hip: the two-map forms of
bn_apply_kernel and bn_bwd_partial_kernel, bn_bwd_apply_dual_kernel; include/ever_hip.h: evk_bn_fwd_train_parts_dual, evk_bn_bwd_dual),
through the C-ABI, BIT FOR BIT against the two-call path they replace: evk_bn_fwd_train_parts on the shortcut map, then
evk_bn_fwd_train_parts_bits on the main map with that result as the residual; evk_bn_bwd_bits on each map in the backward.

Shapes are the smallest at which each code path can go wrong, and every case asserts with the host-only evk_bn_plan that it
still has the property it is there for.  Outputs and workspaces of BOTH paths hold NaN before a launch and sit inside
sentinel-guarded allocations (tests/guard_common.py).  One case is also held against float64 under the bounds
tests/test_bn_gpu.py derives."""
import itertools

import pytest
import torch

from tests.test_bn_gpu import (EPS, MOM, U, Bufs, _affine_ref, _bwd_ref, _chains, _data, _given_stats, _hold, _mask_gradient,
                               _merge_ref, _params, _plan, _pre_ref, _ptr, _records, _stream)

pytestmark = pytest.mark.gpu

PACK_DX = 2
RELU = 1


def _lanes_rows(pl, rows):
    """most rows one thread-row of the first reduce workgroup walks"""
    _, rpb, _, rl = pl[:4]
    return -(-min(rpb, rows) // rl)


# rows, C, what the plan must show, (records of the main map, records of the shortcut map)
CASES = [
    (3, 4, 'below_one_workgroup', (1, 33)),
    (257, 8, 'ragged_elements_and_row_tail', (33, 600)),
    (4099, 64, 'several_blocks_ragged_last', (600, 1100)),
    (1031, 260, 'chunks_divide_nothing', (1100, 1)),
    (640, 2048, 'channel_loop', (33, 1100)),
]
FINAL_FORMS = {1: (8, 32), 33: (8, 32), 600: (2, 128), 1100: (1, 256)}


def _assert_edge(lib, rows, c, edge):
    pl = _plan(lib, rows, c)
    nblk, rpb, tpc, rl = pl[:4]
    n4 = rows * c // 4
    if edge == 'below_one_workgroup':
        assert n4 < 256 and nblk == 1, pl
    elif edge == 'ragged_elements_and_row_tail':
        assert n4 % 64 and n4 % 256 and 1 <= _lanes_rows(pl, rows) % 4 <= 3, (pl, n4)
    elif edge == 'several_blocks_ragged_last':
        assert nblk > 2 and rows % rpb and _lanes_rows(pl, rows) > 4, pl
    elif edge == 'chunks_divide_nothing':
        assert tpc == c // 4 == 65 and 256 % tpc and 64 % tpc and rl * tpc < 256, pl
    elif edge == 'channel_loop':
        assert c // 4 > tpc == 256 and rl == 1, pl
    else:
        raise AssertionError(edge)
    return pl


def _inputs(seed, rows, c, kind):
    gen = torch.Generator().manual_seed(seed)
    za, zb = _data(gen, rows, c), _data(gen, rows, c)
    if kind == 'constant':          # zero variance: invstd = eps^-1/2, xhat = 0
        za[:, 1] = 0.75
        zb[:, 2] = -1.5
    elif kind == 'large_mean':      # |mean| >> std: what the pivots of the records are for
        za[:, 1] += 3.0e3
        zb[:, 0] -= 1.0e4
    return gen, za, zb


def _amax_buf(lib, dev):
    return torch.zeros((int(lib.evk_absmax_words()),), device=dev, dtype=torch.int32)


def _forward_pair(lib, dev, za, zb, pa, pb, reca, recb, rm0, rv0, dual, bufs):
    """(y, bits, save_mean_a, save_invstd_a, save_mean_b, save_invstd_b, rm_a, rv_a, rm_b, rv_b, y_absmax)"""
    from ever_amd import _C
    rows, c = za.shape
    st = _stream()
    (ga, ba), (gb, bb) = pa, pb
    new = bufs.out
    y, sma, sia, smb, sib = new(rows * c), new(c), new(c), new(c), new(c)
    bits = new(lib.evk_relu_bits_bytes(rows * c) // 4, torch.int32)
    rma, rva, rmb, rvb = (t.clone() for t in (rm0[0], rv0[0], rm0[1], rv0[1]))
    amax = _amax_buf(lib, dev)
    wsb = lib.evk_bn_workspace_bytes(rows, c) * (2 if dual else 1)
    ws = new(wsb // 4)
    if dual:
        _C.call('evk_bn_fwd_train_parts_dual', za.data_ptr(), zb.data_ptr(), _ptr(ga), _ptr(ba), rma.data_ptr(), rva.data_ptr(),
                MOM, EPS, _ptr(gb), _ptr(bb), rmb.data_ptr(), rvb.data_ptr(), MOM, EPS, y.data_ptr(), sma.data_ptr(),
                sia.data_ptr(), smb.data_ptr(), sib.data_ptr(), rows, c, reca.data_ptr(), reca.shape[0], recb.data_ptr(),
                recb.shape[0], ws.data_ptr(), wsb, amax.data_ptr(), bits.data_ptr(), st)
    else:
        yb = new(rows * c)
        _C.call('evk_bn_fwd_train_parts', zb.data_ptr(), None, _ptr(gb), _ptr(bb), rmb.data_ptr(), rvb.data_ptr(), MOM, EPS,
                yb.data_ptr(), smb.data_ptr(), sib.data_ptr(), rows, c, 0, recb.data_ptr(), recb.shape[0], ws.data_ptr(), wsb,
                _amax_buf(lib, dev).data_ptr(), st)
        _C.call('evk_bn_fwd_train_parts_bits', za.data_ptr(), yb.data_ptr(), _ptr(ga), _ptr(ba), rma.data_ptr(), rva.data_ptr(),
                MOM, EPS, y.data_ptr(), sma.data_ptr(), sia.data_ptr(), rows, c, RELU, reca.data_ptr(), reca.shape[0],
                ws.data_ptr(), wsb, amax.data_ptr(), bits.data_ptr(), st)
    return dict(y=y, bits=bits, save_mean_a=sma, save_invstd_a=sia, save_mean_b=smb, save_invstd_b=sib, running_mean_a=rma,
                running_var_a=rva, running_mean_b=rmb, running_var_b=rvb, y_absmax=amax)


def _backward_pair(lib, dev, dy, za, zb, pa, pb, fwd, pack_a, pack_b, dual, bufs):
    from ever_amd import _C
    rows, c = za.shape
    st = _stream()
    (ga, ba), (gb, bb) = pa, pb
    new = bufs.out
    dza, dzb = new(rows * c), new(rows * c)
    grads = [new(c) if g is not None else None for g in (ga, ga, gb, gb)]
    amax_a, amax_b = _amax_buf(lib, dev), _amax_buf(lib, dev)
    wsb = lib.evk_bn_workspace_bytes(rows, c) * (2 if dual else 1)
    ws = new(wsb // 4)
    fa, fb = (PACK_DX if pack_a else 0), (PACK_DX if pack_b else 0)
    if dual:
        _C.call('evk_bn_bwd_dual', dy.data_ptr(), za.data_ptr(), zb.data_ptr(), _ptr(ga), fwd['save_mean_a'].data_ptr(),
                fwd['save_invstd_a'].data_ptr(), _ptr(gb), fwd['save_mean_b'].data_ptr(), fwd['save_invstd_b'].data_ptr(),
                dza.data_ptr(), dzb.data_ptr(), _ptr(grads[0]), _ptr(grads[1]), _ptr(grads[2]), _ptr(grads[3]), rows, c, fa, fb,
                ws.data_ptr(), wsb, amax_a.data_ptr(), amax_b.data_ptr(), fwd['bits'].data_ptr(), st)
    else:
        _C.call('evk_bn_bwd_bits', dy.data_ptr(), za.data_ptr(), None, _ptr(ga), _ptr(ba), fwd['save_mean_a'].data_ptr(),
                fwd['save_invstd_a'].data_ptr(), dza.data_ptr(), None, _ptr(grads[0]), _ptr(grads[1]), rows, c, RELU | fa, 1,
                ws.data_ptr(), wsb, amax_a.data_ptr(), fwd['bits'].data_ptr(), st)
        _C.call('evk_bn_bwd_bits', dy.data_ptr(), zb.data_ptr(), None, _ptr(gb), _ptr(bb), fwd['save_mean_b'].data_ptr(),
                fwd['save_invstd_b'].data_ptr(), dzb.data_ptr(), None, _ptr(grads[2]), _ptr(grads[3]), rows, c, fb, 1,
                ws.data_ptr(), wsb, amax_b.data_ptr(), fwd['bits'].data_ptr(), st)
    out = dict(dza=dza, dzb=dzb, dza_absmax=amax_a, dzb_absmax=amax_b)
    for name, g in zip(('dgamma_a', 'dbeta_a', 'dgamma_b', 'dbeta_b'), grads):
        if g is not None:
            out[name] = g
    return out


def _same_bits(got, ref, what):
    for k in ref:
        a, b = got[k].view(torch.int32), ref[k].view(torch.int32)     # (bit images: NaN payloads and packed words alike)
        assert torch.equal(a, b), (k, what, int((a != b).sum()), 'of', a.numel(), 'words differ')


def _run_case(cuda, rows, c, nparts, kind, affine, seed):
    from ever_amd import _C
    lib = _C.load()
    gen, za, zb = _inputs(seed, rows, c, kind)
    reca = _records(gen, za, nparts[0]).to(cuda)
    recb = _records(gen, zb, nparts[1], ragged=False, first_empty=False).to(cuda)
    pa = tuple(None if t is None else t.to(cuda) for t in _params(gen, c, affine)[:2])
    pb = tuple(None if t is None else t.to(cuda) for t in _params(gen, c, affine)[:2])
    rm0 = [(0.5 * torch.randn(c, generator=gen)).to(cuda) for _ in range(2)]
    rv0 = [(0.5 + torch.rand(c, generator=gen)).to(cuda) for _ in range(2)]
    dy = (torch.randn(rows, c, generator=gen) + 0.25).to(cuda)
    za, zb = za.to(cuda), zb.to(cuda)
    what = (rows, c, nparts, kind, 'affine' if affine else 'plain')
    bufs, ref_bufs = Bufs(cuda), Bufs(cuda)
    ref = _forward_pair(lib, cuda, za, zb, pa, pb, reca, recb, rm0, rv0, False, ref_bufs)
    got = _forward_pair(lib, cuda, za, zb, pa, pb, reca, recb, rm0, rv0, True, bufs)
    ref_bufs.check(what + ('forward', 'two-call path'))
    bufs.check(what + ('forward',))
    _same_bits(got, ref, what + ('forward',))
    share = (ref['y'] > 0).float().mean().item()
    assert 0.05 < share < 0.95, ('the ReLU must cut some elements and pass others', what, share)
    for pack_a, pack_b in itertools.product((False, True), repeat=2):
        fused = lib.evk_bn_bwd_dual_fused(PACK_DX if pack_a else 0, PACK_DX if pack_b else 0)
        assert fused == (0 if (pack_a and not pack_b) else 1), (pack_a, pack_b, fused)
        bufs, ref_bufs = Bufs(cuda), Bufs(cuda)
        ref_b = _backward_pair(lib, cuda, dy, za, zb, pa, pb, ref, pack_a, pack_b, False, ref_bufs)
        got_b = _backward_pair(lib, cuda, dy, za, zb, pa, pb, got, pack_a, pack_b, True, bufs)
        ref_bufs.check(what + ('backward', pack_a, pack_b, 'two-call path'))
        bufs.check(what + ('backward', pack_a, pack_b))
        _same_bits(got_b, ref_b, what + ('backward', 'packed' if pack_a else 'fp32', 'packed' if pack_b else 'fp32',
                                         'two-map' if fused else 'two-call inside'))
        for k in ('dza', 'dzb'):
            assert not torch.isnan(got_b[k]).any() or (pack_a if k == 'dza' else pack_b), (k, 'holds an element nobody wrote', what)


@pytest.mark.parametrize('rows,c,edge,nparts', CASES, ids=lambda v: str(v) if not isinstance(v, tuple) else 'x'.join(map(str, v)))
@pytest.mark.parametrize('affine', [True, False], ids=['affine', 'no_affine'])
def test_two_map_passes_equal_the_two_call_path_bit_for_bit(cuda, rows, c, edge, nparts, affine):
    from ever_amd import _C
    lib = _C.load()
    _assert_edge(lib, rows, c, edge)
    for n in nparts:
        assert _plan(lib, n, c, 2)[2:4] == FINAL_FORMS[n], (n, _plan(lib, n, c, 2))
    _run_case(cuda, rows, c, nparts, 'gaussian', affine, 1000 + rows + c)


def test_the_cases_reach_every_form_of_the_record_merge():
    from ever_amd import _C
    lib = _C.load()
    seen = {_plan(lib, n, c, 2)[2:4] for _, c, _, pair in CASES for n in pair}
    assert seen == {(8, 32), (2, 128), (1, 256)}, seen
    assert {n for *_, pair in CASES for n in pair} == {1, 33, 600, 1100}


@pytest.mark.parametrize('nparts,form', [((33, 7), (8, 32)), ((600, 520), (2, 128)), ((1100, 1030), (1, 256))], ids=str)
def test_one_launch_merges_of_both_record_sets(cuda, nparts, form):
    """Where both record sets take the same form of the merge, one launch finishes both BatchNorms (a row of workgroups each);
    the cases above mix forms (two launches) except the first."""
    from ever_amd import _C
    lib = _C.load()
    for rows, c in ((257, 8), (1031, 260)):
        assert all(_plan(lib, n, c, 2)[2:4] == form for n in nparts), (nparts, form)
        _run_case(cuda, rows, c, nparts, 'gaussian', True, 500 + rows + nparts[0])


@pytest.mark.parametrize('kind', ['constant', 'large_mean'])
def test_degenerate_channels_equal_the_two_call_path(cuda, kind):
    """a channel of zero variance; a channel whose mean is thousands of standard deviations away"""
    _run_case(cuda, 4099, 64, (33, 600), kind, True, 77)
    _run_case(cuda, 257, 8, (1, 33), kind, True, 78)


def test_two_map_passes_against_float64(cuda):
    """y, dza, dzb and the four parameter gradients of the two-map passes against float64 computed from the same fp32 inputs,
    under the bounds of tests/test_bn_gpu.py: the pre-activation is the sum of two BatchNorm outputs (each with the bound of
    a single one, plus the rounding of the add: 3 u |shortcut term| as for a stored residual there)."""
    from ever_amd import _C
    lib = _C.load()
    rows, c, nparts = 4099, 64, (33, 600)
    pl = _assert_edge(lib, rows, c, 'several_blocks_ragged_last')
    chain = _chains(pl)[1]
    gen, za, zb = _inputs(5, rows, c, 'gaussian')
    what = (rows, c, 'float64')
    maps = []
    for z, n in ((za, nparts[0]), (zb, nparts[1])):
        rec = _records(gen, z, n)
        mean, var = _merge_ref(rec)
        st = _given_stats(mean, (var + EPS).rsqrt(), 1.001 * U * mean.abs(), None)
        st.e_invstd = 1.001 * U * st.invstd
        gamma, beta, g64, b64 = _params(gen, c, True)
        pre, e_pre = _pre_ref(z, None, _affine_ref(st, g64, b64))
        maps.append(dict(z=z, rec=rec.to(cuda), st=st, gamma=gamma.to(cuda), beta=beta.to(cuda), g64=g64, pre=pre, e_pre=e_pre))
    a, b = maps
    pre = a['pre'] + b['pre']
    e_pre = a['e_pre'] + b['e_pre'] + 3 * U * b['pre'].abs()
    rm0 = [torch.zeros(c, device=cuda) for _ in range(2)]
    rv0 = [torch.ones(c, device=cuda) for _ in range(2)]
    zad, zbd = za.to(cuda), zb.to(cuda)
    pa, pb = (a['gamma'], a['beta']), (b['gamma'], b['beta'])
    bufs = Bufs(cuda)
    fwd = _forward_pair(lib, cuda, zad, zbd, pa, pb, a['rec'], b['rec'], rm0, rv0, True, bufs)
    bufs.check(what)
    _hold('dual y', fwd['y'].view(rows, c), pre.clamp_min(0), e_pre, what)
    dy, g = _mask_gradient(gen, pre, e_pre, True, what)
    bufs = Bufs(cuda)
    bwd = _backward_pair(lib, cuda, dy.to(cuda), zad, zbd, pa, pb, fwd, False, False, True, bufs)
    bufs.check(what)
    for m, tag in ((a, 'a'), (b, 'b')):
        dbeta, e_db, dgamma, e_dg, dx, e_dx = _bwd_ref(m['z'], g, m['st'], m['g64'], True, chain)
        _hold('dual dbeta_' + tag, bwd['dbeta_' + tag], dbeta, e_db, what)
        _hold('dual dgamma_' + tag, bwd['dgamma_' + tag], dgamma, e_dg, what)
        _hold('dual dz' + tag, bwd['dz' + tag].view(rows, c), dx, e_dx, what)


def test_bad_arguments_are_refused_before_any_launch(cuda):
    from ever_amd import _C
    lib = _C.load()
    t = torch.zeros(64, device=cuda)
    p = t.data_ptr()
    small = lib.evk_bn_workspace_bytes(4, 4)      # one single-map workspace: half of what the pair needs
    assert lib.evk_bn_fwd_train_parts_dual(p, p, None, None, None, None, 0.1, 1e-5, None, None, None, None, 0.1, 1e-5, p, p, p, p,
                                           p, 4, 4, p, 1, p, 1, p, small, None, p, None) == -4
    assert lib.evk_bn_fwd_train_parts_dual(p, p, None, None, None, None, 0.1, 1e-5, None, None, None, None, 0.1, 1e-5, p, p, p, p,
                                           p, 4, 4, p, 1, p, 1, p, 2 * small, None, None, None) == -1     # no ReLU bits
    assert lib.evk_bn_bwd_dual(p, p, p, None, p, p, None, p, p, p, p, None, None, None, None, 4, 6, 0, 0, p, 2 * small, None, None, p,
                               None) == -2                                                                 # C % 4
    assert lib.evk_bn_bwd_dual(p, p, p, None, p, p, None, p, p, p, p, None, None, None, None, 4, 4, PACK_DX, PACK_DX, p, 2 * small,
                               None, None, p, None) == -1                                                  # packed without a scale buffer
