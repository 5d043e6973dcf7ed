"""The fused BatchNorm + ReLU + narrow classifier pass (csrc/bn_dot.hip: evk_bn_relu_dot_fwd / _bwd) at its instantiation, grid
and LDS edges, through the C-ABI, against float64 computed on the CPU from the same fp32 inputs.

The statistics are INPUTS at this interface (scale_shift, save_mean, save_invstd are arrays the caller passes): the reference
is formed in float64 from the very fp32 arrays the kernel gets, so their error is zero and what remains is the kernel's own
arithmetic.  Shapes are picked WITH evk_bn_relu_dot_plan: a case names the edges it exists for (`want`) and fails with "no
longer covers" when the plan takes one away; the last test asserts the union.  Outputs and workspace hold NaN before a launch
and are slices of sentinel-guarded allocations (tests/bn_ref_common.py).

Reference:  y = relu(z sc + sh);  out = y w^T + b;  g = (y > 0) (dl w);  dw = dl^T y;  dbias = sum dl;  dbeta, dgamma, dz =
the BatchNorm backward of the masked g with batch statistics (tests/bn_ref_common.py: _bwd_ref, train = 1).

Bounds, derived (u = 2^-24; a fp32 sum along a chain of L roundings errs by at most L u sum|terms|; DESIGN.md §6b has the
measured worst error / bound):
  pre = z sc + sh: 3 u (|z sc| + |sh|) (the product, the sum, and one to spare for either contraction);  y: the same where
      pre > 0, nothing elsewhere (the mask is certain, below);
  out: sum_c |w| e_y + L_f u (sum_c |y w| + |b|), L_f = 4 NCH + 1 + 6 + 1: a lane's 4 NCH products, each rounded once and
      added once, the six butterfly levels, the bias;
  g: K u sum_k |dl_k w_kc| (K products, each rounded and added);
  dw: (L + 1) u sum_pix |y dl| + sum_pix |dl| e_y + u |dw|, dbias: L u sum|dl| + u |dbias|, L = ceil(pix_per_blk / 4) + 2:
      a wave owns every fourth pixel of the workgroup's range, the four waves fold in two levels, the workgroups are summed
      in fp64 and cast once;
  dbeta, dgamma, dz: _bwd_ref with that L, e_g above, and e_mean = e_invstd = 0.
ReLU mask: the upstream gradient dl is per pixel, so an element with an uncertain mask cannot simply go without one; every z
whose float64 pre-activation lies within its bound of zero is moved away BEFORE the launch and the case asserts that none is
left.  Exact zeros are planted instead: channel 0 has sc = 1, sh = 0 and z = 0 on a third of its rows, so that y == 0 in fp32
and fp64 alike and the mask must be off (`>`, not `>=`).
Packed dz (EVK_BN_PACK_DX): a word holds h = fp16(dz / s) and l = fp16(dz / s - h), s = 2^(E - 13) from the exponent E of
the bound in slot 0 (x3_common.hpp: split2h / pack_hl, op_scale).  |dz / s| < 2^14; the residual after h is at most 2^-11 of
it and exact in fp32; l keeps 11 bits of that, or rounds to the fp16 subnormal grid 2^-24: |dz - s (h + l)| <=
max(2^-22 |dz|, 2^-25 s), on top of the fp32 bound of dz itself."""
import ctypes
from functools import partial

import pytest
import torch

from tests.bn_ref_common import U, Bufs, _amax_holds, _bwd_ref, _data, _given_stats, _hold, _params, _ptr, _stream
from tests.guard_common import PAD

pytestmark = pytest.mark.gpu

PACK_DX = 2
WORST = {}              # quantity -> (error / bound, where), of this file's quantities
RAN = set()             # edges whose cases asserted them and ran
hold = partial(_hold, worst=WORST)


# ------------------------------------------------------------------------------------------------ plan and edges
def _plan(lib, rows, c, k):
    out = (ctypes.c_int32 * 5)()
    assert lib.evk_bn_relu_dot_plan(rows, c, k, out) == 0, (rows, c, k, lib.evk_last_error())
    return tuple(out)


def _d(name, rows, c, k, want, bias=True, dbias=True, affine=True, amax='f32'):
    return dict(name=name, rows=rows, c=c, k=k, want=set(want), bias=bias, dbias=dbias, affine=affine, amax=amax)


CASES = [
    # ---- every <NCH, KT> instantiation, both shapes that sit exactly on the LDS budget
    _d('i11_c4', 71, 4, 1, {'<1,1>', 'one_live_lane', 'short_last'}),
    _d('i14_c252', 70, 252, 3, {'<1,4>', 'k_guard'}, amax='pack'),
    _d('i116_c204', 70, 204, 16, {'<1,16>'}, bias=False),
    _d('i116_c64_k5', 133, 64, 5, {'<1,16>', 'k_guard'}, dbias=False),
    _d('i21_c260', 70, 260, 1, {'<2,1>', 'one_live_lane'}, affine=False),
    _d('i24_c512_budget', 70, 512, 4, {'<2,4>', 'lds_budget'}),
    _d('i41_c816', 70, 816, 1, {'<4,1>'}, amax='none'),
    _d('i44_c516_round', 133, 516, 3, {'<4,4>', 'nch3to4', 'one_live_lane', 'k_guard'}, amax='pack'),
    _d('i44_c640', 70, 640, 2, {'<4,4>', 'k_guard'}, bias=False, dbias=False),
    _d('i116_c256_k12_budget', 70, 256, 12, {'<1,16>', 'lds_budget', 'k_guard'}, affine=False, amax='none'),
    # ---- pixel ranges
    _d('rows1', 1, 8, 2, {'one_wg', 'rows=1'}),
    _d('rows3', 3, 8, 2, {'one_wg', 'rows=3'}, amax='pack'),
    _d('rows4', 4, 8, 2, {'one_wg', 'rows=4'}, bias=False),
    _d('rows5', 5, 8, 2, {'one_wg', 'rows=5'}, affine=False),
    _d('rows8', 8, 8, 2, {'one_wg', 'rows=8'}, amax='none'),
    _d('rows9', 9, 8, 2, {'one_wg', 'rows=9'}, dbias=False),
    _d('rows63', 63, 8, 2, {'one_wg', 'rows=63'}),
    _d('rows64', 64, 8, 2, {'one_wg', 'rows=64'}, amax='pack'),
    _d('rows65', 65, 8, 2, {'nblk=2', 'short_last'}),
    _d('rows129', 129, 8, 2, {'nblk=3', 'partner_out_midwalk'}, amax='pack'),
    _d('rows131072', 131072, 8, 2, {'nblk=2048', 'full_grid'}),
    _d('rows131073', 131073, 8, 2, {'nblk=2048', 'empty_wg'}),
    _d('rows262151', 262151, 8, 2, {'nblk=2048', 'cap', 'short_last'}, amax='pack'),
]
assert len({c['name'] for c in CASES}) == len(CASES)
EDGES = ({f'<{n},{k}>' for n, k in ((1, 1), (1, 4), (1, 16), (2, 1), (2, 4), (4, 1), (4, 4))} |
         {f'rows={r}' for r in (1, 3, 4, 5, 8, 9, 63, 64)} |
         {'lds_budget:256x12', 'lds_budget:512x4', 'nch3to4', 'one_live_lane', 'k_guard', 'one_wg', 'short_last', 'empty_wg', 'cap',
          'full_grid', 'partner_out_midwalk', 'neg_gamma', 'gamma0_beta_neg', 'gamma0_beta_pos', 'planted_zeros', 'no_affine',
          'no_bias', 'no_dbias', 'amax', 'no_amax', 'pack'})


def _tags(lib, case):
    rows, c, k = case['rows'], case['c'], case['k']
    nblk, ppb, nch, kt, lds = _plan(lib, rows, c, k)
    c4 = c // 4
    t = {f'<{nch},{kt}>', f'nblk={nblk}'}
    if lds == 65536:
        t |= {'lds_budget', f'lds_budget:{c}x{k}'}
    if c4 % 64 == 1:
        t.add('one_live_lane')            # the last live chunk of a lane row holds one lane
    if nch == 4 and c4 <= 192:
        t.add('nch3to4')                  # three chunks rounded up to four: the fourth is empty
    if kt > k:
        t.add('k_guard')
    live = -(-rows // ppb)                # workgroups that own a pixel
    last = rows - (live - 1) * ppb
    if nblk == 1:
        t |= {'one_wg', f'rows={rows}'}
    if live < nblk:
        t.add('empty_wg')
    if nblk > 1 and last < ppb:
        t.add('short_last')
    if nblk == 2048 and ppb > 64:
        t.add('cap')
    if nblk == 2048 and ppb == 64 and live == nblk and last == ppb:
        t.add('full_grid')
    # a wave walks pixels w, w + 8, ... of its workgroup's range with partners w + 4, ...: unless the range is a whole number
    # of trips, a last pixel's partner lies outside it, and in every workgroup but the last it is a pixel of the NEXT one
    if live > 1 and ppb % 8:
        t.add('partner_out_midwalk')
    t |= {'no_bias'} if not case['bias'] else set()
    t |= {'no_dbias'} if not case['dbias'] else set()
    t |= {'no_affine'} if not case['affine'] else {'neg_gamma', 'gamma0_beta_neg', 'gamma0_beta_pos'}
    t |= {{'f32': 'amax', 'none': 'no_amax', 'pack': 'pack'}[case['amax']], 'planted_zeros'}
    return t


# ------------------------------------------------------------------------------------------------ inputs and the reference
class Ref:
    pass


_REFS = {}


def _reference(lib, case):
    """seeded fp32 inputs of a case and its float64 reference with the bounds, computed once per process"""
    if case['name'] in _REFS:
        return _REFS[case['name']]
    rows, c, k = case['rows'], case['c'], case['k']
    nblk, ppb, nch, kt, _ = _plan(lib, rows, c, k)
    gen = torch.Generator().manual_seed(9000 + rows + 7 * c + 131 * k)
    z = _data(gen, rows, c)
    gamma, beta, g64, b64 = _params(gen, c, case['affine'])
    zd = z.double()
    mean = zd.mean(0).float()
    invstd = (zd.var(0, unbiased=False) + 1e-5).rsqrt().float()
    mean[0], invstd[0] = 0.0, 1.0                         # channel 0: sc = 1, sh = 0 (the planted zeros)
    if case['affine']:
        gamma[0], beta[0] = 1.0, 0.0
        gamma[1], beta[1] = 0.0, -0.75                    # sc = 0: the whole channel is masked
        gamma[2], beta[2] = 0.0, 0.5                      # sc = 0: the whole channel passes, dz = 0 all the same
        gamma[3] = -abs(gamma[3])
        g64, b64 = gamma.double(), beta.double()
    sc = (g64.float() * invstd)                           # fp32, as evk_bn_finalize_parts forms them
    sh = b64.float() - mean * sc
    assert sc[0] == 1.0 and sh[0] == 0.0
    z[::3, 0] = 0.0
    z[0, 0] = 0.0
    scd, shd = sc.double(), sh.double()

    def pre_of(zz):
        zs = zz.double() * scd
        return zs + shd, 3 * U * (zs.abs() + shd.abs())
    for _ in range(6):                                    # move every uncertain pre-activation away from zero
        pre, e_pre = pre_of(z)
        unsure = (pre.abs() <= e_pre) & (e_pre > 0)
        if not unsure.any():
            break
        z = torch.where(unsure, z + 0.25, z)
    pre, e_pre = pre_of(z)
    left = int(((pre.abs() <= e_pre) & (e_pre > 0)).sum())
    assert left == 0, ('elements whose ReLU mask the float64 pre-activation does not decide', case['name'], left)
    planted = (pre[:, 0] == 0) & (e_pre[:, 0] == 0)
    assert int(planted.sum()) >= -(-rows // 3) and bool((z[planted, 0] == 0).all())

    w = 0.5 * torch.randn(k, c, generator=gen)
    bias = torch.randn(k, generator=gen) if case['bias'] else None
    dl = torch.randn(rows, k, generator=gen) + 0.25
    on = pre > 0
    y, e_y = pre.clamp_min(0), e_pre * on
    wd, dld = w.double(), dl.double()
    r = Ref()
    r.plan = (nblk, ppb, nch, kt)
    r.z, r.sc_sh, r.mean, r.invstd, r.gamma, r.w, r.bias, r.dl = z, torch.stack([sc, sh]).contiguous(), mean, invstd, gamma, w, bias, dl
    lf = 4 * nch + 1 + 6 + 1
    bd = bias.double() if bias is not None else torch.zeros(k, dtype=torch.float64)
    r.out = y @ wd.T + bd
    r.e_out = e_y @ wd.abs().T + lf * U * (y @ wd.abs().T + bd.abs())
    g = (dld @ wd) * on
    e_g = k * U * (dld.abs() @ wd.abs()) * on
    chain = -(-ppb // 4) + 2
    r.dw = dld.T @ y
    r.e_dw = (chain + 1) * U * (dld.abs().T @ y) + dld.abs().T @ e_y + U * r.dw.abs()
    r.dbias = dld.sum(0)
    r.e_dbias = chain * U * dld.abs().sum(0) + U * r.dbias.abs()
    zero = torch.zeros(c, dtype=torch.float64)
    st = _given_stats(mean.double(), invstd.double(), zero, zero)
    r.dbeta, r.e_dbeta, r.dgamma, r.e_dgamma, r.dz, r.e_dz = _bwd_ref(z, g, st, g64, 1, chain, e_g=e_g)
    # what the planted zeros are for: with the mask on they would carry a gradient (k0 = 1 there) above the bound of dz
    assert bool(((dld @ wd)[planted, 0].abs() > r.e_dz[planted, 0]).any())
    _REFS[case['name']] = r
    return r


def _op_scale(bits):
    """x3_common.hpp: op_scale"""
    e = (bits >> 23) & 0xff
    f = 127 if e in (0, 255) else e - 13
    return 2.0 ** (max(f, 1) - 127)


class Run:
    pass


def _launch(lib, cuda, case, r):
    """forward and backward of a case; every output NaN-filled and guarded; returns the device outputs"""
    from ever_amd import _C
    rows, c, k = case['rows'], case['c'], case['k']
    dev = lambda t: None if t is None else t.to(cuda)
    z, ss, mean, invstd, gamma, w, bias, dl = (dev(t) for t in (r.z, r.sc_sh, r.mean, r.invstd, r.gamma, r.w, r.bias, r.dl))
    st_ = _stream()
    o = Run()
    o.b = b = Bufs(cuda)
    o.out = b.out(rows * k)
    _C.call('evk_bn_relu_dot_fwd', z.data_ptr(), ss.data_ptr(), w.data_ptr(), _ptr(bias), o.out.data_ptr(), rows, c, k, st_)
    b.check((case['name'], 'fwd'))
    wsb = lib.evk_bn_relu_dot_workspace_bytes(rows, c, k)
    ws = b.out(wsb // 4)
    o.dz, o.dw = b.out(rows * c), b.out(k * c)
    o.dgamma, o.dbeta = (b.out(c), b.out(c)) if case['affine'] else (None, None)
    o.dbias = b.out(k) if case['dbias'] else None
    o.slots = None if case['amax'] == 'none' else b.out(lib.evk_absmax_words(), torch.int32)
    flags = 0
    if case['amax'] == 'pack':
        o.slots.zero_()
        flags = PACK_DX
    _C.call('evk_bn_relu_dot_bwd', dl.data_ptr(), z.data_ptr(), ss.data_ptr(), _ptr(gamma), mean.data_ptr(), invstd.data_ptr(),
            w.data_ptr(), o.dz.data_ptr(), _ptr(o.dgamma), _ptr(o.dbeta), o.dw.data_ptr(), _ptr(o.dbias), rows, c, k, flags,
            ws.data_ptr(), wsb, _ptr(o.slots), st_)
    b.check((case['name'], 'bwd'))
    return o


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_forward_backward_against_fp64_at_plan_edges(cuda, case):
    from ever_amd import _C
    lib = _C.load()
    rows, c, k, name = case['rows'], case['c'], case['k'], case['name']
    tags = _tags(lib, case)
    assert case['want'] <= tags, f"{name} no longer covers {sorted(case['want'] - tags)}: plan {_plan(lib, rows, c, k)}"
    r = _reference(lib, case)
    o = _launch(lib, cuda, case, r)
    hold('dot out', o.out.view(rows, k), r.out, r.e_out, name)
    hold('dot dw', o.dw.view(k, c), r.dw, r.e_dw, name)
    if case['dbias']:
        hold('dot dbias', o.dbias, r.dbias, r.e_dbias, name)
    if case['affine']:
        hold('dot dbeta', o.dbeta, r.dbeta, r.e_dbeta, name)
        hold('dot dgamma', o.dgamma, r.dgamma, r.e_dgamma, name)
    if case['amax'] != 'pack':
        hold('dot dz', o.dz.view(rows, c), r.dz, r.e_dz, name)
        if case['amax'] == 'f32':
            _amax_holds(o.slots, o.dz, (name, 'dz'))
    else:
        words = o.slots.cpu().view(64, 32)
        bits = int(words[0, 0])
        assert bool((words[1:, 0] == 0).all()) and bool((words[:, 1:] == 0).all()), ('packed dz: a word beside slot 0', name)
        top = torch.tensor([bits], dtype=torch.int32).view(torch.float32).double().item()
        assert top == top and top < float('inf'), ('packed dz: slot 0', name, hex(bits))
        assert top >= float((r.dz.abs() - r.e_dz).max()), ('packed dz: slot 0 below max|dz|', name, top, float(r.dz.abs().max()))
        s = _op_scale(bits)
        back = Bufs(cuda)
        dz = back.out(rows * c)
        _C.call('evk_unpack_f16x2', o.dz.data_ptr(), rows * c, o.slots.data_ptr(), dz.data_ptr(), _stream())
        back.check((name, 'unpack'))
        quant = torch.maximum(2.0 ** -22 * (r.dz.abs() + r.e_dz), torch.full_like(r.dz, 2.0 ** -25 * s))
        hold('dot dz packed', dz.view(rows, c), r.dz, r.e_dz + quant, name)
    o.b.check((name, 'after the reads'))
    RAN.update(tags)


def test_two_launches_give_the_same_bits(cuda):
    from ever_amd import _C
    lib = _C.load()
    for name in ('i44_c516_round', 'rows131073', 'i116_c64_k5'):
        case = next(cs for cs in CASES if cs['name'] == name)
        r = _reference(lib, case)
        runs = [_launch(lib, cuda, case, r) for _ in range(2)]
        for field in ('out', 'dz', 'dw', 'dgamma', 'dbeta', 'dbias', 'slots'):
            a, b = getattr(runs[0], field), getattr(runs[1], field)
            if a is None:
                continue
            a, b = a.cpu().view(torch.int32), b.cpu().view(torch.int32)
            assert torch.equal(a, b), (name, field, 'differs between two launches')


# ------------------------------------------------------------------------------------------------ refusals
def _untouched(b):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(whole[PAD:PAD + n]).all()) for whole, n in b.all)


@pytest.mark.parametrize('c,k,how,code', [(260, 5, 'shape', -2), (1024, 1, 'shape_bwd', -2), (64, 17, 'shape', -2), (6, 1, 'shape', -2),
                                          (64, 3, 'workspace', -4), (64, 3, 'pack_without_slots', -1)])
def test_refusals_return_their_code_and_store_nothing(cuda, c, k, how, code):
    """every one of these returns before any launch"""
    from ever_amd import _C
    lib = _C.load()
    rows = 70
    b = Bufs(cuda)
    n = rows * max(c, 8)
    z, ss, w, dl, vec = (torch.zeros(m, device=cuda) for m in (n, 2 * c + 8, 17 * c + 8, rows * 17, c + 8))
    out, dz, dw, dgamma, dbeta, dbias = b.out(rows * 17), b.out(n), b.out(17 * c), b.out(c), b.out(c), b.out(17)
    wsb = max(lib.evk_bn_relu_dot_workspace_bytes(rows, c, min(k, 16)), 1024)
    ws = b.out(wsb // 4)
    slots = b.out(lib.evk_absmax_words(), torch.int32)
    st_ = _stream()
    if how == 'shape':
        rc = lib.evk_bn_relu_dot_fwd(z.data_ptr(), ss.data_ptr(), w.data_ptr(), vec.data_ptr(), out.data_ptr(), rows, c, k, st_)
        assert rc == code and f'C={c} K={k}'.encode() in lib.evk_last_error(), (rc, lib.evk_last_error())
    flags, wsb_arg, slots_arg = 0, wsb, slots.data_ptr()
    if how == 'workspace':
        wsb_arg = lib.evk_bn_relu_dot_workspace_bytes(rows, c, k) - 1
    if how == 'pack_without_slots':
        flags, slots_arg = PACK_DX, None
    rc = lib.evk_bn_relu_dot_bwd(dl.data_ptr(), z.data_ptr(), ss.data_ptr(), vec.data_ptr(), vec.data_ptr(), vec.data_ptr(), w.data_ptr(),
                                 dz.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), dw.data_ptr(), dbias.data_ptr(), rows, c, k, flags,
                                 ws.data_ptr(), wsb_arg, slots_arg, st_)
    msg = lib.evk_last_error()
    assert rc == code and f'C={c} K={k}'.encode() in msg and b'bn_relu_dot_bwd' in msg, (rc, msg)
    b.check((c, k, how))
    assert _untouched(b), ('a refused call stored something', c, k, how)
    out5 = (ctypes.c_int32 * 5)()
    assert lib.evk_bn_relu_dot_plan(rows, c, k, out5) == (code if how.startswith('shape') else 0)


# ------------------------------------------------------------------------------------------------ the union
def test_the_cases_cover_every_edge():
    """Read from the plan the library answers (no launch): all seven instantiations, both shapes on the LDS budget, the
    one-workgroup, short-last, empty-workgroup, full and capped grids and the pack / absmax / NULL-pointer variants are owned by
    a case above; whatever ran in this process asserted the same edges."""
    from ever_amd import _C
    lib = _C.load()
    union = set()
    for case in CASES:
        tags = _tags(lib, case)
        assert case['want'] <= tags, (case['name'], sorted(case['want'] - tags))
        union |= tags
    assert EDGES <= union, sorted(EDGES - union)
    if len(_REFS) == len(CASES):
        assert EDGES <= RAN, sorted(EDGES - RAN)
    if WORST:
        print('\nworst error / bound per quantity:')
        for name, (ratio, what) in sorted(WORST.items()):
            print(f'  {name:16s} {ratio:6.3f}  ({what})')
