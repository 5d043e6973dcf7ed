"""FS-Relation with its two BatchNorm + ReLU passes inside (csrc/relation.hip: relation_fwd_kernel<true>,
relation_bn_bwd_kernel<NCH>) and the hand-over of its records to csrc/bn.hip: evk_bn_bwd_from_partials, at the lane, chunk,
LDS, workgroup and cap edges, through the C-ABI, against float64 computed on the CPU from the same fp32 inputs.

tests/relation_ref_common.py holds the reference, the derived bounds (u = 2^-24) and the cases; tests/test_relation_ref_cpu.py
holds that reference to autograd.  Every stage is referenced to float64 of ITS OWN fp32 inputs: the backward to the r the
forward stored, the records and the hand-over to the g the backward stored.  Outputs and the nine-section workspace hold NaN
before a launch and are slices of sentinel-guarded allocations (tests/bn_ref_common.py: Bufs); out_absmax and the packed
hand-over's dx_absmax are zeroed, as the interface asks ("zero on entry").

The worst error / bound per quantity measured on an MI355X is in DESIGN.md (FS-Relation with BatchNorm)."""
from functools import partial

import pytest
import torch

from tests import relation_ref_common as R
from tests.bn_ref_common import Bufs, _amax_holds, _hold, _ptr, _stream
from tests.guard_common import PAD

pytestmark = pytest.mark.gpu

PACK_DX = 2
E_INVALID, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -4
WORST = {}              # quantity -> (error / bound, where), of this file's quantities
hold = partial(_hold, worst=WORST)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _amax_zeroed_holds(words, out, what):
    """_amax_holds on slots that arrive zero: the maximum over the 64 slots (a cache line apart) is max|out| bit for bit; no
    word between the slots was touched"""
    w = words.cpu().view(64, 32)
    want = int(out.abs().max().reshape(1).cpu().view(torch.int32))
    assert int(w[:, 0].max()) == want, ('out_absmax', what, hex(int(w[:, 0].max())), hex(want))
    assert bool((w[:, 1:] == 0).all()), ('out_absmax: a word between the slots', what)


def _op_scale(bits):
    """x3_common.hpp: op_scale"""
    e = (bits >> 23) & 0xff
    f = 127 if e in (0, 255) else e - 13
    return 2.0 ** (max(f, 1) - 127)


class Run:
    pass


def _device(k, cuda):
    d = Run()
    for name in ('scene', 'zc', 'zf', 'ss_c', 'ss_f', 'mi_c', 'mi_f', 'gamma_c', 'gamma_f', 'dout'):
        setattr(d, name, getattr(k, name).to(cuda))
    return d


def _forward(lib, cuda, k, d, slots='zeroed', ss_f=None):
    """evk_relation_bn_fwd into NaN-filled, guarded out and r"""
    from ever_amd import _C
    o = Run()
    o.b = b = Bufs(cuda)
    o.out, o.r = b.out(k.rows * k.c), b.out(k.rows)
    o.slots = None
    if slots == 'zeroed':
        o.slots = b.out(lib.evk_absmax_words(), torch.int32)
        o.slots.zero_()
    _C.call('evk_relation_bn_fwd', d.scene.data_ptr(), d.zc.data_ptr(), d.ss_c.data_ptr(), d.zf.data_ptr(),
            (d.ss_f if ss_f is None else ss_f).data_ptr(), o.out.data_ptr(), o.r.data_ptr(), k.n, k.hw, k.c, _ptr(o.slots), _stream())
    b.check((k.name, 'fwd'))
    return o


def _pipeline(lib, cuda, k, d):
    """forward, backward and both forms of the hand-over for both BatchNorms; every output NaN-filled and guarded"""
    from ever_amd import _C
    n, c, hw, rows = k.n, k.c, k.hw, k.rows
    o = _forward(lib, cuda, k, d)
    b, st_ = o.b, _stream()
    nb = lib.evk_relation_bn_parts(n, hw)
    wsb = lib.evk_relation_bn_workspace_bytes(n, hw, c)
    assert wsb == nb * c * 9 * 4
    o.ws = b.out(wsb // 4)
    o.dscene, o.gc, o.gf = b.out(n * c), b.out(rows * c), b.out(rows * c)
    _C.call('evk_relation_bn_bwd', d.dout.data_ptr(), d.scene.data_ptr(), d.zc.data_ptr(), d.ss_c.data_ptr(), d.mi_c.data_ptr(),
            d.zf.data_ptr(), d.ss_f.data_ptr(), d.mi_f.data_ptr(), o.r.data_ptr(), o.dscene.data_ptr(), o.gc.data_ptr(),
            o.gf.data_ptr(), n, hw, c, o.ws.data_ptr(), wsb, st_)
    b.check((k.name, 'bwd'))
    coef = b.out(16 * c)
    o.hand = []
    for br, (g, z, gamma, mi) in enumerate(((o.gc, d.zc, d.gamma_c, d.mi_c), (o.gf, d.zf, d.gamma_f, d.mi_f))):
        sums = o.ws[nb * c * (1 + 4 * br):]             # the offsets hip/pointwise.py hands over
        maxima = o.ws[nb * c * (3 + 4 * br):]
        h = Run()
        for pack in (False, True):
            dz, dgamma, dbeta = b.out(rows * c), b.out(c), b.out(c)
            slots = b.out(lib.evk_absmax_words(), torch.int32)
            if pack:
                slots.zero_()
            _C.call('evk_bn_bwd_from_partials', g.data_ptr(), z.data_ptr(), gamma.data_ptr(), mi[0].data_ptr(), mi[1].data_ptr(),
                    sums.data_ptr(), maxima.data_ptr(), nb, dz.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), rows, c,
                    PACK_DX if pack else 0, 1, coef.data_ptr(), 16 * c * 4, slots.data_ptr(), st_)
            b.check((k.name, 'hand-over', br, pack))
            if pack:
                h.dz_p, h.dgamma_p, h.dbeta_p, h.slots_p = dz, dgamma, dbeta, slots
            else:
                h.dz, h.dgamma, h.dbeta, h.slots = dz, dgamma, dbeta, slots
        o.hand.append(h)
    return o


def _everything(o):
    """every output and the workspace of a pipeline, as bits"""
    got = {name: _bits(getattr(o, name)) for name in ('out', 'r', 'slots', 'ws', 'dscene', 'gc', 'gf')}
    for br, h in enumerate(o.hand):
        for name in ('dz', 'dgamma', 'dbeta', 'slots', 'dz_p', 'dgamma_p', 'dbeta_p', 'slots_p'):
            got[f'{name}[{br}]'] = _bits(getattr(h, name))
    return got


def _check(lib, cuda, k, o):
    """every stage of a pipeline within its bound, the planted zeros, the records of the workgroups without pixels"""
    from ever_amd import _C
    n, c, hw, rows, name = k.n, k.c, k.hw, k.rows, k.name
    nb = lib.evk_relation_bn_parts(n, hw)
    nblk, ppb = R.ranges(nb, n, hw)
    f = k.fwd
    # ---- forward
    hold('rel r', o.r, f.r, f.e_r, name)
    out = o.out.cpu().view(rows, c)
    hold('rel out', out, f.out, f.e_out, name)
    assert bool((out[k.planted_f, 0] == 0).all()), ('out at a planted zero', name)
    _amax_zeroed_holds(o.slots, o.out, name)
    # ---- backward, from the r the forward stored
    r = o.r.cpu().double()
    bw = R.backward_stages(f, k.dout, k.scene_pix, r)
    gc, gf = o.gc.cpu().view(rows, c), o.gf.cpu().view(rows, c)
    hold('rel g_f', gf, bw.gf, bw.e_gf, name)
    hold('rel g_c', gc, bw.gc, bw.e_gc, name)
    assert bool((gf[k.planted_f, 0] == 0).all()) and bool((gc[k.planted_c, 0] == 0).all()), ('g at a planted zero', name)
    assert bool((gf[~f.on_f] == 0).all()) and bool((gc[~f.on_c] == 0).all()), ('g where the ReLU was off', name)
    ws = o.ws.cpu()
    assert not bool(torch.isnan(ws).any()), ('a workspace record nobody wrote', name, int(torch.isnan(ws).sum()))
    part, e_part, dscene, e_dscene = R.scene_records(bw, n, hw, nblk, ppb)
    hold('rel scene part', ws[:nb * c].view(nb, c), part, e_part, name)
    hold('rel dscene', o.dscene.view(n, c), dscene, e_dscene, name)
    live = -(-hw // ppb)                                  # workgroups of an image that own a pixel
    empty = torch.zeros(n, nblk, dtype=torch.bool)
    empty[:, live:] = True
    empty = empty.view(nb)
    assert bool((_bits(ws[:nb * c]).view(nb, c)[empty] == 0).all()), ('scene partial of a workgroup without pixels', name)
    # ---- records and hand-over, from the g the backward stored
    for br, (tag, z, g, mi, gamma) in enumerate((('c', k.zc, gc, k.mi_c, k.gamma_c), ('f', k.zf, gf, k.mi_f, k.gamma_f))):
        rec = R.bn_records(z, g, mi[0], mi[1], n, hw, nblk, ppb)
        sums = ws[nb * c * (1 + 4 * br):nb * c * (3 + 4 * br)].view(nb, 2, c)
        maxima = ws[nb * c * (3 + 4 * br):nb * c * (5 + 4 * br)].view(nb, 2, c)
        what = (name, tag)
        hold('rel sum g', sums[:, 0], rec.sg, rec.e_sg, what)
        hold('rel sum g xhat', sums[:, 1], rec.sgx, rec.e_sgx, what)
        assert torch.equal(_bits(maxima[:, 0]), _bits(rec.mg.float())), ('max|g| is not the maximum of the stored |g|', what)
        hold('rel max|xhat|', maxima[:, 1], rec.mx, rec.e_mx, what)
        assert bool((_bits(sums)[empty] == 0).all()) and bool((_bits(maxima)[empty] == 0).all()), \
            ('sums or maxima of a workgroup without pixels', what)
        dbeta, e_db, dgamma, e_dg, dz, e_dz = R.handover_ref(z, g, mi[0], mi[1], gamma, rec)
        h = o.hand[br]
        hold('rel dbeta', h.dbeta, dbeta, e_db, what)
        hold('rel dgamma', h.dgamma, dgamma, e_dg, what)
        hold('rel dz', h.dz.view(rows, c), dz, e_dz, what)
        _amax_holds(h.slots, h.dz, (what, 'dz'))
        hold('rel dbeta', h.dbeta_p, dbeta, e_db, (what, 'packed'))
        hold('rel dgamma', h.dgamma_p, dgamma, e_dg, (what, 'packed'))
        words = h.slots_p.cpu().view(64, 32)
        bits = int(words[0, 0])
        assert bool((words[1:, 0] == 0).all()) and bool((words[:, 1:] == 0).all()), ('packed dz: a word beside slot 0', what)
        top = torch.tensor([bits], dtype=torch.int32).view(torch.float32).double().item()
        assert top == top and top < float('inf'), ('packed dz: slot 0', what, hex(bits))
        assert top >= float((dz.abs() - e_dz).max()), ('packed dz: slot 0 below max|dz|', what, top, float(dz.abs().max()))
        s = _op_scale(bits)
        back = Bufs(cuda)
        unpacked = back.out(rows * c)
        _C.call('evk_unpack_f16x2', h.dz_p.data_ptr(), rows * c, h.slots_p.data_ptr(), unpacked.data_ptr(), _stream())
        back.check((what, 'unpack'))
        quant = torch.maximum(2.0 ** -22 * (dz.abs() + e_dz), torch.full_like(dz, 2.0 ** -25 * s))
        hold('rel dz packed', unpacked.view(rows, c), dz, e_dz + quant, what)
    o.b.check((name, 'after the reads'))
    return gc, r


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize('cs', R.CASES, ids=lambda v: str(v))
def test_every_stage_against_fp64_and_twice_the_same_bits(cuda, cs):
    from ever_amd import _C
    lib = _C.load()
    k = R.case(*cs)
    assert k.undecided == 0, ('elements whose ReLU mask the float64 pre-activation does not decide', k.name, k.undecided)
    d = _device(k, cuda)
    o = _pipeline(lib, cuda, k, d)
    _check(lib, cuda, k, o)
    if cs == (3, 4, 16448):
        nblk, ppb = R.ranges(lib.evk_relation_bn_parts(k.n, k.hw), k.n, k.hw)
        assert (nblk, ppb, -(-k.hw // ppb)) == (256, 65, 254)
    first, again = _everything(o), _everything(_pipeline(lib, cuda, k, d))
    for name in first:
        assert torch.equal(first[name], again[name]), (k.name, name, 'differs between two launches')


def test_saturated_sigmoid_gives_exact_gates_and_finite_gradients(cuda):
    """image 1's scene x 250: |dot| passes 90 on many pixels, where e^-dot overflows or vanishes beside 1.  r is exactly 0 or 1
    there and finite everywhere, every gradient is finite (_hold), g_c is exactly 0 where the stored r is 0 or 1, and the
    bounds hold: they collapse to the absolute floor"""
    from ever_amd import _C
    lib = _C.load()
    k = R.case(*R.SATURATED, R.SATURATED_GAIN)
    assert k.undecided == 0
    f = k.fwd
    far = f.dot.abs() > 90
    assert int(far.sum()) >= k.hw // 4 and bool(far[k.hw:].any()) and not bool(far[:k.hw].any())
    o = _pipeline(lib, cuda, k, _device(k, cuda))
    gc, r = _check(lib, cuda, k, o)
    assert bool(torch.isfinite(r).all())
    assert bool((r[far & (f.dot > 0)] == 1).all()) and bool((r[far & (f.dot < 0)] == 0).all()), 'r beyond |dot| = 90'
    gate = (r == 0) | (r == 1)
    assert bool((gc[gate] == 0).all()), 'g_c where the gate is exactly 0 or 1'


def test_forward_walks_five_channel_trips(cuda):
    """C = 1028: lane 0 takes five trips of the channel loop; the forward has no channel limit (the backward refuses)"""
    from ever_amd import _C
    lib = _C.load()
    k = R.case(*R.FORWARD_ONLY)
    assert k.undecided == 0
    o = _forward(lib, cuda, k, _device(k, cuda))
    hold('rel r', o.r, k.fwd.r, k.fwd.e_r, k.name)
    out = o.out.cpu().view(k.rows, k.c)
    hold('rel out', out, k.fwd.out, k.fwd.e_out, k.name)
    assert bool((out[k.planted_f, 0] == 0).all())
    _amax_zeroed_holds(o.slots, o.out, k.name)
    o.b.check((k.name, 'after the reads'))


@pytest.mark.parametrize('cs', R.CASES + [R.FORWARD_ONLY], ids=lambda v: str(v))
def test_out_absmax_may_be_null_and_stays_zero_for_a_zero_output(cuda, cs):
    """out_absmax = NULL gives the same out and r bits; gamma = beta = 0 on the re-encoding branch (scale = shift = 0) gives an
    output of exact zeros and leaves the zeroed slots zero"""
    from ever_amd import _C
    lib = _C.load()
    k = R.case(*cs)
    d = _device(k, cuda)
    with_slots, without = _forward(lib, cuda, k, d), _forward(lib, cuda, k, d, slots='none')
    assert torch.equal(_bits(with_slots.out), _bits(without.out)) and torch.equal(_bits(with_slots.r), _bits(without.r))
    zero = _forward(lib, cuda, k, d, ss_f=torch.zeros_like(d.ss_f))
    assert bool((_bits(zero.out) == 0).all()), 'an output of zeros'
    assert bool((zero.slots.cpu() == 0).all()), 'out_absmax of an output of zeros'
    assert torch.equal(_bits(zero.r), _bits(with_slots.r))
    for o in (with_slots, without, zero):
        o.b.check((k.name, 'after the reads'))


# ------------------------------------------------------------------------------------------------ refusals
def _untouched(b):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(whole[PAD:PAD + n]).all()) for whole, n in b.all)


@pytest.mark.parametrize('how,c,code', [('shape', 452, E_UNSUPPORTED), ('shape', 6, E_UNSUPPORTED), ('workspace', 64, E_WORKSPACE),
                                        ('null_gc', 64, E_INVALID), ('pack_without_maxima', 64, E_INVALID)])
def test_refusals_return_their_code_and_store_nothing(cuda, how, c, code):
    """every one of these returns before any launch"""
    from ever_amd import _C
    lib = _C.load()
    n, hw = 2, 35
    rows = n * hw
    b = Bufs(cuda)
    size = rows * (c + 4)
    zeros, vec = torch.zeros(size, device=cuda), torch.zeros(2 * c + 8, device=cuda)
    dscene, gc, gf, dz, dgamma, dbeta = b.out(n * c + 8), b.out(size), b.out(size), b.out(size), b.out(c + 4), b.out(c + 4)
    nb = lib.evk_relation_bn_parts(n, hw)
    wsb = lib.evk_relation_bn_workspace_bytes(n, hw, c)
    ws = b.out(wsb // 4 + 8)
    coef = b.out(16 * c + 8)
    slots = b.out(lib.evk_absmax_words(), torch.int32)
    st_, z, v = _stream(), zeros.data_ptr(), vec.data_ptr()
    if how == 'pack_without_maxima':
        rc = lib.evk_bn_bwd_from_partials(z, z, v, v, v, ws.data_ptr(), None, nb, dz.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                                          rows, c, PACK_DX, 1, coef.data_ptr(), 16 * c * 4, slots.data_ptr(), st_)
        want = b'bn_bwd_from_partials'
    else:
        rc = lib.evk_relation_bn_bwd(z, z, z, v, v, z, v, v, z, dscene.data_ptr(), None if how == 'null_gc' else gc.data_ptr(),
                                     gf.data_ptr(), n, hw, c, ws.data_ptr(), wsb - 1 if how == 'workspace' else wsb, st_)
        want = f'relation_bn_bwd: C={c}'.encode() if how == 'shape' else b'relation_bn_bwd'
    msg = lib.evk_last_error()
    assert rc == code and want in msg, (how, c, rc, msg)
    b.check((how, c))
    assert _untouched(b), ('a refused call stored something', how, c)


# ------------------------------------------------------------------------------------------------ through the wrapper
def test_wrapper_takes_448_channels_and_leaves_the_records_where_it_declines(cuda):
    """HF.fs_relation_bn takes C = 448 (the backward's limit), forward and backward, with the values of float64 autograd on
    the CPU; it returns None with `_evk_bn_parts` left on both z for C = 452 and for two maps of different shapes.  (The
    convolution kernels leave records only for whole 64-channel tiles: z carries one record formed here, as an epilogue would
    have.)  The yardstick is autograd, not the layers one by one, and every z whose float64 pre-activation lies within 1e-4
    of zero is moved away first: one ReLU mask that rounds the other way moves dbeta of its channel by a whole g and dz of all
    its rows with it (measured with seed 13: the layer-by-layer path 0.135 off in dzc through one element, this one 1e-7)."""
    import torch.nn.functional as F
    from ever_amd.hip import functional as HF
    from ever_amd.module.layers import BatchNorm2d
    gen = torch.Generator().manual_seed(13)
    n, h, w = 2, 5, 7

    def decided(rows, gamma, beta):
        for _ in range(8):
            pre = (rows - rows.mean(0)) * (rows.var(0, unbiased=False) + R.EPS).rsqrt() * gamma + beta
            near = pre.abs() < 1e-4
            if not near.any():
                return rows
            rows = torch.where(near, rows + 0.25, rows)
        raise AssertionError('a ReLU mask is still undecided')

    def with_record(c, wd, bn):
        rows = decided((torch.randn(n * h * wd, c, generator=gen) + 0.3).double(), bn.weight.detach().double().cpu(),
                       bn.bias.detach().double().cpu()).float()
        rd = rows.double()
        record = torch.stack([torch.full((c,), float(n * h * wd), dtype=torch.float64), rd.mean(0),
                              ((rd - rd.mean(0)) ** 2).sum(0)]).float().contiguous().to(cuda)
        z0 = rows.view(n, h, wd, c).permute(0, 3, 1, 2)                  # NCHW over channels-last memory
        z = z0.to(cuda).requires_grad_()
        assert HF.is_nhwc(z)
        z._evk_bn_parts = (record, 1, False)
        return z0, z

    for c, wf, takes in ((448, w, True), (452, w, False), (64, w + 1, False)):
        torch.manual_seed(c)
        bn_c, bn_f = BatchNorm2d(c).to(cuda).train(), BatchNorm2d(c).to(cuda).train()
        for bn in (bn_c, bn_f):
            torch.nn.init.uniform_(bn.weight, 0.5, 1.5)
            torch.nn.init.uniform_(bn.bias, -0.3, 0.3)
        scene0 = torch.randn(n, c, 1, 1, generator=gen) * 0.1
        (zc0, zc), (zf0, zf) = with_record(c, w, bn_c), with_record(c, wf, bn_f)
        pc, pf = zc._evk_bn_parts, zf._evk_bn_parts
        scene = scene0.to(cuda).requires_grad_()
        out = HF.fs_relation_bn(scene, zc, zf, bn_c, bn_f)
        if not takes:
            assert out is None and zc._evk_bn_parts is pc and zf._evk_bn_parts is pf, (c, wf)
            continue
        assert out is not None and out.shape == (n, c, h, w) and not hasattr(zc, '_evk_bn_parts') and not hasattr(zf, '_evk_bn_parts')
        g = torch.randn(n, c, h, w, generator=gen)
        (out * g.to(cuda)).sum().backward()
        torch.cuda.synchronize()
        got = (out.detach(), scene.grad, zc.grad, zf.grad, bn_c.weight.grad, bn_c.bias.grad, bn_f.weight.grad, bn_f.bias.grad)
        s1, zc1, zf1 = (t.double().contiguous().requires_grad_() for t in (scene0, zc0, zf0))
        ps = [p.detach().double().cpu().requires_grad_() for p in (bn_c.weight, bn_c.bias, bn_f.weight, bn_f.bias)]
        ref = (torch.sigmoid((s1 * F.relu(F.batch_norm(zc1, None, None, ps[0], ps[1], True, 0.1, bn_c.eps))).sum(1, keepdim=True)) *
               F.relu(F.batch_norm(zf1, None, None, ps[2], ps[3], True, 0.1, bn_f.eps)))
        (ref * g.double()).sum().backward()
        want = (ref.detach(), s1.grad, zc1.grad, zf1.grad, ps[0].grad, ps[1].grad, ps[2].grad, ps[3].grad)
        for name, a, b_ in zip(('out', 'dscene', 'dzc', 'dzf', 'dgamma_c', 'dbeta_c', 'dgamma_f', 'dbeta_f'), got, want):
            err = float((a.double().cpu() - b_).abs().max() / b_.abs().max())
            assert err < 5e-5, (c, name, err)


# ------------------------------------------------------------------------------------------------ the printout
def test_print_the_worst_ratios():
    if WORST:
        print('\nworst error / bound per quantity:')
        for name, (ratio, what) in sorted(WORST.items()):
            print(f'  {name:16s} {ratio:6.3f}  ({what})')
