"""The depthwise kernels and the 1x1-map broadcast / sum through the C-ABI, against float64 on the CPU from the same fp32 inputs,
over the case table of tests/depthwise_common.py (every forward and backward form, every lane plan, ragged strip groups, idle
lanes, 72 tiles, asymmetric strides / dilations / paddings, outputs larger than the input).  y, dx, dw, db and the workspace
slab — held at exactly evk_depthwise_bwd_workspace_bytes — are NaN-filled slices inside sentinel-guarded allocations
(tests/guard_common.py); the guards are checked after every launch and every output must be finite.

Exact inputs (the whole table): integers in [-4, 4], every partial sum below 2^24 (depthwise_common.reference states and
asserts the condition), so fp32 FMA in any order is exact and y, dx, dw, db must equal the fp64 reference bit for bit.  Many
pre-activations are exactly 0 there: the fused ReLU's backward must drop them, as torch does.

Unit-normal inputs (one case per lane plan and the 72-tile case), u = 2^-24, derived, not tuned (depthwise_common.reference):
  y, dx    (T + 2) u (sum |x w| + |b|), T taps;
  dw, db   (d + 2) u sum |g x|, d = 16 + (ps - 1) + ceil(tiles / 64) + 63 from evk_depthwise_plan.
An element whose fp64 pre-activation lies inside the forward bound has no certain ReLU mask: it gets dy = 0, and each case
asserts that these are at most 0.1 % of its elements."""
import ctypes

import pytest
import torch

from tests import depthwise_common as DC
from tests.guard_common import guarded, guards_intact

pytestmark = pytest.mark.gpu
U = DC.U


class Bufs:
    """device outputs of one launch: NaN-filled, each inside its own sentinel-guarded allocation"""

    def __init__(self, dev):
        self.dev, self.all = dev, []

    def out(self, n):
        whole, inner = guarded(n, self.dev)
        self.all.append((whole, n))
        return inner

    def check(self, what):
        torch.cuda.synchronize()
        for whole, n in self.all:
            assert guards_intact(whole, n), ('a store beside a buffer', what)


def _lib():
    from ever_amd import _C
    return _C.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nhwc(t, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(dev)


def _nchw(flat, n, c, h, w):
    return flat.cpu().reshape(n, h, w, c).permute(0, 3, 1, 2)


class Device:
    """one case's inputs on the device and its launches"""

    def __init__(self, dev, case, ref):
        self.dev, self.case, self.lib, self.d = dev, case, _lib(), DC.desc(case)
        self.x, self.g = _nhwc(ref['x'], dev), _nhwc(ref['g'], dev)
        self.w = ref['w'].reshape(case['c'], -1).contiguous().to(dev)
        self.b = ref['b'].to(dev) if ref['b'] is not None else None
        self.ws_floats = self.lib.evk_depthwise_bwd_workspace_bytes(ctypes.byref(self.d)) // 4
        self.y = None

    def forward(self):
        c = self.case
        ho, wo = DC.out_size(c)
        bufs = Bufs(self.dev)
        y = bufs.out(c['n'] * ho * wo * c['c'])
        rc = self.lib.evk_depthwise_fwd(ctypes.byref(self.d), self.x.data_ptr(), self.w.data_ptr(),
                                        self.b.data_ptr() if self.b is not None else None, y.data_ptr(), 1 if c['relu'] else 0,
                                        _stream())
        assert rc == 0, self.lib.evk_last_error()
        bufs.check((c['name'], 'forward'))
        self.y = y
        return _nchw(y, c['n'], c['c'], ho, wo)

    def backward(self, dx=True, dw=True, db=True, with_x=True):
        """{name: tensor on the CPU} of the outputs asked for; the slab under 'slab' when dw or db is"""
        c = self.case
        bufs = Bufs(self.dev)
        o = {}
        if dx:
            o['dx'] = bufs.out(self.x.numel())
        if dw:
            o['dw'] = bufs.out(self.w.numel())
        if db:
            o['db'] = bufs.out(c['c'])
        if dw or db:
            o['slab'] = bufs.out(self.ws_floats)
        ptr = lambda k: o[k].data_ptr() if k in o else None      # noqa: E731
        rc = self.lib.evk_depthwise_bwd(ctypes.byref(self.d), self.g.data_ptr(), self.x.data_ptr() if with_x else None,
                                        self.y.data_ptr() if c['relu'] else None, self.w.data_ptr(), ptr('dx'), ptr('dw'), ptr('db'),
                                        ptr('slab'), self.ws_floats * 4 if 'slab' in o else 0, _stream())
        assert rc == 0, self.lib.evk_last_error()
        bufs.check((c['name'], 'backward', dx, dw, db))
        out = {k: v.cpu() for k, v in o.items()}
        for k, v in out.items():
            assert bool(torch.isfinite(v).all()), (c['name'], k, 'holds an element nobody wrote')
        if 'dx' in out:
            out['dx'] = _nchw(out['dx'], c['n'], c['c'], c['h'], c['w'])
        if 'dw' in out:
            out['dw'] = out['dw'].reshape(c['c'], 1, *c['k'])
        return out


@pytest.mark.parametrize('case', DC.CASES, ids=[c['name'] for c in DC.CASES])
def test_exact_inputs_equal_fp64_bit_for_bit(cuda, case):
    ref = DC.reference(case, 'exact')
    dev = Device(cuda, case, ref)
    y = dev.forward()
    assert bool(torch.isfinite(y).all()), 'y holds an element nobody wrote'
    assert torch.equal(y.double(), ref['y']), ('y', int((y.double() != ref['y']).sum()))
    got = dev.backward()
    for k in ('dx', 'dw', 'db'):
        assert got[k].shape == ref[k].shape
        assert torch.equal(got[k].double(), ref[k]), (case['name'], k, int((got[k].double() != ref[k]).sum()), 'elements differ')
    if case['relu']:      # the zeros the ReLU backward has to drop are there (integer data)
        zeros = ref['pre'] == 0
        assert not bool(ref['uncertain'].any())
        assert bool(zeros.any()) and bool((ref['g'][zeros] != 0).any())


@pytest.mark.parametrize('name', DC.NORMAL_CASES)
def test_unit_normal_inputs_within_the_derived_bounds(cuda, name):
    case = DC.BY_NAME[name]
    ref = DC.reference(case, 'normal')
    p = DC.plan(_lib(), case)
    nunc = int(ref['uncertain'].sum())
    assert nunc <= 1e-3 * ref['pre'].numel(), ('elements without a certain mask', nunc)
    dev = Device(cuda, case, ref)
    y = dev.forward()
    assert bool(torch.isfinite(y).all()), 'y holds an element nobody wrote'
    got = dev.backward()
    got['y'] = y
    t, d = ref['taps'], DC.depth(p)
    bounds = {'y': (t + 2) * U * ref['ymag'], 'dx': (t + 2) * U * ref['dxmag'], 'dw': (d + 2) * U * ref['dwmag'],
              'db': (d + 2) * U * ref['dbmag']}
    line = []
    for k, bound in bounds.items():
        err = (got[k].double() - ref[k]).abs()
        line.append(f'{k} {float((err / bound.clamp_min(1e-300)).max()):.3f}')
        assert bool((err <= bound).all()), (name, k, line[-1], int((err > bound).sum()), 'elements outside the bound')
    print(f"{name:14s} cl {p['cl']:2d} tiles {p['tiles']:3d} depth {d:3d}  error / bound: {', '.join(line)}; uncertain {nunc} of "
          f"{ref['pre'].numel()}")
    if case['relu']:      # the mask the backward used is the forward's own output: certain elements agree with fp64
        assert torch.equal((y > 0) & ~ref['uncertain'], (ref['pre'] > 0) & ~ref['uncertain'])


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize('name', DC.PARTIAL_CASES)
def test_partial_requests_write_the_same_bits_and_nothing_else(cuda, name):
    """dx alone (no workspace, no x), dw alone, db alone, dw + db without dx: what is not asked for has no buffer at all, and
    every buffer there is sits between guards"""
    case = DC.BY_NAME[name]
    dev = Device(cuda, case, DC.reference(case, 'normal'))
    dev.forward()
    full = dev.backward()
    only = dev.backward(dx=True, dw=False, db=False, with_x=False)
    assert set(only) == {'dx'} and _same_bits(only['dx'], full['dx'])
    only = dev.backward(dx=False, dw=True, db=False)
    assert set(only) == {'dw', 'slab'} and _same_bits(only['dw'], full['dw']) and _same_bits(only['slab'], full['slab'])
    only = dev.backward(dx=False, dw=False, db=True)
    assert set(only) == {'db', 'slab'} and _same_bits(only['db'], full['db']) and _same_bits(only['slab'], full['slab'])
    only = dev.backward(dx=False, dw=True, db=True)
    assert _same_bits(only['dw'], full['dw']) and _same_bits(only['db'], full['db'])
    # nothing asked for: no launch, no error
    assert dev.lib.evk_depthwise_bwd(ctypes.byref(dev.d), dev.g.data_ptr(), None, None, dev.w.data_ptr(), None, None, None, None, 0,
                                     _stream()) == 0


def test_two_runs_of_the_72_tile_case_give_the_same_bits(cuda):
    case = DC.BY_NAME['t72']
    dev = Device(cuda, case, DC.reference(case, 'normal'))
    dev.forward()
    a, b = dev.backward(), dev.backward()
    assert set(a) == {'dx', 'dw', 'db', 'slab'}
    for k in a:
        assert _same_bits(a[k], b[k]), k


# ---- evk_broadcast_hw / evk_sum_hw ----------------------------------------------------------------------------------------
def _rl(c):
    return 256 // min(c // 4, 8)        # pixel slices per channel group of sum_hw (tpc = min(C / 4, 8) channel groups)


@pytest.mark.parametrize('c', (4, 12, 20, 24, 28, 32, 36, 304))
def test_broadcast_and_sum_are_exact_on_integers(cuda, c):
    """rl = 256, 85, 51, 42, 36, 32: threads past rl * tpc idle for C / 4 = 3, 5, 6, 7; C = 36 and 304 have a ragged last
    channel block and several blocks; HW below, at and above rl, and many trips"""
    lib, st = _lib(), _stream()
    rl = _rl(c)
    assert rl == {4: 256, 12: 85, 20: 51, 24: 42, 28: 36, 32: 32, 36: 32, 304: 32}[c]
    gen = torch.Generator().manual_seed(c)
    for n in (1, 3):
        for hw in sorted({1, rl - 1, rl, rl + 1, 1000}):
            src = torch.randint(-4, 5, (n, c), generator=gen).float()
            bufs = Bufs(cuda)
            dst = bufs.out(n * hw * c)
            assert lib.evk_broadcast_hw(src.to(cuda).data_ptr(), dst.data_ptr(), n, hw, c, st) == 0, lib.evk_last_error()
            bufs.check(('broadcast_hw', n, hw, c))
            assert torch.equal(dst.cpu().reshape(n, hw, c), src[:, None, :].expand(n, hw, c)), ('broadcast_hw', n, hw, c)
            x = torch.randint(-4, 5, (n, hw, c), generator=gen).float()
            total = bufs.out(n * c)
            assert lib.evk_sum_hw(x.to(cuda).data_ptr(), total.data_ptr(), n, hw, c, st) == 0, lib.evk_last_error()
            bufs.check(('sum_hw', n, hw, c))
            t = total.cpu().reshape(n, c)
            assert bool(torch.isfinite(t).all()), ('sum_hw holds an element nobody wrote', n, hw, c)
            assert torch.equal(t.double(), x.double().sum(1)), ('sum_hw', n, hw, c)       # |sum| <= 4000 < 2^24: exact


def test_sum_hw_unit_normal_within_the_depth_bound(cuda):
    """a thread adds ceil(HW / rl) pixels, then rl slices are added in order: at most ceil(HW / rl) + rl roundings, each
    relative to a partial sum of magnitude <= sum |x|"""
    lib, n, hw, c = _lib(), 3, 1000, 36
    rl = _rl(c)
    x = torch.randn((n, hw, c), generator=torch.Generator().manual_seed(9))
    bufs = Bufs(cuda)
    total = bufs.out(n * c)
    assert lib.evk_sum_hw(x.to(cuda).data_ptr(), total.data_ptr(), n, hw, c, _stream()) == 0, lib.evk_last_error()
    bufs.check('sum_hw')
    bound = (-(-hw // rl) + rl) * U * x.double().abs().sum(1)
    err = (total.cpu().reshape(n, c).double() - x.double().sum(1)).abs()
    print(f'sum_hw {n} x {hw} x {c}: error / bound {float((err / bound).max()):.3f}')
    assert bool((err <= bound).all())


def test_broadcast_past_the_workgroup_cap(cuda):
    """C = 4, HW = 2^24 + 3: 65537 workgroups' worth of 16-byte elements on a grid capped at 65536, so the grid-stride loop
    wraps (268 MB written); compared on the device"""
    lib, c, hw = _lib(), 4, 2 ** 24 + 3
    assert -(-hw * (c // 4) // 256) > 65536
    src = torch.tensor([[1.5, -2.0, 3.25, 4.0]], device=cuda)
    bufs = Bufs(cuda)
    dst = bufs.out(hw * c)
    assert lib.evk_broadcast_hw(src.data_ptr(), dst.data_ptr(), 1, hw, c, _stream()) == 0, lib.evk_last_error()
    bufs.check('broadcast_hw past the cap')
    assert torch.equal(dst.view(hw, c), src.expand(hw, c))
