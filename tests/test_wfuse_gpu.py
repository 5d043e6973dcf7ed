"""The weighted-fusion kernels (csrc/wfuse.hip) through the C-ABI, against float64 on the CPU from the same fp32 inputs.  Every
output and the workspace is a NaN-filled slice inside a sentinel-guarded allocation (tests/guard_common.py).

Bounds (u = 2^-24), derived, not tuned; w^ is the float64 normalisation of the fp32 raw weights:
  forward   |y - y64| <= 16 u sum_k |w^_k t_k|: the normalised weight carries at most ~4 roundings for fast_normalize (K - 1
            additions, the eps, the division) and ~8 for softmax (the subtraction, expf, K - 1 additions, the division), one
            rounding per product, K - 1 per sum.  The reference's own fp32 expression stays within 0.22 of this bound over
            20 seeds for either norm: a margin the reference's arithmetic keeps, not one fitted to the kernel;
  dterms    shift 0: <= 8 u w^_k |dy| (the weight's roundings and the product's);  shift 1: <= 12 u w^_k sum_block |dy|
            (three more additions inside the block);
  dots      |d_k - d64_k| <= (D + log2(threads) + 4) u sum |dy up(t_k)|, D (products one thread adds serially into a partial)
            and threads from evk_wfuse_plan: one rounding per fma of the run, one per level of the wave / LDS tree, and room
            for the double sum's rounding to fp32 and second order;
  dweights  the dot bounds b_k pushed through the Jacobian, plus 8 u of each Jacobian term's magnitude:
            fast_normalize  [w_j > 0] ((b_j + sum_k w^_k b_k) + 8 u (|d_j| + sum_k w^_k |d_k|)) / (sum r + eps)
            softmax         w^_j ((b_j + sum_k w^_k b_k) + 8 u (|d_j| + sum_k w^_k |d_k|)).
One-hot: with dy zero but for one element the dot is that single product, bit for bit — a dropped tail shows however loose
the sum bound is.  The backward runs twice into fresh buffers: identical bits.  The plan shows no grid cap (the grid is
ceil(items / share) for every shape, tests/test_bifpn_cpu.py), so no shape crosses one."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests.guard_common import guarded, guards_intact

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
EPS = float(np.float32(1e-4))
P, I = ctypes.c_void_p, ctypes.c_int32


def _plan(lib, shape, k):
    out = (I * 8)()
    assert lib.evk_wfuse_plan(*shape, k, out) == 0, lib.evk_last_error()
    return dict(zip(('grid', 'threads', 'depth', 'ws_bytes', 'quad', 'run', 'dots_at'), list(out)[:7]))


def _ragged(lib, odd):
    """the smallest square one-chunk map (N = 1, C = 4) with more than one workgroup and a last workgroup that is not full"""
    for e in range(3 if odd else 2, 400, 2):
        pl = _plan(lib, (1, e, e, 4), 2)
        items = e * e // (4 if pl['quad'] else 1)
        if pl['grid'] > 1 and items % (pl['threads'] * pl['run']):
            return (1, e, e, 4)
    raise AssertionError('no ragged shape below 400 x 400')


# (N, H, W, C) or a plan search, shifts, what it covers
CASES = [
    ((1, 2, 2, 4), (0, 1), 'a shifted term of one pixel'),
    ((2, 3, 5, 12), (0, 0), 'shift 0 only: odd map, C/4 odd'),
    ((3, 6, 10, 20), (0, 1), 'shifts (0, 1)'),
    ((2, 8, 8, 8), (0, 0, 1), 'shifts (0, 0, 1)'),
    ((2, 4, 4, 4), (0, 1, 0, 1), 'four terms'),
    ('quad', (0, 1), 'plan: quads, a ragged last workgroup'),
    ('elem', (0, 0, 0), 'plan: elements, a ragged last workgroup'),
]
WEIGHTS = {
    'positive': lambda k: [0.7, 1.6, 0.4, 1.1][:k],
    'one negative': lambda k: [0.7, -0.8, 0.4, 1.1][:k],
    'one zero': lambda k: [0.0, 1.6, 0.4, 1.1][:k],
    'all negative': lambda k: [-0.7, -1.6, -0.4, -1.1][:k],
}


class Bufs:
    """device outputs of one call: NaN-filled, each inside its own sentinel-guarded allocation"""

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


def _up(t, s):
    return t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) if s else t


def _pool(t):
    n, h, w, c = t.shape
    return t.reshape(n, h // 2, 2, w // 2, 2, c).sum(dim=(2, 4))


def _normalise64(w, norm):
    w = w.double()
    if norm == 0:
        r = w.clamp_min(0)
        s = r.sum() + EPS
        return r / s, s
    e = torch.exp(w - w.max())
    return e / e.sum(), None


def _shape(lib, shape):
    return _ragged(lib, shape == 'elem') if isinstance(shape, str) else shape


def _arrays(ptrs):
    return (P * len(ptrs))(*ptrs)


def _forward(lib, dts, shifts, dw, norm, shape, dev, what):
    bufs = Bufs(dev)
    n, h, w, c = shape
    y = bufs.out(n * h * w * c)
    rc = lib.evk_wfuse_fwd(_arrays([t.data_ptr() for t in dts]), (I * len(shifts))(*shifts), len(shifts),
                           None if dw is None else dw.data_ptr(), norm, EPS, y.data_ptr(), n, h, w, c,
                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.evk_last_error()
    bufs.check(what)
    return y.cpu().reshape(n, h, w, c)


def _backward(lib, ddy, dts, shifts, dw, norm, shape, dev, what, want_w=True):
    """(dterms, dweights, workspace) on the host, from fresh guarded buffers"""
    bufs = Bufs(dev)
    n, h, w, c = shape
    k = len(shifts)
    pl = _plan(lib, shape, k)
    outs = [bufs.out(n * (h >> s) * (w >> s) * c) for s in shifts]
    gw = bufs.out(k) if want_w else None
    ws = bufs.out(pl['ws_bytes'] // 4) if want_w else None
    rc = lib.evk_wfuse_bwd(ddy.data_ptr(), _arrays([t.data_ptr() for t in dts]), (I * k)(*shifts), k,
                           None if dw is None else dw.data_ptr(), norm, EPS, _arrays([o.data_ptr() for o in outs]),
                           None if gw is None else gw.data_ptr(), None if ws is None else ws.data_ptr(),
                           pl['ws_bytes'] if want_w else 0, n, h, w, c, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.evk_last_error()
    bufs.check(what)
    return ([o.cpu().reshape(n, h >> s, w >> s, c) for o, s in zip(outs, shifts)], None if gw is None else gw.cpu(),
            None if ws is None else ws.cpu(), pl)


def _inputs(shape, shifts, seed):
    n, h, w, c = shape
    g = torch.Generator().manual_seed(seed)
    ts = [torch.randn((n, h >> s, w >> s, c), generator=g) for s in shifts]
    dy = torch.randn((n, h, w, c), generator=g)
    return ts, dy


@pytest.mark.parametrize('norm', [0, 1], ids=['fast_normalize', 'softmax'])
@pytest.mark.parametrize('shape,shifts,what', CASES, ids=[c[2] for c in CASES])
def test_wfuse_forward_and_backward(cuda, shape, shifts, what, norm):
    from ever_amd import _C
    lib = _C.load()
    shape = _shape(lib, shape)
    n, h, w, c = shape
    k = len(shifts)
    ts, dy = _inputs(shape, shifts, 1 + [cse[2] for cse in CASES].index(what))
    dts, ddy = [t.to(cuda) for t in ts], dy.to(cuda)
    t64 = [_up(t.double(), s) for t, s in zip(ts, shifts)]
    dy64 = dy.double()
    for wname, wfn in WEIGHTS.items():
        tag = f'{what} / {("fast_normalize", "softmax")[norm]} / {wname}'
        wraw = torch.tensor(wfn(k), dtype=torch.float32)
        dwt = wraw.to(cuda)
        wh, s64 = _normalise64(wraw, norm)
        dead = norm == 0 and wname == 'all negative'
        # ---- forward
        y = _forward(lib, dts, shifts, dwt, norm, shape, cuda, tag)
        assert torch.isfinite(y).all(), ('y holds an element nobody wrote', tag)
        y64 = sum(wh[i] * t64[i] for i in range(k))
        fb = 16 * U * sum((wh[i] * t64[i]).abs() for i in range(k))
        ferr = (y.double() - y64).abs()
        print(f'{tag:72s} forward error / bound {float((ferr / fb.clamp_min(1e-300)).max()):.3f}')
        assert bool((ferr <= fb).all()), ('forward', tag)
        if dead:
            assert bool((y == 0).all()), ('all weights negative: y is exactly 0', tag)
        # ---- backward, twice
        (g1, gw1, ws1, pl), (g2, gw2, ws2, _) = (_backward(lib, ddy, dts, shifts, dwt, norm, shape, cuda, tag) for _ in range(2))
        for a, b in zip(g1 + [gw1, ws1], g2 + [gw2, ws2]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), ('two runs differ', tag)
        for i, s in enumerate(shifts):
            assert torch.isfinite(g1[i]).all(), ('a gradient holds an element nobody wrote', tag, i)
            if s == 0:
                want, bound = wh[i] * dy64, 8 * U * wh[i] * dy64.abs()
            else:
                want, bound = wh[i] * _pool(dy64), 12 * U * wh[i] * _pool(dy64.abs())
            err = (g1[i].double() - want).abs()
            print(f'{tag:72s} dterm {i} (shift {s}) error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}')
            assert bool((err <= bound).all()), ('dterm', i, tag)
            if dead:
                assert bool((g1[i] == 0).all())
        # ---- the dots (behind the records in the workspace), then the weight gradient
        assert torch.isfinite(ws1).all(), ('the workspace holds a word nobody wrote', tag)
        dots = ws1[pl['dots_at']:pl['dots_at'] + k].double()
        d64 = torch.stack([(dy64 * t64[i]).sum() for i in range(k)])
        mag = torch.stack([(dy64 * t64[i]).abs().sum() for i in range(k)])
        b = (pl['depth'] + math.log2(pl['threads']) + 4) * U * mag
        print(f'{tag:72s} dots error / bound {float(((dots - d64).abs() / b).max()):.3f}')
        assert bool(((dots - d64).abs() <= b).all()), ('dots', tag, dots, d64)
        m64, bm, am = (wh * d64).sum(), (wh * b).sum(), (wh * d64.abs()).sum()
        if norm == 0:
            gate = (wraw > 0).double()
            want = gate * (d64 - m64) / s64
            bound = gate * ((b + bm) + 8 * U * (d64.abs() + am)) / s64
        else:
            want = wh * (d64 - m64)
            bound = wh * ((b + bm) + 8 * U * (d64.abs() + am))
        assert torch.isfinite(gw1).all()
        werr = (gw1.double() - want).abs()
        print(f'{tag:72s} dweights error / bound {float((werr / bound.clamp_min(1e-300)).max()):.3f}')
        assert bool((werr <= bound).all()), ('dweights', tag, gw1, want)
        if dead:
            assert bool((gw1 == 0).all())
        # ---- asking for less gives the same bits: the term gradients without the weight gradient
        only, _, _, _ = _backward(lib, ddy, dts, shifts, dwt, norm, shape, cuda, tag, want_w=False)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(only, g1))


def test_wfuse_unit_weight_one_term_is_nearest_x2(cuda):
    """weights == NULL, one term with shift 1: plain nearest x2 forward (every bit), the 2 x 2 block sum backward"""
    from ever_amd import _C
    lib = _C.load()
    for shape in ((1, 2, 2, 4), (2, 6, 10, 12)):
        (t,), dy = _inputs(shape, (1,), 21)
        dt, ddy = t.to(cuda), dy.to(cuda)
        y = _forward(lib, [dt], (1,), None, 0, shape, cuda, 'unit')
        assert torch.equal(y.view(torch.int32), _up(t, 1).view(torch.int32))
        (g,), _, _, _ = _backward(lib, ddy, [dt], (1,), None, 0, shape, cuda, 'unit', want_w=False)
        n, h, w, c = shape
        d = dy.reshape(n, h // 2, 2, w // 2, 2, c)
        want = (d[:, :, 0, :, 0] + d[:, :, 0, :, 1]) + (d[:, :, 1, :, 0] + d[:, :, 1, :, 1])     # the kernel's order, in fp32
        assert torch.equal(g.view(torch.int32), want.view(torch.int32))


def _item_first_float(i, shape, quad):
    """float offset of the first element item i of the backward owns (csrc/wfuse.hip: wfuse_bwd_kernel)"""
    n, h, w, c = shape
    c4 = c // 4
    if not quad:
        return i * 4
    q, cb = divmod(i, c4)
    r, qx = divmod(q, w // 2)
    return ((r * 2 * w + 2 * qx) * c4 + cb) * 4


@pytest.mark.parametrize('shape,shifts', [((3, 6, 10, 20), (0, 1)), ('quad', (0, 1)), ('elem', (0, 0))],
                         ids=['one workgroup', 'quads, ragged', 'elements, ragged'])
def test_wfuse_dot_of_a_one_hot_gradient_is_the_single_product(cuda, shape, shifts):
    from ever_amd import _C
    lib = _C.load()
    shape = _shape(lib, shape)
    n, h, w, c = shape
    k = len(shifts)
    ts, _ = _inputs(shape, shifts, 31)
    dts = [t.to(cuda) for t in ts]
    ups = [_up(t, s).reshape(-1) for t, s in zip(ts, shifts)]
    pl = _plan(lib, shape, k)
    numel = n * h * w * c
    items = numel // 4 // (4 if pl['quad'] else 1)
    share = pl['threads'] * pl['run']
    assert pl['grid'] == -(-items // share)
    last_wg_first = _item_first_float((pl['grid'] - 1) * share, shape, pl['quad'])
    first_wg_last = _item_first_float(min(share, items) - 1, shape, pl['quad']) + 3
    plants = {'first': 0, 'last (the last workgroup\'s last position)': numel - 1, 'first of the last workgroup': last_wg_first,
              'last item of the first workgroup': first_wg_last}
    wraw = torch.tensor([0.7, 1.6, 0.4][:k]).to(cuda)
    for name, pos in plants.items():
        dy = torch.zeros(numel)
        dy[pos] = 1.37
        _, gw, ws, _ = _backward(lib, dy.to(cuda), dts, shifts, wraw, 0, shape, cuda, name)
        dots = ws[pl['dots_at']:pl['dots_at'] + k]
        want = torch.stack([dy[pos] * u[pos] for u in ups])          # one fp32 product each
        assert torch.equal(dots.view(torch.int32), want.view(torch.int32)), (name, pos, dots, want)
        assert torch.isfinite(gw).all()
