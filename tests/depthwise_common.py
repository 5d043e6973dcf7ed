"""The depthwise kernels (csrc/depthwise.hip) at the edges of their forms and of the backward tiling: the case table, the form
and plan facts each case exists for, and the sets the table has to reach.  No torch.cuda here: tests/test_depthwise_plan_cpu.py
walks the table through evk_depthwise_plan on the host, tests/test_depthwise_edges_gpu.py launches it.

Forms: forward <KW, SW, D1> (28), backward <KW, S1D1> (14).  Backward tiling: cl channel lanes (of 4 channels) x ps = 256 / cl
strips of 4 pixels per workgroup, over 4 rows; strips and rows are counted over max(W, Wo) and max(H, Ho)."""
import ctypes

KTW, KTB, KTH = 8, 4, 4          # forward strip, backward strip, backward rows per tile
PLAN_FIELDS = ('fkw', 'fsw', 'fd1', 'fstrips', 'fblocks', 'bkw', 'bs1d1', 'cl', 'ps', 'bstrips', 'strip_groups', 'row_tiles',
               'cblocks', 'tiles')


def _c(name, n, h, w, c, k, s=(1, 1), p=(0, 0), dil=(1, 1), bias=False, relu=False, facts=()):
    (kh, kw), (sh, sw), (dh, dw) = k, s, dil
    return dict(name=name, n=n, h=h, w=w, c=c, k=k, s=s, p=p, dil=dil, bias=bias, relu=relu,
                fwd=(kw, sw, int(dw == 1)), bwd=(kw, int(sw == 1 and dw == 1)), facts=frozenset(facts))


# name, N, H, W, C, (kh, kw), stride, padding, dilation; `facts`: what the case is in the table for, each one asserted by
# test_depthwise_plan_cpu.py (FACT_CHECKS below).  The channel count decides cl: 4 -> 1, 8 -> 2, 12 / 16 -> 4, 32 -> 8,
# 36 .. 64 -> 16, 132 -> 16 (3 blocks, 15 idle lanes), 96 -> 32, 196 -> 64 (15 idle lanes), 256 -> 64.
CASES = [
    # ---- KW = 1
    _c('k1x1', 3, 5, 9, 4, (1, 1), facts=('cl1', 'wo9', 'fwd_tail')),
    _c('k3x1-s12', 2, 9, 16, 8, (3, 1), s=(1, 2), p=(1, 0), bias=True, facts=('cl2', 'stride_1_2', 'wo8', 's2_even_w')),
    _c('k7x1-ho1', 2, 7, 11, 12, (7, 1), dil=(1, 2), relu=True, facts=('cl4', 'ho1')),
    _c('k1x1-s2-d2', 1, 9, 13, 32, (1, 1), s=(2, 2), dil=(2, 2), bias=True, facts=('cl8', 's2_odd_w')),
    # ---- KW = 2
    _c('k2x2', 2, 10, 10, 16, (2, 2), bias=True, relu=True, facts=('cl4', 'wo9', 'even_kernel')),
    _c('k2x2-s2', 1, 12, 15, 40, (2, 2), s=(2, 2), p=(1, 1), facts=('cl16', 'wo8', 's2_odd_w', 'even_kernel')),
    _c('k5x2-d13', 1, 12, 14, 8, (5, 2), p=(0, 2), dil=(1, 3), bias=True, facts=('cl2', 'dil_1_3', 'pad_0_2', 'ph_ne_pw')),
    _c('k2x2-s2-d2', 3, 9, 8, 96, (2, 2), s=(2, 2), dil=(2, 2), relu=True, facts=('cl32', 's2_even_w')),
    # ---- KW = 3
    _c('k3x3-same+2', 2, 6, 5, 196, (3, 3), p=(3, 3), bias=True, relu=True,
       facts=('cl64', 'idle64', 'wo_gt_w_s1', 'bias_only_border', 'wo9', 'ragged_group')),
    _c('k3x3-s2-same+2', 3, 3, 3, 12, (3, 3), s=(2, 2), p=(3, 3), bias=True, facts=('cl4', 'wo_gt_w_s2', 'bias_only_border')),
    _c('k3x3-d6', 1, 5, 9, 132, (3, 3), p=(6, 6), dil=(6, 6), bias=True,
       facts=('cl16', 'idle16', 'dil_6_6', 'taps_in_padding', 'wo9')),
    _c('k3x3-s2-d12', 2, 11, 12, 32, (3, 3), s=(2, 2), p=(1, 2), dil=(1, 2), facts=('cl8', 'ph_ne_pw', 's2_even_w')),
    # ---- KW = 4
    _c('k4x4', 1, 9, 11, 256, (4, 4), p=(1, 2), bias=True, facts=('cl64', 'ph_ne_pw', 'even_kernel')),
    _c('k4x4-s2', 2, 13, 16, 4, (4, 4), s=(2, 2), p=(1, 1), relu=True, facts=('cl1', 'wo8', 's2_even_w', 'even_kernel')),
    _c('k4x4-d2', 1, 12, 13, 64, (4, 4), p=(3, 3), dil=(2, 2), bias=True, facts=('cl16',)),
    _c('k4x4-s12-d12', 1, 8, 21, 16, (4, 4), s=(1, 2), p=(2, 3), dil=(1, 2), facts=('cl4', 'stride_1_2', 's2_odd_w')),
    # ---- KW = 5
    _c('k2x5-d21', 2, 9, 12, 96, (2, 5), p=(3, 0), dil=(2, 1), bias=True, relu=True,
       facts=('cl32', 'dil_2_1', 'pad_3_0', 'wo8', 'ho_gt_h')),
    _c('k5x5-s2', 1, 11, 17, 8, (5, 5), s=(2, 2), p=(2, 2), bias=True, facts=('cl2', 'wo9', 's2_odd_w')),
    _c('k5x5-s21-d13', 2, 12, 16, 32, (5, 5), s=(2, 1), p=(2, 6), dil=(1, 3), relu=True, facts=('cl8', 'stride_2_1', 'dil_1_3')),
    _c('k5x5-s2-d2', 1, 17, 18, 12, (5, 5), s=(2, 2), p=(4, 4), dil=(2, 2), facts=('cl4', 'wo9', 's2_even_w')),
    # ---- KW = 6
    _c('k6x6', 1, 8, 13, 32, (6, 6), p=(2, 2), facts=('cl8', 'even_kernel')),
    _c('k6x6-s2', 2, 14, 16, 16, (6, 6), s=(2, 2), p=(2, 2), bias=True, facts=('cl4', 'wo8', 'even_kernel')),
    _c('k6x6-d12', 2, 9, 20, 8, (6, 6), p=(1, 0), dil=(1, 2), bias=True, relu=True, facts=('cl2', 'ph_ne_pw', 'even_kernel')),
    _c('k6x6-s2-d2', 1, 15, 17, 4, (6, 6), s=(2, 2), p=(3, 3), dil=(2, 2), bias=True, facts=('cl1', 's2_odd_w')),
    # ---- KW = 7
    _c('k1x7-wo1', 3, 6, 7, 16, (1, 7), bias=True, facts=('cl4', 'wo1')),
    _c('k7x7-s2', 1, 13, 15, 4, (7, 7), s=(2, 2), p=(3, 3), relu=True, facts=('cl1', 'wo8', 's2_odd_w')),
    _c('k7x7-s21-d12', 1, 14, 15, 8, (7, 7), s=(2, 1), p=(3, 6), dil=(1, 2), bias=True, facts=('cl2', 'stride_2_1', 'ph_ne_pw')),
    _c('k7x7-s2-d2', 1, 16, 14, 36, (7, 7), s=(2, 2), p=(6, 6), dil=(2, 2), facts=('cl16', 's2_even_w')),
    # ---- the backward tiling at cl = 64, ps = 4
    # N = 3, 30 x 37, C = 196: 10 strips in 3 groups (the last holds 2, its last strip one pixel), 8 row tiles: 72 tiles, so
    # the reduction's slices 0 .. 7 take two tiles and the others one; 15 idle channel lanes
    _c('t72', 3, 30, 37, 196, (3, 3), p=(1, 1), bias=True, relu=True,
       facts=('cl64', 'idle64', 'ragged_group', 'multi_group', 'tiles_65_127')),
    # the decoder's 256-channel separable convolution at a width with two full strip groups and a ragged third
    _c('c256-w35', 1, 5, 35, 256, (3, 3), p=(1, 1), facts=('cl64', 'ragged_group', 'multi_group')),
    # 7x1 with vertical padding only: the third kernel of the issue's list that has KW = 1 with every tap live
    _c('k7x1', 1, 12, 10, 16, (7, 1), p=(3, 0), bias=True, facts=('cl4', 'pad_3_0')),
]
BY_NAME = {c['name']: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# unit-normal inputs with the derived bounds: one case per cl and the 72-tile case
NORMAL_CASES = ('k1x1', 'k5x2-d13', 'k2x2', 'k3x3-s2-d12', 'k3x3-d6', 'k2x5-d21', 'k4x4', 't72')
# partial requests (dx only, dw only, db only, dw + db)
PARTIAL_CASES = ('k2x5-d21', 'k5x5-s21-d13')

REQUIRED_FWD = {(kw, sw, d1) for kw in range(1, 8) for sw in (1, 2) for d1 in (0, 1)}
REQUIRED_BWD = {(kw, s1d1) for kw in range(1, 8) for s1d1 in (0, 1)}
REQUIRED_CL = {1, 2, 4, 8, 16, 32, 64}
REQUIRED_KERNELS = {(1, 1), (3, 1), (1, 7), (7, 1), (2, 2), (4, 4), (6, 6), (2, 5), (5, 2)}
REQUIRED_FACTS = {
    'idle16', 'idle64', 'ragged_group', 'multi_group', 'tiles_65_127', 'fwd_tail', 'wo1', 'wo8', 'wo9',
    'stride_1_2', 'stride_2_1', 'dil_2_1', 'dil_1_3', 'dil_6_6', 'taps_in_padding', 'pad_0_2', 'pad_3_0', 'ph_ne_pw',
    'wo_gt_w_s1', 'wo_gt_w_s2', 'ho_gt_h', 'bias_only_border', 'ho1', 's2_even_w', 's2_odd_w', 'even_kernel',
} | {f'cl{v}' for v in REQUIRED_CL}
assert len(REQUIRED_FWD) == 28 and len(REQUIRED_BWD) == 14


def out_size(case):
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = case['k'], case['s'], case['p'], case['dil']
    return (case['h'] + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (case['w'] + 2 * pw - dw * (kw - 1) - 1) // sw + 1


def desc(case):
    from ever_amd import _C
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = case['k'], case['s'], case['p'], case['dil']
    ho, wo = out_size(case)
    return _C.ConvDesc(case['n'], case['h'], case['w'], case['c'], ho, wo, case['c'], kh, kw, sh, sw, ph, pw, dh, dw)


def plan_of_desc(lib, d):
    """(return code, the 14 plan words as a dict; every word is -7 when the query refused)"""
    out = (ctypes.c_int32 * len(PLAN_FIELDS))(*([-7] * len(PLAN_FIELDS)))
    rc = lib.evk_depthwise_plan(ctypes.byref(d), out)
    return rc, dict(zip(PLAN_FIELDS, out))


def plan(lib, case):
    rc, p = plan_of_desc(lib, desc(case))
    assert rc == 0, (case['name'], lib.evk_last_error())
    return p


def _only_padding(case):
    """does some output see padding only (every tap outside the map)?  Along one axis: the first output's window ends before 0."""
    (kh, kw), (ph, pw), (dh, dw) = case['k'], case['p'], case['dil']
    return ph >= dh * (kh - 1) + 1 or pw >= dw * (kw - 1) + 1


def _dead_tap(case):
    """a tap that lies in the padding for every output (a zero weight gradient): along one axis, the first tap is outside
    the map even for the last output, or the last tap even for the first"""
    ho, wo = out_size(case)
    for size, o, k, s, p, dl in ((case['h'], ho, case['k'][0], case['s'][0], case['p'][0], case['dil'][0]),
                                 (case['w'], wo, case['k'][1], case['s'][1], case['p'][1], case['dil'][1])):
        if (o - 1) * s - p < 0 or -p + (k - 1) * dl >= size:
            return True
    return False


# fact -> predicate(case, plan words, (Ho, Wo))
FACT_CHECKS = {
    'idle16': lambda c, p, o: p['cl'] == 16 and p['cblocks'] > 1 and p['cblocks'] * 16 > c['c'] // 4,
    'idle64': lambda c, p, o: p['cl'] == 64 and p['cblocks'] * 64 > c['c'] // 4,
    'ragged_group': lambda c, p, o: p['bstrips'] % p['ps'] != 0 and max(c['w'], o[1]) % KTB != 0,
    'multi_group': lambda c, p, o: p['strip_groups'] > 1,
    'tiles_65_127': lambda c, p, o: 65 <= p['tiles'] <= 127 and p['tiles'] % 64 != 0,
    'fwd_tail': lambda c, p, o: (c['n'] * o[0] * p['fstrips'] * (c['c'] // 4)) % 256 != 0,
    'wo1': lambda c, p, o: o[1] == 1, 'wo8': lambda c, p, o: o[1] == 8, 'wo9': lambda c, p, o: o[1] == 9,
    'ho1': lambda c, p, o: o[0] == 1,
    'stride_1_2': lambda c, p, o: c['s'] == (1, 2), 'stride_2_1': lambda c, p, o: c['s'] == (2, 1),
    'dil_2_1': lambda c, p, o: c['dil'] == (2, 1) and c['k'][0] > 1 and p['fd1'] == 1,
    'dil_1_3': lambda c, p, o: c['dil'] == (1, 3) and c['k'][1] > 1,
    'dil_6_6': lambda c, p, o: c['dil'] == (6, 6) and min(c['k']) > 1,
    'taps_in_padding': lambda c, p, o: _dead_tap(c),
    'pad_0_2': lambda c, p, o: c['p'] == (0, 2), 'pad_3_0': lambda c, p, o: c['p'] == (3, 0),
    'ph_ne_pw': lambda c, p, o: c['p'][0] != c['p'][1],
    'wo_gt_w_s1': lambda c, p, o: c['s'] == (1, 1) and o[1] > c['w'] and o[0] > c['h'],
    'wo_gt_w_s2': lambda c, p, o: c['s'] == (2, 2) and o[1] > c['w'] and o[0] > c['h'],
    'ho_gt_h': lambda c, p, o: o[0] > c['h'] and o[1] < c['w'],
    'bias_only_border': lambda c, p, o: c['bias'] and _only_padding(c),
    's2_even_w': lambda c, p, o: c['s'][1] == 2 and c['w'] % 2 == 0,
    's2_odd_w': lambda c, p, o: c['s'][1] == 2 and c['w'] % 2 == 1,
    'even_kernel': lambda c, p, o: c['k'][0] % 2 == 0 and c['k'][1] % 2 == 0,
}
FACT_CHECKS.update({f'cl{v}': (lambda c, p, o, v=v: p['cl'] == v) for v in REQUIRED_CL})
assert set(FACT_CHECKS) == REQUIRED_FACTS


# ---- inputs and the fp64 reference (torch on the CPU) -----------------------------------------------------------------------
U = 2.0 ** -24


def inputs(case, kind):
    """x [N, C, H, W], w [C, 1, kh, kw], bias [C] or None, dy [N, C, Ho, Wo] as fp32.  kind 'exact': integers in [-4, 4];
    'normal': unit normal."""
    import torch
    gen = torch.Generator().manual_seed(1000 + CASES.index(case))
    ho, wo = out_size(case)
    shapes = [(case['n'], case['c'], case['h'], case['w']), (case['c'], 1) + case['k'], (case['c'],), (case['n'], case['c'], ho, wo)]
    if kind == 'exact':
        x, w, b, g = (torch.randint(-4, 5, s, generator=gen).float() for s in shapes)
    else:
        x, w, b, g = (torch.randn(s, generator=gen) for s in shapes)
    return x, w, (b if case['bias'] else None), g


_REF = {}


def reference(case, kind):
    """The fp64 results from the fp32 inputs and the sums of magnitudes the bounds are made of.  Computed once per (case, kind);
    callers must not modify what they get.

    Exact inputs: every term of every sum is an integer of magnitude <= 16 (<= 4 for the bias and for db), so every partial sum
    of y, dx, dw and db in any order is an integer of magnitude <= the sum of the terms' magnitudes; below 2^24 every such
    integer is an fp32 number and every fp32 FMA or addition on the way is exact.  The sums of magnitudes are asserted below
    2^24 here, and 16 x (the largest term count) is the cap they cannot pass.

    Unit-normal inputs, u = 2^-24, T taps:
      y, dx   |err| <= (T + 2) u (sum |x w| + |b|): a chain of T FMAs and the bias addition;
      dw, db  |err| <= (d + 2) u sum |g x| (db: sum |g|), d = 16 + (ps - 1) + ceil(tiles / 64) + 63: a thread's 4 x 4 pixels,
              the workgroup's strips, a reduction slice's tiles, the 64 slices (depth() below).
    Under the fused ReLU an element whose fp64 pre-activation lies inside the forward bound has no certain mask: `uncertain`;
    its dy is set to 0 (in `g`, which the device gets)."""
    import torch
    import torch.nn.functional as F
    key = (case['name'], kind)
    if key in _REF:
        return _REF[key]
    x, w, b, g = inputs(case, kind)
    taps = case['k'][0] * case['k'][1]
    conv = lambda xx, ww, bb: F.conv2d(xx, ww, bb, case['s'], case['p'], case['dil'], groups=case['c'])   # noqa: E731
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    br = b.double().requires_grad_() if b is not None else None
    pre = conv(xr, wr, br)
    xa, wa = x.double().abs().requires_grad_(), w.double().abs().requires_grad_()
    ba = b.double().abs().requires_grad_() if b is not None else None
    mag = conv(xa, wa, ba)
    ybound = (taps + 2) * U * mag.detach()
    uncertain = torch.zeros_like(pre, dtype=torch.bool)
    if case['relu']:
        if kind == 'normal':
            uncertain = pre.detach().abs() <= ybound
            g = torch.where(uncertain, torch.zeros_like(g), g)
        gm = torch.where(pre.detach() > 0, g, torch.zeros_like(g))
    else:
        gm = g
    pre.backward(gm.double())
    mag.backward(gm.double().abs())
    r = dict(x=x, w=w, b=b, g=g, pre=pre.detach(), y=pre.detach().clamp_min(0) if case['relu'] else pre.detach(),
             dx=xr.grad, dw=wr.grad, db=br.grad if b is not None else None,
             ymag=mag.detach(), dxmag=xa.grad, dwmag=wa.grad, dbmag=ba.grad if b is not None else gm.double().abs().sum((0, 2, 3)),
             uncertain=uncertain, taps=taps)
    if b is None:       # db may be asked for without a bias in the forward: the sum of the masked gradient
        r['db'] = gm.double().sum((0, 2, 3))
    if kind == 'exact':
        ho, wo = out_size(case)
        assert 16 * max(taps + 1, case['n'] * ho * wo) < 2 ** 24
        assert max(float(r[k].max()) for k in ('ymag', 'dxmag', 'dwmag', 'dbmag')) < 2 ** 24
    _REF[key] = r
    return r


def depth(p):
    """roundings in the longest chain of a dw / db element under the plan words p"""
    return KTH * KTB + (p['ps'] - 1) + -(-p['tiles'] // 64) + 63
