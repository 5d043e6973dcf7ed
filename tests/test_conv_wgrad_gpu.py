"""Every weight-gradient instantiation (csrc/conv_wgrad*.hip) at its split and geometry edges, through the C-ABI, against a
float64 convolution's weight and bias gradient.

Cases are picked WITH evk_conv2d_wgrad_route: each one names the kernel and the plan property it exists for (`want`) and fails
with "no longer covers" when a retuned planner takes that away; the last test asserts the union.  Operands have a non-zero
mean; dw, db and the whole workspace hold NaN before a launch, and dw / the workspace are slices of larger allocations whose
surroundings hold a sentinel: an element nobody wrote, a partial that is reduced but never written, or a store past the
end fails.

Bound (none is new): e = max|hip - ref64| / max|ref64| <= max(4 e32, 1e-5) for the fp32-grade arithmetics, where e32 is the
same error of torch's fp32 CPU convolution on the same case (4 = f16x2's 22 operand bits against fp32's 24; 1e-5 the bound of
test_planar_weight_gradient); plain bf16 at the grade tests/test_bf16_mode_gpu.py pins (2e-2)."""
import ctypes

import pytest
import torch
import torch.nn.functional as TF

from tests.guard_common import guarded as _guarded, guards_intact as _guards_intact
from tests.wgrad_plan_common import DY_PACKED, PLANAR, SHARED, X_PACKED, conv_desc, fields, planar_ok, wgrad_route

pytestmark = pytest.mark.gpu

BF16_GRADE = 2e-2   # tests/test_bf16_mode_gpu.py

# form -> (arithmetic of evk_conv2d_wgrad_route, flags)
FORMS = {'f32': (0, 0), 'bf16': (1, 0), 'bf16x3': (3, 0), 'f16x2': (2, 0), 'px': (2, X_PACKED), 'pd': (2, DY_PACKED),
         'pxd': (2, X_PACKED | DY_PACKED), 'planar': (2, PLANAR)}
ALL = tuple(FORMS)
SPLIT_FORMS = ('bf16', 'bf16x3', 'f16x2', 'px', 'pd', 'pxd')


def _c(name, n, cin, h, w, cout, kh, kw, s=(1, 1), p=None, dil=(1, 1), want=None, forms=ALL):
    p = (None, None) if p is None else p
    assert set(want or {}) <= set(forms), name
    return dict(name=name, d=(n, h, w, cin, cout, kh, kw, s[0], s[1], p[0], p[1], dil[0], dil[1]), want=want or {}, forms=forms)


def _all(forms, *tags):
    return {f: set(tags) for f in forms}


CASES = [
    # ---- every tile of the single-role kernels in every operand form, the wave-specialised kernel W8 true / false
    _c('tile64x64', 2, 64, 16, 16, 64, 1, 1, want={**_all(('f32',) + SPLIT_FORMS, 'single', 'tile64x64'), 'planar': {'tr1'}}),
    _c('tile64x128', 2, 64, 16, 16, 64, 3, 3, want={**_all(('f32',) + SPLIT_FORMS, 'single', 'tile64x128'), 'planar': {'tr1'}}),
    _c('tile128x64', 2, 64, 16, 16, 96, 1, 1, want=_all(('f32',) + SPLIT_FORMS, 'single', 'tile128x64')),
    _c('tile128x128', 2, 128, 16, 16, 96, 3, 3, want=_all(('f32',) + SPLIT_FORMS, 'single', 'tile128x128')),
    _c('ws_w8', 2, 64, 16, 16, 128, 3, 3, want={**_all(SPLIT_FORMS, 'ws', 'W8'), 'planar': {'tr1'}}),
    _c('ws_wo13', 2, 64, 13, 13, 128, 3, 3, want=_all(SPLIT_FORMS, 'ws', 'W8=false', 'last_step<32')),
    # ---- one split: fewer than 32 pixels, and a pixel count that is no multiple of 32
    _c('m16_single', 1, 64, 4, 4, 64, 3, 3, want=_all(('f32',) + SPLIT_FORMS, 'single', 'splitk1', 'M<32')),
    _c('m16_wide', 1, 128, 2, 8, 128, 3, 3, want={**_all(SPLIT_FORMS, 'ws', 'splitk1', 'M<32'), 'planar': {'tr1', 'splitk1', 'M<32'}}),
    _c('m40_wide', 1, 128, 5, 8, 128, 3, 3, want={**_all(SPLIT_FORMS, 'ws', 'splitk1', 'M%32'), 'planar': {'tr1', 'splitk1', 'M%32'}}),
    _c('m40_single', 1, 64, 5, 8, 64, 3, 3, want={**_all(('f32',) + SPLIT_FORMS, 'single', 'splitk1', 'M%32'), 'planar': {'tr1', 'M%32'}}),
    # ---- several splits: a shorter last chunk, a last step of fewer than 32 pixels, chunks that begin mid-row and straddle images
    _c('short_single', 7, 128, 21, 19, 96, 3, 3,      # 11 chunks of 256, the last 233
       want=_all(('f32',) + SPLIT_FORMS, 'single', 'short_last', 'last_step<32', 'midrow', 'straddle')),
    _c('short_ws', 7, 128, 21, 19, 128, 3, 3, want=_all(SPLIT_FORMS, 'ws', 'W8=false', 'short_last', 'last_step<32', 'midrow', 'straddle')),
    _c('short_tr1', 3, 128, 11, 24, 128, 3, 3,        # 4 chunks of 224, the last 120 (3 steps of 32 + 24)
       want={**_all(SPLIT_FORMS, 'ws', 'short_last'), 'planar': {'tr1', 'short_last', 'last_step<32', 'midrow', 'straddle'}}),
    _c('short_tr9', 1, 64, 9, 32, 128, 3, 3, want={'planar': {'tr9', 'short_last'}, 'f16x2': {'ws', 'short_last'}}),   # 160 + 128
    _c('column_3x1', 1, 64, 257, 1, 128, 3, 1, p=(1, 0),     # chunks 160 + 97 on a map one pixel wide
       want=_all(('f32',) + SPLIT_FORMS, 'single', 'short_last', 'last_step<32')),
    _c('midrow_tr9', 1, 128, 64, 96, 256, 3, 3,     # chunk 256 = 2 2/3 rows; the wave-specialised kernel splits 24 / 12 (shared)
       want={'planar': {'tr9', 'midrow'}, 'f16x2': {'ws', 'midrow', 'shared_differs'}}, forms=('f32', 'f16x2', 'pxd', 'planar')),
    _c('straddle_tr9', 3, 64, 36, 32, 128, 3, 3,    # chunk 256 against images of 1152 pixels
       want={'planar': {'tr9', 'straddle'}, 'f16x2': {'ws', 'straddle'}}),
    _c('straddle_ws', 5, 192, 24, 40, 192, 3, 3,    # 17 chunks of 288 (shared: 9 of 544) against images of 960 pixels
       want={**_all(('bf16x3', 'f16x2', 'pxd'), 'ws', 'straddle', 'midrow', 'short_last'), 'planar': {'tr1', 'straddle', 'midrow', 'shared_differs'}},
       forms=('f32', 'bf16x3', 'f16x2', 'pxd', 'planar')),
    # ---- the half-chip plan differs from the whole-chip one
    _c('shared_ws_tr1', 1, 256, 48, 48, 256, 3, 3, p=(2, 2), dil=(2, 2),    # 9 chunks of 256 against 7 of 352
       want={'f16x2': {'ws', 'shared_differs'}, 'pxd': {'ws', 'shared_differs'}, 'planar': {'tr1', 'shared_differs'}},
       forms=('f16x2', 'px', 'pd', 'pxd', 'planar')),
    _c('shared_tr9', 1, 512, 40, 64, 256, 3, 3,     # nine-tap: 10 chunks of 256 against 8 of 320
       want={'planar': {'tr9', 'shared_differs'}, 'f16x2': {'ws', 'shared_differs'}}, forms=('f16x2', 'pxd', 'planar')),
    # ---- geometry the gathers branch on
    _c('s2_odd', 2, 64, 37, 29, 64, 3, 3, s=(2, 2), p=(1, 1), want={'f16x2': {'single'}}),
    _c('s2x1', 2, 64, 20, 24, 128, 3, 3, s=(2, 1), p=(1, 1), want={'f16x2': {'ws'}, 'planar': {'tr1'}}),
    _c('k1x7', 2, 64, 16, 24, 64, 1, 7, want={'planar': {'tr1'}}),
    _c('k7x1', 2, 64, 16, 24, 64, 7, 1, want={'planar': {'tr1'}}),
    _c('pad0', 2, 128, 18, 18, 128, 3, 3, p=(0, 0), want={'planar': {'tr1'}, 'f16x2': {'ws'}}),
    _c('pad2', 2, 128, 16, 16, 128, 3, 3, p=(2, 2), want={'f16x2': {'ws', 'W8=false'}}),
    _c('pad2x0', 2, 64, 16, 16, 64, 3, 3, p=(2, 0)),
    _c('dil6_32', 1, 128, 32, 32, 128, 3, 3, dil=(6, 6), want={'planar': {'tr1'}, 'f16x2': {'ws'}}),
    _c('dil12_8', 2, 128, 8, 8, 128, 3, 3, dil=(12, 12), want={'planar': {'tr1'}}),     # eight taps read nothing but padding
    _c('dil18_4', 2, 128, 4, 4, 128, 3, 3, dil=(18, 18), want={'f16x2': {'ws', 'W8=false'}}),
    _c('dil18_32', 1, 64, 32, 32, 64, 3, 3, dil=(18, 18), want={'planar': {'tr1'}, 'f16x2': {'single'}}),
    _c('dil2_s2', 2, 64, 17, 17, 64, 3, 3, s=(2, 2), p=(2, 2), dil=(2, 2)),
    _c('cin72_cout200', 2, 72, 12, 12, 200, 3, 3),          # Ktot = 648: ragged column tile; ragged row tile
    _c('cin200_cout136', 2, 200, 12, 12, 136, 3, 3),
    _c('cout520', 1, 64, 10, 10, 520, 3, 3),                # five row tiles, the last with 8 rows; bias gradient of 520 channels
    _c('cout4', 2, 128, 20, 20, 4, 3, 3, want={'f16x2': {'single', 'short_last'}}),
    _c('cin4_cout4', 2, 4, 20, 20, 4, 1, 1, want={'f32': {'tile64x64'}}),
]
assert len({c['name'] for c in CASES}) == len(CASES)

# what the union of the cases must contain: (kernel class, edge)
EDGES = [(k, e) for k in ('single', 'ws', 'tr1') for e in ('splitk1+M<32', 'splitk1+M%32', 'short_last', 'last_step<32', 'midrow', 'straddle')] + \
        [('tr9', e) for e in ('short_last', 'midrow', 'straddle')] + [(k, 'shared_differs') for k in ('ws', 'tr1', 'tr9')]
INSTANTIATIONS = (
    [f'conv_wgrad_kernel<{bm}, {bn}, 2, 2>' for bm in (64, 128) for bn in (64, 128)] +
    [f'conv_wgrad_x3_kernel<{bm}, {bn}, 2, 2, {npx}>' for bm in (64, 128) for bn in (64, 128) for npx in (1, 2, 3, 4)] +
    [f'conv_wgrad_x3ws_kernel<128, 256, {np_}, {w8}, {pk}>' for w8 in ('true', 'false')
     for np_, pk in ((1, 'false, false'), (3, 'false, false'), (2, 'false, false'), (2, 'true, false'), (2, 'false, true'), (2, 'true, true'))] +
    ['conv_wgrad_tr_kernel<1>', 'conv_wgrad_tr_kernel<9>'])
assert len(INSTANTIATIONS) == 34

LAUNCHED = {}     # case name -> {(form, shared): (kernel, tags)}: what actually ran
WORST = {}        # (arithmetic, kernel family) -> (e / bound, case, what)


def case_desc(case):
    n, h, w, cin, cout, kh, kw, sh, sw, ph, pw, dh, dw = case['d']
    return conv_desc(n, h, w, cin, cout, kh, kw, sh, sw, ph, pw, dh, dw)


def plan_tags(lib, d, planes, flags):
    """(kernel name, set of tags) of one launch, read from the plan the library answers"""
    rc, name, (bm, bn, tco, tk, sk, chunk) = wgrad_route(lib, d, planes, flags)
    assert rc == 0, (fields(d), planes, flags, lib.evk_last_error())
    m, hw = d.N * d.Ho * d.Wo, d.Ho * d.Wo
    fam = name.split('<')[0]
    tags = {{'conv_wgrad_kernel': 'single', 'conv_wgrad_x3_kernel': 'single', 'conv_wgrad_x3ws_kernel': 'ws',
             'conv_wgrad_tr_kernel': 'tr9' if name.endswith('<9>') else 'tr1'}[fam]}
    if 'single' in tags:
        tags.add(f'tile{bm}x{bn}')
    if 'ws' in tags:
        tags.add('W8' if d.Wo % 8 == 0 else 'W8=false')
    tags.add('splitk1' if sk == 1 else 'split')
    if m < 32:
        tags.add('M<32')
    if m % 32:
        tags.add('M%32' if sk == 1 else 'last_step<32')
    if sk > 1:
        if m % chunk:
            tags.add('short_last')
        if chunk % d.Wo:
            tags.add('midrow')
        if any(z * chunk // hw != (min(m, (z + 1) * chunk) - 1) // hw for z in range(sk)):
            tags.add('straddle')
    if planes == 2:
        _, _, other = wgrad_route(lib, d, planes, flags ^ SHARED)
        if other[4] != sk:
            tags.add('shared_differs')
    return name, tags, (sk, chunk)


def case_launches(lib, case):
    """[(form, shared flag, kernel, tags)] a case launches: every form it lists, and the half-chip plan where it differs"""
    d = case_desc(case)
    out = []
    for form in case['forms']:
        planes, flags = FORMS[form]
        if form == 'planar' and not planar_ok(d):
            assert 'planar' not in case['want'], (case['name'], 'no longer takes planar operands')
            continue
        name, tags, plan = plan_tags(lib, d, planes, flags)
        out.append((form, 0, name, tags, plan))
        if 'shared_differs' in tags:
            name_sh, tags_sh, plan_sh = plan_tags(lib, d, planes, flags | SHARED)
            out.append((form, SHARED, name_sh, tags_sh, plan_sh))
    return out


def _bits(lib, t, aws, st):
    from ever_amd import _C
    b = torch.zeros(int(lib.evk_absmax_words()), dtype=torch.int32, device=t.device)
    _C.call('evk_absmax', t.data_ptr(), t.numel(), b.data_ptr(), aws.data_ptr(), st)
    return b


def _rel(a, ref):
    return (a.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)


def _reference(d, x, dy):
    """weight and bias gradient in float64 by autograd, and the errors of torch's fp32 CPU convolution against them"""
    out = []
    for dt in (torch.float64, torch.float32):
        w = torch.zeros(d.Cout, d.Cin, d.kh, d.kw, dtype=dt, requires_grad=True)
        b = torch.zeros(d.Cout, dtype=dt, requires_grad=True)
        y = TF.conv2d(x.to(dt), w, b, (d.stride_h, d.stride_w), (d.pad_h, d.pad_w), (d.dil_h, d.dil_w))
        assert y.shape == dy.shape
        (y * dy.to(dt)).sum().backward()
        out.append((w.grad.permute(0, 2, 3, 1).contiguous(), b.grad))
    (dw64, db64), (dw32, db32) = out
    return dw64, db64, _rel(dw32, dw64), _rel(db32, db64)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_weight_gradient_against_fp64(cuda, case):
    from ever_amd import _C
    lib = _C.load()
    d = case_desc(case)
    launches = case_launches(lib, case)
    by_form = {(f, sh): (name, tags) for f, sh, name, tags, _ in launches}
    for form, want in case['want'].items():
        have = by_form[(form, 0)][1]
        assert want <= have, f"{case['name']} no longer covers {sorted(want - have)} for {form}: {by_form[(form, 0)]}"

    st = torch.cuda.current_stream().cuda_stream
    aws = torch.zeros(lib.evk_absmax_workspace_bytes(), dtype=torch.uint8, device=cuda)
    g = torch.Generator().manual_seed(1000 + sum(case['d'][:8]))
    x_nchw = torch.randn(d.N, d.Cin, d.H, d.W, generator=g) + 0.5
    dy_nchw = torch.randn(d.N, d.Cout, d.Ho, d.Wo, generator=g) + 0.25
    dw64, db64, e32_w, e32_b = _reference(d, x_nchw, dy_nchw)
    x = x_nchw.permute(0, 2, 3, 1).contiguous().to(cuda)
    dy = dy_nchw.permute(0, 2, 3, 1).contiguous().to(cuda)
    bx, bd = _bits(lib, x, aws, st), _bits(lib, dy, aws, st)
    packed = {}

    def operand(t, bits, kind):
        if kind == 'fp32':
            return t
        if (id(t), kind) not in packed:
            out = torch.empty_like(t)
            _C.call('evk_pack_planar_f16x2' if kind == 'planar' else 'evk_pack_f16x2', t.data_ptr(), t.numel(), bits.data_ptr(), out.data_ptr(), st)
            packed[(id(t), kind)] = out
        return packed[(id(t), kind)]

    ktot = d.kh * d.kw * d.Cin
    n_dw = d.Cout * ktot
    ws_bytes = {0: lib.evk_conv2d_wgrad_workspace_bytes(ctypes.byref(d)), 1: lib.evk_conv2d_wgrad_x3_workspace_bytes(ctypes.byref(d))}
    results = {}
    for form, shared, name, tags, (sk, chunk) in launches:
        planes, flags = FORMS[form]
        what = (case['name'], form, shared, name, sk, chunk)
        wsb = ws_bytes[1 if planes else 0]
        assert wsb % 4 == 0 and (sk == 1 or wsb >= sk * n_dw * 4), what      # (never launch a plan the workspace cannot hold)
        ws_whole, ws = _guarded(wsb // 4, cuda)
        dw_whole, dw = _guarded(n_dw, cuda)
        want_db = not (flags & (DY_PACKED | PLANAR))
        db = torch.full((d.Cout,), float('nan'), device=cuda) if want_db else None
        dbp = db.data_ptr() if want_db else None
        dp = ctypes.byref(d)
        if form == 'f32':
            _C.call('evk_conv2d_wgrad', dp, x.data_ptr(), dy.data_ptr(), dw.data_ptr(), dbp, ws.data_ptr(), wsb, st)
        elif form == 'bf16':
            _C.call('evk_conv2d_wgrad_bf16', dp, x.data_ptr(), dy.data_ptr(), dw.data_ptr(), dbp, ws.data_ptr(), wsb, st)
        elif form == 'bf16x3':
            _C.call('evk_conv2d_wgrad_x3', dp, x.data_ptr(), dy.data_ptr(), dw.data_ptr(), dbp, ws.data_ptr(), wsb, st)
        else:
            xo = operand(x, bx, 'planar' if flags & PLANAR else 'packed' if flags & X_PACKED else 'fp32')
            do = operand(dy, bd, 'planar' if flags & PLANAR else 'packed' if flags & DY_PACKED else 'fp32')
            _C.call('evk_conv2d_wgrad_f16x2_ex', dp, xo.data_ptr(), bx.data_ptr(), do.data_ptr(), bd.data_ptr(), dw.data_ptr(), dbp,
                    ws.data_ptr(), wsb, flags | shared, st)
        torch.cuda.synchronize()
        assert _guards_intact(dw_whole, n_dw), ('a store beside dw', what)
        assert _guards_intact(ws_whole, wsb // 4), ('a store beside the workspace', what)
        got = dw.cpu().view(d.Cout, d.kh, d.kw, d.Cin)
        assert torch.isfinite(got).all(), ('dw holds an element nobody wrote, or a partial nobody wrote was reduced', what)
        arith = 'f16x2' if planes == 2 else form
        e = _rel(got, dw64)
        bound = BF16_GRADE if form == 'bf16' else max(4 * e32_w, 1e-5)
        key = (arith, name.split('<')[0] + ('<9>' if name.endswith('<9>') else ''))
        if e / bound > WORST.get(key, (0.0,))[0]:
            WORST[key] = (e / bound, case['name'], f'e {e:.2e} e32 {e32_w:.2e}')
        print(f"{case['name']:16s} {form:7s} sh={shared:2d} {name:52s} splitk {sk:3d} chunk {chunk:5d}  dw e {e:.2e} / bound {bound:.2e} (e32 {e32_w:.2e})")
        assert e <= bound, ('dw', what, e, bound, e32_w)
        if want_db:
            eb = _rel(db.cpu(), db64)
            bb = max(4 * e32_b, 1e-5)
            print(f"{'':16s} {'':7s} db rows {d.N * d.Ho * d.Wo} Cout {d.Cout}: e {eb:.2e} / bound {bb:.2e} (e32 {e32_b:.2e})")
            assert torch.isfinite(db).all() and eb <= bb, ('db', what, eb, bb)
        results[(form, shared)] = (got, (sk, chunk))
        LAUNCHED.setdefault(case['name'], {})[(form, shared)] = (name, tags)

    # operand forms agree: packed words are the fp32 operand's (h, l) pair — bit for bit under the same plan; the planar pair
    # is the same pair in another memory order — to the accumulation order
    scale = dw64.abs().max().item()
    for shared in (0, SHARED):
        base = results.get(('f16x2', shared))
        for form in ('px', 'pd', 'pxd'):
            if base and (form, shared) in results:
                assert results[(form, shared)][1] == base[1]
                assert torch.equal(results[(form, shared)][0], base[0]), (case['name'], form, shared, 'packed operands changed the bits')
        ref = results.get(('pxd', shared)) or base
        if ref and ('planar', shared) in results:
            diff = (results[('planar', shared)][0].double() - ref[0].double()).abs().max().item() / scale
            assert diff <= 1e-5, (case['name'], shared, diff)
            # Under the SAME split the two kernels multiply identical (h, l) pairs: they differ by fp32 accumulation order and a
            # handful of roundings of the result (partials, their sum, the scale) only.  e32 is that error for another fp32
            # implementation of the same reduction, so the two stay within 4 e32 of each other, or 16 ulp of the result scale
            # where the reduction is too short for e32 to say anything.  (A tail step that should not be there moves the planar
            # kernel by a term of the operand's low plane, 2^-12 of a product: far below 1e-5 of a long sum, far above this.)
            if results[('planar', shared)][1] == ref[1]:
                tight = max(4 * e32_w, 16 * 2.0 ** -24)
                print(f"{case['name']:16s} planar vs packed, same plan, sh={shared:2d}: {diff:.2e} / bound {tight:.2e}")
                assert diff <= tight, (case['name'], shared, 'planar vs packed under the same plan', diff, tight)


def test_the_cases_cover_every_instantiation_and_edge():
    """Read from the plans the library answers for CASES (no launch): all 34 instantiations, every split edge per kernel class,
    a differing half-chip plan for each wide-tile kernel, both bias-gradient regimes.  Whatever the cases above launched in this
    process is held against the same plans."""
    from ever_amd import _C
    lib = _C.load()
    names, edges, db_rows, packed_multi = set(), set(), set(), False
    for case in CASES:
        d = case_desc(case)
        launches = case_launches(lib, case)
        for form, shared, name, tags, (sk, chunk) in launches:
            names.add(name)
            kind = next(k for k in ('single', 'ws', 'tr1', 'tr9') if k in tags)
            for t in tags:
                edges.add((kind, t))
                if 'splitk1' in tags:
                    edges.add((kind, 'splitk1+' + t))
            if form in ('f32', 'bf16x3', 'f16x2'):
                m = d.N * d.Ho * d.Wo
                db_rows.add(('split' if sk > 1 else 'one', 'rows>256' if m > 256 else 'rows<=256', d.Cout if d.Cout in (4, 520) else 0))
            packed_multi = packed_multi or (form == 'pxd' and {'midrow', 'split'} <= tags)
        if case['name'] in LAUNCHED:
            ran = LAUNCHED[case['name']]
            assert ran == {(f, sh): (name, tags) for f, sh, name, tags, _ in launches}, case['name']
    assert set(INSTANTIATIONS) <= names, sorted(set(INSTANTIATIONS) - names)
    assert set(EDGES) <= edges, sorted(set(EDGES) - edges)
    assert {r[:2] for r in db_rows} >= {('split', 'rows>256'), ('one', 'rows<=256')} and {r[2] for r in db_rows} >= {4, 520}, db_rows
    assert packed_multi
    if WORST:
        print('\nworst e / bound per arithmetic and kernel:')
        for (arith, fam), (r, name, what) in sorted(WORST.items()):
            print(f'  {arith:7s} {fam:26s} {r:5.2f}  ({name}: {what})')
