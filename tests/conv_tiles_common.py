"""The forward / data-gradient tile forms that only large grids reach, forced onto small ragged shapes: the case table,
the instantiation evk_conv2d_route must name for every (case, force, arithmetic, direction), and the set of instantiations
the table has to reach.  No torch.cuda here: tests/test_conv_tiles_cpu.py walks the table on the host, tools/check_tiles.py
(run by tests/test_conv_tiles_gpu.py) launches it.

The planner (csrc/conv_route.hip) takes a 128-row X3 / X3Ws tile, a 128-wide halo tile or a 16-row patch only from 256 (or
512) workgroups on; the fp64 comparisons of the GPU suite are far smaller.  Under EVK_TUNE the planner re-reads EVK_X3_FORCE /
EVK_X3_HALO_FORCE on every call (rows of its kForced table), inside the launch's own plane layout, so the weight planes the
Python layer produced stay valid."""


def _g(name, n, h, w, cin, cout, k, s=1, p=0, dil=1, bias=False, relu=False, **more):
    pair = lambda v: (v, v)   # noqa: E731
    return dict(name=name, n=n, cin=cin, h=h, w=w, cout=cout, k=pair(k), s=pair(s), p=pair(p), dil=pair(dil), bias=bias, relu=relu,
                **more)


ARITH = {'f16x2': 2, 'bf16x3': 3, 'bf16': 1}      # arithmetic -> planes argument of evk_conv2d_route = the kernels' NP

# ---- generic family: implicit-GEMM kernels (conv_igemm_x3.hip, conv_igemm_x3ws.hip) --------------------------------------
GENERIC_ENV = dict(EVK_TUNE='1', EVK_X3_HALO='0')
GENERIC_VAR = 'EVK_X3_FORCE'
GENERIC_FORCES = {   # force -> instantiation, NP left open; every case below takes every one, forward and each residue class
    'w256': 'conv_igemm_x3ws_kernel<128, 256, 2, 2, 2, {np}>',
    'w128': 'conv_igemm_x3ws_kernel<128, 128, 2, 2, 2, {np}>',
    'w64': 'conv_igemm_x3ws_kernel<128, 64, 2, 2, 2, {np}>',
    'c128x128': 'conv_igemm_x3_kernel<128, 128, 2, 2, 1, {np}>',
    'c64x128': 'conv_igemm_x3_kernel<64, 128, 2, 2, 1, {np}>',
    'c128x64': 'conv_igemm_x3_kernel<128, 64, 2, 2, 1, {np}>',
    'c64x64': 'conv_igemm_x3_kernel<64, 64, 2, 2, 1, {np}>',
}
GENERIC_CASES = [
    # M = 8450: 67 row tiles of 128, the last holds 2 rows.  K = 72 of Kpad 96 (a K tail inside the 32-wide step).  Cout 200:
    # 4 column tiles at width 64 (the last 8 wide), 2 at 128, one partial at 256.  w64: 268 tiles on the persistent grid of
    # 256 — 12 workgroups walk two tiles.
    _g('g1', 2, 65, 65, 72, 200, 1, raw=True),
    # odd map under stride 2: four data-gradient residue classes (2x2, 2x1, 1x2 and 1x1 taps), each forced
    _g('g2', 1, 37, 29, 64, 136, 3, s=2, p=1, bias=True, relu=True),
    # taps wholly in the padding; 264 = 256 + 8
    _g('g3', 1, 32, 32, 128, 264, 3, p=6, dil=6),
    # one K step per tile.  w64: 603 tiles — workgroups walk 2 or 3 tiles and the LDS ring crosses a tile boundary on every
    # step.  Data gradient (520 -> 8): a long reduction into an 8-wide output under every tile width.
    _g('g4', 2, 65, 65, 8, 520, 1, raw=True),
    # "same" 3x3 through the gather kernels, Cin not a multiple of 16
    _g('g5', 1, 30, 27, 40, 72, 3, p=1, bias=True),
    # g1 with Cout a whole number of tiles of every width: the statistics epilogue needs Cd % BN == 0 (bn_stats_setup), so it
    # never engages on g1 / g4.  w64: 268 tiles, one per workgroup in statistics mode.
    _g('g6', 2, 65, 65, 72, 256, 1, raw=True, stats=True),
    # three 8-channel chunks per tap, forward and data gradient alike: a 32-element K step spans taps of a multi-tap filter
    # (the K cursor re-derives its tap by division with kw > 1: g4 is 1x1, g5 has 5 chunks per tap).  K = 216 of Kpad 224;
    # four row tiles of 128, the last holds 53 rows
    _g('g7', 1, 19, 23, 24, 24, 3, p=1, bias=True),
]

# ---- halo family: conv3x3_halo_x3.hip, all 3x3 stride 1 pad 1 -------------------------------------------------------------
HALO_ENV = dict(EVK_TUNE='1', EVK_X3_HALO_MIN_WG='0', EVK_WINO='0')
HALO_VAR = 'EVK_X3_HALO_FORCE'
HALO_FORCES = {      # force -> (tile width, patch rows, matrix waves under f16x2; the other arithmetics have four)
    'h64x8': (64, 8, 4), 'm64x8': (64, 8, 8), 'h64x16': (64, 16, 4), 'm64x16': (64, 16, 8),
    'h128x8': (128, 8, 4), 'h128x16': (128, 16, 4), 'm128x8': (128, 8, 8), 'm128x16': (128, 16, 8),
}
HALO_NAME = 'conv3x3_halo_x3_kernel<{bn}, {ph}, {np}, {dma}, {mw}>'
# fwd / dgrad: 'every' = every forced form is taken; 'narrow' = Cd <= 64, the 128-wide forces are refused and the rule's
# <64, 8, ..., 4> runs instead; anything else = the implicit-GEMM instantiation the launch takes whatever the force says
HALO_CASES = [
    # 4.5 chunks of channels, last patch column 8 wide, Cout = 128 + 8; the data gradient has 8.5 chunks and Cd = 64 + 8
    _g('h1', 1, 48, 40, 72, 136, 3, p=1, bias=True, fwd='every', dgrad='every', raw=True),
    _g('h2', 2, 30, 27, 32, 64, 3, p=1, bias=True, relu=True, fwd='narrow', dgrad='conv_igemm_x3_kernel<64, 64, 2, 2, 1, {np}>'),
    # 77 % 16 = 13, 43 = 2 x 16 + 11, 2.5 chunks
    _g('h3', 1, 77, 43, 40, 200, 3, p=1, bias=True, fwd='every', dgrad='conv_igemm_x3_kernel<64, 64, 2, 2, 1, {np}>'),
    # 36 % 16 = 4: the rule refuses the 16-row patch, the force takes it and the last patch row is three quarters empty
    _g('h4', 1, 36, 30, 64, 192, 3, p=1, fwd='every', dgrad='narrow'),
    # the data gradient (72 -> 136) into a 128-wide tile plus an 8-wide one with 4.5 chunks of reduction; 22 % 16 = 6, 29 = 16 + 13
    _g('h5', 2, 22, 29, 136, 72, 3, p=1, bias=True, fwd='every', dgrad='every'),
    # h1 with Cout = one 128-wide tile = two 64-wide ones: the statistics epilogue engages (Cd % BN == 0)
    _g('h6', 1, 48, 40, 72, 128, 3, p=1, bias=True, fwd='every', dgrad='every', raw=True, stats=True),
]

# ---- fp32 family: conv_igemm_f32.hip, route_fp32 is a pure rule (no switch) ---------------------------------------------------
FP32_CASES = [   # (case, forward instantiation, data-gradient instantiation)
    (_g('f32_a', 1, 129, 127, 8, 520, 1), 'conv_igemm_kernel<128, 128, 2, 2>', 'conv_igemm_kernel<64, 64, 2, 2>'),
    (_g('f32_e', 1, 129, 127, 520, 8, 1), 'conv_igemm_kernel<64, 64, 2, 2>', 'conv_igemm_kernel<128, 128, 2, 2>'),
    (_g('f32_c', 1, 257, 257, 4, 40, 3, p=1), 'conv_igemm_kernel<128, 64, 2, 2>', 'conv_igemm_kernel<128, 64, 2, 2>'),
    # 517 row tiles of 256, the last one ragged
    (_g('f32_b', 2, 257, 257, 4, 40, 3, p=1), 'conv_igemm_kernel<256, 64, 4, 1>', 'conv_igemm_kernel<256, 64, 4, 1>'),
]

FAMILIES = {'generic': (GENERIC_ENV, GENERIC_VAR, GENERIC_FORCES, GENERIC_CASES),
            'halo': (HALO_ENV, HALO_VAR, HALO_FORCES, HALO_CASES)}
SWITCHES = ('EVK_WINO', 'EVK_X3_HALO', 'EVK_X3_HALO_MIN_WG', 'EVK_C1_DMA', 'EVK_C1_PS2', 'EVK_C1_SP', 'EVK_X3_WS', 'EVK_TUNE',
            'EVK_X3_FORCE', 'EVK_X3_HALO_FORCE')


def halo_name(force, mode, packed=False, narrow=False):
    bn, ph, mw = HALO_FORCES[force]
    if narrow and bn == 128:          # 128-wide forms need Cd > 64
        bn, ph, mw = 64, 8, 4
    if mode != 'f16x2':               # eight matrix waves exist under f16x2 only
        mw = 4
    np_ = 4 if packed else ARITH[mode]
    return HALO_NAME.format(bn=bn, ph=ph, np=np_, dma='true' if mode == 'f16x2' else 'false', mw=mw)


def expected(family, case, force, mode, packed=False):
    """(forward name, [data-gradient name per residue class]) evk_conv2d_route must answer.  packed: the activation operand
    arrives packed (f16x2 only: NPX = 4)"""
    assert not packed or mode == 'f16x2'
    np_ = 4 if packed else ARITH[mode]
    classes = case['s'][0] * case['s'][1]
    if family == 'generic':
        name = GENERIC_FORCES[force].format(np=np_)
        return name, [name] * classes
    out = []
    for what in (case['fwd'], case['dgrad']):
        if what in ('every', 'narrow'):
            out.append(halo_name(force, mode, packed, narrow=what == 'narrow'))
        else:
            out.append(what.format(np=np_))
    return out[0], [out[1]] * classes


def desc_args(case, planes):
    """arguments of _C.ConvDesc for the descriptor the Python layer builds (every Cin / Cout here is a multiple of 4, and of 8
    under the split arithmetics: nothing is padded)"""
    assert case['cin'] % 4 == 0 and case['cout'] % 4 == 0 and (planes == 0 or (case['cin'] % 8 == 0 and case['cout'] % 8 == 0))
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = case['k'], case['s'], case['p'], case['dil']
    ho, wo = (case['h'] + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (case['w'] + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    return (case['n'], case['h'], case['w'], case['cin'], ho, wo, case['cout'], kh, kw, sh, sw, ph, pw, dh, dw)


def routed(lib, case, planes, packed=False, accum=0, stats=0):
    """(forward name, [data-gradient name per residue class]) from evk_conv2d_route under the current environment"""
    import ctypes
    from ever_amd import _C
    d = _C.ConvDesc(*desc_args(case, planes))
    out = []
    for cls in [-1] + list(range(d.stride_h * d.stride_w)):
        buf = ctypes.create_string_buffer(128)
        flags = (2 if cls < 0 else 4) if packed else 0
        rc = lib.evk_conv2d_route(ctypes.byref(d), cls, planes, flags, accum if cls >= 0 else 0, stats if cls < 0 else 0, 32, buf,
                                  len(buf), None)
        assert rc == 0, lib.evk_last_error()
        out.append(buf.value.decode())
    return out[0], out[1:]


# ---- the instantiations the table has to reach (none of them is reached by another fp64 comparison of the suite) ----------
REQUIRED = {
    # conv_igemm_x3ws_kernel: 3 tiles x NPX 1 (bf16), 2 (f16x2), 3 (bf16x3), 4 (f16x2, packed activations)
    'conv_igemm_x3ws_kernel<128, 256, 2, 2, 2, 1>', 'conv_igemm_x3ws_kernel<128, 256, 2, 2, 2, 2>',
    'conv_igemm_x3ws_kernel<128, 256, 2, 2, 2, 3>', 'conv_igemm_x3ws_kernel<128, 256, 2, 2, 2, 4>',
    'conv_igemm_x3ws_kernel<128, 128, 2, 2, 2, 1>', 'conv_igemm_x3ws_kernel<128, 128, 2, 2, 2, 2>',
    'conv_igemm_x3ws_kernel<128, 128, 2, 2, 2, 3>', 'conv_igemm_x3ws_kernel<128, 128, 2, 2, 2, 4>',
    'conv_igemm_x3ws_kernel<128, 64, 2, 2, 2, 1>', 'conv_igemm_x3ws_kernel<128, 64, 2, 2, 2, 2>',
    'conv_igemm_x3ws_kernel<128, 64, 2, 2, 2, 3>', 'conv_igemm_x3ws_kernel<128, 64, 2, 2, 2, 4>',
    # conv_igemm_x3_kernel: 128x128, 128x64, 64x128
    'conv_igemm_x3_kernel<128, 128, 2, 2, 1, 1>', 'conv_igemm_x3_kernel<128, 128, 2, 2, 1, 2>',
    'conv_igemm_x3_kernel<128, 128, 2, 2, 1, 3>', 'conv_igemm_x3_kernel<128, 128, 2, 2, 1, 4>',
    'conv_igemm_x3_kernel<128, 64, 2, 2, 1, 1>', 'conv_igemm_x3_kernel<128, 64, 2, 2, 1, 2>',
    'conv_igemm_x3_kernel<128, 64, 2, 2, 1, 3>', 'conv_igemm_x3_kernel<128, 64, 2, 2, 1, 4>',
    'conv_igemm_x3_kernel<64, 128, 2, 2, 1, 1>', 'conv_igemm_x3_kernel<64, 128, 2, 2, 1, 2>',
    'conv_igemm_x3_kernel<64, 128, 2, 2, 1, 3>', 'conv_igemm_x3_kernel<64, 128, 2, 2, 1, 4>',
    # conv3x3_halo_x3_kernel, f16x2: the eight forms (weights by DMA), fp32 and packed activations
    'conv3x3_halo_x3_kernel<64, 8, 2, true, 4>', 'conv3x3_halo_x3_kernel<64, 8, 2, true, 8>',
    'conv3x3_halo_x3_kernel<64, 16, 2, true, 4>', 'conv3x3_halo_x3_kernel<64, 16, 2, true, 8>',
    'conv3x3_halo_x3_kernel<128, 8, 2, true, 4>', 'conv3x3_halo_x3_kernel<128, 8, 2, true, 8>',
    'conv3x3_halo_x3_kernel<128, 16, 2, true, 4>', 'conv3x3_halo_x3_kernel<128, 16, 2, true, 8>',
    'conv3x3_halo_x3_kernel<64, 8, 4, true, 4>', 'conv3x3_halo_x3_kernel<64, 8, 4, true, 8>',
    'conv3x3_halo_x3_kernel<64, 16, 4, true, 4>', 'conv3x3_halo_x3_kernel<64, 16, 4, true, 8>',
    'conv3x3_halo_x3_kernel<128, 8, 4, true, 4>', 'conv3x3_halo_x3_kernel<128, 8, 4, true, 8>',
    'conv3x3_halo_x3_kernel<128, 16, 4, true, 4>', 'conv3x3_halo_x3_kernel<128, 16, 4, true, 8>',
    # ... bf16 and bf16x3: four matrix waves, weights through registers
    'conv3x3_halo_x3_kernel<64, 8, 1, false, 4>', 'conv3x3_halo_x3_kernel<64, 16, 1, false, 4>',
    'conv3x3_halo_x3_kernel<128, 8, 1, false, 4>', 'conv3x3_halo_x3_kernel<128, 16, 1, false, 4>',
    'conv3x3_halo_x3_kernel<64, 8, 3, false, 4>', 'conv3x3_halo_x3_kernel<64, 16, 3, false, 4>',
    'conv3x3_halo_x3_kernel<128, 8, 3, false, 4>', 'conv3x3_halo_x3_kernel<128, 16, 3, false, 4>',
    # conv_igemm_kernel (fp32)
    'conv_igemm_kernel<128, 128, 2, 2>', 'conv_igemm_kernel<128, 64, 2, 2>', 'conv_igemm_kernel<256, 64, 4, 1>',
}
# the smallest tiles, which the table reaches as well (the forces c64x64, and what a refused force falls back to)
ALSO_REACHED = {
    'conv_igemm_x3_kernel<64, 64, 2, 2, 1, 1>', 'conv_igemm_x3_kernel<64, 64, 2, 2, 1, 2>',
    'conv_igemm_x3_kernel<64, 64, 2, 2, 1, 3>', 'conv_igemm_x3_kernel<64, 64, 2, 2, 1, 4>',
    'conv_igemm_kernel<64, 64, 2, 2>',
}
assert len(REQUIRED) == 12 + 12 + 16 + 8 + 3 and not (REQUIRED & ALSO_REACHED)


def walk(lib, family):
    """Every (case, force, arithmetic, packed) of a family, in a process with the family's environment: asserts the table and
    returns the set of names.  The raw cases are walked with packed activations too (what tools/check_tiles.py launches)."""
    import os
    env, var, forces, cases = FAMILIES[family]
    assert all(os.environ.get(k) == v for k, v in env.items()), 'run in a process with the family environment'
    names, bad = set(), []
    for force in forces:
        os.environ[var] = force
        for case in cases:
            for mode, planes in ARITH.items():
                for packed in ((False, True) if (mode == 'f16x2' and case.get('raw')) else (False,)):
                    got = routed(lib, case, planes, packed)
                    want = expected(family, case, force, mode, packed)
                    if got != want:
                        bad.append((case['name'], force, mode, packed, got, want))
                    names.add(got[0])
                    names.update(got[1])
    os.environ[var] = ''
    assert not bad, f'{len(bad)} forced routes differ from the table, e.g. {bad[:3]}'
    return names


def walk_fp32(lib):
    names = set()
    for case, fwd, dgrad in FP32_CASES:
        got = routed(lib, case, 0)
        assert got == (fwd, [dgrad]), (case['name'], got, fwd, dgrad)
        names.update((fwd, dgrad))
    return names
