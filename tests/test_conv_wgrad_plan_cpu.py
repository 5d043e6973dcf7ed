"""The planner of the weight-gradient convolutions (route_wgrad / plan_wgrad in csrc/conv_wgrad.hip), asked through
evk_conv2d_wgrad_route on the host: properties every plan must have — no empty split, no uncovered pixel, tiles that cover the
weight, a workspace that holds the partials of EVERY flag combination (the shared plan included) — over a wide grid of
descriptors, and the names held to a record that is not this code (profiles/r06_kernel_stats.csv)."""
import csv
import ctypes
import itertools
import json
import os
import re

from ever_amd import _C
from tests.wgrad_plan_common import (DY_PACKED, PLANAR, SHARED, X_PACKED, X_PLANAR, below_2gib, colsum_blocks, combos, conv_desc,
                                     fields, nine_tap, wgrad_route)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def grid_descs():
    maps = [(1, 1), (2, 3), (7, 7), (8, 8), (13, 13), (16, 16), (24, 40), (31, 17), (32, 32), (37, 29), (36, 32), (64, 96),
            (64, 64), (128, 128), (127, 128)]
    chans = [(4, 4), (8, 520), (64, 64), (64, 128), (72, 96), (128, 136), (200, 64), (256, 256), (520, 4), (256, 200), (192, 192)]
    geoms = [(1, 1, 1)] + [(kh, kw, dil) for kh, kw in ((3, 3), (7, 7), (1, 3)) for dil in (1, 2, 6, 18)]
    for (h, w), (cin, cout), (kh, kw, dil), s, n in itertools.product(maps, chans, geoms, (1, 2), (1, 2, 3, 16)):
        if kh == 7 and (dil > 2 or cin > 256):
            continue
        d = conv_desc(n, h, w, cin, cout, kh, kw, s, s, None, None, dil, dil)
        if d is not None:
            yield d
    # the 2 GiB boundary shapes of test_conv_route_cpu.py: just below, at and above
    for n, s in ((1, 1448), (31, 256), (1, 1450), (32, 256)):
        yield conv_desc(n, s, s, 256, 256, 3, 3)
        yield conv_desc(n, s, s, 256, 256, 1, 1)


def test_plan_properties_hold_over_the_grid():
    lib = _C.load()
    seen, n_plans = set(), 0
    for d in grid_descs():
        m, ktot = d.N * d.Ho * d.Wo, d.kh * d.kw * d.Cin
        ws = {0: lib.evk_conv2d_wgrad_workspace_bytes(ctypes.byref(d)), 1: lib.evk_conv2d_wgrad_x3_workspace_bytes(ctypes.byref(d))}
        for planes, flags in combos(d):
            rc, name, (bm, bn, tco, tk, sk, chunk) = wgrad_route(lib, d, planes, flags)
            what = (fields(d), planes, flags, name, (bm, bn, tco, tk, sk, chunk))
            assert rc == 0, (what, lib.evk_last_error())
            n_plans += 1
            # the split: whole steps of 32 pixels, no empty split, no uncovered pixel
            assert chunk % 32 == 0 and chunk > 0 and sk >= 1, what
            assert (sk - 1) * chunk < m <= sk * chunk, what
            # the tiles cover the weight; the grid is a 31-bit number
            assert tco * bm >= d.Cout and (tco - 1) * bm < d.Cout, what
            if name == 'conv_wgrad_tr_kernel<9>':
                assert tk * 64 == d.Cin and bn == 9 * 64, what
            else:
                assert tk * bn >= ktot and (tk - 1) * bn < ktot, what
            assert tco * tk * sk < 2 ** 31, what
            # the workspace the caller is told to bring holds this plan's partials and the bias gradient's
            wsb = ws[1 if planes else 0]
            if sk > 1:
                assert wsb >= sk * d.Cout * ktot * 4, what
            assert wsb >= colsum_blocks(m) * d.Cout * 4, what
            # the name says what was asked for
            fam = re.match(r'(\w+)<(.*)>$', name)
            args = [a.strip() for a in fam.group(2).split(',')]
            if planes == 0:
                assert fam.group(1) == 'conv_wgrad_kernel' and args == [str(bm), str(bn), '2', '2'], what
                assert (bm, bn) == (64 if d.Cout <= 64 else 128, 64 if ktot <= 64 else 128), what
            elif flags & PLANAR:
                assert name == f'conv_wgrad_tr_kernel<{9 if nine_tap(d) else 1}>' and bm == 128, what
            elif fam.group(1) == 'conv_wgrad_x3ws_kernel':
                tf = {True: 'true', False: 'false'}
                assert args == ['128', '256', str(planes), tf[d.Wo % 8 == 0], tf[bool(flags & X_PACKED)], tf[bool(flags & DY_PACKED)]], what
                assert (bm, bn) == (128, 256) and d.Cout >= 128 and ktot >= 256, what
            else:
                npx = 4 if flags & (X_PACKED | DY_PACKED) else planes
                assert fam.group(1) == 'conv_wgrad_x3_kernel' and args == [str(bm), str(bn), '2', '2', str(npx)], what
                assert (bm, bn) == (64 if d.Cout <= 64 else 128, 64 if ktot <= 64 else 128), what
            # raw buffer loads (32-bit byte offsets): the wide-tile kernels only below 2 GiB per tensor
            if fam.group(1) in ('conv_wgrad_x3ws_kernel', 'conv_wgrad_tr_kernel'):
                assert below_2gib(d), what
            elif planes and d.Cout >= 128 and ktot >= 256:
                assert not below_2gib(d), what
            seen.add(name)
    assert n_plans > 100000
    # all 34 instantiations occurred: 4 fp32 tiles, 4 tiles x 4 operand forms, x3ws W8 x (bf16, bf16x3, f16x2 x 4 packings), 2 planar
    assert len(seen) == 34, sorted(seen)


def test_shared_plan_differs_and_still_fits_the_workspace():
    """EVK_CONV_WGRAD_SHARED changes the split of the wide-tile kernels only, never to more splits than the unshared plan"""
    lib = _C.load()
    differs = set()
    for d in grid_descs():
        for planes, flags in combos(d):
            if flags & SHARED:
                continue
            _, name, plan = wgrad_route(lib, d, planes, flags)
            if planes != 2:
                continue
            _, name_sh, plan_sh = wgrad_route(lib, d, planes, flags | SHARED)
            assert name_sh == name and plan_sh[:4] == plan[:4], (fields(d), flags, name, name_sh)
            assert plan_sh[4] <= plan[4], (fields(d), flags, plan, plan_sh)
            if plan_sh != plan:
                assert name.startswith(('conv_wgrad_x3ws_kernel', 'conv_wgrad_tr_kernel')), (fields(d), flags, name)
                differs.add(name.split('<')[0] + ('<9>' if name.endswith('<9>') else ''))
    assert differs == {'conv_wgrad_x3ws_kernel', 'conv_wgrad_tr_kernel', 'conv_wgrad_tr_kernel<9>'}


def test_names_match_the_recorded_profile():
    """Every conv_wgrad* instantiation in the recorded training step's kernel statistics is what the entry point answers for a
    layer of that step (tests/golden/conv_routes.json is its layer set) under some operand form of the f16x2 arithmetic."""
    lib = _C.load()
    with open(os.path.join(ROOT, 'profiles', 'r06_kernel_stats.csv')) as f:
        recorded = {m.group(1) for row in csv.reader(f) for m in [re.search(r'evk::(conv_wgrad\w*_kernel<[^>]*>)', row[0])] if m}
    assert len(recorded) == 10, sorted(recorded)
    with open(os.path.join(ROOT, 'tests', 'golden', 'conv_routes.json')) as f:
        shapes = [tuple(s[0]) for s in json.load(f)['shapes']]
    # the scene-embedding convolution (2048 -> 256 on the pooled 1 x 1 map) is the step's only layer with Wo % 8 != 0
    scene = (16, 1, 1, 2048, 1, 1, 256, 1, 1, 1, 1, 0, 0, 1, 1)
    answered = {}
    for desc in shapes + [scene]:
        d = _C.ConvDesc(*desc)
        if d.Cin % 4 or d.Cout % 4:
            continue
        for planes, flags in combos(d):
            if planes == 2:
                rc, name, _ = wgrad_route(lib, d, planes, flags)
                assert rc == 0
                answered.setdefault(name, desc)
    assert recorded <= set(answered), sorted(recorded - set(answered))
    assert answered['conv_wgrad_x3ws_kernel<128, 256, 2, false, false, false>'][1:3] == (1, 1)


def test_wgrad_route_checks_its_arguments():
    lib = _C.load()
    d = _C.ConvDesc(2, 32, 32, 64, 32, 32, 128, 3, 3, 1, 1, 1, 1, 1, 1)
    buf = ctypes.create_string_buffer(128)
    plan = (ctypes.c_int32 * 6)()
    ok = lambda *a: lib.evk_conv2d_wgrad_route(*a)   # noqa: E731
    assert ok(ctypes.byref(d), 2, 0, buf, len(buf), None) == 0 and buf.value.startswith(b'conv_wgrad_x3ws_kernel<')
    assert ok(None, 2, 0, buf, len(buf), plan) == -1
    assert ok(ctypes.byref(d), 2, 0, None, 0, plan) == -1
    assert ok(ctypes.byref(d), 4, 0, buf, len(buf), plan) == -1 and ok(ctypes.byref(d), -1, 0, buf, len(buf), plan) == -1
    assert ok(ctypes.byref(d), 2, 64, buf, len(buf), plan) == -1                       # unknown flag
    assert ok(ctypes.byref(d), 3, X_PACKED, buf, len(buf), plan) == -1                 # flags belong to f16x2
    assert ok(ctypes.byref(d), 2, X_PLANAR, buf, len(buf), plan) == -2                 # planar without its pair
    assert b'pairs' in lib.evk_last_error()
    assert ok(ctypes.byref(d), 2, PLANAR, buf, len(buf), plan) == 0 and buf.value == b'conv_wgrad_tr_kernel<9>'
    for bad, word in ((_C.ConvDesc(2, 32, 32, 48, 32, 32, 128, 3, 3, 1, 1, 1, 1, 1, 1), b'Cin=48'),      # Cin % 64
                      (_C.ConvDesc(2, 32, 32, 64, 32, 32, 96, 3, 3, 1, 1, 1, 1, 1, 1), b'Cout=96'),      # Cout % 64
                      (_C.ConvDesc(2, 13, 13, 64, 13, 13, 128, 3, 3, 1, 1, 1, 1, 1, 1), b'Wo=13')):      # Wo % 8
        assert ok(ctypes.byref(bad), 2, PLANAR, buf, len(buf), plan) == -2
        assert word in lib.evk_last_error() and b'Wo % 8' in lib.evk_last_error()
        assert ok(ctypes.byref(bad), 2, X_PACKED | DY_PACKED, buf, len(buf), plan) == 0
    assert ok(ctypes.byref(_C.ConvDesc(1, 8, 8, 6, 8, 8, 8, 1, 1, 1, 1, 0, 0, 1, 1)), 0, 0, buf, len(buf), plan) == -2   # Cin % 4
    assert ok(ctypes.byref(_C.ConvDesc(1, 8, 8, 8, 8, 8, 8, 1, 1, 0, 1, 0, 0, 1, 1)), 0, 0, buf, len(buf), plan) == -1   # stride 0
    huge = _C.ConvDesc(64, 512, 512, 128, 512, 512, 128, 1, 1, 1, 1, 0, 0, 1, 1)                                     # 2^31 elements
    assert ok(ctypes.byref(huge), 2, 0, buf, len(buf), plan) == -2
