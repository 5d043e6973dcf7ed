"""The planner of the forward / data-gradient convolutions (csrc/conv_route.hpp), asked through evk_conv2d_route on the host.

tests/golden/conv_routes.json is a kernel trace of the commit BEFORE the planner existed (tools/record_conv_routes.py on a
256-CU MI355X; the file names the commit): per shape the launches of every case under the default switches, and the ones
that differ under each other switch setting.  The planner must name the same instantiation for every one of them."""
import ctypes
import json
import math
import os
import subprocess
import sys

import pytest

from ever_amd import _C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, 'tests', 'golden', 'conv_routes.json')) as f:
    GOLDEN = json.load(f)
PLANES = {'fp32': 0, 'bf16': 1, 'f16x2': 2, 'bf16x3': 3}
SWITCHES = ('EVK_WINO', 'EVK_X3_HALO', 'EVK_X3_HALO_MIN_WG', 'EVK_C1_DMA', 'EVK_C1_PS2', 'EVK_C1_SP', 'EVK_X3_WS', 'EVK_TUNE')


def route(lib, d, cls, planes, packed=0, accum=0, stats=0, cus_per_xcd=32):
    """(kernel name, plane layout) of one launch; ('', 0) for a residue class without one"""
    buf = ctypes.create_string_buffer(128)
    layout = ctypes.c_int32(-1)
    flags = (2 if cls < 0 else 4) if packed else 0
    rc = lib.evk_conv2d_route(ctypes.byref(d), cls, planes, flags, accum, stats, cus_per_xcd, buf, len(buf), ctypes.byref(layout))
    assert rc == 0, lib.evk_last_error()
    return buf.value.decode(), layout.value


def check_setting(setting):
    """runs in a process that has the setting's switches in its environment (they are read once)"""
    lib = _C.load()
    bad, n = [], 0
    for desc, case_set, launches, diff in GOLDEN['shapes']:
        d = _C.ConvDesc(*desc)
        for pos, ci in enumerate(GOLDEN['case_sets'][case_set]):
            arith, direction, packed, stats, accum = GOLDEN['cases'][ci]
            want = [GOLDEN['kernels'][k] for k, _grid in diff.get(setting, {}).get(str(pos), launches[pos])]
            classes = [-1] if direction == 'fwd' else range(d.stride_h * d.stride_w)
            got = [route(lib, d, c, PLANES[arith], packed, accum, stats, GOLDEN['compute_units'] // 8)[0] for c in classes]
            if [g for g in got if g] != want:
                bad.append((desc, arith, direction, packed, stats, accum, want, got))
            n += 1
    assert not bad, f'{setting}: {len(bad)} of {n} cases route differently, e.g. {bad[:3]}'
    return n


@pytest.mark.parametrize('setting', ['default', 'wino2_minwg0', 'wino0', 'halo0', 'dma0', 'dma2', 'ps2_2', 'ws0', 'ws2'])
def test_routes_match_the_recorded_kernel_trace(setting):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(GOLDEN['settings'][setting])
    code = f'import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, "tests")!r}]; ' \
           f'import test_conv_route_cpu as t; print("cases", t.check_setting({setting!r}))'
    p = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert 'cases 5225' in p.stdout


def _jobs(lib, d, for_dgrad):
    n = lib.evk_conv2d_split_job_count(ctypes.byref(d), for_dgrad)
    arr = (_C.SplitJob * max(n, 1))()
    got = lib.evk_conv2d_split_jobs(ctypes.byref(d), 4096, for_dgrad, 1 << 20, arr, n)
    assert 0 <= got <= n
    return [arr[i] for i in range(got)], arr


def _conv3(n, h, w, cin, cout):
    return _C.ConvDesc(n, h, w, cin, h, w, cout, 3, 3, 1, 1, 1, 1, 1, 1)


def plane_bytes(layout, rows, k):
    """bytes the producer writes for a 3x3 stride-1 layer: generic [3][rows][Kpad32(9 k)]; halo 3 planes x 9 taps and Winograd
    2 planes x 12 taps of [chunks of 16][rows][16] (split_weight.hpp)"""
    ch = (k + 15) // 16 * 16
    taps = {0: 3 * ((9 * k + 31) // 32 * 32), 1: 3 * 9 * ch, 2: 2 * 12 * ch}[layout]
    return taps * rows * 2


def test_producers_and_launches_agree_on_the_plane_layout():
    """The layout evk_conv2d_split_jobs lays the planes out in (kind, arg[3]) is the layout of the kernel evk_conv2d_route names,
    forward and stride-1 data gradient, in every split arithmetic; evk_conv2d_split_weight_bytes covers it.  Inputs of 2 GiB and
    more: the Winograd kernel loads its halo through a buffer descriptor (32-bit byte offsets) and cannot take them — the halo
    layout AND the halo kernel, stated outright."""
    lib = _C.load()
    grid = [_conv3(n, s, s, ci, co) for n in (1, 2, 16) for s in (8, 16, 32, 64, 128) for ci, co in ((64, 64), (256, 256), (256, 128), (200, 96), (128, 200))]
    grid += [_conv3(1, 616, 344, 96, 96), _conv3(8, 136, 128, 256, 256), _conv3(1, 1448, 1448, 256, 256), _conv3(31, 256, 256, 256, 256)]
    huge = [_conv3(1, 1450, 1450, 256, 256), _conv3(32, 256, 256, 256, 256)]
    seen = set()
    for d in grid + huge:
        for for_dgrad in (0, 1):
            jobs, _keep = _jobs(lib, d, for_dgrad)
            assert len(jobs) == 1
            rows, k = (d.Cin, d.Cout) if for_dgrad else (d.Cout, d.Cin)
            for planes in (1, 2, 3):
                for packed in ((0, 1) if planes == 2 else (0,)):
                    name, layout = route(lib, d, 0 if for_dgrad else -1, planes, packed)
                    want = 0 if jobs[0].kind != 2 else (2 if planes == 2 and jobs[0].arg[3] else 1)
                    assert layout == want, (tuple(getattr(d, f) for f, _ in d._fields_), for_dgrad, planes, name, layout, want)
                    assert name.startswith({0: 'conv_igemm_x3', 1: 'conv3x3_halo_x3_kernel', 2: 'conv3x3_wino_x3_kernel'}[layout]), name
                    assert lib.evk_conv2d_split_weight_bytes(ctypes.byref(d), for_dgrad) >= plane_bytes(layout, rows, k)
                    seen.add(layout)
    assert seen == {0, 1, 2}
    for d in huge:
        assert d.N * d.H * d.W * d.Cin * 4 >= 2 ** 31
        for for_dgrad in (0, 1):
            jobs, _keep = _jobs(lib, d, for_dgrad)
            assert jobs[0].kind == 2 and jobs[0].arg[3] == 0
            for packed in (0, 1):
                name, layout = route(lib, d, 0 if for_dgrad else -1, 2, packed)
                assert layout == 1 and name == f'conv3x3_halo_x3_kernel<128, 16, {4 if packed else 2}, true, 8>', name
    # just below 2 GiB the same layers take the Winograd kernel and its planes
    for d in (_conv3(1, 1448, 1448, 256, 256), _conv3(31, 256, 256, 256, 256)):
        assert route(lib, d, -1, 2)[1] == 2 and _jobs(lib, d, 0)[0][0].arg[3] == 1


def test_route_entry_point_checks_its_arguments():
    lib = _C.load()
    d = _C.ConvDesc(2, 32, 32, 64, 16, 16, 128, 3, 3, 2, 2, 1, 1, 1, 1)
    buf = ctypes.create_string_buffer(128)
    assert lib.evk_conv2d_route(None, -1, 2, 0, 0, 0, 32, buf, len(buf), None) == -1
    assert lib.evk_conv2d_route(ctypes.byref(d), 4, 2, 0, 0, 0, 32, buf, len(buf), None) == -1   # classes 0..3
    assert lib.evk_conv2d_route(ctypes.byref(d), -1, 7, 0, 0, 0, 32, buf, len(buf), None) == -1
    assert [route(lib, d, c, 3)[0] != '' for c in range(4)] == [True] * 4
    # 1x1 stride 2: only residue class (0, 0) has a tap
    d = _C.ConvDesc(16, 128, 128, 256, 64, 64, 512, 1, 1, 2, 2, 0, 0, 1, 1)
    assert [route(lib, d, c, 2)[0] != '' for c in range(4)] == [True, False, False, False]


def test_empty_residue_classes_are_exactly_those_no_tap_reaches():
    """Data gradient of a strided (and dilated) convolution: input position i = c + j * stride receives output o through tap k
    iff i + pad == o * stride + k * dil.  evk_conv2d_route answers "no launch" for the residue class (cy, cx) exactly when brute
    force over the map finds no such (i, k, o) on one of the two axes — strides 1..4, dilations 1..6, kernels 1..7, paddings
    0..2 dil, a different combination on each axis (the gcd(dil, stride) > 1 branch of plan_axis included)."""
    lib = _C.load()
    size = 64
    axes = [(s, dil, k, pad) for s in range(1, 5) for dil in range(1, 7) for k in range(1, 8) for pad in range(0, 2 * dil + 1)]

    def reached(c, s, dil, k, pad):
        out = (size + 2 * pad - dil * (k - 1) - 1) // s + 1
        return any((i + pad - t * dil) % s == 0 and 0 <= (i + pad - t * dil) // s < out for i in range(c, size, s) for t in range(k))

    n_empty = n_gcd = n = 0
    for j, (sh, dh, kh, ph) in enumerate(axes):
        sw, dw, kw, pw = axes[(j * 577 + 131) % len(axes)]     # (577 is coprime to the list's length: every combination on both axes)
        ho, wo = (size + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (size + 2 * pw - dw * (kw - 1) - 1) // sw + 1
        d = _C.ConvDesc(1, size, size, 64, ho, wo, 64, kh, kw, sh, sw, ph, pw, dh, dw)
        for cy in range(sh):
            for cx in range(sw):
                want = reached(cy, sh, dh, kh, ph) and reached(cx, sw, dw, kw, pw)
                got = route(lib, d, cy * sw + cx, 3)[0] != ''
                assert got == want, ((sh, dh, kh, ph), (sw, dw, kw, pw), (cy, cx), got, want)
                n += 1
                n_empty += not want
                n_gcd += (not want) and ((cy + ph) % math.gcd(dh, sh) != 0 or (cx + pw) % math.gcd(dw, sw) != 0)
    assert len({a for a in axes}) == len(axes) and math.gcd(577, len(axes)) == 1
    assert n > 8000 and n_empty > 1000 and n_gcd > 1000, (n, n_empty, n_gcd)
