"""Properties of the GroupNorm reduce plan (csrc/groupnorm.hip: gn_plan), asked of the library on the host through evk_gn_plan —
the same function the launchers call, no Python copy: no chunk without rows, no row without a chunk, a chunk's rows a whole
number of thread-rows, the 256-chunk cap, the thread shape inside one workgroup, and a workspace that is exactly the partial
records plus the group coefficients."""
import ctypes

import numpy as np

from ever_amd import _C

CHANNELS = list(range(4, 2049 + 4, 4)) + [4096]       # (2052 is the last of the range)
PER, CAP = 65536, 256                                   # elements a chunk aims at, chunks at most


def _hw_for(c):
    hw = set(range(1, 601))
    for e in range(25):
        hw.update((2 ** e - 1, 2 ** e, 2 ** e + 1))
    for k in (1, 2, CAP - 1, CAP, CAP + 1):            # HW * C straddles k chunks' worth
        r = k * PER // c
        hw.update((r - 1, r, r + 1, r + 2))
    return sorted(r for r in hw if r >= 1)


def _plans(lib):
    out = (ctypes.c_int32 * 4)()
    fn = lib.evk_gn_plan
    table = []
    for c in CHANNELS:
        for hw in _hw_for(c):
            assert fn(hw, c, out) == 0, (hw, c, lib.evk_last_error())
            table.append((hw, c) + tuple(out))
    return np.array(table, dtype=np.int64)


def test_plan_covers_every_row_once_and_sizes_the_workspace():
    lib = _C.load()
    assert 2052 in CHANNELS and 4096 in CHANNELS
    t = _plans(lib)
    assert len(t) > 300000
    hw, c, nchunk, rpc, tpc, rl = t.T

    def bad(cond, what):
        i = np.flatnonzero(~cond)
        assert i.size == 0, (what, [tuple(int(v) for v in t[j]) for j in i[:5]])

    bad((nchunk >= 1) & (nchunk <= CAP), '1 <= nchunk <= 256')
    bad(rpc % rl == 0, 'rows_per_chunk % rl')
    bad(((nchunk - 1) * rpc < hw) & (hw <= nchunk * rpc), 'cover: no empty chunk, no uncovered row')
    bad(tpc == np.minimum(c // 4, 256), 'tpc == min(C / 4, 256)')
    bad((rl >= 1) & (tpc * rl <= 256), 'tpc * rl <= 256')
    # the regimes tests/test_groupnorm_edges_gpu.py launches exist in the plan
    assert (nchunk == 1).any() and nchunk.max() > 250 and (256 % tpc != 0).any() and (c // 4 > tpc).any()
    assert ((nchunk > 1) & (nchunk * rpc > hw)).any()
    # the workspace: [N][nchunk][2][C] partial sums, then 2 N G coefficients
    ws = lib.evk_gn_workspace_bytes
    for k, row in enumerate(t.tolist()):
        h, cc, nc = row[:3]
        n, g = ((1, 1), (3, cc // 4), (2, cc))[k % 3]
        assert ws(n, h, cc, g) == (n * nc * 2 * cc + 2 * n * g) * 4, (n, h, cc, g, nc)


def test_plan_refuses_what_the_launchers_refuse():
    lib = _C.load()
    out = (ctypes.c_int32 * 4)()
    for hw, c, rc in ((0, 64, -1), (-5, 64, -1), (16, 0, -1), (16, -4, -1), (16, 6, -2), (16, 2050, -2)):
        assert lib.evk_gn_plan(hw, c, out) == rc, (hw, c)
    assert lib.evk_gn_plan(16, 64, None) == -1
    assert b'gn_plan' in lib.evk_last_error()
    assert lib.evk_gn_plan(2 ** 36, 2048, out) == 0 and out[0] == 256 and out[1] == 2 ** 28      # (64-bit rows)
