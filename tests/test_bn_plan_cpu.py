"""Properties of the BatchNorm reduce plan (csrc/bn_common.hpp: bn_plan), asked of the library on the host through evk_bn_plan — the
same function the launchers call, no Python copy: no workgroup without rows, no row without a workgroup, a workgroup's rows a
whole number of thread-rows, the caps, the same for the pool backward's quads, and a workspace that holds all of it."""
import ctypes

import numpy as np

from ever_amd import _C

CHANNELS = list(range(4, 2049, 4))
PLAIN, POOL = 0, 1
PER = {PLAIN: 32768, POOL: 65536}       # elements a workgroup aims at
CAP = {PLAIN: 512, POOL: 2048}          # workgroups at most


def _rows_for(c):
    rows = set(range(1, 601))
    for e in range(25):
        rows.update((2 ** e - 1, 2 ** e, 2 ** e + 1))
    for kind in (PLAIN, POOL):          # the products that straddle one workgroup's worth and the cap
        for k in (1, 2, CAP[kind] - 1, CAP[kind], CAP[kind] + 1):
            r = k * PER[kind] // c
            rows.update((r - 1, r, r + 1, r + 2))
    for k in (1, 2, CAP[POOL] - 1, CAP[POOL], CAP[POOL] + 1):     # (the same for maps with quads)
        rows.update(4 * (k * PER[POOL] // c // 4 + d) for d in (-1, 0, 1))
    return sorted(r for r in rows if r >= 1)


def _plans(lib, kind):
    out = (ctypes.c_int32 * 6)()
    fn = lib.evk_bn_plan
    table = []
    for c in CHANNELS:
        for r in _rows_for(c):
            assert fn(r, c, kind, out) == 0, (r, c, kind, lib.evk_last_error())
            table.append((r, c) + tuple(out))
    return np.array(table, dtype=np.int64)


def _check(t, kind, lib):
    rows, c, nblk, rpb, tpc, rl, qn, qpb = t.T

    def bad(cond, what):
        i = np.flatnonzero(~cond)
        assert i.size == 0, (what, kind, [tuple(int(v) for v in t[j]) for j in i[:5]])

    bad((tpc >= 1) & (rl >= 1) & (tpc * rl <= 256), 'tpc * rl <= 256')
    bad((tpc <= c // 4) & ((tpc == c // 4) | (tpc == 256)), 'tpc is C / 4 up to the workgroup')
    bad(rpb % rl == 0, 'rows_per_blk % rl')
    bad(((nblk - 1) * rpb < rows) & (rows <= nblk * rpb), 'cover: no empty workgroup, no uncovered row')
    bad((nblk >= 1) & (nblk <= CAP[kind]), 'cap')
    has_q = (rows % 4 == 0) & (kind == POOL)
    bad(np.where(has_q, qpb >= 1, (qn == 0) & (qpb == 0)), 'quads only for the pool plan of rows % 4 == 0')
    q = rows // 4
    qs = np.maximum(qpb, 1)
    bad(np.where(has_q, (qpb % rl == 0) & ((qn - 1) * qs < q) & (q <= qn * qs) & (qn <= CAP[POOL]), True), 'quad cover')
    # the workspace (csrc/bn_common.hpp: BnWorkspace): partial records [nblk][2][C], 8 C coefficients, records of maxima
    # [nblk][2][C] (packed dx)
    need = (2 * np.maximum(nblk, qn) * 2 * c + 8 * c) * 4
    for cc in np.unique(c):
        m = c == cc
        have = lib.evk_bn_workspace_bytes(int(rows[m].max()), int(cc))
        assert have == lib.evk_bn_workspace_bytes(1, int(cc))         # (one size per channel count)
        assert (need[m] <= have).all(), ('workspace', kind, int(cc), int(need[m].max()), have)


def test_plan_covers_every_row_once_and_fits_the_workspace():
    lib = _C.load()
    for kind in (PLAIN, POOL):
        t = _plans(lib, kind)
        assert len(t) > 300000 and (kind == PLAIN or (t[:, 6] > 1).sum() > 20000)
        _check(t, kind, lib)
        if kind == PLAIN:       # the edges tests/test_bn_gpu.py launches exist in the plan
            nblk = t[:, 2]
            assert nblk.max() == 512 and (nblk == 1).any() and (t[:, 5] == 64).any() and (t[:, 4] == 256).any()


def test_plan_refuses_what_the_launchers_refuse():
    lib = _C.load()
    out = (ctypes.c_int32 * 6)()
    for rows, c, kind in ((0, 64, 0), (16, 6, 0), (16, 2052, 0), (16, 0, 1), (16, 64, 3), (2 ** 31, 4, 1)):
        assert lib.evk_bn_plan(rows, c, kind, out) == -2, (rows, c, kind)
    assert lib.evk_bn_plan(16, 64, 0, None) == -1
    for nparts, want in ((1, (8, 8, 32)), (511, (8, 8, 32)), (512, (32, 2, 128)), (1023, (32, 2, 128)), (1024, (64, 1, 256))):
        assert lib.evk_bn_plan(nparts, 64, 2, out) == 0 and (out[0], out[2], out[3]) == want, (nparts, tuple(out))
    assert lib.evk_bn_plan(2 ** 36, 2048, 0, out) == 0 and out[0] == 512      # (64-bit rows: the plain plan)
