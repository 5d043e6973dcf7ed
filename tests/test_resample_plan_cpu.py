"""The bilinear resampling plan (csrc/resample.hip: bilinear_plan), asked of the library on the host through
evk_upsample_bilinear_plan — the function bilinear_fwd_launch and bilinear_bwd_launch call, no Python copy of its predicates.

What the kernels take on trust from that plan, checked here with aten's coordinate formula in numpy float32 on the plan's own
scale bits (tests/resample_common.py):
  tile kernels   the input rows / columns one 4 x 16 output tile reads fit the planned patch, the patch fits 64 KiB of LDS,
                 the batch fits gridDim.z
  wave kernel    the clamped candidate range of every input index fits its 16 lanes, and (for the element kernels too, which
                 walk the same range) holds every output that reads that input
Sizes 1..200 against 1..260 on one axis at a time (the other axis fixed at 4 -> 8, which passes every predicate), each with
N in {1, 65535, 65536} and C in {4, 124, 128, 132, 256, 512, 1024, 1028} (and once per C without 16-byte alignment), forward and
backward."""
import ctypes

import numpy as np
import pytest

from ever_amd import _C
from tests.resample_common import (CASES, KERNEL_NAMES, LDS_BYTES, SCALAR, SLICE_CASES, TILE32, TILE64, TILE_C, TILE_R, VEC, WAVE,
                                   WAVE_CANDIDATES, candidate_range, case_id, plan, slice_vec, src_index)

BATCHES = (1, 65535, 65536)
CHANNELS = (4, 124, 128, 132, 256, 512, 1024, 1028)
FIXED_IN, FIXED_OUT = 4, 8


def _tile_spans(i0, i1, size_out, tile):
    """input extent i1(last) - i0(first) + 1 of every `tile` consecutive outputs (the last tile ragged)"""
    first = np.arange(0, size_out, tile)
    last = np.minimum(first + tile, size_out) - 1
    return i1[last] - i0[first] + 1


def _check_axis(size_in, size_out, scale, inv_scale, tile, patch_bound, wave_planned, what):
    i0, i1 = src_index(scale, size_in, size_out)
    assert (_tile_spans(i0, i1, size_out, tile) <= patch_bound).all(), ('patch', what, patch_bound)
    lo, hi = candidate_range(inv_scale, size_in, size_out)
    o = np.arange(size_out)
    for idx in (i0, i1):        # every output that reads input i lies in i's candidate range
        assert ((lo[idx] <= o) & (o <= hi[idx])).all(), ('candidates miss a reader', what)
    if wave_planned:
        assert (hi - lo + 1 <= WAVE_CANDIDATES).all(), ('candidates overflow the wave', what, int((hi - lo + 1).max()))


@pytest.mark.parametrize('axis', ['rows', 'cols'])
def test_plan_keeps_every_kernel_inside_its_patch_and_candidate_table(axis):
    lib = _C.load()
    fn = lib.evk_upsample_bilinear_plan
    out = (ctypes.c_int32 * 8)()
    combos = [(n, c, 1) for n in BATCHES for c in CHANNELS] + [(1, c, 0) for c in CHANNELS]
    seen = set()
    for size_in in range(1, 201):
        for size_out in range(1, 261):
            hi, ho, wi, wo = (size_in, size_out, FIXED_IN, FIXED_OUT) if axis == 'rows' else (FIXED_IN, FIXED_OUT, size_in, size_out)
            what = (axis, size_in, size_out)
            fwd_geo, bwd_geo, wave = set(), set(), False
            for n, c, vec in combos:
                assert fn(n, hi, wi, ho, wo, c, vec, 0, out) == 0, what
                k, prow, pcol, nbytes = out[0], out[1], out[2], out[3]
                fwd_geo.add((prow, pcol, out[4], out[5]))
                seen.add(k)
                assert nbytes == min(prow * pcol * c * 4, 2 ** 31 - 1), (what, n, c, 'patch bytes')
                if not vec:
                    assert k == SCALAR, (what, n, c, k)
                elif k in (TILE32, TILE64):
                    assert n <= 65535 and nbytes <= LDS_BYTES and c >= 128 and (k == TILE32) == (c <= 128), (what, n, c, k, nbytes)
                else:
                    assert k == VEC, (what, n, c, k)
                assert fn(n, hi, wi, ho, wo, c, vec, 1, out) == 0, what
                k = out[0]
                bwd_geo.add(tuple(out[4:8]))
                seen.add(k)
                if not vec:
                    assert k == SCALAR, (what, n, c, k)
                elif k == WAVE:
                    assert hi > 1 and wi > 1 and 128 <= c <= 1024, (what, n, c)
                    wave = True
                else:
                    assert k == VEC, (what, n, c, k)
            # the geometry is a function of the four sizes alone, and the backward gets the forward's scales
            assert len(fwd_geo) == 1 and len(bwd_geo) == 1, what
            prow, pcol, sy_bits, sx_bits = next(iter(fwd_geo))
            scales = np.array(next(iter(bwd_geo)), dtype=np.int32).view(np.float32)
            assert scales[:2].view(np.int32).tolist() == [sy_bits, sx_bits], what
            sy, sx, isy, isx = scales
            if axis == 'rows':
                _check_axis(hi, ho, sy, isy, TILE_R, prow, wave, what)
            else:
                _check_axis(wi, wo, sx, isx, TILE_C, pcol, wave, what)
            if size_in == 1 and size_out == 1:      # (the fixed axis, once)
                _check_axis(FIXED_IN, FIXED_OUT, sx if axis == 'rows' else sy, isx if axis == 'rows' else isy,
                            TILE_C if axis == 'rows' else TILE_R, pcol if axis == 'rows' else prow, True, (axis, 'fixed'))
    assert seen == {SCALAR, VEC, TILE32, TILE64, WAVE}      # the sweep reaches every kernel


def test_gpu_case_table_lands_on_the_kernels_it_names():
    """Every row of the GPU test's table, dense and slice, against the plan.  The one row the table leaves open,
    3 x 3 -> 12 x 12, sits ON the wave kernel's bound: scale = float(2 / 11) rounds UP, 1 / scale rounds to 5.5 exactly, so
    2 / scale + 5 == 16 in float and the wave kernel takes it (an exact 2 / 11 would give the same side: 16 <= 16)."""
    lib = _C.load()
    for n, c, hi, wi, ho, wo, want_f, want_b in CASES:
        f = plan(lib, n, hi, wi, ho, wo, c, c % 4 == 0, False)
        b = plan(lib, n, hi, wi, ho, wo, c, c % 4 == 0, True)
        print(f'{case_id((n, c, hi, wi, ho, wo))}: forward {KERNEL_NAMES[f[0]]} (patch {f[1]} x {f[2]}, {f[3]} bytes), '
              f'backward {KERNEL_NAMES[b[0]]} (2 / sy + 5 = {2 * b[6] + 5:.9g}, 2 / sx + 5 = {2 * b[7] + 5:.9g})')
        assert f[0] == want_f, (case_id((n, c, hi, wi, ho, wo)), 'forward', KERNEL_NAMES[f[0]], 'no longer', KERNEL_NAMES[want_f])
        if want_b is not None:
            assert b[0] == want_b, (case_id((n, c, hi, wi, ho, wo)), 'backward', KERNEL_NAMES[b[0]], 'no longer', KERNEL_NAMES[want_b])
        else:
            inv = np.float32(1) / (np.float32(hi - 1) / np.float32(ho - 1))
            assert b[6] == inv and b[7] == inv and np.float32(2) * inv + np.float32(5) == np.float32(16)
            assert b[0] == WAVE, KERNEL_NAMES[b[0]]
    for (n, c, hi, wi, ho, wo), c0, ctot, want_f, want_b in SLICE_CASES:
        vec = slice_vec(c, c0, ctot)
        assert plan(lib, n, hi, wi, ho, wo, c, vec, False)[0] == want_f, (c, c0, ctot)
        assert plan(lib, n, hi, wi, ho, wo, c, vec, True)[0] == want_b, (c, c0, ctot)
    # the notes of the table: what makes a row take the kernel it takes
    assert plan(lib, 1, 4, 4, 8, 8, 512, True, False)[3] > LDS_BYTES
    assert plan(lib, 1, 4, 4, 8, 8, 256, True, False)[3] <= LDS_BYTES
    assert plan(lib, 1, 3, 3, 6, 6, 1024, True, False)[3] > LDS_BYTES
    assert plan(lib, 1, 2, 2, 16, 16, 1028, True, False)[3] <= LDS_BYTES
    assert plan(lib, 1, 1, 4, 3, 8, 256, True, True)[4] == 0 and plan(lib, 1, 1, 4, 3, 8, 256, True, True)[6] == 3
    assert plan(lib, 1, 4, 4, 1, 1, 128, True, True)[4:] == (0, 0, 1, 1)


def test_plan_refuses_bad_arguments():
    lib = _C.load()
    out = (ctypes.c_int32 * 8)()
    assert lib.evk_upsample_bilinear_plan(1, 4, 4, 8, 8, 128, 1, 0, None) == -1
    for bad in ((0, 4, 4, 8, 8, 128, 1), (1, 0, 4, 8, 8, 128, 1), (1, 4, 4, 8, 0, 128, 1), (1, 4, 4, 8, 8, 0, 0),
                (1, 4, 4, 8, 8, 6, 1)):      # (16-byte accesses on C % 4 != 0)
        assert lib.evk_upsample_bilinear_plan(*bad, 0, out) == -1, bad
        assert lib.evk_upsample_bilinear_plan(*bad, 1, out) == -1, bad
