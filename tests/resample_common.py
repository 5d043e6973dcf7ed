"""What the bilinear tests share: the exported host plan (evk_upsample_bilinear_plan — the function the launchers call, no Python
copy of its predicates), aten's align_corners=True coordinate formula in numpy float32, and the table of GPU cases with the
kernel each one exists to reach.  tests/test_resample_plan_cpu.py asserts the table against the plan without a GPU, so that
an edit to a predicate cannot silently move a case of tests/test_resample_edges_gpu.py off its kernel."""
import ctypes

import numpy as np

SCALAR, VEC, TILE32, TILE64, WAVE = range(5)
KERNEL_NAMES = ('scalar element', 'vec element', 'tile-32', 'tile-64', 'wave')
TILE_R, TILE_C = 4, 16          # output pixels per workgroup of the tile kernels (csrc/resample.hip: kTileR, kTileC)
WAVE_CANDIDATES = 16            # candidate slots per axis of the wave kernel (lane & 15)
LDS_BYTES = 64 * 1024

_out = (ctypes.c_int32 * 8)()


def plan(lib, n, hi, wi, ho, wo, c, vec, backward):
    """(kernel, patch rows, patch cols, patch bytes, sy, sx, isy, isx); the four scales as np.float32"""
    rc = lib.evk_upsample_bilinear_plan(n, hi, wi, ho, wo, c, int(vec), int(backward), _out)
    assert rc == 0, ((n, hi, wi, ho, wo, c, vec, backward), lib.evk_last_error())
    f = np.array(_out[4:8], dtype=np.int32).view(np.float32)
    return (_out[0], _out[1], _out[2], _out[3], f[0], f[1], f[2], f[3])


def src_index(scale, size_in, size_out):
    """aten's upsample_bilinear2d, align_corners=True: src = scale * dst in float, i0 = (int)src, i1 = i0 + (i0 < in - 1).
    `scale` is the float32 the kernels receive.  Returns int arrays (i0, i1) over dst = 0 .. size_out - 1."""
    s = np.float32(scale) * np.arange(size_out, dtype=np.float32)
    assert s.dtype == np.float32
    i0 = np.minimum(s.astype(np.int64), size_in - 1)
    i1 = i0 + (i0 < size_in - 1)
    return i0, i1


def candidate_range(inv_scale, size_in, size_out):
    """The backward kernels' clamped candidate range of every input index, in their float32 arithmetic:
    floor((i - 1) * is) - 1 .. ceil((i + 1) * is) + 1.  Returns int arrays (lo, hi) over i = 0 .. size_in - 1."""
    i = np.arange(size_in, dtype=np.float32)
    inv = np.float32(inv_scale)
    lo = np.floor((i - np.float32(1)) * inv).astype(np.int64) - 1
    hi = np.ceil((i + np.float32(1)) * inv).astype(np.int64) + 1
    return np.maximum(lo, 0), np.minimum(hi, size_out - 1)


# (N, C, Hi, Wi, Ho, Wo, forward kernel, backward kernel); None = recorded by the plan test, not prescribed
CASES = (
    (2, 128, 19, 19, 17, 17, TILE32, WAVE),     # down-sampling, ragged tiles on both axes, input pixels no output reads
    (1, 128, 12, 20, 12, 20, TILE32, WAVE),     # equal size: a copy, bit for bit, both ways
    (2, 128, 3, 5, 11, 19, TILE32, WAVE),       # non-integer ratio, odd column count for the two-pixels-per-wave loop
    (1, 256, 5, 3, 10, 6, TILE64, WAVE),
    (1, 512, 4, 4, 8, 8, VEC, WAVE),            # the patch exceeds 64 KiB
    (1, 1024, 3, 3, 6, 6, VEC, WAVE),           # all four accumulators
    (1, 1024, 2, 2, 16, 16, TILE64, VEC),       # four channel passes; not narrow
    (1, 1028, 2, 2, 16, 16, TILE64, VEC),       # five channel passes, the last one partial; C > 1024
    (1, 1028, 3, 3, 6, 6, VEC, VEC),
    (1, 128, 3, 3, 12, 12, TILE32, None),       # 2 / scale + 5 sits on 16
    (1, 128, 3, 3, 13, 13, TILE32, VEC),        # 2 / scale + 5 is past 16
    (1, 128, 4, 2, 8, 16, TILE32, VEC),         # narrow on one axis only
    (1, 256, 1, 4, 3, 8, TILE64, VEC),          # sy = 0, Hi = 1
    (1, 128, 4, 4, 1, 1, TILE32, WAVE),         # only dx[0, 0] is non-zero
    (2, 4, 7, 9, 3, 20, VEC, VEC),
    (2, 6, 5, 7, 9, 4, SCALAR, SCALAR),
    (2, 1, 16, 16, 37, 23, SCALAR, SCALAR),
)
# slice calls: (index into CASES or an explicit dense case, c0, Ctot, forward kernel, backward kernel)
SLICE_CASES = (
    (CASES[0][:6], 4, 128 + 12, TILE32, WAVE),
    (CASES[2][:6], 4, 128 + 12, TILE32, WAVE),
    (CASES[3][:6], 4, 256 + 12, TILE64, WAVE),
    ((1, 8, 3, 5, 6, 9), 2, 11, SCALAR, SCALAR),   # c0 and Ctot off the 16-byte grid: must take the scalar kernel
)


def slice_vec(c, c0, ctot):
    """the alignment the slice entry points pass on (include/ever_hip.h: evk_upsample_bilinear_plan, `vec`)"""
    return c % 4 == 0 and c0 % 4 == 0 and ctot % 4 == 0


def case_id(case):
    n, c, hi, wi, ho, wo = case[:6]
    return f'{n}x{c}-{hi}x{wi}to{ho}x{wo}'
