"""What the test-time-augmentation tests share: the exported host plan of the dihedral kernels (evk_d4_plan — the function the
launchers call, no Python copy of its predicates), the eight ops as torch expressions, the table of GPU cases with the kernel
each one exists to reach (tests/test_transform_cpu.py asserts the table against the plan without a GPU, so that a moved
threshold cannot silently take a case of tests/test_d4_gpu.py off its kernel), the toy model and the transform sets of the
fixture tests/golden/tta_ref.npz (written by tools/gen_golden_tta.py from the reference's own tta)."""
import contextlib
import ctypes
import os

import torch

SCALAR, VEC, TILE = range(3)
KERNEL_NAMES = ('scalar element', 'vec element', 'LDS tile')
MAX_TERMS = 16                      # per evk_d4_merge launch
INVERSE = (0, 1, 2, 5, 4, 3, 6, 7)  # the op that undoes each op
SWAP_OPS, PLAIN_OPS = (1, 3, 5, 7), (0, 2, 4, 6)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tta_ref.npz')

_out = (ctypes.c_int32 * 6)()


def plan(lib, n, h, w, c, op):
    """(kernel, tile rows, tile cols, LDS row stride in floats, LDS bytes, elements per thread)"""
    rc = lib.evk_d4_plan(n, h, w, c, op, _out)
    assert rc == 0, ((n, h, w, c, op), lib.evk_last_error())
    return tuple(_out)


@contextlib.contextmanager
def forced(lib, kernel):
    """evk_d4_force_kernel for the length of the block: the plan names `kernel` wherever it is legal"""
    before = lib.evk_d4_force_kernel(kernel)
    try:
        yield
    finally:
        lib.evk_d4_force_kernel(before)


def d4_ref(x, op):
    """op = swap | flip_rows << 1 | flip_cols << 2 (transpose first, then flip) on the last two axes of NCHW x, in torch"""
    y = x.transpose(2, 3) if op & 1 else x
    dims = [d for d, bit in ((2, 2), (3, 4)) if op & bit]
    return torch.flip(y, dims) if dims else y


# the reference's transforms as ops: rot90(x, k, [2, 3]) for k = 1, 2, 3; flip(x, [3]); flip(x, [2]); transpose(2, 3)
ROT90_OPS, HFLIP_OP, VFLIP_OP, TRANSPOSE_OP, ANTI_TRANSPOSE_OP = {1: 3, 2: 6, 3: 5}, 4, 2, 1, 7


# ------------------------------------------------------------------------------------------------ apply cases
# (N, H, W, C, op, kernel).  Maps: one pixel, one row, one column, a tile edge -1 / +1 on either axis (31 x 33, 33 x 31: the
# tile is 32, 16 or 8 pixels on a side, by C), whole tiles (32 x 32), several tiles (64 x 40).
def _apply_cases():
    cases = []

    def add(kernel, c, maps, ops, n=1):
        cases.extend((n, h, w, c, op, kernel) for h, w in maps for op in ops)

    # LDS tile, 32 x 32 pixels (C <= 4): every swap op on the ragged and the multi-tile maps, the small maps with two each
    add(TILE, 1, ((31, 33), (33, 31), (64, 40)), SWAP_OPS)
    add(TILE, 3, ((31, 33), (33, 31)), SWAP_OPS, n=3)
    add(TILE, 3, ((64, 40),), SWAP_OPS)
    add(TILE, 1, ((1, 1), (1, 7), (7, 1), (32, 32)), (1, 7))
    add(TILE, 4, ((1, 1), (1, 7), (7, 1), (32, 32)), (3, 5))      # 16 elements per thread
    add(TILE, 2, ((33, 31),), (1, 5))
    # LDS tile, 16 x 16 pixels (4 < C <= 16) and 8 x 8 pixels (16 < C <= 64): pixels off the 16-byte grid
    add(TILE, 6, ((31, 33), (33, 31)), SWAP_OPS)
    add(TILE, 6, ((64, 40),), (3, 5), n=3)
    add(TILE, 6, ((1, 7),), (3,))
    add(TILE, 6, ((7, 1),), (5,))
    add(TILE, 6, ((1, 1),), (1,))
    add(TILE, 21, ((31, 33),), SWAP_OPS)
    add(TILE, 21, ((33, 31), (64, 40)), (1, 7))
    add(TILE, 21, ((1, 1), (1, 7), (7, 1)), (5,))
    # an NCHW-contiguous [2, 6, H, W] map is [12, H, W, 1]
    add(TILE, 1, ((31, 33),), SWAP_OPS, n=12)
    add(SCALAR, 1, ((31, 33),), PLAIN_OPS, n=12)
    # element per thread, scalar: rows map to rows; a swap op only on a pixel off the 16-byte grid that no tile holds
    add(SCALAR, 3, ((31, 33),), PLAIN_OPS)
    add(SCALAR, 1, ((64, 40),), (2, 4, 6))
    add(SCALAR, 6, ((1, 1), (1, 7), (7, 1)), (6,))
    add(SCALAR, 2, ((33, 31),), (2,), n=3)
    add(SCALAR, 67, ((31, 33),), SWAP_OPS)
    # element per thread, 16 bytes: every op on C % 4 == 0 past the crossover (C > 4)
    add(VEC, 4, ((31, 33),), PLAIN_OPS)
    add(VEC, 8, ((33, 31),), (6,))
    add(VEC, 8, ((33, 31), (64, 40)), (3, 5))
    add(VEC, 12, ((1, 7),), (4, 3))
    add(VEC, 12, ((31, 33),), (1, 7))
    add(VEC, 20, ((7, 1),), (2,))
    add(VEC, 20, ((1, 1),), (0, 1))
    add(VEC, 132, ((31, 33),), (6,), n=3)
    add(VEC, 20, ((31, 33),), SWAP_OPS)
    add(VEC, 20, ((33, 31),), (3,), n=3)
    add(VEC, 132, ((33, 31),), SWAP_OPS)
    add(VEC, 132, ((7, 1),), (5,))
    add(VEC, 132, ((32, 32),), (7,))
    return tuple(cases)


APPLY_CASES = _apply_cases()
# kernels the plan is forced onto with evk_d4_force_kernel (the measurement hook): the tile on pixels past the crossover, the
# element kernels on a narrow swapped pixel.  (N, H, W, C, op, forced kernel)
FORCED_CASES = (
    (1, 31, 33, 20, 3, TILE), (2, 33, 31, 8, 5, TILE), (1, 9, 7, 64, 1, TILE), (1, 33, 31, 16, 7, TILE),
    (1, 33, 31, 4, 3, VEC), (1, 33, 31, 4, 5, SCALAR), (1, 33, 31, 6, 1, SCALAR),
)

# ------------------------------------------------------------------------------------------------ merge cases
OPS_CYCLE = (3, 0, 5, 4, 1, 6, 7, 2)       # term k of a mixed case has op OPS_CYCLE[k % 8]
# (N, C, Ho, Wo, term count, ops: 'mixed' | 'plain', kernel).  Non-square maps: a swapped term is [N, Wo, Ho, C].
MERGE_CASES = (
    (2, 3, 33, 31, 1, 'mixed', TILE),
    (12, 1, 31, 33, 2, 'mixed', TILE),       # the NCHW alias of [2, 6, 31, 33]
    (2, 4, 33, 31, 3, 'mixed', TILE),        # 16 accumulators per thread
    (1, 6, 20, 12, 7, 'mixed', TILE),
    (1, 5, 33, 31, 8, 'mixed', TILE),
    (1, 3, 20, 12, 16, 'mixed', TILE),
    (1, 2, 20, 12, 17, 'mixed', TILE),       # chained through acc
    (2, 20, 33, 31, 8, 'mixed', VEC),
    (1, 20, 7, 5, 17, 'mixed', VEC),
    (1, 132, 5, 3, 7, 'mixed', VEC),
    (2, 21, 9, 7, 8, 'mixed', TILE),         # the 8 x 8 tile
    (1, 8, 33, 31, 8, 'mixed', VEC),
    (1, 67, 9, 7, 8, 'mixed', SCALAR),
    (1, 3, 33, 31, 3, 'plain', SCALAR),
    (1, 3, 20, 12, 17, 'plain', SCALAR),
)


def merge_ops(nterms, kind):
    cyc = OPS_CYCLE if kind == 'mixed' else PLAIN_OPS
    return [cyc[k % len(cyc)] for k in range(nterms)]


def merge_kernel(lib, n, c, ho, wo, ops):
    """the kernel of one evk_d4_merge launch: the tile kernel if any term's plan is the tile, the 16-byte element kernel if
    every term's plan is, else the scalar one (include/ever_hip.h)"""
    ks = [plan(lib, n, *((wo, ho) if op & 1 else (ho, wo)), c, op)[0] for op in ops]
    return TILE if TILE in ks else VEC if all(k == VEC for k in ks) else SCALAR


def apply_id(case):
    n, h, w, c, op, kernel = case
    return f'{n}x{h}x{w}x{c}-op{op}-{KERNEL_NAMES[kernel].split()[0]}'


def merge_id(case):
    n, c, ho, wo, nt, kind, kernel = case
    return f'{n}x{ho}x{wo}x{c}-{nt}{kind}-{KERNEL_NAMES[kernel].split()[0]}'


# ------------------------------------------------------------------------------------------------ the fixture's model and sets
def toy_model(x):
    """x[:, :2] * ramp, ramp[h, w] = 1 + h / 8 + w / 64 built from the shape at call time: position-dependent, so a wrong inverse
    shows; one IEEE multiply per element, so the CPU and the device agree to the bit"""
    h, w = x.shape[2], x.shape[3]
    ramp = (1 + torch.arange(h, device=x.device, dtype=torch.float32).view(h, 1) / 8
            + torch.arange(w, device=x.device, dtype=torch.float32).view(1, w) / 64)
    return x[:, :2] * ramp


def anti_transpose_class(transform_base):
    """the eighth symmetry, which the reference has no class for, as a user would write it on `transform_base`"""
    class AntiTranspose(transform_base):
        def transform(self, inputs):
            return torch.flip(torch.transpose(inputs, 2, 3), [2, 3])

        def inv_transform(self, transformed_inputs):
            return torch.flip(torch.transpose(transformed_inputs, 2, 3), [2, 3])
    return AntiTranspose


def transform_label(t):
    """the fixture's key of a transform's transformed input, `in_<label>`: each distinct transform is stored once"""
    name = type(t).__name__ + str(getattr(t, 'k', ''))
    if name == 'Scale':
        name += '_%s_%s' % ('x'.join(map(str, t.size)) if t.size else '', t.scale_factor or '')
    return name


FIXTURE_SHAPE = (2, 3, 12, 20)
FIXTURE_SETS = ('d4', 'no_transpose', 'scale')


def fixture_sets(segm, transform_base):
    """the three transform lists of the fixture from a `segm` module (the reference's or this package's) and its Transform"""
    anti = anti_transpose_class(transform_base)
    seven = [segm.Identity(), segm.Rotate90k(1), segm.Rotate90k(2), segm.Rotate90k(3), segm.HorizontalFlip(),
             segm.VerticalFlip(), anti()]
    return {
        'd4': seven[:6] + [segm.Transpose(), anti()],
        'no_transpose': seven,
        'scale': [segm.Identity(), segm.Scale(scale_factor=0.75), segm.HorizontalFlip(), segm.Scale(size=(17, 9))],
    }
