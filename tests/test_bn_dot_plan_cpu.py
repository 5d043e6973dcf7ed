"""The plan of the fused BatchNorm + ReLU + classifier pass (csrc/bn_dot.hip: dot_plan), asked of the library on the host through
evk_bn_relu_dot_plan — the function both launchers call, no Python copy: the admission test of the Python wrapper
(hip/pointwise.py: bn_relu_dot_admits) agrees with it on every (C, K), the grid covers every pixel under its cap, an admitted
shape fits the LDS, the workspace is exactly what the launcher carves, and every <NCH, KT> instantiation is where the GPU
tests (tests/test_bn_dot_gpu.py) look for it."""
import ctypes

import pytest

from ever_amd import _C
from ever_amd.hip.pointwise import bn_relu_dot_admits

CHANNELS = list(range(4, 1101, 4)) + [1, 2, 3, 5, 6, 7, 18, 63, 65, 254, 255, 257, 258, 513, 514, 815, 817, 818, 1022, 1023, 1025]
CLASSES = list(range(0, 18))
ROWS = (1, 63, 64, 65, 131072, 131073, 2 ** 36)


def _plan(lib, rows, c, k):
    out = (ctypes.c_int32 * 5)()
    rc = lib.evk_bn_relu_dot_plan(rows, c, k, out)
    return rc, tuple(out)


def test_python_gate_and_plan_admit_the_same_shapes():
    lib = _C.load()
    assert 0 in CLASSES and 17 in CLASSES and 1100 in CHANNELS and any(c % 4 for c in CHANNELS)
    admitted = 0
    for c in CHANNELS:
        for k in CLASSES:
            rc, pl = _plan(lib, 4096, c, k)
            assert rc in (0, -2), (c, k, rc)
            assert bn_relu_dot_admits(c, k, (1, 1)) == (rc == 0), (c, k, rc, lib.evk_last_error())
            if rc == 0:
                admitted += 1
                nblk, ppb, nch, kt, lds = pl
                assert lds == 16 * (4 + k) * c and lds <= 65536, (c, k, pl)
                assert nch in (1, 2, 4) and 64 * nch >= c // 4 and kt in (1, 4, 16) and kt >= k, (c, k, pl)
                assert nch == 1 or kt <= 4, (c, k, pl)
            else:
                msg = lib.evk_last_error().decode()
                assert f'C={c} K={k}' in msg, (c, k, msg)
    assert admitted > 1000
    for shape in ((3, 3), (1, 3), (3, 1), ()):
        assert not bn_relu_dot_admits(64, 1, shape)


def test_grid_covers_every_pixel_under_its_cap():
    lib = _C.load()
    for rows in ROWS:
        for c, k in ((4, 1), (8, 2), (256, 12), (512, 4), (816, 1)):
            rc, (nblk, ppb, nch, kt, lds) = _plan(lib, rows, c, k)
            assert rc == 0, (rows, c, k, lib.evk_last_error())
            assert 1 <= nblk <= 2048 and nblk * ppb >= rows, (rows, nblk, ppb)
            assert ppb == -(-rows // nblk) and nblk == min(2048, -(-rows // 64)), (rows, nblk, ppb)
            # the layout evk_bn_relu_dot_bwd carves: sums and maxima [nblk][2][C] each, dW partials [nblk][K][C], dbias
            # partials [nblk][K], 16 C floats of coefficients
            assert lib.evk_bn_relu_dot_workspace_bytes(rows, c, k) == 4 * (nblk * ((4 + k) * c + k) + 16 * c), (rows, c, k)
    assert _plan(lib, 2 ** 36, 8, 2)[1][:2] == (2048, 2 ** 25)           # (64-bit rows)
    assert _plan(lib, 131073, 8, 2)[1][:2] == (2048, 65)                 # 2017 workgroups hold every pixel: 31 stay empty
    assert -(-131073 // 65) == 2017
    assert lib.evk_bn_relu_dot_workspace_bytes(0, 8, 2) == 0 and lib.evk_bn_relu_dot_workspace_bytes(64, 8, 0) == 0


PINNED = [
    # (C, K) -> (NCH, KT): one row per instantiation, the rounding 3 -> 4 chunks, both shapes on the LDS budget
    ((4, 1), (1, 1)), ((256, 1), (1, 1)), ((252, 3), (1, 4)), ((256, 4), (1, 4)), ((204, 16), (1, 16)), ((64, 5), (1, 16)),
    ((256, 12), (1, 16)), ((260, 1), (2, 1)), ((512, 1), (2, 1)), ((260, 2), (2, 4)), ((512, 4), (2, 4)), ((516, 1), (4, 1)),
    ((816, 1), (4, 1)), ((516, 3), (4, 4)), ((640, 2), (4, 4)), ((680, 2), (4, 4)),
]
REFUSED = [(260, 5), (320, 16), (820, 1), (1024, 1), (64, 17), (4, 17), (256, 13), (512, 5), (516, 4), (684, 2), (64, 0), (0, 1), (-4, 1)]


@pytest.mark.parametrize('shape,want', PINNED, ids=lambda v: 'x'.join(map(str, v)))
def test_instantiation_table(shape, want):
    lib = _C.load()
    rc, pl = _plan(lib, 1000, *shape)
    assert rc == 0 and pl[2:4] == want, (shape, rc, pl)


def test_every_instantiation_is_pinned_and_the_refusals_refuse():
    lib = _C.load()
    assert {w for _, w in PINNED} == {(1, 1), (1, 4), (1, 16), (2, 1), (2, 4), (4, 1), (4, 4)}
    assert [s for s, _ in PINNED if 16 * (4 + s[1]) * s[0] == 65536] == [(256, 12), (512, 4)]
    out = (ctypes.c_int32 * 5)(*([-7] * 5))
    for c, k in REFUSED:
        assert lib.evk_bn_relu_dot_plan(1000, c, k, out) == -2, (c, k)
        assert f'C={c} K={k}' in lib.evk_last_error().decode(), (c, k, lib.evk_last_error())
        assert not bn_relu_dot_admits(c, k, (1, 1)), (c, k)
    for rows in (0, -1):
        assert lib.evk_bn_relu_dot_plan(rows, 64, 1, out) == -2, rows
    assert tuple(out) == (-7,) * 5, 'a refusal wrote its answer'
    assert lib.evk_bn_relu_dot_plan(1000, 64, 1, None) == -1 and b'bn_relu_dot_plan' in lib.evk_last_error()
