"""The thread plan of the row LayerNorm / layer-scale kernels (csrc/row_groups.hpp) through evk_ln_plan and the workspace
sizes, on the host: a row belongs to L lanes (a power of two <= 64) holding ceil(C / 4 / L) 16-byte columns each, the grid is
capped whatever the row count, the backward records are one [2][C] per workgroup, and what is out of scope is refused."""
import ctypes

import pytest

from ever_amd import _C

CHANNELS = (4, 8, 96, 100, 128, 192, 384, 768, 1024, 1536, 2048)


def _plan(r, c):
    out = (ctypes.c_int32 * 4)(-7, -7, -7, -7)
    rc = _C.load().evk_ln_plan(r, c, out)
    return rc, tuple(out)


@pytest.mark.parametrize('c', CHANNELS)
def test_lanes_and_columns_cover_the_row(c):
    rc, (lanes, cols, rows, wgs) = _plan(1000, c)
    assert rc == 0
    assert 1 <= lanes <= 64 and lanes & (lanes - 1) == 0
    assert lanes * cols >= c // 4 > lanes * (cols - 1)
    assert rows * lanes == 256 and wgs >= 1


def test_c96_does_not_idle_half_a_wave():
    _, (lanes, cols, _, _) = _plan(1000, 96)
    assert lanes * cols == 24            # every lane of a group holds live columns


@pytest.mark.parametrize('c', CHANNELS)
def test_workgroups_are_bounded_whatever_the_row_count(c):
    counts = [_plan(r, c)[1][3] for r in (1, 2 ** 20, 2 ** 30)]
    assert counts[0] == 1 and counts[1] <= counts[2] <= 4096
    assert counts[2] == _plan(2 ** 40, c)[1][3]      # the cap, not a function of R
    rows = _plan(1, c)[1][2]
    assert _plan(rows + 1, c)[1][3] == 2


@pytest.mark.parametrize('c', CHANNELS)
@pytest.mark.parametrize('r', (1, 257, 2 ** 20, 2 ** 30))
def test_workspace_is_one_record_per_workgroup(r, c):
    lib = _C.load()
    wgs = _plan(r, c)[1][3]
    assert lib.evk_ln_bwd_workspace_bytes(r, c) == wgs * 2 * c * 4
    n, hw = (1, r) if r < 4 else (4, r // 4)
    assert lib.evk_scale_residual_bwd_workspace_bytes(n, hw, c) == _plan(n * hw, c)[1][3] * c * 4


@pytest.mark.parametrize('r,c', [(8, 0), (8, 6), (8, 2052), (0, 96), (-3, 96), (8, -4)])
def test_refusals(r, c):
    lib = _C.load()
    rc, out = _plan(r, c)
    assert rc in (-1, -2) and out == (-7, -7, -7, -7) and lib.evk_last_error()
    assert lib.evk_ln_bwd_workspace_bytes(r, c) == 0
    # the launch entries refuse the same shapes before they look at a pointer or launch anything: safe without a GPU
    assert lib.evk_ln_fwd(None, None, None, 1e-6, None, None, None, r, c, None) == rc
    assert lib.evk_ln_bwd(None, None, None, None, None, None, None, None, r, c, None, 0, None) == rc
    assert lib.evk_scale_residual_fwd(None, None, None, None, None, 1, r, c, None) == rc
    assert lib.evk_scale_residual_bwd(None, None, None, None, None, None, 1, r, c, None, 0, None) == rc


def test_null_plan_pointer_and_null_tensors_are_refused():
    lib = _C.load()
    assert lib.evk_ln_plan(8, 96, None) == -1
    assert lib.evk_ln_fwd(None, None, None, 1e-6, None, None, None, 8, 96, None) == -1
    assert lib.evk_scale_residual_fwd(None, None, None, None, None, 2, 4, 96, None) == -1
