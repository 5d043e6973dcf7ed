"""evk_attn_plan on the host: tiles and trips consistent with N, LDS within the compute unit's budget, and every refusal the
launches make (include/ever_hip.h: RoPE self-attention)."""
import ctypes

import pytest

LDS_PER_CU = 160 * 1024
EVK_E_INVALID, EVK_E_UNSUPPORTED = -1, -2


def _lib():
    from ever_amd import _C
    return _C.load()


def _plan(b, n, h, d, prefix):
    out = (ctypes.c_int32 * 6)(*([-7] * 6))
    return _lib().evk_attn_plan(b, n, h, d, prefix, out), tuple(out)


@pytest.mark.parametrize('d', [32, 64])
def test_tiles_and_trips_follow_n(d):
    for n in range(1, 301):
        for b, h in ((1, 1), (2, 3)):
            rc, (tq, tk, trips, grid, lds, lds_kv) = _plan(b, n, h, d, min(5, n))
            assert rc == 0, (n, d)
            assert tq >= 16 and tk >= 16 and tq % 16 == 0 and tk % 16 == 0
            assert (trips - 1) * tk < n <= trips * tk, (n, tk, trips)
            assert grid == b * h * -(-n // tq), (n, tq, grid)
            # two staged tiles of tk rows and d floats at least; within what one workgroup may take and a CU holds
            assert 2 * tk * d * 4 <= lds <= 64 * 1024 and lds <= lds_kv <= 64 * 1024
            assert 2 * lds_kv <= LDS_PER_CU      # two workgroups to a compute unit


def test_plan_is_the_same_for_every_prefix():
    assert len({_plan(2, 100, 3, 64, p)[1] for p in (0, 1, 5, 100)}) == 1


@pytest.mark.parametrize('b,n,h,d,prefix,code', [
    (1, 4, 1, 48, 0, EVK_E_UNSUPPORTED), (1, 4, 1, 128, 0, EVK_E_UNSUPPORTED), (1, 4, 1, 16, 0, EVK_E_UNSUPPORTED),
    (1, 4, 1, 6, 0, EVK_E_INVALID), (1, 4, 3, 2, 0, EVK_E_INVALID), (1, 0, 1, 64, 0, EVK_E_INVALID),
    (1, -3, 1, 64, 0, EVK_E_INVALID), (1, 4, 1, 64, 5, EVK_E_INVALID), (1, 4, 1, 64, -1, EVK_E_INVALID),
    (0, 4, 1, 64, 0, EVK_E_INVALID), (1, 4, 0, 64, 0, EVK_E_INVALID)])
def test_refusals(b, n, h, d, prefix, code):
    rc, out = _plan(b, n, h, d, prefix)
    assert rc == code
    assert out == (-7,) * 6, 'a refused plan wrote its output'
    assert _lib().evk_last_error()


def test_null_out_and_workspace_of_refused_shapes():
    lib = _lib()
    assert lib.evk_attn_plan(1, 4, 1, 64, 0, None) == EVK_E_INVALID
    assert lib.evk_attn_bwd_workspace_bytes(1, 4, 1, 48) == 0
    assert lib.evk_attn_bwd_workspace_bytes(1, 0, 1, 64) == 0
    assert lib.evk_attn_bwd_workspace_bytes(2, 5, 3, 64) >= 2 * 5 * 3 * 4


def test_host_refusals_of_the_launchers_need_no_device():
    lib = _lib()
    assert lib.evk_attn_fwd(None, None, None, None, None, 1, 4, 1, 64, 0, None) == EVK_E_INVALID
    assert lib.evk_attn_fwd(None, None, None, None, None, 1, 4, 1, 128, 0, None) == EVK_E_UNSUPPORTED
    assert lib.evk_attn_bwd(None, None, None, None, None, None, None, 1, 4, 1, 64, 0, None, 0, None) == 0   # nothing asked for
    assert lib.evk_tokens_prepend_fwd(None, None, None, 1, 4, 1, 8, None) == EVK_E_INVALID
    assert lib.evk_tokens_prepend_fwd(None, None, None, 1, 4, 0, 8, None) == EVK_E_INVALID
    assert lib.evk_tokens_prepend_fwd(None, None, None, 1, 4, 1, 6, None) == EVK_E_INVALID
