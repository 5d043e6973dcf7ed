"""Helpers shared by the weight-gradient plan tests (tests/test_conv_wgrad_plan_cpu.py, tests/test_conv_wgrad_gpu.py): descriptors,
the flags of evk_conv2d_wgrad_f16x2_ex, and evk_conv2d_wgrad_route as a Python call."""
import ctypes

from ever_amd import _C

X_PACKED, DY_PACKED, X_PLANAR, DY_PLANAR, SHARED = 2, 4, 8, 16, 32
PLANAR = X_PLANAR | DY_PLANAR
GIB2 = 0x7fffffff


def conv_desc(n, h, w, cin, cout, kh, kw, sh=1, sw=1, ph=None, pw=None, dh=1, dw=1):
    """descriptor with "same"-style padding unless given; None if the output would be empty"""
    ph = dh * (kh - 1) // 2 if ph is None else ph
    pw = dw * (kw - 1) // 2 if pw is None else pw
    ho = (h + 2 * ph - dh * (kh - 1) - 1) // sh + 1
    wo = (w + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    if ho < 1 or wo < 1:
        return None
    return _C.ConvDesc(n, h, w, cin, ho, wo, cout, kh, kw, sh, sw, ph, pw, dh, dw)


def wgrad_route(lib, d, planes, flags=0):
    """(status, kernel name, (bm, bn, tiles_co, tiles_k, splitk, chunk))"""
    buf = ctypes.create_string_buffer(128)
    plan = (ctypes.c_int32 * 6)()
    rc = lib.evk_conv2d_wgrad_route(ctypes.byref(d), planes, flags, buf, len(buf), plan)
    return rc, buf.value.decode(), tuple(plan)


def fields(d):
    return tuple(getattr(d, f) for f, _ in d._fields_)


def below_2gib(d):
    return d.N * d.H * d.W * d.Cin * 4 < GIB2 and d.N * d.Ho * d.Wo * d.Cout * 4 < GIB2


def nine_tap(d):
    return (d.kh, d.kw, d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w) == (3, 3, 1, 1, 1, 1, 1, 1) and \
        d.W % 32 == 0 and d.Wo == d.W and d.Ho == d.H


def planar_ok(d):
    return d.Cin % 64 == 0 and d.Cout % 64 == 0 and d.Wo % 8 == 0 and below_2gib(d)


def combos(d):
    """every (arithmetic, flags) the C-ABI accepts for the descriptor"""
    out = [(0, 0), (1, 0), (3, 0)]
    forms = [0, X_PACKED, DY_PACKED, X_PACKED | DY_PACKED] + ([PLANAR] if planar_ok(d) else [])
    return out + [(2, f | s) for f in forms for s in (0, SHARED)]


def colsum_blocks(m):
    return min(1024, max(1, (m + 255) // 256))
