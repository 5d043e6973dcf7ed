"""The numpy statement of the four pyramid-pooling functions (include/ever_hip.h: evk_ppm_*) and the case table of their
tests.  Arrays are NHWC.  The fp32 forms follow the header's orders operation by operation (numpy rounds every fp32
operation on its own); the float64 forms use the SAME fp32 tap indices and weights."""
import math

import numpy as np

F32 = np.float32
U24 = 2.0 ** -24        # half an ulp of 1: one fp32 rounding
N = 2

# (H, W, C, Cp, bins): every map with every kind of bin list, the channel counts rotating; b > H on the small maps
CASES = [
    (1, 1, 4, 4, (1,)), (1, 1, 8, 12, (6,)), (1, 1, 4, 4, (1, 2, 3, 6)), (1, 1, 100, 4, (2, 2)),
    (2, 3, 8, 4, (2,)), (2, 3, 4, 12, (8,)), (2, 3, 100, 4, (1, 2, 3, 6)), (2, 3, 8, 4, (3,)), (2, 3, 8, 4, (6, 3, 2, 1)),
    (5, 7, 100, 12, (3,)), (5, 7, 8, 4, (6, 3, 2, 1)), (5, 7, 4, 4, (2, 2)), (5, 7, 8, 4, (8,)), (5, 7, 256, 4, (1,)),
    (6, 6, 256, 4, (6,)), (6, 6, 8, 12, (1, 2, 3, 6)), (6, 6, 4, 4, (2, 2)), (6, 6, 8, 4, (3,)),
    (12, 12, 100, 12, (1, 2, 3, 6)), (12, 12, 8, 4, (8,)), (12, 12, 4, 4, (1,)), (12, 12, 256, 4, (6, 3, 2, 1)),
    (12, 12, 8, 4, (2,)),
    (13, 9, 256, 12, (1, 2, 3, 6)), (13, 9, 100, 4, (6, 3, 2, 1)), (13, 9, 8, 4, (2,)), (13, 9, 4, 12, (3,)),
    (13, 9, 8, 4, (8,)), (13, 9, 8, 4, (6,)),
    (33, 20, 8, 12, (1, 2, 3, 6)), (33, 20, 100, 4, (8,)), (33, 20, 4, 4, (6,)), (33, 20, 256, 4, (2, 2)),
    (33, 20, 8, 4, (1,)), (33, 20, 4, 4, (3,)),
    # a second channel chunk per the plan: C > 256 in the pool's cell pass, K Cp > 1024 in the expand backward's row pass
    (13, 9, 260, 4, (1, 2, 3, 6)), (5, 7, 4, 260, (1, 2, 3, 6)),
]


def case_id(case):
    h, w, c, cp, bins = case
    return f'{h}x{w}-c{c}-cp{cp}-b' + '_'.join(str(b) for b in bins)


def windows(length, b):
    """aten's adaptive windows of an axis: [(start, end)] * b"""
    return [((i * length) // b, -((-(i + 1) * length) // b)) for i in range(b)]


def pool_fwd64(x, b):
    """float64 window sums and the window counts: ([N,b,b,C], [b,b])"""
    n, h, w, c = x.shape
    x = x.astype(np.float64)
    s = np.zeros((n, b, b, c))
    a = np.zeros((n, b, b, c))
    cnt = np.zeros((b, b))
    for i, (ys, ye) in enumerate(windows(h, b)):
        for j, (xs, xe) in enumerate(windows(w, b)):
            s[:, i, j] = x[:, ys:ye, xs:xe].sum(axis=(1, 2))
            a[:, i, j] = np.abs(x[:, ys:ye, xs:xe]).sum(axis=(1, 2))
            cnt[i, j] = (ye - ys) * (xe - xs)
    return s, a, cnt


def taps(b, length):
    """(i0, i1, l0, l1) of the `length` outputs of an axis with b sources, in fp32 as the header states them"""
    y = np.arange(length, dtype=F32)
    s = F32(b) / F32(length)
    src = np.maximum(s * (y + F32(0.5)) - F32(0.5), F32(0.0)).astype(F32)
    i0 = np.minimum(src.astype(np.int32), b - 1)
    i1 = i0 + (i0 < b - 1)
    l1 = (src - i0.astype(F32)).astype(F32)
    l0 = (F32(1.0) - l1).astype(F32)
    return i0, i1, l0, l1


def expand_fwd(z, h, w, dtype):
    """the bilinear align_corners=False sample of z [N,b,b,Cp] at every pixel of an h x w map, in `dtype` arithmetic with
    the fp32 taps; an axis whose taps coincide contributes the tap itself"""
    b = z.shape[1]
    y0, y1, ly0, ly1 = taps(b, h)
    x0, x1, lx0, lx1 = taps(b, w)
    z = z.astype(dtype)
    lx0, lx1 = lx0.astype(dtype)[None, None, :, None], lx1.astype(dtype)[None, None, :, None]
    ly0, ly1 = ly0.astype(dtype)[None, :, None, None], ly1.astype(dtype)[None, :, None, None]
    samex, samey = (x1 == x0)[None, None, :, None], (y1 == y0)[None, :, None, None]

    def row(yi):
        r = z[:, yi]
        p0, p1 = r[:, :, x0], r[:, :, x1]
        return np.where(samex, p0, lx0 * p0 + lx1 * p1)

    top, bot = row(y0), row(y1)
    return np.where(samey, top, ly0 * top + ly1 * bot).astype(dtype)


def axis_weights(b, length):
    """(W, M): W[y, i] the weight of source i in output y (float64 of the fp32 taps; 1 where the taps coincide) and M the
    membership (which sources an output reads, whatever the weight's value)"""
    i0, i1, l0, l1 = taps(b, length)
    wm = np.zeros((length, b))
    mm = np.zeros((length, b), dtype=bool)
    for y in range(length):
        if i1[y] == i0[y]:
            wm[y, i0[y]] = 1.0
        else:
            wm[y, i0[y]] = float(l0[y])
            wm[y, i1[y]] = float(l1[y])
            mm[y, i1[y]] = True
        mm[y, i0[y]] = True
    return wm, mm


def expand_bwd64(dy, b):
    """dz [N,b,b,Cp] in float64, the sum of |w dy| over the support, and the support size S [b,b]"""
    n, h, w, _ = dy.shape
    wy, my = axis_weights(b, h)
    wx, mx = axis_weights(b, w)
    dy = dy.astype(np.float64)
    dz = np.einsum('yi,xj,nyxc->nijc', wy, wx, dy)
    mag = np.einsum('yi,xj,nyxc->nijc', np.abs(wy), np.abs(wx), np.abs(dy))
    support = np.outer(my.sum(0), mx.sum(0))
    return dz, mag, support


def pool_bwd32(dps, bins, h, w, dskip):
    """dx [N,h,w,C] in fp32, the header's order: dskip (or +0), then bins in order, the windows of a bin row-major, each
    quotient one division"""
    n, c = dps[0].shape[0], dps[0].shape[3]
    dx = np.zeros((n, h, w, c), dtype=F32) if dskip is None else dskip.astype(F32).copy()
    for dp, b in zip(dps, bins):
        for i, (ys, ye) in enumerate(windows(h, b)):
            for j, (xs, xe) in enumerate(windows(w, b)):
                q = (dp[:, i, j].astype(F32) / F32((ye - ys) * (xe - xs))).astype(F32)
                dx[:, ys:ye, xs:xe] = (dx[:, ys:ye, xs:xe] + q[:, None, None, :]).astype(F32)
    return dx


def cells(length, bins):
    """the elementary cells of an axis: sorted distinct window edges of all bins"""
    e = {0, length}
    for b in bins:
        for s, t in windows(length, b):
            e.update((s, t))
    return sorted(e)


def expected_plan(n, h, w, c, cp, bins):
    """what evk_ppm_plan must name for a case"""
    ncy, ncx = len(cells(h, bins)) - 1, len(cells(w, bins)) - 1
    nchunk, rchunk = math.ceil(c / 256), math.ceil(len(bins) * cp / 1024)
    sb, sb2 = sum(bins), sum(b * b for b in bins)
    return [0, 16, ncy, ncx, n * ncy * nchunk, nchunk, n * sb2, n * h * w, n * h * rchunk, rchunk,
            math.ceil(n * sb * (cp // 4) / 256), 256, 4 * n * ncy * ncx * c, 4 * n * h * sb * cp, sb, sb2]
