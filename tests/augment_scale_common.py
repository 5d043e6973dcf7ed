"""The numpy statement of the rescale step of evk_augment_scale_batch (include/ever_hip.h) — the DEFINITION the GPU tests
compare with bit for bit — and aten's CPU result, the second witness it is held to within a derived bound.

numpy evaluates every float32 operation below on its own, correctly rounded, with no fused multiply-add: each line is the
arithmetic of the kernel, operation for operation.  `python tests/augment_scale_common.py` repeats the survey the contract's
"relation to aten" rests on (70 (size, factor) cases) and prints what it finds."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import preprocess_common as pc

f32 = np.float32


def scaled_hw(h, w, f):
    """aten's output sizes"""
    return int(math.floor(float(h) * f)), int(math.floor(float(w) * f))


def inv_scale(f):
    """s of the contract: float(1.0 / double(f))"""
    return f32(1.0 / float(f))


def s_bits(f):
    return int(np.array(inv_scale(f), dtype=f32).view(np.uint32))


def ratio(n, nz):
    """ry of the contract: one fp32 division, 0 for a single output row"""
    return f32(n - 1) / f32(nz - 1) if nz > 1 else f32(0)


def unscaled(h, w, f):
    """the samples the pass does not scale at all: Z = S, bit for bit"""
    return scaled_hw(h, w, f) == (h, w) and inv_scale(f) == f32(1)


def _axis(n, nz):
    pos = ratio(n, nz) * np.arange(nz, dtype=f32)                       # sy = ry * float(a)
    i0 = np.minimum(pos.astype(np.int64), n - 1)                         # y0 = min(int(sy), Hs - 1)
    i1 = i0 + (i0 < n - 1)                                               # y1 = y0 + (y0 < Hs - 1)
    lo = pos - i0.astype(f32)                                            # ly = sy - float(y0)
    hi = f32(1) - lo                                                     # hy = 1 - ly
    assert pos.dtype == lo.dtype == hi.dtype == f32
    return i0, i1, lo, hi


def bilinear(src, f):
    """Z [Hz, Wz, C] fp32 of a [Hs, Ws, C] uint8 or fp32 source"""
    h, w = src.shape[:2]
    hz, wz = scaled_hw(h, w, f)
    p = np.asarray(src).astype(f32)                                      # p** = float(raw)
    if unscaled(h, w, f):
        return p
    y0, y1, ly, hy = _axis(h, hz)
    x0, x1, lx, hx = _axis(w, wz)
    ly, hy = ly[:, None, None], hy[:, None, None]
    lx, hx = lx[None, :, None], hx[None, :, None]
    top = hx * p[y0][:, x0] + lx * p[y0][:, x1]                          # hx * p00 + lx * p01
    bot = hx * p[y1][:, x0] + lx * p[y1][:, x1]                          # hx * p10 + lx * p11
    z = hy * top + ly * bot
    assert z.dtype == f32 and z.shape == (hz, wz, p.shape[2])
    return z


def nearest(m, f):
    """Zm [Hz, Wz] of a [Hs, Ws] label map of any integer dtype"""
    h, w = m.shape
    hz, wz = scaled_hw(h, w, f)
    s = inv_scale(f)
    iy = np.minimum(np.floor(np.arange(hz, dtype=f32) * s).astype(np.int64), h - 1)
    ix = np.minimum(np.floor(np.arange(wz, dtype=f32) * s).astype(np.int64), w - 1)
    return np.asarray(m)[np.ix_(iy, ix)]


def augment_scale_ref(images, masks, scales, ops, origins, crop, out_size, mean, std, mask_pad_value, out_mask_dtype=None):
    """evk_augment_scale_batch on the CPU: the statement above, then evk_augment_batch's own CPU evaluation on Z
    (tests/preprocess_common.augment_ref: torch ops, `sub().div()`)"""
    z = [torch.from_numpy(np.ascontiguousarray(bilinear(im.cpu().numpy(), f))) for im, f in zip(images, scales)]
    zm = None
    if masks is not None:
        zm = [torch.from_numpy(np.ascontiguousarray(nearest(m.cpu().numpy(), f))) for m, f in zip(masks, scales)]
    return pc.augment_ref(z, zm, ops, origins, crop, out_size, mean, std, mask_pad_value, out_mask_dtype)


# ------------------------------------------------------------------------------------------------------------ aten, the witness
def aten_bilinear(src, f):
    """aten's CPU bilinear (align_corners=True) of the source cast to fp32: [Hz, Wz, C]"""
    x = torch.from_numpy(np.asarray(src).astype(f32)).permute(2, 0, 1)[None]
    return F.interpolate(x, scale_factor=f, mode='bilinear', align_corners=True)[0].permute(1, 2, 0).numpy()


def aten_nearest(m, f):
    return F.interpolate(torch.from_numpy(np.asarray(m))[None, None], scale_factor=f, mode='nearest')[0][0].numpy()


def image_bound(src):
    """The bound of the contract on |statement - aten| before normalisation.  Both sides combine the same four taps with
    weights in [0, 1] that sum to 1, in at most 9 roundings of relative 2^-24 each, and every intermediate is at most
    max|source| in magnitude (up to those roundings): each side is within about 9 * 2^-24 * max|source| of the exact
    value, the two within 8 * 2^-23 * max|source| of each other with room to spare (2 ulp of 255 was the worst seen)."""
    return 8.0 * 2.0 ** -23 * float(np.abs(np.asarray(src).astype(np.float64)).max())


def survey():
    g = np.random.default_rng(0)
    cases = differ = 0
    worst, label_diff = 0.0, []
    for h, w in ((13, 9), (3, 5), (16, 16), (7, 31), (32, 20), (4, 4), (5, 8)):
        for f in (0.34, 0.5, 0.75, 1.0, 1.1, 1.25, 1.5, 1.75, 2.0, 0.9):
            if min(scaled_hw(h, w, f)) < 1:
                continue
            src = g.integers(0, 256, (h, w, 3)).astype(f32)
            d = float(np.abs(aten_bilinear(src, f) - bilinear(src, f)).max())
            cases, differ, worst = cases + 1, differ + (d > 0), max(worst, d)
            m = g.integers(0, 7, (h, w)).astype(np.uint8)
            if not np.array_equal(aten_nearest(m, f), nearest(m, f)):
                label_diff.append((h, w, f))
    print(f'bilinear: {cases} cases, {differ} not bit-equal to aten, worst |diff| {worst} (bound {8 * 2.0 ** -23 * 255})')
    print(f'nearest: {len(label_diff)} of {cases} cases differ from aten: {label_diff}')


if __name__ == '__main__':
    survey()
