"""The float64 reference of FS-Relation with its two BatchNorm + ReLU passes inside (csrc/relation.hip: relation_fwd_kernel<true>,
relation_bn_bwd_kernel<NCH>, and the hand-over of its records to bn.hip: evk_bn_bwd_from_partials), its derived bounds and the
seeded cases.  No torch.cuda here: tests/test_relation_ref_cpu.py holds the formulas to autograd, tests/test_relation_bn_edges_gpu.py
holds the kernels to the formulas.

The statistics are INPUTS at this interface.  mean, invstd are formed in float64 from the case's z and cast to fp32; scale =
gamma invstd and shift = beta - mean scale are formed in float64 from those fp32 values and cast.  The reference uses the very
fp32 arrays the kernels get, so their error is zero.  Every stage is referenced to float64 of THAT stage's actual fp32 inputs:
the backward takes the forward's stored fp32 r, the records and the hand-over take the g the backward stored.

  forward    y = relu(z sc + sh) (both branches);  dot = sum_c scene y_c;  r = 1 / (1 + e^-dot);  out = r y_f
  backward   g_f = (y_f > 0) dout r;  dotb = sum_c dout y_f;  dz = dotb r (1 - r);  g_c = (y_c > 0) scene dz;
             dscene = sum_pix y_c dz
  records    per workgroup (nb = evk_relation_bn_parts(N, HW) of them, nb / N per image, ppb = ceil(HW / (nb / N)) pixels each;
             wave w owns pixels p0 + w, p0 + w + 4, ...): (sum g, sum g xhat), (max|g|, max|xhat|) of both BatchNorms, xhat =
             (z - mean) invstd, and the scene partial sum y_c dz
  hand-over  dbeta, dgamma, dz of BatchNorm from the stored g (tests/bn_ref_common.py: _bwd_ref, train = 1)

Bounds (u = 2^-24; a chain of L roundings errs by at most L u sum|terms|):
  pre, y      3 u (|z sc| + |sh|): the product, the sum, one to spare for either contraction; y the same where pre > 0
  both dots   sum|a| e_y + L_d u sum|a y|,  L_d = 5 ceil(C / 256) + 6: five roundings per trip of a lane (four products, of
              which three additions and the one into the running sum), six butterfly levels
  r           r (1 - r) e_dot + K u r + 2^-126
              K = 5 = 2 + 1 + 2.  expf: the HIP math API reference (ROCm documentation, "HIP math API", single precision
              floating-point mathematical functions) lists a maximum error of 1 ulp; one ulp of a value just above a power
              of two is 2^-23 of it = 2 u.  Division: csrc/Makefile compiles with -O3 and neither -ffast-math nor
              -fno-hip-fp32-correctly-rounded-divide-sqrt, and hipcc's default is -fhip-fp32-correctly-rounded-divide-sqrt
              (clang's documentation of the flag: "fp32 divide and sqrt are correctly rounded"): half an ulp = u.  Plus 2 for
              the negation and the addition 1 + e.  Each of them reaches r with a factor (1 - r) <= 1.
              2^-126 is the absolute floor: below the smallest normal fp32 a result has no relative precision (e^-dot
              overflows for dot < -88.7, where the true r < 2.9e-39 and the kernel's is 0; the hardware reciprocal and
              exponential may flush subnormals)
  out         |y_f| e_r + r e_y + u |out|
  g_f         u |dout r|
  dz          r (1 - r) e_dotb + 4 u |dz|  (1 - r, two products, one to spare)
  g_c         |scene| e_dz + u |g_c|
  scene partial, dscene   L u sum|y dz| + sum(|y| e_dz + |dz| e_y) + u |dscene|,  L = ceil(ppb / 4) + 2: a wave owns every
              fourth pixel of the range, two fold levels over the four waves; the partials are folded in fp64 and cast once
  sum records L u sum|g|;  (L + 1) u sum|g xhat| + sum|g| 2 u |xhat|
  max|g|      the maximum of the stored |g| over the range BIT FOR BIT;  max|xhat| within 2 u |xhat| of the float64 maximum
  packed dz   the fp32 bound + max(2^-22 |dz|, 2^-25 s), as in tests/test_bn_dot_gpu.py

ReLU masks: the upstream gradient of the content branch is per pixel (scene dz), so an element with an uncertain mask cannot go
without one.  Every z of either branch whose float64 pre-activation lies within its bound of zero is moved away before the
launch; `undecided` counts what is left and must be 0.  Exact zeros are planted instead: channel 0 of both branches has sc = 1,
sh = 0 and z = 0 on a third of the pixels, where y == 0 in fp32 and fp64 alike and the mask must be off."""
import functools

import torch

from tests.bn_ref_common import U, _bwd_ref, _data, _given_stats, _params

EPS = 1e-5
K_SIGMOID = 5
FLT_MIN = 2.0 ** -126

# (N, C, HW), each for one reason (FS-Relation with BatchNorm)
CASES = [
    (1, 4, 1),          # one lane, one pixel, three idle waves
    (1, 4, 3),          # fewer pixels than waves
    (2, 64, 131),       # lanes 16-63 idle; 3 workgroups of 44 pixels, the last 43: the fourth wave is one pixel short
    (2, 256, 67),       # 64 chunks: every lane once, the last shape of NCH = 1
    (2, 260, 65),       # NCH = 2 with only lane 0's second chunk live
    (1, 448, 6),        # the limit: 64 512 bytes of LDS
    (3, 4, 16448),      # the cap: 256 workgroups of 65 pixels per image, 254 own pixels (the last of them 3), two own none;
                        # the forward's 49 344 pixels need a second trip of its 8192 x 4 grid
]
FORWARD_ONLY = (1, 1028, 3)     # five channel trips for lane 0; the forward has no channel limit
SATURATED = (2, 64, 131)        # with image 1's scene x 250: |dot| passes 90 on many pixels
SATURATED_GAIN = 250.0


def ranges(nb, n, hw):
    """(workgroups per image, pixels per workgroup) from nb = evk_relation_bn_parts(n, hw)"""
    assert nb % n == 0
    nblk = nb // n
    return nblk, -(-hw // nblk)


def wave_pixels(hw, nblk, ppb):
    """the pixels of one image that wave w of workgroup b walks, as relation_bn_bwd_kernel does"""
    for b in range(nblk):
        p0, p1 = b * ppb, min(hw, b * ppb + ppb)
        for w in range(4):
            yield b, w, range(p0 + w, p1, 4)


def per_range(t, n, hw, nblk, ppb, how='sum'):
    """[n hw, c] -> [n nblk, c]: the sum (or the maximum, of non-negative t) over every workgroup's pixel range; a range
    without pixels gives 0"""
    c = t.shape[1]
    pad = torch.zeros(n, nblk * ppb, c, dtype=t.dtype)
    pad[:, :hw] = t.view(n, hw, c)
    pad = pad.view(n, nblk, ppb, c)
    return (pad.sum(2) if how == 'sum' else pad.amax(2)).reshape(n * nblk, c)


class Obj:
    pass


def act(z, sc, sh):
    """y = relu(z sc + sh) in float64 with its bound, the mask, and the pre-activation with its bound; sc, sh float64"""
    zs = z.double() * sc
    pre, e_pre = zs + sh, 3 * U * (zs.abs() + sh.abs())
    on = pre > 0
    return pre.clamp_min(0), e_pre * on, on, pre, e_pre


def dot_chain(c):
    return 5 * (-(-c // 256)) + 6


def forward_stages(scene_pix, zc, sc_c, sh_c, zf, sc_f, sh_f):
    """scene_pix [rows, C] float64 (the image's scene vector on each of its pixels); z fp32 or float64; sc, sh float64"""
    f = Obj()
    c = zc.shape[1]
    f.yc, f.e_yc, f.on_c, _, _ = act(zc, sc_c, sh_c)
    f.yf, f.e_yf, f.on_f, _, _ = act(zf, sc_f, sh_f)
    f.dot = (scene_pix * f.yc).sum(1)
    f.e_dot = (scene_pix.abs() * f.e_yc).sum(1) + dot_chain(c) * U * (scene_pix * f.yc).abs().sum(1)
    f.r, f.q = torch.sigmoid(f.dot), torch.sigmoid(-f.dot)            # q = 1 - r without the cancellation
    f.e_r = f.r * f.q * f.e_dot + K_SIGMOID * U * f.r + FLT_MIN
    f.out = f.r[:, None] * f.yf
    f.e_out = f.yf.abs() * f.e_r[:, None] + f.r[:, None] * f.e_yf + U * f.out.abs()
    return f


def backward_stages(f, dout, scene_pix, r):
    """f: forward_stages of the same inputs (its activations and masks); r [rows] float64: the r the backward is GIVEN"""
    b = Obj()
    c = dout.shape[1]
    d = dout.double()
    b.gf = f.on_f * d * r[:, None]
    b.e_gf = U * b.gf.abs()
    b.dotb = (d * f.yf).sum(1)
    b.e_dotb = (d.abs() * f.e_yf).sum(1) + dot_chain(c) * U * (d * f.yf).abs().sum(1)
    b.dz = b.dotb * r * (1 - r)
    b.e_dz = r * (1 - r) * b.e_dotb + 4 * U * b.dz.abs()
    b.gc = f.on_c * scene_pix * b.dz[:, None]
    b.e_gc = (scene_pix.abs() * b.e_dz[:, None] + U * b.gc.abs()) * f.on_c
    b.terms = f.yc * b.dz[:, None]                                     # what the scene gradient sums over the pixels
    b.e_terms = f.yc.abs() * b.e_dz[:, None] + b.dz.abs()[:, None] * f.e_yc
    return b


def scene_records(b, n, hw, nblk, ppb):
    """the scene partial per workgroup [n nblk, C] and dscene [n, C], with their bounds"""
    chain = -(-ppb // 4) + 2
    c = b.terms.shape[1]
    part = per_range(b.terms, n, hw, nblk, ppb)
    e_in = chain * U * per_range(b.terms.abs(), n, hw, nblk, ppb) + per_range(b.e_terms, n, hw, nblk, ppb)
    dscene = part.view(n, nblk, c).sum(1)
    return part, e_in + U * part.abs(), dscene, e_in.view(n, nblk, c).sum(1) + U * dscene.abs()


def bn_records(z, g, mean, invstd, n, hw, nblk, ppb):
    """(sum g, sum g xhat, max|g|, max|xhat|) per workgroup [n nblk, C] in float64 from the STORED g, and their bounds (the
    maximum of |g| has none: it is exact)"""
    chain = -(-ppb // 4) + 2
    gd = g.double()
    xh = (z.double() - mean.double()) * invstd.double()
    rng = functools.partial(per_range, n=n, hw=hw, nblk=nblk, ppb=ppb)
    rec = Obj()
    rec.sg, rec.e_sg = rng(gd), chain * U * rng(gd.abs())
    rec.sgx = rng(gd * xh)
    rec.e_sgx = (chain + 1) * U * rng((gd * xh).abs()) + rng(gd.abs() * 2 * U * xh.abs())
    rec.mg = rng(gd.abs(), how='max')
    rec.mx = rng(xh.abs(), how='max')
    rec.e_mx = 2 * U * rec.mx
    return rec


def handover_ref(z, g, mean, invstd, gamma, rec):
    """dbeta, e, dgamma, e, dz, e of the BatchNorm backward from the stored g and the kernel's own records (rec: bn_records
    of the same g): the sums are the records folded in fp64 and cast once"""
    zero = torch.zeros(z.shape[1], dtype=torch.float64)
    st = _given_stats(mean.double(), invstd.double(), zero, zero)
    gd = g.double()
    e_sums = (rec.e_sg.sum(0) + U * gd.sum(0).abs(),
              rec.e_sgx.sum(0) + U * (gd * (z.double() - st.mean) * st.invstd).sum(0).abs())
    return _bwd_ref(z, gd, st, gamma.double(), 1, 0, e_sums=e_sums)


def _branch(gen, rows, c):
    """z, gamma, mean | invstd [2][C], scale | shift [2][C] of one branch (fp32), channel 0 planted, uncertain masks moved"""
    z = _data(gen, rows, c)
    gamma, beta, _, _ = _params(gen, c, True)
    zd = z.double()
    mean = zd.mean(0).float()
    invstd = (zd.var(0, unbiased=False) + EPS).rsqrt().float()
    mean[0], invstd[0], gamma[0], beta[0] = 0.0, 1.0, 1.0, 0.0        # channel 0: sc = 1, sh = 0 (the planted zeros)
    scale = gamma.double() * invstd.double()
    sc, sh = scale.float(), (beta.double() - mean.double() * scale).float()
    assert sc[0] == 1.0 and sh[0] == 0.0
    z[::3, 0] = 0.0
    scd, shd = sc.double(), sh.double()
    for _ in range(6):                                                # move every uncertain pre-activation away from zero
        _, _, _, pre, e_pre = act(z, scd, shd)
        unsure = (pre.abs() <= e_pre) & (e_pre > 0)
        if not unsure.any():
            break
        z = torch.where(unsure, z + 0.25, z)
    _, _, _, pre, e_pre = act(z, scd, shd)
    undecided = int(((pre.abs() <= e_pre) & (e_pre > 0)).sum())
    planted = (pre[:, 0] == 0) & (e_pre[:, 0] == 0)
    assert int(planted.sum()) == -(-rows // 3) and bool((z[planted, 0] == 0).all())
    return z, gamma, torch.stack([mean, invstd]).contiguous(), torch.stack([sc, sh]).contiguous(), undecided, planted


@functools.lru_cache(maxsize=None)
def case(n, c, hw, gain=1.0):
    """the seeded fp32 inputs of a case and the float64 forward with its bounds; computed once per process, never written to"""
    gen = torch.Generator().manual_seed(7000 + 1000 * n + 7 * c + hw)
    rows = n * hw
    k = Obj()
    k.n, k.c, k.hw, k.rows, k.name = n, c, hw, rows, (n, c, hw) if gain == 1.0 else (n, c, hw, 'saturated')
    k.zc, k.gamma_c, k.mi_c, k.ss_c, left_c, k.planted_c = _branch(gen, rows, c)
    k.zf, k.gamma_f, k.mi_f, k.ss_f, left_f, k.planted_f = _branch(gen, rows, c)
    k.undecided = left_c + left_f
    k.scene = torch.randn(n, c, generator=gen) * 0.2                  # keeps the sigmoid off its tails
    if gain != 1.0:
        k.scene[1] *= gain
    k.dout = torch.randn(rows, c, generator=gen)
    k.scene_pix = k.scene.double().repeat_interleave(hw, 0)
    k.fwd = forward_stages(k.scene_pix, k.zc, k.ss_c[0].double(), k.ss_c[1].double(), k.zf, k.ss_f[0].double(), k.ss_f[1].double())
    return k
