"""The float64 reference that tests/test_relation_bn_edges_gpu.py holds the FS-Relation BatchNorm kernels to
(tests/relation_ref_common.py), checked without a GPU: its staged formulas are the gradients autograd finds, its cases leave no
ReLU mask undecided, and the pixel ranges it derives from the library's record count cover every pixel once."""
import pytest
import torch
import torch.nn.functional as F

from tests import relation_ref_common as R
from tests.bn_ref_common import _bwd_ref, _data, _given_stats, _params

ALL_CASES = [(cs, 1.0) for cs in R.CASES + [R.FORWARD_ONLY]] + [(R.SATURATED, R.SATURATED_GAIN)]


@pytest.mark.parametrize('n,c,hw', [(2, 8, 5), (3, 12, 7)])
def test_staged_formulas_are_what_autograd_finds(n, c, hw):
    """sigmoid((s * relu(bn(zc))).sum(1)) * relu(bn(zf)) with training-mode batch_norm, autograd in float64, against
    forward_stages / backward_stages / _bwd_ref.  The stages take the statistics as float64 arguments; here they get the
    batch statistics of z UNCAST (the fp32 cast of mean / invstd is all that would separate them from batch_norm's own, and
    the GPU cases pass the cast values to kernel and reference alike), so no residual is left: 1e-10 relative."""
    gen = torch.Generator().manual_seed(100 * n + c)
    rows = n * hw
    zc, zf = _data(gen, rows, c).double(), _data(gen, rows, c).double()
    _, _, gam_c, bet_c = _params(gen, c, True)
    _, _, gam_f, bet_f = _params(gen, c, True)
    scene = torch.randn(n, c, generator=gen).double() * 0.2
    dout = torch.randn(rows, c, generator=gen).double()
    stats = []
    for z, gam, bet in ((zc, gam_c, bet_c), (zf, gam_f, bet_f)):
        mean, invstd = z.mean(0), (z.var(0, unbiased=False) + R.EPS).rsqrt()
        scale = gam * invstd
        stats.append((mean, invstd, scale, bet - mean * scale))
    scene_pix = scene.repeat_interleave(hw, 0)
    f = R.forward_stages(scene_pix, zc, stats[0][2], stats[0][3], zf, stats[1][2], stats[1][3])
    b = R.backward_stages(f, dout, scene_pix, f.r)
    dscene = b.terms.view(n, hw, c).sum(1)
    zero = torch.zeros(c, dtype=torch.float64)
    got = {'out': f.out, 'dscene': dscene}
    for tag, z, g, gam, st in (('c', zc, b.gc, gam_c, stats[0]), ('f', zf, b.gf, gam_f, stats[1])):
        dbeta, _, dgamma, _, dz, _ = _bwd_ref(z, g, _given_stats(st[0], st[1], zero, zero), gam, 1, 0)
        got.update({f'dbeta_{tag}': dbeta, f'dgamma_{tag}': dgamma, f'dz_{tag}': dz})

    nchw = lambda t: t.view(n, hw, c).permute(0, 2, 1).reshape(n, c, hw, 1)      # noqa: E731
    back = lambda t: t.reshape(n, c, hw).permute(0, 2, 1).reshape(rows, c)       # noqa: E731
    leaves = [t.clone().requires_grad_() for t in (scene.view(n, c, 1, 1), nchw(zc), nchw(zf), gam_c, bet_c, gam_f, bet_f)]
    s, tc, tf, gc, bc, gf, bf = leaves
    yc = F.relu(F.batch_norm(tc, None, None, gc, bc, True, 0.1, R.EPS))
    yf = F.relu(F.batch_norm(tf, None, None, gf, bf, True, 0.1, R.EPS))
    out = torch.sigmoid((s * yc).sum(1, keepdim=True)) * yf
    out.backward(nchw(dout))
    want = {'out': back(out.detach()), 'dscene': s.grad.view(n, c), 'dz_c': back(tc.grad), 'dz_f': back(tf.grad),
            'dgamma_c': gc.grad, 'dbeta_c': bc.grad, 'dgamma_f': gf.grad, 'dbeta_f': bf.grad}
    assert bool((f.yc == 0).any()) and bool((f.yf > 0).any())          # both sides of either mask are there
    for name, w in want.items():
        rel = float((got[name] - w).abs().max() / w.abs().max())
        assert rel <= 1e-10, (name, rel)


@pytest.mark.parametrize('cs,gain', ALL_CASES, ids=lambda v: str(v))
def test_no_case_leaves_a_relu_mask_undecided(cs, gain):
    """a condition of the GPU cases, not a measurement: after the nudge no float64 pre-activation of either branch lies
    within its bound of zero, and the planted zeros of channel 0 are exact"""
    k = R.case(*cs, gain)
    assert k.undecided == 0, ('elements whose ReLU mask the float64 pre-activation does not decide', k.name, k.undecided)
    for planted, y, on in ((k.planted_c, k.fwd.yc, k.fwd.on_c), (k.planted_f, k.fwd.yf, k.fwd.on_f)):
        assert int(planted.sum()) == -(-k.rows // 3)
        assert bool((y[planted, 0] == 0).all()) and not bool(on[planted, 0].any())
    # what the planted zeros are for: with the mask on they would carry a gradient
    assert bool((k.dout[k.planted_f, 0] != 0).all()) and bool((k.scene[:, 0] != 0).all())


@pytest.mark.parametrize('cs', R.CASES, ids=lambda v: str(v))
def test_record_ranges_cover_every_pixel_once(cs):
    from ever_amd import _C
    lib = _C.load()
    n, c, hw = cs
    nb = lib.evk_relation_bn_parts(n, hw)
    assert lib.evk_relation_bn_workspace_bytes(n, hw, c) == nb * c * 9 * 4
    nblk, ppb = R.ranges(nb, n, hw)
    assert nblk * ppb >= hw and nblk <= 256
    seen = [0] * hw
    owners = set()
    for b, w, pixels in R.wave_pixels(hw, nblk, ppb):
        for p in pixels:
            seen[p] += 1
            owners.add(b)
    assert seen == [1] * hw
    live = len(owners)
    last = hw - (live - 1) * ppb
    want = {(1, 4, 1): (1, 1, 1, 1), (1, 4, 3): (1, 3, 1, 3), (2, 64, 131): (3, 44, 3, 43), (2, 256, 67): (2, 34, 2, 33),
            (2, 260, 65): (2, 33, 2, 32), (1, 448, 6): (1, 6, 1, 6), (3, 4, 16448): (256, 65, 254, 3)}[cs]
    assert (nblk, ppb, live, last) == want, (cs, nblk, ppb, live, last)
    # per_range sums what the waves walk
    t = torch.arange(n * hw * 2, dtype=torch.float64).view(n * hw, 2)
    rec = R.per_range(t, n, hw, nblk, ppb).view(n, nblk, 2)
    for b in (0, live - 1, nblk - 1):
        rows = [p for bb, w, pixels in R.wave_pixels(hw, nblk, ppb) if bb == b for p in pixels]
        assert torch.equal(rec[n - 1, b], t.view(n, hw, 2)[n - 1, rows].sum(0) if rows else torch.zeros(2, dtype=torch.float64))
