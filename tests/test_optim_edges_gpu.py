"""The multi-tensor optimizer kernels (csrc/optim.hip) — SGD, Adam / AdamW, the gradient norm with its clip coefficient, the
DDP bucket pack — called directly through the C ABI on address / size tables built here, past one trip of their grids
(evk_opt_blocks_per_tensor workgroups of 256 threads per tensor: 32768 elements, 131072 for the 16-byte SGD loop) and at
addresses that are 4- but not 16-byte aligned, where the SGD kernel takes its scalar loop (the path every gradient that is a
view into a DDP bucket takes).

Every tensor a kernel writes is a slice of a sentinel-guarded allocation (tests/guard_common.py); a misaligned tensor starts
one element into its slice and that element must keep its NaN.

References: torch.optim.SGD / Adam / AdamW on float64 copies on the CPU, with the hyper-parameters rounded to the floats the
kernels receive and the gradients multiplied by the same clip coefficient.  Tolerances are the project's
(tests/test_train_gpu.py): SGD rtol 1e-5, atol 1e-6 on parameters and momentum buffers; Adam rtol 2e-5, atol 2e-6 on the
parameters.  Adam's moments are held to rtol 1e-5 plus 4 ulp of the tensor's largest moment as absolute slack: exp_avg =
m + (g - m)(1 - beta1) cancels where g is near -9 m, and exp_avg_sq squares g + wd p, which cancels where the two terms
meet — the rounding of the operands stays, which no fp32 evaluation can avoid, and an rtol alone would refuse torch's own.
Whatever is a selection or a single fp32 operation (the pack, the two SGD loops against each other, the device learning
rate) is compared bit for bit.  The norm is accumulated in fp64 and rounded once: 4 ulp of fp32 around the float64 value
(sqrt and the double -> float conversion)."""
import numpy as np
import pytest
import torch

from tests.guard_common import guarded, guards_intact

pytestmark = pytest.mark.gpu

F32_EPS = float(np.finfo(np.float32).eps)
GRID = 128 * 256                    # elements one trip of a scalar grid-stride loop covers (asserted below)
SGD_SIZES = (1, 3, 4, 5, 255, 1031, 32768, 32769, 131079)
ADAM_SIZES = (1, 5, 1031, 32768, 32769, 70001)
NORM_SIZES = (1, 255, 256, 257, 32767, 32769, 100003)
PACK_SIZES = (1, 5, 32767, 32768, 32769, 40001)


def f32(v):
    """the value a float argument has once it crossed the C ABI"""
    return float(np.float32(v))


def _lib():
    from ever_amd import _C
    return _C.load()


def _call(name, *args):
    from ever_amd import _C
    _C.call(name, *args)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _table(vals, cuda):
    return torch.tensor([int(v) for v in vals], dtype=torch.int64, device=cuda)


class Slot:
    """values on the device inside a guarded allocation, `shift` elements (4 bytes each) into the 256-byte aligned slice"""

    def __init__(self, values, cuda, shift=0):
        self.n, self.shift = values.numel(), shift
        self.whole, self.inner = guarded(self.n + shift, cuda)
        self.t = self.inner[shift:]
        self.t.copy_(values.reshape(-1))
        assert self.t.data_ptr() % 16 == (4 * shift) % 16

    def ptr(self):
        return self.t.data_ptr()

    def fetch(self, what, nan_ok=False):
        torch.cuda.synchronize()
        assert guards_intact(self.whole, self.n + self.shift), f'{what}: wrote outside its tensor'
        assert bool(torch.isnan(self.inner[:self.shift]).all()), f'{what}: wrote in front of a misaligned tensor'
        got = self.t.cpu()
        assert nan_ok or not bool(torch.isnan(got).any()), f'{what}: NaN'
        return got


def _same_bits(got, ref, what):
    bad = got.view(torch.int32) != ref.view(torch.int32)
    assert not bool(bad.any()), (f'{what}: {int(bad.sum())} of {bad.numel()} elements differ in their bits, first at '
                                 f'{int(bad.nonzero()[0])}: {got[bad][0].item()!r} vs {ref[bad][0].item()!r}')


def _allclose(got, ref, rtol, atol, what):
    err = (got.double() - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bool(bad.any()), (f'{what}: {int(bad.sum())} of {bad.numel()} elements off, worst {err.max().item():.3e} '
                                 f'(rtol {rtol:g}, atol {atol:g})')


def _randn(sizes, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) * scale for n in sizes]


def test_size_tables_straddle_the_grid():
    """by sizes: one element either side of one trip of each loop, several trips, a tail the 16-byte loop leaves"""
    assert _lib().evk_opt_blocks_per_tensor() * 256 == GRID
    for sizes in (SGD_SIZES, ADAM_SIZES, NORM_SIZES, PACK_SIZES):
        assert min(sizes) == 1 and any(n <= GRID for n in sizes) and any(n == GRID + 1 for n in sizes)
        assert any(n > 2 * GRID for n in sizes) or sizes is PACK_SIZES
    assert GRID in SGD_SIZES and GRID in ADAM_SIZES and GRID in PACK_SIZES
    assert any(n > 4 * GRID and n % 4 for n in SGD_SIZES)          # two 16-byte trips and a scalar tail
    assert any(n % 4 == 0 for n in SGD_SIZES) and any(n < 4 for n in SGD_SIZES)
    assert {255, 256, 257} <= set(NORM_SIZES)                       # one workgroup's threads


# ------------------------------------------------------------------------------------------------ SGD
def _sgd_launch(cuda, ps, gs, bs, lr, momentum, dampening, wd, nesterov, first, clip=None, lr_dev=None):
    pt, gt = _table([s.ptr() for s in ps], cuda), _table([s.ptr() for s in gs], cuda)
    bt = None if bs is None else _table([s.ptr() for s in bs], cuda)
    nt = _table([s.n for s in ps], cuda)
    _call('evk_sgd_multi_lr', pt.data_ptr(), gt.data_ptr(), None if bt is None else bt.data_ptr(), nt.data_ptr(), len(ps),
          lr, None if lr_dev is None else lr_dev.data_ptr(), momentum, dampening, wd, 1 if nesterov else 0, 1 if first else 0,
          None if clip is None else clip.data_ptr(), _stream())
    torch.cuda.synchronize()


SGD_GRID = [(m, d, False, wd, clip) for m in (0.0, 0.9) for d in (0.0, 0.1) for wd in (0.0, 1e-4) for clip in (None, 0.37, 1.0)]
SGD_GRID += [(0.9, 0.0, True, wd, clip) for wd in (0.0, 1e-4) for clip in (None, 0.37, 1.0)]


@pytest.mark.parametrize('momentum,dampening,nesterov,wd,clip', SGD_GRID,
                         ids=lambda v: 'noclip' if v is None else str(v))
def test_sgd_multi_matches_float64_torch_sgd(cuda, momentum, dampening, nesterov, wd, clip):
    lr = 0.05
    p0 = _randn(SGD_SIZES, 1)
    ps = [Slot(p, cuda) for p in p0]
    bs = [Slot(torch.full((n,), float('nan')), cuda) for n in SGD_SIZES] if momentum else None   # the first step writes them
    clip_dev = None if clip is None else torch.tensor([clip], device=cuda)
    cc = 1.0 if clip is None else f32(clip)
    qs = [p.double().requires_grad_() for p in p0]
    ref = torch.optim.SGD(qs, lr=f32(lr), momentum=f32(momentum), dampening=f32(dampening), weight_decay=f32(wd),
                          nesterov=nesterov)
    for step in range(3):
        g0 = _randn(SGD_SIZES, 10 + step)
        gs = [Slot(g, cuda) for g in g0]
        _sgd_launch(cuda, ps, gs, bs, lr, momentum, dampening, wd, nesterov, step == 0, clip_dev)
        for q, g in zip(qs, g0):
            q.grad = g.double() * cc
        ref.step()
        for k, q in enumerate(qs):
            what = f'step {step} size {SGD_SIZES[k]}'
            _allclose(ps[k].fetch(what), q.detach(), 1e-5, 1e-6, what + ' parameter')
            _same_bits(gs[k].fetch(what), g0[k], what + ' gradient (read only)')
            if momentum:
                _allclose(bs[k].fetch(what), ref.state[q]['momentum_buffer'], 1e-5, 1e-6, what + ' momentum buffer')


def _sgd_two_steps(cuda, shift_p, shift_g, shift_b, sizes, lr=0.05, lr_dev=None):
    p0 = _randn(sizes, 2)
    ps = [Slot(p, cuda, shift_p) for p in p0]
    bs = [Slot(torch.full((n,), float('nan')), cuda, shift_b) for n in sizes]
    clip = torch.tensor([0.37], device=cuda)
    for step in range(2):
        gs = [Slot(g, cuda, shift_g) for g in _randn(sizes, 20 + step)]
        _sgd_launch(cuda, ps, gs, bs, lr, 0.9, 0.1, 1e-4, False, step == 0, clip, lr_dev)
    return [s.fetch('parameter') for s in ps], [s.fetch('momentum buffer') for s in bs]


ALIGN_SIZES = (1, 5, 1031, 40000, 131079)


def test_sgd_scalar_and_16_byte_loops_round_identically(cuda):
    """The parameter, the gradient, the momentum buffer in turn one element into a flat buffer (a FlatGradDDP gradient is such
    a view): the scalar loop takes over, for 40000 and 131079 elements with two and five trips, and must give the bits the
    16-byte loop gives — it is fused-multiply-add for fused-multiply-add the same arithmetic."""
    assert sum(1 for n in ALIGN_SIZES if n > GRID) >= 2 and any(n > 4 * GRID for n in ALIGN_SIZES)
    want_p, want_b = _sgd_two_steps(cuda, 0, 0, 0, ALIGN_SIZES)
    for shifts in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (3, 2, 1)):
        got_p, got_b = _sgd_two_steps(cuda, *shifts, ALIGN_SIZES)
        for k, n in enumerate(ALIGN_SIZES):
            _same_bits(got_p[k], want_p[k], f'shifts {shifts} size {n} parameter')
            _same_bits(got_b[k], want_b[k], f'shifts {shifts} size {n} momentum buffer')


def test_sgd_reads_the_learning_rate_from_the_device_word(cuda):
    sizes = (5, 1031, 40000)
    want_p, want_b = _sgd_two_steps(cuda, 0, 0, 0, sizes, lr=0.05)
    got_p, got_b = _sgd_two_steps(cuda, 0, 0, 0, sizes, lr=999.0, lr_dev=torch.tensor([0.05], device=cuda))
    for k, n in enumerate(sizes):
        _same_bits(got_p[k], want_p[k], f'size {n} parameter')
        _same_bits(got_b[k], want_b[k], f'size {n} momentum buffer')


def test_sgd_without_momentum_needs_no_buffers_and_with_momentum_refuses_none(cuda):
    from ever_amd._C import HipKernelError
    sizes = (3, 1031, 32769)
    p0, g0 = _randn(sizes, 3), _randn(sizes, 4)
    ps, gs = [Slot(p, cuda) for p in p0], [Slot(g, cuda, 1) for g in g0]
    with pytest.raises(HipKernelError, match='status -1: sgd_multi: momentum needs buffers'):
        _sgd_launch(cuda, ps, gs, None, 0.05, 0.9, 0.0, 1e-4, False, True)
    for k, s in enumerate(ps):
        _same_bits(s.fetch('refused launch'), p0[k], 'a refused launch changed a parameter')
    _sgd_launch(cuda, ps, gs, None, 0.05, 0.0, 0.0, 1e-4, False, False)
    for k, s in enumerate(ps):
        want = p0[k].double() - f32(0.05) * (g0[k].double() + f32(1e-4) * p0[k].double())
        _allclose(s.fetch('no momentum'), want, 1e-5, 1e-6, f'size {sizes[k]}')


def test_fused_sgd_with_a_parameter_that_joins_at_step_two(cuda):
    """a fresh (first_step) and a warm launch in the same step, sharing one clip coefficient — against float64 torch SGD"""
    import ever_amd as er
    shapes = [(1031,), (40000,), (7, 3), (16, 4, 3, 3)]
    late = 2
    p0 = [torch.randn(s, generator=torch.Generator().manual_seed(30 + k)) for k, s in enumerate(shapes)]
    ps = [p.to(cuda).requires_grad_() for p in p0]
    qs = [p.double().requires_grad_() for p in p0]
    kw = dict(momentum=0.9, weight_decay=1e-4, nesterov=False)
    oa = er.opt.FusedSGD(ps, lr=0.05, **kw)
    ob = torch.optim.SGD(qs, lr=f32(0.05), momentum=f32(0.9), weight_decay=f32(1e-4))
    for step in range(3):
        for k, (p, q) in enumerate(zip(ps, qs)):
            g = torch.randn(shapes[k], generator=torch.Generator().manual_seed(100 * step + k))
            if k == late and step == 0:
                p.grad = q.grad = None
                continue
            p.grad, q.grad = g.to(cuda), g.double()
        oa.fused_clip(max_norm=0.5)
        ref_norm = torch.nn.utils.clip_grad_norm_([q for q in qs if q.grad is not None], max_norm=f32(0.5))
        _check_norm(oa.last_grad_norm.item(), ref_norm.item())
        oa.step()
        ob.step()
        for k, (p, q) in enumerate(zip(ps, qs)):
            _allclose(p.detach().cpu(), q.detach(), 1e-5, 1e-6, f'step {step} parameter {shapes[k]}')
            if 'momentum_buffer' in ob.state[q]:
                _allclose(oa.state[p]['momentum_buffer'].cpu(), ob.state[q]['momentum_buffer'], 1e-5, 1e-6,
                          f'step {step} momentum buffer {shapes[k]}')
    assert not torch.equal(ps[late].detach().cpu(), p0[late])


# ------------------------------------------------------------------------------------------------ Adam
def _adam_launch(cuda, ps, gs, ms, vs, lr, b1, b2, eps, wd, decoupled, step, clip=None, bc=None):
    tabs = [_table([s.ptr() for s in group], cuda) for group in (ps, gs, ms, vs)]
    nt = _table([s.n for s in ps], cuda)
    bc1, bc2s = bc if bc is not None else (1.0 - b1 ** step, (1.0 - b2 ** step) ** 0.5)
    _call('evk_adam_multi', *[t.data_ptr() for t in tabs], nt.data_ptr(), len(ps), lr, b1, b2, eps, wd, decoupled, bc1, bc2s,
          None if clip is None else clip.data_ptr(), _stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize('clip', [None, 0.37], ids=['noclip', 'clip'])
@pytest.mark.parametrize('wd', [0.0, 0.02])
@pytest.mark.parametrize('decoupled', [0, 1], ids=['adam', 'adamw'])
def test_adam_multi_matches_float64_torch_adam(cuda, decoupled, wd, clip):
    lr, b1, b2, eps = 0.01, 0.9, 0.99, 1e-8
    p0 = _randn(ADAM_SIZES, 5)
    ps = [Slot(p, cuda) for p in p0]
    ms = [Slot(torch.zeros(n), cuda) for n in ADAM_SIZES]
    vs = [Slot(torch.zeros(n), cuda) for n in ADAM_SIZES]
    clip_dev = None if clip is None else torch.tensor([clip], device=cuda)
    cc = 1.0 if clip is None else f32(clip)
    qs = [p.double().requires_grad_() for p in p0]
    ref = (torch.optim.AdamW if decoupled else torch.optim.Adam)(qs, lr=f32(lr), betas=(f32(b1), f32(b2)), eps=f32(eps),
                                                                 weight_decay=f32(wd))
    for step in range(1, 5):
        g0 = _randn(ADAM_SIZES, 40 + step)
        gs = [Slot(g, cuda) for g in g0]
        _adam_launch(cuda, ps, gs, ms, vs, lr, b1, b2, eps, wd, decoupled, step, clip_dev)
        for q, g in zip(qs, g0):
            q.grad = g.double() * cc
        ref.step()
        for k, q in enumerate(qs):
            what = f'step {step} size {ADAM_SIZES[k]}'
            st = ref.state[q]
            _allclose(ps[k].fetch(what), q.detach(), 2e-5, 2e-6, what + ' parameter')
            for name, slot in (('exp_avg', ms[k]), ('exp_avg_sq', vs[k])):
                _allclose(slot.fetch(what), st[name], 1e-5, 4 * F32_EPS * st[name].abs().max().item(), f'{what} {name}')
            _same_bits(gs[k].fetch(what), g0[k], what + ' gradient (read only)')


def test_adam_refuses_bias_corrections_that_are_not_positive(cuda):
    from ever_amd._C import HipKernelError
    p0 = _randn((5,), 6)
    ps, gs = [Slot(p0[0], cuda)], [Slot(p0[0], cuda)]
    ms, vs = [Slot(torch.zeros(5), cuda)], [Slot(torch.zeros(5), cuda)]
    for bc in ((0.0, 0.5), (-0.1, 0.5), (0.5, 0.0), (0.5, -1.0)):
        with pytest.raises(HipKernelError, match='adam_multi: bad bias correction'):
            _adam_launch(cuda, ps, gs, ms, vs, 0.01, 0.9, 0.99, 1e-8, 0.0, 0, 1, bc=bc)
    _same_bits(ps[0].fetch('refused'), p0[0], 'a refused launch changed a parameter')
    assert bool((ms[0].fetch('refused') == 0).all()) and bool((vs[0].fetch('refused') == 0).all())


# ------------------------------------------------------------------------------------------------ norm and clip coefficient
def _sqnorm(cuda, grads, max_norm, shifts=None):
    """-> (total_norm, clip_coef) as numpy float32 scalars; the partial sums live in exactly blocks * ntensors guarded doubles"""
    shifts = shifts or [0] * len(grads)
    gs = [Slot(g, cuda, s) for g, s in zip(grads, shifts)]
    nb = _lib().evk_opt_blocks_per_tensor()
    pw, pi = guarded(nb * len(grads), cuda, dtype=torch.float64)
    ow, oi = guarded(2, cuda)
    gt, nt = _table([s.ptr() for s in gs], cuda), _table([s.n for s in gs], cuda)       # (alive until the kernel has run)
    _call('evk_sqnorm_multi', gt.data_ptr(), nt.data_ptr(), len(gs), pi.data_ptr(), max_norm, oi.data_ptr(),
          oi.data_ptr() + 4, _stream())
    torch.cuda.synchronize()
    assert guards_intact(pw, pi.numel()) and guards_intact(ow, 2), 'sqnorm_multi wrote outside its outputs'
    for s, g in zip(gs, grads):
        got = s.fetch('gradient', nan_ok=True)
        assert got.view(torch.int32).equal(g.view(torch.int32)), 'sqnorm_multi changed a gradient'
    part = pi.cpu()
    want = torch.stack([g.double().square().sum() for g in grads])
    if bool(torch.isfinite(want).all()):
        assert not bool(torch.isnan(part).any()), 'a partial sum was never written'
        got = part.view(len(grads), nb).sum(1)
        assert bool(((got - want).abs() <= 1e-12 * want).all()), 'per-tensor partial sums'
    out = oi.cpu().numpy()
    return out[0], out[1]


def _norm64(grads):
    return float(torch.sqrt(sum(g.double().square().sum() for g in grads)))


def _check_norm(tn, ref):
    assert abs(float(tn) - ref) <= 4 * float(np.spacing(np.float32(ref))), (float(tn), ref)


def _check_coef_above(coef, tn, max_norm):
    want = f32(max_norm) / (float(tn) + 1e-6)
    assert want < 1 and abs(float(coef) - want) <= 2 * float(np.spacing(np.float32(want))), (float(coef), want)


def test_sqnorm_and_clip_coefficient_across_sizes_and_alignment(cuda):
    grads = _randn(NORM_SIZES, 7)
    shifts = [1 if n == 32769 else 0 for n in NORM_SIZES]
    ref = _norm64(grads)
    tn, coef = _sqnorm(cuda, grads, 2 * ref, shifts)
    _check_norm(tn, ref)
    assert float(coef) == 1.0                  # below max_norm: exactly 1
    tn, coef = _sqnorm(cuda, grads, ref / 3, shifts)
    _check_norm(tn, ref)
    _check_coef_above(coef, tn, ref / 3)


def test_sqnorm_of_300_small_tensors(cuda):
    """clip_coef_kernel strides 150 times over the 38400 partial sums"""
    sizes = [1 + (7 * k) % 13 for k in range(300)]
    grads = _randn(sizes, 8)
    ref = _norm64(grads)
    tn, coef = _sqnorm(cuda, grads, 1.0)
    _check_norm(tn, ref)
    _check_coef_above(coef, tn, 1.0)


def test_sqnorm_of_zeros_huge_values_inf_and_nan(cuda):
    sizes = (5, 1031, 32769)
    zeros = [torch.zeros(n) for n in sizes]
    tn, coef = _sqnorm(cuda, zeros, 35.0)
    assert float(tn) == 0.0 and float(coef) == 1.0
    huge = [torch.full((n,), 1e20) * (1 + torch.arange(n) % 3) for n in sizes]      # squares overflow fp32
    assert not bool(torch.isfinite(huge[0] * huge[0]).any())
    ref = _norm64(huge)
    tn, coef = _sqnorm(cuda, huge, 35.0)
    assert np.isfinite(tn)
    _check_norm(tn, ref)
    _check_coef_above(coef, tn, 35.0)
    grads = _randn(sizes, 9)
    grads[2][32768] = float('inf')             # (the element of the second trip)
    tn, coef = _sqnorm(cuda, grads, 35.0)
    assert float(tn) == float('inf') and float(coef) == 0.0 and not np.signbit(coef)
    grads = _randn(sizes, 9)
    grads[1][1030] = float('nan')
    tn, coef = _sqnorm(cuda, grads, 35.0)
    assert np.isnan(tn)
    # torch.nn.utils.clip_grad_norm_(error_if_nonfinite=False): clamp(max_norm / (nan + 1e-6), max=1) is NaN — the step is
    # poisoned where everyone can see it, not taken unclipped by the tensors that happen to be finite
    assert np.isnan(coef), f'a NaN norm gave the clip coefficient {float(coef)!r}'
    ps = [torch.nn.Parameter(g.clone()) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    assert bool(torch.isnan(torch.nn.utils.clip_grad_norm_(ps, 35.0))) and all(bool(torch.isnan(p.grad).all()) for p in ps)


def test_fused_sgd_step_after_a_nan_gradient_matches_torch(cuda):
    import ever_amd as er
    shapes = [(1031,), (7, 3), (40000,), (5,)]
    p0 = [torch.randn(s, generator=torch.Generator().manual_seed(50 + k)) for k, s in enumerate(shapes)]
    ps, qs = [p.to(cuda).requires_grad_() for p in p0], [p.clone().requires_grad_() for p in p0]
    kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-4)
    oa, ob = er.opt.FusedSGD(ps, **kw), torch.optim.SGD(qs, **kw)
    for step in range(2):
        for k, (p, q) in enumerate(zip(ps, qs)):
            g = torch.randn(shapes[k], generator=torch.Generator().manual_seed(60 + 10 * step + k))
            if step == 1 and k == 2:
                g[39999] = float('nan')
            if k == 3:
                continue                        # (never has a gradient: stays as it is on both sides)
            p.grad, q.grad = g.to(cuda), g.clone()
        oa.fused_clip(max_norm=0.5)
        norm = torch.nn.utils.clip_grad_norm_([q for q in qs if q.grad is not None], max_norm=0.5)
        assert bool(torch.isnan(oa.last_grad_norm)) == bool(torch.isnan(norm)) == (step == 1)
        oa.step()
        ob.step()
        for k, (p, q) in enumerate(zip(ps, qs)):
            got, want = p.detach().cpu(), q.detach()
            assert torch.equal(torch.isnan(got), torch.isnan(want)), (step, shapes[k], int(torch.isnan(got).sum()))
            assert bool(torch.isnan(want).all()) == (step == 1 and k != 3)
            assert torch.allclose(got, want, rtol=1e-5, atol=1e-6, equal_nan=True), (step, shapes[k])


# ------------------------------------------------------------------------------------------------ bucket pack
@pytest.mark.parametrize('scale', [1.0, 1.0 / 3.0, 0.5], ids=['1', 'third', 'half'])
def test_pack_multi_scales_into_4_byte_slots_and_leaves_the_gaps(cuda, scale):
    srcs = _randn(PACK_SIZES, 11)
    null_k, own_k = 1, 3            # a tensor without a gradient (zeros); a gradient that already is a view of its slot
    offsets, off = [], 1
    for k, n in enumerate(PACK_SIZES):
        offsets.append(off)
        off += n + (1, 3, 2, 5, 1, 7)[k]
    assert any(o % 4 for o in offsets) and len({o % 4 for o in offsets}) >= 3
    total = off
    dw, di = guarded(total, cuda)
    di[offsets[own_k]:offsets[own_k] + PACK_SIZES[own_k]].copy_(srcs[own_k])
    devs = [s.to(cuda) for s in srcs]
    ptrs = [d.data_ptr() for d in devs]
    ptrs[null_k] = 0
    ptrs[own_k] = di.data_ptr() + 4 * offsets[own_k]
    st, nt, ot = _table(ptrs, cuda), _table(PACK_SIZES, cuda), _table(offsets, cuda)    # (alive until the kernel has run)
    _call('evk_pack_multi', st.data_ptr(), nt.data_ptr(), ot.data_ptr(), len(srcs), scale, di.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert guards_intact(dw, total), 'pack_multi wrote outside the bucket'
    got = di.cpu()
    want = torch.full((total,), float('nan'))
    for k, n in enumerate(PACK_SIZES):
        want[offsets[k]:offsets[k] + n] = torch.zeros(n) if k == null_k else srcs[k] * torch.tensor(scale, dtype=torch.float32)
    gap = torch.isnan(want)
    assert int(gap.sum()) == total - sum(PACK_SIZES)
    assert bool(torch.isnan(got[gap]).all()), 'pack_multi wrote into a gap between two slots'
    _same_bits(got[~gap], want[~gap], 'packed bucket')
    for k, d in enumerate(devs):
        _same_bits(d.cpu(), srcs[k], f'source {k} (read only)')
