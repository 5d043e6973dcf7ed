"""The token prefix kernels (csrc/tokens.hip) through the C ABI: forward bit-exact against torch.cat, the patch gradient a
bit-exact copy, the prefix gradient on integer-valued inputs bit-exact against float64 (every partial sum is an exact fp32
number, so any summation order gives the same bits and a lost or doubled sample does not).  All outputs are NaN-filled slices
of sentinel-guarded, exactly sized allocations (tests/guard_common.py)."""
import pytest
import torch

from tests.guard_common import guarded, guards_intact

pytestmark = pytest.mark.gpu

# (B, P, HW, C)
CASES = {
    'smallest': (1, 1, 1, 4),
    'b3_p5_hw1_c4': (3, 5, 1, 4),
    'b1_p5_c64': (1, 5, 7, 64),
    'b3_p1_c64': (3, 1, 9, 64),
    'vit_like': (2, 5, 196, 384),
    'second_grid_trip': (3, 5, 1500, 256),    # 3 x 1505 x 64 16-byte words: past 1024 workgroups of 256 lanes
}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _fetch(whole, inner, what):
    torch.cuda.synchronize()
    assert guards_intact(whole, inner.numel()), f'{what}: wrote outside its allocation'
    got = inner.cpu()
    assert not bool(torch.isnan(got).any()), f'{what}: {int(torch.isnan(got).sum())} of {got.numel()} elements unwritten'
    return got


def _same_bits(got, ref, what):
    bad = got.contiguous().view(torch.int32) != ref.contiguous().view(torch.int32)
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} of {bad.numel()} elements differ in their bits'


@pytest.mark.parametrize('name', list(CASES))
def test_prepend_forward_and_backward(name):
    from ever_amd import _C
    b, p, hw, c = CASES[name]
    assert name != 'second_grid_trip' or b * (p + hw) * c // 4 > 1024 * 256
    dev = torch.device('cuda:0')
    gen = torch.Generator().manual_seed(7)
    patch = torch.randn(b, hw, c, generator=gen)
    prefix = torch.randn(p, c, generator=gen)
    dout = torch.randint(-64, 65, (b, p + hw, c), generator=gen).float()
    ref = torch.cat([prefix[None].expand(b, -1, -1), patch], dim=1)
    ow, out = guarded(ref.numel(), dev)
    patch_d, prefix_d = patch.to(dev), prefix.to(dev)
    _C.call('evk_tokens_prepend_fwd', patch_d.data_ptr(), prefix_d.data_ptr(), out.data_ptr(), b, hw, p, c, _stream())
    _same_bits(_fetch(ow, out, 'out').reshape(ref.shape), ref, f'{name} out')
    xw, dpatch = guarded(patch.numel(), dev)
    pw, dprefix = guarded(prefix.numel(), dev)
    dout_d = dout.to(dev)
    _C.call('evk_tokens_prepend_bwd', dout_d.data_ptr(), dpatch.data_ptr(), dprefix.data_ptr(), b, hw, p, c, _stream())
    _same_bits(_fetch(xw, dpatch, 'dpatch').reshape(patch.shape), dout[:, p:].contiguous(), f'{name} dpatch')
    _same_bits(_fetch(pw, dprefix, 'dprefix').reshape(prefix.shape), dout[:, :p].double().sum(0).float(), f'{name} dprefix')
    # partial requests
    xw, dpatch = guarded(patch.numel(), dev)
    pw, dprefix = guarded(prefix.numel(), dev)
    _C.call('evk_tokens_prepend_bwd', dout_d.data_ptr(), None, dprefix.data_ptr(), b, hw, p, c, _stream())
    _same_bits(_fetch(pw, dprefix, 'dprefix alone').reshape(prefix.shape), dout[:, :p].double().sum(0).float(), f'{name} dprefix alone')
    assert bool(torch.isnan(dpatch).all()) and guards_intact(xw, dpatch.numel())


def test_wrapper_matches_cat_and_autograd():
    from ever_amd.hip import functional as HF
    dev = torch.device('cuda:0')
    gen = torch.Generator().manual_seed(3)
    patch = torch.randn(3, 6, 8, generator=gen).to(dev).requires_grad_(True)
    prefix = torch.randn(5, 8, generator=gen).to(dev).requires_grad_(True)
    w = torch.randint(-8, 9, (3, 11, 8), generator=gen).float().to(dev)
    out = HF.prepend_tokens(patch, prefix)
    (out * w).sum().backward()
    ref = torch.cat([prefix.detach()[None].expand(3, -1, -1), patch.detach()], dim=1)
    _same_bits(out.detach().cpu(), ref.cpu(), 'out')
    _same_bits(patch.grad.cpu(), w[:, 5:].contiguous().cpu(), 'dpatch')
    _same_bits(prefix.grad.cpu(), w[:, :5].double().sum(0).float().cpu(), 'dprefix')


def test_refusals_leave_the_output_untouched():
    from ever_amd import _C
    lib = _C.load()
    dev = torch.device('cuda:0')
    x = torch.randn(64, device=dev)
    ow, out = guarded(64, dev)
    for b, hw, p, c in ((1, 4, 0, 8), (1, 4, 1, 6), (1, 4, 1, 0), (0, 4, 1, 8), (1, 0, 1, 8)):
        assert lib.evk_tokens_prepend_fwd(x.data_ptr(), x.data_ptr(), out.data_ptr(), b, hw, p, c, _stream()) < 0
        assert lib.evk_tokens_prepend_bwd(x.data_ptr(), out.data_ptr(), out.data_ptr(), b, hw, p, c, _stream()) < 0
    assert lib.evk_tokens_prepend_fwd(None, x.data_ptr(), out.data_ptr(), 1, 1, 1, 8, _stream()) < 0
    torch.cuda.synchronize()
    assert guards_intact(ow, 64) and bool(torch.isnan(out).all())
