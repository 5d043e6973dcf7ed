"""The plain FS-Relation kernels of csrc/relation.hip (evk_relation_fwd / evk_relation_bwd; the forward is the instantiation
without BatchNorm of the body it shares with evk_relation_bn_fwd) at their edges, called through the C ABI into NaN-filled,
sentinel-guarded outputs and workspace (tests/guard_common.py): nothing outside a result may be written, nothing inside it may
stay NaN — the workspace included, whose every partial record is summed by the scene-gradient fold.

Reference: sigmoid((scene * content).sum(1, keepdim=True)) * feat and its autograd on the CPU in fp64, inputs scaled as in
test_ops_gpu.py::test_gap_relation_mean4 so that the sigmoid stays off its tails.  Tolerance: nothing fixed in advance — aten's
own fp32 CPU result is measured against the same fp64 reference, and the kernel may err at most twice as much plus 4 ulp of the
largest |reference| (tests/yardstick_common.py).  Called twice, the entry points give the same bits: the fold order is fixed."""
import functools

import pytest
import torch

from tests.guard_common import guarded, guards_intact
from tests.yardstick_common import as_close_as_aten

pytestmark = pytest.mark.gpu

# (N, C, HW), each for one reason
CASES = [
    (1, 4, 1),          # one lane, one pixel, one block
    (2, 260, 65),       # C / 4 = 65: lane 0 takes a second channel trip; two blocks per image of 33 and 32 pixels
    (3, 4, 16448),      # 256 blocks (the cap) of 65 pixels: the last two of every image own none and still store zero partials;
                        # 49344 pixels > the 32768 of one forward grid pass: a ragged second trip of the wave-stride loop
    (1, 4096, 3),       # the backward's limit C <= 4096: 64 KB of dynamic LDS
]
OUTPUTS = ('out', 'r', 'dscene', 'dcontent', 'dfeat')


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _case(n, c, hw):
    """fp32 inputs [N, C] / [N, HW, C] and the five results of aten in fp64 and in fp32, laid out as the kernels write them;
    never written to"""
    gen = torch.Generator().manual_seed(1000 * c + hw + n)
    scene = torch.randn(n, c, generator=gen) * 0.2
    content = torch.randn(n, hw, c, generator=gen) * 0.3
    feat = torch.randn(n, hw, c, generator=gen)
    dout = torch.randn(n, hw, c, generator=gen)
    refs = []
    for dt in (torch.float64, torch.float32):
        s = scene.to(dt).view(n, c, 1, 1).requires_grad_()
        ct, ft = (t.to(dt).permute(0, 2, 1).reshape(n, c, hw, 1).requires_grad_() for t in (content, feat))
        r = torch.sigmoid((s * ct).sum(1, keepdim=True))
        out = r * ft
        out.backward(dout.to(dt).permute(0, 2, 1).reshape(n, c, hw, 1))
        pix = lambda t: t.detach().reshape(n, c, hw).permute(0, 2, 1).contiguous()      # noqa: E731
        refs.append(dict(out=pix(out), r=r.detach().reshape(n, hw), dscene=s.grad.reshape(n, c), dcontent=pix(ct.grad),
                         dfeat=pix(ft.grad)))
    return (scene, content, feat, dout) + tuple(refs)


def _run(cuda, dev_in, n, c, hw):
    """one forward and one backward call; the five results and the workspace on the host, after the guard checks"""
    from ever_amd import _C
    sd, cd, fd, gd = dev_in
    ws_bytes = _C.load().evk_relation_workspace_bytes(n, hw, c)
    sizes = dict(out=n * hw * c, r=n * hw, dscene=n * c, dcontent=n * hw * c, dfeat=n * hw * c, workspace=ws_bytes // 4)
    buf = {k: guarded(v, cuda) for k, v in sizes.items()}
    p = {k: inner.data_ptr() for k, (_, inner) in buf.items()}
    _C.call('evk_relation_fwd', sd.data_ptr(), cd.data_ptr(), fd.data_ptr(), p['out'], p['r'], n, hw, c, _stream())
    _C.call('evk_relation_bwd', gd.data_ptr(), sd.data_ptr(), cd.data_ptr(), fd.data_ptr(), p['r'], p['dscene'], p['dcontent'],
            p['dfeat'], n, hw, c, p['workspace'], ws_bytes, _stream())
    torch.cuda.synchronize()
    got = {}
    for k, (whole, inner) in buf.items():
        assert guards_intact(whole, inner.numel()), f'{k}: written outside'
        got[k] = inner.cpu()
        assert not bool(torch.isnan(got[k]).any()), f'{k}: {int(torch.isnan(got[k]).sum())} of {got[k].numel()} elements unwritten'
    return got


@pytest.mark.parametrize('n,c,hw', CASES, ids=lambda v: str(v))
def test_relation_matches_fp64_as_well_as_aten_fp32_and_repeats_its_bits(cuda, n, c, hw):
    """Measured on an MI355X, kernel error / aten fp32 error (both against fp64), printed per output and case: out 1.000 in every
    case (the same product of the same two roundings), r 0.95 ... 1.00, dscene 0.90 ... 1.60 (worst: 3 x 4, 16448 pixels, whose
    sum is folded per wave, per workgroup and then over 256 partials: 4.7e-6 against 2.9e-6), dcontent 0.78 ... 1.00, dfeat
    1.00 ... 1.33.  No output uses more than 0.36 of its bound."""
    from ever_amd import _C
    scene, content, feat, dout, ref64, ref32 = _case(n, c, hw)
    dev_in = tuple(t.to(cuda) for t in (scene, content, feat, dout))
    got = _run(cuda, dev_in, n, c, hw)
    shapes = dict(out=(n, hw, c), r=(n, hw), dscene=(n, c), dcontent=(n, hw, c), dfeat=(n, hw, c))
    for k in OUTPUTS:
        as_close_as_aten(got[k].view(shapes[k]), ref64[k], ref32[k], f'relation ({n}, {c}, {hw}) {k}')
    # workgroups past the last pixel of an image leave exact zeros for the fold
    nblk = _C.load().evk_relation_workspace_bytes(1, hw, c) // (4 * c)
    ppb = -(-hw // nblk)
    empty = got['workspace'].view(n, nblk, c)[:, -(-hw // ppb):]
    if (n, c, hw) == (3, 4, 16448):
        assert (nblk, ppb, empty.shape[1]) == (256, 65, 2)
    assert bool((empty == 0).all()), 'a workgroup that owns no pixel stored a partial other than zero'
    again = _run(cuda, dev_in, n, c, hw)
    for k in OUTPUTS + ('workspace',):
        assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), f'{k}: a second call gave other bits'


def test_relation_bwd_refuses_more_than_4096_channels_without_a_launch(cuda):
    from ever_amd import _C
    n, c, hw = 1, 4100, 3
    x = torch.zeros(n * hw * c, device=cuda)
    ws_bytes = _C.load().evk_relation_workspace_bytes(n, hw, c)
    buf = [guarded(v, cuda) for v in (n * c, n * hw * c, n * hw * c, ws_bytes // 4)]
    (ds, dc, df, ws) = (inner.data_ptr() for _, inner in buf)
    rc = _C.load().evk_relation_bwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), ds, dc, df, n, hw, c,
                                    ws, ws_bytes, _stream())
    assert rc == -2 and b'relation_bwd: C=4100' in _C.load().evk_last_error()      # EVK_E_UNSUPPORTED
    torch.cuda.synchronize()
    for whole, inner in buf:
        assert guards_intact(whole, inner.numel()) and bool(torch.isnan(inner).all()), 'a refused call wrote something'
