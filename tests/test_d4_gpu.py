"""The dihedral kernels of csrc/d4.hip at their dispatch edges, through the C ABI into NaN-filled, sentinel-guarded outputs
(tests/guard_common.py): nothing outside the result may be written, nothing inside it may stay unwritten.  The cases come from
tests/tta_common.py; tests/test_transform_cpu.py holds each of them on the kernel it names.

evk_d4_apply is a permutation of 32-bit words: inputs are random bit patterns (NaNs with payloads, infinities, -0.0, denormals
among them) and the result is compared bit for bit with the op's torch expression on the CPU.  evk_d4_merge is compared bit for
bit with the reference's `sum(outs) / len(outs)` on the CPU (sequential fp32 adds from an integer 0, then a true division) on
values randn * 2^randint(-6, 6), where a reciprocal multiply or another order of additions differs on a third of the elements
and more.  No tolerance anywhere in this file."""
import ctypes
import functools

import pytest
import torch

from tests import tta_common as tc
from tests.guard_common import guarded, guards_intact

pytestmark = pytest.mark.gpu

FILL_NAN = 0x7fc00000       # the word guarded() fills a result with
SPECIALS = (0x7fc00001, 0x7f800001, 0xffc12345, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff, 0x00000000)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from ever_amd import _C
    return _C.load()


def _words(gen, *shape):
    """random 32-bit patterns as int32, the special values sprinkled in, none equal to the fill word"""
    w = torch.randint(-2 ** 31, 2 ** 31, shape, generator=gen, dtype=torch.int64)
    flat = w.view(-1)
    idx = torch.randperm(flat.numel(), generator=gen)[:max(1, flat.numel() // 4)]
    sp = torch.tensor(SPECIALS, dtype=torch.int64)
    flat[idx] = sp[torch.arange(idx.numel()) % len(SPECIALS)]
    flat[(flat & 0xffffffff) == FILL_NAN] = FILL_NAN + 1
    return ((w + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32)


def _ref_nhwc(x, op):
    """the op's torch expression on a CPU [N, H, W, C] tensor"""
    return tc.d4_ref(x.permute(0, 3, 1, 2), op).permute(0, 2, 3, 1).contiguous()


def _fetch_words(whole, inner, what):
    torch.cuda.synchronize()
    assert guards_intact(whole, inner.numel()), f'{what}: wrote outside its output'
    got = inner.view(torch.int32).cpu()
    left = int((got == FILL_NAN).sum())
    assert left == 0, f'{what}: left {left} of {got.numel()} elements unwritten'
    return got


def _same_words(got, ref, what):
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    bad = got != ref
    assert not bool(bad.any()), (f'{what}: {int(bad.sum())} of {bad.numel()} words differ, first at '
                                 f'{tuple(int(v) for v in bad.nonzero()[0])}: {int(got[bad][0]) & 0xffffffff:#010x} vs '
                                 f'{int(ref[bad][0]) & 0xffffffff:#010x}')


def _apply(lib, xd, n, h, w, c, op, what):
    ho, wo = (w, h) if op & 1 else (h, w)
    whole, inner = guarded(n * h * w * c, xd.device)
    rc = lib.evk_d4_apply(xd.data_ptr(), inner.data_ptr(), n, h, w, c, op, _stream())
    assert rc == 0, (what, lib.evk_last_error())
    return _fetch_words(whole, inner, what).view(n, ho, wo, c)


# ------------------------------------------------------------------------------------------------ apply
@pytest.mark.parametrize('case', tc.APPLY_CASES, ids=tc.apply_id)
def test_apply_permutes_words_and_its_inverse_undoes_it(cuda, case):
    n, h, w, c, op, kernel = case
    lib = _lib()
    assert tc.plan(lib, n, h, w, c, op)[0] == kernel
    x = _words(torch.Generator().manual_seed(h * 1000 + w * 10 + c + op), n, h, w, c)
    y = _apply(lib, x.to(cuda), n, h, w, c, op, tc.apply_id(case))
    _same_words(y, _ref_nhwc(x, op), tc.apply_id(case))
    back = _apply(lib, y.to(cuda), n, y.shape[1], y.shape[2], c, tc.INVERSE[op], tc.apply_id(case) + ' inverse')
    _same_words(back, x, tc.apply_id(case) + ' inverse')


@pytest.mark.parametrize('case', tc.FORCED_CASES, ids=tc.apply_id)
def test_apply_on_a_forced_kernel(cuda, case):
    """the kernels only evk_d4_force_kernel reaches: the tile past the crossover, the element kernels on a narrow swap"""
    n, h, w, c, op, kernel = case
    lib = _lib()
    with tc.forced(lib, kernel):
        assert tc.plan(lib, n, h, w, c, op)[0] == kernel
        x = _words(torch.Generator().manual_seed(7 * h + w + c + op), n, h, w, c)
        y = _apply(lib, x.to(cuda), n, h, w, c, op, tc.apply_id(case))
    _same_words(y, _ref_nhwc(x, op), tc.apply_id(case))


@pytest.mark.parametrize('layout', ['nhwc', 'nchw', 'strided'])
@pytest.mark.parametrize('op', range(8))
def test_wrapper_keeps_the_layout_and_differentiates(cuda, op, layout):
    """HF.d4 on a dense-NHWC tensor, on an NCHW-contiguous one (the [N*C, H, W, 1] alias: no conversion) and on a slice; the
    backward is d4(g, inverse(op)) bit for bit"""
    from ever_amd.hip import functional as HF
    n, c, h, w = 2, 6, 31, 33
    gen = torch.Generator().manual_seed(op)
    xw = _words(gen, n, c, h, w + (3 if layout == 'strided' else 0))
    ho, wo = (w, h) if op & 1 else (h, w)
    gw = _words(gen, n, c, ho, wo)
    x = xw.view(torch.float32).to(cuda)
    if layout == 'nhwc':
        x = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    elif layout == 'strided':
        x, xw = x[..., 3:], xw[..., 3:]
    x.requires_grad_()
    y = HF.d4(x, op)
    assert y.shape == (n, c, ho, wo)
    assert HF.is_nhwc(y) if layout == 'nhwc' else y.is_contiguous()
    _same_words(y.detach().contiguous().view(torch.int32).cpu(), tc.d4_ref(xw, op).contiguous(), f'd4 op {op} {layout}')
    y.backward(gw.view(torch.float32).to(cuda))
    assert x.grad.shape == x.shape
    _same_words(x.grad.contiguous().view(torch.int32).cpu(), tc.d4_ref(gw, tc.INVERSE[op]).contiguous(),
                f'd4 backward op {op} {layout}')


# ------------------------------------------------------------------------------------------------ merge
@functools.lru_cache(maxsize=None)
def _merge_case(n, c, ho, wo, nt, kind):
    """NHWC fp32 terms, their ops, and the reference's plain sum and mean on the CPU; shared, never written to"""
    gen = torch.Generator().manual_seed(ho * 1000 + wo * 10 + c + nt)
    ops = tc.merge_ops(nt, kind)
    terms = []
    for op in ops:
        hk, wk = (wo, ho) if op & 1 else (ho, wo)
        terms.append(torch.randn(n, hk, wk, c, generator=gen)
                     * torch.pow(2.0, torch.randint(-6, 7, (n, hk, wk, c), generator=gen).float()))
    outs = [_ref_nhwc(t, op) for t, op in zip(terms, ops)]
    return terms, ops, sum(outs), sum(outs) / len(outs)


def _merge(lib, tds, ops, acc, y, n, ho, wo, c, count):
    tp = (ctypes.c_void_p * len(tds))(*[t.data_ptr() for t in tds])
    op = (ctypes.c_int32 * len(tds))(*ops)
    rc = lib.evk_d4_merge(tp, op, len(tds), None if acc is None else acc.data_ptr(), y.data_ptr(), n, ho, wo, c, count,
                          _stream())
    assert rc == 0, lib.evk_last_error()


def _merge_chain(lib, tds, ops, dims, count, cuda, what):
    """the whole list in launches of 16 terms, each into its own guarded result, chained through acc"""
    n, ho, wo, c = dims
    acc = None
    for i in range(0, len(tds), tc.MAX_TERMS):
        last = i + tc.MAX_TERMS >= len(tds)
        whole, inner = guarded(n * ho * wo * c, cuda)
        _merge(lib, tds[i:i + tc.MAX_TERMS], ops[i:i + tc.MAX_TERMS], acc, inner, n, ho, wo, c, count if last else 0)
        got = _fetch_words(whole, inner, what)
        acc = inner
    return got.view(n, ho, wo, c)


@pytest.mark.parametrize('case', tc.MERGE_CASES, ids=tc.merge_id)
def test_merge_equals_the_reference_expression_bit_for_bit(cuda, case):
    n, c, ho, wo, nt, kind, kernel = case
    lib = _lib()
    terms, ops, ref_sum, ref_mean = _merge_case(n, c, ho, wo, nt, kind)
    assert tc.merge_kernel(lib, n, c, ho, wo, ops[:tc.MAX_TERMS]) == kernel
    tds = [t.to(cuda) for t in terms]
    got = _merge_chain(lib, tds, ops, (n, ho, wo, c), nt, cuda, tc.merge_id(case))
    _same_words(got, ref_mean.view(torch.int32), tc.merge_id(case) + ' mean')
    # count = 0 leaves the plain sum
    got = _merge_chain(lib, tds, ops, (n, ho, wo, c), 0, cuda, tc.merge_id(case))
    _same_words(got, ref_sum.view(torch.int32), tc.merge_id(case) + ' sum')


@pytest.mark.parametrize('case', [tc.MERGE_CASES[0], tc.MERGE_CASES[7], tc.MERGE_CASES[11]], ids=tc.merge_id)
def test_merge_of_negative_zeros_is_positive_zero(cuda, case):
    """`0 + (-0.0)` is +0.0: the sum starts from 0.0f, not from the first term"""
    n, c, ho, wo, _, kind, _ = case
    lib = _lib()
    for nt in (1, 3):
        ops = tc.merge_ops(nt, kind)
        tds = [torch.full((n, ho * wo * c), -0.0, device=cuda) for _ in ops]
        got = _merge_chain(lib, tds, ops, (n, ho, wo, c), nt, cuda, 'negative zeros')
        assert bool((got == 0).all()), f'{int((got != 0).sum())} words are not +0.0, e.g. {int(got[got != 0][0]) & 0xffffffff:#x}'


@pytest.mark.parametrize('case', [tc.MERGE_CASES[3], tc.MERGE_CASES[7], tc.MERGE_CASES[10], tc.MERGE_CASES[13]],
                         ids=tc.merge_id)
def test_merge_may_write_over_its_accumulator(cuda, case):
    n, c, ho, wo, nt, kind, kernel = case
    lib = _lib()
    terms, ops, _, _ = _merge_case(n, c, ho, wo, nt, kind)
    assert tc.merge_kernel(lib, n, c, ho, wo, ops) == kernel
    tds = [t.to(cuda) for t in terms]
    accv = torch.randn(n, ho, wo, c, generator=torch.Generator().manual_seed(3))
    outs = [_ref_nhwc(t, op) for t, op in zip(terms, ops)]
    ref = accv
    for o in outs:
        ref = ref + o
    ref = ref / nt
    whole, inner = guarded(accv.numel(), cuda)
    inner.copy_(accv.view(-1))
    _merge(lib, tds, ops, inner, inner, n, ho, wo, c, nt)
    torch.cuda.synchronize()
    assert guards_intact(whole, inner.numel())
    _same_words(inner.view(torch.int32).cpu().view(n, ho, wo, c), ref.view(torch.int32), 'y aliases acc')


@pytest.mark.parametrize('layout', ['nhwc', 'nchw', 'mixed'])
def test_wrapper_mean_in_either_layout(cuda, layout):
    """HF.d4_mean on 17 terms (two launches): dense-NHWC terms, NCHW-contiguous terms ([N*C, H, W, 1]: no conversion), and a
    list whose terms do not share a layout (brought to the first term's)"""
    from ever_amd.hip import functional as HF
    n, c, ho, wo, nt = 2, 6, 20, 12, 17
    terms, ops, _, ref_mean = _merge_case(n, c, ho, wo, nt, 'mixed')
    ref = ref_mean.permute(0, 3, 1, 2)
    tds = []
    for k, t in enumerate(terms):
        t = t.to(cuda).permute(0, 3, 1, 2)            # logical NCHW over NHWC memory
        if layout == 'nchw' or (layout == 'mixed' and k % 2):
            t = t.contiguous()
        tds.append(t)
    before = dict(HF.d4_stats)
    with torch.no_grad():
        y = HF.d4_mean(tds, ops)
    assert y.shape == (n, c, ho, wo)
    assert y.is_contiguous() if layout == 'nchw' else HF.is_nhwc(y)
    assert HF.d4_stats['mean'] == before['mean'] + 1 and HF.d4_stats['mean_launches'] == before['mean_launches'] + 2
    _same_words(y.contiguous().view(torch.int32).cpu(), ref.contiguous().view(torch.int32), f'd4_mean {layout}')
    with pytest.raises(HF.HipPathError):
        HF.d4_mean([tds[0].clone().requires_grad_()], [ops[0]])
    with pytest.raises(ValueError):
        HF.d4_mean(tds[:2], [ops[0], ops[0]])       # the second term's dims do not fit
