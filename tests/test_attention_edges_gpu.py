"""The fused RoPE attention kernels (csrc/attention.hip) at their edges, called directly through the C ABI.  o, lse, dqkv and
the workspace are NaN-filled slices of sentinel-guarded, exactly sized allocations (tests/guard_common.py), and so are the
sin / cos tables' surroundings: an element nobody wrote stays NaN, a store beside a slice breaks a sentinel.

Reference: the full-tensor float64 evaluation of the reference expression on the CPU (tests/attention_common.py).
Tolerance, per case and per tensor: max(3 e_aten, 8 * 2^-23 * max|ref|), where e_aten is the max abs error of aten's own fp32
evaluation of the same expression on the CPU against the same float64 reference — a property of the reference, not of the
kernel.  (A CPU emulation of a tiled fp32 online softmax lands at 0.35-2.11 e_aten over these shapes; at N = 1 aten's output
error is 0, hence the floor.)

Shapes come from evk_attn_plan: Tq is the query tile, Tk the key tile.  q, k and v are independent asymmetric random data.  The
spiked cases carry no RoPE so that the spiked key's logit is what the test sets it to; everything else about them is as usual."""
import ctypes
import math

import pytest
import torch

from tests import attention_common as AC
from tests.guard_common import guarded, guards_intact

pytestmark = pytest.mark.gpu

# name -> (B, N, H, D, prefix, rope, data); N and prefix may be expressions of Tq, Tk and N
CASES = {
    'n1_prefix1': (1, '1', 1, 32, 'N', 'trig', 'normal'),            # a single token, none rotated
    'n1_prefix0': (2, '1', 3, 64, '0', 'trig', 'normal'),
    'n2_prefix0': (2, '2', 3, 64, '0', 'trig', 'normal'),            # every token rotated
    'tk_minus_1': (2, 'Tk-1', 3, 64, '5', 'trig', 'normal'),
    'tk': (2, 'Tk', 3, 64, '5', 'trig', 'normal'),
    'tk_plus_1': (2, 'Tk+1', 3, 64, '5', 'trig', 'normal'),          # the lone key on a second trip
    'tk_plus_1_d32': (1, 'Tk+1', 1, 32, '0', 'trig', 'normal'),
    'three_trips': (1, '2*Tk+1', 3, 32, '5', 'trig', 'normal'),
    'three_trips_d64': (2, '2*Tk+1', 1, 64, '0', 'random', 'normal'),
    'tq_minus_1': (1, 'Tq-1', 3, 32, '5', 'random', 'normal'),
    'tq_plus_1': (2, 'Tq+1', 1, 64, '5', 'random', 'normal'),
    'prefix_n': (2, 'Tk+1', 3, 64, 'N', 'trig', 'normal'),           # tables of zero rows
    'no_rope': (2, 'Tk+1', 3, 32, '0', None, 'normal'),
    'no_rope_d64': (1, 'Tq+1', 1, 64, '0', None, 'normal'),
    'random_tables_d32': (2, 'Tk+1', 3, 32, '5', 'random', 'normal'),  # the general adjoint
    'saturated': (1, '2*Tk+1', 3, 64, '5', 'trig', 'saturated'),     # the largest scaled logit > 100
    'saturated_d32': (2, 'Tk+1', 1, 32, '0', 'trig', 'saturated'),
    'spike_last_tile': (1, '2*Tk+1', 3, 64, '0', None, 'spike_last'),  # the running maximum jumps on the last trip
    'spike_second_tile': (2, '2*Tk+1', 1, 32, '0', None, 'spike_second'),
}


def _lib():
    from ever_amd import _C
    return _C.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _plan(b, n, h, d, prefix):
    out = (ctypes.c_int32 * 6)()
    assert _lib().evk_attn_plan(b, n, h, d, prefix, out) == 0
    return tuple(out)


def _resolve(name):
    b, n, h, d, prefix, rope, data = CASES[name]
    tq, tk = _plan(1, 1, h, d, 0)[:2]
    n = eval(n, {}, dict(Tq=tq, Tk=tk))
    prefix = eval(prefix, {}, dict(N=n))
    assert _plan(b, n, h, d, prefix)[2] == -(-n // tk)
    return b, n, h, d, prefix, rope, data, tk


_BUILT = {}


def _case(name):
    """inputs, the float64 reference and aten's fp32 errors; computed once per case and left unchanged"""
    if name in _BUILT:
        return _BUILT[name]
    b, n, h, d, prefix, rope, data, tk = _resolve(name)
    gen = torch.Generator().manual_seed(1000 + list(CASES).index(name))
    qkv = torch.randn(b, n, 3, h, d, generator=gen)
    d_o = torch.randn(b, n, h * d, generator=gen)
    sin = cos = None
    if rope == 'trig':
        sin, cos = AC.trig_tables(n - prefix, d, gen)
    elif rope == 'random':
        sin, cos = AC.random_tables(n - prefix, d, gen)
    scale = 1.0 / math.sqrt(d)
    if data == 'saturated':
        qkv[:, :, 0:2] *= math.sqrt(110.0 / AC.max_logit(qkv, sin, cos, prefix))   # q and k: the largest scaled logit is 110
    elif data.startswith('spike'):
        qi, kj = 3, (n - 1 if data == 'spike_last' else tk + 2)
        q = qkv[:, qi, 0]                          # [B, H, D]
        qkv[:, kj, 1] = q * (40.0 / (scale * (q * q).sum(-1, keepdim=True)))     # logit of (qi, kj) = 40
    ref = AC.evaluate(qkv, sin, cos, prefix, d_o, torch.float64, False)
    aten = AC.evaluate(qkv, sin, cos, prefix, d_o, torch.float32, True)
    if data == 'saturated':
        assert AC.max_logit(qkv, sin, cos, prefix) > 100.0
    if data.startswith('spike'):
        assert float(ref['lse'][:, :, 3].min()) > 39.0
    bound = {}
    for key in ('o', 'lse', 'dqkv'):
        e_aten = float((aten[key].double() - ref[key]).abs().max())
        bound[key] = (max(3.0 * e_aten, 8.0 * 2.0 ** -23 * float(ref[key].abs().max())), e_aten)
    _BUILT[name] = dict(dims=(b, n, h, d, prefix), qkv=qkv, d_o=d_o, sin=sin, cos=cos, ref=ref, bound=bound)
    return _BUILT[name]


def _table(t, rows, d, dev):
    """a sin / cos table in an exactly sized guarded allocation (zero rows: a valid pointer to nothing); None stays None"""
    if t is None:
        return None, None
    whole, inner = guarded(rows * d, dev)
    inner.copy_(t.reshape(-1))
    return whole, inner


def _ptr(t):
    return None if t is None else t.data_ptr()


def _fetch(whole, inner, what):
    torch.cuda.synchronize()
    assert guards_intact(whole, inner.numel()), f'{what}: wrote outside its allocation'
    got = inner.cpu()
    assert not bool(torch.isnan(got).any()), f'{what}: {int(torch.isnan(got).sum())} of {got.numel()} elements unwritten or NaN'
    return got


def _same_bits(a, b, what):
    bad = a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} of {bad.numel()} elements differ in their bits'


def _close(got, ref, bound, what):
    tol, e_aten = bound
    err = float((got.double().reshape(ref.shape) - ref).abs().max())
    print(f'{what}: max err {err:.3e}, aten {e_aten:.3e}, ratio {err / e_aten if e_aten else float("inf"):.2f}, bound {tol:.3e}')
    assert err <= tol, f'{what}: max err {err:.3e} > {tol:.3e} (aten fp32: {e_aten:.3e})'


def _forward(c, dev, with_lse):
    b, n, h, d, prefix = c['dims']
    qkv = c['qkv'].to(dev)
    sw, sin = _table(c['sin'], n - prefix, d, dev)
    cw, cos = _table(c['cos'], n - prefix, d, dev)
    ow, o = guarded(b * n * h * d, dev)
    lw, lse = guarded(b * h * n, dev) if with_lse else (None, None)
    from ever_amd import _C
    _C.call('evk_attn_fwd', qkv.data_ptr(), _ptr(sin), _ptr(cos), o.data_ptr(), _ptr(lse), b, n, h, d, prefix, _stream())
    got_o = _fetch(ow, o, 'o')
    got_lse = _fetch(lw, lse, 'lse') if with_lse else None
    for w, t in ((sw, sin), (cw, cos)):
        assert w is None or guards_intact(w, t.numel())
    return got_o, got_lse


def _backward(c, dev, o, lse):
    b, n, h, d, prefix = c['dims']
    qkv, d_o = c['qkv'].to(dev), c['d_o'].to(dev)
    _, sin = _table(c['sin'], n - prefix, d, dev)
    _, cos = _table(c['cos'], n - prefix, d, dev)
    gw, dqkv = guarded(qkv.numel(), dev)
    ws_bytes = _lib().evk_attn_bwd_workspace_bytes(b, n, h, d)
    assert ws_bytes > 0 and ws_bytes % 4 == 0
    ww, ws = guarded(ws_bytes // 4, dev)
    from ever_amd import _C
    o_d, lse_d = o.to(dev), lse.to(dev)
    _C.call('evk_attn_bwd', qkv.data_ptr(), _ptr(sin), _ptr(cos), o_d.data_ptr(), d_o.data_ptr(), lse_d.data_ptr(),
            dqkv.data_ptr(), b, n, h, d, prefix, ws.data_ptr(), ws_bytes, _stream())
    got = _fetch(gw, dqkv, 'dqkv')
    torch.cuda.synchronize()
    assert guards_intact(ww, ws.numel()), 'workspace: wrote outside its allocation'
    return got


@pytest.mark.parametrize('name', list(CASES))
def test_forward_and_backward_against_float64(name):
    dev = torch.device('cuda:0')
    c = _case(name)
    o, lse = _forward(c, dev, True)
    _close(o, c['ref']['o'], c['bound']['o'], f'{name} o')
    _close(lse, c['ref']['lse'], c['bound']['lse'], f'{name} lse')
    o_eval, _ = _forward(c, dev, False)
    _same_bits(o_eval, o, f'{name}: o without lse against o with lse')
    dqkv = _backward(c, dev, o, lse)
    _close(dqkv, c['ref']['dqkv'], c['bound']['dqkv'], f'{name} dqkv')
    o2, lse2 = _forward(c, dev, True)
    _same_bits(o2, o, f'{name}: o, second run')
    _same_bits(lse2, lse, f'{name}: lse, second run')
    _same_bits(_backward(c, dev, o, lse), dqkv, f'{name}: dqkv, second run')


def test_null_dqkv_is_nothing_to_do():
    dev = torch.device('cuda:0')
    x = torch.randn(8, device=dev)
    assert _lib().evk_attn_bwd(x.data_ptr(), None, None, None, None, None, None, 1, 1, 1, 32, 0, None, 0, _stream()) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize('what,b,n,h,d,prefix', [
    ('d48', 1, 4, 1, 48, 0), ('d128', 1, 4, 1, 128, 0), ('d16', 1, 4, 2, 16, 0), ('hd_not_4', 1, 4, 1, 6, 0),
    ('n0', 1, 0, 1, 32, 0), ('prefix_past_n', 1, 4, 1, 32, 5), ('prefix_negative', 1, 4, 1, 32, -1), ('null_qkv', 1, 4, 1, 32, 0),
    ('null_o', 1, 4, 1, 32, 0), ('sin_without_cos', 1, 4, 1, 32, 0), ('workspace_short', 1, 4, 1, 32, 0)])
def test_refusals_leave_the_outputs_untouched(what, b, n, h, d, prefix):
    dev = torch.device('cuda:0')
    lib = _lib()
    rows = max(n, 1)
    qkv = torch.randn(b * rows * 3 * h * d, device=dev)
    tab = torch.randn(rows * d, device=dev)
    ow, o = guarded(b * rows * h * d, dev)
    lw, lse = guarded(b * h * rows, dev)
    gw, dqkv = guarded(qkv.numel(), dev)
    ww, ws = guarded(b * rows * h, dev)
    q_ptr = None if what == 'null_qkv' else qkv.data_ptr()
    o_ptr = None if what == 'null_o' else o.data_ptr()
    cos_ptr = None if what == 'sin_without_cos' else tab.data_ptr()
    ws_bytes = ws.numel() * 4 - (4 if what == 'workspace_short' else 0)
    rc_f = lib.evk_attn_fwd(q_ptr, tab.data_ptr(), cos_ptr, o_ptr, lse.data_ptr(), b, n, h, d, prefix, _stream())
    rc_b = lib.evk_attn_bwd(q_ptr, tab.data_ptr(), cos_ptr, o_ptr, tab.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), b, n, h, d,
                            prefix, ws.data_ptr(), ws_bytes, _stream())
    torch.cuda.synchronize()
    if what != 'workspace_short':
        assert rc_f < 0, (what, rc_f)
    assert rc_b < 0, (what, rc_b)
    assert lib.evk_last_error()
    for whole, inner in ((ow, o), (lw, lse), (gw, dqkv), (ww, ws)):
        if what == 'workspace_short' and (inner is o or inner is lse):     # (that forward is a valid call and ran)
            continue
        assert guards_intact(whole, inner.numel())
        assert bool(torch.isnan(inner).all()), f'{what}: a refused call wrote an output'
