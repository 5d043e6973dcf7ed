"""Shared by tests/test_conv_launches_gpu.py and tools/gen_golden_conv_launches.py: what the convolution host wrappers
(ever_amd/hip/conv.py, module/fold.py) LAUNCH for a table of small cases, one per branch of their dispatch.

`record(name)` replaces `ever_amd._C.call` — every family module calls it as `_C.call` — for the duration of one case and
stores, per call, the entry name and its arguments read through `_C.SIGNATURES[name]`: a descriptor as its 15 fields, integers
and floats as values, pointers as 0 (null) / 1, by-reference integers not at all, and the last argument, the stream, as 'main'
(the raw stream that was current when the case began) or 'side'.  With them the per-case deltas of `absmax_stats`,
`relu_bits_stats` and `wgrad_stream_stats`.  A case starts from fresh tensors and an empty plane cache and ends joined and
synchronised, so its record does not depend on the cases before it; forward and backward both run inside the recorded region.
Branches are forced with the module switches, not with large maps."""
import contextlib
import ctypes
import json
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_launches.json')
MATHS = ('f16x2', 'bf16x3', 'bf16', 'f32')
_STATS = ('absmax_stats', 'relu_bits_stats', 'wgrad_stream_stats')
_INTS = (ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_size_t)


def _arg(ctype, a, is_stream, main):
    from ever_amd import _C
    if ctype is _C._DP:
        return [int(getattr(a._obj, f)) for f, _ in _C.ConvDesc._fields_]
    if ctype is ctypes.c_void_p:
        a = getattr(a, 'value', a)
        if is_stream:
            return 'main' if (a or 0) == main else 'side'
        return 0 if not a else 1
    if ctype in _INTS:
        return int(getattr(a, 'value', a))
    if ctype is ctypes.c_float:
        return float(getattr(a, 'value', a))
    return None          # by-reference integers, job arrays: not part of the record


@contextlib.contextmanager
def _switches(math='f16x2', tr_min_hw=128 * 128, pack_gain=1.0, early=0, packed=True, lazy_res=True, batch=1, side=True):
    """every switch a case depends on, set for its duration (the defaults are the production ones) and put back"""
    from ever_amd.hip import conv
    from ever_amd.hip import functional as HF
    prev = (HF.set_conv_math(math), conv._WGRAD_TR_MIN_HW, conv._WGRAD_PACK_GAIN, HF._WGRAD_EARLY_MODE, HF._PACKED,
            HF._LAZY_RES, HF._WGRAD_BATCH[0], HF.set_wgrad_stream(side))
    conv._WGRAD_TR_MIN_HW, conv._WGRAD_PACK_GAIN = tr_min_hw, pack_gain
    HF._WGRAD_EARLY_MODE, HF._PACKED, HF._LAZY_RES, HF._WGRAD_BATCH[0] = early, packed, lazy_res, batch
    try:
        yield
    finally:
        HF.set_conv_math(prev[0])
        conv._WGRAD_TR_MIN_HW, conv._WGRAD_PACK_GAIN = prev[1], prev[2]
        HF._WGRAD_EARLY_MODE, HF._PACKED, HF._LAZY_RES, HF._WGRAD_BATCH[0] = prev[3:7]
        HF.set_wgrad_stream(prev[7])


def record(name, dev):
    """{'calls': [[entry, arg, ...], ...], '<stats>': {key: delta}} of CASES[name]"""
    from ever_amd import _C
    from ever_amd.hip import functional as HF
    from ever_amd.hip import weight_planes
    run, switches = CASES[name]
    calls = []
    real = _C.call
    with _switches(**switches):
        weight_planes.clear()
        torch.cuda.synchronize()
        main = HF._stream()
        before = {s: dict(getattr(HF, s)) for s in _STATS}

        def spy(entry, *args):
            types = _C.SIGNATURES[entry][1]
            assert len(types) == len(args), entry
            row = [entry]
            for i, (t, a) in enumerate(zip(types, args)):
                v = _arg(t, a, i == len(args) - 1, main)
                if v is not None:
                    row.append(v)
            calls.append(row)
            return real(entry, *args)
        _C.call = spy
        try:
            torch.manual_seed(1234)
            run(dev)
            HF.wait_wgrad_stream()
            torch.cuda.synchronize()
        finally:
            _C.call = real
        out = {'calls': calls}
        for s in _STATS:
            out[s] = {k: v - before[s][k] for k, v in getattr(HF, s).items()}
    return out


def flag_word(row):
    """the flag word (the one uint32 argument) of a recorded call"""
    from ever_amd import _C
    kept = [t for t in _C.SIGNATURES[row[0]][1] if t is _C._DP or t is ctypes.c_void_p or t in _INTS or t is ctypes.c_float]
    (i,) = [i for i, t in enumerate(kept) if t is ctypes.c_uint32]
    return row[1 + i]


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


# ---------------------------------------------------------------------------------------------------------- the cases
CASES = {}


def _case(name, **switches):
    def deco(fn):
        assert name not in CASES, name
        CASES[name] = (fn, switches)
        return fn
    return deco


def _x(dev, n, c, h, w, grad=True):
    return torch.randn(n, c, h, w, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(grad)


def _w(dev, cout, cin, k, channels_last=True):
    w = torch.randn(cout, cin, k, k, device=dev) / (cin * k * k) ** 0.5
    return (w.contiguous(memory_format=torch.channels_last) if channels_last else w).requires_grad_()


def _b(dev, cout):
    return torch.randn(cout, device=dev).requires_grad_()


def _back(*ys):
    sum((y * y).sum() for y in ys).backward()


def _conv(dev, cin, cout, k=3, n=2, hw=8, bias=True, relu=False, channels_last=True, **kw):
    from ever_amd.hip import functional as HF
    y = HF.conv2d(_x(dev, n, cin, hw, hw), _w(dev, cout, cin, k, channels_last), _b(dev, cout) if bias else None,
                  padding=k // 2, relu=relu, **kw)
    _back(y)


def _bn_params(dev, c):
    return (torch.rand(c, device=dev) + 0.5).requires_grad_(), (torch.randn(c, device=dev) * 0.1).requires_grad_()


# 1. the four arithmetics; 2. channel padding and narrow outputs; 3. a handful of GEMM rows
for _m in MATHS:
    _case(f'plain_{_m}', math=_m)(lambda dev: _conv(dev, 16, 16, relu=True))
_case('pad_cin3')(lambda dev: _conv(dev, 3, 16, bias=False))
_case('narrow8_cout1')(lambda dev: _conv(dev, 16, 1, k=1))
_case('pad_cin3_cout5')(lambda dev: _conv(dev, 3, 5))
_case('pad_cin3_cout5_f32', math='f32')(lambda dev: _conv(dev, 3, 5))
_case('small_m_1x1')(lambda dev: _conv(dev, 64, 64, k=1, hw=1))


# 4. statistics records from the epilogue, and the "packed dy" field the BatchNorm's backward acts on
def _conv_bn(dev, cout, relu, bias):
    from ever_amd.hip import functional as HF
    y = HF.conv2d(_x(dev, 2, 16, 8, 8), _w(dev, cout, 16, 3), _b(dev, cout) if bias else None, padding=1, relu=relu,
                  bn_stats=True)
    gm, bt = _bn_params(dev, cout)
    _back(HF.batch_norm_act(y, gm, bt, None, None, True, 0.1, 1e-5, relu=True))


for _cout in (64, 68):
    for _relu in (False, True):
        for _bias in (False, True):
            _case(f'stats_cout{_cout}_relu{int(_relu)}_bias{int(_bias)}')(
                lambda dev, c=_cout, r=_relu, b=_bias: _conv_bn(dev, c, r, b))
_case('stats_cout64_bf16x3', math='bf16x3')(lambda dev: _conv_bn(dev, 64, False, False))
_case('stats_cout64_bf16', math='bf16')(lambda dev: _conv_bn(dev, 64, False, False))


# 5. BatchNorm -> convolution: the input arrives packed, and so does the output gradient
def _chain(dev, width=64, tail_bn=True):
    """(512 rows: the BatchNorm pass stores its output packed from 256 rows on.)  tail_bn=False: the second convolution's
    output gradient comes from the loss, in fp32, so only its input is packed."""
    import ever_amd as er
    from ever_amd.hip import functional as HF
    convs = [er.module.Conv2d(width, width, 3, padding=1, bias=False).to(dev) for _ in range(2)]
    bns = [er.module.BatchNorm2d(width).to(dev).train() for _ in range(2)]
    h = _x(dev, 2, width, 16, 16)
    h = bns[0](convs[0](h, bn_stats=True), relu=True, conv_only=True)
    assert HF._is_packed(h) == (HF._PACKED and HF.get_conv_math() == 'f16x2')
    _back(bns[1](convs[1](h, bn_stats=True), relu=True) if tail_bn else convs[1](h))


_case('chain_packed')(_chain)
_case('chain_fp32_operands', packed=False)(_chain)
_case('chain_packed_x_fp32_dy')(lambda dev: _chain(dev, tail_bn=False))


# 6. conv2d_fork
def _layer(dev, cin, cout, k, stride=1):
    import ever_amd as er
    return er.module.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=False).to(dev)


def _fork_identity(dev):
    from ever_amd.hip import functional as HF
    y, s = HF.conv2d_fork(_x(dev, 2, 64, 8, 8), _layer(dev, 64, 64, 3), bn_stats=(True, False))
    gm, bt = _bn_params(dev, 64)
    _back(HF.batch_norm_act(y, gm, bt, None, None, True, 0.1, 1e-5, residual=s, relu=True, lazy_res=True))


def _fork_short(dev, stride, only_second=False):
    from ever_amd.hip import functional as HF
    y, s = HF.conv2d_fork(_x(dev, 2, 16, 8, 8), _layer(dev, 16, 32, 3, stride), _layer(dev, 16, 32, 1, stride))
    _back(s) if only_second else _back(y, s)


_case('fork_identity_lazy_bits')(_fork_identity)
_case('fork_identity_bits_materialised', lazy_res=False)(_fork_identity)
_case('fork_strided_1x1_shortcut')(lambda dev: _fork_short(dev, 2))
_case('fork_stride1_shortcut')(lambda dev: _fork_short(dev, 1))
_case('fork_only_second_branch')(lambda dev: _fork_short(dev, 1, only_second=True))


# 7. a claimed gradient slot
def _slot_conv2d(dev):
    from ever_amd.hip import functional as HF
    x, slot = _x(dev, 2, 16, 8, 8), HF.GradSlot()
    y = HF.conv2d(x, _w(dev, 16, 16, 3), None, padding=1, grad_slot=slot)
    assert slot.claimed
    _back(y, HF.slot_output(x, slot))


def _slot_fork(dev):
    from ever_amd.hip import functional as HF
    x, slot = _x(dev, 2, 16, 8, 8), HF.GradSlot()
    x._evk_grad_slot = slot
    y, s = HF.conv2d_fork(x, _layer(dev, 16, 32, 3), _layer(dev, 16, 32, 1))
    del x._evk_grad_slot
    assert slot.claimed
    _back(y, s, HF.slot_output(x, slot))


_case('slot_conv2d')(_slot_conv2d)
_case('slot_fork')(_slot_fork)

# 8. the weight gradient behind the planar pack, forked behind / in front of its data gradient
for _early in (0, 1, 2):
    _case(f'wgrad_planar_early{_early}', tr_min_hw=1024, early=_early)(
        lambda dev: _conv(dev, 64, 128, n=1, hw=32, bias=False))
# (EVK_WGRAD_EARLY=1 forks every layer's weight gradient first, the planar ones or not)
_case('wgrad_early1_not_planar', early=1)(lambda dev: _conv(dev, 16, 16, bias=False))

# 9. the weight gradient behind the plain pack
_case('wgrad_pack_both', pack_gain=1e9)(lambda dev: _conv(dev, 16, 16, bias=False))
_case('wgrad_pack_x_already_packed', pack_gain=1e9)(lambda dev: _chain(dev, tail_bn=False))
_case('wgrad_pack_both_already_packed', pack_gain=1e9)(_chain)
_case('wgrad_pack_refused_by_bias_gradient', pack_gain=1e9)(lambda dev: _conv(dev, 16, 16, bias=True))


# 10. where the weight gradient is launched
def _stack(dev):
    from ever_amd.hip import functional as HF
    h = _x(dev, 2, 16, 8, 8)
    for _ in range(3):
        h = HF.conv2d(h, _w(dev, 16, 16, 3), None, padding=1)
    _back(h)


_case('wgrad_main_stream', side=False)(lambda dev: _conv(dev, 16, 16))
_case('wgrad_batched_stack', batch=4)(_stack)
_case('wgrad_batched_chain_packed', batch=4)(_chain)       # (the packed flag of x is among what is resolved when queued)
_case('wgrad_stack_unbatched')(_stack)
_case('wgrad_param_strides_break_the_contract')(lambda dev: _conv(dev, 16, 16, channels_last=False))


# 11. transposed convolution
def _transpose(dev, k=2):
    from ever_amd.hip import functional as HF
    w = (torch.randn(8, 8, k, k, device=dev) * 0.2).contiguous(memory_format=torch.channels_last).requires_grad_()
    _back(HF.conv_transpose2d(_x(dev, 2, 8, 8, 8), w, _b(dev, 8), stride=2))


_case('transpose_f16x2')(_transpose)
_case('transpose_f32', math='f32')(_transpose)
_case('transpose_1x1_f16x2')(lambda dev: _transpose(dev, 1))


# 12. the stem
def _stem(dev, bn_stats):
    from ever_amd.hip import functional as HF
    _back(HF.stem_conv7x7s2(_x(dev, 2, 4, 16, 16, grad=False), _w(dev, 64, 4, 7), bn_stats=bn_stats))


for _m in ('f16x2', 'bf16x3', 'bf16'):
    for _stats in (False, True):
        _case(f'stem_{_m}_stats{int(_stats)}', math=_m)(lambda dev, s=_stats: _stem(dev, s))


# 13. the folded inference convolution
def _folded(dev, cin, residual):
    import ever_amd as er
    from ever_amd.module import fold
    conv = er.module.Conv2d(cin, 16, 3, padding=1, bias=False).to(dev)
    fold.fold_batchnorm(torch.nn.Sequential(conv, er.module.BatchNorm2d(16).to(dev)))
    with torch.no_grad():
        res = _x(dev, 2, 16, 8, 8, grad=False) if residual else None
        fold.folded_conv2d(_x(dev, 2, cin, 8, 8, grad=False), conv, residual=res, relu=True)


for _cin in (3, 16):
    for _res in (False, True):
        _case(f'folded_cin{_cin}_res{int(_res)}')(lambda dev, c=_cin, r=_res: _folded(dev, c, r))
_case('folded_cin16_res1_bf16x3', math='bf16x3')(lambda dev: _folded(dev, 16, True))
_case('folded_cin16_res1_f32', math='f32')(lambda dev: _folded(dev, 16, True))

# every entry the table has to reach, and both streams of a weight gradient (tests/test_conv_launches_gpu.py)
REQUIRED_ENTRIES = {
    'evk_pack_planar_f16x2', 'evk_pack_f16x2', 'evk_conv2d_dgrad_f16x2_masked', 'evk_conv2d_dgrad_f16x2_ex',
    'evk_conv2d_pack_dgrad_weight', 'evk_pad_channels', 'evk_unpad_channels', 'evk_relu_bwd', 'evk_conv2d_fwd_x3_stats',
    'evk_conv2d_fwd_bf16', 'evk_conv2d_wgrad_f16x2', 'evk_conv2d_wgrad_f16x2_ex', 'evk_conv_transpose2d_wgrad_x3',
    'evk_stem_s2d_weight_bwd',
}
WGRAD_ENTRIES = ('evk_conv2d_wgrad', 'evk_conv2d_wgrad_x3', 'evk_conv2d_wgrad_bf16', 'evk_conv2d_wgrad_f16x2',
                 'evk_conv2d_wgrad_f16x2_ex')
