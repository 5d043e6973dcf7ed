"""dev tool / test helper: the large forward / data-gradient tile forms forced onto small ragged shapes, against float64.

usage: <family environment> python tools/check_tiles.py generic|halo [force ...]

tests/conv_tiles_common.py holds the cases, the forces and the instantiation each (case, force, arithmetic, direction) must
take; tests/test_conv_tiles_gpu.py runs this in a child process per family (the routing switches are read once per process;
under EVK_TUNE the force variable is re-read on every launch, so the forces are switched here, in-process).

Part 1, per case, force and arithmetic (f16x2, bf16x3, bf16): the route evk_conv2d_route names must be the table's — a force
that fell back fails — then ever_amd.hip.functional.conv2d forward and backward, y and dx against the float64 reference of
tests/test_conv_geometry_gpu.py (its inputs, its ReLU-kink masking, its bounds: e = max|hip - ref64| / max|ref64| <=
max(4 e32, 5e-6), e32 the same error of torch's fp32 CPU convolution; plain bf16: 2e-2).

Part 2, raw C-ABI, f16x2, the table's `raw` cases under each force: packed activations (forward flag 2, data gradient flag 4:
the NPX = 4 instantiations) bit for bit equal to the fp32 operand; the statistics epilogue against the output it wrote (mean
1e-6, variance 1e-5, tools/check_dma.py's bounds; it engages only where Cout is whole tiles: the `stats` cases, where it
must, with one record per row tile of the forced form); the accumulate epilogue of the data gradient against float64.  Outputs
and records are NaN-filled slices between sentinels (tests/guard_common.py): an element nobody wrote or a store beside the
tensor fails."""
import ctypes, os, re, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import conv_tiles_common as T  # noqa: E402
from tests.guard_common import guarded, guards_intact  # noqa: E402
from tests.test_conv_geometry_gpu import BF16_GRADE, _inputs, _reference  # noqa: E402
from ever_amd import _C  # noqa: E402
from ever_amd.hip import functional as HF  # noqa: E402

family = sys.argv[1]
ENV, VAR, FORCES, CASES = T.FAMILIES[family]
forces = sys.argv[2:] or list(FORCES)
assert all(os.environ.get(k) == v for k, v in ENV.items()), f'{family}: run with {ENV}'
dev = torch.device('cuda:0')
lib = _C.load()
worst, bad = {}, []


def rel(a, ref):   # on the device, in float64
    return float((a.detach().double() - ref).abs().max() / ref.abs().max())


def note(what, name, e, bound, extra=''):
    print(f'{what:32s} {name:46s} e {e:.2e} / bound {bound:.2e} {extra}')
    direction = 'dgrad' if what.endswith(' dx') else 'fwd'
    for nm in name.split(' | '):
        if e / bound > worst.get((nm, direction), (-1.0,))[0]:
            worst[nm, direction] = (e / bound, what, e, bound)
    if not e <= bound:
        bad.append((what, name, e, bound))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def row_tiles(name, c):
    """row tiles (patches) of the named instantiation on a raw case = statistics records it writes: the launch itself, not
    only evk_conv2d_route, took the forced tile"""
    m = re.match(r'conv_igemm_x3(?:ws)?_kernel<(\d+),', name)
    if m:
        return -(-c['n'] * c['h'] * c['w'] // int(m.group(1)))
    ph = int(re.match(r'conv3x3_halo_x3_kernel<\d+, (\d+),', name).group(1))
    return c['n'] * -(-c['h'] // ph) * -(-c['w'] // 16)


t0 = time.time()
refs = {}
for c in CASES:   # float64 / fp32 references on the CPU, once per case (plain bf16 has its own ReLU band)
    refs[c['name'], False] = _reference(c, False)
    refs[c['name'], True] = _reference(c, True) if c['relu'] else refs[c['name'], False]
t_ref = time.time() - t0

# ---- part 1: through the Python layer, every arithmetic -----------------------------------------------------------------
t0 = time.time()
for c in CASES:
    _, x, wt, b = _inputs(c)
    xg = x.to(dev).requires_grad_(True)
    wg = wt.to(dev).contiguous(memory_format=torch.channels_last)
    bg = b.to(dev) if b is not None else None
    for mode, planes in T.ARITH.items():
        r64, e32, gy = refs[c['name'], mode == 'bf16']
        y64, dx64, gyg = r64['y'].to(dev), r64['dx'].to(dev), gy.to(dev)
        prev = HF.set_conv_math(mode)
        try:
            for force in forces:
                os.environ[VAR] = force
                fwd, dgrad = T.routed(lib, c, planes)
                want = T.expected(family, c, force, mode)
                assert (fwd, dgrad) == want, (c['name'], force, mode, (fwd, dgrad), want)
                y = HF.conv2d(xg, wg, bg, stride=c['s'], padding=c['p'], dilation=c['dil'], relu=c['relu'])
                dx, = torch.autograd.grad(y, xg, gyg)
                torch.cuda.synchronize()
                assert y.shape == y64.shape and dx.shape == dx64.shape
                assert torch.isfinite(y).all() and torch.isfinite(dx).all(), (c['name'], force, mode)
                for k, got, ref, name in (('y', y, y64, fwd), ('dx', dx, dx64, ' | '.join(sorted(set(dgrad))))):
                    bound = BF16_GRADE if mode == 'bf16' else max(4 * e32[k], 5e-6)
                    note(f"{c['name']} {force} {mode} {k}", name, rel(got, ref), bound, f'(e32 {e32[k]:.2e})')
        finally:
            HF.set_conv_math(prev)
            os.environ[VAR] = ''
t_py = time.time() - t0

# ---- part 2: raw C-ABI, f16x2: packed operands, statistics epilogue, accumulate epilogue -----------------------------------
t0 = time.time()
st = torch.cuda.current_stream().cuda_stream
aws = torch.zeros(lib.evk_absmax_workspace_bytes(), dtype=torch.uint8, device=dev)


def scale(t):
    b = torch.zeros(int(lib.evk_absmax_words()), dtype=torch.int32, device=dev)
    _C.call('evk_absmax', t.data_ptr(), t.numel(), b.data_ptr(), aws.data_ptr(), st)
    return b


def pack(t, bits):
    p = torch.empty_like(t)
    _C.call('evk_pack_f16x2', t.data_ptr(), t.numel(), bits.data_ptr(), p.data_ptr(), st)
    return p


for c in [c for c in CASES if c.get('raw')]:
    assert not c['relu'] and c['s'] == (1, 1)
    n, h, w, cin, cout = c['n'], c['h'], c['w'], c['cin'], c['cout']
    d = _C.ConvDesc(*T.desc_args(c, 2))
    g, x, wt, b = _inputs(c)
    r64, e32, gy = refs[c['name'], False]
    x, wt, dy = nhwc(x).to(dev), nhwc(wt).to(dev), nhwc(gy).to(dev)
    bg = b.to(dev) if b is not None else None
    acc = torch.randn(n, h, w, cin, generator=torch.Generator().manual_seed(5)).to(dev)
    y64 = nhwc(r64['y']).to(dev)
    dxa64 = nhwc(r64['dx']).to(dev) + acc.double()
    # the fp32 convolution's error is e32 of max|dx|; of max|dx + acc| it is that times max|dx| / max|dx + acc|, and the one
    # rounding of the add (2^-24) is left out: not above the bound as tests/test_conv_geometry_gpu.py states it
    e32a = e32['dx'] * float(r64['dx'].abs().max()) / float(dxa64.abs().max())
    bx, bw, bdy = scale(x), scale(wt), scale(dy)
    xp, dyp = pack(x, bx), pack(dy, bdy)
    pf = torch.empty(lib.evk_conv2d_split_weight_bytes(ctypes.byref(d), 0), dtype=torch.uint8, device=dev)
    pd = torch.empty(lib.evk_conv2d_split_weight_bytes(ctypes.byref(d), 1), dtype=torch.uint8, device=dev)
    _C.call('evk_conv2d_split_weight_f16x2', ctypes.byref(d), wt.data_ptr(), 0, pf.data_ptr(), bw.data_ptr(), st)
    _C.call('evk_conv2d_split_weight_f16x2', ctypes.byref(d), wt.data_ptr(), 1, pd.data_ptr(), bw.data_ptr(), st)
    cap = int(lib.evk_conv2d_stats_max_parts(ctypes.byref(d)))
    for force in forces:
        os.environ[VAR] = force
        outs = []
        for src, packed in ((x, False), (xp, True)):
            want = T.expected(family, c, force, 'f16x2', packed)
            for stats in (0, 1):
                got = T.routed(lib, c, 2, packed, stats=stats)
                assert got == want, (c['name'], force, packed, stats, got, want)
                yw, y = guarded(n * h * w * cout, dev)       # NaN inside, sentinels around: output, records
                y = y.view(n, h, w, cout)
                pw, parts = guarded(max(cap, 1) * 3 * cout, dev)
                npart = ctypes.c_int32(0)
                _C.call('evk_conv2d_fwd_f16x2', ctypes.byref(d), src.data_ptr(), bx.data_ptr(), pf.data_ptr(), bw.data_ptr(),
                        bg.data_ptr() if bg is not None else None, None, y.data_ptr(), 2 if packed else 0,
                        parts.data_ptr() if stats else None, cap if stats else 0, ctypes.byref(npart), None, st)
                torch.cuda.synchronize()
                outs.append(y)
                what = f"raw {c['name']} {force} {'packed' if packed else 'fp32'} x{' stats' if stats else ''}"
                if not (guards_intact(yw, y.numel()) and guards_intact(pw, parts.numel())):
                    bad.append((what + ': a store beside the output / the records', got[0], float('nan'), 0.0))
                note(what + ' y', got[0], rel(y, y64), max(4 * e32['y'], 5e-6), f"(e32 {e32['y']:.2e})")
                if stats:
                    assert (npart.value > 0) == bool(c.get('stats')), (c['name'], force, npart.value)
                if stats and npart.value > 0:
                    assert npart.value == row_tiles(got[0], c), (c['name'], force, got[0], npart.value, row_tiles(got[0], c))
                    rec = parts[:npart.value * 3 * cout].view(npart.value, 3, cout).double()
                    assert bool(torch.isfinite(rec).all()) and bool(torch.isnan(parts[npart.value * 3 * cout:]).all()), what
                    cnt, mean, m2 = rec[:, 0], rec[:, 1], rec[:, 2]
                    tot = cnt.sum(0)
                    gm = (cnt * mean).sum(0) / tot
                    var = (m2 + cnt * (mean - gm) ** 2).sum(0) / tot
                    yd = y.double().view(-1, cout)
                    assert bool((tot == yd.shape[0]).all()), (c['name'], force, tot.tolist()[:8], yd.shape)
                    em = float((gm - yd.mean(0)).abs().max() / yd.abs().max())
                    ev = float((var - yd.var(0, unbiased=False)).abs().max() / yd.var(0, unbiased=False).max())
                    note(what + ' mean', got[0], em, 1e-6, f'({npart.value} records)')
                    note(what + ' var', got[0], ev, 1e-5)
        for o in outs[1:]:
            if not torch.equal(outs[0], o):
                bad.append((f"raw {c['name']} {force}: packed / statistics forward differs from the plain one", want[0],
                            float((outs[0] - o).abs().max()), 0.0))
        gs = []
        for src, packed in ((dy, False), (dyp, True)):
            want = T.expected(family, c, force, 'f16x2', packed)
            got = T.routed(lib, c, 2, packed, accum=1)
            assert got == want, (c['name'], force, packed, got, want)
            dw_, dx = guarded(x.numel(), dev)
            dx = dx.view_as(x)
            _C.call('evk_conv2d_dgrad_f16x2_ex', ctypes.byref(d), src.data_ptr(), bdy.data_ptr(), pd.data_ptr(), bw.data_ptr(),
                    acc.data_ptr(), dx.data_ptr(), None, 4 if packed else 0, st)
            torch.cuda.synchronize()
            gs.append(dx)
            if not guards_intact(dw_, dx.numel()):
                bad.append((f"raw {c['name']} {force}: a store beside dx", got[1][0], float('nan'), 0.0))
            note(f"raw {c['name']} {force} {'packed' if packed else 'fp32'} dy accum dx", got[1][0], rel(dx, dxa64),
                 max(4 * e32a, 5e-6), f'(e32 {e32a:.2e})')
        if not torch.equal(gs[0], gs[1]):
            bad.append((f"raw {c['name']} {force}: packed data gradient differs from the plain one", want[1][0],
                        float((gs[0] - gs[1]).abs().max()), 0.0))
    os.environ[VAR] = ''
t_raw = time.time() - t0

print('\nworst e / bound per instantiation and direction:')
for (name, direction), (r, what, e, bound) in sorted(worst.items()):
    print(f'  {name:46s} {direction:5s} {r:5.2f}  ({what}: e {e:.2e} / {bound:.2e})')
print(f'references {t_ref:.1f} s, python layer {t_py:.1f} s, raw {t_raw:.1f} s')
assert not bad, bad
print('check_tiles ok', family, ' '.join(forces))
