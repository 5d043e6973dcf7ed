"""dev tool (GPU box): the loss and metric entry points of two builds of the library, output buffer by output buffer.

    python tools/ab_loss_bits.py A.so B.so            digests of every output, compared; exit status 1 on a difference
    python tools/ab_loss_bits.py A.so B.so --time     time per C-ABI call (HIP events), three alternated runs per library

Every entry point of csrc/loss.hip, loss_pixel.hip and metric.hip runs over a fixed case list in a fresh child process per
library (EVK_LIB selects the build).  Inputs are seeded on the CPU, so both runs read the same bytes.  A digest is the
SHA-256 of a buffer's bytes: loss scalars, the K finals of `stats`, dlogits, per-pixel losses, the confusion matrix.
The cases sit at the edges of the launch grids (forward: 1 / 2 / 4 workgroups and the capped grid; the 1024-pixel grid's
second workgroup and cap; the backward cap), of the class counts and of the labels; tests/test_loss_edges_gpu.py checks the
same edges against float64.  OHEM's inputs are distinct values, so no tie sits at the threshold (which of several equal
losses the backward keeps is arbitrary by design)."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGNORE = 255
CAP = 4194304 + 2048 * 256 + 3      # capped forward grid (2048 workgroups) with a ragged tail
BWD = 1048577                       # one element past the backward grid's cap
NARROW = (1025, 262145)             # second workgroup / one past the cap of the 1024-pixel grid


def _inputs(npix, c, seed, all_ignored=False):
    import torch
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(npix, c, generator=g) * 2.0            # NHWC memory: [pixels, C]
    labels = torch.randint(0, max(c, 2), (npix,), generator=g)
    if npix >= 8:
        labels[torch.rand(npix, generator=g) < 0.05] = IGNORE
        labels[:3] = IGNORE
        labels[-2:] = IGNORE
    if all_ignored:
        labels[:] = IGNORE
    prefill = torch.randn(npix, c, generator=g)
    return logits.cuda(), labels.cuda(), prefill.cuda()


def _cases():
    """yield (name, callable -> {buffer name: tensor})"""
    import torch
    from ever_amd import _C
    lib = _C.load()
    st = torch.cuda.current_stream().cuda_stream
    gs = torch.full((), 0.75, device='cuda')
    f32 = lambda *shape: torch.empty(shape, device='cuda', dtype=torch.float32)

    def grad_buf(prefill, accumulate):
        return prefill.clone() if accumulate else torch.empty_like(prefill)

    def bce(npix, pw=1.0, red=0, eps=0.0, acc=0, all_ignored=False, scale=True):
        x, y, pre = _inputs(npix, 1, 11 + npix % 997, all_ignored)
        stats = torch.zeros(lib.evk_loss_stats_doubles(2), device='cuda', dtype=torch.float64)
        loss, d = f32(), grad_buf(pre, acc)
        _C.call('evk_bce_fwd_ex', x.data_ptr(), y.data_ptr(), npix, IGNORE, eps, pw, red, loss.data_ptr(), stats.data_ptr(), st)
        _C.call('evk_bce_bwd_ex', x.data_ptr(), y.data_ptr(), npix, IGNORE, eps, pw, red, stats.data_ptr(),
                gs.data_ptr() if scale else 0, d.data_ptr(), acc, st)
        return {'loss': loss, 'stats': stats[:2], 'dlogits': d}

    def dice(npix, c, ich=-1, acc=0, all_ignored=False):
        x, y, pre = _inputs(npix, c, 23 + c, all_ignored)
        stats = torch.zeros(lib.evk_loss_stats_doubles(2 * c), device='cuda', dtype=torch.float64)
        loss, d = f32(), grad_buf(pre, acc)
        _C.call('evk_dice_stats', x.data_ptr(), y.data_ptr(), npix, c, IGNORE, stats.data_ptr(), st)
        _C.call('evk_dice_finish', stats.data_ptr(), c, 1.0, ich, loss.data_ptr(), st)
        _C.call('evk_dice_bwd', x.data_ptr(), y.data_ptr(), npix, c, IGNORE, stats.data_ptr(), 1.0, ich, gs.data_ptr(),
                d.data_ptr(), acc, st)
        return {'loss': loss, 'stats': stats[:2 * c], 'dlogits': d}

    def ce(npix, c, eps=0.0, acc=0, all_ignored=False):
        x, y, pre = _inputs(npix, c, 37 + c, all_ignored)
        stats = torch.zeros(lib.evk_loss_stats_doubles(3), device='cuda', dtype=torch.float64)
        loss, d = f32(), grad_buf(pre, acc)
        _C.call('evk_ce_fwd', x.data_ptr(), y.data_ptr(), npix, c, IGNORE, eps, loss.data_ptr(), stats.data_ptr(), st)
        _C.call('evk_ce_bwd', x.data_ptr(), y.data_ptr(), npix, c, IGNORE, eps, stats.data_ptr(), gs.data_ptr(), d.data_ptr(),
                acc, st)
        return {'loss': loss, 'stats': stats[:3], 'dlogits': d}

    def soft_ce(npix, c):
        x, _, pre = _inputs(npix, c, 41 + c)
        t = torch.softmax(pre, dim=1).contiguous()
        stats = torch.zeros(lib.evk_loss_stats_doubles(1), device='cuda', dtype=torch.float64)
        loss, d = f32(), torch.empty_like(x)
        _C.call('evk_soft_ce_fwd', x.data_ptr(), t.data_ptr(), npix, c, loss.data_ptr(), stats.data_ptr(), st)
        _C.call('evk_soft_ce_bwd', x.data_ptr(), t.data_ptr(), npix, c, gs.data_ptr(), d.data_ptr(), st)
        return {'loss': loss, 'stats': stats[:1], 'dlogits': d}

    def prob_stats(npix, c, acc=0, all_ignored=False):
        x, y, pre = _inputs(npix, c, 53 + c, all_ignored)
        stats = torch.zeros(lib.evk_prob_stats_doubles(c), device='cuda', dtype=torch.float64)
        g = torch.randn(2, c, generator=torch.Generator().manual_seed(5)).cuda()
        d = grad_buf(pre, acc)
        _C.call('evk_prob_stats', x.data_ptr(), y.data_ptr(), npix, c, IGNORE, stats.data_ptr(), st)
        _C.call('evk_prob_stats_bwd', x.data_ptr(), y.data_ptr(), npix, c, IGNORE, g[0].data_ptr(), g[1].data_ptr(),
                d.data_ptr(), acc, st)
        return {'stats': stats[:3 * c], 'dlogits': d}

    def focal(n, mode, mean):
        x, y, _ = _inputs(n, 1, 61 + mode)
        t = (y == 1).float()
        stats = torch.zeros(1 + 256, device='cuda', dtype=torch.float64)
        loss, d = f32(), torch.empty_like(x)
        _C.call('evk_focal_fwd', x.data_ptr(), t.data_ptr(), n, 2.0, 0.25 if mode == 1 else -1.0, mode, mean, loss.data_ptr(),
                stats.data_ptr(), st)
        _C.call('evk_focal_bwd', x.data_ptr(), t.data_ptr(), n, 2.0, 0.25 if mode == 1 else -1.0, mode, mean, gs.data_ptr(),
                d.data_ptr(), st)
        return {'loss': loss, 'stats': stats[:1], 'dlogits': d}

    def ce_pixel(npix, c, all_ignored=False):
        x, y, pre = _inputs(npix, c, 71 + c, all_ignored)
        gpix = pre[:, 0].contiguous()
        gpix[::7] = 0.0                     # a zero upstream gradient takes the fill path
        out, d = f32(npix), torch.empty_like(x)
        _C.call('evk_ce_pixel_fwd', x.data_ptr(), y.data_ptr(), npix, c, IGNORE, out.data_ptr(), st)
        _C.call('evk_ce_pixel_bwd', x.data_ptr(), y.data_ptr(), npix, c, IGNORE, gpix.data_ptr(), d.data_ptr(), st)
        return {'loss_pix': out, 'dlogits': d}

    def ohem(n, ratio):
        g = torch.Generator().manual_seed(83)
        v = (torch.randperm(n, generator=g) + 1).float() * 1e-3     # distinct: no tie anywhere
        v[::97] = 0.0                                               # zeros are never kept; the threshold is far above them
        v = v.cuda()
        state = torch.zeros(lib.evk_ohem_state_bytes(), device='cuda', dtype=torch.uint8)
        loss, d = f32(), torch.empty_like(v)
        _C.call('evk_ohem_fwd', v.data_ptr(), n, int(ratio * n), loss.data_ptr(), state.data_ptr(), st)
        _C.call('evk_ohem_bwd', v.data_ptr(), n, state.data_ptr(), gs.data_ptr(), d.data_ptr(), st)
        sums = state[(4 + 2048) * 8:(4 + 2048) * 8 + 16].view(torch.float64)
        return {'loss': loss, 'stats': sums, 'dlosses': d}

    def confusion(n, classes, from_logits):
        x, y, _ = _inputs(n, classes if from_logits else 1, 91 + classes)
        g = torch.Generator().manual_seed(7)
        yt = torch.randint(0, classes, (n,), generator=g)
        yt[::13] = IGNORE
        yt = yt.cuda()
        cm = torch.zeros(classes, classes, device='cuda', dtype=torch.int64)
        if from_logits:
            _C.call('evk_confusion_from_logits', x.data_ptr(), yt.data_ptr(), n, classes, classes, cm.data_ptr(), st)
        else:
            yp = torch.randint(-1, classes + 1, (n,), generator=g).cuda()
            _C.call('evk_confusion_matrix', yt.data_ptr(), yp.data_ptr(), n, classes, cm.data_ptr(), st)
        return {'cm': cm}

    for n in (1, 2049, 6145, CAP, BWD):
        yield f'bce n={n}', lambda n=n: bce(n)
        yield f'dice C=1 n={n}', lambda n=n: dice(n, 1)
        yield f'ce C=2 n={n}', lambda n=n: ce(n, 2)
        yield f'soft_ce C=2 n={n}', lambda n=n: soft_ce(n, 2)
    yield 'bce pos_weight=2.5', lambda: bce(6145, pw=2.5)
    yield 'bce sum', lambda: bce(6145, red=1)
    yield 'bce sum pos_weight=0.5 smoothing=0.1', lambda: bce(6145, pw=0.5, red=1, eps=0.1)
    yield 'bce no grad_scale', lambda: bce(2049, scale=False)
    for c in (1, 2, 3, 16):
        for ich in (-1, 0, c - 1):
            yield f'dice C={c} ignore_channel={ich}', lambda c=c, ich=ich: dice(6145, c, ich)
    for c in (2, 64, 65, 150):
        for eps in (0.0, 0.1):
            yield f'ce C={c} smoothing={eps}', lambda c=c, eps=eps: ce(2049, c, eps)
    yield 'soft_ce C=19', lambda: soft_ce(6145, 19)
    for c in (1, 2, 64):
        yield f'prob_stats C={c}', lambda c=c: prob_stats(1025, c)
    for n in NARROW + (BWD,):
        yield f'prob_stats C=2 n={n}', lambda n=n: prob_stats(n, 2)
        yield f'ce_pixel C=2 n={n}', lambda n=n: ce_pixel(n, 2)
    yield 'ce_pixel C=65', lambda: ce_pixel(1025, 65)
    for mode in (0, 1, 2):
        for n in NARROW:
            yield f'focal mode={mode} n={n}', lambda mode=mode, n=n: focal(n, mode, 0 if mode == 2 else 1)
    yield f'focal mode=1 sum n={BWD}', lambda: focal(BWD, 1, 0)
    yield 'accumulate bce', lambda: bce(6145, acc=1)
    yield 'accumulate dice C=1', lambda: dice(6145, 1, acc=1)
    yield 'accumulate dice C=3', lambda: dice(6145, 3, acc=1)
    yield 'accumulate ce C=5', lambda: ce(6145, 5, eps=0.1, acc=1)
    yield 'accumulate prob_stats C=1', lambda: prob_stats(1025, 1, acc=1)
    yield 'accumulate prob_stats C=3', lambda: prob_stats(1025, 3, acc=1)
    yield 'all ignored bce', lambda: bce(2049, all_ignored=True)
    yield 'all ignored dice C=3', lambda: dice(2049, 3, all_ignored=True)
    yield 'all ignored ce C=3 accumulate', lambda: ce(2049, 3, acc=1, all_ignored=True)
    yield 'all ignored prob_stats C=3', lambda: prob_stats(1025, 3, all_ignored=True)
    yield 'all ignored ce_pixel C=3', lambda: ce_pixel(1025, 3, all_ignored=True)
    yield 'ohem n=1025 keep=0.5', lambda: ohem(1025, 0.5)
    yield 'ohem n=262145 keep=0.05', lambda: ohem(262145, 0.05)
    for classes in (64, 65):
        for n in NARROW:
            yield f'confusion classes={classes} n={n}', lambda c=classes, n=n: confusion(n, c, False)
            yield f'confusion from logits classes={classes} n={n}', lambda c=classes, n=n: confusion(n, c, True)


def _timed():
    """yield (name, callable) of single C-ABI calls on persistent buffers, at 1 048 576 and 4 194 304 pixels"""
    import torch
    from ever_amd import _C
    lib = _C.load()
    st = torch.cuda.current_stream().cuda_stream
    gs = torch.full((), 0.75, device='cuda')
    for n in (1048576, 4194304):
        for c in (1, 2, 8):
            x, y, pre = _inputs(n, c, 3 + c)
            d, loss = torch.empty_like(x), torch.empty((), device='cuda')
            s = torch.zeros(max(lib.evk_loss_stats_doubles(2 * c + 3), lib.evk_prob_stats_doubles(c)), device='cuda', dtype=torch.float64)
            a = (x.data_ptr(), y.data_ptr(), n)
            tag = f'C={c} n={n}'
            if c == 1:
                t = (y == 1).float()
                yield f'bce_fwd {tag}', lambda a=a, s=s, loss=loss: _C.call('evk_bce_fwd_ex', *a, IGNORE, 0.0, 1.0, 0, loss.data_ptr(), s.data_ptr(), st)
                yield f'focal_fwd {tag}', lambda x=x, t=t, s=s, loss=loss, n=n: _C.call('evk_focal_fwd', x.data_ptr(), t.data_ptr(), n, 2.0, 0.25, 1, 1, loss.data_ptr(), s.data_ptr(), st)
            else:
                t = torch.softmax(pre, dim=1).contiguous()
                yield f'ce_fwd {tag}', lambda a=a, c=c, s=s, loss=loss: _C.call('evk_ce_fwd', *a, c, IGNORE, 0.1, loss.data_ptr(), s.data_ptr(), st)
                yield f'ce_bwd {tag}', lambda a=a, c=c, s=s, d=d: _C.call('evk_ce_bwd', *a, c, IGNORE, 0.1, s.data_ptr(), gs.data_ptr(), d.data_ptr(), 0, st)
                yield f'soft_ce_fwd {tag}', lambda x=x, t=t, c=c, s=s, loss=loss, n=n: _C.call('evk_soft_ce_fwd', x.data_ptr(), t.data_ptr(), n, c, loss.data_ptr(), s.data_ptr(), st)
                yield f'soft_ce_bwd {tag}', lambda x=x, t=t, c=c, d=d, n=n: _C.call('evk_soft_ce_bwd', x.data_ptr(), t.data_ptr(), n, c, gs.data_ptr(), d.data_ptr(), st)
                yield f'ce_pixel_fwd {tag}', lambda a=a, c=c, d=d: _C.call('evk_ce_pixel_fwd', *a, c, IGNORE, d.data_ptr(), st)
                yield f'ce_pixel_bwd {tag}', lambda a=a, c=c, pre=pre, d=d: _C.call('evk_ce_pixel_bwd', *a, c, IGNORE, pre.data_ptr(), d.data_ptr(), st)
            yield f'dice_stats {tag}', lambda a=a, c=c, s=s: _C.call('evk_dice_stats', *a, c, IGNORE, s.data_ptr(), st)
            yield f'dice_bwd {tag}', lambda a=a, c=c, s=s, d=d: _C.call('evk_dice_bwd', *a, c, IGNORE, s.data_ptr(), 1.0, -1, gs.data_ptr(), d.data_ptr(), 0, st)
            yield f'prob_stats {tag}', lambda a=a, c=c, s=s: _C.call('evk_prob_stats', *a, c, IGNORE, s.data_ptr(), st)
            g = torch.randn(2, c, generator=torch.Generator().manual_seed(5)).cuda()
            yield f'prob_stats_bwd {tag}', lambda a=a, c=c, g=g, d=d: _C.call('evk_prob_stats_bwd', *a, c, IGNORE, g[0].data_ptr(), g[1].data_ptr(), d.data_ptr(), 0, st)
        v = torch.rand(n, generator=torch.Generator().manual_seed(9)).cuda()
        state = torch.zeros(lib.evk_ohem_state_bytes(), device='cuda', dtype=torch.uint8)
        loss = torch.empty((), device='cuda')
        yield f'ohem_fwd n={n}', lambda v=v, state=state, loss=loss, n=n: _C.call('evk_ohem_fwd', v.data_ptr(), n, n // 10, loss.data_ptr(), state.data_ptr(), st)


def _child(out_path, timing):
    import torch
    sys.path.insert(0, ROOT)
    res = {}
    if timing:
        for name, fn in _timed():
            for _ in range(5):
                fn()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(31)]
            ev[0].record()
            for i in range(30):
                fn()
                ev[i + 1].record()
            torch.cuda.synchronize()
            ts = sorted(ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(30))
            res[name] = ts[15]      # median us per call
    else:
        for name, fn in _cases():
            out = fn()
            torch.cuda.synchronize()
            res[name] = {k: (v.numel() * v.element_size(), hashlib.sha256(v.contiguous().cpu().numpy().tobytes()).hexdigest())
                         for k, v in out.items()}
    with open(out_path, 'w') as f:
        json.dump(res, f)


def _run(lib, timing, tag):
    out = os.path.join(os.environ.get('TMPDIR', '/tmp'), f'ab_loss_bits_{os.getpid()}_{tag}.json')
    env = dict(os.environ, EVK_LIB=os.path.abspath(lib))
    subprocess.run([sys.executable, os.path.abspath(__file__), '--child', out] + (['--time'] if timing else []), check=True,
                   env=env, timeout=600)
    with open(out) as f:
        res = json.load(f)
    os.remove(out)
    return res


def main(argv):
    timing = '--time' in argv
    if '--child' in argv:
        return _child(argv[argv.index('--child') + 1], timing)
    a, b = [x for x in argv if not x.startswith('--')][:2]
    if timing:
        runs = {a: [], b: []}
        for r in range(3):
            for lib in (a, b):
                runs[lib].append(_run(lib, True, f't{r}'))
        print(f'median us per C-ABI call (30 calls, HIP events), three alternated runs each\nA = {a}\nB = {b}')
        print(f'{"call":34s} {"A":>27s}   {"B":>27s}  A spread  verdict')
        for name in runs[a][0]:
            ta, tb = [r[name] for r in runs[a]], [r[name] for r in runs[b]]
            level = min(tb) <= max(ta) and min(ta) <= max(tb)
            gap = (min(tb) - max(ta)) / max(ta) if min(tb) > max(ta) else (max(tb) - min(ta)) / min(ta)
            verdict = 'level (ranges overlap)' if level else f'{"ABOVE" if gap > 0 else "below"} by {abs(gap) * 100:.1f} % (closest runs)'
            print(f'{name:34s} ' + ' '.join(f'{t:8.2f}' for t in ta) + '   ' + ' '.join(f'{t:8.2f}' for t in tb)
                  + f'  {(max(ta) - min(ta)) / min(ta) * 100:7.1f}%  {verdict}')
        return 0
    ra, rb = _run(a, False, 'a'), _run(b, False, 'b')
    assert list(ra) == list(rb), 'the two runs saw different case lists'
    nbuf = nbytes = 0
    bad = []
    for name in ra:
        assert ra[name].keys() == rb[name].keys(), name
        for k, (size, digest) in ra[name].items():
            nbuf += 1
            nbytes += size
            if [size, digest] != rb[name][k]:
                bad.append(f'{name}: {k}')
    print(f'A = {a}\nB = {b}\n{len(ra)} cases, {nbuf} output buffers, {nbytes} bytes compared: '
          + ('every digest equal' if not bad else f'{len(bad)} buffers DIFFER'))
    for x in bad:
        print('  differs:', x)
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
