"""dev tool (GPU box): whole-scene tiled inference, `scene_inference` (magic/bigimage/scene.py: one gather launch per chunk, one
stitch launch per column strip, one finalise pass) against `sliding_window_inference` of the same tree (a slice copy per
window, a stack per chunk, two read-modify-write launches per window, one division), in one process.

scene    1 x 3 x S x S scenes (S = 4096, 8192), window 512, stride 256, batch 8 and 16, 6 classes, with (a) FarSeg-R50 in eval
         mode and (b) a near-free callable (the tile's channels, repeated to 6), so the tiling overhead shows alone.  Per row:
         wall time per scene of both sides (host clock around a synchronise, alternating rounds, medians), the new side's split
         into gather / model / stitch / finalise (HIP events around each call, from one extra pass), tiling launches per scene
         of both sides counted at their call sites (the model's own launches excluded), and the peak device memory above the
         scene for a scores and for a labels result.
kernels  evk_stitch_add on one column strip of 8 windows (the launch the scene makes) and evk_stitch_finalize on the 8192^2
         scene, in microseconds and TB/s of algorithmic bytes (stitch_add: the scores once, the covered accumulator elements
         and coverage read and written; finalise: accumulator and coverage read, result written), each against its byte bound
         at the 6.3 TB/s a streaming copy reaches on this chip.  The strips rotate over the scene's columns and four score
         buffers; what a last-level cache still holds between two launches of one strip is part of the figure.

One JSON line.  Fails without a device.
usage: python tools/bench_scene.py [--rounds R] [--sizes 4096,8192] [--batches 8,16] [--skip-model] [--skip-kernels]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ever_amd as er  # noqa: E402
from ever_amd import _C  # noqa: E402
from ever_amd.hip import functional as HF  # noqa: E402
from ever_amd.magic.bigimage import SceneStitcher, scene_inference, sliding_window, sliding_window_inference  # noqa: E402

KERNEL, STRIDE, CLASSES = 512, 256, 6
STREAM_TBS = 6.3


def _median(v):
    return sorted(v)[len(v) // 2]


def _wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out      # ms


def _near_free(tiles):
    return tiles.repeat(1, 2, 1, 1)       # 3 -> 6 channels: one copy launch


def _farseg_r50(dev):
    torch.manual_seed(0)
    m = er.module.FarSeg(dict(head=dict(fpn_decoder=dict(classifier_config=dict(num_classes=CLASSES)))))
    return m.to(dev).eval()


class _Split:
    """HIP events around every call of the four phases of scene_inference"""

    def __init__(self, model):
        self.model, self.spans = model, {k: [] for k in ('gather', 'model', 'stitch', 'finalise')}
        self.saved = (HF.augment_batch, HF.stitch_add, HF.stitch_finalize)

    def _timed(self, key, fn):
        def run(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **kw)
            e1.record()
            self.spans[key].append((e0, e1))
            return out
        return run

    def __enter__(self):
        HF.augment_batch = self._timed('gather', self.saved[0])
        HF.stitch_add = self._timed('stitch', self.saved[1])
        HF.stitch_finalize = self._timed('finalise', self.saved[2])
        return self._timed('model', self.model)

    def __exit__(self, *exc):
        HF.augment_batch, HF.stitch_add, HF.stitch_finalize = self.saved

    def ms(self):
        torch.cuda.synchronize()
        return {k: round(sum(a.elapsed_time(b) for a, b in v), 2) for k, v in self.spans.items()}


def _peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return round(peak / 2 ** 20, 1)


def bench_scene(args, dev, variants):
    rows = []
    for size in args.sizes:
        scene = torch.randn(1, 3, size, size, device=dev)
        boxes = np.unique(sliding_window((size, size), KERNEL, STRIDE), axis=0)
        strips = len(np.unique(boxes[:, 0]))
        for name, model in variants:
            for bs in args.batches:
                new = lambda: scene_inference(model, scene, KERNEL, STRIDE, batch_size=bs)
                old = lambda: sliding_window_inference(model, scene, KERNEL, STRIDE, batch_size=bs)
                a, b = new(), old()
                torch.cuda.synchronize()
                diff = float((a - b).abs().max())
                same = bool(torch.equal(a, b))
                del a, b
                times = {'new': [], 'old': []}
                for _ in range(args.rounds):
                    for k, f in (('new', new), ('old', old)):
                        ms, out = _wall(f)
                        del out
                        times[k].append(ms)
                split = _Split(model)
                before = dict(HF.stitch_stats), HF.augment_stats['calls']
                with split as timed_model:
                    out = scene_inference(timed_model, scene, KERNEL, STRIDE, batch_size=bs)
                    del out
                chunks = -(-len(boxes) // bs)
                launches_new = (HF.augment_stats['calls'] - before[1]) + (HF.stitch_stats['launches'] - before[0]['launches']) + 1
                # per window a slice copy inside torch.stack (one cat launch per chunk) and two read-modify-writes, the two
                # zero fills and the division
                launches_old = chunks + 2 * len(boxes) + 3
                row = dict(scene=f'1x3x{size}x{size}', model=name, batch=bs, windows=len(boxes), strips=strips,
                           new_ms=round(_median(times['new']), 1), old_ms=round(_median(times['old']), 1),
                           new_range=[round(min(times['new']), 1), round(max(times['new']), 1)],
                           old_range=[round(min(times['old']), 1), round(max(times['old']), 1)],
                           speedup=round(_median(times['old']) / _median(times['new']), 3), split_ms=split.ms(),
                           tiling_launches_new=launches_new, tiling_launches_old=launches_old,
                           max_abs_diff=diff, same_bits=same,
                           peak_mb_new_scores=_peak_mb(new),
                           peak_mb_new_labels=_peak_mb(lambda: scene_inference(model, scene, KERNEL, STRIDE, batch_size=bs,
                                                                               output='labels')),
                           peak_mb_old_scores=_peak_mb(old),
                           peak_mb_old_labels=_peak_mb(lambda: old().argmax(dim=1).to(torch.uint8)))
                rows.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
        del scene
        torch.cuda.empty_cache()
    return rows


def _time_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def bench_kernels(args, dev):
    out = []
    for size in args.sizes:
        for cl in (True, False):
            st = SceneStitcher(CLASSES, size, size, dev, channels_last=cl)
            m = 8
            bufs = [torch.randn(m, CLASSES, KERNEL, KERNEL, device=dev) for _ in range(4)]
            if cl:
                bufs = [b.contiguous(memory_format=torch.channels_last) for b in bufs]
            cols = list(range(0, size - KERNEL + 1, STRIDE))
            origins = [[(y * STRIDE, x0) for y in range(m)] for x0 in cols]
            rows_cov = (m - 1) * STRIDE + KERNEL
            nbytes = 4.0 * m * CLASSES * KERNEL * KERNEL + 8.0 * rows_cov * KERNEL * (CLASSES + 1)
            # the C-ABI directly, with the origin tables uploaded beforehand: the wrapper's upload is not the kernel's time
            recs = [(ctypes.c_int64 * (2 * m))(*[v for yx in o for v in yx]) for o in origins]
            tabs = [torch.tensor([v for yx in o for v in yx], dtype=torch.int64, device=dev) for o in origins]
            stream = HF._stream()

            def add(i):
                j = i % len(cols)
                _C.call('evk_stitch_add', recs[j], tabs[j].data_ptr(), m, bufs[i % 4].data_ptr(), st.acc.data_ptr(),
                        st.count.data_ptr(), CLASSES, size, size, KERNEL, KERNEL, 0 if cl else 1, stream)

            for i in range(len(cols)):
                add(i)
            t = _median([_time_us(add, 4 * len(cols)) for _ in range(args.rounds)])
            row = dict(kernel='stitch_add', scene=size, layout='nhwc' if cl else 'nchw', windows=m, us=round(t, 1),
                       tbs=round(nbytes / t / 1e6, 3), bound_us=round(nbytes / STREAM_TBS / 1e6, 1))
            out.append(row)
            n = st.acc.numel()
            res = torch.empty_like(st.acc)
            lab = torch.empty((size, size), device=dev, dtype=torch.uint8)
            for mode, fn, nb in (('scores', lambda i: HF.stitch_finalize(st.acc, st.count, 'scores', out=res), 8.0 * n + 4.0 * size * size),
                                 ('labels-u8', lambda i: HF.stitch_finalize(st.acc, st.count, 'labels', out=lab), 4.0 * n + 5.0 * size * size)):
                fn(0)
                t = _median([_time_us(fn, 5) for _ in range(args.rounds)])
                out.append(dict(kernel=f'stitch_finalize {mode}', scene=size, layout='nhwc' if cl else 'nchw', us=round(t, 1),
                                tbs=round(nb / t / 1e6, 3), bound_us=round(nb / STREAM_TBS / 1e6, 1)))
            del st, bufs, res, lab
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--sizes', type=lambda s: [int(v) for v in s.split(',')], default=[4096, 8192])
    ap.add_argument('--batches', type=lambda s: [int(v) for v in s.split(',')], default=[8, 16])
    ap.add_argument('--skip-model', action='store_true', help='only the near-free callable')
    ap.add_argument('--skip-kernels', action='store_true')
    ap.add_argument('--skip-scene', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    res = dict(tool='bench_scene', rounds=args.rounds, kernel=KERNEL, stride=STRIDE, classes=CLASSES)
    with torch.no_grad():
        if not args.skip_kernels:
            res['kernels'] = bench_kernels(args, dev)
        if not args.skip_scene:
            variants = [('near-free', _near_free)] + ([] if args.skip_model else [('FarSeg-R50', _farseg_r50(dev))])
            res['scene'] = bench_scene(args, dev, variants)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
