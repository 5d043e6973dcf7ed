"""dev tool (GPU box): the fused batch augmentation WITH the rescale step (evk_augment_scale_batch, one launch) against the aten
chain on the same device tensors, in the manner of tools/bench_augment.py (whose helpers it imports).

Both sides are one `THBatchAugment(scale_range=(f, f))` under the same `np.random.seed`, so they draw the same parameters:
the fused side is its CUDA path (one `HF.augment_batch(..., scales=...)` call), the aten side its per-image path on the same
device tensors (the image cast to fp32 through THRandomScale's expression — `F.interpolate` bilinear align_corners / nearest —
then THRandomRotate90k -> THRandomHorizontalFlip -> THRandomVerticalFlip -> THRandomCrop -> channel-first ->
THMeanStdNormalize -> THDivisiblePad per image, then torch.stack).

rows    the three batch shapes of DESIGN 2.16 (16 x 1024^2 x 3 -> 16 x 3 x 512^2 with uint8 and with int64 labels, 8 x 1024^2 x 4
        -> 8 x 4 x 1024^2 with int64 labels) at factors 0.5, 1.25 and 2.0, mixed ops.
ops     the first shape at 1.25 with each of the eight ops fixed, NHWC and NCHW output, kernel alone: what the transposing ops
        cost without a tile form.

Warm-up first, HIP events, alternating rounds, medians.  us per batch.  `kernel us` is a window of evk_augment_scale_batch
calls alone on a table uploaded once; its algorithmic TB/s counts, once each, four taps read per output element inside the
window that lies inside the scaled image, one label read per such pixel, and every output byte written.  `unscaled us` is
evk_augment_batch for the same output (same ops, origins drawn on the unscaled size).  `fused us` is the whole THBatchAugment
call, draws, record table and upload included.  The fused result is compared with the chain's on the device: whether the
labels are equal, and the largest |difference| of the normalised images.  One JSON line; --table adds markdown tables.  Fails
without a device.
usage: python tools/bench_augment_scale.py [--rounds R] [--iters K] [--skip-rows] [--skip-ops] [--table]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_augment as ba  # noqa: E402
from ever_amd import _C  # noqa: E402
from ever_amd.hip import functional as HF  # noqa: E402
from ever_amd.hip.augment import _f32_bits, scaled_hw  # noqa: E402
from ever_amd.preprocess.thsegm import THBatchAugment  # noqa: E402

FACTORS = (0.5, 1.25, 2.0)


def _augmenter(op, crop, c, mask_dtype, factor, channels_last=True):
    mean, std = (ba.MEAN4, ba.STD4) if c == 4 else (ba.MEAN4[:c], ba.STD4[:c])
    kw = dict()
    if op != 'mixed':
        k, h, v = ba._decompose(op)
        kw = dict(rotate_k=k, hflip_p=float(h), vflip_p=float(v))
    return THBatchAugment(crop, 32, mean, std, channels_last=channels_last, mask_dtype=mask_dtype,
                          scale_range=None if factor is None else (factor, factor), **kw)


def _draw(aug, images, factor, seed=1):
    """(ops, origins) as `aug` draws them under `seed` for sources rescaled by `factor` (None: not rescaled)"""
    np.random.seed(seed)
    ops, origins = [], []
    for im in images:
        if factor is not None:
            np.random.choice([factor], size=1)
        k, h, v = aug.rotate_k, not (aug.hflip_p < 0.5), not (aug.vflip_p < 0.5)
        if aug.rotate_k is None:
            k, h, v = int(np.random.choice([0, 1, 2, 3], 1)[0]), not (0.5 < np.random.uniform()), not (0.5 < np.random.uniform())
        op = HF.D4_ROT90.get(k, 0)
        op = HF.d4_compose(op, HF.D4_HFLIP) if h else op
        op = HF.d4_compose(op, HF.D4_VFLIP) if v else op
        hz, wz = (im.shape[0], im.shape[1]) if factor is None else scaled_hw(im.shape[0], im.shape[1], factor)
        ht, wt = HF.d4_out_hw(hz, wz, op)
        ops.append(op)
        origins.append((int(np.random.randint(0, max(ht, aug.crop_size[0]) - aug.crop_size[0] + 1)),
                        int(np.random.randint(0, max(wt, aug.crop_size[1]) - aug.crop_size[1] + 1))))
    return ops, origins


def _kernel_only(aug, images, masks, factor):
    """(closure that enqueues only the entry point, algorithmic bytes): evk_augment_scale_batch with a factor, evk_augment_batch
    without; the table is uploaded once"""
    ops, origins = _draw(aug, images, factor)
    dev, n, c = images[0].device, len(images), images[0].shape[2]
    ch, cw = aug.crop_size
    ho, wo = aug.out_size
    wide_out = aug.mask_dtype is torch.int64 or masks[0].dtype == torch.int64
    mode = 3 if masks[0].dtype == torch.int64 else 2 if wide_out else 1
    recs, nbytes = [], 0.0
    for im, m, op, (y0, x0) in zip(images, masks, ops, origins):
        recs += [im.data_ptr(), m.data_ptr(), im.shape[0], im.shape[1], op, y0, x0, 0]
        hz, wz = im.shape[0], im.shape[1]
        if factor is not None:
            hz, wz = scaled_hw(hz, wz, factor)
            recs += [hz, wz, _f32_bits(1.0 / factor), 0]
        ht, wt = HF.d4_out_hw(hz, wz, op)
        px = max(min(ht - y0, ch), 0) * max(min(wt - x0, cw), 0)
        taps = 1 if factor is None else 4
        nbytes += px * (taps * c * im.element_size() + m.element_size()) + ho * wo * (c * 4 + (8 if wide_out else 1))
    host = torch.tensor(recs, dtype=torch.int64)
    table = host.to(dev)
    mean = torch.tensor(aug.mean, dtype=torch.float32, device=dev)
    std = torch.tensor(aug.std, dtype=torch.float32, device=dev)
    out = torch.empty(n * c * ho * wo, dtype=torch.float32, device=dev)
    labels = torch.empty(n * ho * wo, dtype=torch.int64 if wide_out else torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    keep = (host, table, mean, std, out, labels)
    entry = 'evk_augment_batch' if factor is None else 'evk_augment_scale_batch'

    def run():
        _C.call(entry, host.data_ptr(), table.data_ptr(), n, c, ch, cw, ho, wo, mean.data_ptr(), std.data_ptr(), aug.mask_pad_value,
                0 if aug.channels_last else 1, 1 if images[0].dtype == torch.float32 else 0, mode, out.data_ptr(), labels.data_ptr(), st)
        return keep
    return run, nbytes


def _kernel_us(args, run):
    run()
    return ba._median([ba._events(run, 4 * args.iters) for _ in range(args.rounds)])


def _compare(args, fused_fn, chain_fn):
    keep = {}

    def fused():
        np.random.seed(1)
        keep['fused'] = fused_fn()

    def chain():
        np.random.seed(1)
        keep['chain'] = chain_fn()

    fused()
    chain()
    torch.cuda.synchronize()
    (fi, fm), (ci, cm) = keep['fused'], keep['chain']
    diff = float((fi.contiguous() - ci.contiguous()).abs().max().item())
    labels_equal = bool(torch.equal(fm, cm))
    times = {'fused': [], 'chain': [], 'fused_host': [], 'chain_host': []}
    for _ in range(args.rounds):
        times['fused'].append(ba._events(fused, args.iters))
        times['chain'].append(ba._events(chain, max(2, args.iters // 4)))
        times['fused_host'].append(ba._host(fused, args.iters))
        times['chain_host'].append(ba._host(chain, max(2, args.iters // 4)))
    return {k: ba._median(v) for k, v in times.items()}, labels_equal, diff


def bench_rows(args, dev):
    out = []
    cfgs = (('16x1024x1024x3 -> 16x3x512x512', 16, 3, (512, 512), None), ('16x1024x1024x3 -> 16x3x512x512', 16, 3, (512, 512), torch.int64),
            ('8x1024x1024x4 -> 8x4x1024x1024', 8, 4, (1024, 1024), torch.int64))
    for shape, n, c, crop, mask_dtype in cfgs:
        images, masks = ba._sources(n, 1024, c, dev)
        for factor in FACTORS:
            fused = _augmenter('mixed', crop, c, mask_dtype, factor)
            chain = _augmenter('mixed', crop, c, mask_dtype, factor, channels_last=False)
            t, labels_equal, diff = _compare(args, lambda: fused(images, masks), lambda: chain._per_image(images, masks))
            kern, nbytes = _kernel_only(fused, images, masks, factor)
            ku = _kernel_us(args, kern)
            plain, pbytes = _kernel_only(_augmenter('mixed', crop, c, mask_dtype, None), images, masks, None)
            pu = _kernel_us(args, plain)
            out.append(dict(shape=shape, labels='int64' if mask_dtype is torch.int64 else 'uint8', factor=factor,
                            kernel_us=round(ku, 1), kernel_tbs=round(nbytes / ku / 1e6, 3), unscaled_us=round(pu, 1),
                            unscaled_tbs=round(pbytes / pu / 1e6, 3), fused_us=round(t['fused'], 1), aten_us=round(t['chain'], 1),
                            speedup=round(t['chain'] / t['fused'], 2), fused_host_us=round(t['fused_host'], 1),
                            aten_host_us=round(t['chain_host'], 1), aten_labels_equal=labels_equal, aten_max_abs_diff=diff))
        del images, masks
        torch.cuda.empty_cache()
    return out


def bench_ops(args, dev):
    out = []
    n, c, crop, factor = 16, 3, (512, 512), 1.25
    images, masks = ba._sources(n, 1024, c, dev)
    for channels_last in (True, False):
        row = dict(layout='nhwc' if channels_last else 'nchw', factor=factor)
        for op in range(8):
            kern, nbytes = _kernel_only(_augmenter(op, crop, c, None, factor, channels_last), images, masks, factor)
            plain, _ = _kernel_only(_augmenter(op, crop, c, None, None, channels_last), images, masks, None)
            ku, pu = _kernel_us(args, kern), _kernel_us(args, plain)
            row[f'op{op}'] = dict(us=round(ku, 1), tbs=round(nbytes / ku / 1e6, 3), unscaled_us=round(pu, 1))
        out.append(row)
    return out


def _table(res):
    lines = []
    if 'rows' in res:
        lines += ['| batch | labels | factor | kernel us (TB/s) | unscaled kernel us (TB/s) | fused us | aten chain us | aten / fused | host us fused / aten | aten labels equal | aten image max abs diff |',
                  '|---|---|---|---|---|---|---|---|---|---|---|']
        lines += [f"| {r['shape']} | {r['labels']} | {r['factor']} | {r['kernel_us']} ({r['kernel_tbs']}) | {r['unscaled_us']} ({r['unscaled_tbs']}) | {r['fused_us']} | "
                  f"{r['aten_us']} | {r['speedup']}x | {r['fused_host_us']} / {r['aten_host_us']} | {r['aten_labels_equal']} | {r['aten_max_abs_diff']:.3g} |"
                  for r in res['rows']]
    if 'ops' in res:
        lines += ['', '| layout | ' + ' | '.join(f'op {o} scaled (TB/s) / unscaled us' for o in range(8)) + ' |', '|---|' + '---|' * 8]
        lines += [f"| {r['layout']} | " + ' | '.join(f"{r[f'op{o}']['us']} ({r[f'op{o}']['tbs']}) / {r[f'op{o}']['unscaled_us']}" for o in range(8)) + ' |'
                  for r in res['ops']]
    return '\n'.join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--skip-rows', action='store_true')
    ap.add_argument('--skip-ops', action='store_true')
    ap.add_argument('--table', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    _C.load()
    res = dict(tool='bench_augment_scale', rounds=args.rounds, iters=args.iters)
    with torch.no_grad():
        if not args.skip_ops:
            res['ops'] = bench_ops(args, dev)
        if not args.skip_rows:
            res['rows'] = bench_rows(args, dev)
    print(json.dumps(res))
    if args.table:
        print(_table(res))


if __name__ == '__main__':
    main()
