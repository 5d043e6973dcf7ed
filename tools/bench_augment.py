"""dev tool (GPU box): the fused batch augmentation (csrc/augment.hip, one launch) against the aten chain on the same device.

Both sides are `THBatchAugment` under the same `np.random.seed`, so they draw the same parameters: the fused side is its CUDA
path (one `HF.augment_batch` call), the aten side its per-image path on the same device tensors (THRandomRotate90k ->
THRandomHorizontalFlip -> THRandomVerticalFlip -> THRandomCrop -> channel-first -> THMeanStdNormalize -> THDivisiblePad per
image, then torch.stack, NCHW-contiguous as the reference leaves it).  A uniform batch fixes the op through rotate_k and flip
probabilities of 0 or 1; the mixed batch draws them.

rows    16 sources of 1024 x 1024 x 3 uint8 with uint8 masks -> 16 x 3 x 512^2, for each of the eight ops and a mixed batch, with
        uint8 and with int64 label output; 8 sources of 1024 x 1024 x 4 -> 8 x 4 x 1024^2 (the C3 configuration).
forms   the transposing ops with the direct form (16-byte stores), the LDS-tile form and the direct form with 4-byte stores
        forced (evk_augment_force_kernel), NHWC and NCHW output, uint8 and fp32 sources, C = 1, 3, 4, 6, 8, 16: what the
        dispatch rule of evk_augment_plan follows.

Warm-up first, HIP events, alternating rounds, medians.  us per batch; algorithmic TB/s = (window bytes read + bytes written,
once each) / time; host us = wall clock to enqueue a batch (no synchronise inside the window).  `kernel us` is a window of
evk_augment_batch calls alone on a table uploaded once (what the device needs); `fused us` is the whole THBatchAugment call,
draws, record table and upload included (what a caller waits for when the host is the limit, as it is at these sizes).  The
fused image is compared with the chain's bit for bit and the share of equal words is reported.  One JSON line; --table adds
markdown tables.  Fails without a device.
usage: python tools/bench_augment.py [--rounds R] [--iters K] [--skip-rows] [--skip-forms] [--table]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ever_amd  # noqa: E402,F401
from ever_amd import _C  # noqa: E402
from ever_amd.hip import functional as HF  # noqa: E402
from ever_amd.preprocess.thsegm import THBatchAugment  # noqa: E402

FORMS = ('direct', 'tile', 'direct4')      # evk_augment_force_kernel: 16-byte-store direct, LDS tile, 4-byte-store direct
MEAN4, STD4 = (123.675, 116.28, 103.53, 110.0), (58.395, 57.12, 57.375, 60.5)


def _decompose(op):
    """(k, hflip, vflip) whose composition, in the pipeline's order, is `op`"""
    for k in range(4):
        for h in (0, 1):
            for v in (0, 1):
                o = HF.D4_ROT90.get(k, 0)
                o = HF.d4_compose(o, HF.D4_HFLIP) if h else o
                o = HF.d4_compose(o, HF.D4_VFLIP) if v else o
                if o == op:
                    return k, h, v
    raise ValueError(op)


def _events(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # us


def _host(fn, iters):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    dt = (time.perf_counter() - t) * 1e6 / iters
    torch.cuda.synchronize()
    return dt


def _median(v):
    return sorted(v)[len(v) // 2]


def _algorithmic_bytes(n, c, crop, out, src_bytes, mask_in, mask_out):
    px_in, px_out = crop[0] * crop[1], out[0] * out[1]
    return float(n * (px_in * (c * src_bytes + mask_in) + px_out * (c * 4 + mask_out)))


def _sources(n, size, c, dev, f32=False, wide=False):
    g = torch.Generator(device=dev).manual_seed(n * size + c)
    if f32:
        images = [torch.randn(size, size, c, device=dev, generator=g) for _ in range(n)]
    else:
        images = [torch.randint(0, 256, (size, size, c), device=dev, generator=g, dtype=torch.uint8) for _ in range(n)]
    masks = [torch.randint(0, 6, (size, size), device=dev, generator=g, dtype=torch.uint8) for _ in range(n)]
    return images, [m.long() for m in masks] if wide else masks


def _augmenters(op, crop, c, mask_dtype, channels_last=True):
    mean, std = ((MEAN4, STD4) if c == 4 else (MEAN4[:c], STD4[:c])) if c <= 4 else (tuple(MEAN4[0] for _ in range(c)),
                                                                                      tuple(STD4[0] for _ in range(c)))
    if op == 'mixed':
        kw = dict()
    else:
        k, h, v = _decompose(op)
        kw = dict(rotate_k=k, hflip_p=float(h), vflip_p=float(v))
    fused = THBatchAugment(crop, 32, mean, std, channels_last=channels_last, mask_dtype=mask_dtype, **kw)
    chain = THBatchAugment(crop, 32, mean, std, channels_last=False, mask_dtype=mask_dtype, **kw)
    return fused, chain


def _kernel_only(args, aug, images, masks, seed=1):
    """a closure that enqueues only evk_augment_batch, on the records `aug` draws under `seed`: the table is uploaded once, so
    a window of these calls is bound by the kernel, not by the host"""
    np.random.seed(seed)
    ops, origins = [], []
    for im in images:
        k, h, v = aug.rotate_k, not (aug.hflip_p < 0.5), not (aug.vflip_p < 0.5)
        if aug.rotate_k is None:
            k, h, v = int(np.random.choice([0, 1, 2, 3], 1)[0]), not (0.5 < np.random.uniform()), not (0.5 < np.random.uniform())
        op = HF.D4_ROT90.get(k, 0)
        op = HF.d4_compose(op, HF.D4_HFLIP) if h else op
        op = HF.d4_compose(op, HF.D4_VFLIP) if v else op
        ht, wt = HF.d4_out_hw(im.shape[0], im.shape[1], op)
        ops.append(op)
        origins.append((int(np.random.randint(0, ht - aug.crop_size[0] + 1)), int(np.random.randint(0, wt - aug.crop_size[1] + 1))))
    dev, n, c = images[0].device, len(images), images[0].shape[2]
    recs = []
    for im, m, op, (y0, x0) in zip(images, masks, ops, origins):
        recs += [im.data_ptr(), m.data_ptr(), im.shape[0], im.shape[1], op, y0, x0, 0]
    host = torch.tensor(recs, dtype=torch.int64)
    table = host.to(dev)
    mean = torch.tensor(aug.mean, dtype=torch.float32, device=dev)
    std = torch.tensor(aug.std, dtype=torch.float32, device=dev)
    ho, wo = aug.out_size
    wide_out = aug.mask_dtype is torch.int64 or masks[0].dtype == torch.int64
    mode = 3 if masks[0].dtype == torch.int64 else 2 if wide_out else 1
    out = torch.empty(n * c * ho * wo, dtype=torch.float32, device=dev)
    labels = torch.empty(n * ho * wo, dtype=torch.int64 if wide_out else torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    keep = (host, table, mean, std, out, labels)

    def run():
        _C.call('evk_augment_batch', host.data_ptr(), table.data_ptr(), n, c, aug.crop_size[0], aug.crop_size[1], ho, wo,
                mean.data_ptr(), std.data_ptr(), aug.mask_pad_value, 0 if aug.channels_last else 1,
                1 if images[0].dtype == torch.float32 else 0, mode, out.data_ptr(), labels.data_ptr(), st)
        return keep
    return run


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
    same = float((fi.contiguous().view(torch.int32) == ci.contiguous().view(torch.int32)).float().mean().item())
    assert torch.equal(fm, cm), 'labels differ'
    times = {'fused': [], 'chain': [], 'fused_host': [], 'chain_host': []}
    for _ in range(args.rounds):
        times['fused'].append(_events(fused, args.iters))
        times['chain'].append(_events(chain, max(2, args.iters // 4)))
        times['fused_host'].append(_host(fused, args.iters))
        times['chain_host'].append(_host(chain, max(2, args.iters // 4)))
    return {k: _median(v) for k, v in times.items()}, same


def bench_rows(args, dev):
    out = []
    cfgs = (('16x1024x1024x3 -> 16x3x512x512', 16, 3, (512, 512), None), ('16x1024x1024x3 -> 16x3x512x512', 16, 3, (512, 512), torch.int64),
            ('8x1024x1024x4 -> 8x4x1024x1024', 8, 4, (1024, 1024), torch.int64))
    for shape, n, c, crop, mask_dtype in cfgs:
        images, masks = _sources(n, 1024, c, dev)
        mo = 8 if mask_dtype is torch.int64 else 1
        nbytes = _algorithmic_bytes(n, c, crop, crop, 1, 1, mo)
        for op in list(range(8)) + ['mixed']:
            fused, chain = _augmenters(op, crop, c, mask_dtype)
            t, same = _compare(args, lambda: fused(images, masks), lambda: chain._per_image(images, masks))
            kern = _kernel_only(args, fused, images, masks)
            kern()
            ku = _median([_events(kern, 4 * args.iters) for _ in range(args.rounds)])
            out.append(dict(shape=shape, labels='int64' if mo == 8 else 'uint8', op=op, kernel_us=round(ku, 1),
                            kernel_tbs=round(nbytes / ku / 1e6, 3), fused_us=round(t['fused'], 1),
                            aten_us=round(t['chain'], 1), speedup=round(t['chain'] / t['fused'], 2),
                            fused_tbs=round(nbytes / t['fused'] / 1e6, 3), fused_host_us=round(t['fused_host'], 1),
                            aten_host_us=round(t['chain_host'], 1), aten_same_bits=round(same, 4)))
        del images, masks
        torch.cuda.empty_cache()
    return out


def bench_forms(args, dev, lib):
    out = []
    n, crop = 16, (512, 512)
    for c, f32 in ((1, False), (3, False), (4, False), (6, False), (8, False), (16, False), (3, True), (4, True), (16, True)):
        images, masks = _sources(n, 1024, c, dev, f32=f32)
        nbytes = _algorithmic_bytes(n, c, crop, crop, 4 if f32 else 1, 1, 1)
        for channels_last in (True, False):
            row = dict(C=c, src='fp32' if f32 else 'uint8', layout='nhwc' if channels_last else 'nchw')
            for op in (1, 3, 5, 7):
                fused, _ = _augmenters(op, crop, c, None, channels_last)
                times = {k: [] for k in (0, 1, 2)}

                kern = _kernel_only(args, fused, images, masks)

                def run(k):
                    lib.evk_augment_force_kernel(k)
                    return kern()

                a = [t.clone() for t in run(0)[4:]]
                for k in (1, 2):
                    b = run(k)[4:]
                    torch.cuda.synchronize()
                    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]), (c, f32, op, k)
                for _ in range(args.rounds):
                    for k in (0, 1, 2):
                        times[k].append(_events(lambda: run(k), 4 * args.iters))
                lib.evk_augment_force_kernel(-1)
                row[f'op{op}'] = {FORMS[k]: dict(us=round(_median(v), 1), tbs=round(nbytes / _median(v) / 1e6, 3))
                                  for k, v in times.items()}
            out.append(row)
        del images, masks
        torch.cuda.empty_cache()
    return out


def _table(res):
    lines = []
    if 'rows' in res:
        lines += ['| batch | labels | op | kernel us | kernel TB/s | fused us | aten chain us | aten / fused | fused TB/s | host us fused | host us aten | same bits |',
                  '|---|---|---|---|---|---|---|---|---|---|---|---|']
        lines += [f"| {r['shape']} | {r['labels']} | {r['op']} | {r['kernel_us']} | {r['kernel_tbs']} | {r['fused_us']} | {r['aten_us']} | {r['speedup']} | {r['fused_tbs']} | "
                  f"{r['fused_host_us']} | {r['aten_host_us']} | {r['aten_same_bits']} |" for r in res['rows']]
    if 'forms' in res:
        lines += ['', '| C | source | layout | ' + ' | '.join(f'op {o} direct / tile / direct4 us' for o in (1, 3, 5, 7)) + ' |', '|---|---|---|---|---|---|---|']
        lines += [f"| {r['C']} | {r['src']} | {r['layout']} | "
                  + ' | '.join(f"{r[f'op{o}']['direct']['us']} / {r[f'op{o}']['tile']['us']} / {r[f'op{o}']['direct4']['us']}" for o in (1, 3, 5, 7)) + ' |'
                  for r in res['forms']]
    return '\n'.join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--skip-rows', action='store_true')
    ap.add_argument('--skip-forms', action='store_true')
    ap.add_argument('--table', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    lib = _C.load()
    res = dict(tool='bench_augment', rounds=args.rounds, iters=args.iters)
    with torch.no_grad():
        if not args.skip_forms:
            res['forms'] = bench_forms(args, dev, lib)
        if not args.skip_rows:
            res['rows'] = bench_rows(args, dev)
    print(json.dumps(res))
    if args.table:
        print(_table(res))


if __name__ == '__main__':
    main()
