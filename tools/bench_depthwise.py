"""dev tool (GPU box): the depthwise kernels (csrc/depthwise.hip) against the block-diagonal dense path they replace, on
the same tensors in the same call: forward and backward (dx + dw + db) in microseconds and algorithmic TB/s (x + y + w
forward; dy + x read, dx written backward).  Warm-up first, HIP events, alternating A/B rounds, medians; one JSON line.
usage: python tools/bench_depthwise.py [--rounds R] [--iters K]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ever_amd  # noqa: E402,F401
from ever_amd import _C  # noqa: E402
from ever_amd.hip import functional as HF  # noqa: E402

SHAPES = [  # (N, C, H, W, k, stride)
    (16, 304, 128, 128, 3, 1),
    (16, 256, 128, 128, 3, 1),
    (16, 128, 128, 128, 3, 2),
]


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=10)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    _C.load()
    out = []
    for n, c, h, w, k, s in SHAPES:
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(n, h, w, c, device=dev, generator=g).permute(0, 3, 1, 2).requires_grad_()
        wt = (torch.randn(c, 1, k, k, device=dev, generator=g) * 0.3).contiguous(memory_format=torch.channels_last)
        wt.requires_grad_()
        b = torch.zeros(c, device=dev, requires_grad=True)
        p = k // 2
        ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        dy = torch.randn(n, ho, wo, c, device=dev, generator=g).permute(0, 3, 1, 2)

        def fwd_dw():
            return HF.depthwise_conv2d(x, wt, b, s, p, 1)

        def fwd_dense():
            return HF.conv2d(x, HF.grouped_dense_weight(wt, c), b, s, p, 1)

        res = {}
        for name, f in (('depthwise', fwd_dw), ('dense', fwd_dense)):
            with torch.no_grad():
                f()
            y = f()
            y.backward(dy)
        torch.cuda.synchronize()
        times = {('depthwise', 'fwd'): [], ('depthwise', 'bwd'): [], ('dense', 'fwd'): [], ('dense', 'bwd'): []}
        for _ in range(args.rounds):
            for name, f in (('depthwise', fwd_dw), ('dense', fwd_dense)):
                with torch.no_grad():
                    times[(name, 'fwd')].append(_time(f, args.iters))
                ys = [f() for _ in range(args.iters)]
                torch.cuda.synchronize()
                it = iter(ys)
                times[(name, 'bwd')].append(_time(lambda: next(it).backward(dy), args.iters))
                del ys
        med = {key: sorted(v)[len(v) // 2] for key, v in times.items()}
        fwd_bytes = 4.0 * (x.numel() + n * c * ho * wo + wt.numel())
        bwd_bytes = 4.0 * (2 * x.numel() + n * c * ho * wo)
        for name in ('depthwise', 'dense'):
            res[name] = dict(fwd_us=round(med[(name, 'fwd')], 1), bwd_us=round(med[(name, 'bwd')], 1),
                             fwd_tbs=round(fwd_bytes / med[(name, 'fwd')] / 1e6, 3),
                             bwd_tbs=round(bwd_bytes / med[(name, 'bwd')] / 1e6, 3))
        res['speedup_fwd'] = round(med[('dense', 'fwd')] / med[('depthwise', 'fwd')], 2)
        res['speedup_bwd'] = round(med[('dense', 'bwd')] / med[('depthwise', 'bwd')], 2)
        out.append(dict(shape=f'{n}x{c}x{h}x{w} k{k} s{s}', fwd_bytes=fwd_bytes, bwd_bytes=bwd_bytes, **res))
        del x, wt, b, dy
        torch.cuda.empty_cache()
    print(json.dumps(dict(tool='bench_depthwise', rounds=args.rounds, iters=args.iters, results=out)))


if __name__ == '__main__':
    main()
