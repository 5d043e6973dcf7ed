"""dev tool (GPU box): the HRNet exchange kernels (csrc/hr_fuse.hip) against the same arithmetic composed from aten ops on
channels_last tensors, on the four stage-4 output shapes of HRNetV2-W48 at 16 x 3 x 512^2, in one process.  Forward: y =
ReLU(sum of the terms), a BatchNorm term as scale / shift of the raw map, an up-sampled term read in place (fused) or
addcmul -> nearest interpolate -> add per term -> relu (aten).  Backward: the masked gradient and its block sums for every
coarser term, from one read of dy (fused) or threshold_backward + one sum-pool per shift (aten).  The parent commit cannot run
HRNet at all, so the aten composition is the baseline.  Warm-up first, HIP events, alternating A/B rounds, medians; times in
microseconds and algorithmic bytes / time in TB/s (the bytes of the fused form: every term once at its own size, y and its
bits; dy, the bits, the masked gradient and the pools).  One JSON line.  Fails without a device.
usage: python tools/bench_hr_fuse.py [--rounds R] [--iters K] [--batch B]"""
import argparse
import ctypes
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ever_amd  # noqa: E402,F401
from ever_amd import _C  # noqa: E402

CH, HW = (48, 96, 192, 384), (128, 64, 32, 16)      # HRNetV2-W48 branches on a 512^2 image


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
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--batch', type=int, default=16)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    lib = _C.load()
    st = torch.cuda.current_stream().cuda_stream
    n, out = args.batch, []
    for i in range(4):
        c, h = CH[i], HW[i]
        g = torch.Generator(device=dev).manual_seed(1 + i)
        terms = []      # (map as logical NCHW over NHWC memory, shift, scale_shift or None): j ascending, as the module
        for j in range(4):
            s = max(j - i, 0)
            z = torch.randn(n, h >> s, h >> s, c, device=dev, generator=g).permute(0, 3, 1, 2)
            ss = None if j == i else torch.stack([torch.rand(c, device=dev, generator=g) + 0.5,
                                                  0.2 * torch.randn(c, device=dev, generator=g)])
            terms.append((z, s, ss))
        dy = torch.randn(n, h, h, c, device=dev, generator=g).permute(0, 3, 1, 2)
        shifts = sorted({s for _, s, _ in terms if s})
        y = torch.empty_like(dy)
        bits = torch.empty((lib.evk_relu_bits_bytes(y.numel()) // 4,), device=dev, dtype=torch.int32)
        dm = torch.empty_like(dy)
        pools = {s: torch.empty((n, h >> s, h >> s, c), device=dev) for s in shifts}
        tp = (ctypes.c_void_p * 4)(*[z.data_ptr() for z, _, _ in terms])
        sh = (ctypes.c_int32 * 4)(*[s for _, s, _ in terms])
        sp = (ctypes.c_void_p * 4)(*[None if ss is None else ss.data_ptr() for _, _, ss in terms])

        def fused_fwd():
            _C.call('evk_hr_fuse_fwd', tp, sh, sp, 4, y.data_ptr(), bits.data_ptr(), None, n, h, h, c, st)

        def fused_bwd():
            _C.call('evk_hr_fuse_bwd', dy.data_ptr(), bits.data_ptr(), dm.data_ptr(),
                    *[pools[s].data_ptr() if s in pools else None for s in (1, 2, 3)], n, h, h, c, st)

        keep = {}

        def aten_fwd():
            acc = None
            for z, s, ss in terms:
                t = z if ss is None else torch.addcmul(ss[1].view(1, c, 1, 1), z, ss[0].view(1, c, 1, 1))
                if s:
                    t = F.interpolate(t, scale_factor=1 << s, mode='nearest')
                acc = t if acc is None else acc + t
            keep['y'] = torch.relu(acc)

        def aten_bwd():
            m = torch.ops.aten.threshold_backward(dy, keep['y'], 0)
            keep['p'] = [F.avg_pool2d(m, 1 << s, divisor_override=1) for s in shifts]

        with torch.no_grad():
            for f in (fused_fwd, aten_fwd, fused_bwd, aten_bwd):
                f()
            torch.cuda.synchronize()
            # the two arms compute the same thing
            assert (y - keep['y']).abs().max().item() < 1e-4
            assert (dm - torch.ops.aten.threshold_backward(dy, y, 0)).abs().max().item() == 0
            for s, p in zip(shifts, keep['p']):
                assert (pools[s].permute(0, 3, 1, 2) - p).abs().max().item() < 1e-3
            times = {k: [] for k in ('fused_fwd', 'aten_fwd', 'fused_bwd', 'aten_bwd')}
            for _ in range(args.rounds):
                for name, f in (('fused_fwd', fused_fwd), ('aten_fwd', aten_fwd), ('fused_bwd', fused_bwd), ('aten_bwd', aten_bwd)):
                    times[name].append(_time(f, args.iters))
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        fwd_bytes = 4.0 * (sum(z.numel() for z, _, _ in terms) + y.numel() + bits.numel())
        bwd_bytes = 4.0 * (2 * dy.numel() + bits.numel() + sum(p.numel() for p in pools.values()))
        out.append(dict(output=i, shape=f'{n}x{c}x{h}x{h}', term_shifts=[s for _, s, _ in terms],
                        fwd_bytes=fwd_bytes, bwd_bytes=bwd_bytes,
                        fused=dict(fwd_us=round(med['fused_fwd'], 1), bwd_us=round(med['fused_bwd'], 1),
                                   fwd_tbs=round(fwd_bytes / med['fused_fwd'] / 1e6, 3),
                                   bwd_tbs=round(bwd_bytes / med['fused_bwd'] / 1e6, 3)),
                        aten=dict(fwd_us=round(med['aten_fwd'], 1), bwd_us=round(med['aten_bwd'], 1)),
                        speedup_fwd=round(med['aten_fwd'] / med['fused_fwd'], 2),
                        speedup_bwd=round(med['aten_bwd'] / med['fused_bwd'], 2)))
        del terms, dy, y, bits, dm, pools, keep
        torch.cuda.empty_cache()
    print(json.dumps(dict(tool='bench_hr_fuse', rounds=args.rounds, iters=args.iters, batch=n, results=out)))


if __name__ == '__main__':
    main()
