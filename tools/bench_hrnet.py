"""dev tool (GPU box): HRNetSeg (HRNetV2-W48 + HRNetHead, 6 classes, cross-entropy) at 16 x 3 x 512^2: forward + backward +
FusedSGD step, reported as tiles/s the way bench.py reports FarSeg (warm-up, then timed steps between two synchronisations).
The batch comes from bench.make_batch.  One JSON line, with how the exchange's terms entered (ever_amd/hip/hr.py:
hr_fuse_stats).  Fails without a device.
usage: python tools/bench_hrnet.py [--steps K] [--warmup W] [--batch B] [--type hrnetv2_w48]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import ever_amd as er  # noqa: E402
from ever_amd import _C  # noqa: E402
from ever_amd.hip import functional as HF  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--type', default='hrnetv2_w48')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    _C.load()
    torch.manual_seed(2333)
    model = er.module.HRNetSeg(dict(encoder=dict(hrnet_type=args.type), head=dict(num_classes=6))).to(dev).train()
    opt = er.opt.FusedSGD(model.parameters(), lr=0.007, momentum=0.9, weight_decay=1e-4)
    x, _ = bench.make_batch(dev, args.batch, 0)
    g = torch.Generator(device=dev).manual_seed(2333)
    y = torch.randint(0, 6, (args.batch, x.shape[2], x.shape[3]), device=dev, generator=g)
    y[:, :8, :8] = 255

    def step():
        out = model(x, y)
        sum(v for k, v in out.items() if k.endswith('loss')).backward()
        opt.step()
        opt.zero_grad(set_to_none=True)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    before = dict(HF.hr_fuse_stats)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    terms = {k: (HF.hr_fuse_stats[k] - before[k]) // args.steps for k in before}
    print(json.dumps(dict(tool='bench_hrnet', metric=f'512x512 tiles/sec fwd+bwd, HRNetSeg {args.type}',
                          value=round(args.batch / dt, 2), unit='tiles/s', step_ms=round(dt * 1e3, 2), batch=args.batch,
                          steps=args.steps, warmup=args.warmup, exchange_terms_per_step=terms,
                          max_memory_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
                          workload=f'HRNetSeg {args.type} + HRNetHead, 6 classes, CE, 3-band 512x512, fwd+bwd+FusedSGD step, '
                                   'inputs resident in HBM')))


if __name__ == '__main__':
    main()
