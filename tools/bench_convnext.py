"""Measurements of the ConvNeXt path on one MI355X (README "ConvNeXt"):

  (a) evk_ln_fwd / evk_ln_bwd and evk_scale_residual_fwd / _bwd against the aten expressions on the same device, at the stage
      shapes of convnext_tiny and convnext_base for a 16 x 3 x 512 x 512 batch: microseconds and TB/s of algorithmic bytes
  (b) one block per stage of convnext_tiny, forward + backward, by kernel family (hip/timing.py spans), with the 7x7
      depthwise kernel's time against its byte bound
  (c) ConvNeXtEncoder(tiny) + FPN + AssymetricDecoder, 6 classes, cross entropy, batch 16, forward + backward + FusedSGD

    python tools/bench_convnext.py [--parts abc] [--reps 20] [--out FILE]

Every figure is a median over --reps runs after warm-up; the two sides of (a) run interleaved, rep by rep."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ever_amd as er  # noqa: E402
from ever_amd import _C  # noqa: E402
from ever_amd.hip import functional as HF  # noqa: E402
from ever_amd.hip import timing  # noqa: E402

HBM_PEAK = 8.0e12        # bytes/s (MI355X data sheet); the copy kernels of this project reach ~6.1e12
SHAPES = {'tiny': [(262144, 96), (65536, 192), (16384, 384), (4096, 768)],
          'base': [(262144, 128), (65536, 256), (16384, 512), (4096, 1024)]}
EPS, KEEP = 1e-6, 0.9
LINES = []


def say(s=''):
    print(s, flush=True)
    LINES.append(s)


def _time_pair(fns, reps, warm=3):
    """median microseconds of each callable, run interleaved rep by rep"""
    for _ in range(warm):
        for f in fns:
            f()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b) * 1e3)
    return [statistics.median(t) for t in ts]


def _row(what, r, c, nbytes, us_hip, us_aten):
    say(f'{what:22s} {r:7d} x {c:4d}  {us_hip:9.1f} us {nbytes / us_hip * 1e-6:6.2f} TB/s | aten {us_aten:9.1f} us '
        f'{nbytes / us_aten * 1e-6:6.2f} TB/s | aten / fused {us_aten / us_hip:5.2f}x' + ('   <-- fused is SLOWER' if us_hip > us_aten else ''))


def part_a(dev, reps):
    say('(a) fused kernels against aten, same device, interleaved; TB/s of algorithmic bytes (LayerNorm 2|x| forward, 3|x| backward; '
        'layer-scale residual 3|x| each way)')
    lib = _C.load()
    st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    n = 16
    for size, shapes in SHAPES.items():
        say(f'convnext_{size}')
        for r, c in shapes:
            hw = r // n
            x, dy = torch.randn(r, c, device=dev), torch.randn(r, c, device=dev)
            g, b = torch.rand(c, device=dev) + 0.5, torch.randn(c, device=dev)
            y, dx = torch.empty_like(x), torch.empty_like(x)
            mean, rstd = torch.empty(r, device=dev), torch.empty(r, device=dev)
            dg, db = torch.empty(c, device=dev), torch.empty(c, device=dev)
            wsb = lib.evk_ln_bwd_workspace_bytes(r, c)
            ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
            nb = 4.0 * r * c

            def ln_f():
                _C.call('evk_ln_fwd', x.data_ptr(), g.data_ptr(), b.data_ptr(), EPS, y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                        r, c, st())

            def ln_b():
                _C.call('evk_ln_bwd', dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), g.data_ptr(), dx.data_ptr(),
                        dg.data_ptr(), db.data_ptr(), r, c, ws.data_ptr(), wsb, st())
            xa, ga, ba = x.clone().requires_grad_(), g.clone().requires_grad_(), b.clone().requires_grad_()
            ya = F.layer_norm(xa, (c,), ga, ba, EPS)

            def at_f():
                with torch.no_grad():
                    F.layer_norm(x, (c,), g, b, EPS)

            def at_b():
                torch.autograd.grad(ya, (xa, ga, ba), dy, retain_graph=True)
            us = _time_pair([ln_f, at_f], reps)
            _row('layer_norm forward', r, c, 2 * nb, *us)
            us = _time_pair([ln_b, at_b], reps)
            _row('layer_norm backward', r, c, 3 * nb, *us)
            del ya, xa
            # the block tail: input + drop_path(gamma * z)
            a, z = torch.randn(r, c, device=dev), torch.randn(r, c, device=dev)
            s = (torch.floor(KEEP + torch.rand(n, device=dev)) / KEEP).contiguous()
            dz = torch.empty_like(z)
            wsb2 = lib.evk_scale_residual_bwd_workspace_bytes(n, hw, c)

            def sr_f():
                _C.call('evk_scale_residual_fwd', a.data_ptr(), z.data_ptr(), g.data_ptr(), s.data_ptr(), y.data_ptr(), n, hw, c, st())

            def sr_b():
                _C.call('evk_scale_residual_bwd', dy.data_ptr(), z.data_ptr(), g.data_ptr(), s.data_ptr(), dz.data_ptr(),
                        dg.data_ptr(), n, hw, c, ws.data_ptr(), wsb2, st())
            a4, z4 = a.view(n, hw, c), z.view(n, hw, c)
            mask = (s * KEEP).view(n, 1, 1)

            def expr(zz, gg):
                return a4 + (gg * zz).div(KEEP) * mask
            za, ga = z4.clone().requires_grad_(), g.clone().requires_grad_()
            out = expr(za, ga)

            def at_sf():
                with torch.no_grad():
                    expr(z4, g)

            def at_sb():
                torch.autograd.grad(out, (za, ga), dy.view(n, hw, c), retain_graph=True)
            us = _time_pair([sr_f, at_sf], reps)
            _row('scale_residual forward', r, c, 3 * nb, *us)
            us = _time_pair([sr_b, at_sb], reps)
            _row('scale_residual backwd', r, c, 3 * nb, *us)
            del out, za
    say()


def part_b(dev, reps):
    say('(b) one convnext_tiny block per stage, batch 16 of 512 x 512, forward + backward, by kernel family '
        '(median of the per-run sums; bound = algorithmic bytes at 8 TB/s or FLOPs at the fp16 matrix peak / 3 partial products, whichever is larger)')
    from ever_amd.module.dinov3 import Block
    HF.set_wgrad_stream(False)           # the kernels one after the other on one stream, as bench.py times them
    for (r, c) in SHAPES['tiny']:
        side = int((r // 16) ** 0.5)
        blk = Block(c, drop_path=0.1, layer_scale_init_value=1e-6).to(dev).train()
        x = HF.empty_nhwc(16, c, side, side, dev).normal_().requires_grad_()
        gy = HF.empty_nhwc(16, c, side, side, dev).normal_()

        def run():
            for p in blk.parameters():
                p.grad = None
            x.grad = None
            blk(x).backward(gy)
            HF.wait_wgrad_stream()
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        fam = {}
        for _ in range(reps):
            with timing.KernelTimer() as kt:
                run()
            torch.cuda.synchronize()
            for k, d in kt.summary(peak_flops=2.5e15 / 3, peak_bytes=HBM_PEAK).items():
                fam.setdefault(k, []).append((d['seconds'], d['bound_seconds'], d['launches'], d['bytes']))
        total = sum(statistics.median(v[0] for v in vs) for vs in fam.values())
        say(f'stage {c:4d} channels, {side} x {side}: {total * 1e6:9.1f} us in timed spans')
        for k in sorted(fam, key=lambda k: -statistics.median(v[0] for v in fam[k])):
            sec = statistics.median(v[0] for v in fam[k])
            bound, launches, nbytes = fam[k][0][1], fam[k][0][2], fam[k][0][3]
            say(f'    {k:14s} {launches:3d} launches {sec * 1e6:9.1f} us  {100 * sec / total:5.1f} %   bound {bound * 1e6:8.1f} us '
                f'({sec / max(bound, 1e-12):5.2f}x)   {nbytes / sec * 1e-12 if sec else 0:5.2f} TB/s')
    HF.set_wgrad_stream(True)
    say('    (depthwise: the 7x7 kernel runs on a tiling chosen for 3x3; its line above is the number for a later retune)')
    say()


def part_c(dev, reps):
    say('(c) ConvNeXtEncoder(convnext_tiny) + FPN(256) + AssymetricDecoder(128), 6 classes, cross entropy, batch 16 of 512 x 512, '
        'forward + backward + FusedSGD')

    class Seg(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.en = er.module.ConvNeXtEncoder(dict(convnext_type='convnext_tiny', drop_path_rate=0.1))
            self.fpn = er.module.FPN(self.en.output_channels(), 256)
            self.decoder = er.module.AssymetricDecoder(256, 128, classifier_config=dict(num_classes=6, scale_factor=4))

        def forward(self, x):
            return self.decoder(self.fpn(self.en(x)))
    m = Seg().to(dev).train()
    opt = er.opt.FusedSGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    x = torch.randn(16, 3, 512, 512, device=dev)
    y = torch.randint(0, 6, (16, 512, 512), device=dev)

    def step():
        loss = HF.cross_entropy(m(x), y, ignore_index=255)
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        return loss
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        loss = step()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    med = statistics.median(ts)
    say(f'    step {med * 1e3:8.2f} ms (min {min(ts) * 1e3:.2f}, max {max(ts) * 1e3:.2f}) = {16 / med:7.1f} tiles/s; loss {loss.item():.4f}; '
        f'peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB')
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='abc')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    say(f'{torch.cuda.get_device_name(0)}, torch {torch.__version__}, conv math {HF.get_conv_math()}, {args.reps} reps')
    for p, fn in (('a', part_a), ('b', part_b), ('c', part_c)):
        if p in args.parts:
            fn(dev, args.reps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
