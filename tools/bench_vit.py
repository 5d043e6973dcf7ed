"""Measurements of the ViT path on one MI355X (README "DINOv3 ViT"):

  (a) HF.attention forward and backward against the reference's aten expression (the RoPE chain, the transposes and
      F.scaled_dot_product_attention, fp32) on the same device and the same random data: 16 x 1029 tokens (512 x 512 input,
      4 storage tokens) and 16 x 201 tokens (224 x 224) for ViT-S / B / L (6, 12, 16 heads of 64).  Microseconds, the fraction
      of the 155 TF fp32-MFMA rate (4 N^2 D H B FLOP forward, 10 N^2 D H B backward: five products of 2 N^2 D) and aten / fused
  (b) one ViT-B block, forward + backward, by kernel family (hip/timing.py spans)
  (c) ViTEncoder(vit_base) + FPN(256) + AssymetricDecoder(128), 6 classes, cross entropy, batch 16 of 512 x 512,
      forward + backward + FusedSGD
  (d) python bench.py in a parent tree (--parent DIR, with its own built library) against this tree, four interleaved rounds

    python tools/bench_vit.py [--parts abc] [--reps 20] [--parent DIR] [--out FILE]

Every figure is a median over --reps runs after warm-up; the two sides of (a) run interleaved, rep by rep.  Parts a-c set no
time limit of their own: on a shared GPU machine run the tool under one (`timeout -k 10 300 python tools/bench_vit.py ...`);
each bench.py child of part d has a 600 s limit."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ever_amd as er  # noqa: E402
from ever_amd.hip import functional as HF  # noqa: E402
from ever_amd.hip import timing  # noqa: E402

MFMA_F32 = 155e12        # FLOP/s of v_mfma_f32_*_f32 measured on this part
HBM_PEAK = 8.0e12
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


def _rotate_half(x):
    """element d of the result is -x[d + D/2] in the first half and x[d - D/2] in the second: a roll by D/2 and a sign"""
    half = x.shape[-1] // 2
    sign = torch.ones(x.shape[-1], dtype=x.dtype, device=x.device)
    sign[:half] = -1
    return torch.roll(x, half, dims=-1) * sign


def _aten_attention(qkv, heads, sin, cos):
    """the reference's expression: reshape, unbind, transposes, RoPE on the last rows of q and k, SDPA, transpose back"""
    b, n, c3 = qkv.shape
    c = c3 // 3
    q, k, v = [t.transpose(1, 2) for t in torch.unbind(qkv.reshape(b, n, 3, heads, c // heads), 2)]
    prefix = n - sin.shape[0]

    def rope(t):
        body = t[:, :, prefix:, :]
        return torch.cat((t[:, :, :prefix, :], body * cos + _rotate_half(body) * sin), dim=-2)
    x = F.scaled_dot_product_attention(rope(q), rope(k), v)
    return x.transpose(1, 2).reshape(b, n, c)


def part_a(dev, reps):
    say('(a) HF.attention against the aten expression, same device, same random data, interleaved; fraction of the 155 TF fp32 '
        'MFMA rate; aten / fused')
    for n, hw in ((1029, 1024), (201, 196)):
        for name, heads in (('ViT-S', 6), ('ViT-B', 12), ('ViT-L', 16)):
            b, d = 16, 64
            qkv = torch.randn(b, n, 3 * heads * d, device=dev)
            ang = torch.rand(hw, d // 2, device=dev).tile(2) * 6.28
            sin, cos = torch.sin(ang), torch.cos(ang)
            gy = torch.randn(b, n, heads * d, device=dev)
            qh, qa = qkv.clone().requires_grad_(), qkv.clone().requires_grad_()
            yh, ya = HF.attention(qh, heads, (sin, cos)), _aten_attention(qa, heads, sin, cos)
            err = float((yh - ya).detach().abs().max())

            def hip_f():
                with torch.no_grad():
                    HF.attention(qkv, heads, (sin, cos))

            def at_f():
                with torch.no_grad():
                    _aten_attention(qkv, heads, sin, cos)

            def hip_b():
                torch.autograd.grad(yh, qh, gy, retain_graph=True)

            def at_b():
                torch.autograd.grad(ya, qa, gy, retain_graph=True)
            flop = 4.0 * n * n * d * heads * b
            for what, fns, fl in (('forward', (hip_f, at_f), flop), ('backward', (hip_b, at_b), 2.5 * flop)):
                us_h, us_a = _time_pair(fns, reps)
                say(f'{name} {b} x {n:4d} x {heads:2d} x {d} {what:8s} {us_h:9.1f} us {fl / us_h * 1e6 / MFMA_F32:6.3f} of 155 TF | aten '
                    f'{us_a:9.1f} us | aten / fused {us_a / us_h:5.2f}x' + ('   <-- fused is SLOWER' if us_h > us_a else ''))
            say(f'    max |fused - aten| of the output {err:.2e}')
            del yh, ya, qh, qa
    say()


def part_b(dev, reps):
    say('(b) one ViT-B block (768 channels, 12 heads), 16 x 1029 tokens, forward + backward, by kernel family (median of the '
        'per-run sums; bound = algorithmic bytes at 8 TB/s or FLOPs at the fp16 matrix peak / 3 partial products, whichever is '
        'larger; the attention family\'s FLOPs are fp32-MFMA FLOPs: its bound at 155 TF is printed beside it)')
    from ever_amd.module.dinov3 import RopePositionEmbedding, SelfAttentionBlock
    from ever_amd.module.layers import LayerNorm
    HF.set_wgrad_stream(False)           # the kernels one after the other on one stream, as bench.py times them
    blk = SelfAttentionBlock(768, 12, qkv_bias=True, init_values=1e-5, norm_layer=LayerNorm).to(dev).train()
    for m in blk.modules():
        if hasattr(m, 'reset_parameters'):
            m.reset_parameters()
    rope = RopePositionEmbedding(768, num_heads=12, dtype=torch.float32).to(dev)(H=32, W=32)
    x = torch.randn(16, 1029, 768, device=dev).requires_grad_()
    gy = torch.randn(16, 1029, 768, device=dev)

    def run():
        for p in blk.parameters():
            p.grad = None
        x.grad = None
        blk(x, rope).backward(gy)
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
            fam.setdefault(k, []).append((d['seconds'], d['bound_seconds'], d['launches'], d['bytes'], d.get('flops', 0.0)))
    total = sum(statistics.median(v[0] for v in vs) for vs in fam.values())
    say(f'block: {total * 1e6:9.1f} us in timed spans')
    for k in sorted(fam, key=lambda k: -statistics.median(v[0] for v in fam[k])):
        sec = statistics.median(v[0] for v in fam[k])
        bound, launches = fam[k][0][1], fam[k][0][2]
        extra = f'   fp32-MFMA bound {fam[k][0][4] / MFMA_F32 * 1e6:8.1f} us' if k == 'attention' else ''
        say(f'    {k:14s} {launches:3d} launches {sec * 1e6:9.1f} us  {100 * sec / total:5.1f} %   bound {bound * 1e6:8.1f} us '
            f'({sec / max(bound, 1e-12):5.2f}x)' + extra)
    HF.set_wgrad_stream(True)
    say()


def part_c(dev, reps):
    say('(c) ViTEncoder(vit_base) + FPN(256) + AssymetricDecoder(128), 6 classes, cross entropy, batch 16 of 512 x 512, '
        'forward + backward + FusedSGD')

    class Seg(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.en = er.module.ViTEncoder(dict(vit_type='vit_base', vit_kwargs=dict(n_storage_tokens=4, layerscale_init=1e-5)))
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


def part_d(parent, rounds=4):
    say(f'(d) python bench.py --gpus 1 --steps 40 --warmup 5 --no-cpu-baseline, parent tree against this tree, {rounds} interleaved '
        'rounds (odd rounds parent first); the step calls none of the new code')
    res = {'parent': [], 'new': []}
    for r in range(rounds):
        order = ('parent', 'new') if r % 2 == 0 else ('new', 'parent')
        for side in order:
            cwd = parent if side == 'parent' else ROOT
            p = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', '40', '--warmup', '5', '--no-cpu-baseline'],
                               cwd=cwd, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                say(f'    round {r + 1} {side}: bench.py failed with status {p.returncode}; stopping')
                say(p.stderr[-400:])
                return
            line = json.loads(p.stdout.strip().splitlines()[-1])
            res[side].append(line['value'])
            say(f'    round {r + 1} {side:6s} {line["value"]:8.2f} tiles/s {line["ms_per_step"]:8.3f} ms/step '
                f'host enqueue {line["host_enqueue_ms_per_step"]:7.3f} ms/step')
    for side, v in res.items():
        say(f'    range {side:6s} {min(v):.2f} .. {max(v):.2f}   mean {statistics.mean(v):.2f}')
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='abc')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--parent', default=None, help='a checkout of the parent commit with its own built library, for part d')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if 'd' in args.parts:          # first, before this process opens the device: bench.py runs in children
        if not args.parent:
            sys.exit('part d needs --parent DIR')
        part_d(args.parent)
    if set(args.parts) & set('abc'):
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
