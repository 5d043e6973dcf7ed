"""dev tool (GPU box): the test-time-augmentation kernels (csrc/d4.hip) in one process.

merge   the fused mean (one evk_d4_merge over the raw model outputs with the inverse ops) against the reference's aten chain on
        the same device (`inv_transform` of each output, then `sum(outs) / len(outs)`), for the full eight-element set and for
        [Identity, HorizontalFlip, VerticalFlip, Rotate90k(1..3)], on 16 x 1 x 512^2, 16 x 6 x 512^2 and 1 x 6 x 2048^2, each
        channels-last and NCHW-contiguous.  The fused result is checked bit for bit against the chain with a true division first.
apply   per swap op, evk_d4_apply through each kernel the plan can be forced onto (evk_d4_force_kernel: 0 scalar element, 1 16-byte
        element, 2 LDS tile) on [N, 512, 512, C], C = 1 ... 64: what places the pixel width below which a swap term takes the tile.

Warm-up first, HIP events, alternating A/B rounds, medians; times in microseconds, algorithmic bytes / time in TB/s (merge:
every term once and the result; apply: one read and one write).  One JSON line.  Fails without a device.
usage: python tools/bench_tta.py [--rounds R] [--iters K] [--skip-apply] [--skip-merge]"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ever_amd  # noqa: E402,F401
from ever_amd import _C  # noqa: E402
from ever_amd.hip import functional as HF  # noqa: E402
from ever_amd.magic.transform import segm  # noqa: E402

SHAPES = ((16, 1, 512, 512), (16, 6, 512, 512), (1, 6, 2048, 2048))
APPLY_C = (1, 3, 4, 6, 8, 16, 32, 64)
KERNELS = ('scalar', 'vec', 'tile')


class _AntiTranspose(ever_amd.Transform):
    def transform(self, inputs):
        return torch.flip(torch.transpose(inputs, 2, 3), [2, 3])

    inv_transform = transform


def _sets():
    six = [segm.Identity(), segm.HorizontalFlip(), segm.VerticalFlip(), segm.Rotate90k(1), segm.Rotate90k(2), segm.Rotate90k(3)]
    return {'d4_8': six + [segm.Transpose(), _AntiTranspose()], 'flips_rot_6': six}


def _op(t):
    return 7 if isinstance(t, _AntiTranspose) else t.d4_op


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # us


def _median(v):
    return sorted(v)[len(v) // 2]


def bench_merge(args, dev):
    out = []
    for n, c, h, w in SHAPES:
        for layout in ('nhwc', 'nchw'):
            for name, cfg in _sets().items():
                g = torch.Generator(device=dev).manual_seed(n + c + len(cfg))
                ops = [_op(t) for t in cfg]
                outs = []       # the raw model outputs: the model saw T_k(image), so output k has T_k's dims
                for op in ops:
                    hk, wk = (w, h) if op & 1 else (h, w)
                    t = torch.randn(n, c, hk, wk, device=dev, generator=g)
                    outs.append(t.contiguous(memory_format=torch.channels_last) if layout == 'nhwc' else t)
                inv = [HF.d4_inverse(op) for op in ops]
                keep = {}

                def fused():
                    keep['fused'] = HF.d4_mean(outs, inv)

                def aten():
                    back = [segm.d4_torch(o, i) for o, i in zip(outs, inv)]
                    keep['aten'] = sum(back) / len(back)

                with torch.no_grad():
                    fused()
                    aten()
                    torch.cuda.synchronize()
                    # the yardstick is the reference expression as the CPU evaluates it: adds in order, then a TRUE division
                    # (a tensor divisor).  aten's device kernel for `tensor / python_number` multiplies by the reciprocal
                    # instead, which is the same only for a power-of-two count: recorded, not required.
                    true_div = sum(segm.d4_torch(o, i) for o, i in zip(outs, inv)) / torch.full((), float(len(outs)), device=dev)
                    bits = [t.contiguous().view(torch.int32) for t in (keep['fused'], true_div, keep['aten'])]
                    assert torch.equal(bits[0], bits[1]), (n, c, h, w, layout, name)
                    aten_same = round(float((bits[0] == bits[2]).float().mean().item()), 4)
                    del true_div, bits
                    times = {'fused': [], 'aten': []}
                    for _ in range(args.rounds):
                        for k, f in (('fused', fused), ('aten', aten)):
                            times[k].append(_time(f, args.iters))
                fu, at = _median(times['fused']), _median(times['aten'])
                nbytes = 4.0 * n * c * h * w * (len(cfg) + 1)
                out.append(dict(shape=f'{n}x{c}x{h}x{w}', layout=layout, set=name, terms=len(cfg), fused_us=round(fu, 1),
                                aten_us=round(at, 1), aten_chain_same_bits=aten_same, fused_tbs=round(nbytes / fu / 1e6, 3), speedup=round(at / fu, 2)))
                del outs, keep
                torch.cuda.empty_cache()
    return out


def bench_apply(args, dev, lib):
    st = torch.cuda.current_stream().cuda_stream
    plan = (ctypes.c_int32 * 6)()
    out = []
    h = w = 512
    for c in APPLY_C:
        n = max(1, 256 // c)      # ~256 MiB per map: input and result together are twice the last-level cache
        x = torch.randn(n, h, w, c, device=dev)
        y = torch.empty(n, w, h, c, device=dev)
        lib.evk_d4_force_kernel(-1)
        lib.evk_d4_plan(n, h, w, c, 1, plan)
        row = dict(C=c, shape=f'{n}x{h}x{w}x{c}', default=KERNELS[plan[0]])
        for op in (1, 3, 5, 7):
            legal = []
            for k in range(3):
                lib.evk_d4_force_kernel(k)
                lib.evk_d4_plan(n, h, w, c, op, plan)
                if plan[0] == k:
                    legal.append(k)
            times = {k: [] for k in legal}

            def run(k):
                lib.evk_d4_force_kernel(k)
                _C.call('evk_d4_apply', x.data_ptr(), y.data_ptr(), n, h, w, c, op, st)

            for k in legal:
                run(k)
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for k in legal:
                    times[k].append(_time(lambda: run(k), args.iters))
            nbytes = 8.0 * x.numel()
            row[f'op{op}'] = {KERNELS[k]: dict(us=round(_median(v), 1), tbs=round(nbytes / _median(v) / 1e6, 3))
                              for k, v in times.items()}
        lib.evk_d4_force_kernel(-1)
        out.append(row)
        del x, y
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--skip-apply', action='store_true')
    ap.add_argument('--skip-merge', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    lib = _C.load()
    res = dict(tool='bench_tta', rounds=args.rounds, iters=args.iters)
    if not args.skip_apply:
        res['apply'] = bench_apply(args, dev, lib)
    if not args.skip_merge:
        res['merge'] = bench_merge(args, dev)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
