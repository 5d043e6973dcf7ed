"""dev tool (GPU box): the weighted-fusion kernels (csrc/wfuse.hip) against the same arithmetic from aten ops on the same device
(the reference's expression, fpn.py:206-218, 265: UpsamplingNearest2d -> stack -> broadcast multiply -> sum, and its autograd
backward), on 16 x 256 x {128^2, 64^2, 32^2, 16^2} NHWC maps, for the two-term node with one shifted term and for the
three-term node; then a BiFPN(256, [4, 8, 16, 32]) forward + backward step on the fused path and on the layer-by-layer path
(a forward hook on every up-sampling module, which materialises the nearest x2).  The parent commit has no BiFPN, so the aten
chain in the same process is the yardstick.  Warm-up first, HIP events, alternating A/B rounds, medians; times in microseconds
and algorithmic bytes / time in TB/s (the bytes of the fused form: every term once at its own size and y; dy, every term
gradient and every term once more for the weight gradient).  One JSON line.  Fails without a device.
usage: python tools/bench_bifpn.py [--rounds R] [--iters K] [--batch B] [--no-step]"""
import argparse
import ctypes
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ever_amd as er  # noqa: E402
from ever_amd import _C  # noqa: E402

C, HW = 256, (128, 64, 32, 16)
FORMS = {'two terms, one shifted': (0, 1), 'three terms': (0, 0, 0)}
EPS = 1e-4


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


def _alternate(arms, rounds, iters):
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, f in arms.items():
            times[k].append(_time(f, iters))
    return {k: _median(v) for k, v in times.items()}, {k: (min(v), max(v)) for k, v in times.items()}


def node(lib, n, h, shifts, dev, rounds, iters):
    k = len(shifts)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev).manual_seed(h + k)
    ts = [torch.randn(n, h >> s, h >> s, C, device=dev, generator=g).permute(0, 3, 1, 2) for s in shifts]
    dy = torch.randn(n, h, h, C, device=dev, generator=g).permute(0, 3, 1, 2)
    w = torch.tensor([0.7, 1.6, 0.4][:k], device=dev)
    y = torch.empty_like(dy)
    dts = [torch.empty_like(t) for t in ts]
    dw = torch.empty(k, device=dev)
    ws_bytes = lib.evk_wfuse_workspace_bytes(n, h, h, C, k)
    ws = torch.empty(ws_bytes // 4, device=dev)
    tp = (ctypes.c_void_p * k)(*[t.data_ptr() for t in ts])
    dp = (ctypes.c_void_p * k)(*[t.data_ptr() for t in dts])
    sh = (ctypes.c_int32 * k)(*shifts)

    def fused_fwd():
        _C.call('evk_wfuse_fwd', tp, sh, k, w.data_ptr(), 0, EPS, y.data_ptr(), n, h, h, C, st)

    def fused_bwd():
        _C.call('evk_wfuse_bwd', dy.data_ptr(), tp, sh, k, w.data_ptr(), 0, EPS, dp, dw.data_ptr(), ws.data_ptr(), ws_bytes,
                n, h, h, C, st)

    leaves = [t.detach().requires_grad_() for t in ts] + [w.detach().requires_grad_()]
    keep = {}

    def aten_fwd():
        fs = [F.interpolate(t, scale_factor=2.0, mode='nearest') if s else t for t, s in zip(leaves[:k], shifts)]
        r = F.relu(leaves[k])
        wn = r / (torch.sum(r, dim=0, keepdim=True) + EPS)
        keep['y'] = torch.sum(wn.view(k, 1, 1, 1, 1) * torch.stack(fs, dim=0), dim=0)

    def aten_bwd():
        keep['g'] = torch.autograd.grad(keep['y'], leaves, dy, retain_graph=True)

    for f in (fused_fwd, aten_fwd, fused_bwd, aten_bwd):
        f()
    torch.cuda.synchronize()
    # the two arms compute the same thing
    assert (y - keep['y']).abs().max().item() < 1e-4
    for a, b in zip(dts, keep['g'][:k]):
        assert (a - b).abs().max().item() < 1e-4
    dw_pair = dict(fused=[round(v, 4) for v in dw.tolist()], aten=[round(v, 4) for v in keep['g'][k].tolist()])   # (reported:
    # aten's is a chain of fp32 reductions over the whole map, the kernel's a double sum of bounded fp32 partials)
    med, spread = _alternate(dict(fused_fwd=fused_fwd, aten_fwd=aten_fwd, fused_bwd=fused_bwd, aten_bwd=aten_bwd), rounds, iters)
    fwd_bytes = 4.0 * (sum(t.numel() for t in ts) + y.numel())
    bwd_bytes = 4.0 * (dy.numel() + 2 * sum(t.numel() for t in ts))
    return dict(shape=f'{n}x{C}x{h}x{h}', shifts=list(shifts), fwd_bytes=fwd_bytes, bwd_bytes=bwd_bytes,
                fused=dict(fwd_us=round(med['fused_fwd'], 1), bwd_us=round(med['fused_bwd'], 1),
                           fwd_tbs=round(fwd_bytes / med['fused_fwd'] / 1e6, 3), bwd_tbs=round(bwd_bytes / med['fused_bwd'] / 1e6, 3)),
                aten=dict(fwd_us=round(med['aten_fwd'], 1), bwd_us=round(med['aten_bwd'], 1)),
                spread_us={k: [round(a, 1), round(b, 1)] for k, (a, b) in spread.items()}, dweights=dw_pair,
                speedup_fwd=round(med['aten_fwd'] / med['fused_fwd'], 2), speedup_bwd=round(med['aten_bwd'] / med['fused_bwd'], 2))


def step(n, dev, rounds, iters):
    torch.manual_seed(0)
    fused = er.module.BiFPN(C, [4, 8, 16, 32]).to(dev).train()
    import copy
    layered = copy.deepcopy(fused)
    for up in layered.upsample_modules:
        up.register_forward_hook(lambda m, i, o: None)
    g = torch.Generator(device=dev).manual_seed(7)
    xs = [torch.randn(n, h, h, C, device=dev, generator=g).permute(0, 3, 1, 2).requires_grad_() for h in HW]
    gs = [torch.randn(n, h, h, C, device=dev, generator=g).permute(0, 3, 1, 2) for h in HW]

    def run(m):
        def f():
            for p in m.parameters():
                p.grad = None
            for x in xs:
                x.grad = None
            torch.autograd.backward(m(list(xs)), gs)
        return f

    arms = dict(fused=run(fused), layer_by_layer=run(layered))
    for f in arms.values():
        f()
    torch.cuda.synchronize()
    med, spread = _alternate(arms, rounds, max(iters // 4, 2))
    return dict(model=f'BiFPN({C}, [4, 8, 16, 32])', maps=[f'{n}x{C}x{h}x{h}' for h in HW],
                fused_us=round(med['fused'], 1), layer_by_layer_us=round(med['layer_by_layer'], 1),
                spread_us={k: [round(a, 1), round(b, 1)] for k, (a, b) in spread.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--no-step', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    lib = _C.load()
    out = []
    for name, shifts in FORMS.items():
        for h in HW:
            out.append(dict(form=name, **node(lib, args.batch, h, shifts, dev, args.rounds, args.iters)))
            torch.cuda.empty_cache()
    res = dict(tool='bench_bifpn', rounds=args.rounds, iters=args.iters, batch=args.batch, nodes=out)
    if not args.no_step:
        res['step'] = step(args.batch, dev, args.rounds, args.iters)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
