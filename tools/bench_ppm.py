"""dev tool (GPU box): the pyramid-pooling kernels (csrc/ppm.hip) against the same arithmetic from aten ops on the same device
(the reference's expression, ops.py:92-100 and ppm.py:31-33: K adaptive average pools, K bilinear align_corners=False
interpolations, torch.cat, and its autograd backward) on 16 x 2048 x 64^2, 16 x 2048 x 32^2 and 16 x 512 x 64^2 NHWC maps with
512 pooled channels and bins (1, 2, 3, 6); then a PyramidPoolModule forward + backward on the fused path and layer by layer
(aten's pool, interpolate and cat around the module's own blocks), and one PSPNet-R50 training step (3 x 512^2, batch 16,
6 classes).  The parent commit has no pyramid pooling, so the aten chain in the same process is the yardstick.  Warm-up
first, HIP events, alternating rounds, medians; times in microseconds and algorithmic bytes / time in TB/s (the bytes of
the fused form: x and the pools; x, the pooled maps and the concat map; the pooled slices of dcat and dz; the skip slice,
dp and dx).  One JSON line.  Fails without a device.
usage: python tools/bench_ppm.py [--rounds R] [--iters K] [--batch B] [--no-step]"""
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

BINS, CP = (1, 2, 3, 6), 512
SHAPES = [(2048, 64), (2048, 32), (512, 64)]


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # us


def _alternate(arms, rounds, iters):
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, f in arms.items():
            times[k].append(_time(f, iters))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    return med, {k: [round(min(v), 1), round(max(v), 1)] for k, v in times.items()}


def _nhwc(n, c, h, w, dev, g):
    return torch.randn(n, h, w, c, device=dev, generator=g).permute(0, 3, 1, 2)


def kernels(lib, n, c, h, dev, rounds, iters):
    k = len(BINS)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev).manual_seed(c + h)
    x = _nhwc(n, c, h, h, dev, g)
    zs = [_nhwc(n, CP, b, b, dev, g) for b in BINS]
    dcat = _nhwc(n, c + k * CP, h, h, dev, g)
    ps = [torch.empty(n, b, b, c, device=dev).permute(0, 3, 1, 2) for b in BINS]
    dps = [_nhwc(n, c, b, b, dev, g) for b in BINS]
    dzs = [torch.empty_like(z) for z in zs]
    cat, dx = torch.empty_like(dcat), torch.empty_like(x)
    ba = (ctypes.c_int32 * k)(*BINS)
    tab = lambda ts: (ctypes.c_void_p * k)(*[t.data_ptr() for t in ts])       # noqa: E731
    pws = lib.evk_ppm_pool_workspace_bytes(n, h, h, c, ba, k)
    ews = lib.evk_ppm_expand_bwd_workspace_bytes(n, h, h, c, CP, ba, k)
    ws = torch.empty(max(pws, ews) // 4, device=dev)
    pt, zt, dzt, dpt = tab(ps), tab(zs), tab(dzs), tab(dps)

    def pool_fwd():
        _C.call('evk_ppm_pool_fwd', x.data_ptr(), pt, ba, k, n, h, h, c, ws.data_ptr(), pws, st)

    def expand_fwd():
        _C.call('evk_ppm_expand_fwd', x.data_ptr(), zt, ba, k, cat.data_ptr(), n, h, h, c, CP, st)

    def expand_bwd():
        _C.call('evk_ppm_expand_bwd', dcat.data_ptr(), dzt, ba, k, n, h, h, c, CP, ws.data_ptr(), ews, st)

    def pool_bwd():
        _C.call('evk_ppm_pool_bwd', dpt, ba, k, dcat.data_ptr(), c + k * CP, dx.data_ptr(), n, h, h, c, st)

    xl = x.detach().requires_grad_()
    zl = [z.detach().requires_grad_() for z in zs]
    keep = {}

    def aten_pool_fwd():
        keep['p'] = [F.adaptive_avg_pool2d(xl, b) for b in BINS]

    def aten_expand_fwd():
        keep['cat'] = torch.cat([xl] + [F.interpolate(z, (h, h), mode='bilinear', align_corners=False) for z in zl], dim=1)

    def aten_expand_bwd():      # the concat's backward: the K interpolation gradients and the slice copy for x
        keep['gz'] = torch.autograd.grad(keep['cat'], [xl] + zl, dcat, retain_graph=True)

    def aten_pool_bwd():        # the K pool gradients and autograd's sum of them with the skip gradient
        gs = torch.autograd.grad(keep['p'], [xl] * 1, dps, retain_graph=True)[0]
        keep['gx'] = gs + keep['gz'][0]

    fused = dict(pool_fwd=pool_fwd, expand_fwd=expand_fwd, expand_bwd=expand_bwd, pool_bwd=pool_bwd)
    aten = dict(pool_fwd=aten_pool_fwd, expand_fwd=aten_expand_fwd, expand_bwd=aten_expand_bwd, pool_bwd=aten_pool_bwd)
    for f in list(fused.values()) + list(aten.values()):
        f()
    torch.cuda.synchronize()
    # the two arms compute the same thing
    for a, b in zip(ps, keep['p']):
        assert (a - b).abs().max().item() < 1e-4
    assert (cat - keep['cat']).abs().max().item() < 1e-4
    for a, b in zip(dzs, keep['gz'][1:]):
        assert (a - b).abs().max().item() < 1e-3 * max(b.abs().max().item(), 1.0)
    assert (dx - keep['gx']).abs().max().item() < 1e-4
    arms = {'fused_' + name: f for name, f in fused.items()}
    arms.update({'aten_' + name: f for name, f in aten.items()})
    med, spread = _alternate(arms, rounds, iters)
    nbytes = dict(pool_fwd=4.0 * (x.numel() + sum(p.numel() for p in ps)),
                  expand_fwd=4.0 * (x.numel() + sum(z.numel() for z in zs) + cat.numel()),
                  expand_bwd=4.0 * (n * h * h * k * CP + sum(z.numel() for z in zs)),
                  pool_bwd=4.0 * (2 * x.numel() + sum(p.numel() for p in dps)))
    out = dict(shape=f'{n}x{c}x{h}x{h}', pool_channels=CP, bins=list(BINS))
    for name in fused:
        fu, at = med['fused_' + name], med['aten_' + name]
        out[name] = dict(bytes=nbytes[name], fused_us=round(fu, 1), aten_us=round(at, 1),
                         fused_tbs=round(nbytes[name] / fu / 1e6, 3), aten_tbs=round(nbytes[name] / at / 1e6, 3),
                         speedup=round(at / fu, 2), spread_us=dict(fused=spread['fused_' + name], aten=spread['aten_' + name]))
    return out


def _layer_by_layer(m, x):
    size = x.shape[-2:]
    out = [x]
    for blk, b in zip(m.pools, m.bins):
        out.append(F.interpolate(blk[1](F.adaptive_avg_pool2d(x, b)), size=size, mode='bilinear', align_corners=False))
    return m.dropout(m.conv(torch.cat(out, dim=1)))


def module(n, c, h, dev, rounds, iters):
    torch.manual_seed(0)
    m = er.module.PyramidPoolModule(c, CP, 512, BINS).to(dev).train()
    g = torch.Generator(device=dev).manual_seed(11)
    x = _nhwc(n, c, h, h, dev, g).requires_grad_()
    gy = _nhwc(n, 512, h, h, dev, g)

    def run(fn):
        def f():
            for p in m.parameters():
                p.grad = None
            x.grad = None
            fn(x).backward(gy)
        return f

    arms = dict(fused=run(m), layer_by_layer=run(lambda t: _layer_by_layer(m, t)))
    for f in arms.values():
        f()
    torch.cuda.synchronize()
    med, spread = _alternate(arms, rounds, max(iters // 4, 2))
    return dict(module=f'PyramidPoolModule({c}, {CP}, 512, {BINS})', map=f'{n}x{c}x{h}x{h}', fused_us=round(med['fused'], 1),
                layer_by_layer_us=round(med['layer_by_layer'], 1), spread_us=spread)


def step(n, dev, rounds, iters):
    torch.manual_seed(0)
    m = er.module.PSPNet(dict(head=dict(num_classes=6))).to(dev).train()
    opt = er.opt.FusedSGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, 3, 512, 512, generator=g).to(dev)
    y = torch.randint(0, 6, (n, 512, 512), generator=g).to(dev)

    def f():
        opt.zero_grad(set_to_none=True)
        sum(m(x, y).values()).backward()
        opt.step()

    f()
    torch.cuda.synchronize()
    med, spread = _alternate(dict(step=f), rounds, max(iters // 4, 2))
    return dict(model='PSPNet-R50 (output stride 8, PPMHead defaults, 6 classes)', input=f'{n}x3x512x512',
                step_ms=round(med['step'] / 1e3, 2), tiles_per_s=round(n / (med['step'] / 1e6), 1),
                spread_ms=[round(v / 1e3, 2) for v in spread['step']])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=12)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--no-step', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    lib = _C.load()
    res = dict(tool='bench_ppm', rounds=args.rounds, iters=args.iters, batch=args.batch, kernels=[], modules=[])
    for c, h in SHAPES:
        res['kernels'].append(kernels(lib, args.batch, c, h, dev, args.rounds, args.iters))
        torch.cuda.empty_cache()
    for c, h in SHAPES:
        res['modules'].append(module(args.batch, c, h, dev, args.rounds, args.iters))
        torch.cuda.empty_cache()
    if not args.no_step:
        res['step'] = step(args.batch, dev, args.rounds, args.iters)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
