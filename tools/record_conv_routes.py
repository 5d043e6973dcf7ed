"""dev tool: which kernel every forward / data-gradient convolution launches, recorded from a kernel trace.

    rocprofv3 --kernel-trace --output-format csv -d TRACE_DIR -- python tools/record_conv_routes.py run CASES.json
    python tools/record_conv_routes.py golden RUN_DIR OUT.json [--commit ID]

`run` (GPU) walks the shape grid below: one launch per (shape, arithmetic, direction, epilogue) on zero-filled buffers, each
preceded by a tiny evk_absmax launch that separates the cases in the trace, and writes the case list.  The routing switches
(EVK_WINO, EVK_X3_HALO, ...) are read once per process: one `run` per setting, into RUN_DIR/cases_<setting>.json and
RUN_DIR/trace_<setting>/ (one of them named `default`).  `golden` (no GPU) cuts the traces at the separators and writes, per
case, the demangled kernel names with template arguments and the grid in workgroups: tests/golden/conv_routes.json, which
tests/test_conv_route_cpu.py holds evk_conv2d_route to.
"""
import csv
import ctypes
import glob
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FIELDS = ('N', 'H', 'W', 'Cin', 'Ho', 'Wo', 'Cout', 'kh', 'kw', 'stride_h', 'stride_w', 'pad_h', 'pad_w', 'dil_h', 'dil_w')
SWITCHES = ('EVK_WINO', 'EVK_X3_HALO', 'EVK_X3_HALO_MIN_WG', 'EVK_C1_DMA', 'EVK_C1_PS2', 'EVK_C1_SP', 'EVK_X3_WS')


def conv(n, h, w, cin, cout, k=3, s=1, d=1, pad=None):
    p = d * (k - 1) // 2 if pad is None else pad
    ho = (h + 2 * p - d * (k - 1) - 1) // s + 1
    wo = (w + 2 * p - d * (k - 1) - 1) // s + 1
    return (n, h, w, cin, ho, wo, cout, k, k, s, s, p, p, d, d)


def shape_grid():
    """every distinct convolution of the benchmark configurations at their real batch sizes, batch 2 at the golden
    fixtures' sizes, and the geometries the routing rules special-case"""
    g = []
    for n, s4 in ((16, 128), (2, 64), (2, 32), (2, 16)):   # s4: side of the stride-4 map (512^2 / 256^2 / 128^2 / 64^2 tiles)
        s8, s16, s32 = s4 // 2, s4 // 4, s4 // 8
        # ResNet-50 bottlenecks
        g += [conv(n, s4, s4, 64, 64, 1), conv(n, s4, s4, 64, 64, 3), conv(n, s4, s4, 64, 256, 1), conv(n, s4, s4, 256, 64, 1),
              conv(n, s4, s4, 256, 128, 1), conv(n, s4, s4, 128, 128, 3, 2), conv(n, s4, s4, 256, 512, 1, 2),
              conv(n, s8, s8, 128, 512, 1), conv(n, s8, s8, 512, 128, 1), conv(n, s8, s8, 128, 128, 3),
              conv(n, s8, s8, 512, 256, 1), conv(n, s8, s8, 256, 256, 3, 2), conv(n, s8, s8, 512, 1024, 1, 2),
              conv(n, s16, s16, 256, 1024, 1), conv(n, s16, s16, 1024, 256, 1), conv(n, s16, s16, 256, 256, 3),
              conv(n, s16, s16, 1024, 512, 1), conv(n, s16, s16, 512, 512, 3, 2), conv(n, s16, s16, 1024, 2048, 1, 2),
              conv(n, s32, s32, 512, 2048, 1), conv(n, s32, s32, 2048, 512, 1), conv(n, s32, s32, 512, 512, 3)]
        # ResNet-18 basic blocks
        g += [conv(n, s4, s4, 64, 128, 3, 2), conv(n, s4, s4, 64, 128, 1, 2), conv(n, s8, s8, 128, 256, 3, 2),
              conv(n, s8, s8, 128, 256, 1, 2), conv(n, s16, s16, 256, 512, 3, 2), conv(n, s16, s16, 256, 512, 1, 2)]
        # FPN laterals / outputs, decoder, FS-Relation, ChangeMixin, classifier
        for side, c50, c18 in ((s4, 256, 64), (s8, 512, 128), (s16, 1024, 256), (s32, 2048, 512)):
            g += [conv(n, side, side, c50, 256, 1), conv(n, side, side, c18, 256, 1), conv(n, side, side, 256, 256, 3),
                  conv(n, side, side, 256, 128, 3), conv(n, side, side, 128, 128, 3), conv(n, side, side, 256, 256, 1)]
        g += [conv(n, 1, 1, 2048, 256, 1), conv(n, 1, 1, 512, 256, 1), conv(n, s4, s4, 128, 16, 1), conv(n, s4, s4, 256, 16, 3),
              conv(n, s4, s4, 16, 16, 3)]
    # DeepLabv3+ / ASPP (output stride 16)
    for n, s in ((16, 32), (2, 16)):
        g += [conv(n, s, s, 2048, 256, 3, 1, d) for d in (6, 12, 18)]
        g += [conv(n, s, s, 2048, 256, 1), conv(n, s, s, 1280, 256, 1), conv(n, 4 * s, 4 * s, 256, 48, 1),
              conv(n, 4 * s, 4 * s, 304, 256, 3), conv(n, 4 * s, 4 * s, 256, 256, 3, 1, 2)]
    # FreeNet (hyperspectral scenes: Cin = 200 / 96), a 616 x 344 scene and its stride-2 / stride-4 maps
    g += [conv(1, 616, 344, 200, 96, 3), conv(1, 616, 344, 96, 96, 3), conv(1, 616, 344, 96, 128, 3, 2), conv(1, 308, 172, 128, 128, 3),
          conv(1, 308, 172, 128, 192, 3, 2), conv(1, 154, 86, 192, 192, 3), conv(1, 154, 86, 256, 256, 3), conv(1, 616, 344, 96, 128, 1),
          conv(1, 616, 344, 128, 200, 3), conv(1, 616, 344, 200, 128, 1)]
    # the stride-4 map of a 416-wide tile, H % 16 in 1..8, output widths 64 / 96 / 200
    g += [conv(16, 104, 104, 256, 256, 3), conv(16, 104, 104, 64, 64, 3), conv(16, 104, 104, 256, 128, 3)]
    g += [conv(8, h, 128, 256, 256, 3) for h in (129, 130, 136, 137, 72)]
    g += [conv(16, 128, 128, 256, c, 3) for c in (64, 96, 200)] + [conv(16, 128, 128, 256, c, 1) for c in (96, 200)]
    out = []
    for d in g:
        if d not in out:
            out.append(d)
    return out


def cases_of(d):
    """the launches of one shape: (arithmetic, direction, packed operand, statistics epilogue, accumulate operand)"""
    cin, cout = d[3], d[6]
    cs = []
    if cin % 8 == 0:
        for packed in (0, 1):
            cs += [('f16x2', 'fwd', packed, st, acc) for st in (0, 1) for acc in (0, 1)]
        cs += [('bf16x3', 'fwd', 0, 0, 0), ('bf16x3', 'fwd', 0, 1, 0), ('bf16x3', 'fwd', 0, 0, 1)]
        cs += [('bf16', 'fwd', 0, 0, 0), ('bf16', 'fwd', 0, 1, 0)]
    cs += [('fp32', 'fwd', 0, 0, 0), ('fp32', 'fwd', 0, 0, 1)]
    if cout % 8 == 0:
        for packed in (0, 1):
            cs += [('f16x2', 'dgrad', packed, 0, acc) for acc in (0, 1)]
        cs += [(ar, 'dgrad', 0, 0, acc) for ar in ('bf16x3', 'bf16') for acc in (0, 1)]
    if cout % 4 == 0:
        cs += [('fp32', 'dgrad', 0, 0, acc) for acc in (0, 1)]
    return cs


def run(cases_path):
    import torch
    from ever_amd import _C
    lib = _C.load()
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    nw = int(lib.evk_absmax_words())
    one = torch.full((nw,), 0x3f800000, dtype=torch.int32, device=dev)   # operand scales: max|x| = max|w| = 1
    sep_src = torch.zeros(64, device=dev)
    sep_bits = torch.zeros(nw, dtype=torch.int32, device=dev)
    aws = torch.zeros(int(lib.evk_absmax_workspace_bytes()), dtype=torch.uint8, device=dev)
    rows = []
    npart = ctypes.c_int32(0)
    for d in shape_grid():
        desc = _C.ConvDesc(*d)
        dp = ctypes.byref(desc)
        n, h, w, cin, ho, wo, cout, kh, kw = d[:9]
        xe, ye = n * h * w * cin, n * ho * wo * cout
        x, y = torch.zeros(xe, device=dev), torch.zeros(ye, device=dev)
        extra = torch.zeros(max(xe, ye), device=dev)
        wbytes = max(int(lib.evk_conv2d_split_weight_bytes(dp, 0)), int(lib.evk_conv2d_split_weight_bytes(dp, 1)),
                     4 * cout * kh * kw * cin)
        wbuf = torch.zeros(wbytes, dtype=torch.uint8, device=dev)
        cap = int(lib.evk_conv2d_stats_max_parts(dp))
        parts = torch.zeros(cap * 3 * cout, device=dev)
        X, Y, E, W, S = x.data_ptr(), y.data_ptr(), extra.data_ptr(), wbuf.data_ptr(), one.data_ptr()
        for ar, direction, packed, stats, acc in cases_of(d):
            _C.call('evk_absmax', sep_src.data_ptr(), 64, sep_bits.data_ptr(), aws.data_ptr(), st)   # the separator
            pb, pc = (parts.data_ptr(), cap) if stats else (None, 0)
            res = E if acc else None
            if direction == 'fwd':
                if ar == 'f16x2':
                    _C.call('evk_conv2d_fwd_f16x2', dp, X, S, W, S, None, res, Y, 2 if packed else 0, pb, pc,
                            ctypes.byref(npart), None, st)
                elif ar == 'bf16x3':
                    if stats:
                        _C.call('evk_conv2d_fwd_x3_stats', dp, X, W, None, Y, 0, pb, pc, ctypes.byref(npart), st)
                    elif acc:
                        _C.call('evk_conv2d_fwd_x3_res', dp, X, W, None, res, Y, 0, st)
                    else:
                        _C.call('evk_conv2d_fwd_x3', dp, X, W, None, Y, 0, st)
                elif ar == 'bf16':
                    _C.call('evk_conv2d_fwd_bf16', dp, X, W, None, Y, 0, pb, pc, ctypes.byref(npart), st)
                elif acc:
                    _C.call('evk_conv2d_fwd_res', dp, X, W, None, res, Y, 0, st)
                else:
                    _C.call('evk_conv2d_fwd', dp, X, W, None, Y, 0, st)
            else:
                if ar == 'f16x2':
                    _C.call('evk_conv2d_dgrad_f16x2_ex', dp, Y, S, W, S, res, X, None, 4 if packed else 0, st)
                elif ar == 'bf16x3':
                    _C.call('evk_conv2d_dgrad_x3', dp, Y, W, res, X, st)
                elif ar == 'bf16':
                    _C.call('evk_conv2d_dgrad_bf16', dp, Y, W, res, X, st)
                else:
                    _C.call('evk_conv2d_dgrad', dp, Y, W, res, X, st)
            rows.append([list(d), ar, direction, packed, stats, acc])
        torch.cuda.synchronize()
        del x, y, extra, wbuf, parts
    _C.call('evk_absmax', sep_src.data_ptr(), 64, sep_bits.data_ptr(), aws.data_ptr(), st)
    torch.cuda.synchronize()
    prop = torch.cuda.get_device_properties(0)
    with open(cases_path, 'w') as f:
        json.dump(dict(device=prop.name or prop.gcnArchName, compute_units=prop.multi_processor_count,
                       switches={k: os.environ[k] for k in SWITCHES if k in os.environ}, cases=rows), f)
    print(f'{len(rows)} cases on {prop.name} ({prop.multi_processor_count} CUs)')


def short_name(name):
    """'void evk::conv_igemm_x3_kernel<128, 64, 2, 2, 1, 2>(evk::IGemmArgs)' -> 'conv_igemm_x3_kernel<128, 64, 2, 2, 1, 2>'"""
    m = re.match(r'(?:void )?(?:evk::)?([A-Za-z0-9_]+(?:<[^()]*>)?)', name)
    return m.group(1) if m else name


def parse(cases_path, trace_dir):
    """(meta, rows): rows[i] = the case with its launches [[kernel name, workgroups], ...] appended"""
    with open(cases_path) as f:
        meta = json.load(f)
    files = sorted(glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True), key=os.path.getmtime)
    assert files, trace_dir
    with open(files[-1], newline='') as f:
        disp = sorted(csv.DictReader(f), key=lambda r: int(r['Dispatch_Id']))
    groups, cur, prev_sep = [], None, False
    for r in disp:
        name = r['Kernel_Name']
        if 'absmax' in name:
            if not prev_sep:
                cur = []
                groups.append(cur)
            prev_sep = True
            continue
        prev_sep = False
        if cur is not None and 'evk::conv' in name:
            gx, wx = int(r['Grid_Size_X']), int(r['Workgroup_Size_X'])
            assert gx % wx == 0 and int(r['Grid_Size_Y']) == 1 and int(r['Grid_Size_Z']) == 1, r
            cur.append([short_name(name), gx // wx])
    assert groups and not groups[-1], 'the trace must end on a separator'
    groups.pop()
    assert len(groups) == len(meta['cases']) and all(groups), (len(groups), len(meta['cases']))
    return meta, [c + [k] for c, k in zip(meta['cases'], groups)]


def golden(run_dir, out_path, commit):
    """RUN_DIR/cases_<setting>.json + RUN_DIR/trace_<setting>/ of every switch setting -> one file, one line per shape:
    [desc, case set, launches of each case under the default switches, {setting: {case position: launches that differ}}];
    a launch is [index into "kernels", workgroups]"""
    names = sorted(f[len('cases_'):-len('.json')] for f in os.listdir(run_dir) if f.startswith('cases_'))
    assert 'default' in names
    names.remove('default')
    runs = {s: parse(os.path.join(run_dir, f'cases_{s}.json'), os.path.join(run_dir, f'trace_{s}')) for s in ['default'] + names}
    meta, base = runs['default']
    kernels = sorted({k[0] for _, rows in runs.values() for r in rows for k in r[6]})
    enc = lambda launches: [[kernels.index(n), g] for n, g in launches]
    cases, case_sets, shapes = [], [], {}
    for i, r in enumerate(base):
        c = r[1:6]
        if c not in cases:
            cases.append(c)
        shapes.setdefault(tuple(r[0]), []).append(i)
    lines = []
    for d, idx in shapes.items():
        cs = [cases.index(base[i][1:6]) for i in idx]
        if cs not in case_sets:
            case_sets.append(cs)
        diff = {}
        for s in names:
            rows = runs[s][1]
            assert all(rows[i][:6] == base[i][:6] for i in idx)
            dd = {str(p): enc(rows[i][6]) for p, i in enumerate(idx) if rows[i][6] != base[i][6]}
            if dd:
                diff[s] = dd
        lines.append(json.dumps([list(d), case_sets.index(cs), [enc(base[i][6]) for i in idx], diff], separators=(',', ':')))
    head = dict(commit=commit, device=meta['device'] or 'gfx950', compute_units=meta['compute_units'],
                settings={s: runs[s][0]['switches'] for s in ['default'] + names}, kernels=kernels,
                cases=cases, case_sets=case_sets)
    with open(out_path, 'w') as f:
        f.write('{' + ',\n'.join(f'{json.dumps(k)}: {json.dumps(v)}' for k, v in head.items()))
        f.write(',\n"shapes": [\n' + ',\n'.join(lines) + '\n]}\n')
    print(f'{out_path}: {len(lines)} shapes, {len(base)} cases, {len(names) + 1} settings')


if __name__ == '__main__':
    if sys.argv[1] == 'run':
        run(sys.argv[2])
    else:
        golden(sys.argv[2], sys.argv[3], sys.argv[sys.argv.index('--commit') + 1] if '--commit' in sys.argv else None)
