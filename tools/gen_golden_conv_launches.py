"""TEST INFRASTRUCTURE ONLY — writes tests/golden/conv_launches.json: what the convolution host wrappers launch for every
case of tests/conv_launch_common.py, recorded on an MI355X from the tree this file is run in.

The fixture pins the wrappers' dispatch ACROSS commits, so it is recorded from the commit a change starts from, not from the
change: in a worktree of that commit (git worktree add -f <dir> <commit>, its library built or copied in) with this file,
tests/conv_launch_common.py and tests/test_conv_launches_gpu.py copied into it,

    cd <dir> && python tools/gen_golden_conv_launches.py --commit <commit> [--out FILE]

Writes data only: per case the list of [entry name, argument, ...] rows and the counter deltas, and the commit named."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import conv_launch_common as lc  # noqa: E402


def main():
    import torch
    p = argparse.ArgumentParser()
    p.add_argument('--commit', required=True, help='the commit of the tree this runs in (recorded in the fixture)')
    p.add_argument('--out', default=lc.GOLDEN)
    args = p.parse_args()
    dev = torch.device('cuda:0')
    cases = {}
    for name in lc.CASES:
        try:
            cases[name] = lc.record(name, dev)
        except (RuntimeError, ValueError, AssertionError) as e:        # (reported below with every other case's result)
            cases[name] = {'calls': [], 'error': repr(e)}
            print(f'{name}: {e!r}')
    # a record must not depend on what ran before it: every case once more, after all the others
    bad = [f'{name}: a second recording differs from the first' for name in lc.CASES
           if 'error' not in cases[name] and lc.record(name, dev) != cases[name]]
    bad += [f'{name}: launched nothing' for name, rec in cases.items() if not rec['calls']]
    seen = {c[0] for rec in cases.values() for c in rec['calls']}
    if not seen >= lc.REQUIRED_ENTRIES:
        bad.append(f'never launched: {sorted(lc.REQUIRED_ENTRIES - seen)}')
    streams = {c[-1] for rec in cases.values() for c in rec['calls'] if c[0] in lc.WGRAD_ENTRIES}
    if streams != {'main', 'side'}:
        bad.append(f'weight gradients ran on {sorted(streams)} only')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('{"recorded_from": %s, "cases": {\n' % json.dumps(args.commit))
        f.write(',\n'.join(' %s: %s' % (json.dumps(k), json.dumps(v, separators=(',', ':'))) for k, v in cases.items()))
        f.write('\n}}\n')
    ncalls = sum(len(rec['calls']) for rec in cases.values())
    print(f'wrote {args.out}: {len(cases)} cases, {ncalls} calls, {len(seen)} entry points, {os.path.getsize(args.out)} bytes')
    for k, v in cases.items():
        print(f"  {k:40s} {' '.join(c[0][4:] for c in v['calls'])}")
    if bad:
        raise SystemExit('NOT a fixture to commit: ' + '; '.join(bad))


if __name__ == '__main__':
    main()
