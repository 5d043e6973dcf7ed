"""Every forward / data-gradient tile form at ragged shapes against float64 (csrc/conv_igemm_x3ws.hip, conv_igemm_x3.hip,
conv3x3_halo_x3.hip, conv_igemm_f32.hip; reference call sites: the convolutions of ever/module/_resnets.py, fpn.py, farseg.py).

The planner takes the large forms — the persistent wave-specialised kernel, 128-row single-role tiles, 128-wide halo tiles,
16-row patches, eight matrix waves, the fp32 128 x 128 / 128 x 64 / 256 x 64 tiles — only from 256 or 512 workgroups on, so the
other fp64 comparisons of this suite reach the smallest tile of each family and the large ones run at tidy production sizes
only.  Here they are forced (EVK_TUNE + EVK_X3_FORCE / EVK_X3_HALO_FORCE, re-read on every launch) onto the table of
tests/conv_tiles_common.py: a last row tile holding 2 of 128 rows, a last column tile 8 wide under a 256-wide tile, a K tail
inside the 32-wide step, persistent workgroups that walk 2 or 3 tiles of one K step each, a 16-row patch hanging over the map by
12 rows, 4.5 channel chunks under eight matrix waves.  tools/check_tiles.py asserts the route of every launch first (a force
that fell back fails) and compares y and dx with float64 in f16x2, bf16x3 and bf16, then packed operands, the statistics and
the accumulate epilogues through the C-ABI.  tests/test_conv_tiles_cpu.py pins the table to the planner without a GPU."""
import os
import re
import subprocess
import sys

import pytest

from tests import conv_tiles_common as T
from tests.test_conv_geometry_gpu import _run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('family', list(T.FAMILIES))
def test_forced_tile_forms_match_fp64(cuda, family):
    env = {k: v for k, v in os.environ.items() if k not in T.SWITCHES}
    env.update(T.FAMILIES[family][0])
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'check_tiles.py'), family], env=env, capture_output=True,
                         text=True, timeout=300)
    tail = out.stdout[out.stdout.rfind('worst e / bound'):] if 'worst e / bound' in out.stdout else out.stdout[-3000:]
    print(tail)
    assert out.returncode == 0 and 'check_tiles ok' in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    # the child's table lists every instantiation the family is there for, in both directions
    listed = set(re.findall(r'^  (conv[^>]*>) +(fwd|dgrad) ', tail, re.M))
    family_names = {n for n in T.REQUIRED if n.startswith('conv3x3_halo' if family == 'halo' else 'conv_igemm_x3')}
    assert {(n, d) for n in family_names for d in ('fwd', 'dgrad')} <= listed, sorted(family_names - {n for n, _ in listed})


@pytest.mark.parametrize('case,fwd,dgrad', T.FP32_CASES, ids=[c[0]['name'] for c in T.FP32_CASES])
def test_fp32_tiles_match_fp64(cuda, case, fwd, dgrad):
    """route_fp32 is a pure rule: in process, the route asserted before the launch; y, dx (and dw, db) within the bounds of
    tests/test_conv_geometry_gpu.py"""
    from ever_amd import _C
    assert T.routed(_C.load(), case, 0) == (fwd, [dgrad])
    _run(cuda, case, 'f32')
