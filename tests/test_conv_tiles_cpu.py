"""The table of tests/conv_tiles_common.py against the planner (csrc/conv_route.hip), asked through evk_conv2d_route on the
host: every forced route the GPU test (tests/test_conv_tiles_gpu.py, tools/check_tiles.py) launches is the instantiation the
table says, the table reaches every instantiation it is there for, and without the forces it would reach almost none of them.
An edit of kForced or of the planner's rules that changes what the GPU test runs fails here, on the build machine.

The routing switches are read once per process: one child per family environment."""
import os
import subprocess
import sys

import pytest

from tests import conv_tiles_common as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(env, code):
    full = {k: v for k, v in os.environ.items() if k not in T.SWITCHES}
    full.update(env)
    code = f'import sys; sys.path.insert(0, {ROOT!r}); from tests import test_conv_tiles_cpu as t; {code}'
    p = subprocess.run([sys.executable, '-c', code], env=full, capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return p.stdout


def names_of(family):
    """runs in a process that has the family's switches in its environment"""
    from ever_amd import _C
    for name in sorted(T.walk(_C.load(), family)):
        print('name', name)


def _names(out):
    return {line[5:] for line in out.splitlines() if line.startswith('name ')}


@pytest.fixture(scope='module')
def reached():
    """family -> the instantiations its forced table reaches (the walk asserts every expectation of the table)"""
    return {family: _names(_child(T.FAMILIES[family][0], f't.names_of({family!r})')) for family in T.FAMILIES}


@pytest.mark.parametrize('family', list(T.FAMILIES))
def test_forced_routes_are_the_table_s(reached, family):
    names = reached[family]
    kernels = {'generic': ('conv_igemm_x3ws_kernel', 'conv_igemm_x3_kernel'), 'halo': ('conv3x3_halo_x3_kernel', 'conv_igemm_x3_kernel')}
    assert names and all(n.startswith(kernels[family]) for n in names), names
    # a refused 128-wide force (Cd <= 64) is in the table as the rule's narrow form, not as a silent pass
    if family == 'halo':
        h2 = next(c for c in T.HALO_CASES if c['name'] == 'h2')
        assert T.expected('halo', h2, 'm128x16', 'f16x2')[0] == 'conv3x3_halo_x3_kernel<64, 8, 2, true, 4>'
        h1 = next(c for c in T.HALO_CASES if c['name'] == 'h1')
        assert T.expected('halo', h1, 'm128x16', 'f16x2', packed=True) == ('conv3x3_halo_x3_kernel<128, 16, 4, true, 8>',
                                                                           ['conv3x3_halo_x3_kernel<128, 16, 4, true, 8>'])
        assert T.expected('halo', h1, 'm128x16', 'bf16x3')[0] == 'conv3x3_halo_x3_kernel<128, 16, 3, false, 4>'


def test_the_table_reaches_every_instantiation_it_is_there_for(reached):
    from ever_amd import _C
    union = set().union(*reached.values()) | T.walk_fp32(_C.load())
    assert T.REQUIRED <= union, sorted(T.REQUIRED - union)
    assert union == T.REQUIRED | T.ALSO_REACHED, sorted(union ^ (T.REQUIRED | T.ALSO_REACHED))


def default_routes():
    """runs in a process without any routing switch"""
    from ever_amd import _C
    lib = _C.load()
    for _env, _var, _forces, cases in T.FAMILIES.values():
        for c in cases:
            for mode, planes in T.ARITH.items():
                fwd, dgrad = T.routed(lib, c, planes)
                print('route', c['name'], mode, 'fwd', fwd)
                for name in dgrad:
                    print('route', c['name'], mode, 'dgrad', name)


def test_without_the_forces_the_cases_stay_on_the_small_tiles():
    """why forcing is needed: under the default switches no case of the two families reaches a 128-row X3 / X3Ws tile, except
    g4's forward (603 tiles of 128 x 128 ... one K step)"""
    out = _child({}, 't.default_routes()')
    rows = [line.split(' ', 4)[1:] for line in out.splitlines() if line.startswith('route ')]
    assert len(rows) == 3 * (sum(1 + c['s'][0] * c['s'][1] for c in T.GENERIC_CASES + T.HALO_CASES))
    large = {(case, direction) for case, _mode, direction, name in rows
             if name.startswith(('conv_igemm_x3_kernel<128', 'conv_igemm_x3ws_kernel<128'))}
    assert large == {('g4', 'fwd')}, large
