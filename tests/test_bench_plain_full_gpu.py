"""bench.py on the GPU at a tiny batch: a plain run times exactly --steps steps and carries none of the --full fields;
--dump-outputs writes the last step's losses and model state; --full (without its two child processes) adds the roofline
objects and host_unblocked_ms_per_step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')
FULL_ONLY = ('host_unblocked_ms_per_step', 'roofline', 'roofline_wgrad', 'board_power', 'hip_graph_replay', 'cpu_baseline')


def _line(args):
    out = subprocess.run([sys.executable, BENCH, '--gpus', '1', '--batch', '2', '--warmup', '1'] + args, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith('{"metric"')][-1])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(cuda, tmp_path):
    d = _line(['--steps', '3', '--dump-outputs', str(tmp_path / 'dump')])
    assert d['steps'] == 3 and d['ms_per_step'] > 0 and d['value'] > 0
    for k in ('metric', 'unit', 'higher_is_better', 'dtype'):
        assert k in d
    assert not [k for k in FULL_ONLY if k in d]
    names = sorted(os.listdir(tmp_path / 'dump'))
    assert names == ['bce_loss.npy', 'dice_loss.npy', 'model_state.npy'], names
    for n in names:
        a = np.load(tmp_path / 'dump' / n)
        assert a.dtype == np.float32 and np.isfinite(a).all()
    assert np.load(tmp_path / 'dump' / 'model_state.npy').size == 1 << 22


@pytest.mark.gpu
def test_full_run_adds_the_rooflines_and_the_host_probe(cuda):
    d = _line(['--steps', '2', '--full', '--no-cpu-baseline', '--no-graph-line'])
    assert d['steps'] == 2 and d['host_unblocked_ms_per_step'] > 0
    assert d['roofline']['frac'] > 0 and d['roofline_wgrad']['frac'] > 0 and 'library_fp16_gemm' in d['roofline']
