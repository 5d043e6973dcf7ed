"""`bench.py --dump-outputs DIR` (the last timed step's outputs as float .npy files, a fixed sample of a large model state)
and the plain / `--full` split of its options.  No GPU: dump_outputs is called on a small CPU module."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _model():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(64, 32), torch.nn.BatchNorm1d(32))
    m(torch.randn(8, 64))   # moves the running statistics
    return m


def _state(m):
    return np.concatenate([t.detach().reshape(-1).float().numpy() for t in m.state_dict().values() if t.is_floating_point()])


def test_dump_outputs_writes_the_losses_and_the_whole_small_state(tmp_path):
    m = _model()
    out = {'bce_loss': torch.tensor(0.25, requires_grad=True) * 2, 'dice_loss': torch.tensor(0.5), 'count': torch.tensor(3)}
    bench.dump_outputs(str(tmp_path / 'd'), out, m)
    assert sorted(os.listdir(tmp_path / 'd')) == ['bce_loss.npy', 'count.npy', 'dice_loss.npy', 'model_state.npy']
    assert np.load(tmp_path / 'd' / 'bce_loss.npy').dtype == np.float32 and float(np.load(tmp_path / 'd' / 'bce_loss.npy')) == 0.5
    assert np.load(tmp_path / 'd' / 'count.npy').dtype == np.float64 and float(np.load(tmp_path / 'd' / 'count.npy')) == 3.0
    state = np.load(tmp_path / 'd' / 'model_state.npy')
    assert state.dtype == np.float32
    np.testing.assert_array_equal(state, _state(m))   # 64*32 + 32 + 4*32 values < DUMP_SAMPLE: all of them, in order


def test_dump_outputs_samples_a_large_state_at_fixed_positions(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_SAMPLE', 500)
    m = _model()
    out = {'bce_loss': torch.tensor(1.0)}
    bench.dump_outputs(str(tmp_path / 'a'), out, m)
    bench.dump_outputs(str(tmp_path / 'b'), out, m)
    a, b = np.load(tmp_path / 'a' / 'model_state.npy'), np.load(tmp_path / 'b' / 'model_state.npy')
    assert a.shape == (500,) and a.dtype == np.float32
    np.testing.assert_array_equal(a, b)
    full = _state(m)
    idx = torch.randperm(full.size, generator=torch.Generator().manual_seed(0))[:500].sort().values.numpy()
    np.testing.assert_array_equal(a, full[idx])


def test_plain_run_turns_every_extra_off_and_full_keeps_the_switches(monkeypatch):
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--steps', '7'])
    args = bench.parse()
    assert args.steps == 7 and not args.full and args.dump_outputs is None
    # no event timer inside the timed steps, no hip_graph_replay child (nor board_power), no CPU baseline
    assert args.no_kernel_timer and args.no_graph_line and args.no_cpu_baseline
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--dump-outputs', 'x'])
    args = bench.parse()
    assert args.full and args.dump_outputs == 'x'
    assert not (args.no_kernel_timer or args.no_graph_line or args.no_cpu_baseline)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--no-cpu-baseline'])
    args = bench.parse()
    assert args.no_cpu_baseline and not (args.no_kernel_timer or args.no_graph_line)
