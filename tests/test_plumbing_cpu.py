"""CPU plumbing (BASELINE config 1): ever_amd's Launcher / Trainer / data-parallel trainer drive a
model end to end without a GPU, and reproduce the REFERENCE Launcher's run step for step."""
import json
import os
import sys

import pytest
import torch

import ever_amd as er
from tests import plumbing_common as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')


def _spy(launcher, records):
    orig = launcher._logger.train_log

    def wrapped(**kw):
        records.append(dict(step=int(kw['step']), lr=float(kw['lr']), **{k: float(v) for k, v in kw['loss_dict'].items()}))
        return orig(**kw)

    launcher._logger.train_log = wrapped


def test_launcher_reproduces_the_reference_launcher_run(tmp_path):
    """tests/golden/launcher_r18.json was recorded from the reference's own Launcher (gen_golden.py):
    per-step losses, the lagging lr sequence, checkpoint files + index, final weights."""
    with open(os.path.join(GOLD, 'launcher_r18.json')) as f:
        gold = json.load(f)
    torch.manual_seed(0)
    model = pc.OracleFarSeg(dict())
    loader = torch.utils.data.DataLoader(pc.ToyTiles(), batch_size=2, shuffle=False)
    sched = er.builder.make_learningrate(dict(type='poly', params=dict(base_lr=0.01, power=0.9, max_iters=3)))
    opt = er.builder.make_optimizer(er.AttrDict.from_dict(dict(type='sgd', params=dict(momentum=0.9, weight_decay=1e-4, lr=sched.base_lr))),
                                    params=model.custom_param_groups())
    tl = er.Launcher(str(tmp_path), model, opt, sched, mixed_precision='fp32')
    records = []
    _spy(tl, records)
    last = tl.train_by_config(loader, config=er.AttrDict.from_dict(dict(num_iters=3, save_ckpt_interval_epoch=1000)))
    assert [r['step'] for r in records] == [1, 2, 3]
    for got, ref in zip(records, gold['records']):
        assert got['lr'] == pytest.approx(ref['lr'], rel=1e-12)        # lr(k-1) logged after step k (one-step lag)
        for k in ('bce_loss', 'dice_loss', 'total_loss'):
            assert got[k] == pytest.approx(ref[k], rel=2e-5), (got, ref)
    assert last['bce_loss'] == pytest.approx(gold['records'][-1]['bce_loss'], rel=2e-5)
    files = sorted(f for f in os.listdir(tmp_path) if not f.endswith('.log'))
    assert files == gold['files']                                       # checkpoint-3.pth + checkpoint_info.json
    with open(tmp_path / 'checkpoint_info.json') as f:
        assert json.load(f) == gold['index']
    ck = torch.load(tmp_path / 'checkpoint-3.pth', weights_only=False)
    assert list(ck.keys()) == ['model', 'global_step', 'opt'] and ck['global_step'] == 3
    assert not any(k.startswith('module.') for k in ck['model'])
    for k, (s, nrm) in gold['final_state'].items():
        assert float(ck['model'][k].double().norm()) == pytest.approx(nrm, rel=1e-4, abs=1e-6), k
    # resume: a new launcher on the same dir picks up step 3 and the optimizer state
    model2 = pc.OracleFarSeg(dict())
    opt2 = er.builder.make_optimizer(er.AttrDict.from_dict(dict(type='sgd', params=dict(momentum=0.9, lr=0.01))), params=model2.parameters())
    tl2 = er.Launcher(str(tmp_path), model2, opt2, sched)
    tl2.init()
    assert tl2.global_step == 3
    assert torch.equal(model2.state_dict()['en.resnet.conv1.weight'], ck['model']['en.resnet.conv1.weight'])


def test_trainer_cli_runs_config1_on_cpu(tmp_path):
    """`ever.trainer` entry with a python config file + command-line overrides (R18, 4-band 256x256, batch 2)."""
    cfg = tmp_path / 'farseg_r18.py'
    cfg.write_text(pc.CONFIG_TEMPLATE.format(n=2, hw=256, iters=2, dist=False))
    model_dir = tmp_path / 'run'
    trainer, args = er.trainer.get_trainer('base', return_args=True, argv=[
        '--config_path', str(cfg), '--model_dir', str(model_dir), 'train.num_iters', '2'])
    assert args.mixed_precision == 'fp32' and trainer.config.train.num_iters == 2
    out = trainer.run()
    tl = out['launcher']
    assert tl.global_step == 2 and os.path.exists(model_dir / 'config.pkl') and os.path.exists(model_dir / 'checkpoint-2.pth')
    assert er.config.import_config(str(model_dir / 'config.pkl')).model.type == 'OracleFarSeg'


def test_forward_times_accumulates_micro_batches(tmp_path):
    model = pc.OracleFarSeg(dict())
    loader = torch.utils.data.DataLoader(pc.ToyTiles(), batch_size=1, shuffle=False)
    sched = er.builder.make_learningrate(dict(type='constant', params=dict(base_lr=0.0)))
    opt = er.builder.make_optimizer(er.AttrDict.from_dict(dict(type='torch_sgd', params=dict(lr=0.0))), params=model.parameters())
    tl = er.Launcher(str(tmp_path), model, opt, sched)
    seen = []
    orig = model.backward

    def spy(loss_dict, amp, scaler, **kw):
        seen.append({k: float(v) for k, v in loss_dict.items()})
        return orig(loss_dict, amp, scaler, **kw)

    model.backward = spy
    tl.train_iters(loader, num_iters=1, forward_times=2, save_ckpt_interval_epoch=1000)
    assert len(seen) == 2  # two micro-batches, each loss pre-divided by forward_times
    model.eval()
    with torch.no_grad():
        pass
    assert all(0 < v < 1 for d in seen for v in d.values())


def _ddp_worker(rank, world, port, tmp, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    sys.path.insert(0, ROOT)
    import ever_amd as er2
    from tests import plumbing_common as pc2
    torch.set_num_threads(2)
    cfg = os.path.join(tmp, 'cfg.py')
    if rank == 0:
        with open(cfg, 'w') as f:
            f.write(pc2.CONFIG_TEMPLATE.format(n=4, hw=64, iters=2, dist=True))
    import time
    while not os.path.exists(cfg):
        time.sleep(0.05)
    time.sleep(0.2)
    trainer = er2.trainer.get_trainer('th_ddp', argv=['--config_path', cfg, '--model_dir', os.path.join(tmp, 'run')])
    records = []
    out = None

    def hook(tl):
        if tl.is_main_process:
            _spy(tl, records)

    out = trainer.run(after_construct_launcher_callbacks=[hook])
    tl = out['launcher']
    sd = tl.unwrapped_model.state_dict()
    digest = float(sum(v.double().sum() for k, v in sd.items() if v.is_floating_point() and 'running' not in k))
    sampler = None
    q.put((rank, digest, records, tl.global_step))
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


def test_data_parallel_trainer_two_ranks_gloo(tmp_path):
    """world_size 2 on CPU/gloo: the th_ddp trainer shards the minibatch stream, all-reduces gradients,
    keeps replicas bit-identical and reduces the logged losses onto rank 0."""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=600) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (r0, d0, rec0, s0), (r1, d1, rec1, s1) = res
    assert s0 == s1 == 2
    assert d0 == d1, 'replicas diverged: gradient all-reduce / broadcast broken'
    assert len(rec0) == 2 and len(rec1) == 0  # only the master logs
    assert all(0 < r['bce_loss'] < 2 for r in rec0)


def test_ptr_array_and_i32_array_hold_what_the_c_abi_reads():
    """hip/_base.py: the host arrays behind a `const float* const*` / `const int32_t*` argument — a tensor's data pointer,
    a null pointer for None, the ints, with the lengths given"""
    from ever_amd.hip._base import i32_array, ptr_array
    t = torch.zeros((4,))
    p = ptr_array([t, None])
    assert len(p) == 2 and p[0] == t.data_ptr() and not p[1]
    v = i32_array((0, 1))
    assert len(v) == 2 and list(v) == [0, 1]
