"""EVK_BN_DUAL at block and model level (module/_resnets.py: _dual_ok / _block_end; hip/norm.py: batch_norm_act_dual): a residual
block with a shortcut convolution runs its last BatchNorm and the shortcut's in passes that take both maps.  Nothing computed
changes, so outputs, gradients, running statistics and the weights after an update are BIT-identical with the switch on
and off — and the counters show which path ran."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


def _blocks():
    from ever_amd.module import _resnets as R
    from ever_amd.module.layers import BatchNorm2d
    return {
        'bottleneck': lambda: R.Bottleneck(64, 64, 1, torch.nn.Sequential(R.conv1x1(64, 256, 1), BatchNorm2d(256))),
        'basic': lambda: R.BasicBlock(64, 128, 2, torch.nn.Sequential(R.conv1x1(64, 128, 2), BatchNorm2d(128))),
    }


def _run_block(cuda, make, state, dual, prepare=None, train=True):
    """one forward + backward of a fresh block under the switch: (everything to compare, counters)"""
    from ever_amd.hip import functional as HF
    block = make().to(cuda)
    block.load_state_dict(state)
    block.train(train)
    if prepare is not None:
        prepare(block)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 64, 32, 32, generator=g).to(cuda).contiguous(memory_format=torch.channels_last).requires_grad_()
    prev = HF.set_bn_dual(dual)
    HF.relu_bits_stats.update({k: 0 for k in HF.relu_bits_stats})
    try:
        y = block(x)
        gy = torch.randn(y.shape, generator=g).to(cuda).contiguous(memory_format=torch.channels_last)
        y.backward(gy)
        torch.cuda.synchronize()
    finally:
        HF.set_bn_dual(prev)
    out = {'y': y.detach().clone(), 'dx': x.grad.clone()}
    out.update({'grad ' + k: p.grad.clone() for k, p in block.named_parameters()})
    out.update({'state ' + k: v.clone() for k, v in block.state_dict().items()})
    return out, dict(HF.relu_bits_stats)


def _state(make):
    torch.manual_seed(5)
    block = make()
    with torch.no_grad():
        for m in block.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
                m.running_mean.normal_(0, 0.3)
                m.running_var.uniform_(0.5, 1.5)
    return copy.deepcopy(block.state_dict())


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, (what, bad[:6])


@pytest.mark.parametrize('kind', ['bottleneck', 'basic'])
def test_block_is_bit_identical_with_the_switch_on_and_off(cuda, kind):
    make = _blocks()[kind]
    state = _state(make)
    off, st_off = _run_block(cuda, make, state, False)
    on, st_on = _run_block(cuda, make, state, True)
    assert st_off['dual'] == 0 and st_off['forward'] == 1 and st_off['lazy'] == 1 and st_off['masked_bn'] == 1, st_off
    assert st_on['dual'] == 1 and st_on['forward'] == 1 and st_on['lazy'] == 1 and st_on['masked_bn'] == 1, st_on
    _assert_same(on, off, kind)
    moved = [k for k in on if k.startswith('state ') and 'running' in k and torch.equal(on[k], state[k[6:]].to(cuda))]
    assert not moved, ('running statistics that did not move', moved)
    nbt = [int(v) for k, v in on.items() if k.endswith('num_batches_tracked')]
    assert nbt and all(v == 1 for v in nbt), nbt


def _sync_shortcut(block):
    from ever_amd.module.sync_bn import SyncBatchNorm
    old = block.downsample[1]
    new = SyncBatchNorm(old.num_features).to(old.weight.device)
    new.load_state_dict(old.state_dict())
    block.downsample[1] = new


def _hook_shortcut(block):
    block.seen = []
    block.downsample.register_forward_hook(lambda m, i, o: block.seen.append(1))
    block.downsample[1].register_forward_hook(lambda m, i, o: block.seen.append(tuple(o.shape)))


@pytest.mark.parametrize('why', ['sync_bn', 'forward_hook', 'eval'])
def test_block_falls_back_where_the_two_map_passes_do_not_apply(cuda, why):
    make = _blocks()['bottleneck']
    state = _state(make)
    prepare = {'sync_bn': _sync_shortcut, 'forward_hook': _hook_shortcut, 'eval': None}[why]
    train = why != 'eval'
    off, _ = _run_block(cuda, make, state, False, prepare, train)
    on, st_on = _run_block(cuda, make, state, True, prepare, train)
    assert st_on['dual'] == 0, (why, st_on)
    _assert_same(on, off, why)


def _train_step(cuda, dual):
    import ever_amd as er
    from ever_amd.hip import functional as HF
    from oracle import portable
    from tests.test_e2e_gpu import _hip_model
    meta = dict(resnet_type='resnet50', in_channels=3, num_classes=1, decoder_channels=256, classifier_kernel=1)
    prev = HF.set_bn_dual(dual)
    HF.relu_bits_stats.update({k: 0 for k in HF.relu_bits_stats})
    try:
        m = _hip_model(meta, cuda).train()
        opt = er.opt.FusedSGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
        x, y = portable.synthetic_batch('bn_dual', 2, 3, 64, 64, 1)
        x, y = torch.from_numpy(x).to(cuda), torch.from_numpy(y).to(cuda)
        losses = m.loss(m.head(m.en(x)), y)
        sum(losses.values()).backward()
        out = {'loss ' + k: v.detach().clone() for k, v in losses.items()}
        out.update({'grad ' + k: p.grad.detach().clone() for k, p in m.named_parameters()})
        opt.step()
        torch.cuda.synchronize()
        out.update({'state ' + k: v.detach().clone() for k, v in m.state_dict().items()})
    finally:
        HF.set_bn_dual(prev)
    return out, dict(HF.relu_bits_stats)


def test_farseg_r50_training_step_is_bit_identical_with_the_switch_on_and_off(cuda):
    """losses, every gradient and the state dict after the SGD update.  (On 64 x 64 tiles the shortcut blocks of the last two
    stages have too few rows for their convolutions to leave statistics records: those keep the layer-by-layer path.)"""
    off, st_off = _train_step(cuda, False)
    on, st_on = _train_step(cuda, True)
    assert st_off['dual'] == 0 and st_on['dual'] >= 2, (st_off, st_on)
    assert st_on['forward'] == st_off['forward'] and st_on['lazy'] == st_off['lazy'], (st_off, st_on)
    assert st_on['masked_bn'] == st_off['masked_bn'] and st_on['materialized'] == st_off['materialized'], (st_off, st_on)
    _assert_same(on, off, 'FarSeg-R50')
