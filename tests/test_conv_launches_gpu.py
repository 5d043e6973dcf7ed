"""What the convolution host wrappers launch, case by case, against a recording of the same cases from the commit named in
tests/golden/conv_launches.json (tools/gen_golden_conv_launches.py): entry names, descriptors, flag words, null / non-null
operands and the stream of every C-ABI call, plus the operand-scale, ReLU-bit and side-stream counters.  The fp64 tests cannot
see a wrapper that stops taking a packed, planar or side-stream path — the numbers stay right, only slower — this one does.
The cases and the recorder are in tests/conv_launch_common.py."""
import json

import pytest

from tests import conv_launch_common as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    return lc.load_golden()['cases']


@pytest.mark.parametrize('name', list(lc.CASES))
def test_launch_sequence_is_the_recorded_one(cuda, golden, name):
    got = json.loads(json.dumps(lc.record(name, cuda)))
    want = golden[name]
    for i, (a, b) in enumerate(zip(got['calls'], want['calls'])):
        assert a == b, f'{name}: call {i} is {a}, recorded {b}'
    assert [c[0] for c in got['calls']] == [c[0] for c in want['calls']], name
    assert got == want, name


def test_the_packed_cases_carry_the_packed_flags(golden):
    """read from the fixture (no launch).  EVK_CONV_X_PACKED = 2, EVK_CONV_DY_PACKED = 4, EVK_BN_PACK_Y = 4, a packed dx of the
    BatchNorm backward = 2: the chain's first BatchNorm writes packed, the second convolution reads x packed, both read dy packed
    (fp32 everywhere with the switch off); an operand that arrives packed gets no pack pass in front of the weight gradient"""
    def flags(case, entry):
        return [lc.flag_word(c) for c in golden[case]['calls'] if c[0] == entry]
    assert [f & 2 for f in flags('chain_packed', 'evk_conv2d_fwd_f16x2')] == [0, 2]
    assert [f & 4 for f in flags('chain_packed', 'evk_bn_fwd_train_parts')] == [4, 0]
    assert [f & 2 for f in flags('chain_packed', 'evk_bn_bwd_bits')] == [2, 2]
    assert [f & 4 for f in flags('chain_packed', 'evk_conv2d_dgrad_f16x2_ex')] == [4, 4]
    assert [f & 6 for f in flags('chain_packed', 'evk_conv2d_wgrad_f16x2_ex')] == [6, 4]        # (backward: second layer first)
    assert golden['chain_packed']['absmax_stats']['packed'] == 3
    for entry in ('evk_conv2d_fwd_f16x2', 'evk_bn_fwd_train_parts', 'evk_bn_bwd_bits', 'evk_conv2d_dgrad_f16x2_ex'):
        assert not any(f & 6 for f in flags('chain_fp32_operands', entry)), entry
    assert [f & 6 for f in flags('chain_packed_x_fp32_dy', 'evk_conv2d_wgrad_f16x2_ex')] == [2, 4]
    names = lambda case: [c[0] for c in golden[case]['calls']]   # noqa: E731
    assert 'evk_pack_f16x2' not in names('chain_packed')
    # pack pays everywhere: x fp32 / dy fp32 -> two passes; second layer of the chain without its BatchNorm: x packed, dy from
    # the loss -> one pass (dy), then the first layer: dy packed -> one pass (x); both packed -> the first layer's x alone
    assert names('wgrad_pack_both').count('evk_pack_f16x2') == 2
    assert names('wgrad_pack_x_already_packed').count('evk_pack_f16x2') == 2
    assert [f & 6 for f in flags('wgrad_pack_x_already_packed', 'evk_conv2d_wgrad_f16x2_ex')] == [6, 6]
    assert names('wgrad_pack_both_already_packed').count('evk_pack_f16x2') == 1
    assert names('wgrad_pack_refused_by_bias_gradient').count('evk_pack_f16x2') == 0
    assert [f & 6 for f in flags('wgrad_batched_chain_packed', 'evk_conv2d_wgrad_f16x2_ex')] == [6, 4]


def test_the_cases_reach_every_branch_they_are_there_for(golden):
    """read from the fixture (no launch): a switch that no longer forces its branch would empty a case silently"""
    assert set(golden) == set(lc.CASES)
    calls = [c for rec in golden.values() for c in rec['calls']]
    seen = {c[0] for c in calls}
    assert seen >= lc.REQUIRED_ENTRIES, lc.REQUIRED_ENTRIES - seen
    streams = {c[-1] for c in calls if c[0] in lc.WGRAD_ENTRIES}
    assert streams == {'main', 'side'}, streams
