"""The forms and the backward tiling of the depthwise kernels (csrc/depthwise.hip: dw_plan) asked of the library on the host
through evk_depthwise_plan — the function the launchers and the workspace size take them from: the case table of
tests/depthwise_common.py states a form and plan facts per case and must reach every form, every cl and every fact; the cl
rule's property; the workspace formula; the refusals (the kernel extent against the padded input among them), which the launch
entries repeat before they look at a pointer."""
import ctypes

import pytest

from ever_amd import _C
from tests import depthwise_common as DC

IDS = [c['name'] for c in DC.CASES]


@pytest.mark.parametrize('case', DC.CASES, ids=IDS)
def test_case_has_the_form_and_the_plan_facts_it_states(case):
    lib = _C.load()
    p = DC.plan(lib, case)
    ho, wo = DC.out_size(case)
    assert (p['fkw'], p['fsw'], p['fd1']) == case['fwd'] and (p['bkw'], p['bs1d1']) == case['bwd']
    for fact in case['facts']:
        assert DC.FACT_CHECKS[fact](case, p, (ho, wo)), (case['name'], fact, p)
    # the tiling covers the larger of the input and the output map, and the grid fits
    c4 = case['c'] // 4
    assert p['cl'] * p['ps'] == 256 and p['cblocks'] * p['cl'] >= c4 > (p['cblocks'] - 1) * p['cl']
    assert p['bstrips'] * DC.KTB >= max(case['w'], wo) > (p['bstrips'] - 1) * DC.KTB
    assert p['strip_groups'] * p['ps'] >= p['bstrips'] > (p['strip_groups'] - 1) * p['ps']
    assert p['row_tiles'] * DC.KTH >= max(case['h'], ho) > (p['row_tiles'] - 1) * DC.KTH
    assert p['tiles'] == case['n'] * p['row_tiles'] * p['strip_groups']
    assert p['fstrips'] * DC.KTW >= wo > (p['fstrips'] - 1) * DC.KTW
    assert p['fblocks'] == -(-case['n'] * ho * p['fstrips'] * c4 // 256)
    taps = case['k'][0] * case['k'][1]
    assert lib.evk_depthwise_bwd_workspace_bytes(ctypes.byref(DC.desc(case))) == p['tiles'] * (taps + 1) * case['c'] * 4
    assert case['n'] <= 3 and max(case['h'], case['w'], ho, wo) <= 40


def test_table_reaches_every_form_lane_count_and_fact():
    lib = _C.load()
    plans = [DC.plan(lib, c) for c in DC.CASES]
    assert {(p['fkw'], p['fsw'], p['fd1']) for p in plans} == DC.REQUIRED_FWD
    assert {(p['bkw'], p['bs1d1']) for p in plans} == DC.REQUIRED_BWD
    assert {p['cl'] for p in plans} == DC.REQUIRED_CL
    assert set().union(*(c['facts'] for c in DC.CASES)) == DC.REQUIRED_FACTS
    assert DC.REQUIRED_KERNELS <= {c['k'] for c in DC.CASES}
    assert {(c['bias'], c['relu']) for c in DC.CASES} == {(False, False), (False, True), (True, False), (True, True)}
    # the subsets of the GPU file: one unit-normal case per cl and the 72-tile case; the partial requests
    by = dict(zip(DC.BY_NAME, plans))
    assert {by[n]['cl'] for n in DC.NORMAL_CASES} == DC.REQUIRED_CL and by['t72']['tiles'] == 72 and 't72' in DC.NORMAL_CASES
    assert all(n in DC.BY_NAME for n in DC.PARTIAL_CASES)


def test_references_stay_inside_their_caps():
    """what the GPU file relies on, from the reference alone: exact inputs keep every sum of magnitudes below 2^24 (asserted
    inside reference()) and put exact zeros with a non-zero gradient under every fused ReLU; the unit-normal seeds leave at
    most 0.1 % of a case's elements without a certain mask"""
    for case in DC.CASES:
        r = DC.reference(case, 'exact')
        if case['relu']:
            zeros = r['pre'] == 0
            assert bool(zeros.any()) and bool((r['g'][zeros] != 0).any()), case['name']
    for name in DC.NORMAL_CASES:
        r = DC.reference(DC.BY_NAME[name], 'normal')
        assert int(r['uncertain'].sum()) <= 1e-3 * r['pre'].numel(), name
        assert DC.BY_NAME[name]['relu'] or not bool(r['uncertain'].any())


def _desc_c(c, h=8, w=8):
    return _C.ConvDesc(1, h, w, c, h, w, c, 3, 3, 1, 1, 1, 1, 1, 1)


@pytest.mark.parametrize('c4', list(range(1, 130)) + [152, 256, 512, 513])
def test_lanes_are_a_power_of_two_and_no_narrower_width_idles_fewer(c4):
    rc, p = DC.plan_of_desc(_C.load(), _desc_c(4 * c4))
    assert rc == 0
    cl = p['cl']
    assert 1 <= cl <= 64 and cl & (cl - 1) == 0 and p['ps'] * cl == 256
    idle = -(-c4 // cl) * cl - c4
    narrower = [w for w in (1, 2, 4, 8, 16, 32) if w < cl]
    assert all(-(-c4 // w) * w - c4 >= idle for w in narrower if w >= 16), (c4, cl)
    if c4 <= 16:          # the narrowest power of two that holds the channels in one block
        assert cl >= c4 > cl // 2 and p['cblocks'] == 1
    else:                 # at least a quarter wave; a wider block only where it idles no more lanes
        assert cl >= 16
        for w in (32, 64):
            if w > cl:
                assert -(-c4 // w) * w - c4 > idle, (c4, cl, w)


def test_lane_counts_of_the_channel_counts_in_use():
    lib = _C.load()
    got = {c: DC.plan_of_desc(lib, _desc_c(c))[1]['cl'] for c in (4, 8, 12, 16, 32, 64, 96, 132, 196, 256, 304, 2048)}
    assert got == {4: 1, 8: 2, 12: 4, 16: 4, 32: 8, 64: 16, 96: 32, 132: 16, 196: 64, 256: 64, 304: 16, 2048: 64}


UNTOUCHED = {k: -7 for k in DC.PLAN_FIELDS}
REFUSED = [
    # descriptor, return code, a word of the message
    (_C.ConvDesc(2, 16, 16, 32, 16, 16, 64, 3, 3, 1, 1, 1, 1, 1, 1), -2, b'Cin'),
    (_C.ConvDesc(2, 16, 16, 6, 16, 16, 6, 3, 3, 1, 1, 1, 1, 1, 1), -2, b'multiple of 4'),
    (_C.ConvDesc(2, 16, 16, 32, 6, 6, 32, 3, 3, 3, 3, 1, 1, 1, 1), -2, b'stride'),
    (_C.ConvDesc(2, 16, 16, 32, 16, 16, 32, 8, 3, 1, 1, 1, 1, 1, 1), -2, b'kernel'),
    (_C.ConvDesc(2, 16, 16, 32, 16, 16, 32, 3, 3, 1, 1, 1, 1, 0, 1), -2, b'dilation'),
    (_C.ConvDesc(2, 16, 16, 32, 16, 16, 32, 3, 3, 1, 1, -1, 1, 1, 1), -2, b'padding'),
    (_C.ConvDesc(0, 16, 16, 32, 16, 16, 32, 3, 3, 1, 1, 1, 1, 1, 1), -1, b'non-positive'),
    (_C.ConvDesc(2, 16, 16, 32, 15, 16, 32, 3, 3, 1, 1, 1, 1, 1, 1), -1, b'output size'),
    # H + 2 ph - dh (kh - 1) - 1 == -1 under stride 2: truncating division answers Ho = 1, flooring 0
    (_C.ConvDesc(1, 4, 8, 4, 1, 3, 4, 3, 3, 2, 2, 0, 0, 2, 1), -1, b'extent 5 along H'),
    (_C.ConvDesc(1, 8, 4, 4, 3, 1, 4, 3, 3, 2, 2, 0, 0, 1, 2), -1, b'extent 5 along W'),
    (_C.ConvDesc(1, 2, 9, 4, 1, 9, 4, 2, 1, 2, 1, 0, 0, 3, 1), -1, b'extent 4 along H'),
    # far too small: refused by the extent too, whatever Ho says
    (_C.ConvDesc(1, 2, 8, 4, 1, 8, 4, 7, 1, 1, 1, 0, 0, 1, 1), -1, b'along H'),
]


@pytest.mark.parametrize('d,rc,word', REFUSED, ids=[r[2].decode() + f'-{i}' for i, r in enumerate(REFUSED)])
def test_refusals_leave_the_answer_untouched_and_the_launches_repeat_them(d, rc, word):
    lib = _C.load()
    got, p = DC.plan_of_desc(lib, d)
    assert got == rc and p == UNTOUCHED and word in lib.evk_last_error(), lib.evk_last_error()
    assert lib.evk_depthwise_bwd_workspace_bytes(ctypes.byref(d)) == 0
    # the launch entries refuse the same descriptors before they look at a pointer or launch anything: safe without a GPU
    assert lib.evk_depthwise_fwd(ctypes.byref(d), None, None, None, None, 0, None) == rc
    assert word in lib.evk_last_error()
    assert lib.evk_depthwise_bwd(ctypes.byref(d), None, None, None, None, None, None, None, None, 0, None) == rc
    assert word in lib.evk_last_error()


def test_extent_equal_to_the_padded_input_is_accepted():
    """the smallest legal map: one output; one row or column less is the refusal above"""
    lib = _C.load()
    for d in (_C.ConvDesc(1, 5, 8, 4, 1, 3, 4, 3, 3, 2, 2, 0, 0, 2, 1), _C.ConvDesc(1, 3, 3, 4, 1, 1, 4, 3, 3, 2, 2, 1, 1, 2, 2)):
        rc, p = DC.plan_of_desc(lib, d)
        assert rc == 0 and p['tiles'] >= 1, lib.evk_last_error()


def test_null_pointers_and_grids_that_do_not_fit():
    lib = _C.load()
    ok = _desc_c(32)
    assert lib.evk_depthwise_plan(ctypes.byref(ok), None) == -1
    assert lib.evk_depthwise_plan(None, (ctypes.c_int32 * 14)()) == -1
    assert lib.evk_depthwise_fwd(ctypes.byref(ok), None, None, None, None, 0, None) == -1
    assert lib.evk_depthwise_bwd(ctypes.byref(ok), None, None, None, None, None, None, None, None, 0, None) == -1
    # 2^31 forward workgroups: N Ho strips C/4 / 256 with C = 2^20, a 2^11 x 2^13 map
    big = _C.ConvDesc(2 ** 10, 2 ** 11, 2 ** 13, 2 ** 20, 2 ** 11, 2 ** 13, 2 ** 20, 1, 1, 1, 1, 0, 0, 1, 1)
    rc, p = DC.plan_of_desc(lib, big)
    assert rc == -2 and p == UNTOUCHED and b'grid' in lib.evk_last_error()
    assert lib.evk_depthwise_fwd(ctypes.byref(big), 1, 1, None, 1, 0, None) == -2
    # more than 65535 channel blocks of 64 lanes
    wide = _C.ConvDesc(1, 1, 1, 2 ** 24 + 256, 1, 1, 2 ** 24 + 256, 1, 1, 1, 1, 0, 0, 1, 1)
    rc, p = DC.plan_of_desc(lib, wide)
    assert rc == -2 and p == UNTOUCHED and b'grid' in lib.evk_last_error()
    assert lib.evk_depthwise_bwd(ctypes.byref(wide), 1, None, None, 1, 1, None, None, None, 0, None) == -2
