"""BiFPN without a GPU: the four classes and their state-dict layout against the reference's (tests/golden/bifpn_keys.json,
tools/gen_golden_bifpn.py), Fusion's initial values and asserts, the argument checks of the evk_wfuse_* entry points (every
one returns before a launch), the host-only plan, and the loud failure on CPU tensors."""
import ctypes
import json
import os

import pytest
import torch

import ever_amd as er
from ever_amd import _C
from tests import bifpn_common as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
P, I = ctypes.c_void_p, ctypes.c_int32


def test_classes_are_exported():
    for name in ('Fusion', 'FastNormalizedFusionConv3x3', 'NormalizedFusionConv3x3', 'BiFPN'):
        assert name in er.module.__all__ and hasattr(er.module, name), name
    from ever_amd.module.layers import UpsamplingNearest2d
    assert issubclass(UpsamplingNearest2d, torch.nn.UpsamplingNearest2d)
    assert issubclass(er.module.FastNormalizedFusionConv3x3, torch.nn.Sequential)


@pytest.mark.parametrize('case', sorted(bc.KEY_CASES))
def test_state_dict_layout_equals_the_reference(case):
    want = json.load(open(os.path.join(GOLD, 'bifpn_keys.json')))[case]
    sd = er.module.BiFPN(256, **bc.KEY_CASES[case]).state_dict()
    assert list(sd) == list(want)
    for k, v in sd.items():
        assert list(v.shape) == want[k], k
    for k in ('bin_fusion_modules.0.0.weights', 'bin_fusion_modules.0.1.0.weight', 'bin_fusion_modules.0.1.2.bias',
              'bin_fusion_modules.0.2.running_mean', 'triple_fusion_modules.2.0.weights'):
        assert k in sd


def test_fusion_initial_values_and_asserts():
    assert torch.equal(er.module.Fusion(3).weights.detach(), torch.ones(3))
    assert torch.equal(er.module.Fusion(2, 'softmax').weights.detach(), torch.zeros(2))
    assert er.module.Fusion.eps == 0.0001
    f = er.module.Fusion(2)
    with torch.no_grad():
        f.weights.fill_(3.0)
    f.reset_parameters()
    assert torch.equal(f.weights.detach(), torch.ones(2))
    with pytest.raises(AssertionError):
        er.module.Fusion(1)
    with pytest.raises(AssertionError):
        er.module.Fusion(2, 'sigmoid')
    m = er.module.BiFPN(8, [4, 8, 16, 16], 'softmax', 'maxpool')
    assert all(b[0].norm_method == 'softmax' for b in list(m.bin_fusion_modules) + list(m.triple_fusion_modules))
    # the repeated stride: 1x1 Conv-BN-ReLU in place of the resampling, at the reference's positions
    assert isinstance(m.upsample_modules[0], torch.nn.Sequential) and isinstance(m.upsample_modules[1], torch.nn.UpsamplingNearest2d)
    assert isinstance(m.downsample_modules[0][0], torch.nn.MaxPool2d) and isinstance(m.downsample_modules[2][0], torch.nn.Conv2d)
    assert m.downsample_modules[2][0].kernel_size == (1, 1)


def _fwd(lib, nterms=2, shifts=(0, 1), terms=(16, 16), weights=16, norm=0, n=1, h=8, w=8, c=8, y=16):
    k = max(len(shifts), 1)
    return lib.evk_wfuse_fwd((P * k)(*terms[:k]), (I * k)(*shifts), nterms, weights, norm, 1e-4, y, n, h, w, c, None)


def _bwd(lib, nterms=2, shifts=(0, 1), terms=(16, 16), dterms=(16, 16), weights=16, norm=0, dy=16, dw=16, ws=16, ws_bytes=1 << 20,
         n=1, h=8, w=8, c=8):
    k = max(len(shifts), 1)
    return lib.evk_wfuse_bwd(dy, (P * k)(*terms[:k]), (I * k)(*shifts), nterms, weights, norm, 1e-4, (P * k)(*dterms[:k]), dw, ws,
                             ws_bytes, n, h, w, c, None)


def test_wfuse_entry_points_check_before_launch():
    """(the pointers are never dereferenced: every call below returns before a launch)"""
    lib = _C.load()
    for call in (_fwd, _bwd):
        assert call(lib, c=6) == -2 and b'multiple of 4' in lib.evk_last_error()
        assert call(lib, nterms=0) == -2 and b'terms' in lib.evk_last_error()
        assert call(lib, nterms=5) == -2 and b'terms' in lib.evk_last_error()
        assert call(lib, shifts=(0, 2)) == -2 and b'shift 2' in lib.evk_last_error()
        assert call(lib, h=7) == -2 and b'must be even' in lib.evk_last_error()
        assert call(lib, w=5) == -2 and b'must be even' in lib.evk_last_error()
        assert call(lib, norm=2) == -2 and b'norm = 2' in lib.evk_last_error()
        assert call(lib, n=1 << 15, h=1 << 10, w=1 << 10, c=4) == -2 and b'2^31' in lib.evk_last_error()
        assert call(lib, h=0) == -1 and call(lib, c=-4) == -1
        assert call(lib, terms=(16, None)) == -1 and b'term 1' in lib.evk_last_error()
    assert _fwd(lib, y=None) == -1
    assert lib.evk_wfuse_fwd(None, None, 1, None, 0, 1e-4, 16, 1, 8, 8, 8, None) == -1
    assert _bwd(lib, dy=None) == -1
    assert _bwd(lib, weights=None) == -1 and _bwd(lib, ws=None) == -1        # the weight gradient needs both
    assert _bwd(lib, ws=24) == -1                                            # a workspace off the 16-byte grid
    assert _bwd(lib, dterms=(None, None), dw=None) == -1 and b'no output' in lib.evk_last_error()
    assert _bwd(lib, ws_bytes=16) == -2 and b'workspace' in lib.evk_last_error()


@pytest.mark.parametrize('shape', [(1, 2, 2, 4), (2, 3, 5, 12), (3, 6, 10, 20), (2, 64, 64, 64), (16, 128, 128, 256)])
def test_wfuse_plan_and_workspace_agree(shape):
    lib = _C.load()
    n, h, w, c = shape
    out = (I * 8)()
    for k in (1, 2, 3, 4):
        assert lib.evk_wfuse_plan(n, h, w, c, k, out) == 0, lib.evk_last_error()
        grid, threads, depth, ws_bytes, quad, run, dots_at = list(out)[:7]
        assert ws_bytes == lib.evk_wfuse_workspace_bytes(n, h, w, c, k) > 0
        assert threads == 256 and quad == int(h % 2 == 0 and w % 2 == 0)
        items = n * h * w * (c // 4) // (4 if quad else 1)
        assert grid == -(-items // (threads * run))                 # no cap: the grid grows with the map
        assert depth == run * (4 if quad else 1) * 4                # floats of one thread's run, each one product of a partial
        assert dots_at == 4 * grid and ws_bytes == 4 * (dots_at + 4)
    assert lib.evk_wfuse_plan(n, h, w, 6, 2, out) == -2 and lib.evk_wfuse_workspace_bytes(n, h, w, 6, 2) == 0
    assert lib.evk_wfuse_plan(n, h, w, c, 5, out) == -2 and lib.evk_wfuse_plan(n, h, w, c, 2, None) == -1


def test_cpu_tensors_are_refused():
    from ever_amd.hip import functional as HF
    assert 'weighted_fuse' in HF.__all__ and 'upsample_nearest2x' in HF.__all__ and all(hasattr(HF, n) for n in HF.__all__)
    with pytest.raises(ValueError, match='1 to 4 terms'):
        HF.weighted_fuse([], None)
    with pytest.raises(ValueError, match='norm_method'):
        HF.weighted_fuse([(torch.zeros(1, 4, 2, 2), 0)], None, 'sigmoid')
    with pytest.raises(HF.HipPathError):
        HF.weighted_fuse([(torch.zeros(1, 4, 2, 2), 0), (torch.zeros(1, 4, 1, 1), 1)], torch.ones(2))
    with pytest.raises(HF.HipPathError):
        er.module.Fusion(2)([torch.zeros(1, 4, 2, 2), torch.zeros(1, 4, 2, 2)])
    m = er.module.BiFPN(8, [4, 8, 16, 32])
    with pytest.raises(HF.HipPathError):
        m([torch.zeros(1, 8, 16 >> i, 16 >> i) for i in range(4)])
    from ever_amd.module.layers import UpsamplingNearest2d
    with pytest.raises(NotImplementedError):
        UpsamplingNearest2d(scale_factor=4.)(torch.zeros(1, 4, 2, 2))


def test_install_as_ever_exposes_bifpn():
    import sys
    saved = {k: v for k, v in sys.modules.items() if k == 'ever' or k.startswith('ever.')}
    try:
        er.install_as_ever()
        import ever.module as em
        assert em.BiFPN is er.module.BiFPN and em.Fusion is er.module.Fusion
    finally:
        for k in [k for k in sys.modules if k == 'ever' or k.startswith('ever.')]:
            del sys.modules[k]
        sys.modules.update(saved)
