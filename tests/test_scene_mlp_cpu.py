"""CPU: the FS-Relation scene-MLP entry points (include/ever_hip.h: evk_relation_scene_*) check their arguments before any
launch, so the refusals can be read without a GPU; the Python mirror of the shape rule agrees with the library."""
import ctypes

from ever_amd import _C


def _ptrs(n, null_at=None):
    return (ctypes.c_void_p * n)(*[None if i == null_at else 4096 * (i + 1) for i in range(n)])


def _fwd(lib, levels, n, k, c, b1_null_at=None):
    a = _ptrs(max(levels, 1))
    return lib.evk_relation_scene_fwd(4096, a, _ptrs(max(levels, 1), b1_null_at), a, a, 4096, 4096, levels, n, k, c, None)


def _bwd(lib, levels, n, k, c, ws_bytes=1 << 30):
    a = _ptrs(max(levels, 1))
    return lib.evk_relation_scene_bwd(4096, 4096, a, a, a, 4096, 4096, a, a, a, a, levels, n, k, c, 4096, ws_bytes, None)


def test_unsupported_shapes_are_refused_before_any_launch():
    from ever_amd.hip.pointwise import scene_mlp_admits
    lib = _C.load()
    for levels, n, k, c, word in ((4, 33, 512, 64, b'rows'), (9, 16, 512, 64, b'levels'), (4, 16, 6, 64, b'multiples of 4'),
                                  (4, 16, 512, 6, b'multiples of 4')):
        assert not scene_mlp_admits(levels, n, k, c)
        for call in (_fwd, _bwd):
            assert call(lib, levels, n, k, c) == -2 and word in lib.evk_last_error(), (levels, n, k, c)   # EVK_E_UNSUPPORTED
    assert scene_mlp_admits(4, 16, 2048, 256) and scene_mlp_admits(8, 32, 8, 4) and scene_mlp_admits(1, 1, 4, 4)
    assert _fwd(lib, 4, 16, 512, 64, b1_null_at=2) == -2 and b'without bias' in lib.evk_last_error()
    assert lib.evk_relation_scene_fwd(4096, _ptrs(4), None, _ptrs(4), _ptrs(4), 4096, 4096, 4, 16, 512, 64, None) == -2
    assert _fwd(lib, 0, 16, 512, 64) == -1 and _bwd(lib, 4, 0, 512, 64) == -1                              # EVK_E_INVALID
    assert lib.evk_relation_scene_fwd(None, _ptrs(4), _ptrs(4), _ptrs(4), _ptrs(4), 4096, 4096, 4, 16, 512, 64, None) == -1
    assert lib.evk_relation_scene_fwd(4100, _ptrs(4), _ptrs(4), _ptrs(4), _ptrs(4), 4096, 4096, 4, 16, 512, 64, None) == -1


def test_slice_workspace_follows_the_shapes_alone():
    """slices x ceil(K / 256) workgroups cover the 256 CUs, at most 64 slices, never more than there are weight rows"""
    lib = _C.load()

    def slices(levels, n, k, c):
        nbytes = lib.evk_relation_scene_bwd_workspace_bytes(levels, n, k, c)
        assert nbytes % (4 * n * k) == 0
        return nbytes // (4 * n * k)
    assert slices(4, 16, 2048, 256) == 32          # FarSeg-R50: 8 column blocks x 32 slices of 32 weight rows
    assert slices(4, 16, 512, 64) == 64 and slices(4, 3, 512, 64) == 64
    assert slices(1, 1, 8, 4) == 4 and slices(8, 32, 1028, 96) == 52
    assert lib.evk_relation_scene_bwd_workspace_bytes(0, 16, 512, 64) == 0
    assert _bwd(lib, 4, 16, 2048, 256, ws_bytes=32 * 16 * 2048 * 4 - 1) == -4                             # EVK_E_WORKSPACE
