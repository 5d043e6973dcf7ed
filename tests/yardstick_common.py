"""The tolerance of the kernel tests that fix nothing in advance: aten's own fp32 CPU result is measured against the same fp64
reference as the kernel, and the kernel may err at most twice as much plus a few ulp of the largest |reference| (the floor for
cases whose yardstick is 0).  The factor two is the margin of test_ops_gpu.py::test_conv_split_matches_fp64_as_well_as_fp32_mfma."""
import numpy as np


def ulp(v):
    return float(np.spacing(np.float32(abs(v))))


def as_close_as_aten(got, ref64, ref32, what, ulps=4):
    """max |got - ref64| <= 2 max |aten fp32 - ref64| + ulps ulp(max |ref64|); returns error / yardstick for the record"""
    assert got.shape == ref64.shape, (what, tuple(got.shape), tuple(ref64.shape))
    yard = (ref32.double() - ref64).abs().max().item()
    err = (got.double() - ref64).abs().max().item()
    floor = ulps * ulp(ref64.abs().max().item())
    ratio = err / yard if yard else float('nan')
    print(f'{what}: kernel err {err:.3e}, aten fp32 err {yard:.3e}, ratio {ratio:.3f}, '
          f'bound {2 * yard + floor:.3e} (used {err / (2 * yard + floor):.3f})')
    assert err <= 2 * yard + floor, f'{what}: err {err:.3e} > 2 * {yard:.3e} + {floor:.3e}'
    return ratio
