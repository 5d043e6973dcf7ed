"""Sentinel-guarded device allocations for the kernel tests: an output (or a workspace) is a NaN-filled slice inside a larger
allocation whose surroundings hold a sentinel.  An element nobody wrote stays NaN, a store beside the slice breaks the sentinel."""
import torch

PAD = 64            # elements of sentinel on either side (64 floats keep the slice 256-byte aligned)
SENTINEL = 12345.0


def guarded(n, device, dtype=torch.float32):
    """(whole, inner): a NaN-filled slice of n elements inside a sentinel-filled allocation"""
    whole = torch.full((n + 2 * PAD,), SENTINEL, device=device, dtype=dtype)
    inner = whole[PAD:PAD + n]
    inner.fill_(float('nan'))
    return whole, inner


def guards_intact(whole, n):
    return bool((whole[:PAD] == SENTINEL).all() and (whole[PAD + n:] == SENTINEL).all())
