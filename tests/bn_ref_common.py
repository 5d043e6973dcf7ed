"""What the float64 tests of the BatchNorm family share (tests/test_bn_gpu.py: bn.hip, bn_pool.hip; tests/test_bn_dot_gpu.py:
bn_dot.hip; tests/test_relation_bn_edges_gpu.py with tests/relation_ref_common.py: relation.hip's BatchNorm form): NaN-filled outputs inside sentinel-guarded allocations, the error / bound assertion, the operand-scale check, the
float64 BatchNorm backward with its derived bounds (u = 2^-24; DESIGN.md §6b carries the derivation) and the seeded inputs."""
import torch

from tests.guard_common import guarded, guards_intact

U = 2.0 ** -24
NAN_BITS = 0x7fc00000
LEFT_OUT = 1e-3         # share of elements (windows) that may go without a gradient

WORST = {}              # quantity -> (error / bound, where)


class Bufs:
    """device outputs of one case: NaN-filled, each inside its own sentinel-guarded allocation"""

    def __init__(self, dev):
        self.dev, self.all = dev, []

    def out(self, n, dtype=torch.float32):
        nf = (n * torch.empty((), dtype=dtype).element_size() + 3) // 4
        whole, inner = guarded(nf, self.dev)
        self.all.append((whole, nf))
        return inner.view(dtype)[:n]

    def workspace(self, lib, rows, c):
        nbytes = lib.evk_bn_workspace_bytes(rows, c)
        return self.out(nbytes // 4), nbytes

    def check(self, what):
        torch.cuda.synchronize()
        for whole, n in self.all:
            assert guards_intact(whole, n), ('a store beside a buffer', what)


def _amax_holds(words, out, what):
    """the maximum over the 64 slots (a cache line apart) is max|out| bit for bit; no other word was touched"""
    w = words.cpu().view(64, 32)
    want = int(out.abs().max().reshape(1).cpu().view(torch.int32))
    assert int(w[:, 0].max()) == want, ('absmax', what, hex(int(w[:, 0].max())), hex(want))
    assert bool((w[:, 1:] == NAN_BITS).all()), ('absmax: a word between the slots', what)


def _hold(name, got, ref, bound, what, worst=WORST):
    got = got.detach().cpu()
    assert torch.isfinite(got).all(), (name, 'holds an element nobody wrote', what)
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.expand_as(err).clamp_min(1e-300))
    top = ratio.max().item()
    if top > worst.get(name, (-1.0,))[0]:
        worst[name] = (top, what)
    print(f'{str(what):44s} {name:14s} error / bound {top:.3f}')
    assert top <= 1.0, (name, what, 'error / bound', top)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Stats:
    pass


def _given_stats(mean, invstd, e_mean, e_invstd):
    st = Stats()
    st.mean, st.invstd, st.e_mean, st.e_invstd = mean, invstd, e_mean, e_invstd
    return st


def _bwd_ref(x, g, st, gamma, train, chain, e_g=None, e_sums=None):
    """dbeta, dgamma, dx of BatchNorm in float64 from the masked gradient g, and their bounds.  st: the statistics the kernel
    is GIVEN and their error against the true ones; chain: the reduce pass's; e_g: the error g itself arrives with;
    e_sums: (e_dbeta, e_dgamma) of sums that were not formed by the reduce pass"""
    xd = x.double()
    rows = xd.shape[0]
    xc = xd - st.mean
    xh = xc * st.invstd
    e_xh = st.invstd * st.e_mean + xc.abs() * st.e_invstd + 2 * U * xh.abs()
    gx = g * xh
    dbeta, dgamma = g.sum(0), gx.sum(0)
    if e_sums is None:
        e_db = chain * U * g.abs().sum(0) + U * dbeta.abs()
        e_dg = (chain + 1) * U * gx.abs().sum(0) + (g.abs() * e_xh).sum(0) + U * dgamma.abs()
        if e_g is not None:
            e_db = e_db + e_g.sum(0)
            e_dg = e_dg + (e_g * xh.abs()).sum(0)
    else:
        e_db, e_dg = e_sums
    k0 = gamma * st.invstd
    e_k0 = gamma.abs() * st.e_invstd + U * k0.abs()
    zero = torch.zeros_like(dbeta)
    k1, k2 = (dbeta / rows, dgamma / rows) if train else (zero, zero)
    e_k1, e_k2 = (e_db / rows + U * k1.abs(), e_dg / rows + U * k2.abs()) if train else (zero, zero)
    inner = g - k1 - xh * k2
    dx = k0 * inner
    e_dx = (k0.abs() * (e_k1 + xh.abs() * e_k2 + k2.abs() * e_xh + (0.0 if e_g is None else e_g)) + e_k0 * inner.abs() +
            4 * U * k0.abs() * (g.abs() + k1.abs() + (xh * k2).abs()))
    return dbeta, e_db, dgamma, e_dg, dx, e_dx


def _params(gen, c, affine):
    if not affine:
        return None, None, torch.ones(c, dtype=torch.float64), torch.zeros(c, dtype=torch.float64)
    gamma = (0.5 + torch.rand(c, generator=gen)) * torch.where(torch.rand(c, generator=gen) < 0.25, -1.0, 1.0)
    beta = 0.5 * torch.randn(c, generator=gen)
    return gamma, beta, gamma.double(), beta.double()


def _data(gen, rows, c):
    """seeded randn with a scale and an offset of its own per channel"""
    return torch.randn(rows, c, generator=gen) * (0.5 + 1.5 * torch.rand(c, generator=gen)) + 2 * torch.rand(c, generator=gen) - 1
