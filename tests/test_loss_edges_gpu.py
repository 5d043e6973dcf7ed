"""The pixel losses and evaluation metrics (csrc/loss.hip, csrc/loss_pixel.hip and csrc/metric.hip) at the edges
of their launch grids, class counts and labels.

Reference: the same formula in float64 torch on the CPU, from the same fp32 inputs; gradients by autograd on it.
Tolerances: the project's loss 1e-5 / gradient 1e-4 (test_ops_gpu.py::test_losses), taken relative to the reference's own
maximum with atol = 0 — at 4 million pixels a gradient is 2.5e-7, so any absolute slack would hide everything.  Whatever is
an integer (valid-pixel counts, label histograms, confusion matrices, numbers of kept elements) is compared exactly.

Grid facts the sizes below are chosen around:
  BCE/dice/CE forward  ceil(npix / 2048) workgroups, at most 2048: second workgroup at 2,049 pixels, cap at 4,194,304
  every backward       ceil(n / 256) workgroups, at most 4096: cap at 1,048,576 elements
  statistics, focal,   ceil(n / 1024) workgroups, at most 256: cap at 262,144 elements
  OHEM, confusion
Logits are laid out [1, C, H, W] over dense NHWC memory, so no transposition kernel runs in front of the loss."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

RTOL_LOSS, RTOL_GRAD = 1e-5, 1e-4
IGNORE = 255


# ------------------------------------------------------------------------------------------------ helpers
def _close(got, ref, rtol, what):
    """max |got - ref| <= rtol * max |ref|, wherever the reference is finite; `got` must be finite there."""
    got, ref = got.detach().cpu().double(), ref.detach().double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    fin = torch.isfinite(ref)
    assert bool(fin.any()), f'{what}: the reference has no finite value'
    assert bool(torch.isfinite(got[fin]).all()), f'{what}: not finite where the float64 reference is'
    scale = ref[fin].abs().max().item()
    err = (got[fin] - ref[fin]).abs().max().item()
    print(f'{what}: max err {err:.3e}, reference max {scale:.3e}, ratio {err / scale if scale else 0.0:.3e} (bound {rtol:g})')
    assert err <= rtol * scale, f'{what}: max err {err:.3e} > {rtol:g} * {scale:.3e}'


def _nhw(npix):
    """[1, H, W] with H * W = npix; a ragged width where npix has a small factor, else W = 1"""
    for w in (7, 5, 3, 2):
        if npix % w == 0 and npix > w:
            return 1, npix // w, w
    return 1, npix, 1


def _nhwc_randn(npix, c, g, scale):
    n, h, w = _nhw(npix)
    return (torch.randn(n, h, w, c, generator=g) * scale).permute(0, 3, 1, 2)   # logical NCHW over NHWC memory


def _mark_ignored(labels, g, ignore):
    """about 5 % ignored anywhere, and always the first three and the last two pixels: a dropped tail changes the count"""
    n = labels.numel()
    if n < 8:
        return
    labels[torch.rand(n, generator=g) < 0.05] = ignore
    labels[:3] = ignore
    labels[-2:] = ignore
    labels[3], labels[-3] = 1, 0


@functools.lru_cache(maxsize=6)
def _pixels(npix, c, ignore=IGNORE, scale=2.0):
    """(fp32 logits [1, C, H, W], int64 labels [1, H, W]); shared by the tests of one size — never written to"""
    g = torch.Generator().manual_seed(1000 * c + npix % 997)
    logits = _nhwc_randn(npix, c, g, scale)
    labels = torch.randint(0, max(c, 2), (npix,), generator=g)
    if npix == 1:
        labels[0] = 1
    _mark_ignored(labels, g, ignore)
    return logits, labels.reshape(_nhw(npix))


@functools.lru_cache(maxsize=2)
def _soft_target(npix, c):
    g = torch.Generator().manual_seed(77 + npix % 997)
    return torch.softmax(_nhwc_randn(npix, c, g, 1.0), dim=1)


def _range_logits(npix, c, seed):
    """randn mixed with values at which a naive exp / softmax overflows fp32"""
    g = torch.Generator().manual_seed(seed)
    n, h, w = _nhw(npix)
    big = torch.tensor([-80., -20., 0., 20., 80.])[torch.randint(0, 5, (n, h, w, c), generator=g)]
    x = torch.where(torch.rand(n, h, w, c, generator=g) < 0.5, big, torch.randn(n, h, w, c, generator=g) * 2)
    return x.permute(0, 3, 1, 2)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _loss_stats(k, cuda):
    from ever_amd import _C
    return torch.zeros((_C.load().evk_loss_stats_doubles(k),), device=cuda, dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ float64 references
def _ref_bce(x, labels, ignore=IGNORE):
    yp, yt = x.reshape(-1), labels.reshape(-1)
    valid = yt != ignore
    return TF.binary_cross_entropy_with_logits(yp[valid], yt[valid].to(x.dtype))


def _ref_dice(x, labels, smooth=1.0, ignore=IGNORE, ignore_channel=-1):
    """_ref_dice of test_ops_gpu.py in the dtype of `x`"""
    c = x.size(1)
    yp, yt = x.permute(0, 2, 3, 1).reshape(-1, c), labels.reshape(-1)
    valid = yt != ignore
    yp, yt = yp[valid], yt[valid]
    keep = torch.ones(c, dtype=torch.bool)
    if c == 1:
        prob, tgt = yp.sigmoid(), yt.reshape(-1, 1).to(x.dtype)
    else:
        prob, tgt = yp.log_softmax(dim=1).exp(), TF.one_hot(yt.long(), c).to(x.dtype)
        if ignore_channel != -1:
            keep[ignore_channel] = False
    prob, tgt = prob[:, keep], tgt[:, keep]
    inter = (prob * tgt).sum(0)
    z = prob.sum(0) + tgt.sum(0) + smooth
    return 1. - ((2 * inter + smooth) / z).mean()


def _ref_soft_ce(x, target):
    return -(target.to(x.dtype) * TF.log_softmax(x, dim=1)).mean(dim=(0, 2, 3)).sum()


def _ref_prob_stats(x, labels, ignore=IGNORE):
    """(tp, sum p, sum y) per class over the valid pixels, as losses.py::tversky_loss_with_logits consumes them"""
    c = x.size(1)
    yp, yt = x.permute(0, 2, 3, 1).reshape(-1, c), labels.reshape(-1)
    valid = yt != ignore
    yp, yt = yp[valid], yt[valid]
    if c > 1:
        p, y = yp.log_softmax(dim=1).exp(), TF.one_hot(yt, c).to(x.dtype)
    else:
        p, y = TF.logsigmoid(yp).exp(), yt.to(x.dtype).unsqueeze(1)
    return (p * y).sum(0), p.sum(0), y.sum(0)


def _ref_tversky(tp, sp, sy, alpha, beta, gamma, smooth=1.0):
    fp, fn = sp - tp, sy - tp
    coeff = (tp + smooth) / (tp + alpha * fn + beta * fp + smooth)
    return ((1. - coeff) ** gamma).mean()


def _ref_focal(x, y, gamma, normalize):
    with torch.no_grad():
        p = x.sigmoid()
        w = ((1 - p) * y + p * (1 - y)).pow(gamma)
    if not normalize:
        return TF.binary_cross_entropy_with_logits(x, y, w, reduction='mean')
    losses = TF.binary_cross_entropy_with_logits(x, y, reduction='none')
    modulated = losses * w
    return modulated.sum() * (losses.sum() / modulated.sum())


def _ref_sigmoid_focal(x, y, alpha, gamma, reduction):
    p = x.sigmoid()
    ce = TF.binary_cross_entropy_with_logits(x, y, reduction='none')
    loss = ce * ((1 - (p * y + (1 - p) * (1 - y))) ** gamma)
    if alpha >= 0:
        loss = (alpha * y + (1 - alpha) * (1 - y)) * loss
    return loss.mean() if reduction == 'mean' else loss.sum()


# ------------------------------------------------------------------------------------------------ one loss, both sides
def _hip_loss(kind, lg, yg, ignore, **kw):
    from ever_amd.hip import functional as HF
    from ever_amd.module import loss as L
    if kind == 'bce':
        return L.binary_cross_entropy_with_logits(lg, yg, ignore_index=ignore)
    if kind == 'dice':
        return L.dice_loss_with_logits(lg, yg, 1.0, ignore, kw.get('ignore_channel', -1), sync_statistics=False)
    if kind == 'ce':
        return HF.cross_entropy(lg, yg, ignore_index=ignore, label_smoothing=kw.get('eps', 0.0))
    if kind == 'softce':
        return L.soft_cross_entropy(lg, yg)
    if kind == 'tversky':
        return L.tversky_loss_with_logits(lg, yg, kw['alpha'], kw['beta'], kw['gamma'], 1.0, ignore, sync_statistics=False)
    raise KeyError(kind)


def _ref_loss(kind, x, y, ignore, **kw):
    if kind == 'bce':
        return _ref_bce(x, y, ignore)
    if kind == 'dice':
        return _ref_dice(x, y, 1.0, ignore, kw.get('ignore_channel', -1))
    if kind == 'ce':
        return TF.cross_entropy(x, y, ignore_index=ignore, label_smoothing=kw.get('eps', 0.0))
    if kind == 'softce':
        return _ref_soft_ce(x, y)
    if kind == 'tversky':
        return _ref_tversky(*_ref_prob_stats(x, y, ignore), kw['alpha'], kw['beta'], kw['gamma'])
    raise KeyError(kind)


def _check_loss(cuda, kind, logits, target, ignore=IGNORE, what='', **kw):
    """loss and gradient of one loss against float64; `target` is the labels, or the distribution of soft CE.
    The upstream gradient is 0.7, so the kernels' grad_scale operand is not the trivial 1."""
    xr = logits.double().requires_grad_()
    ref = _ref_loss(kind, xr, target, ignore, **kw)
    (ref * 0.7).backward()
    lg = logits.to(cuda).requires_grad_()
    out = _hip_loss(kind, lg, target.to(cuda), ignore, **kw)
    (out * 0.7).backward()
    _close(out, ref, RTOL_LOSS, f'{what} {kind} loss')
    _close(lg.grad, xr.grad, RTOL_GRAD, f'{what} {kind} gradient')
    if kind != 'softce':
        gone = (target == ignore).unsqueeze(1).expand_as(logits)
        assert not bool(lg.grad.cpu()[gone].any()), f'{what} {kind}: a gradient on an ignored pixel'
    return out, lg.grad


# ================================================================================================ 1. loss.hip grid edges
GRID_SIZES = [1, 255, 257, 2048, 2049, 6145, 4194304, 4194304 + 2048 * 256 + 3]
GRID_KINDS = {'bce': ('bce', 1), 'dice1': ('dice', 1), 'dice2': ('dice', 2), 'ce2': ('ce', 2), 'softce2': ('softce', 2)}


@pytest.mark.parametrize('npix', GRID_SIZES)
@pytest.mark.parametrize('name', list(GRID_KINDS))
def test_partial_sum_grid_edges(cuda, name, npix):
    """One workgroup, its last thread, the second workgroup, three workgroups with a ragged tail, the 2048-workgroup cap
    exactly and one ragged grid-stride step past it (both also beyond the 4096-workgroup cap of the backward)."""
    kind, c = GRID_KINDS[name]
    logits, labels = _pixels(npix, c)
    _check_loss(cuda, kind, logits, _soft_target(npix, c) if kind == 'softce' else labels, what=f'npix={npix}')


@pytest.mark.parametrize('npix', GRID_SIZES)
def test_dice_sigmoid_statistics_are_exact_on_zero_logits(cuda, npix):
    """All-zero logits: p = 1 / (1 + exp(-0)) is exactly 0.5, so inter = 0.5 * sum y and z = 0.5 * valid + sum y are sums
    of multiples of 0.5 — exact in fp64 in any order.  A pixel dropped or counted twice shows as a whole 0.5."""
    from ever_amd import _C
    _, labels = _pixels(npix, 1)
    valid = int((labels != IGNORE).sum())
    ones = int((labels == 1).sum())
    x, y = torch.zeros(npix, device=cuda), labels.to(cuda)
    stats = _loss_stats(2, cuda)
    _C.call('evk_dice_stats', x.data_ptr(), y.data_ptr(), npix, 1, IGNORE, stats.data_ptr(), _stream())
    assert stats[:2].cpu().tolist() == [0.5 * ones, 0.5 * valid + ones]


@pytest.mark.parametrize('npix', GRID_SIZES[-2:])
def test_valid_pixel_counts_are_exact_at_the_grid_cap(cuda, npix):
    """stats[1] of BCE and of CE through the C ABI: the number of valid pixels, summed over 2048 partials"""
    from ever_amd import _C
    loss = torch.empty((), device=cuda)
    logits, labels = _pixels(npix, 1)
    x, y, stats = logits.to(cuda), labels.to(cuda), _loss_stats(2, cuda)
    _C.call('evk_bce_fwd_ex', x.data_ptr(), y.data_ptr(), npix, IGNORE, 0.0, 1.0, 0, loss.data_ptr(), stats.data_ptr(),
            _stream())
    assert stats[1].item() == int((labels != IGNORE).sum())
    logits, labels = _pixels(npix, 2)
    x, y, stats = logits.to(cuda), labels.to(cuda), _loss_stats(3, cuda)
    _C.call('evk_ce_fwd', x.data_ptr(), y.data_ptr(), npix, 2, IGNORE, 0.0, loss.data_ptr(), stats.data_ptr(), _stream())
    assert stats[1].item() == int((labels != IGNORE).sum())


# ================================================================================================ 2. backward / nr_grid caps
NR_SIZES = [1024, 1025, 262144, 262145, 1048576, 1048577]
TVERSKY = dict(alpha=0.3, beta=0.6, gamma=1.5)


def _check_tversky(cuda, logits, labels, what):
    """the raw statistics (sy exactly: it is the label histogram), then the loss on top of them with its gradient"""
    from ever_amd.hip import functional as HF
    c = logits.shape[1]
    st = HF.prob_stats(logits.to(cuda), labels.to(cuda), IGNORE).cpu()
    tp, sp, sy = _ref_prob_stats(logits.double(), labels)
    yv = labels[labels != IGNORE]
    hist = np.bincount(yv.numpy(), minlength=c) if c > 1 else np.array([int(yv.sum())])
    assert st[2].tolist() == hist.tolist(), f'{what}: sum y is not the label histogram'
    assert sy.tolist() == hist.tolist()
    _close(st[0], tp, RTOL_LOSS, f'{what} tp')
    _close(st[1], sp, RTOL_LOSS, f'{what} sum p')
    _check_loss(cuda, 'tversky', logits, labels, what=what, **TVERSKY)


@pytest.mark.parametrize('npix', NR_SIZES)
@pytest.mark.parametrize('c', [1, 2])
def test_tversky_at_the_grid_caps(cuda, c, npix):
    logits, labels = _pixels(npix, c)
    _check_tversky(cuda, logits, labels, f'npix={npix} C={c}')


FOCAL_MODES = {
    'focal': [dict(gamma=2.0, normalize=False)],
    'focal_normalized': [dict(gamma=2.0, normalize=True)],
    'sigmoid_focal_mean': [dict(alpha=a, gamma=g, reduction='mean') for a in (-1, 0.25) for g in (0, 1.5, 2)],
    'sigmoid_focal_sum': [dict(alpha=a, gamma=g, reduction='sum') for a in (-1, 0.25) for g in (0, 1.5, 2)],
}


def _check_focal(cuda, mode, x, y, what):
    from ever_amd.module import loss as L
    hip, ref = (L.focal_loss, _ref_focal) if mode.startswith('focal') else (L.sigmoid_focal_loss, _ref_sigmoid_focal)
    yg = y.to(cuda)
    for cfg in FOCAL_MODES[mode]:
        xr = x.double().requires_grad_()
        want = ref(xr, y.double(), **cfg)
        (want * 0.7).backward()
        xg = x.to(cuda).requires_grad_()
        got = hip(xg, yg, **cfg)
        (got * 0.7).backward()
        _close(got, want, RTOL_LOSS, f'{what} {mode} {cfg} loss')
        _close(xg.grad, xr.grad, RTOL_GRAD, f'{what} {mode} {cfg} gradient')


@pytest.mark.parametrize('n', NR_SIZES)
@pytest.mark.parametrize('mode', list(FOCAL_MODES))
def test_focal_at_the_grid_caps(cuda, mode, n):
    g = torch.Generator().manual_seed(31 + n % 997)
    x = torch.randn(n, generator=g) * 3
    y = (torch.rand(n, generator=g) > 0.6).float()
    _check_focal(cuda, mode, x, y, f'n={n}')


def _check_ce_pixel(cuda, logits, labels, what, ignore=IGNORE):
    """forward and backward (per-pixel upstream gradient, a tenth of it exactly 0: the kernel's shortcut)"""
    from ever_amd.module import loss as L
    g = torch.Generator().manual_seed(5)
    up = torch.rand(labels.shape, generator=g)
    up[torch.rand(labels.shape, generator=g) < 0.1] = 0.0
    xr = logits.double().requires_grad_()
    ref = TF.cross_entropy(xr, labels, ignore_index=ignore, reduction='none')
    ref.backward(up.double())
    lg = logits.to(cuda).requires_grad_()
    pix = L.cross_entropy_per_pixel(lg, labels.to(cuda), ignore)
    pix.backward(up.to(cuda))
    _close(pix, ref, RTOL_LOSS, f'{what} per-pixel CE')
    _close(lg.grad, xr.grad, RTOL_GRAD, f'{what} per-pixel CE gradient')
    assert not bool(pix.detach().cpu()[labels == ignore].any())
    assert not bool(lg.grad.cpu()[(labels == ignore).unsqueeze(1).expand_as(logits)].any())


@pytest.mark.parametrize('npix', NR_SIZES[-2:])
def test_cross_entropy_per_pixel_at_the_backward_grid_cap(cuda, npix):
    _check_ce_pixel(cuda, *_pixels(npix, 2), f'npix={npix}')


# ================================================================================================ 3. class counts
CLASS_NPIX = [2049, 5000]


@pytest.mark.parametrize('npix', CLASS_NPIX)
@pytest.mark.parametrize('c,ignore_channel', [(2, -1), (3, -1), (3, 0), (3, 2), (16, -1), (16, 0), (16, 15)])
def test_dice_class_counts_and_ignore_channel(cuda, c, ignore_channel, npix):
    """C = 16 is the last count whose 256 x 2C doubles fit the 64 KiB of LDS"""
    logits, labels = _pixels(npix, c)
    _check_loss(cuda, 'dice', logits, labels, what=f'npix={npix} C={c} ignore_channel={ignore_channel}',
                ignore_channel=ignore_channel)


def test_dice_refuses_seventeen_classes_and_says_why(cuda):
    from ever_amd import _C
    from ever_amd.module import loss as L
    logits, labels = _pixels(2049, 17)
    with pytest.raises(_C.HipKernelError, match=r'C=17 outside \[1,16\]'):
        L.dice_loss_with_logits(logits.to(cuda), labels.to(cuda))


@pytest.mark.parametrize('npix', CLASS_NPIX)
@pytest.mark.parametrize('c', [2, 64, 65, 150])
def test_cross_entropy_class_counts(cuda, c, npix):
    logits, labels = _pixels(npix, c)
    _check_loss(cuda, 'ce', logits, labels, what=f'npix={npix} C={c}')


@pytest.mark.parametrize('npix', CLASS_NPIX)
@pytest.mark.parametrize('c', [2, 64])
def test_tversky_class_counts(cuda, c, npix):
    """C = 64 fills the three per-thread arrays of prob_stats"""
    logits, labels = _pixels(npix, c)
    _check_tversky(cuda, logits, labels, f'npix={npix} C={c}')


def test_prob_stats_refuses_sixty_five_classes(cuda):
    from ever_amd import _C
    from ever_amd.hip import functional as HF
    logits, labels = _pixels(2049, 65)
    with pytest.raises(_C.HipKernelError, match=r'C=65 outside \[1,64\]'):
        HF.prob_stats(logits.to(cuda), labels.to(cuda), IGNORE)


@pytest.mark.parametrize('npix', CLASS_NPIX)
@pytest.mark.parametrize('c', [2, 150])
def test_cross_entropy_per_pixel_class_counts(cuda, c, npix):
    _check_ce_pixel(cuda, *_pixels(npix, c), f'npix={npix} C={c}')


# ================================================================================================ 4. label edges
@pytest.mark.parametrize('eps', [0.0, 0.1, 0.5])
def test_negative_ignore_index_and_label_smoothing_gradient(cuda, eps):
    """ignore_index = -1 (the default of label_smoothing_cross_entropy) with -1 among the labels; the smoothing term of
    the gradient against torch's label_smoothing="""
    from ever_amd.module import loss as L
    logits, labels = _pixels(2049, 5, ignore=-1)
    assert int((labels == -1).sum()) > 5
    _check_loss(cuda, 'ce', logits, labels, ignore=-1, what=f'ignore=-1 eps={eps}', eps=eps)
    xr = logits.double().requires_grad_()
    ref = TF.cross_entropy(xr, labels, ignore_index=-1, label_smoothing=eps)
    ref.backward()
    lg = logits.to(cuda).requires_grad_()
    out = L.label_smoothing_cross_entropy(lg, labels.to(cuda), eps=eps) if eps else \
        L.cross_entropy(lg, labels.to(cuda), ignore_index=-1)
    out.backward()
    _close(out, ref, RTOL_LOSS, f'module loss eps={eps}')
    _close(lg.grad, xr.grad, RTOL_GRAD, f'module gradient eps={eps}')


def test_dice_ignore_index_zero_is_also_a_class(cuda):
    logits, labels = _pixels(2049, 3, ignore=0)
    assert int((labels == 0).sum()) > 100
    _check_loss(cuda, 'dice', logits, labels, ignore=0, what='ignore_index=0')


def _same_nan_pattern(got, ref, what):
    got, ref = got.detach().cpu().double().reshape(-1), ref.detach().double().reshape(-1)
    assert torch.isnan(got).tolist() == torch.isnan(ref).tolist(), (what, got.tolist(), ref.tolist())
    ok = ~torch.isnan(ref)
    if bool(ok.any()):
        _close(got[ok], ref[ok], RTOL_LOSS, what)


@pytest.mark.parametrize('name', ['bce1', 'dice1', 'dice3', 'ce3', 'tversky1', 'tversky3'])
def test_all_pixels_ignored_equals_the_reference_on_an_empty_selection(cuda, name):
    """mean over nothing: NaN for BCE and CE, 0 for the ratio losses (smooth / smooth); every gradient exactly 0"""
    kind, c = name[:-1], int(name[-1])
    logits, _ = _pixels(2049, c)
    labels = torch.full(_nhw(2049), IGNORE)
    kw = TVERSKY if kind == 'tversky' else {}
    ref = _ref_loss(kind, logits.double(), labels, IGNORE, **kw)
    lg = logits.to(cuda).requires_grad_()
    out = _hip_loss(kind, lg, labels.to(cuda), IGNORE, **kw)
    out.backward()
    _same_nan_pattern(out, ref, f'all ignored {name}')
    assert not bool(lg.grad.cpu().ne(0).any()), f'all ignored {name}: non-zero (or NaN) gradient'


def test_all_pixels_ignored_cross_entropy_sum_is_zero(cuda):
    from ever_amd.hip import functional as HF
    logits, _ = _pixels(2049, 3)
    labels = torch.full(_nhw(2049), IGNORE)
    lg = logits.to(cuda).requires_grad_()
    out = HF.cross_entropy(lg, labels.to(cuda), ignore_index=IGNORE, reduction='sum')
    assert out.item() == 0.0
    assert TF.cross_entropy(logits.double(), labels, ignore_index=IGNORE, reduction='sum').item() == 0.0


def test_all_pixels_ignored_ohem_is_the_mean_of_nothing(cuda):
    from ever_amd.module import loss as L
    logits, _ = _pixels(2049, 3)
    labels = torch.full(_nhw(2049), IGNORE)
    lg = logits.to(cuda).requires_grad_()
    pix = L.cross_entropy_per_pixel(lg, labels.to(cuda), IGNORE)
    assert not bool(pix.detach().cpu().ne(0).any())
    out = L.online_hard_example_mining(pix, 0.5)
    out.backward()
    top = torch.zeros(2049).topk(1024).values
    _same_nan_pattern(out, top[top != 0].double().mean(), 'all ignored OHEM')
    assert not bool(lg.grad.cpu().ne(0).any())


def test_cross_entropy_per_pixel_is_zero_outside_the_classes(cuda):
    """ignored pixels and labels outside [0, C): loss and gradient exactly 0; the rest as torch"""
    from ever_amd.module import loss as L
    logits, labels = _pixels(2049, 3)
    labels = labels.clone().reshape(-1)
    labels[10:40:3], labels[41:70:4], labels[-9] = 300, -5, 3
    labels = labels.reshape(_nhw(2049))
    out_of_range = (labels < 0) | (labels >= 3)
    lg = logits.to(cuda).requires_grad_()
    pix = L.cross_entropy_per_pixel(lg, labels.to(cuda), IGNORE)
    pix.sum().backward()
    xr = logits.double().requires_grad_()
    ref = TF.cross_entropy(xr, torch.where(out_of_range, torch.full_like(labels, IGNORE), labels), ignore_index=IGNORE,
                           reduction='none')
    ref.sum().backward()
    assert not bool(pix.detach().cpu()[out_of_range].ne(0).any())
    assert not bool(lg.grad.cpu()[out_of_range.unsqueeze(1).expand_as(logits)].ne(0).any())
    _close(pix, ref, RTOL_LOSS, 'per-pixel CE')
    _close(lg.grad, xr.grad, RTOL_GRAD, 'per-pixel CE gradient')


# ================================================================================================ 5. range
@pytest.mark.parametrize('name', ['bce1', 'dice1', 'dice3', 'ce3', 'ce3_smoothed', 'softce3', 'tversky1', 'tversky3'])
def test_large_logits_stay_finite_and_accurate(cuda, name):
    """logits from {-80, -20, 0, 20, 80} mixed with randn: exp(160) inside a naive softmax is inf in fp32"""
    kind, c = name.split('_')[0][:-1], int(name.split('_')[0][-1])
    logits = _range_logits(2049, c, seed=9 + c)
    _, labels = _pixels(2049, c)
    kw = dict(TVERSKY) if kind == 'tversky' else (dict(eps=0.1) if name.endswith('smoothed') else {})
    _check_loss(cuda, kind, logits, _soft_target(2049, c) if kind == 'softce' else labels, what='range', **kw)


@pytest.mark.parametrize('mode', list(FOCAL_MODES))
def test_large_logits_focal(cuda, mode):
    x = _range_logits(2049, 1, seed=3).reshape(-1)
    y = (torch.rand(2049, generator=torch.Generator().manual_seed(4)) > 0.6).float()
    _check_focal(cuda, mode, x, y, 'range')


def test_large_logits_cross_entropy_per_pixel(cuda):
    _check_ce_pixel(cuda, _range_logits(2049, 3, seed=12), _pixels(2049, 3)[1], 'range')


# ================================================================================================ 6. accumulate = 1
@pytest.mark.parametrize('name', ['bce1', 'dice1', 'dice3', 'ce3', 'prob_stats3'])
def test_backward_accumulate_adds_onto_the_prefill(cuda, name):
    """dlogits pre-filled with random values, accumulate = 1: bit for bit prefill + (the accumulate = 0 result), and
    ignored pixels (whose gradient is 0) keep the prefill."""
    from ever_amd import _C
    kind, c = name[:-1], int(name[-1])
    npix = 2049
    logits, labels = _pixels(npix, c)
    x, y = logits.to(cuda), labels.to(cuda)
    assert x.permute(0, 2, 3, 1).is_contiguous()
    gen = torch.Generator().manual_seed(17)
    scale = torch.tensor(0.7, device=cuda)
    loss = torch.empty((), device=cuda)
    st = _stream()
    if kind == 'bce':
        stats = _loss_stats(2, cuda)
        _C.call('evk_bce_fwd_ex', x.data_ptr(), y.data_ptr(), npix, IGNORE, 0.0, 1.0, 0, loss.data_ptr(), stats.data_ptr(), st)

        def bwd(d, acc):
            _C.call('evk_bce_bwd_ex', x.data_ptr(), y.data_ptr(), npix, IGNORE, 0.0, 1.0, 0, stats.data_ptr(),
                    scale.data_ptr(), d.data_ptr(), acc, st)
    elif kind == 'dice':
        stats = _loss_stats(2 * c, cuda)
        _C.call('evk_dice_stats', x.data_ptr(), y.data_ptr(), npix, c, IGNORE, stats.data_ptr(), st)

        def bwd(d, acc):
            _C.call('evk_dice_bwd', x.data_ptr(), y.data_ptr(), npix, c, IGNORE, stats.data_ptr(), 1.0, -1,
                    scale.data_ptr(), d.data_ptr(), acc, st)
    elif kind == 'ce':
        stats = _loss_stats(3, cuda)
        _C.call('evk_ce_fwd', x.data_ptr(), y.data_ptr(), npix, c, IGNORE, 0.1, loss.data_ptr(), stats.data_ptr(), st)

        def bwd(d, acc):
            _C.call('evk_ce_bwd', x.data_ptr(), y.data_ptr(), npix, c, IGNORE, 0.1, stats.data_ptr(), scale.data_ptr(),
                    d.data_ptr(), acc, st)
    else:
        gtp = torch.randn(c, generator=gen).to(cuda)
        gsp = torch.randn(c, generator=gen).to(cuda)

        def bwd(d, acc):
            _C.call('evk_prob_stats_bwd', x.data_ptr(), y.data_ptr(), npix, c, IGNORE, gtp.data_ptr(), gsp.data_ptr(),
                    d.data_ptr(), acc, st)
    plain = torch.full_like(x, float('nan'))
    bwd(plain, 0)
    prefill = torch.randn(x.shape, generator=gen).to(cuda).contiguous(memory_format=torch.channels_last)
    assert prefill.stride() == x.stride() or c == 1
    acc = prefill.clone()
    bwd(acc, 1)
    assert bool(torch.isfinite(plain).all()) and bool(plain.ne(0).any())
    assert torch.equal(acc, prefill + plain), f'{name}: max diff {(acc - (prefill + plain)).abs().max().item():.3e}'
    gone = (y == IGNORE).unsqueeze(1).expand_as(x)
    assert int(gone.sum()) >= 5 * c and torch.equal(acc[gone], prefill[gone])


# ================================================================================================ 7. OHEM
def _ohem_input(n, keep, seed):
    """A third zeros, two negatives and a -0.0, and — where the keep-th largest value is positive — a block of values tied
    exactly at the threshold, spread evenly over the array (so over different workgroups), of which `keep` admits only a
    part.  With keep beyond the number of positives (ratio 0.999) the keep-th value is 0 or below: no tie is admitted."""
    g = torch.Generator().manual_seed(seed)
    nzero = n // 3
    special = torch.tensor([-0.75, -2.5, -0.0]) if n >= 16 else torch.zeros(0)
    npos = n - nzero - special.numel()
    tie = 1.0
    if 2 <= keep < npos - 2:
        t_in = min(5, keep - 1)                   # ties inside the top `keep` ...
        t_out = min(4, npos - keep - 1)           # ... and tied values that must stay out
        above = 1.5 + 2.0 * torch.rand(keep - t_in, generator=g)
        ties = torch.full((t_in + t_out,), tie)
        below = 0.01 + 0.9 * torch.rand(npos - keep - t_out, generator=g)
    else:
        above, ties, below = 1.5 + 2.0 * torch.rand(npos, generator=g), torch.zeros(0), torch.zeros(0)
    x = torch.empty(n)
    where_ties = torch.linspace(0, n - 1, ties.numel()).round().long() if ties.numel() else torch.zeros(0, dtype=torch.long)
    assert where_ties.unique().numel() == ties.numel()
    rest = torch.ones(n, dtype=torch.bool)
    rest[where_ties] = False
    others = torch.cat([above, below, torch.zeros(nzero), special])
    x[where_ties] = ties
    x[rest] = others[torch.randperm(others.numel(), generator=g)]
    return x


def _ohem_reference(x, keep):
    top = x.topk(keep).values
    kept = top[top != 0]
    return kept.double().mean(), kept


def _check_ohem_gradient(x, grad, kept, what):
    """a valid selection: exactly the kept non-zero elements (any of the tied ones), equal weights summing to the
    upstream gradient 1, nothing below the threshold"""
    nz = grad != 0
    assert int(nz.sum()) == kept.numel(), f'{what}: {int(nz.sum())} non-zero gradients, {kept.numel()} kept non-zero values'
    if kept.numel() == 0:
        return
    assert grad[nz].unique().numel() == 1
    # each weight is fl32(1 / count): their fp64 sum is within one fp32 rounding, 2^-24, of 1
    assert abs(grad.double().sum().item() - 1.0) <= 2.0 ** -23, f'{what}: gradients sum to {grad.double().sum().item()!r}'
    assert x[nz].min().item() >= kept.min().item(), f'{what}: a kept value below the threshold'
    assert bool(nz[x > kept.min()].all()) and not bool(nz[x == 0].any())


OHEM_CASES = [(n, r) for n in (1024, 1025, 262144, 262145, 1048577) for r in (0.05, 0.5, 0.999) if int(r * n) >= 1]


@pytest.mark.parametrize('n,ratio', OHEM_CASES)
def test_ohem_value_gradient_and_second_backward(cuda, n, ratio):
    """Value against topk; the gradient is a valid selection in BOTH of two backward passes over one forward
    (retain_graph=True).  The passes agree bit for bit off the tied values; among values tied at the threshold in different
    workgroups, which ones are admitted is the order their atomics arrive in (arbitrary, as in torch.topk)."""
    from ever_amd.module import loss as L
    keep = int(ratio * n)
    x = _ohem_input(n, keep, seed=n % 997 + int(ratio * 1000))
    want, kept = _ohem_reference(x, keep)
    xg = x.to(cuda).requires_grad_()
    got = L.online_hard_example_mining(xg, ratio)
    _close(got, want, RTOL_LOSS, f'n={n} keep={keep} OHEM')
    grads = []
    for last in (False, True):
        xg.grad = None
        got.backward(retain_graph=not last)
        grads.append(xg.grad.cpu().clone())
        _check_ohem_gradient(x, grads[-1], kept, f'n={n} keep={keep} backward {len(grads)}')
    off_ties = x != kept.min() if kept.numel() else torch.ones(n, dtype=torch.bool)
    assert torch.equal(grads[0][off_ties], grads[1][off_ties])
    if 2 <= keep < int((x > 0).sum()) - 2:
        tied = int((x == kept.min()).sum())
        assert tied >= 2 and int((x > kept.min()).sum()) + tied > keep, 'the input has no partly admitted ties'
        assert (torch.nonzero(x == kept.min()).reshape(-1) // 256).unique().numel() >= 2


def test_ohem_single_value(cuda):
    """n = 1 with keep = 1 through the C ABI (the wrapper's ratio < 1 cannot ask for it)"""
    from ever_amd import _C
    x = torch.tensor([0.625], device=cuda)
    state = torch.empty((_C.load().evk_ohem_state_bytes(),), device=cuda, dtype=torch.uint8)
    loss, d = torch.empty((), device=cuda), torch.full((1,), float('nan'), device=cuda)
    _C.call('evk_ohem_fwd', x.data_ptr(), 1, 1, loss.data_ptr(), state.data_ptr(), _stream())
    _C.call('evk_ohem_bwd', x.data_ptr(), 1, state.data_ptr(), None, d.data_ptr(), _stream())
    assert loss.item() == 0.625 and d.tolist() == [1.0]


@pytest.mark.parametrize('n,ties_at,keep', [(1025, (300, 301, 302, 303), 12), (1048577, (0, 1048576), 9)])
def test_ohem_second_backward_is_bit_identical_with_partly_admitted_ties(cuda, n, ties_at, keep):
    """Values tied at the threshold of which `keep` admits only a part, placed where the order of admission is fixed:
    in neighbouring lanes of one wavefront (one atomic instruction), and in one thread's first and second grid-stride step
    (elements 0 and 4096 * 256).  The tie counter used to survive the first backward, so the second pass gave every tied
    value a zero gradient."""
    from ever_amd import _C
    g = torch.Generator().manual_seed(n % 997)
    x = 0.01 + 0.9 * torch.rand(n, generator=g)
    x[::3] = 0.0
    admitted = len(ties_at) // 2
    free = torch.nonzero(x).reshape(-1)
    free = free[~torch.isin(free, torch.tensor(ties_at))]
    x[free[torch.randperm(free.numel(), generator=g)[:keep - admitted]]] = 2.0 + torch.rand(keep - admitted, generator=g)
    x[list(ties_at)] = 1.0
    want, kept = _ohem_reference(x, keep)
    assert kept.numel() == keep and kept.min().item() == 1.0 and int((kept == 1.0).sum()) == admitted
    xg = x.to(cuda)
    state = torch.empty((_C.load().evk_ohem_state_bytes(),), device=cuda, dtype=torch.uint8)
    loss = torch.empty((), device=cuda)
    _C.call('evk_ohem_fwd', xg.data_ptr(), n, keep, loss.data_ptr(), state.data_ptr(), _stream())
    _close(loss, want, RTOL_LOSS, f'n={n} keep={keep} OHEM')
    grads = []
    for _ in range(2):
        d = torch.full((n,), float('nan'), device=cuda)
        _C.call('evk_ohem_bwd', xg.data_ptr(), n, state.data_ptr(), None, d.data_ptr(), _stream())
        grads.append(d.cpu())
    counts = [int((d != 0).sum()) for d in grads]
    print(f'n={n} keep={keep}: non-zero gradients per backward pass {counts}')
    assert counts == [keep, keep], f'non-zero gradients per backward pass {counts}, kept values {keep}'
    _check_ohem_gradient(x, grads[0], kept, 'first backward')
    assert torch.equal(grads[0], grads[1])


def test_ohem_second_backward_through_autograd(cuda):
    """the same through the wrapper: loss.backward(retain_graph=True) twice"""
    from ever_amd.module import loss as L
    x = torch.tensor([0.0, 3.0, 1.0, 1.0, 1.0, 0.5, 0.0, 0.25, 1.0, 0.125])
    want, kept = _ohem_reference(x, 3)      # 3.0 and two of the four 1.0
    xg = x.to(cuda).requires_grad_()
    got = L.online_hard_example_mining(xg, 0.3)
    _close(got, want, RTOL_LOSS, 'OHEM')
    got.backward(retain_graph=True)
    first = xg.grad.cpu().clone()
    xg.grad = None
    got.backward()
    _check_ohem_gradient(x, first, kept, 'first backward')
    assert torch.equal(first, xg.grad.cpu())


# ================================================================================================ 8. confusion matrix
def _bincount_cm(y_true, y_pred, c):
    yt, yp = y_true.reshape(-1).numpy(), y_pred.reshape(-1).numpy()
    ok = (yt >= 0) & (yt < c) & (yp >= 0) & (yp < c)
    return np.bincount(yt[ok] * c + yp[ok], minlength=c * c).reshape(c, c)


def _cm_labels(n, c, g):
    y = torch.randint(0, c, (n,), generator=g)
    y[torch.rand(n, generator=g) < 0.05] = 255
    y[torch.rand(n, generator=g) < 0.05] = -1
    y[:2], y[-2:] = 255, -1
    return y


@pytest.mark.parametrize('n', [1025, 262145])
@pytest.mark.parametrize('c', [2, 64, 65])
def test_confusion_matrix_from_predictions_is_exact(cuda, c, n):
    """C * C = 4096 is the last histogram kept in LDS, 65 the first on global atomics; labels 255 and -1 and predictions
    outside [0, C) are skipped; two updates add"""
    from ever_amd.metric import ConfusionMatrix
    g = torch.Generator().manual_seed(c * 7 + n % 997)
    total, cm = np.zeros((c, c), dtype=np.int64), ConfusionMatrix(c)
    for _ in range(2):
        yt = _cm_labels(n, c, g)
        yp = torch.randint(0, c, (n,), generator=g)
        yp[torch.rand(n, generator=g) < 0.05] = c
        yp[torch.rand(n, generator=g) < 0.05] = -3
        yp[-1], yp[0] = 1000, c - 1
        want = _bincount_cm(yt, yp, c)
        assert 0 < want.sum() < n
        batch = cm.forward(yt.to(cuda), yp.to(cuda))
        assert batch.toarray().astype(np.int64).tolist() == want.tolist()
        total += want
        assert cm.dense_cm.astype(np.int64).tolist() == total.tolist()


@pytest.mark.parametrize('n', [1025, 262145])
@pytest.mark.parametrize('cl,c', [(1, 2), (2, 2), (64, 64), (65, 65), (5, 9)])
def test_confusion_matrix_from_logits_is_exact_and_first_maximum_wins(cuda, cl, c, n):
    """threshold 0 for one channel, else argmax; the logits are multiples of 0.5 (many exact ties, whole pixels of equal
    logits among them): the first maximum wins, as in torch.argmax"""
    from ever_amd.metric import ConfusionMatrix
    g = torch.Generator().manual_seed(cl * 11 + c + n % 997)
    nn, h, w = _nhw(n)
    total, cm = np.zeros((c, c), dtype=np.int64), ConfusionMatrix(c)
    for _ in range(2):
        yt = _cm_labels(n, c, g)
        z = (torch.randn(nn, h, w, cl, generator=g) * 1.5).round() / 2
        z.reshape(-1, cl)[::17] = 0.5
        logits = z.permute(0, 3, 1, 2)
        pred = (logits[:, 0] > 0).long() if cl == 1 else logits.argmax(1)
        if cl > 1:
            rows = z.reshape(-1, cl)
            assert int((rows == rows.max(1, keepdim=True).values).sum(1).gt(1).sum()) > n // 20, 'no ties in the input'
            assert int(pred.reshape(-1)[::17].abs().sum()) == 0
        want = _bincount_cm(yt, pred, c)
        cm.forward_logits(yt.reshape(nn, h, w).to(cuda), logits.to(cuda))
        total += want
        assert cm.dense_cm.astype(np.int64).tolist() == total.tolist()
