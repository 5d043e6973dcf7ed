"""What the preprocessing tests share with tools/gen_golden_preprocess.py: the sources of the fixture
tests/golden/preprocess_ref.npz, the list of per-image cases and the batch pipelines, each written against a namespace `pp`
with `function`, `thcomm` and `thsegm` modules — the reference's when the fixture is written, this package's when it is
checked — so both sides run the same calls under the same `np.random.seed`; and the CPU evaluation of evk_augment_batch's
semantics (include/ever_hip.h) that the GPU tests compare with."""
import os
import types

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'preprocess_ref.npz')
MEAN3, STD3 = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
MEAN4, STD4 = (123.675, 116.28, 103.53, 110.0), (58.395, 57.12, 57.375, 60.5)
LABELS = np.array([0, 1, 2, 3, 4, 5, 255])

# (height, width) of the sources; every one exists with 3 and with 4 channels, a uint8 and an int64 mask
SOURCE_SIZES = ((13, 21), (37, 33), (21, 13), (40, 40), (33, 37))


def make_sources():
    """{'img3_i', 'img4_i': uint8 [H, W, C]; 'mask_i': uint8 [H, W] of labels 0..5 and 255} from a private generator"""
    rng = np.random.RandomState(20240)
    out = {}
    for i, (h, w) in enumerate(SOURCE_SIZES):
        out[f'img3_{i}'] = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        out[f'img4_{i}'] = rng.randint(0, 256, (h, w, 4)).astype(np.uint8)
        out[f'mask_{i}'] = LABELS[rng.randint(0, len(LABELS), (h, w))].astype(np.uint8)
    return out


def namespace(function, thcomm, thsegm):
    return types.SimpleNamespace(function=function, thcomm=thcomm, thsegm=thsegm)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def per_image_cases(pp, src):
    """name -> thunk.  A thunk seeds np.random itself and returns whatever the call returns (tensor, tuple, tuple with None)."""
    S, C, F = pp.thsegm, pp.thcomm, pp.function
    img, mask = _t(src['img3_0']), _t(src['mask_0'])
    big, bigmask = _t(src['img3_1']), _t(src['mask_1'])
    fimg, fmask = img.float(), mask.float()
    chw = img.permute(2, 0, 1).contiguous()
    cases = {}

    def add(name, seed, fn):
        def thunk():
            np.random.seed(seed)
            return fn()
        cases[name] = thunk

    for seed in range(6):
        add(f'rot90k_s{seed}', seed, lambda: S.THRandomRotate90k()(img, mask))
        add(f'hflip_s{seed}', seed, lambda: S.THRandomHorizontalFlip()(img, mask))
        add(f'vflip_s{seed}', seed, lambda: S.THRandomVerticalFlip()(img, mask))
    add('rot90k_nomask', 1, lambda: S.THRandomRotate90k()(img))
    add('rot90k_fixed3', 0, lambda: S.THRandomRotate90k(3)(img, mask))
    add('hflip_nomask', 3, lambda: S.THRandomHorizontalFlip(0.9)(img))
    add('vflip_nomask', 3, lambda: S.THRandomVerticalFlip(0.9)(img))
    for seed in (0, 5):
        add(f'crop_s{seed}', seed, lambda: S.THRandomCrop((9, 10))(big, bigmask))
        add(f'crop_pad_rows_s{seed}', seed, lambda: S.THRandomCrop((16, 16))(img, mask))          # 13 < 16 rows, 21 >= 16 columns
        add(f'crop_pad_cols_s{seed}', seed, lambda: S.THRandomCrop((12, 40))(big, bigmask))       # 37 >= 12 rows, 33 < 40 columns
    add('crop_nomask', 2, lambda: S.THRandomCrop((9, 10))(big))
    add('scale', 4, lambda: S.THRandomScale()(fimg, fmask))
    add('scale_nomask', 9, lambda: S.THRandomScale((0.5, 1.5), 0.5)(fimg))
    add('channel_first', 0, lambda: C.THChannelFirst()(big))
    add('channel_first2', 0, lambda: C.THChannelFirst2()(big, bigmask))
    add('normalize', 0, lambda: C.THMeanStdNormalize()(chw))
    add('normalize2', 0, lambda: C.THMeanStdNormalize2((1.5, 2.5, 3.5), (0.3, 0.7, 1.1))(chw, mask))
    add('divisible_pad', 0, lambda: C.THDivisiblePad(32, 7)(chw.float(), mask))
    add('divisible_pad_nomask', 0, lambda: C.THDivisiblePad(8)(chw.float()))
    add('divisible_pad_to_size', 0, lambda: C.THDivisiblePad(8, 255, (40, 48))(chw.float(), mask))
    add('fn_normalize_4d', 0, lambda: F.th_mean_std_normalize(chw.float()[None]))
    add('fn_divisible_pad_2d', 0, lambda: F.th_divisible_pad(mask, 16, value=9))
    add('fn_divisible_pad_4d', 0, lambda: F.th_divisible_pad(chw.float()[None], 16))
    add('fn_pad_to_size_3d', 0, lambda: F.th_pad_to_size(chw, (14, 30), value=3))
    add('pipeline_funcwrapper', 0, lambda: C.Pipeline(C.FuncWrapper(lambda a, b: (a + 1, b)), C.THChannelFirst2())(big, bigmask))
    return cases


# name -> (channels, crop, size divisor, mean, std, mask_pad_value, int64 masks, seed)
BATCHES = {
    'batch_pad_ring': (3, (16, 16), 32, MEAN3, STD3, 255, False, 7),
    'batch_crop_past_source': (3, (40, 24), 32, MEAN3, STD3, 255, False, 11),     # 40 rows > 13, 21, 33, 37; 24 columns > 13, 21
    'batch_c4_int64': (4, (12, 20), 16, MEAN4, STD4, 7, True, 3),
}


def batch_inputs(src, name, device='cpu'):
    c, _, _, _, _, _, wide, _ = BATCHES[name]
    images = [_t(src[f'img{c}_{i}']).to(device) for i in range(len(SOURCE_SIZES))]
    masks = [_t(src[f'mask_{i}']) for i in range(len(SOURCE_SIZES))]
    return images, [(m.long() if wide else m).to(device) for m in masks]


def run_batch_per_image(pp, src, name):
    """the chain the fused pass replaces, from the per-image classes of `pp`, image by image, then torch.stack"""
    c, crop, div, mean, std, pad, _, seed = BATCHES[name]
    S, C = pp.thsegm, pp.thcomm
    pipe = C.Pipeline(S.THRandomRotate90k(), S.THRandomHorizontalFlip(), S.THRandomVerticalFlip(), S.THRandomCrop(crop),
                      C.THChannelFirst2(), C.THMeanStdNormalize2(mean, std), C.THDivisiblePad(div, pad))
    images, masks = batch_inputs(src, name)
    np.random.seed(seed)
    outs = [pipe(im, m) for im, m in zip(images, masks)]
    return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])


def flatten(result):
    """(arity, [arrays]) of what a case returned: arity 0 for a bare tensor, else the tuple length; None entries are dropped
    from the arrays and recorded as -1 in `kinds`"""
    items = result if isinstance(result, tuple) else (result,)
    kinds = [-1 if it is None else 1 for it in items]
    arrays = [np.ascontiguousarray(it.numpy()) for it in items if it is not None]
    return (len(items) if isinstance(result, tuple) else 0), kinds, arrays


# ------------------------------------------------------------------------------------------------ evk_augment_batch on the CPU
def d4_hw(x, op):
    """op = swap | flip_rows << 1 | flip_cols << 2 (transpose first, then flip) on the first two axes of [H, W, ...]"""
    y = x.transpose(0, 1) if op & 1 else x
    dims = [d for d, bit in ((0, 2), (1, 4)) if op & bit]
    return torch.flip(y, dims) if dims else y


def augment_ref(images, masks, ops, origins, crop, out_size, mean, std, mask_pad_value, out_mask_dtype=None):
    """the semantics of evk_augment_batch in torch ops on the CPU: ([N, C, Ho, Wo] fp32, [N, Ho, Wo] labels or None)"""
    ch, cw = crop
    ho, wo = out_size
    outs, mouts = [], []
    for i, im in enumerate(images):
        t = d4_hw(im.cpu(), ops[i])
        y0, x0 = origins[i]
        win = torch.zeros((ch, cw, t.shape[2]), dtype=t.dtype)
        part = t[y0:y0 + ch, x0:x0 + cw]
        win[:part.shape[0], :part.shape[1]] = part
        v = win.permute(2, 0, 1).float()
        if mean is not None:
            v = v.sub(torch.tensor(mean, dtype=torch.float32).view(-1, 1, 1)).div(torch.tensor(std, dtype=torch.float32).view(-1, 1, 1))
        out = torch.zeros((t.shape[2], ho, wo), dtype=torch.float32)
        out[:, :ch, :cw] = v
        outs.append(out)
        if masks is not None:
            mt = d4_hw(masks[i].cpu(), ops[i])
            mwin = torch.zeros((ch, cw), dtype=mt.dtype)
            mpart = mt[y0:y0 + ch, x0:x0 + cw]
            mwin[:mpart.shape[0], :mpart.shape[1]] = mpart
            mout = torch.full((ho, wo), mask_pad_value, dtype=out_mask_dtype or mt.dtype)
            mout[:ch, :cw] = mwin.to(mout.dtype)
            mouts.append(mout)
    return torch.stack(outs), (torch.stack(mouts) if masks is not None else None)
