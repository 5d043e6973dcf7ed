"""Whole-scene tiled inference on the fused gather and stitch kernels: `scene_inference` is `sliding_window_inference` with
each chunk's windows cut out (and normalised) by ONE `HF.augment_batch` launch, their scores added into the scene by one
`HF.stitch_add` launch per column strip, and the mean scores or the class map made by one `HF.stitch_finalize` pass;
`SceneStitcher` is the accumulating half alone, for rasters that are read from disk window by window.

On CPU tensors both evaluate the same arithmetic with torch ops (accumulate in box order, divide once, `argmax` / `>`), so
they run and are tested without a device; on the device every step is a HIP kernel (csrc/augment.hip, csrc/stitch.hip)."""
import numpy as np
import torch

from .sliding_window import sliding_window

__all__ = ['SceneStitcher', 'scene_inference']


def _as_boxes(boxes):
    b = np.asarray(boxes, dtype=np.int64)
    if b.ndim != 2 or b.shape[1] != 4 or b.shape[0] == 0:
        raise ValueError(f'boxes must be [M, 4] (xmin, ymin, xmax, ymax) with M >= 1, got shape {b.shape}')
    return b


class SceneStitcher:
    """The scene accumulator [num_classes, height, width] and its coverage plane [height, width], zeroed.  `add` takes window
    scores at arbitrary boxes of one size; `scores` gives their mean over the covering windows, `labels` the class map.
    channels_last: the accumulator (and `scores()`) in NHWC memory, the layout the HIP models write; else contiguous."""

    def __init__(self, num_classes, height, width, device, channels_last=True):
        for name, v in (('num_classes', num_classes), ('height', height), ('width', width)):
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v <= 0:
                raise ValueError(f'SceneStitcher: {name} must be a positive integer, got {v!r}')
        self.num_classes, self.height, self.width = int(num_classes), int(height), int(width)
        self.device = torch.device(device)
        self.channels_last = bool(channels_last)
        if self.channels_last:
            self.acc = torch.zeros((self.height, self.width, self.num_classes), device=self.device).permute(2, 0, 1)
        else:
            self.acc = torch.zeros((self.num_classes, self.height, self.width), device=self.device)
        self.count = torch.zeros((self.height, self.width), device=self.device)

    def reset(self):
        self.acc.zero_()
        self.count.zero_()

    @torch.no_grad()
    def add(self, scores, boxes):
        """scores [M, num_classes, h, w] fp32 on the stitcher's device, boxes [M, 4] = (xmin, ymin, xmax, ymax), each h x w and
        inside the scene.  Windows are added in the order given (on the device: one launch per run of boxes with equal xmin)."""
        boxes = _as_boxes(boxes)
        if scores.dim() != 4 or scores.shape[0] != len(boxes) or scores.shape[1] != self.num_classes:
            raise ValueError(f'SceneStitcher.add: scores {tuple(scores.shape)} for {len(boxes)} boxes and {self.num_classes} classes')
        if scores.dtype != torch.float32 or scores.device != self.device:
            raise ValueError(f'SceneStitcher.add: fp32 scores on {self.device} required, got {scores.dtype} on {scores.device}')
        h, w = int(scores.shape[2]), int(scores.shape[3])
        if ((boxes[:, 2] - boxes[:, 0] != w) | (boxes[:, 3] - boxes[:, 1] != h)).any():
            raise ValueError(f'SceneStitcher.add: every box must have the scores\' size {h} x {w}')
        if (boxes[:, :2] < 0).any() or (boxes[:, 2] > self.width).any() or (boxes[:, 3] > self.height).any():
            raise ValueError(f'SceneStitcher.add: a box is not inside the {self.height} x {self.width} scene')
        if self.device.type != 'cuda':
            for s, (x0, y0, x1, y1) in zip(scores, boxes):
                self.acc[:, y0:y1, x0:x1] += s
                self.count[y0:y1, x0:x1] += 1
            return
        from ...hip import functional as HF
        i = 0
        while i < len(boxes):
            j = i + 1
            while j < len(boxes) and boxes[j, 0] == boxes[i, 0]:
                j += 1
            HF.stitch_add(self.acc, self.count, scores[i:j], [(int(b[1]), int(b[0])) for b in boxes[i:j]])
            i = j

    @torch.no_grad()
    def scores(self, out=None):
        """[num_classes, height, width]: accumulator / coverage (NaN where nothing was added).  out: None (a new tensor in
        the accumulator's layout), a tensor of its shape and strides, or `self.acc` for in place."""
        if self.device.type != 'cuda':
            if out is None:
                return self.acc / self.count
            return torch.div(self.acc, self.count, out=out)
        from ...hip import functional as HF
        return HF.stitch_finalize(self.acc, self.count, 'scores', out=out)

    @torch.no_grad()
    def labels(self, dtype=torch.uint8, threshold=None, fill_label=255):
        """[height, width] of `dtype` (uint8 or int64): the first maximal mean score's class (two classes or more), or
        `mean score > threshold` (one class, which needs a threshold); `fill_label` where nothing was added."""
        if dtype not in (torch.uint8, torch.int64):
            raise ValueError(f'SceneStitcher.labels: uint8 or int64 labels, got {dtype}')
        if (self.num_classes == 1) != (threshold is not None):
            raise ValueError(f'SceneStitcher.labels: {self.num_classes} class(es) with threshold={threshold} (one class needs a '
                             f'threshold, more take the argmax)')
        if dtype == torch.uint8 and (self.num_classes > 256 or not 0 <= int(fill_label) <= 255):
            raise ValueError(f'SceneStitcher.labels: {self.num_classes} classes / fill_label {fill_label} do not fit uint8')
        if self.device.type != 'cuda':
            q = self.acc / self.count
            lab = (q[0] > threshold) if self.num_classes == 1 else q.argmax(dim=0)
            lab = lab.to(dtype)
            lab[self.count == 0] = fill_label
            return lab
        from ...hip import functional as HF
        return HF.stitch_finalize(self.acc, self.count, 'labels', label_dtype=dtype, threshold=threshold, fill_label=fill_label)


def _cpu_image(scene, raster, mean, std):
    """the logical [N, C, H, W] fp32 image of a CPU scene"""
    if not raster:
        return scene
    x = (scene if scene.dim() == 4 else scene[None]).to(torch.float32)
    if mean is not None:
        x = x.sub(torch.tensor([float(v) for v in mean], dtype=torch.float32)).div(
            torch.tensor([float(v) for v in std], dtype=torch.float32))
    return x.permute(0, 3, 1, 2)


@torch.no_grad()
def scene_inference(model, scene, kernel_size, stride, batch_size=8, activation=None, *, mean=None, std=None,
                    output='scores', label_dtype=torch.uint8, threshold=None):
    """`sliding_window_inference(model, scene, kernel_size, stride, batch_size, activation)` for whole scenes: the same boxes
    in the same order, the same sums and one division, so the scores have the same bits wherever the model's have.

    scene: a logical [N, C, H, W] fp32 tensor (brought to NHWC once if it is not there already), or an [H, W, C] /
    [N, H, W, C] raster, uint8 or fp32, normalised on the way in as `(float(v) - mean) / std` when `mean` / `std` are given (a
    uint8 scene, a 3-D scene and a scene with mean / std are rasters).  model: eval mode, [B, C, h, w] tiles ->
    [B, classes, h, w] scores (output stride 1).  output: 'scores' -> [N, classes, H, W] fp32; 'labels' -> [N, H, W] of
    `label_dtype`: argmax of the mean scores (255 where nothing was added), or `> threshold` for one class, without the
    normalised scores ever being stored."""
    if output not in ('scores', 'labels'):
        raise ValueError(f'scene_inference: output must be \'scores\' or \'labels\', got {output!r}')
    if (mean is None) != (std is None):
        raise ValueError('scene_inference: mean and std come together or not at all')
    if scene.dim() not in (3, 4):
        raise ValueError(f'scene_inference: a 3-D raster or a 4-D scene is required, got {tuple(scene.shape)}')
    raster = scene.dim() == 3 or scene.dtype == torch.uint8 or mean is not None
    if scene.dtype not in (torch.uint8, torch.float32) or (not raster and scene.dtype != torch.float32):
        raise ValueError(f'scene_inference: a uint8 or fp32 scene is required, got {scene.dtype}')
    on_device = scene.is_cuda
    if on_device:
        from ...hip import functional as HF
        if raster:
            rasters = scene if scene.dim() == 4 else scene[None]
        else:
            rasters = scene.permute(0, 2, 3, 1)
        rasters = rasters if rasters.is_contiguous() else rasters.contiguous()      # [N, H, W, C]
        n, ih, iw, _ = rasters.shape
    else:
        image = _cpu_image(scene, raster, mean, std)
        n, _, ih, iw = image.shape
    boxes = np.unique(sliding_window((ih, iw), kernel_size, stride), axis=0)
    kh, kw = int(boxes[0, 3] - boxes[0, 1]), int(boxes[0, 2] - boxes[0, 0])
    st = out = None
    for b in range(n):
        for i in range(0, len(boxes), batch_size):
            chunk = boxes[i:i + batch_size]
            if on_device:
                # each window from its own row slab: the gather kernel's 2^31-element limit then holds per slab, not per scene
                tiles, _ = HF.augment_batch([rasters[b, y0:y1] for _, y0, _, y1 in chunk], None, [0] * len(chunk),
                                            [(0, int(x0)) for x0, _, _, _ in chunk], (kh, kw), (kh, kw), mean, std,
                                            channels_last=True)
            else:
                tiles = torch.stack([image[b, :, y0:y1, x0:x1] for x0, y0, x1, y1 in chunk])
            scores = model(tiles)
            if activation is not None:
                scores = activation(scores)
            if scores.dim() != 4 or scores.shape[0] != len(chunk) or tuple(scores.shape[2:]) != (kh, kw):
                raise ValueError(f'scene_inference: the model gave {tuple(scores.shape)} for {len(chunk)} tiles of {kh} x {kw} '
                                 f'(models whose output stride is not 1 are not supported)')
            if st is None:
                cl = on_device and scores.permute(0, 2, 3, 1).is_contiguous()
                st = SceneStitcher(int(scores.shape[1]), ih, iw, scores.device, channels_last=cl)
                if output == 'labels':
                    out = torch.empty((n, ih, iw), device=scores.device, dtype=label_dtype)
                elif n > 1:
                    out = torch.empty((n, ih, iw, st.num_classes) if cl else (n, st.num_classes, ih, iw), device=scores.device)
                    out = out.permute(0, 3, 1, 2) if cl else out
            st.add(scores, chunk)
        if output == 'labels':
            if on_device:
                _labels_into(st, out[b], label_dtype, threshold)
            else:
                out[b] = st.labels(label_dtype, threshold)
        elif n > 1:
            st.scores(out=out[b])
        else:
            out = st.scores(out=st.acc)[None]        # one scene: in place, no second [C, H, W] tensor
        if b + 1 < n:
            st.reset()
    return out


def _labels_into(st, dst, dtype, threshold):
    from ...hip import functional as HF
    if (st.num_classes == 1) != (threshold is not None):
        raise ValueError(f'scene_inference: {st.num_classes} class(es) with threshold={threshold} (one class needs a threshold, '
                         f'more take the argmax)')
    return HF.stitch_finalize(st.acc, st.count, 'labels', out=dst, label_dtype=dtype, threshold=threshold)
