"""TEST INFRASTRUCTURE ONLY — writes tests/golden/tta_ref.npz from the imported reference.

Runs where the reference tree is available (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_tta.py

Imports the reference through oracle.gen_golden.import_reference() and runs ITS `tta` and `MultiTransform` on the CPU, on one
2 x 3 x 12 x 20 input, with the toy model and the three transform sets of tests/tta_common.py (the eight symmetries of the
square, seven of them without Transpose, a set with two `Scale`s).  Writes data only: the input, the transformed input of every distinct
transform and the three results."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402
from tests import tta_common  # noqa: E402


def main():
    ever = import_reference()
    from ever.magic.transform import segm, tta
    torch.manual_seed(20)
    x = torch.randn(*tta_common.FIXTURE_SHAPE)
    out = {'input': x.numpy()}
    for name, cfg in tta_common.fixture_sets(segm, ever.Transform).items():
        for t, im in zip(cfg, ever.MultiTransform(*cfg).transform(x)):
            if type(t).__name__ != 'Identity':      # (the input itself)
                out['in_' + tta_common.transform_label(t)] = np.ascontiguousarray(im.numpy())
        out[name] = tta.tta(tta_common.toy_model, x, cfg).numpy()
    path = tta_common.GOLDEN
    np.savez_compressed(path, **out)
    print(f'wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays')


if __name__ == '__main__':
    main()
