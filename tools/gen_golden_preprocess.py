"""TEST INFRASTRUCTURE ONLY — writes tests/golden/preprocess_ref.npz from the imported reference.

Runs where the reference tree is available (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_preprocess.py

Imports the reference through oracle.gen_golden.import_reference() and runs ITS `ever.preprocess` classes and functions on the
CPU under fixed `np.random.seed`s: the per-image cases and the three batch pipelines of tests/preprocess_common.py (rotate,
flips, crop, channel-first, normalise, divisible pad, image by image, then torch.stack).  Writes data only: the sources and
masks, and per case the tuple arity, which entries are None, and the result arrays."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import import_reference  # noqa: E402
from tests import preprocess_common as pc  # noqa: E402


def main():
    import_reference()
    import ever.preprocess.function as function
    import ever.preprocess.thcomm as thcomm
    import ever.preprocess.thsegm as thsegm
    pp = pc.namespace(function, thcomm, thsegm)
    src = pc.make_sources()
    out = dict(src)
    for name, thunk in pc.per_image_cases(pp, src).items():
        arity, kinds, arrays = pc.flatten(thunk())
        out[f'{name}/arity'] = np.array(arity)
        out[f'{name}/kinds'] = np.array(kinds)
        for j, a in enumerate(arrays):
            out[f'{name}/{j}'] = a
    for name in pc.BATCHES:
        image, mask = pc.run_batch_per_image(pp, src, name)
        out[f'{name}/image'], out[f'{name}/mask'] = image.numpy(), mask.numpy()
    np.savez_compressed(pc.GOLDEN, **out)
    print(f'wrote {pc.GOLDEN}: {os.path.getsize(pc.GOLDEN)} bytes, {len(out)} arrays')


if __name__ == '__main__':
    main()
