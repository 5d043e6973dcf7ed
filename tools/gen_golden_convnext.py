"""Fixtures of the ConvNeXt tests from the reference implementation.  Development machine only: needs the reference tree.

    python tools/gen_golden_convnext.py /path/to/reference

The reference's dinov3/models/convnext.py is loaded BY FILE PATH (it needs torch and numpy only; the package import would
pull in the transformer), filled with the hash-generated weights of tests/convnext_common.py and run on the CPU.  Writes
  tests/golden/convnext_keys.json  state-dict key order and shapes of convnext_{tiny,small,base,large}: names and numbers
  tests/golden/convnext_ref.npz    per reduced case ('sq' 2x3x64x64, 'odd' 2x3x72x56): the four get_intermediate_layers maps,
                                   the forward_features tensors, the input gradient of the fixed linear functional,
                                   oracle.gen_golden.grad_digest of every parameter and four full gradients."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import grad_digest  # noqa: E402
from tests import convnext_common as cc  # noqa: E402


def load_reference(ref_root):
    path = os.path.join(ref_root, 'ever', 'module', 'dinov3', 'models', 'convnext.py')
    spec = importlib.util.spec_from_file_location('reference_convnext', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(ref_root):
    ref = load_reference(ref_root)
    golden = os.path.join(ROOT, 'tests', 'golden')
    keys = {}
    for size in cc.SIZES:
        sd = ref.get_convnext_arch('convnext_' + size)().state_dict()
        keys['convnext_' + size] = [[k, list(v.shape)] for k, v in sd.items()]
    with open(os.path.join(golden, 'convnext_keys.json'), 'w') as f:
        json.dump(keys, f, separators=(',', ':'))
    out = {}
    for case in cc.CASES:
        torch.manual_seed(0)
        model = cc.load_filled(ref.ConvNeXt(**cc.REDUCED)).train()
        outs, dx = cc.run_case(model, case, cc.case_input(case))
        for k, v in outs.items():
            out[f'{case}/{k}'] = v.contiguous().numpy().astype(np.float32)
        out[f'{case}/dx'] = dx.numpy().astype(np.float32)
        named = cc.named_grads(model)
        digest = grad_digest(named)
        out[f'{case}/digest'] = np.array([digest[k] for k, _ in named], dtype=np.float64)
        grads = dict(named)
        for k in cc.FULL_GRADS:
            out[f'{case}/grad/{k}'] = grads[k].grad.numpy().astype(np.float32)
    out['param_names'] = np.array([k for k, _ in named])
    np.savez_compressed(os.path.join(golden, 'convnext_ref.npz'), **out)
    for fn in ('convnext_keys.json', 'convnext_ref.npz'):
        print(fn, os.path.getsize(os.path.join(golden, fn)), 'bytes')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
