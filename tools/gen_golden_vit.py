"""Fixtures of the ViT tests from the reference implementation.  Development machine only: needs the reference tree.

    python tools/gen_golden_vit.py

The reference package is imported through oracle.gen_golden.import_reference() (its vision_transformer.py imports `ever`
itself, which needs the wandb / prettytable / albumentations stubs), filled with the hash-generated weights of
tests/vit_common.py and run on the CPU.  Writes
  tests/golden/vit_keys.json  state-dict key order and shapes of vit_small, vit_base, vit_large, vitl16_sat493m: names and numbers
  tests/golden/vit_ref.npz    per run of tests/vit_common.py RUNS (reduced model, case): the forward_features tensors, the
                              get_intermediate_layers(n=[0, 1], reshape, class token, extra tokens) outputs, the input gradient of
                              the fixed linear functional, oracle.gen_golden.grad_digest of every parameter and four full
                              gradients; and the RoPE tables of ROPE_TABLES (eval mode, and training mode under a fixed seed)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import grad_digest, import_reference  # noqa: E402
from tests import vit_common as vc  # noqa: E402


def main():
    import_reference()
    from ever.module.dinov3.layers import RopePositionEmbedding
    from ever.module.dinov3.models import vision_transformer as ref
    golden = os.path.join(ROOT, 'tests', 'golden')
    keys = {}
    for size in vc.SIZES:
        with torch.device('meta'):
            sd = getattr(ref, size)().state_dict()
        keys[size] = [[k, list(v.shape)] for k, v in sd.items()]
    with open(os.path.join(golden, 'vit_keys.json'), 'w') as f:
        json.dump(keys, f, separators=(',', ':'))
    out = {}
    for tag, case in vc.RUNS:
        torch.manual_seed(0)
        model = vc.load_filled(ref.DinoVisionTransformer(**vc.MODELS[tag]), tag).train()
        outs, dx = vc.run_case(model, tag, case, vc.case_input(case))
        pre = f'{tag}/{case}'
        for k, v in outs.items():
            out[f'{pre}/{k}'] = v.contiguous().numpy().astype(np.float32)
        out[f'{pre}/dx'] = dx.numpy().astype(np.float32)
        named = vc.named_grads(model)
        digest = grad_digest(named)
        out[f'{pre}/digest'] = np.array([digest[k] for k, _ in named], dtype=np.float64)
        grads = dict(named)
        for k in vc.FULL_GRADS:
            out[f'{pre}/grad/{k}'] = grads[k].grad.numpy().astype(np.float32)
        out[f'{tag}/param_names'] = np.array([k for k, _ in named])
    for name in vc.ROPE_TABLES:
        sin, cos = vc.rope_table(RopePositionEmbedding, name)
        out[f'rope/{name}/sin'], out[f'rope/{name}/cos'] = sin.numpy(), cos.numpy()
    np.savez_compressed(os.path.join(golden, 'vit_ref.npz'), **out)
    for fn in ('vit_keys.json', 'vit_ref.npz'):
        print(fn, os.path.getsize(os.path.join(golden, fn)), 'bytes')


if __name__ == '__main__':
    main()
