"""What the ViT fixture generator (tools/gen_golden_vit.py) and the tests that read its fixtures share: the reduced models,
their hash-generated weights and inputs (oracle/portable.py), and the fixed linear functional whose gradients are stored."""
import numpy as np
import torch

from oracle import portable

# layerscale_init = 1 and scales in [0.5, 1.5]: with the released 1e-5 the blocks would vanish from the output
_COMMON = dict(depth=2, num_heads=2, n_storage_tokens=4, mask_k_bias=True, layerscale_init=1.0, norm_layer='layernormbf16',
               pos_embed_rope_dtype='fp32', untie_global_and_local_cls_norm=True)
MODELS = {'d32': dict(_COMMON, embed_dim=64), 'd64': dict(_COMMON, embed_dim=128)}
# 'odd': a 3 x 5 grid (only H != W shows a swapped RoPE axis); 'long': 9 x 8 + 5 = 77 tokens, past one key tile
CASES = {'sq': (2, 3, 64, 64), 'odd': (2, 3, 48, 80), 'long': (1, 3, 144, 128)}
RUNS = (('d32', 'sq'), ('d32', 'odd'), ('d32', 'long'), ('d64', 'odd'))
FULL_GRADS = ('cls_token', 'blocks.0.attn.qkv.bias', 'blocks.1.ls1.gamma', 'blocks.0.attn.proj.weight')
SIZES = ('vit_small', 'vit_base', 'vit_large', 'vitl16_sat493m')
ROPE_TABLES = {        # name -> (constructor arguments, training mode, seed, (H, W))
    'eval_3x5': (dict(embed_dim=64, num_heads=2, dtype=torch.float32), False, None, (3, 5)),
    'eval_d64_9x8': (dict(embed_dim=128, num_heads=2, dtype=torch.float32), False, None, (9, 8)),
    'train_rescale2_3x5': (dict(embed_dim=64, num_heads=2, rescale_coords=2, dtype=torch.float32), True, 11, (3, 5)),
    'train_all_4x7': (dict(embed_dim=128, num_heads=2, rescale_coords=2, shift_coords=0.25, jitter_coords=1.5,
                           normalize_coords='max', dtype=torch.float32), True, 12, (4, 7)),
}


def fill_vit(state_dict, tag):
    """{name: array}: matrices He-uniform on their fan-in, norm weights and layer scales in [0.5, 1.5], the bias mask ones /
    zeros / ones over the q / k / v thirds (the released checkpoints'), the RoPE periods as constructed, every other vector
    (biases, tokens) in [-0.2, 0.2] — each entry keyed by its name"""
    out = {}
    for name, t in state_dict.items():
        shape = tuple(t.shape)
        key = f'vit/{tag}/{name}'
        if name.endswith('bias_mask'):
            third = shape[0] // 3
            out[name] = np.concatenate([np.ones(third), np.zeros(third), np.ones(third)]).astype(np.float32)
        elif name == 'rope_embed.periods':
            out[name] = t.detach().cpu().numpy().copy()
        elif name.endswith('.weight') and len(shape) >= 2:
            b = float(np.sqrt(6.0 / int(np.prod(shape[1:]))))
            out[name] = portable.uniform(key, shape, -b, b)
        elif name.endswith('.weight') or name.endswith('gamma'):
            out[name] = portable.uniform(key, shape, 0.5, 1.5)
        else:
            out[name] = portable.uniform(key, shape, -0.2, 0.2)
    return out


def load_filled(model, tag):
    filled = fill_vit(model.state_dict(), tag)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v).copy()) for k, v in filled.items()}, strict=True)
    return model


def case_input(case):
    return torch.from_numpy(portable.normalish(f'vit/{case}/x', CASES[case]))


def run_case(model, tag, case, x):
    """forward_features and get_intermediate_layers on x and the fixed linear functional of their outputs, differentiated.
    Returns ({name: output tensor}, input gradient); parameter gradients are left on the model."""
    x = x.detach().clone().requires_grad_(True)
    model.zero_grad(set_to_none=True)
    feats = model.forward_features(x)
    layers = model.get_intermediate_layers(x, n=[0, 1], reshape=True, return_class_token=True, return_extra_tokens=True)
    outs = dict(cls=feats['x_norm_clstoken'], storage=feats['x_storage_tokens'], patch=feats['x_norm_patchtokens'],
                prenorm=feats['x_prenorm'])
    for i, (m, c, e) in enumerate(layers):
        outs.update({f'map{i}': m, f'cls{i}': c, f'extra{i}': e})
    loss = 0.0
    for k, v in outs.items():
        w = torch.from_numpy(portable.uniform(f'vit/{tag}/{case}/w/{k}', tuple(v.shape))).to(v.device)
        loss = loss + (v * w).sum()
    loss.backward()
    return {k: v.detach() for k, v in outs.items()}, x.grad.detach()


def named_grads(model):
    """(name, parameter) of every parameter that takes a gradient in run_case, in state-dict order (local_cls_norm is only
    used on the second crop list in training mode)"""
    return [(k, p) for k, p in model.named_parameters() if not k.startswith('local_cls_norm.')]


def rope_table(cls, name):
    """(sin, cos) of ROPE_TABLES[name] from a RopePositionEmbedding class, on the CPU"""
    kwargs, training, seed, (h, w) = ROPE_TABLES[name]
    m = cls(**kwargs).train(training)
    if seed is not None:
        torch.manual_seed(seed)
    return m(H=h, W=w)
