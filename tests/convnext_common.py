"""What the ConvNeXt fixture generator (tools/gen_golden_convnext.py) and the tests that read its fixtures share: the reduced
model, its hash-generated weights and inputs (oracle/portable.py), and the fixed linear functional whose gradients are stored."""
import numpy as np
import torch

from oracle import portable

REDUCED = dict(depths=[1, 1, 2, 1], dims=[8, 16, 32, 64], layer_scale_init_value=1.0)
CASES = {'sq': (2, 3, 64, 64), 'odd': (2, 3, 72, 56)}      # 'odd': maps 18x14, 9x7, 4x3, 2x1 — the 2x2/s2 layers drop a row and a column
FULL_GRADS = ('stages.0.0.gamma', 'stages.2.1.norm.weight', 'downsample_layers.1.0.weight', 'norm.bias')
SIZES = ('tiny', 'small', 'base', 'large')


def fill_convnext(state_dict):
    """{name: float32 array}: convolution and Linear weights He-uniform on their fan-in, LayerNorm weights and layer scales
    in [0.5, 1.5], biases in [-0.2, 0.2] — every entry keyed by its name (norms.3.* is norm.* registered twice: same values)"""
    out = {}
    for name, t in state_dict.items():
        shape = tuple(t.shape)
        key = 'convnext/' + name.replace('norms.3.', 'norm.')
        if len(shape) >= 2:
            b = float(np.sqrt(6.0 / int(np.prod(shape[1:]))))
            out[name] = portable.uniform(key, shape, -b, b)
        elif name.endswith('weight') or name.endswith('gamma'):
            out[name] = portable.uniform(key, shape, 0.5, 1.5)
        else:
            out[name] = portable.uniform(key, shape, -0.2, 0.2)
    return out


def load_filled(model):
    filled = fill_convnext(model.state_dict())
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in filled.items()}, strict=True)
    return model


def case_input(case):
    return torch.from_numpy(portable.normalish(f'convnext/{case}/x', CASES[case]))


def run_case(model, case, x):
    """Both forward forms on x and the fixed linear functional of their outputs, differentiated.  Returns
    ({name: output tensor}, input gradient); parameter gradients are left on the model."""
    x = x.detach().clone().requires_grad_(True)
    model.zero_grad(set_to_none=True)
    maps = model.get_intermediate_layers(x, n=[0, 1, 2, 3], reshape=True, norm=True)
    feats = model.forward_features(x)
    outs = {f'map{i}': m for i, m in enumerate(maps)}
    outs.update(cls=feats['x_norm_clstoken'], patch=feats['x_norm_patchtokens'], prenorm=feats['x_prenorm'])
    loss = 0.0
    for k, v in outs.items():
        w = torch.from_numpy(portable.uniform(f'convnext/{case}/w/{k}', tuple(v.shape))).to(v.device)
        loss = loss + (v * w).sum()
    loss.backward()
    return {k: v.detach() for k, v in outs.items()}, x.grad.detach()


def named_grads(model):
    """(name, parameter) of every parameter once, in state-dict order (norms.3.* is norm.*)"""
    return [(k, p) for k, p in model.named_parameters()]
