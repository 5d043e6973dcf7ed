"""What the BiFPN fixtures' writer (tools/gen_golden_bifpn.py) and their readers (tests/test_bifpn_*.py) share: the cases, the
portable weights and inputs, and the end-to-end composition.  Everything is regenerated from oracle/portable.py; only the
reference's outputs are stored under tests/golden."""
import numpy as np
import torch

from oracle import portable

# name -> (normalized_fusion, downsample_op, feature_strides, input map edges)
MODULE_CASES = {
    'fast_conv': ('fast_normalize', 'conv', [4, 8, 16, 32], (32, 16, 8, 4)),
    'softmax_maxpool': ('softmax', 'maxpool', [4, 8, 16, 32], (32, 16, 8, 4)),
    'fast_conv_repeat': ('fast_normalize', 'conv', [4, 8, 16, 16], (8, 4, 2, 2)),
}
MODULE_C, MODULE_N = 16, 2
# state-dict layouts recorded in bifpn_keys.json: name -> constructor arguments after in_channels = 256
KEY_CASES = {
    'default': dict(feature_strides=[4, 8, 16, 32]),
    'maxpool': dict(feature_strides=[4, 8, 16, 32], downsample_op='maxpool'),
    'repeat': dict(feature_strides=[4, 8, 16, 16]),
}
E2E = dict(name='bifpn_e2e_r18', n=2, hw=64, num_classes=6, width=64, decoder_width=32, stride=4)
# The Fusion node that carries one negative raw weight (fast_normalize: its ReLU gate is shut, its term leaves with weight 0).
# A three-input node: with ONE live term a node's weight gradient is zero in exact arithmetic (the BatchNorm behind the node
# does not see the scale of its input), and a two-input node would compare rounding residues.
NEGATIVE = ('triple_fusion_modules.0.0.weights',)


def stored_stride(edge):
    """maps of 32 x 32 are stored at every second pixel (fixture size); smaller ones in full"""
    return 2 if edge >= 32 else 1


def fusion_weights(name, n, norm_method):
    """raw Fusion.weights away from their initial values (ones / zeros): a wrong Jacobian would not show at the initial point"""
    if norm_method == 'softmax':
        return portable.uniform(name, (n,), -1.0, 1.0)
    w = portable.uniform(name, (n,), 0.3, 1.7)
    if any(name.endswith(k) for k in NEGATIVE):
        w[1] = -0.4
    return w


def load_portable(m, prefix=''):
    """fill_state_dict for everything, then the Fusion weights (fill_state_dict would draw them as biases, in [-0.2, 0.2])"""
    sd = m.state_dict()
    filled = portable.fill_state_dict(sd)
    norms = {k + '.weights': mod.norm_method for k, mod in m.named_modules() if hasattr(mod, 'norm_method')}
    for k in filled:
        if k in norms:
            filled[k] = fusion_weights(k[len(prefix):] if k.startswith(prefix) else k, filled[k].shape[0], norms[k])
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in filled.items()}, strict=True)
    return m


def module_inputs(case):
    edges = MODULE_CASES[case][3]
    xs = [portable.normalish(f'bifpn_module/{case}/x{i}', (MODULE_N, MODULE_C, e, e)) for i, e in enumerate(edges)]
    gs = [portable.uniform(f'bifpn_module/{case}/g{i}', (MODULE_N, MODULE_C, e, e)) for i, e in enumerate(edges)]
    return xs, gs


class BiFPNSeg(torch.nn.Module):
    """ResNet-18 -> FPN -> BiFPN -> AssymetricDecoder on the modules of `mods` (ever_amd.module here, the reference's in the
    fixture writer): logits at the input's size"""

    def __init__(self, mods):
        super().__init__()
        w, dw = E2E['width'], E2E['decoder_width']
        self.en = mods.ResNetEncoder(dict(resnet_type='resnet18'))
        self.fpn = mods.FPN([64, 128, 256, 512], w)
        self.bifpn = mods.BiFPN(w, [4, 8, 16, 32])
        self.decoder = mods.AssymetricDecoder(w, dw, classifier_config=dict(scale_factor=4, num_classes=E2E['num_classes'],
                                                                            kernel_size=1))

    def forward(self, x):
        return self.decoder(self.bifpn(list(self.fpn(self.en(x)))))
