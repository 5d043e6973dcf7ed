"""HRNetV2 bodies (reference ever/module/_hrnet.py:187-659) on the HIP layers.

Constructor arguments, attribute names, child indices, state-dict keys and their order equal the reference's, so its
checkpoints load; parameters keep torch's default initialisation, as there (the reference defines kaiming / constant
helpers and never calls them).  The residual blocks are this package's (module/_resnets.py: the same attribute names,
BatchNorm momentum 0.1); every fuse / transition layer is a HipSequential of this package's Conv2d / BatchNorm2d / ReLU.  What is specific to
HRNet, the exchange at the end of a HighResolutionModule, runs as ONE kernel pass per output each way (HF.hr_fuse): the
BatchNorm of every incoming term is applied while the sum is formed, up-sampling is an index shift, and the backward reads
the output's gradient once for all terms.
"""
import torch
import torch.nn as nn

from ..hip import functional as HF
from ._resnets import BasicBlock, Bottleneck
from .fold import _takes_epilogue_stats, _use_folded, conv_bn, folded_conv2d
from .layers import BatchNorm2d, Conv2d, HipSequential, ReLU

BN_MOMENTUM = 0.1

__all__ = ['HighResolutionNet', 'HighResolutionModule', 'hrnetv2_w18', 'hrnetv2_w32', 'hrnetv2_w40', 'hrnetv2_w48']


def _extra(c):
    """the four published widths share everything but the branch channels (reference _hrnet.py:38-155)"""
    return dict(
        stage1=dict(num_modules=1, num_branches=1, block='BOTTLENECK', num_blocks=(4,), num_channels=(64,), fuse_method='SUM'),
        stage2=dict(num_modules=1, num_branches=2, block='BASIC', num_blocks=(4, 4), num_channels=(c, 2 * c),
                    fuse_method='SUM'),
        stage3=dict(num_modules=4, num_branches=3, block='BASIC', num_blocks=(4, 4, 4), num_channels=(c, 2 * c, 4 * c),
                    fuse_method='SUM'),
        stage4=dict(num_modules=3, num_branches=4, block='BASIC', num_blocks=(4, 4, 4, 4),
                    num_channels=(c, 2 * c, 4 * c, 8 * c), fuse_method='SUM'))


model_extra = dict(hrnetv2_w18=_extra(18), hrnetv2_w32=_extra(32), hrnetv2_w40=_extra(40), hrnetv2_w48=_extra(48))


def _bn(channels):
    return BatchNorm2d(channels, momentum=BN_MOMENTUM)


def _hooked(*mods):
    return any(m._forward_hooks or m._forward_pre_hooks for m in mods)


class HighResolutionModule(nn.Module):
    def __init__(self, num_branches, blocks, num_blocks, num_inchannels, num_channels, fuse_method, multi_scale_output=True):
        super().__init__()
        self._check_branches(num_branches, blocks, num_blocks, num_inchannels, num_channels)
        self.num_inchannels = num_inchannels
        self.fuse_method = fuse_method
        self.num_branches = num_branches
        self.multi_scale_output = multi_scale_output
        self.branches = self._make_branches(num_branches, blocks, num_blocks, num_channels)
        self.fuse_layers = self._make_fuse_layers()
        self.relu = ReLU(False)

    def _check_branches(self, num_branches, blocks, num_blocks, num_inchannels, num_channels):
        if num_branches != len(num_blocks):
            raise ValueError('NUM_BRANCHES({}) <> NUM_BLOCKS({})'.format(num_branches, len(num_blocks)))
        if num_branches != len(num_channels):
            raise ValueError('NUM_BRANCHES({}) <> NUM_CHANNELS({})'.format(num_branches, len(num_channels)))
        if num_branches != len(num_inchannels):
            raise ValueError('NUM_BRANCHES({}) <> NUM_INCHANNELS({})'.format(num_branches, len(num_inchannels)))
        if num_branches > 4:
            raise NotImplementedError('ever_amd HighResolutionModule: the exchange kernels sum at most 4 branches')

    def _make_one_branch(self, branch_index, block, num_blocks, num_channels, stride=1):
        downsample = None
        if stride != 1 or self.num_inchannels[branch_index] != num_channels[branch_index] * block.expansion:
            downsample = nn.Sequential(
                Conv2d(self.num_inchannels[branch_index], num_channels[branch_index] * block.expansion, kernel_size=1,
                       stride=stride, bias=False),
                _bn(num_channels[branch_index] * block.expansion))
        layers = [block(self.num_inchannels[branch_index], num_channels[branch_index], stride, downsample)]
        self.num_inchannels[branch_index] = num_channels[branch_index] * block.expansion
        for _ in range(1, num_blocks[branch_index]):
            layers.append(block(self.num_inchannels[branch_index], num_channels[branch_index]))
        return nn.Sequential(*layers)

    def _make_branches(self, num_branches, block, num_blocks, num_channels):
        return nn.ModuleList([self._make_one_branch(i, block, num_blocks, num_channels) for i in range(num_branches)])

    def _make_fuse_layers(self):
        if self.num_branches == 1:
            return None
        num_branches, num_inchannels = self.num_branches, self.num_inchannels
        fuse_layers = []
        for i in range(num_branches if self.multi_scale_output else 1):
            fuse_layer = []
            for j in range(num_branches):
                if j > i:
                    # (the nn.Upsample child keeps the reference's indices; the up-sampling itself is hr_fuse's index shift)
                    fuse_layer.append(HipSequential(
                        Conv2d(num_inchannels[j], num_inchannels[i], 1, 1, 0, bias=False),
                        _bn(num_inchannels[i]),
                        nn.Upsample(scale_factor=2 ** (j - i), mode='nearest')))
                elif j == i:
                    fuse_layer.append(nn.Identity())
                else:
                    conv3x3s = []
                    for k in range(i - j):
                        if k == i - j - 1:
                            conv3x3s.append(HipSequential(
                                Conv2d(num_inchannels[j], num_inchannels[i], 3, 2, 1, bias=False),
                                _bn(num_inchannels[i])))
                        else:
                            conv3x3s.append(HipSequential(
                                Conv2d(num_inchannels[j], num_inchannels[j], 3, 2, 1, bias=False),
                                _bn(num_inchannels[j]),
                                ReLU(False)))
                    fuse_layer.append(HipSequential(*conv3x3s))
            fuse_layers.append(nn.ModuleList(fuse_layer))
        return nn.ModuleList(fuse_layers)

    def get_num_inchannels(self):
        return self.num_inchannels

    @staticmethod
    def _conv_bn_term(conv, bn, x, shift):
        """bn(conv(x)) as a term of HF.hr_fuse: the folded convolution's output at inference, else the raw convolution output
        with the BatchNorm for hr_fuse to apply; a BatchNorm of another kind, or hooks on either layer (or global ones), run
        the two layers by their own forward and the result enters as a plain term"""
        if _use_folded(conv, bn):
            return folded_conv2d(x, conv), shift, None
        if type(bn) is not BatchNorm2d or _hooked(conv, bn) or HF.observers_active():
            return bn(conv(x, bn_stats=_takes_epilogue_stats(bn))), shift, None
        return conv(x, bn_stats=_takes_epilogue_stats(bn)), shift, bn

    def _up_term(self, layer, x, shift):
        """fuse_layers[i][j], j > i: conv1x1 -> BatchNorm -> nearest x 2^(j-i)"""
        if _hooked(layer, layer[2]):
            raise NotImplementedError('ever_amd HighResolutionModule: the nearest up-sampling of a fuse layer happens inside the '
                                      'exchange kernel, so a hook on the layer or on its nn.Upsample has nothing to observe; '
                                      'hook its convolution or its BatchNorm instead')
        return self._conv_bn_term(layer[0], layer[1], x, shift)

    def _down_term(self, chain, x):
        """fuse_layers[i][j], j < i: (conv3x3s2 -> BatchNorm -> ReLU) x (i-j-1), then conv3x3s2 -> BatchNorm"""
        last = chain[len(chain) - 1]
        if _hooked(chain, last) or len(last) != 2:
            return chain(x), 0, None
        for sub in list(chain)[:-1]:
            x = sub(x)
        return self._conv_bn_term(last[0], last[1], x, 0)

    def forward(self, x):
        if self.num_branches == 1:
            return [self.branches[0](x[0])]
        for i in range(self.num_branches):
            x[i] = self.branches[i](x[i])
        x_fuse = []
        for i in range(len(self.fuse_layers)):
            terms = []
            for j in range(self.num_branches):      # j ascending: the reference's order of summation
                if j == i:
                    terms.append((x[j], 0, None))
                elif j > i:
                    terms.append(self._up_term(self.fuse_layers[i][j], x[j], j - i))
                else:
                    terms.append(self._down_term(self.fuse_layers[i][j], x[j]))
            x_fuse.append(HF.hr_fuse(terms))
        return x_fuse


blocks_dict = {'BASIC': BasicBlock, 'BOTTLENECK': Bottleneck}


class HighResolutionNet(nn.Module):
    def __init__(self, extra, norm_eval=True, zero_init_residual=False, frozen_stages=-1):
        super().__init__()
        self.norm_eval = norm_eval
        self.frozen_stages = frozen_stages
        self.zero_init_residual = zero_init_residual
        self.extra = extra
        # stem
        self.conv1 = Conv2d(3, 64, kernel_size=3, stride=2, padding=1, bias=False)
        self.bn1 = _bn(64)
        self.conv2 = Conv2d(64, 64, kernel_size=3, stride=2, padding=1, bias=False)
        self.bn2 = _bn(64)
        self.relu = ReLU(inplace=True)

        self.stage1_cfg = self.extra['stage1']
        num_channels = self.stage1_cfg['num_channels'][0]
        block = blocks_dict[self.stage1_cfg['block']]
        num_blocks = self.stage1_cfg['num_blocks'][0]
        stage1_out_channels = num_channels * block.expansion
        self.layer1 = self._make_layer(block, 64, num_channels, num_blocks)

        self.stage2_cfg = self.extra['stage2']
        block = blocks_dict[self.stage2_cfg['block']]
        num_channels = [c * block.expansion for c in self.stage2_cfg['num_channels']]
        self.transition1 = self._make_transition_layer([stage1_out_channels], num_channels)
        self.stage2, pre_stage_channels = self._make_stage(self.stage2_cfg, num_channels)

        self.stage3_cfg = self.extra['stage3']
        block = blocks_dict[self.stage3_cfg['block']]
        num_channels = [c * block.expansion for c in self.stage3_cfg['num_channels']]
        self.transition2 = self._make_transition_layer(pre_stage_channels, num_channels)
        self.stage3, pre_stage_channels = self._make_stage(self.stage3_cfg, num_channels)

        self.stage4_cfg = self.extra['stage4']
        block = blocks_dict[self.stage4_cfg['block']]
        num_channels = [c * block.expansion for c in self.stage4_cfg['num_channels']]
        self.transition3 = self._make_transition_layer(pre_stage_channels, num_channels)
        self.stage4, pre_stage_channels = self._make_stage(self.stage4_cfg, num_channels)

        self._frozen_stages()

    def _make_transition_layer(self, num_channels_pre_layer, num_channels_cur_layer):
        num_branches_cur, num_branches_pre = len(num_channels_cur_layer), len(num_channels_pre_layer)
        transition_layers = []
        for i in range(num_branches_cur):
            if i < num_branches_pre:
                if num_channels_cur_layer[i] != num_channels_pre_layer[i]:
                    transition_layers.append(HipSequential(
                        Conv2d(num_channels_pre_layer[i], num_channels_cur_layer[i], 3, 1, 1, bias=False),
                        _bn(num_channels_cur_layer[i]),
                        ReLU(inplace=True)))
                else:
                    transition_layers.append(nn.Identity())
            else:
                conv3x3s = []
                for j in range(i + 1 - num_branches_pre):
                    inchannels = num_channels_pre_layer[-1]
                    outchannels = num_channels_cur_layer[i] if j == i - num_branches_pre else inchannels
                    conv3x3s.append(HipSequential(
                        Conv2d(inchannels, outchannels, 3, 2, 1, bias=False), _bn(outchannels), ReLU(inplace=True)))
                transition_layers.append(HipSequential(*conv3x3s))
        return nn.ModuleList(transition_layers)

    def _make_layer(self, block, inplanes, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or inplanes != planes * block.expansion:
            downsample = nn.Sequential(Conv2d(inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                                       _bn(planes * block.expansion))
        layers = [block(inplanes, planes, stride, downsample)]
        inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(inplanes, planes))
        return nn.Sequential(*layers)

    def _frozen_stages(self):
        if self.frozen_stages >= 0:      # the stem
            for m in [self.conv1, self.bn1, self.conv2, self.bn2]:
                for param in m.parameters():
                    param.requires_grad = False
        if self.frozen_stages == 1:
            for param in self.layer1.parameters():
                param.requires_grad = False

    def _make_stage(self, layer_config, num_inchannels, multi_scale_output=True):
        num_modules = layer_config['num_modules']
        block = blocks_dict[layer_config['block']]
        modules = []
        for i in range(num_modules):
            # multi_scale_output is only used by the last module
            reset_multi_scale_output = multi_scale_output or i != num_modules - 1
            modules.append(HighResolutionModule(layer_config['num_branches'], block, layer_config['num_blocks'], num_inchannels,
                                                layer_config['num_channels'], layer_config['fuse_method'],
                                                reset_multi_scale_output))
            num_inchannels = modules[-1].get_num_inchannels()
        return nn.Sequential(*modules), num_inchannels

    def conv_bn_pairs(self):
        """the stem's convolution / BatchNorm neighbours, for module/fold.py (the other pairs sit in blocks and Sequentials)"""
        return [(self.conv1, self.bn1), (self.conv2, self.bn2)]

    def check_channels(self):
        """The BatchNorm and exchange kernels read 16 bytes per lane along the channel axis: every branch width must be a
        multiple of 4.  hrnetv2_w18 (18-channel branch) builds, loads and saves, and cannot run."""
        for name in ('stage1', 'stage2', 'stage3', 'stage4'):
            cfg = self.extra[name]
            bad = [c for c in cfg['num_channels'] if (c * blocks_dict[cfg['block']].expansion) % 4]
            if bad:
                raise NotImplementedError(f'ever_amd HighResolutionNet: {name} has a branch of {bad[0]} channels; the BatchNorm and '
                                          f'exchange kernels need channel counts that are multiples of 4 (C % 4 == 0)')

    def forward(self, x):
        self.check_channels()
        HF._require_cuda(x, 'HighResolutionNet input')
        x = conv_bn(self.conv1, self.bn1, x, relu=True)
        x = conv_bn(self.conv2, self.bn2, x, relu=True)
        x = self.layer1(x)

        x_list = []
        for i in range(self.stage2_cfg['num_branches']):
            t = self.transition1[i]
            x_list.append(x if isinstance(t, nn.Identity) else t(x))
        y_list = self.stage2(x_list)

        x_list = []
        for i in range(self.stage3_cfg['num_branches']):
            t = self.transition2[i]
            x_list.append(y_list[i] if isinstance(t, nn.Identity) else t(y_list[-1]))
        y_list = self.stage3(x_list)

        x_list = []
        for i in range(self.stage4_cfg['num_branches']):
            t = self.transition3[i]
            x_list.append(y_list[i] if isinstance(t, nn.Identity) else t(y_list[-1]))
        return self.stage4(x_list)

    def train(self, mode=True):
        super().train(mode)
        if mode and self.norm_eval:
            for m in self.modules():
                if isinstance(m, nn.BatchNorm2d):
                    m.eval()
        return self


def _factory(name):
    def build(pretrained=False, weight_path=None, norm_eval=False, frozen_stages=-1):
        model = HighResolutionNet(model_extra[name], norm_eval, zero_init_residual=False, frozen_stages=frozen_stages)
        if pretrained:
            if weight_path is None:
                raise ValueError(f'ever_amd {name}: pretrained=True needs weight_path (a local state dict); nothing is downloaded')
            state_dict = torch.load(weight_path, map_location=torch.device('cpu'))
            model.load_state_dict(state_dict, strict=False)
        return model
    build.__name__ = build.__qualname__ = name
    build.__doc__ = f'HRNetV2 {name[-3:].upper()} (reference _hrnet.py:610-659); pretrained weights only from a local weight_path.'
    return build


hrnetv2_w18, hrnetv2_w32 = _factory('hrnetv2_w18'), _factory('hrnetv2_w32')
hrnetv2_w40, hrnetv2_w48 = _factory('hrnetv2_w40'), _factory('hrnetv2_w48')
