from . import loss  # noqa: F401
from .aspp import ASPPHead, AtrousSpatialPyramidPool
from .changestar import ChangeMixin, ChangeStarFarSeg
from . import dinov3  # noqa: F401
from .convnext_encoder import ConvNeXtEncoder
from .deeplab import DeepLabV3Plus
from .deeplabv3p_head import Deeplabv3pDecoder, Deeplabv3pHead
from .farseg import FarSeg, FarSegPP
from .fpn import FPN, AssymetricDecoder, BiFPN, FastNormalizedFusionConv3x3, Fusion, NormalizedFusionConv3x3
from .freenet import FreeNet
from .hrnet import HRNetEncoder
from .hrnet_head import HRNetHead, SimpleFusion
from .hrnet_seg import HRNetSeg
from ._hrnet import HighResolutionModule, HighResolutionNet
from .fs_relation import FarSegHead, FarSegPPHead, FSRelation, FSRelationV2
from .layers import (AdaptiveAvgPool2d, BatchNorm2d, Conv2d, ConvTranspose2d, HipSequential, LayerNorm, MaxPool2d, ReLU,
                     UpsamplingBilinear2d, to_hip)
from .ops import Bf16compatible, ConvBlock, ConvUpsampling, DepthwiseConv2d, PoolBlock, SeparableConv2d, SeparableConvBlock
from .ppm import PPMHead, PyramidPoolModule
from .pspnet import PSPNet
from .resnet import ResNetEncoder
from .vit_encoder import ViTEncoder

__all__ = ['ResNetEncoder', 'FPN', 'AssymetricDecoder', 'FSRelation', 'FSRelationV2', 'FarSegHead', 'FarSegPPHead', 'FarSeg', 'FarSegPP', 'FreeNet', 'ChangeMixin', 'ChangeStarFarSeg', 'ConvBlock',
           'Bf16compatible', 'ConvUpsampling', 'Conv2d', 'ConvTranspose2d', 'BatchNorm2d', 'ReLU', 'MaxPool2d', 'UpsamplingBilinear2d',
           'AdaptiveAvgPool2d', 'HipSequential', 'to_hip', 'loss',
           'DepthwiseConv2d', 'SeparableConv2d', 'SeparableConvBlock', 'PoolBlock', 'AtrousSpatialPyramidPool', 'ASPPHead',
           'Deeplabv3pDecoder', 'Deeplabv3pHead', 'DeepLabV3Plus',
           'HighResolutionModule', 'HighResolutionNet', 'HRNetEncoder', 'SimpleFusion', 'HRNetHead', 'HRNetSeg',
           'Fusion', 'FastNormalizedFusionConv3x3', 'NormalizedFusionConv3x3', 'BiFPN',
           'LayerNorm', 'ConvNeXtEncoder', 'dinov3', 'ViTEncoder', 'PyramidPoolModule', 'PPMHead', 'PSPNet']
