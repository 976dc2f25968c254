"""PFAN salient object detection on the MI355X kernels -- drop-in for the reference module
SimpleAICV/salient_object_detection/models/pfan_segmentation.py (PFANSegmentation :155, the 13 factories :313-379).

Interface contract: same constructor arguments, the same module tree and construction order (a seeded construction draws the same
initial weights; checkpoints load key for key: `backbone.*`, `high_level_cpfe_{3,4}.*`, `*.conv.layer.{0,1}.*`,
`upsample_conv{1,3}.layer.{0,1}.*`, `pred_conv.{weight,bias}`; `sigmoid` holds no state), `forward(x) -> fp32 probabilities
[B, 1, H, W]`.

Execution: the network is the semantic-segmentation PFAN with one output channel, and `ConvBnActBlock`, `CPFE` and
`ConvTransposeBnActBlock` are that module's classes (one copy).  The head differs: `pred_conv` (3x3, cpfe_planes -> 1), the
reference's `pred.float()` and its sigmoid are ONE streaming kernel each way (`ops.conv3x3_c1`, csrc/salient.hip): fp32 accumulation,
fp32 output, the logit is never rounded to bf16, and its weight / bias gradients are ordered sums.  When `cpfe_planes` is outside
that kernel's range (a multiple of 8 from 8 to 64) the head runs as `ops.conv2d` + `torch.sigmoid` on the fp32 logits.
`head_route` ('fused' or 'generic') names the route a model takes.  Measured on one MI355X at [8, 32, 1024, 1024] in bf16
(profiles/salient_step.json) the fused route takes 0.59 ms forward + backward against 2.00 ms for the generic
one, so 'fused' is the default wherever the kernel applies.

The DINOv3-ViT PFAN variant of the reference (dinov3_vit_pfan_segmentation.py) is not built."""
import torch
import torch.nn as nn

from .... import ops
from ...detection.models import backbones
from ...semantic_segmentation.models.pfan_semantic_segmentation import CPFE, ConvBnActBlock, ConvTransposeBnActBlock, _resize

__all__ = [
    'resnet18_pfan_segmentation',
    'resnet34_pfan_segmentation',
    'resnet50_pfan_segmentation',
    'resnet101_pfan_segmentation',
    'resnet152_pfan_segmentation',
    'vanb0_pfan_segmentation',
    'vanb1_pfan_segmentation',
    'vanb2_pfan_segmentation',
    'vanb3_pfan_segmentation',
    'convformers18_pfan_segmentation',
    'convformers36_pfan_segmentation',
    'convformerm36_pfan_segmentation',
    'convformerb36_pfan_segmentation',
]


class PFANSegmentation(nn.Module):

    def __init__(self, backbone_type, backbone_pretrained_path='', planes=[32, 64, 160, 256], cpfe_planes=32,
                 use_gradient_checkpoint=False):
        super(PFANSegmentation, self).__init__()
        self.use_gradient_checkpoint = use_gradient_checkpoint
        self.backbone = backbones.__dict__[backbone_type](**{'pretrained_path': backbone_pretrained_path,
                                                             'use_gradient_checkpoint': use_gradient_checkpoint})
        p = cpfe_planes

        def block(cin, k, act):
            return ConvBnActBlock(cin, p, kernel_size=k, stride=1, padding=k // 2, groups=1, dilation=1, has_bn=True, has_act=act)

        def up():
            return ConvTransposeBnActBlock(p, p, kernel_size=2, stride=2, groups=1, has_bn=True, has_act=True)

        # (construction order = the reference's: it fixes the order the initial weights are drawn in)
        self.high_level_cpfe_3 = CPFE(inplanes=planes[-2], planes=p, dilation_rate_list=[3, 5, 7])
        self.high_level_cpfe_4 = CPFE(inplanes=planes[-1], planes=p, dilation_rate_list=[3, 5, 7])
        self.high_level_conv = block(2 * p, 1, False)
        self.low_level_conv_1 = block(planes[-4], 3, True)
        self.low_level_conv_2 = block(planes[-3], 3, True)
        self.low_level_conv = block(2 * p, 1, False)
        self.reduce_conv1 = block(2 * p, 1, False)
        self.upsample_conv1 = up()
        self.upsample_conv2 = block(p, 3, True)
        self.upsample_conv3 = up()
        self.pred_conv = nn.Conv2d(p, 1, kernel_size=3, stride=1, padding=1, bias=True)
        self.sigmoid = nn.Sigmoid()
        self.head_route = 'fused' if ops.conv3x3_c1_supports(p) else 'generic'

    def forward(self, x):
        x1, x2, x3, x4 = self.backbone(x)                       # strides 4, 8, 16, 32
        g4 = _resize(self.high_level_cpfe_4(x4), x3.shape[2:])
        g3 = self.high_level_cpfe_3(x3)
        high = self.high_level_conv(torch.cat((g3, g4.to(g3.dtype)), dim=1))
        high = _resize(high, x1.shape[2:])
        l1 = self.low_level_conv_1(x1)
        l2 = _resize(self.low_level_conv_2(x2), x1.shape[2:])
        low = self.low_level_conv(torch.cat((l1, l2.to(l1.dtype)), dim=1))
        feats = self.reduce_conv1(torch.cat((low, high.to(low.dtype)), dim=1))
        feats = self.upsample_conv3(self.upsample_conv2(self.upsample_conv1(feats)))       # x4: the input resolution
        if self.head_route == 'fused':
            return ops.conv3x3_c1(feats, self.pred_conv.weight, self.pred_conv.bias, sigmoid=True)
        pred = ops.conv2d(feats, self.pred_conv.weight, self.pred_conv.bias, 1, 1)
        return torch.sigmoid(pred.float()).contiguous()


def _pfan_segmentation(backbone_type, backbone_pretrained_path, planes, **kwargs):
    return PFANSegmentation(backbone_type=backbone_type, backbone_pretrained_path=backbone_pretrained_path, planes=planes, **kwargs)


_RESNET_BASIC, _RESNET_BOTTLENECK, _VAN = [64, 128, 256, 512], [256, 512, 1024, 2048], [64, 128, 320, 512]


def resnet18_pfan_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_segmentation('resnet18backbone', backbone_pretrained_path, _RESNET_BASIC, **kwargs)


def resnet34_pfan_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_segmentation('resnet34backbone', backbone_pretrained_path, _RESNET_BASIC, **kwargs)


def resnet50_pfan_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_segmentation('resnet50backbone', backbone_pretrained_path, _RESNET_BOTTLENECK, **kwargs)


def resnet101_pfan_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_segmentation('resnet101backbone', backbone_pretrained_path, _RESNET_BOTTLENECK, **kwargs)


def resnet152_pfan_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_segmentation('resnet152backbone', backbone_pretrained_path, _RESNET_BOTTLENECK, **kwargs)


def vanb0_pfan_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_segmentation('vanb0backbone', backbone_pretrained_path, [32, 64, 160, 256], **kwargs)


def vanb1_pfan_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_segmentation('vanb1backbone', backbone_pretrained_path, _VAN, **kwargs)


def vanb2_pfan_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_segmentation('vanb2backbone', backbone_pretrained_path, _VAN, **kwargs)


def vanb3_pfan_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_segmentation('vanb3backbone', backbone_pretrained_path, _VAN, **kwargs)


def convformers18_pfan_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_segmentation('convformers18backbone', backbone_pretrained_path, _VAN, **kwargs)


def convformers36_pfan_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_segmentation('convformers36backbone', backbone_pretrained_path, _VAN, **kwargs)


def convformerm36_pfan_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_segmentation('convformerm36backbone', backbone_pretrained_path, [96, 192, 384, 576], **kwargs)


def convformerb36_pfan_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_segmentation('convformerb36backbone', backbone_pretrained_path, [128, 256, 512, 768], **kwargs)
