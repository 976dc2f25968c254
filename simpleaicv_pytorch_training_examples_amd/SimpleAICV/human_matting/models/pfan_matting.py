"""PFAN human matting on the MI355X kernels -- drop-in for the reference module SimpleAICV/human_matting/models/pfan_matting.py
(PFANMatting :157, the 13 factories :466-529).

Interface contract: same constructor arguments, the same module tree and construction order (a seeded construction draws the same
initial weights; checkpoints load key for key: `backbone.*`, `global_*` and `local_*` with `*.conv.layer.{0,1}.*`,
`*_upsample_conv{1,3}.layer.{0,1}.*`, `global_pred_conv.{weight,bias}`, `local_pred_conv.{weight,bias}`; `sigmoid` holds no state),
`forward(x) -> (global_pred [B, 3, H, W], local_pred [B, 1, H, W], fused_pred [B, 1, H, W])`, all fp32 probabilities, under
autocast too.

Execution: two PFAN decoders over one backbone, built from the semantic-segmentation module's `ConvBnActBlock`, `CPFE` and
`ConvTransposeBnActBlock` (one copy).  The local head -- `local_pred_conv` (3x3, cpfe_planes -> 1), `.float()` and the sigmoid -- is
ONE streaming kernel each way (`ops.conv3x3_c1`, csrc/salient.hip) where `ops.conv3x3_c1_supports(cpfe_planes)` holds, else
`ops.conv2d` + `torch.sigmoid` on the fp32 logits; `head_route` ('fused' or 'generic') names the route a model takes.  The global
head has three output channels: `ops.conv2d` and a sigmoid on the fp32 logits.  `collaborative_matting` is one kernel each way
(`ops.collaborative_matting`, csrc/matting.hip): the first maximum of the three global probabilities selects 0, local_pred or 1,
and the gradient reaches local_pred only where that maximum is class 1, as through the reference's masks.

The DINOv3-ViT PFAN variant of the reference (dinov3_vit_pfan_matting.py) is not built."""
import torch
import torch.nn as nn

from .... import ops
from ...detection.models import backbones
from ...semantic_segmentation.models.pfan_semantic_segmentation import CPFE, ConvBnActBlock, ConvTransposeBnActBlock, _resize

__all__ = [
    'resnet18_pfan_matting',
    'resnet34_pfan_matting',
    'resnet50_pfan_matting',
    'resnet101_pfan_matting',
    'resnet152_pfan_matting',
    'vanb0_pfan_matting',
    'vanb1_pfan_matting',
    'vanb2_pfan_matting',
    'vanb3_pfan_matting',
    'convformers18_pfan_matting',
    'convformers36_pfan_matting',
    'convformerm36_pfan_matting',
    'convformerb36_pfan_matting',
]


class PFANMatting(nn.Module):

    def __init__(self, backbone_type, backbone_pretrained_path='', planes=[32, 64, 160, 256], cpfe_planes=32,
                 use_gradient_checkpoint=False):
        super(PFANMatting, self).__init__()
        self.use_gradient_checkpoint = use_gradient_checkpoint
        self.backbone = backbones.__dict__[backbone_type](**{'pretrained_path': backbone_pretrained_path,
                                                             'use_gradient_checkpoint': use_gradient_checkpoint})
        p = cpfe_planes

        def block(cin, k, act):
            return ConvBnActBlock(cin, p, kernel_size=k, stride=1, padding=k // 2, groups=1, dilation=1, has_bn=True, has_act=act)

        def up():
            return ConvTransposeBnActBlock(p, p, kernel_size=2, stride=2, groups=1, has_bn=True, has_act=True)

        # (construction order = the reference's: it fixes the order the initial weights are drawn in)
        self.global_high_level_cpfe_3 = CPFE(inplanes=planes[-2], planes=p, dilation_rate_list=[3, 5, 7])
        self.global_high_level_cpfe_4 = CPFE(inplanes=planes[-1], planes=p, dilation_rate_list=[3, 5, 7])
        self.global_high_level_conv = block(2 * p, 1, False)
        self.global_low_level_conv_1 = block(planes[-4], 3, True)
        self.global_low_level_conv_2 = block(planes[-3], 3, True)
        self.global_low_level_conv = block(2 * p, 1, False)
        self.global_reduce_conv1 = block(2 * p, 1, False)
        self.global_upsample_conv1 = up()
        self.global_upsample_conv2 = block(p, 3, True)
        self.global_upsample_conv3 = up()
        self.global_pred_conv = nn.Conv2d(p, 3, kernel_size=3, stride=1, padding=1, bias=True)

        self.local_high_level_cpfe_3 = CPFE(inplanes=planes[-2], planes=p, dilation_rate_list=[3, 5, 7])
        self.local_high_level_cpfe_4 = CPFE(inplanes=planes[-1], planes=p, dilation_rate_list=[3, 5, 7])
        self.local_high_level_conv = block(2 * p, 1, False)
        self.local_low_level_conv_1 = block(planes[-4], 3, True)
        self.local_low_level_conv_2 = block(planes[-3], 3, True)
        self.local_low_level_conv = block(2 * p, 1, False)
        self.local_reduce_conv1 = block(4 * p, 1, False)
        self.local_upsample_conv1 = up()
        self.local_upsample_conv2 = block(p, 3, True)
        self.local_upsample_conv3 = up()
        self.local_pred_conv = nn.Conv2d(p, 1, kernel_size=3, stride=1, padding=1, bias=True)
        self.sigmoid = nn.Sigmoid()
        self.head_route = 'fused' if ops.conv3x3_c1_supports(p) else 'generic'

    def forward(self, x):
        x1, x2, x3, x4 = self.backbone(x)                       # strides 4, 8, 16, 32
        size3, size1 = x3.shape[2:], x1.shape[2:]

        def cat(*ts):
            return torch.cat([ts[0]] + [t.to(ts[0].dtype) for t in ts[1:]], dim=1)

        # global decoder
        g4 = _resize(self.global_high_level_cpfe_4(x4), size3)
        g3 = self.global_high_level_cpfe_3(x3)
        high_g = _resize(self.global_high_level_conv(cat(g3, g4)), size1)
        l1 = self.global_low_level_conv_1(x1)
        l2 = _resize(self.global_low_level_conv_2(x2), size1)
        low_g = self.global_low_level_conv(cat(l1, l2))
        feats = self.global_reduce_conv1(cat(low_g, high_g))
        feats = self.global_upsample_conv3(self.global_upsample_conv2(self.global_upsample_conv1(feats)))
        global_pred = ops.conv2d(feats, self.global_pred_conv.weight, self.global_pred_conv.bias, 1, 1)
        global_pred = torch.sigmoid(global_pred.float())

        # local decoder: it also reads the global decoder's low- and high-level features
        f3 = self.local_high_level_cpfe_3(x3)
        f4 = _resize(self.local_high_level_cpfe_4(x4), size3)
        high_f = _resize(self.local_high_level_conv(cat(f3, f4)), size1)
        high_f = cat(high_f, high_g)
        m1 = self.local_low_level_conv_1(x1)
        m2 = _resize(self.local_low_level_conv_2(x2), size1)
        low_f = self.local_low_level_conv(cat(m1, m2))
        feats = self.local_reduce_conv1(cat(low_f, low_g, high_f))
        feats = self.local_upsample_conv3(self.local_upsample_conv2(self.local_upsample_conv1(feats)))
        if self.head_route == 'fused':
            local_pred = ops.conv3x3_c1(feats, self.local_pred_conv.weight, self.local_pred_conv.bias, sigmoid=True)
        else:
            local_pred = ops.conv2d(feats, self.local_pred_conv.weight, self.local_pred_conv.bias, 1, 1)
            local_pred = torch.sigmoid(local_pred.float()).contiguous()
        return global_pred, local_pred, self.collaborative_matting(global_pred, local_pred)

    def collaborative_matting(self, global_pred, local_pred):
        # class 0 background, 1 the local (unknown) region, 2 the global foreground
        if global_pred.is_cuda:
            return ops.collaborative_matting(global_pred, local_pred)
        idx = torch.max(global_pred, dim=1)[1].unsqueeze(1)
        return local_pred * (idx == 1).float() + (idx == 2).float()


def _pfan_matting(backbone_type, backbone_pretrained_path, planes, **kwargs):
    return PFANMatting(backbone_type=backbone_type, backbone_pretrained_path=backbone_pretrained_path, planes=planes, **kwargs)


_RESNET_BASIC, _RESNET_BOTTLENECK, _VAN = [64, 128, 256, 512], [256, 512, 1024, 2048], [64, 128, 320, 512]


def resnet18_pfan_matting(backbone_pretrained_path='', **kwargs):
    return _pfan_matting('resnet18backbone', backbone_pretrained_path, _RESNET_BASIC, **kwargs)


def resnet34_pfan_matting(backbone_pretrained_path='', **kwargs):
    return _pfan_matting('resnet34backbone', backbone_pretrained_path, _RESNET_BASIC, **kwargs)


def resnet50_pfan_matting(backbone_pretrained_path='', **kwargs):
    return _pfan_matting('resnet50backbone', backbone_pretrained_path, _RESNET_BOTTLENECK, **kwargs)


def resnet101_pfan_matting(backbone_pretrained_path='', **kwargs):
    return _pfan_matting('resnet101backbone', backbone_pretrained_path, _RESNET_BOTTLENECK, **kwargs)


def resnet152_pfan_matting(backbone_pretrained_path='', **kwargs):
    return _pfan_matting('resnet152backbone', backbone_pretrained_path, _RESNET_BOTTLENECK, **kwargs)


def vanb0_pfan_matting(backbone_pretrained_path='', **kwargs):
    return _pfan_matting('vanb0backbone', backbone_pretrained_path, [32, 64, 160, 256], **kwargs)


def vanb1_pfan_matting(backbone_pretrained_path='', **kwargs):
    return _pfan_matting('vanb1backbone', backbone_pretrained_path, _VAN, **kwargs)


def vanb2_pfan_matting(backbone_pretrained_path='', **kwargs):
    return _pfan_matting('vanb2backbone', backbone_pretrained_path, _VAN, **kwargs)


def vanb3_pfan_matting(backbone_pretrained_path='', **kwargs):
    return _pfan_matting('vanb3backbone', backbone_pretrained_path, _VAN, **kwargs)


def convformers18_pfan_matting(backbone_pretrained_path='', **kwargs):
    return _pfan_matting('convformers18backbone', backbone_pretrained_path, _VAN, **kwargs)


def convformers36_pfan_matting(backbone_pretrained_path='', **kwargs):
    return _pfan_matting('convformers36backbone', backbone_pretrained_path, _VAN, **kwargs)


def convformerm36_pfan_matting(backbone_pretrained_path='', **kwargs):
    return _pfan_matting('convformerm36backbone', backbone_pretrained_path, [96, 192, 384, 576], **kwargs)


def convformerb36_pfan_matting(backbone_pretrained_path='', **kwargs):
    return _pfan_matting('convformerb36backbone', backbone_pretrained_path, [128, 256, 512, 768], **kwargs)
