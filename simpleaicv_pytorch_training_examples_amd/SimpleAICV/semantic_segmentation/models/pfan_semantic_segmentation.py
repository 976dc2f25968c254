"""PFAN semantic segmentation on the MI355X kernels -- drop-in for the reference module
SimpleAICV/semantic_segmentation/models/pfan_semantic_segmentation.py (ConvBnActBlock :34, CPFE :68, ConvTransposeBnActBlock :125,
PFANSemanticSegmentation :155, the 13 factories :331-412).

Interface contract: same constructor arguments, the same module tree and construction order (a seeded construction draws the same
initial weights; checkpoints load key for key: `backbone.*`, `high_level_cpfe_{3,4}.{conv_1_1,conv_dil_3,conv_dil_5,conv_dil_7}.weight`,
`*.conv.layer.{0,1}.*`, `upsample_conv{1,3}.layer.{0,1}.*`, `pred_conv.{weight,bias}`), `forward(x) -> [B, num_classes, H, W]`.

Execution (every activation NCHW-shaped over NHWC memory, in the compute dtype):
  * CPFE: the 1x1 and the three dilated 3x3 convolutions (Cin -> 32 each) are one GEMM plus the tap gather of csrc/semseg.hip
    (`ops.cpfe_convs`), which writes the concatenated block directly; then the fused conv + BatchNorm + ReLU (`ops.conv_bn_act`).
  * the three bilinear resizes: the feature-pyramid resize kernel without a lateral (`ops.resize_bilinear`), whose
    backward is a fixed-order gather; fp32 output as under torch.autocast, the next convolution casts it back.
  * channel concatenations: torch.cat of NHWC tensors (channel-axis interleave, no layout change).
  * ConvTranspose2d(kernel 2, stride 2): a per-pixel linear map onto 4 * Cout values and a pixel shuffle, then the BatchNorm
    (+ ReLU) kernels (`ops.batch_norm2d`, `ops.act`).
  * pred_conv: `ops.conv2d` (implicit GEMM with the bias epilogue).
The DINOv3-ViT PFAN variant of the reference (dinov3_vit_pfan_semantic_segmentation.py) is not built."""
import torch
import torch.nn as nn

from .... import ops, ops_tfm
from ...detection.models import backbones

__all__ = [
    'resnet18_pfan_semantic_segmentation',
    'resnet34_pfan_semantic_segmentation',
    'resnet50_pfan_semantic_segmentation',
    'resnet101_pfan_semantic_segmentation',
    'resnet152_pfan_semantic_segmentation',
    'vanb0_pfan_semantic_segmentation',
    'vanb1_pfan_semantic_segmentation',
    'vanb2_pfan_semantic_segmentation',
    'vanb3_pfan_semantic_segmentation',
    'convformers18_pfan_semantic_segmentation',
    'convformers36_pfan_semantic_segmentation',
    'convformerm36_pfan_semantic_segmentation',
    'convformerb36_pfan_semantic_segmentation',
]


def _resize(x, size):
    """F.interpolate(x, size=size, mode='bilinear') on NHWC data"""
    if tuple(x.shape[2:]) == tuple(size):
        return x
    return ops.resize_bilinear(x, size)


class ConvBnActBlock(nn.Module):
    """Conv2d -> BatchNorm2d -> ReLU with the reference's switches; nn.Conv2d / nn.BatchNorm2d hold the parameters only.  Dense,
    undilated convolutions are what this model uses and what has a kernel here."""

    def __init__(self, inplanes, planes, kernel_size, stride, padding, groups=1, dilation=1, has_bn=True, has_act=True):
        super(ConvBnActBlock, self).__init__()
        if groups != 1 or dilation != 1:
            raise NotImplementedError('ConvBnActBlock: only groups=1, dilation=1 convolutions have kernels (dilated ones run inside CPFE)')
        self.layer = nn.Sequential(
            nn.Conv2d(inplanes, planes, kernel_size, stride=stride, padding=padding, groups=groups, dilation=dilation, bias=not has_bn),
            nn.BatchNorm2d(planes) if has_bn else nn.Sequential(),
            nn.ReLU(inplace=True) if has_act else nn.Sequential(),
        )
        self.stride, self.padding, self.has_bn, self.has_act = stride, padding, has_bn, has_act

    def forward(self, x):
        conv = self.layer[0]
        if self.has_bn:
            return ops.conv_bn_act(x, conv.weight, self.layer[1], self.stride, self.padding, self.has_act)
        y = ops.conv2d(x, conv.weight, conv.bias, self.stride, self.padding)
        return ops.act(y, 'relu') if self.has_act else y


class CPFE(nn.Module):
    """Context-aware pyramid feature extraction: a 1x1 and three dilated 3x3 convolutions of the same input, concatenated, then a
    3x3 conv + BN + ReLU back to `planes` channels."""

    def __init__(self, inplanes=512, planes=32, dilation_rate_list=[3, 5, 7]):
        super(CPFE, self).__init__()
        self.conv_1_1 = nn.Conv2d(inplanes, planes, kernel_size=1, stride=1, padding=0, bias=False)
        for d, rate in zip((3, 5, 7), dilation_rate_list):
            setattr(self, f'conv_dil_{d}', nn.Conv2d(inplanes, planes, kernel_size=3, stride=1, dilation=rate, padding=rate, bias=False))
        self.conv = ConvBnActBlock(planes * 4, planes, kernel_size=3, stride=1, padding=1, groups=1, dilation=1, has_bn=True,
                                   has_act=True)

    def forward(self, x):
        dil = [self.conv_dil_3, self.conv_dil_5, self.conv_dil_7]
        x = ops.cpfe_convs(x, self.conv_1_1.weight, [m.weight for m in dil], [m.dilation[0] for m in dil])
        return self.conv(x)


class ConvTransposeBnActBlock(nn.Module):
    """ConvTranspose2d(kernel = stride) -> BatchNorm2d -> ReLU.  With kernel_size == stride == 2 every input pixel owns its 2 x 2
    output pixels: a linear map per pixel onto (di, dj, cout) and a pixel shuffle."""

    def __init__(self, inplanes, planes, kernel_size, stride, groups=1, has_bn=True, has_act=True):
        super(ConvTransposeBnActBlock, self).__init__()
        if groups != 1 or kernel_size != 2 or stride != 2:
            raise NotImplementedError('ConvTransposeBnActBlock: only kernel_size=2, stride=2, groups=1 has a kernel')
        self.layer = nn.Sequential(
            nn.ConvTranspose2d(inplanes, planes, kernel_size=kernel_size, stride=stride, groups=groups, bias=not has_bn),
            nn.BatchNorm2d(planes) if has_bn else nn.Sequential(),
            nn.ReLU(inplace=True) if has_act else nn.Sequential(),
        )
        self.has_bn, self.has_act = has_bn, has_act

    def forward(self, x):
        deconv = self.layer[0]
        dt = ops.compute_dtype()
        x = ops._nhwc(x, dt)
        b, ci, h, w = x.shape
        co = deconv.weight.shape[1]
        wm = deconv.weight.permute(2, 3, 1, 0).reshape(4 * co, ci)                  # rows (di, dj, cout)
        bm = deconv.bias.repeat(4) if deconv.bias is not None else None
        y = ops_tfm.linear_nd(x.permute(0, 2, 3, 1), wm, bm)                        # [B, H, W, 4 * Cout]
        y = y.view(b, h, w, 2, 2, co).permute(0, 1, 3, 2, 4, 5).reshape(b, 2 * h, 2 * w, co).permute(0, 3, 1, 2)
        if self.has_bn:
            y = ops.batch_norm2d(y, self.layer[1])
        return ops.act(y, 'relu') if self.has_act else y


class PFANSemanticSegmentation(nn.Module):
    """num_classes counts the background class."""

    def __init__(self, backbone_type, backbone_pretrained_path='', planes=[32, 64, 160, 256], cpfe_planes=32, num_classes=151,
                 use_gradient_checkpoint=False):
        super(PFANSemanticSegmentation, self).__init__()
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
        self.pred_conv = nn.Conv2d(p, num_classes, kernel_size=3, stride=1, padding=1, bias=True)

    def forward(self, x):
        x1, x2, x3, x4 = self.backbone(x)                       # strides 4, 8, 16, 32
        # high-level features: CPFE on C4 and C5, merged at C4's resolution, carried to C2's
        g4 = _resize(self.high_level_cpfe_4(x4), x3.shape[2:])
        g3 = self.high_level_cpfe_3(x3)
        high = self.high_level_conv(torch.cat((g3, g4.to(g3.dtype)), dim=1))
        high = _resize(high, x1.shape[2:])
        # low-level features: C2 and C3 at C2's resolution
        l1 = self.low_level_conv_1(x1)
        l2 = _resize(self.low_level_conv_2(x2), x1.shape[2:])
        low = self.low_level_conv(torch.cat((l1, l2.to(l1.dtype)), dim=1))
        feats = self.reduce_conv1(torch.cat((low, high.to(low.dtype)), dim=1))
        feats = self.upsample_conv3(self.upsample_conv2(self.upsample_conv1(feats)))       # x4: the input resolution
        return ops.conv2d(feats, self.pred_conv.weight, self.pred_conv.bias, 1, 1)


def _pfan_semantic_segmentation(backbone_type, backbone_pretrained_path, planes, **kwargs):
    return PFANSemanticSegmentation(backbone_type=backbone_type, backbone_pretrained_path=backbone_pretrained_path, planes=planes,
                                    **kwargs)


_RESNET_BASIC, _RESNET_BOTTLENECK, _VAN = [64, 128, 256, 512], [256, 512, 1024, 2048], [64, 128, 320, 512]


def resnet18_pfan_semantic_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_semantic_segmentation('resnet18backbone', backbone_pretrained_path, _RESNET_BASIC, **kwargs)


def resnet34_pfan_semantic_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_semantic_segmentation('resnet34backbone', backbone_pretrained_path, _RESNET_BASIC, **kwargs)


def resnet50_pfan_semantic_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_semantic_segmentation('resnet50backbone', backbone_pretrained_path, _RESNET_BOTTLENECK, **kwargs)


def resnet101_pfan_semantic_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_semantic_segmentation('resnet101backbone', backbone_pretrained_path, _RESNET_BOTTLENECK, **kwargs)


def resnet152_pfan_semantic_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_semantic_segmentation('resnet152backbone', backbone_pretrained_path, _RESNET_BOTTLENECK, **kwargs)


def vanb0_pfan_semantic_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_semantic_segmentation('vanb0backbone', backbone_pretrained_path, [32, 64, 160, 256], **kwargs)


def vanb1_pfan_semantic_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_semantic_segmentation('vanb1backbone', backbone_pretrained_path, _VAN, **kwargs)


def vanb2_pfan_semantic_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_semantic_segmentation('vanb2backbone', backbone_pretrained_path, _VAN, **kwargs)


def vanb3_pfan_semantic_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_semantic_segmentation('vanb3backbone', backbone_pretrained_path, _VAN, **kwargs)


def convformers18_pfan_semantic_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_semantic_segmentation('convformers18backbone', backbone_pretrained_path, _VAN, **kwargs)


def convformers36_pfan_semantic_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_semantic_segmentation('convformers36backbone', backbone_pretrained_path, _VAN, **kwargs)


def convformerm36_pfan_semantic_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_semantic_segmentation('convformerm36backbone', backbone_pretrained_path, [96, 192, 384, 576], **kwargs)


def convformerb36_pfan_semantic_segmentation(backbone_pretrained_path='', **kwargs):
    return _pfan_semantic_segmentation('convformerb36backbone', backbone_pretrained_path, [128, 256, 512, 768], **kwargs)
