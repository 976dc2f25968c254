"""ResNet backbones of the reference's text-recognition family (SimpleAICV/text_recognition/models/backbones/resnet.py) on the
engine's fused convolution blocks: same class and factory names, constructor arguments, `state_dict` keys and initialisation draw
order (equal seeds give equal weights).  The image is 32 x W; layers 3 and 4 halve the HEIGHT only: their first block has a
(3, 1) convolution with stride (2, 1), padding (1, 0) and a 1 x 1 shortcut with stride (2, 1).  The engine's convolution has one
stride and one padding, so these two are composed:
  * the 1 x 1 stride-(2, 1) shortcut is a row slice x[:, :, ::2, :] followed by the stride-1 1 x 1 block (ops.conv_bn_act);
  * the (3, 1) stride-(2, 1) convolution runs through torch (F.conv2d on the channels-last tensor), followed by
    ops.batch_norm2d and ops.act.
Their feature maps are at most 4 rows high (8 rows in, 4 out in layer 3; 4 in, 2 out in layer 4).  Every other convolution is the
classification ResNet's fused block."""
import torch.nn as nn
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

from ..... import ops
from ....classification.backbones.resnet import ConvBnActBlock as _ConvBnActBlock, _init_like_reference
from ....classification.common import load_state_dict

__all__ = [
    'resnet18backbone',
    'resnet34backbone',
    'resnet50backbone',
    'resnet101backbone',
    'resnet152backbone',
]


class ConvBnActBlock(_ConvBnActBlock):
    """the classification block; a tuple stride (2, 1) takes one of the two composed forms of the module docstring"""

    def forward(self, x, residual=None, act=None, **kw):
        if not isinstance(self.stride, tuple):
            return super().forward(x, residual=residual, act=act, **kw)
        conv, bn = self.layer[0], self.layer[1]
        relu = self.has_act if act is None else act
        if self.stride != (2, 1) or residual is not None or kw:
            raise NotImplementedError(f'ConvBnActBlock(stride={self.stride}) with a residual or a fused option')
        if conv.kernel_size == (1, 1):
            return ops.conv_bn_act(x[:, :, ::2, :], conv.weight, bn, 1, 0, relu)
        if conv.kernel_size == (3, 1) and self.padding == (1, 0):
            x = ops._nhwc(x)
            y = F.conv2d(x, conv.weight.to(x.dtype), None, stride=(2, 1), padding=(1, 0))
            y = ops.batch_norm2d(y, bn)
            return ops.act(y, 'relu') if relu else y
        raise NotImplementedError(f'ConvBnActBlock(kernel_size={conv.kernel_size}, stride={self.stride}, padding={self.padding})')


def _downsample(stride, inplanes, outplanes):
    return (max(stride) if isinstance(stride, tuple) else stride) != 1 or inplanes != outplanes


class BasicBlock(nn.Module):

    def __init__(self, inplanes, planes, kernel_size, stride, padding):
        super(BasicBlock, self).__init__()
        self.downsample = _downsample(stride, inplanes, planes)
        self.conv1 = ConvBnActBlock(inplanes, planes, kernel_size=kernel_size, stride=stride, padding=padding, groups=1,
                                    has_bn=True, has_act=True)
        self.conv2 = ConvBnActBlock(planes, planes, kernel_size=3, stride=1, padding=1, groups=1, has_bn=True, has_act=False)
        self.relu = nn.ReLU(inplace=True)
        if self.downsample:
            self.downsample_conv = ConvBnActBlock(inplanes, planes, kernel_size=1, stride=stride, padding=0, groups=1,
                                                  has_bn=True, has_act=False)

    def forward(self, x):
        out = self.conv1(x)
        identity = self.downsample_conv(x) if self.downsample else x
        return self.conv2(out, residual=identity, act=True)          # relu(bn2(conv2(out)) + identity) in conv2's BN-apply kernel


class Bottleneck(nn.Module):

    def __init__(self, inplanes, planes, kernel_size, stride, padding):
        super(Bottleneck, self).__init__()
        self.downsample = _downsample(stride, inplanes, planes * 4)
        self.conv1 = ConvBnActBlock(inplanes, planes, kernel_size=1, stride=1, padding=0, groups=1, has_bn=True, has_act=True)
        self.conv2 = ConvBnActBlock(planes, planes, kernel_size=kernel_size, stride=stride, padding=padding, groups=1,
                                    has_bn=True, has_act=True)
        self.conv3 = ConvBnActBlock(planes, planes * 4, kernel_size=1, stride=1, padding=0, groups=1, has_bn=True, has_act=False)
        self.relu = nn.ReLU(inplace=True)
        if self.downsample:
            self.downsample_conv = ConvBnActBlock(inplanes, planes * 4, kernel_size=1, stride=stride, padding=0, groups=1,
                                                  has_bn=True, has_act=False)

    def forward(self, x):
        out = self.conv2(self.conv1(x))
        identity = self.downsample_conv(x) if self.downsample else x
        return self.conv3(out, residual=identity, act=True)


class ResNetBackbone(nn.Module):

    def __init__(self, block, layer_nums, inplanes=64, use_gradient_checkpoint=False):
        super(ResNetBackbone, self).__init__()
        self.block = block
        self.layer_nums = layer_nums
        self.inplanes = inplanes
        self.planes = [inplanes, inplanes * 2, inplanes * 4, inplanes * 8]
        self.expansion = 1 if block is BasicBlock else 4
        self.use_gradient_checkpoint = use_gradient_checkpoint

        self.conv1 = ConvBnActBlock(3, self.inplanes, kernel_size=7, stride=2, padding=3, groups=1, has_bn=True, has_act=True)
        self.maxpool1 = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self.make_layer(self.block, self.planes[0], self.layer_nums[0], kernel_size=3, stride=1, padding=1)
        self.layer2 = self.make_layer(self.block, self.planes[1], self.layer_nums[1], kernel_size=3, stride=2, padding=1)
        self.layer3 = self.make_layer(self.block, self.planes[2], self.layer_nums[2], kernel_size=(3, 1), stride=(2, 1),
                                      padding=(1, 0))
        self.layer4 = self.make_layer(self.block, self.planes[3], self.layer_nums[3], kernel_size=(3, 1), stride=(2, 1),
                                      padding=(1, 0))
        self.out_channels = [p * self.expansion for p in self.planes]
        _init_like_reference(self)

    def make_layer(self, block, planes, layer_nums, kernel_size, stride, padding):
        layers = []
        for i in range(0, layer_nums):
            if i == 0:
                layers.append(block(self.inplanes, planes, kernel_size, stride, padding))
            else:
                layers.append(block(self.inplanes, planes, kernel_size=3, stride=1, padding=1))
            self.inplanes = planes * self.expansion
        return nn.Sequential(*layers)

    def forward(self, x):
        x = ops.pack_stem_input(x, self.conv1.layer[0])
        x = self.conv1(x)
        mp = self.maxpool1
        x = ops.max_pool2d(x, mp.kernel_size, mp.stride, mp.padding)
        outs = []
        for stage in (self.layer1, self.layer2, self.layer3, self.layer4):
            x = checkpoint(stage, x, use_reentrant=False) if self.use_gradient_checkpoint else stage(x)
            outs.append(x)
        return outs


def _resnetbackbone(block, layers, inplanes, pretrained_path='', **kwargs):
    model = ResNetBackbone(block, layers, inplanes, **kwargs)
    if pretrained_path:
        load_state_dict(pretrained_path, model)
    else:
        print('no backbone pretrained model!')
    return model


def resnet18backbone(pretrained_path='', **kwargs):
    return _resnetbackbone(BasicBlock, [2, 2, 2, 2], 64, pretrained_path=pretrained_path, **kwargs)


def resnet34backbone(pretrained_path='', **kwargs):
    return _resnetbackbone(BasicBlock, [3, 4, 6, 3], 64, pretrained_path=pretrained_path, **kwargs)


def resnet50backbone(pretrained_path='', **kwargs):
    return _resnetbackbone(Bottleneck, [3, 4, 6, 3], 64, pretrained_path=pretrained_path, **kwargs)


def resnet101backbone(pretrained_path='', **kwargs):
    return _resnetbackbone(Bottleneck, [3, 4, 23, 3], 64, pretrained_path=pretrained_path, **kwargs)


def resnet152backbone(pretrained_path='', **kwargs):
    return _resnetbackbone(Bottleneck, [3, 8, 36, 3], 64, pretrained_path=pretrained_path, **kwargs)
