"""The encoder-only mask transformer (EoMT) on a DINOv3 ViT -- drop-in for the reference's
SimpleAICV/universal_segmentation/models/dinov3_universal_segmentation.py (ScaleBlock :29, UniversalSegmentation :64, factories
:182-215): same constructor arguments, parameter names, registration and random-draw order, so seeds and checkpoints carry over.

The learned queries are concatenated in front of the patch tokens before block `block_nums - query_block_nums`; from there on
ops_tfm.rope leaves that token prefix unrotated (the backbone's SelfAttention passes the prefix length).  predict() runs on
the package's kernels: the class and query projections are linear_nd (+ gelu), a ScaleBlock is the SAM decoder's 2x2
transposed-convolution helper, gelu, the depthwise 3x3 and a LayerNorm over NHWC memory; the `bqc,bchw->bqhw` product is one
batched matmul on the token layout, and the resize to image_size is ops_tfm.upsample4_bilinear when it is the usual factor 4
(patch 16: two ScaleBlocks) and F.interpolate otherwise."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

from .... import ops, ops_tfm
from ...detection.models import backbones
from ...interactive_segmentation.models.segment_anything.mask_decoder import _conv_transpose_2x2

__all__ = [
    'dinov3_vit_small_patch16_universal_segmentation',
    'dinov3_vit_small_plus_patch16_universal_segmentation',
    'dinov3_vit_base_patch16_universal_segmentation',
    'dinov3_vit_large_patch16_universal_segmentation',
    'dinov3_vit_large_plus_patch16_universal_segmentation',
    'dinov3_vit_huge_plus_patch16_universal_segmentation',
]


class ScaleBlock(nn.Module):
    """ConvTranspose2d(2, 2) -> GELU -> depthwise 3x3 -> LayerNorm over channels, on [B, H, W, C] tokens (NHWC memory)."""

    def __init__(self, inplanes):
        super(ScaleBlock, self).__init__()
        self.conv1 = nn.ConvTranspose2d(inplanes, inplanes, kernel_size=2, stride=2, padding=0, output_padding=0, bias=True)
        self.act = nn.GELU()
        self.conv2 = nn.Conv2d(inplanes, inplanes, kernel_size=3, padding=1, groups=inplanes, bias=False)
        self.norm = nn.LayerNorm(inplanes)

    def forward(self, x):
        x = ops_tfm.gelu(_conv_transpose_2x2(x, self.conv1))
        x = ops.depthwise_conv2d(x.permute(0, 3, 1, 2), self.conv2.weight, None, 1, 1)           # NCHW-shaped view of NHWC memory
        return ops_tfm.layer_norm(x.permute(0, 2, 3, 1), self.norm.weight, self.norm.bias, self.norm.eps)


class UniversalSegmentation(nn.Module):
    """num_classes counts the background (no-object) class."""

    def __init__(self, backbone_type, backbone_pretrained_path='', image_size=512, query_num=100, num_classes=151,
                 query_block_nums=4, use_gradient_checkpoint=False):
        super(UniversalSegmentation, self).__init__()
        self.image_size = image_size
        self.query_num = query_num
        self.num_classes = num_classes
        self.query_block_nums = query_block_nums
        self.use_gradient_checkpoint = use_gradient_checkpoint

        self.backbone = backbones.__dict__[backbone_type](**{
            'pretrained_path': backbone_pretrained_path,
            'use_gradient_checkpoint': use_gradient_checkpoint,
        })
        embedding_planes = self.backbone.out_channels
        patch_size = self.backbone.patch_size
        self.grid_size = image_size // patch_size
        self.block_nums = len(self.backbone.blocks)

        self.query_embedding = nn.Embedding(query_num, embedding_planes)
        self.class_pred = nn.Linear(embedding_planes, num_classes)
        self.query_proj = nn.Sequential(nn.Linear(embedding_planes, embedding_planes), nn.GELU(),
                                        nn.Linear(embedding_planes, embedding_planes), nn.GELU(),
                                        nn.Linear(embedding_planes, embedding_planes))
        upscale_blocks_num = max(1, int(math.log2(patch_size)) - 2)
        self.upscale_blocks = nn.ModuleList([ScaleBlock(embedding_planes) for _ in range(upscale_blocks_num)])

    def predict(self, x):
        q = x[:, :self.query_num, :]
        class_preds = ops_tfm.linear_nd(q, self.class_pred.weight, self.class_pred.bias)
        b, c = x.shape[0], x.shape[2]
        x = x[:, self.query_num:, :].reshape(b, self.grid_size, self.grid_size, c)               # [B, h, w, C]
        for i in (0, 2):
            q = ops_tfm.gelu(ops_tfm.linear_nd(q, self.query_proj[i].weight, self.query_proj[i].bias))
        q = ops_tfm.linear_nd(q, self.query_proj[4].weight, self.query_proj[4].bias)
        for block in self.upscale_blocks:
            if self.use_gradient_checkpoint:
                x = checkpoint(block, x, use_reentrant=False)
            else:
                x = block(x)
        h, w = x.shape[1], x.shape[2]
        # mask_preds[b, q, y, x] = <q[b, q, :], x[b, y, x, :]>: the reference's einsum on the token layout
        mask_preds = torch.bmm(q, x.reshape(b, h * w, c).to(q.dtype).transpose(1, 2)).view(b, self.query_num, h, w)
        if self.image_size == 4 * h and self.image_size == 4 * w:
            mask_preds = ops_tfm.upsample4_bilinear(mask_preds)
        else:
            mask_preds = F.interpolate(mask_preds, (self.image_size, self.image_size), mode="bilinear")
        return mask_preds, class_preds

    def forward(self, x):
        x = self.backbone.patch_embed(x)                                                         # [B, h, w, C]
        _, H, W, _ = x.shape
        x = x.flatten(1, 2)
        rope_sincos = self.backbone.rope_embed(H=H, W=W)
        for idx, block in enumerate(self.backbone.blocks):
            if idx == self.block_nums - self.query_block_nums:
                queries = self.query_embedding.weight[None, :, :].expand(x.shape[0], -1, -1)
                x = torch.cat([queries.to(x.dtype), x], dim=1)
            if self.use_gradient_checkpoint:
                x = checkpoint(block, x, rope_sincos, use_reentrant=False)
            else:
                x = block(x, rope_sincos)
        norm = self.backbone.norm
        return self.predict(ops_tfm.layer_norm(x, norm.weight, norm.bias, norm.eps))


def _universal_segmentation(backbone_type, backbone_pretrained_path, **kwargs):
    return UniversalSegmentation(backbone_type=backbone_type, backbone_pretrained_path=backbone_pretrained_path, **kwargs)


def dinov3_vit_small_patch16_universal_segmentation(backbone_pretrained_path='', **kwargs):
    return _universal_segmentation('dinov3_vit_small_patch16_backbone', backbone_pretrained_path, **kwargs)


def dinov3_vit_small_plus_patch16_universal_segmentation(backbone_pretrained_path='', **kwargs):
    return _universal_segmentation('dinov3_vit_small_plus_patch16_backbone', backbone_pretrained_path, **kwargs)


def dinov3_vit_base_patch16_universal_segmentation(backbone_pretrained_path='', **kwargs):
    return _universal_segmentation('dinov3_vit_base_patch16_backbone', backbone_pretrained_path, **kwargs)


def dinov3_vit_large_patch16_universal_segmentation(backbone_pretrained_path='', **kwargs):
    return _universal_segmentation('dinov3_vit_large_patch16_backbone', backbone_pretrained_path, **kwargs)


def dinov3_vit_large_plus_patch16_universal_segmentation(backbone_pretrained_path='', **kwargs):
    return _universal_segmentation('dinov3_vit_large_plus_patch16_backbone', backbone_pretrained_path, **kwargs)


def dinov3_vit_huge_plus_patch16_universal_segmentation(backbone_pretrained_path='', **kwargs):
    return _universal_segmentation('dinov3_vit_huge_plus_patch16_backbone', backbone_pretrained_path, **kwargs)
