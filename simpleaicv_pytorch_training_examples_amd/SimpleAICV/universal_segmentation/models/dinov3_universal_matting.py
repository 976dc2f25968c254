"""The encoder-only mask transformer with matting heads on a DINOv3 ViT -- drop-in for the reference's
SimpleAICV/universal_segmentation/models/dinov3_universal_matting.py (ScaleBlock :29, UniversalMatting :64, factories :260-293): same
constructor arguments, parameter names, registration and random-draw order, so seeds and checkpoints carry over.

The backbone walk with the query prefix and the query / class projections are dinov3_universal_segmentation's.  The per-query mask
logits [B, h, w, Q] stay on the token (NHWC) layout: the global branch repeats every query channel three times (channel 3 q + c, the
reference's repeat_interleave(3, dim=1)) and both branches run two EoMT ScaleBlocks on NHWC memory.  ops.matting_head then reads the
[B, H, W, 3Q] and [B, H, W, Q] logits once and writes the three fp32 predictions once (csrc/unimat.hip); they are returned as
[B, Q, 3 | 1, H, W] views of that channels-last memory, which ops.matting_match_cost and ops.take_rows read in place."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

from .... import ops, ops_tfm
from ...detection.models import backbones
from .dinov3_universal_segmentation import ScaleBlock

__all__ = [
    'dinov3_vit_small_patch16_universal_matting',
    'dinov3_vit_small_plus_patch16_universal_matting',
    'dinov3_vit_base_patch16_universal_matting',
    'dinov3_vit_large_patch16_universal_matting',
    'dinov3_vit_large_plus_patch16_universal_matting',
    'dinov3_vit_huge_plus_patch16_universal_matting',
]


_BLOCK_ELEMENTS = 2 ** 29          # elements of a ScaleBlock's largest tensor per call (1 GiB in bf16)


def _scale_block(block, x):
    """ScaleBlock.forward for any channel count.  The GEMM and the depthwise kernel take channels in 16-byte chunks; 3Q and Q
    channels (300 and 100 in the reference config) are no multiple of 8, so such a block runs on zero-padded channels: padded
    weights give exact zeros there through the transposed convolution, GELU and the depthwise 3x3, and the LayerNorm sees the C
    real channels only, in fp32 (its kernel takes C as a multiple of 4 there; any other C goes to torch's LayerNorm)."""
    c = x.shape[-1]
    pad = (-c) % 8
    cp = c + pad
    b, h, w, _ = x.shape
    # the transposed convolution's output [B, h, w, 4 Cp] of the last global block is 5 GB at batch 8, 1024 x 1024, Q = 100, past the
    # 4 GiB a GEMM operand may span: such a block runs image group after image group
    group = max(1, _BLOCK_ELEMENTS // (h * w * 4 * cp))
    if b > group:
        return torch.cat([_scale_block(block, part) for part in x.split(group, dim=0)], dim=0)
    if pad == 0:
        return block(x)
    w1 = F.pad(block.conv1.weight, (0, 0, 0, 0, 0, pad, 0, pad))                                 # [Cp, Cp, 2, 2]
    y = ops_tfm.linear_nd(F.pad(x, (0, pad)), w1.permute(2, 3, 1, 0).reshape(4 * cp, cp), F.pad(block.conv1.bias, (0, pad)).repeat(4))
    y = ops_tfm.gelu(y.view(b, h, w, 2, 2, cp).permute(0, 1, 3, 2, 4, 5).reshape(b, 2 * h, 2 * w, cp))
    y = ops.depthwise_conv2d(y.permute(0, 3, 1, 2), F.pad(block.conv2.weight, (0, 0, 0, 0, 0, 0, 0, pad)), None, 1, 1)
    y = y.permute(0, 2, 3, 1)[..., :c]
    norm = block.norm
    if c % 4 == 0:                  # the LayerNorm kernel takes rows of whole 16-byte chunks: C = 100, 300 are that in fp32, not in bf16
        return ops_tfm.layer_norm(y.float().contiguous(), norm.weight, norm.bias, norm.eps).to(x.dtype)
    # a channel count that is no multiple of 4 (the tiny test models: Q = 5) has no kernel: torch's LayerNorm, in fp32
    return F.layer_norm(y.float(), (c, ), norm.weight.float(), norm.bias.float(), norm.eps).to(x.dtype)


class UniversalMatting(nn.Module):
    """num_classes counts the background (no-object) class."""

    def __init__(self, backbone_type, backbone_pretrained_path='', image_size=1024, query_num=100, num_classes=2, query_block_nums=4,
                 use_gradient_checkpoint=False):
        super(UniversalMatting, self).__init__()
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
        self.global_upscale_blocks = nn.ModuleList([ScaleBlock(query_num * 3) for _ in range(2)])
        self.local_upscale_blocks = nn.ModuleList([ScaleBlock(query_num) for _ in range(2)])
        self.sigmoid = nn.Sigmoid()

    def _run(self, blocks, x):
        for block in blocks:
            if self.use_gradient_checkpoint:
                x = checkpoint(_scale_block, block, x, use_reentrant=False)
            else:
                x = _scale_block(block, x)
        return x

    def predict(self, x):
        q = x[:, :self.query_num, :]
        class_preds = ops_tfm.linear_nd(q, self.class_pred.weight, self.class_pred.bias)
        b, c = x.shape[0], x.shape[2]
        x = x[:, self.query_num:, :].reshape(b, self.grid_size, self.grid_size, c)               # [B, h, w, C]
        for i in (0, 2):
            q = ops_tfm.gelu(ops_tfm.linear_nd(q, self.query_proj[i].weight, self.query_proj[i].bias))
        q = ops_tfm.linear_nd(q, self.query_proj[4].weight, self.query_proj[4].bias)
        x = self._run(self.upscale_blocks, x)
        h, w = x.shape[1], x.shape[2]
        # mask_preds[b, y, x, q] = <x[b, y, x, :], q[b, q, :]>: the reference's einsum, on the token layout
        mask_preds = torch.bmm(x.reshape(b, h * w, c).to(q.dtype), q.transpose(1, 2)).view(b, h, w, self.query_num)
        global_logits = self._run(self.global_upscale_blocks, torch.repeat_interleave(mask_preds, 3, dim=3))
        local_logits = self._run(self.local_upscale_blocks, mask_preds)
        global_preds, local_preds, fused_preds = ops.matting_head(global_logits.permute(0, 3, 1, 2), local_logits.permute(0, 3, 1, 2))
        return global_preds, local_preds, fused_preds, class_preds

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


def _universal_matting(backbone_type, backbone_pretrained_path, **kwargs):
    return UniversalMatting(backbone_type=backbone_type, backbone_pretrained_path=backbone_pretrained_path, **kwargs)


def dinov3_vit_small_patch16_universal_matting(backbone_pretrained_path='', **kwargs):
    return _universal_matting('dinov3_vit_small_patch16_backbone', backbone_pretrained_path, **kwargs)


def dinov3_vit_small_plus_patch16_universal_matting(backbone_pretrained_path='', **kwargs):
    return _universal_matting('dinov3_vit_small_plus_patch16_backbone', backbone_pretrained_path, **kwargs)


def dinov3_vit_base_patch16_universal_matting(backbone_pretrained_path='', **kwargs):
    return _universal_matting('dinov3_vit_base_patch16_backbone', backbone_pretrained_path, **kwargs)


def dinov3_vit_large_patch16_universal_matting(backbone_pretrained_path='', **kwargs):
    return _universal_matting('dinov3_vit_large_patch16_backbone', backbone_pretrained_path, **kwargs)


def dinov3_vit_large_plus_patch16_universal_matting(backbone_pretrained_path='', **kwargs):
    return _universal_matting('dinov3_vit_large_plus_patch16_backbone', backbone_pretrained_path, **kwargs)


def dinov3_vit_huge_plus_patch16_universal_matting(backbone_pretrained_path='', **kwargs):
    return _universal_matting('dinov3_vit_huge_plus_patch16_backbone', backbone_pretrained_path, **kwargs)
