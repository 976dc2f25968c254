"""SAM matting (a SAM whose every mask output is refined into an alpha matte) on the MI355X kernels -- drop-in for the reference
module SimpleAICV/interactive_segmentation/models/segment_anything_matting/sam_matting.py (FUSION :89, SAMMATTING :305, factories
sam_b_matting / sam_l_matting / sam_h_matting :522-552).

Interface contract: same constructor arguments, module tree and state_dict keys (`image_encoder.*`, `prompt_encoder.*`,
`mask_decoder.*`, `fusion_pred_list.{i}.{global,local}_*.layer.{0,1}.*`, `fusion_pred_list.{i}.{global,local}_pred_conv.*`), and
`forward`, `forward_image_encoder`, `forward_prompt_encoder_mask_decoder`, `collaborative_matting`.  Outputs are
(global_preds [B, M, 3, S, S], local_preds [B, M, 1, S, S], fused_preds [B, M, 1, S, S], iou_preds [B, M]), fp32 probabilities, S
the image size; `fusion_pred_list` is indexed by the mask index, so `mask_out_idxs=[1, 3]` runs heads 1 and 3.

Execution: FUSION is built from the blocks of the PFAN models (`ConvBnActBlock`, `ConvTransposeBnActBlock`, `_resize`, the one-channel
3x3 + sigmoid head `ops.conv3x3_c1`, `ops.collaborative_matting`); no convolution kernel is new.  The two combine convolutions read a
concatenation that ends in the one-channel mask (65 and 129 channels); the concatenation is padded with zero channels to whole 16-byte
chunks and the weight with zero columns, which leaves the product and both gradients as they are."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..... import ops
from ....semantic_segmentation.models.pfan_semantic_segmentation import ConvBnActBlock, ConvTransposeBnActBlock, _resize
from ..segment_anything.image_encoder import ViTImageEncoder
from ..segment_anything.prompt_encoder import PromptEncoder
from .mask_decoder_matting import MaskDecoderMatting

__all__ = [
    'sam_b_matting',
    'sam_l_matting',
    'sam_h_matting',
]

CHUNK = 8


def _combine(block, parts):
    """block (a 1x1 ConvBnActBlock) on the channel concatenation of parts, whose channel count need not be whole chunks"""
    dt = ops.compute_dtype()
    parts = [ops._nhwc(t, dt) for t in parts]
    c = sum(t.shape[1] for t in parts)
    pad = -c % CHUNK
    weight = block.layer[0].weight
    if pad:
        b, _, h, w = parts[0].shape
        parts.append(torch.zeros((b, h, w, pad), dtype=dt, device=parts[0].device).permute(0, 3, 1, 2))
        weight = F.pad(weight, (0, 0, 0, 0, 0, pad))
    return ops.conv_bn_act(torch.cat(parts, dim=1), weight, block.layer[1], block.stride, block.padding, block.has_act)


class FUSION(nn.Module):

    def __init__(self, planes=[32, 256], cpfe_planes=32):
        super(FUSION, self).__init__()
        p = cpfe_planes

        def block(cin, k, act):
            return ConvBnActBlock(cin, p, kernel_size=k, stride=1, padding=k // 2, groups=1, dilation=1, has_bn=True, has_act=act)

        def up():
            return ConvTransposeBnActBlock(p, p, kernel_size=2, stride=2, groups=1, has_bn=True, has_act=True)

        # (construction order = the reference's: it fixes the order the initial weights are drawn in)
        self.global_feat3_reduce_conv = block(planes[-1], 1, True)
        self.global_feat1_reduce_conv = block(planes[-2], 1, True)
        self.global_combine_conv = block(2 * p + 1, 1, False)
        self.global_reduce_conv = block(p, 1, True)
        self.global_upsample_conv1 = up()
        self.global_upsample_conv2 = block(p, 3, True)
        self.global_upsample_conv3 = up()
        self.global_pred_conv = nn.Conv2d(p, 3, kernel_size=3, stride=1, padding=1, bias=True)

        self.local_feat3_reduce_conv = block(planes[-1], 1, True)
        self.local_feat1_reduce_conv = block(planes[-2], 1, True)
        self.local_combine_conv = block(4 * p + 1, 1, False)
        self.local_reduce_conv = block(p, 1, True)
        self.local_upsample_conv1 = up()
        self.local_upsample_conv2 = block(p, 3, True)
        self.local_upsample_conv3 = up()
        self.local_pred_conv = nn.Conv2d(p, 1, kernel_size=3, stride=1, padding=1, bias=True)

        self.sigmoid = nn.Sigmoid()
        self.head_route = 'fused' if ops.conv3x3_c1_supports(p) else 'generic'

    def forward(self, batch_masks, batch_feat3, batch_feat1):
        """batch_masks [B, 1, s, s] mask logits, batch_feat3 [B, planes[-1], s / 4, s / 4], batch_feat1 [B, planes[-2], s, s]
        -> global_pred [B, 3, 4s, 4s], local_pred [B, 1, 4s, 4s], fp32 probabilities"""
        size1 = batch_feat1.shape[2:]
        feat3_g = _resize(self.global_feat3_reduce_conv(batch_feat3), size1)
        feat1_g = _combine(self.global_feat1_reduce_conv, [batch_feat1])      # (planes[-2] may be less than a chunk)
        feats = self.global_reduce_conv(_combine(self.global_combine_conv, [feat1_g, feat3_g, batch_masks]))
        feats = self.global_upsample_conv3(self.global_upsample_conv2(self.global_upsample_conv1(feats)))
        global_pred = ops.conv2d(feats, self.global_pred_conv.weight, self.global_pred_conv.bias, 1, 1)
        global_pred = torch.sigmoid(global_pred.float())

        # the local decoder also reads the global decoder's two reduced maps
        feat3_l = _resize(self.local_feat3_reduce_conv(batch_feat3), size1)
        feat1_l = _combine(self.local_feat1_reduce_conv, [batch_feat1])
        feats = self.local_reduce_conv(_combine(self.local_combine_conv, [feat1_l, feat3_l, feat1_g, feat3_g, batch_masks]))
        feats = self.local_upsample_conv3(self.local_upsample_conv2(self.local_upsample_conv1(feats)))
        if self.head_route == 'fused':
            local_pred = ops.conv3x3_c1(feats, self.local_pred_conv.weight, self.local_pred_conv.bias, sigmoid=True)
        else:
            local_pred = ops.conv2d(feats, self.local_pred_conv.weight, self.local_pred_conv.bias, 1, 1)
            local_pred = torch.sigmoid(local_pred.float()).contiguous()
        return global_pred, local_pred


class SAMMATTING(nn.Module):

    def __init__(self, image_size=1024, patch_size=16, inplanes=3, image_encoder_embedding_planes=768,
                 image_encoder_block_nums=12, image_encoder_head_nums=12, image_encoder_mlp_ratio=4,
                 image_encoder_window_size=14, image_encoder_global_attn_indexes=[2, 5, 8, 11],
                 prompt_encoder_embedding_planes=256, prompt_encoder_mask_inter_planes=16,
                 mask_decoder_num_multimask_outputs=3, mask_decoder_iou_prediction_head_block_nums=3,
                 mask_decoder_iou_prediction_head_hidden_planes=256, matting_planes=[32, 256], matting_cpfe_planes=32,
                 use_gradient_checkpoint=False, frozen_image_encoder=False, frozen_prompt_encoder=False,
                 frozen_mask_decoder=False):
        super(SAMMATTING, self).__init__()
        self.image_encoder = ViTImageEncoder(
            image_size=image_size, patch_size=patch_size, inplanes=inplanes,
            embedding_planes=image_encoder_embedding_planes, block_nums=image_encoder_block_nums,
            head_nums=image_encoder_head_nums, mlp_ratio=image_encoder_mlp_ratio,
            out_planes=prompt_encoder_embedding_planes, window_size=image_encoder_window_size,
            global_attn_indexes=image_encoder_global_attn_indexes, use_gradient_checkpoint=use_gradient_checkpoint)
        self.prompt_encoder = PromptEncoder(image_size=image_size, patch_size=patch_size,
                                            embedding_planes=prompt_encoder_embedding_planes,
                                            mask_inter_planes=prompt_encoder_mask_inter_planes)
        self.mask_decoder = MaskDecoderMatting(
            inplanes=prompt_encoder_embedding_planes, num_multimask_outputs=mask_decoder_num_multimask_outputs,
            iou_prediction_head_block_nums=mask_decoder_iou_prediction_head_block_nums,
            iou_prediction_head_hidden_planes=mask_decoder_iou_prediction_head_hidden_planes)

        self.num_mask_tokens = mask_decoder_num_multimask_outputs + 1
        self.fusion_pred_list = nn.ModuleList(
            [FUSION(planes=matting_planes, cpfe_planes=matting_cpfe_planes) for _ in range(self.num_mask_tokens)])
        self.sigmoid = nn.Sigmoid()

        if frozen_image_encoder:
            for param in self.image_encoder.parameters():
                param.requires_grad = False
        if frozen_prompt_encoder:
            for param in self.prompt_encoder.parameters():
                param.requires_grad = False
        if frozen_mask_decoder:
            for param in self.mask_decoder.parameters():
                param.requires_grad = False

    def forward(self, batch_images, batch_prompts, mask_out_idxs=[0, 1, 2, 3]):
        return self.forward_prompt_encoder_mask_decoder(self.image_encoder(batch_images), batch_prompts,
                                                        mask_out_idxs=mask_out_idxs)

    def forward_image_encoder(self, batch_images):
        return self.image_encoder(batch_images)

    def forward_prompt_encoder_mask_decoder(self, batch_image_embeddings, batch_prompts, mask_out_idxs=[0, 1, 2, 3]):
        device = batch_image_embeddings.device
        points = batch_prompts['prompt_point']
        boxes = batch_prompts['prompt_box']
        mask = batch_prompts['prompt_mask']
        points = points.to(device) if points is not None else None
        boxes = boxes.to(device) if boxes is not None else None
        mask = mask.to(device) if mask is not None else None
        sparse_embeddings, dense_embeddings = self.prompt_encoder(points=points, boxes=boxes, masks=mask)
        mask_preds, iou_preds, feat3, feat1 = self.mask_decoder(image_embeddings=batch_image_embeddings,
                                                                image_pe=self.prompt_encoder.get_dense_pe_layer(),
                                                                sparse_prompt_embeddings=sparse_embeddings,
                                                                dense_prompt_embeddings=dense_embeddings,
                                                                mask_out_idxs=mask_out_idxs)
        global_preds, local_preds, fused_preds = [], [], []
        for idx, mask_out_idx in enumerate(mask_out_idxs):
            global_pred, local_pred = self.fusion_pred_list[mask_out_idx](mask_preds[:, idx:idx + 1, :, :], feat3, feat1)
            global_preds.append(global_pred)
            local_preds.append(local_pred)
            fused_preds.append(self.collaborative_matting(global_pred, local_pred))
        global_preds = torch.stack(global_preds, dim=1)
        local_preds = torch.stack(local_preds, dim=1)
        fused_preds = torch.stack(fused_preds, dim=1)
        return global_preds, local_preds, fused_preds, torch.sigmoid(iou_preds.float())

    def collaborative_matting(self, global_pred, local_pred):
        # class 0 background, 1 the local (unknown) region, 2 the global foreground
        if global_pred.is_cuda:
            return ops.collaborative_matting(global_pred, local_pred)
        idx = torch.max(global_pred, dim=1)[1].unsqueeze(1)
        return local_pred * (idx == 1).float() + (idx == 2).float()


def _sam_matting(image_size, patch_size, image_encoder_embedding_planes, image_encoder_block_nums, image_encoder_head_nums,
                 image_encoder_global_attn_indexes, prompt_encoder_embedding_planes, **kwargs):
    return SAMMATTING(image_size=image_size, patch_size=patch_size,
                      image_encoder_embedding_planes=image_encoder_embedding_planes,
                      image_encoder_block_nums=image_encoder_block_nums, image_encoder_head_nums=image_encoder_head_nums,
                      image_encoder_global_attn_indexes=image_encoder_global_attn_indexes,
                      prompt_encoder_embedding_planes=prompt_encoder_embedding_planes, **kwargs)


def sam_b_matting(image_size=1024, patch_size=16, **kwargs):
    return _sam_matting(image_size=image_size, patch_size=patch_size, image_encoder_embedding_planes=768,
                        image_encoder_block_nums=12, image_encoder_head_nums=12,
                        image_encoder_global_attn_indexes=[2, 5, 8, 11], prompt_encoder_embedding_planes=256, **kwargs)


def sam_l_matting(image_size=1024, patch_size=16, **kwargs):
    return _sam_matting(image_size=image_size, patch_size=patch_size, image_encoder_embedding_planes=1024,
                        image_encoder_block_nums=24, image_encoder_head_nums=16,
                        image_encoder_global_attn_indexes=[5, 11, 17, 23], prompt_encoder_embedding_planes=256, **kwargs)


def sam_h_matting(image_size=1024, patch_size=16, **kwargs):
    return _sam_matting(image_size=image_size, patch_size=patch_size, image_encoder_embedding_planes=1280,
                        image_encoder_block_nums=32, image_encoder_head_nums=16,
                        image_encoder_global_attn_indexes=[7, 15, 23, 31], prompt_encoder_embedding_planes=256, **kwargs)
