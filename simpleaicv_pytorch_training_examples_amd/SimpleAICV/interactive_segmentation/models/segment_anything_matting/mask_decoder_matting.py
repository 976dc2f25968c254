"""SAM mask decoder that also hands out the two feature maps the matting heads read -- drop-in for the reference module
SimpleAICV/interactive_segmentation/models/segment_anything_matting/mask_decoder_matting.py (MaskDecoderMatting :19): the
parameters, their names and the execution are MaskDecoder's (../segment_anything/mask_decoder.py).

forward(...) -> (mask_preds [B, M, 4h, 4w], iou_preds [B, M], feat3 [B, C, h, w], feat1 [B, C / 8, 4h, 4w]): feat3 is the two-way
transformer's image tokens as a map, feat1 the upscaled embedding; both NCHW-shaped over NHWC memory, views of tensors the decoder
holds anyway (the reference clones them; nothing here writes into them)."""
import torch

from ..... import ops_tfm
from ..segment_anything.mask_decoder import _INDEX_CACHE, MaskDecoder, _conv_transpose_2x2


class MaskDecoderMatting(MaskDecoder):

    def forward(self, image_embeddings, image_pe, sparse_prompt_embeddings, dense_prompt_embeddings,
                mask_out_idxs=[0, 1, 2, 3]):
        output_tokens = torch.cat([self.iou_token.weight, self.mask_tokens.weight], dim=0)
        output_tokens = output_tokens.unsqueeze(0).expand(sparse_prompt_embeddings.size(0), -1, -1)
        tokens = torch.cat((output_tokens, sparse_prompt_embeddings), dim=1)

        if image_embeddings.shape[0] != tokens.shape[0]:        # one image feature for several prompts
            src = torch.repeat_interleave(image_embeddings, tokens.shape[0], dim=0)
        else:
            src = image_embeddings
        src = (src + dense_prompt_embeddings.to(src.dtype)).contiguous(memory_format=torch.channels_last)
        pos_src = torch.repeat_interleave(image_pe, tokens.shape[0], dim=0)
        b, c, h, w = src.shape

        hs, src = self.transformer(src, pos_src, tokens)        # src: [B, HW, C] tokens
        iou_token_out = hs[:, 0, :]
        mask_tokens_out = hs[:, 1:(1 + self.num_mask_tokens), :]

        up = self.output_upscaling
        src = src.reshape(b, h, w, c)
        feat3 = src.permute(0, 3, 1, 2)
        x = _conv_transpose_2x2(src, up[0])                                      # [B, 2H, 2W, C/4]
        x = ops_tfm.gelu(ops_tfm.layer_norm(x, up[1].weight, up[1].bias, up[1].eps))
        x = ops_tfm.gelu(_conv_transpose_2x2(x, up[3]))                         # [B, 4H, 4W, C/8]
        feat1 = x.permute(0, 3, 1, 2)
        hyper_in = torch.stack([self.output_hypernetworks_mlps[i](mask_tokens_out[:, i, :])
                                for i in range(self.num_mask_tokens)], dim=1)   # [B, T, C/8]
        b, h4, w4, c8 = x.shape
        mask_preds = ops_tfm.hyper_product(x.view(b, h4 * w4, c8), hyper_in).view(b, -1, h4, w4)
        iou_preds = self.iou_prediction_head(iou_token_out)
        idxs = [int(i) for i in mask_out_idxs]
        if idxs == list(range(mask_preds.shape[1])):
            return mask_preds, iou_preds, feat3, feat1
        if idxs == list(range(idxs[0], idxs[0] + len(idxs))):
            return mask_preds[:, idxs[0]:idxs[0] + len(idxs)], iou_preds[:, idxs[0]:idxs[0] + len(idxs)], feat3, feat1
        key = (tuple(idxs), mask_preds.device)
        sel = _INDEX_CACHE.get(key)
        if sel is None:
            sel = _INDEX_CACHE[key] = torch.tensor(idxs, dtype=torch.long, device=mask_preds.device)
        return mask_preds.index_select(1, sel), iou_preds.index_select(1, sel), feat3, feat1
