"""Per-iteration SAM matting training loop of the reference tools/interactive_matting_scripts.py (train_sam_matting :22-330) on the
MI355X engine.

Loop semantics are kept: the prompt-type draw on the host (tools/interactive_segmentation_scripts._choose_prompts), one
image-encoder forward, one decoder pass plus decoder_iters refinement passes whose new prompts (an error-region click and the best
fused matte at 1/4 resolution) are sampled without gradient from the previous pass's fused_preds
(get_decoder_iters_prompt_points_and_prompt_mask with config.mask_threshold = 0.5 on probabilities), the matting criterion over all
passes, the inf / nan batch skip, gradient accumulation with `no_sync()`, gradient clipping, GradScaler, the per-iteration scheduler
and the reference log line with the eight loss terms.  train_sam_matting is a `step_fn` over the epoch engine (tools/loop.py,
run_epoch), so the differences are the engine's: the manual per-parameter all-reduce is the bucketed all-reduce, skip decisions stay
on the device and reach the host `host_sync_lag` iterations later, no per-iteration barrier.  The step runs eagerly (no
graph_inputs: the prompt draw decides the step's shape on the host, and the captured SAM step measured no gain on one GPU)."""
from ..engine import any_nonfinite
from .interactive_segmentation_scripts import _choose_prompts, frozen_parts_to_eval, get_decoder_iters_prompt_points_and_prompt_mask
from .loop import begin_training, run_epoch

LOSS_KEYS = ('global_pred_trimap_ce_loss', 'global_pred_trimap_iou_loss', 'local_pred_alpha_loss', 'local_pred_laplacian_loss',
             'fusion_pred_alpha_loss', 'fusion_pred_laplacian_loss', 'composition_loss', 'iou_predict_loss')


def train_sam_matting(train_loader, model, criterion, optimizer, scheduler, epoch, logger, config):
    device, amp = begin_training(model, logger, config)
    frozen_parts_to_eval(model, config)
    net = model.module

    def step_fn(data):
        """image encoder, 1 + decoder_iters decoder passes, the criterion"""
        images = data['image'].to(device, non_blocking=True)
        targets = tuple(data[k].to(device, non_blocking=True) for k in ('mask', 'trimap', 'fg_map', 'bg_map'))
        prompts, decoder_iters = _choose_prompts(config, data['prompt_point'], data['prompt_box'], data['prompt_mask'], device)
        bad = any_nonfinite(images)
        with amp():
            embeddings = net.forward_image_encoder(images)
            outs = net.forward_prompt_encoder_mask_decoder(embeddings, prompts, mask_out_idxs=config.mask_out_idxs)
        all_iter = [[o] for o in outs]
        for _ in range(decoder_iters):
            prompts = get_decoder_iters_prompt_points_and_prompt_mask(outs[2], outs[3], targets[0], prompts, config)
            with amp():
                outs = net.forward_prompt_encoder_mask_decoder(embeddings, prompts, mask_out_idxs=config.mask_out_idxs)
            for acc, o in zip(all_iter, outs):
                acc.append(o)
        with amp():
            loss_value = criterion(images, all_iter, list(targets))
        return bad, loss_value, images.size(0)

    # (the total of the eight terms stays the chain of adds in the criterion's order that this loop has always formed)
    return run_epoch(train_loader, model, optimizer, scheduler, epoch, logger, config, step_fn, 'loss', 6,
                     term_names=LOSS_KEYS, chained_total=True, ema=False)
