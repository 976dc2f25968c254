"""Per-iteration SAM matting training loop of the reference tools/interactive_matting_scripts.py (train_sam_matting :22-330) on the
MI355X engine.

Loop semantics are kept: the prompt-type draw on the host (tools/interactive_segmentation_scripts._choose_prompts), one
image-encoder forward, one decoder pass plus decoder_iters refinement passes whose new prompts (an error-region click and the best
fused matte at 1/4 resolution) are sampled without gradient from the previous pass's fused_preds
(get_decoder_iters_prompt_points_and_prompt_mask with config.mask_threshold = 0.5 on probabilities), the matting criterion over all
passes, the inf / nan batch skip, gradient accumulation with `no_sync()`, gradient clipping, GradScaler, the per-iteration scheduler
and the reference log line with the eight loss terms.  Differences, as in train_sam_segmentation: the manual per-parameter all-reduce
is the engine's bucketed all-reduce, skip decisions stay on the device and reach the host `host_sync_lag` iterations later, no
per-iteration barrier.  The step runs eagerly (the prompt draw decides the step's shape on the host, and the captured SAM step
measured no gain on one GPU)."""
import collections

import torch
from torch.amp.autocast_mode import autocast

from ..engine import any_nonfinite
from ..SimpleAICV.classification.common import AverageMeter, get_amp_type
from .interactive_segmentation_scripts import _choose_prompts, get_decoder_iters_prompt_points_and_prompt_mask
from .scripts import _device_of, all_reduce_sum_packed

LOSS_KEYS = ('global_pred_trimap_ce_loss', 'global_pred_trimap_iou_loss', 'local_pred_alpha_loss', 'local_pred_laplacian_loss',
             'fusion_pred_alpha_loss', 'fusion_pred_laplacian_loss', 'composition_loss', 'iou_predict_loss')


def train_sam_matting(train_loader, model, criterion, optimizer, scheduler, epoch, logger, config):
    losses = AverageMeter()
    model.train()
    if config.frozen_image_encoder:
        model.module.image_encoder.eval()
    if config.frozen_prompt_encoder:
        model.module.prompt_encoder.eval()
    if config.frozen_mask_decoder:
        model.module.mask_decoder.eval()
    device = _device_of(model)
    amp_type = get_amp_type(model)
    local_rank = config.local_rank
    total_rank = getattr(config, 'total_rank', 0)
    main = local_rank == 0 and total_rank == 0
    if main:
        logger.info(f'use_amp: {config.use_amp}, amp_type: {amp_type}!')
    iters = len(train_loader.dataset) // config.batch_size
    iter_index = 1
    acc_steps = config.accumulation_steps
    assert acc_steps >= 1, 'illegal accumulation_steps!'
    lag = getattr(config, 'host_sync_lag', 2)
    scaler = getattr(config, 'scaler', None) if config.use_amp else None
    clip_norm = getattr(config, 'clip_max_norm', 0) or 0
    clip_value = getattr(config, 'clip_grad_value', 0) or 0
    pending = collections.deque()
    carried_bad = None
    net = model.module

    def drain(keep):
        nonlocal iter_index
        while len(pending) > keep:
            packed, n, log_fmt = pending.popleft()
            vals = packed.tolist()
            if vals[0]:
                if main:
                    logger.info('skip this batch!')
                iter_index -= 1
                continue
            loss = vals[1] / float(config.gpus_num)
            losses.update(loss, n)
            if log_fmt is not None and main:
                terms = ''.join(f'{k}: {v / float(config.gpus_num) * acc_steps:.4f}, ' for k, v in zip(LOSS_KEYS, vals[2:]))
                logger.info(log_fmt.format(loss=loss * acc_steps) + terms)

    def amp():
        return autocast(device_type=device.type, dtype=amp_type, enabled=bool(config.use_amp))

    def forward_backward(images, targets, prompts, decoder_iters, boundary):
        """image encoder, 1 + decoder_iters decoder passes, the criterion, (scaled) backward -> packed [skip, loss / acc, terms]"""
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
        loss = sum(loss_value.values())
        terms = torch.stack([loss_value[k].detach().float() for k in LOSS_KEYS]) / acc_steps
        bad = bad | (loss == 0.) | ~torch.isfinite(loss) | ~torch.isfinite(terms).all()
        loss = loss / acc_steps
        scaled = scaler.scale(loss) if scaler is not None else loss
        if boundary:
            scaled.backward()
        else:
            with model.no_sync():
                scaled.backward()
        packed = torch.cat([torch.stack([bad.float(), loss.detach().float()]), terms])
        all_reduce_sum_packed(packed, model, config.group)
        return packed

    def update(packed):
        model.finish_gradient_sync()
        skip_flag = packed[0:1]
        if getattr(config, 'skip_inf_nan_grad', False) or scaler is not None:
            optimizer.check_finite()
            skip_flag = torch.maximum(skip_flag, optimizer.found_inf)
        inv_scale = scaler.state[2:3] if scaler is not None else None
        if clip_value > 0:
            optimizer.clip_grad_value_(clip_value, inv_scale)
            inv_scale = None
        if clip_norm > 0:
            optimizer.clip_grad_norm_(clip_norm, inv_scale)
            inv_scale = None
        optimizer.step(inv_scale, skip_flag)
        if scaler is not None:
            scaler._found_inf = optimizer.found_inf
            scaler.update()
        optimizer.zero_grad()

    micro = 0      # accumulation phase by issued micro-batch (see tools/scripts.py train_classification)
    for data in train_loader:
        micro += 1
        images = data['image'].to(device, non_blocking=True)
        targets = tuple(data[k].to(device, non_blocking=True) for k in ('mask', 'trimap', 'fg_map', 'bg_map'))
        prompts, decoder_iters = _choose_prompts(config, data['prompt_point'], data['prompt_box'], data['prompt_mask'], device)
        boundary = micro % acc_steps == 0
        packed = forward_backward(images, targets, prompts, decoder_iters, boundary)
        if carried_bad is not None:
            packed = torch.cat([torch.maximum(packed[0:1], carried_bad), packed[1:]])
        carried_bad = None if boundary else packed[0:1]
        if boundary:
            update(packed)
            scheduler.step(optimizer, iter_index / iters + (epoch - 1))
            log_fmt = None
            if iter_index % int(config.print_interval * acc_steps) == 0:
                log_fmt = (f'train: epoch {epoch:0>4d}, iter [{int(iter_index // acc_steps):0>6d}, '
                           f'{int(iters // acc_steps):0>6d}], lr: {scheduler.current_lr:.6f}, ' + 'loss: {loss:.4f}, ')
            pending.append((packed, images.size(0), log_fmt))
        drain(lag)
        iter_index += 1
    drain(0)
    return losses.avg * acc_steps
