"""Training / evaluation loops of the universal-matting family (reference tools/universal_matting_scripts.py):

  validate_human_matting_for_all_dataset    (reference :174-190)
  validate_human_matting                    (reference :193-302)
  train_universal_matting                   (reference :305-500)

The training loop is a `step_fn` over tools.loop.run_epoch: the reference's accumulation with `no_sync()`, the skip of a batch
whose loss is zero, inf or NaN (which is what UniversalMattingLoss returns when nothing was matched), clipping, scaler, EMA,
per-iteration scheduler and its log line (`total_loss`, then the seven loss names).  The step runs eagerly: the Hungarian
assignment needs the cost matrix on the host once per step.  Evaluation is tools.human_matting_scripts.EvalMeter over
tools.loop.timed_eval_pass on the decoder's best matte per image (config.decoder keeps topk = 1), an image that keeps no query
counting as an all-zero matte; the resize back to the scaled size is torch's bilinear one (the reference calls cv2.resize)."""
import collections

import numpy as np
import torch
import torch.nn.functional as F

from ..engine import any_nonfinite
from .human_matting_scripts import EvalMeter
from .loop import begin_training, for_all_datasets, run_epoch, timed_eval_pass


def validate_human_matting(test_loader, model, decoder, config):
    eval_metric = EvalMeter(config)

    def batch_fn(model, data, device):
        images, masks, sizes, origin_sizes = data['image'].to(device), data['mask'].to(device), data['size'], data['origin_size']
        yield
        outs = model(images)
        batch_masks, _, _ = decoder(outs, sizes, origin_sizes)
        yield
        mask_h, mask_w = masks.shape[1], masks.shape[2]
        outputs = torch.zeros((len(batch_masks), 1, mask_h, mask_w), dtype=torch.float32, device=device)
        for i, (mattes, size) in enumerate(zip(batch_masks, sizes)):
            if len(mattes) == 0:
                continue
            h, w = int(size[0]), int(size[1])
            matte = torch.from_numpy(np.squeeze(mattes, axis=0)).to(device)
            if tuple(matte.shape) != (h, w):
                matte = F.interpolate(matte[None, None], size=[h, w], mode='bilinear')[0, 0]
            outputs[i, 0, 0:h, 0:w] = matte
        eval_metric.add_batch_result(outputs, masks)

    load_ms, inference_ms = timed_eval_pass(test_loader, model, config, batch_fn)
    eval_metric.compute_all_metrics()
    result_dict = collections.OrderedDict()
    result_dict['per_image_load_time'] = f'{load_ms:.3f}ms'
    result_dict['per_image_inference_time'] = f'{inference_ms:.3f}ms'
    for key, attr in (('f_squared_beta_average', 'f_squared_beta_average'), ('f_squared_beta_max', 'f_squared_beta_max'),
                      ('mean_precision', 'precision_average'), ('mean_recall', 'recall_average'), ('max_precision', 'precision_max'),
                      ('max_recall', 'recall_max'), ('miou_average', 'miou_average'), ('miou_max', 'miou_max'), ('sad', 'sad'),
                      ('mae', 'mae'), ('mse', 'mse'), ('grad', 'grad'), ('conn', 'conn')):
        result_dict[key] = getattr(eval_metric, attr)
    return result_dict


validate_human_matting_for_all_dataset = for_all_datasets(validate_human_matting)


def train_universal_matting(train_loader, model, criterion, optimizer, scheduler, epoch, logger, config):
    '''train universal matting model for one epoch (reference tools/universal_matting_scripts.py:305-500):
    `global_preds, local_preds, fused_preds, class_preds = model(images)`, `criterion(global_preds, local_preds, fused_preds,
    class_preds, trimaps, masks, labels)`, and the log line `train: epoch 0001, iter [00010, 00157], lr: 0.000400, total_loss: 3.1875,
    global_trimap_ce_loss: ..., ..., class_loss: ..., `.'''
    device, amp = begin_training(model, logger, config)

    def step_fn(data):
        images = data['image'].to(device, non_blocking=True)
        masks = [m.to(device, non_blocking=True) for m in data['mask']]
        trimaps = [t.to(device, non_blocking=True) for t in data['trimap']]
        labels = [l.to(device, non_blocking=True) for l in data['label']]
        bad = any_nonfinite(images)
        with amp():
            global_preds, local_preds, fused_preds, class_preds = model(images)
            loss_value = criterion(global_preds, local_preds, fused_preds, class_preds, trimaps, masks, labels)
        return bad, loss_value, images.size(0)

    return run_epoch(train_loader, model, optimizer, scheduler, epoch, logger, config, step_fn, 'total_loss', 5)
