"""Training / evaluation loops of the universal-segmentation family (reference tools/universal_segmentation_scripts.py):

  test_semantic_segmentation_dataset    (reference :28-218)
  train_universal_segmentation          (reference :945-1124)

The training loop is a `step_fn` over tools.loop.run_epoch: the reference's accumulation with `no_sync()`, the skip of a batch
whose loss is zero, inf or NaN (which is what UniversalSegmentationLoss returns when nothing was matched), clipping, scaler, EMA,
per-iteration scheduler and its log line (`total_loss`, then mask_loss, dice_loss, class_loss).  The step runs eagerly: the
Hungarian assignment needs the cost matrix on the host once per step.  The instance / salient / parsing evaluation functions of the
reference file are not ported."""
import collections

import numpy as np
import torch

from ..engine import any_nonfinite
from .loop import begin_training, run_epoch, timed_eval_pass


def _nearest_resize(masks, h, w):
    """[N, H, W] -> [N, h, w], nearest neighbour with cv2.INTER_NEAREST's source index floor(dst * scale)"""
    n, sh, sw = masks.shape
    if (sh, sw) == (h, w):
        return masks
    ys = np.minimum((np.arange(h) * (sh / h)).astype(np.int64), sh - 1)
    xs = np.minimum((np.arange(w) * (sw / w)).astype(np.int64), sw - 1)
    return masks[:, ys][:, :, xs]


def test_semantic_segmentation_dataset(test_loader, model, decoder, config):
    nc = config.num_classes
    totals = torch.zeros((4, nc), dtype=torch.float64)                      # intersect, pred, gt, union

    def batch_fn(model, data, device):
        nonlocal totals
        images, masks, sizes, origin_sizes = data['image'].to(device), data['mask'].to(device), data['size'], data['origin_size']
        yield
        outs = model(images)
        batch_masks, batch_scores, batch_classes = decoder(outs, sizes, origin_sizes)
        yield
        totals = totals.to(device)
        for pred_masks, classes, gt, size in zip(batch_masks, batch_classes, masks, sizes):
            h, w = int(size[0]), int(size[1])
            pred = np.zeros((h, w), dtype=np.float32)
            if len(pred_masks) != 0:
                # predicted foreground classes start at 0, the label map's at 1; later (lower-scored) masks overwrite
                for per_mask, per_class in zip(_nearest_resize(pred_masks, h, w), classes + 1):
                    pred[per_mask > 0] = per_class
            pred = torch.from_numpy(pred).to(device).reshape(-1)
            gt = gt[0:h, 0:w].reshape(-1)
            hist = lambda t: torch.histc(t.float(), bins=nc, min=0, max=nc - 1).double()
            inter, area_pred, area_gt = hist(pred[pred == gt]), hist(pred), hist(gt)
            totals += torch.stack([inter, area_pred, area_gt, area_pred + area_gt - inter])

    load_ms, inference_ms = timed_eval_pass(test_loader, model, config, batch_fn)
    result_dict = collections.OrderedDict()
    result_dict['per_image_load_time'] = f'{load_ms:.3f}ms'
    result_dict['per_image_inference_time'] = f'{inference_ms:.3f}ms'
    inter, area_pred, area_gt, union = totals.cpu()
    exist = area_gt != 0
    ratio = lambda a, b: torch.where(b != 0, a / b.clamp_min(1e-300), torch.zeros_like(a)) * 100.
    metrics = {'mean_precision': ratio(inter, area_pred), 'mean_recall': ratio(inter, area_gt), 'mean_iou': ratio(inter, union),
               'mean_dice': 2. * ratio(inter, area_pred + area_gt)}
    exist_num_class = float(exist.sum())
    result_dict['exist_num_class'] = exist_num_class
    for name, per_class in metrics.items():
        result_dict[name] = per_class[exist].sum() / exist_num_class if exist_num_class > 0 else 0.
    return result_dict


def train_universal_segmentation(train_loader, model, criterion, optimizer, scheduler, epoch, logger, config):
    '''train universal segmentation model for one epoch (reference tools/universal_segmentation_scripts.py:945-1124):
    `mask_preds, class_preds = model(images)`, `criterion(mask_preds, class_preds, masks, labels)`, and the log line
    `train: epoch 0001, iter [00010, 00157], lr: 0.000400, total_loss: 61.8750, mask_loss: ..., dice_loss: ..., class_loss: ..., `.'''
    device, amp = begin_training(model, logger, config)

    def step_fn(data):
        images = data['image'].to(device, non_blocking=True)
        masks = [m.to(device, non_blocking=True) for m in data['mask']]
        labels = [l.to(device, non_blocking=True) for l in data['label']]
        bad = any_nonfinite(images)
        with amp():
            mask_preds, class_preds = model(images)
            loss_value = criterion(mask_preds, class_preds, masks, labels)
        return bad, loss_value, images.size(0)

    return run_epoch(train_loader, model, optimizer, scheduler, epoch, logger, config, step_fn, 'total_loss', 5)
