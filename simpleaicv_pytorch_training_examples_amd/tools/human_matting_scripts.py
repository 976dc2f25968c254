"""Training / evaluation loops of the human-matting family (reference tools/human_matting_scripts.py):

  EvalMeter                                 (reference :26-171)
  validate_human_matting_for_all_dataset    (reference :174-191)
  validate_human_matting                    (reference :194-272)
  train_human_matting                       (reference :275-520)
  first_dataset_metric: what the entry script checkpoints by (reference tools/train_human_matting_model.py:215-235)

The training loop is a `step_fn` over tools.loop.run_epoch, evaluation the metric code over tools.loop.timed_eval_pass: the reference's skip / accumulation / clipping / scaler / EMA /
scheduler semantics and its log line with the seven loss names.  The criterion dict is routed as the reference routes it
(:320-346): the trimap losses read global_pred, the local losses local_pred + mask + trimap, the fusion losses fused_pred + mask,
CompositionLoss the image, the mask, fg_map, bg_map and fused_pred.  The iteration has static shapes and no host read (the fused
losses take their gradients as device tensors), so config.use_step_graph captures it whole."""
import collections

import numpy as np
import torch
from scipy.ndimage import gaussian_filter, label

from ..engine import any_nonfinite
from .loop import begin_training, for_all_datasets, run_epoch, timed_eval_pass
from .salient_object_detection_scripts import first_dataset_metric  # noqa: F401  (the same rule, one copy)

_FOUR_CONNECTED = [[0, 1, 0], [1, 1, 1], [0, 1, 0]]


class EvalMeter:
    """The reference's accumulator: precision / recall / IoU / F-measure per threshold and sad / mae / mse / grad / conn per image.
    The per-threshold foreground counts are taken on the tensors' device (three integers per sample and threshold) and come to the
    host once per batch; the five matting errors are the reference's numpy code on the host, per image, as the reference does.
    `cal_conn` needs the largest 4-connected component of a binary map: scipy.ndimage.label replaces
    cv2.connectedComponentsWithStats (both number components in scan order; np.argmax takes the first of equally large ones)."""

    def __init__(self, config):
        self.thresh = config.thresh
        self.squared_beta = config.squared_beta
        self.thresh_num = len(self.thresh)

        self.precision_list = np.zeros(self.thresh_num, dtype=np.float32)
        self.recall_list = np.zeros(self.thresh_num, dtype=np.float32)
        self.miou_list = np.zeros(self.thresh_num, dtype=np.float32)
        self.sample_num = 0
        self.f_squared_beta_list = []

        self.f_squared_beta_average = 0
        self.f_squared_beta_max = 0
        self.miou_average = 0
        self.miou_max = 0
        self.precision_average = 0
        self.recall_average = 0
        self.precision_max = 0
        self.recall_max = 0

        self.sad = 0
        self.mae = 0
        self.mse = 0
        self.grad = 0
        self.conn = 0

    def add_batch_result(self, preds, masks):
        # preds [b, 1, h, w] probabilities, masks [b, h, w]
        assert preds.shape[1] == 1
        preds = preds[:, 0].float()
        masks = masks.to(preds.device).float()
        thresh = torch.tensor(self.thresh, dtype=torch.float32, device=preds.device).view(-1, 1, 1, 1)
        pred_foreground, mask_foreground = preds.unsqueeze(0) > thresh, masks.unsqueeze(0) > thresh          # [T, b, h, w]
        counts = torch.stack([(pred_foreground & mask_foreground).sum(dim=(2, 3)), mask_foreground.sum(dim=(2, 3)),
                              pred_foreground.sum(dim=(2, 3))], dim=1).cpu().numpy()                           # [T, 3, b] int64
        for i in range(self.thresh_num):
            intersection, all_masks, all_preds = counts[i, 0], counts[i, 1], counts[i, 2]
            union = all_preds + all_masks - intersection
            self.precision_list[i] += np.sum(intersection / (all_preds + 1e-4))
            self.recall_list[i] += np.sum(intersection / (all_masks + 1e-4))
            self.miou_list[i] += np.sum(intersection / (union + 1e-4))

        preds, masks = preds.cpu().numpy(), masks.cpu().numpy()
        nan_inf_count = 0
        for per_pred, per_mask in zip(preds, masks):
            if np.any(np.isinf(per_pred)) or np.any(np.isnan(per_pred)):
                nan_inf_count += 1
                print('per image pred nan or inf pred!')
                continue
            self.sad += np.sum(np.abs(per_mask - per_pred)) / 1000
            self.mae += np.sum(np.abs(per_mask - per_pred)) / (per_mask.shape[0] * per_mask.shape[1])
            self.mse += np.sum((per_mask - per_pred) ** 2) / (per_mask.shape[0] * per_mask.shape[1])
            self.grad += self.cal_gradient(per_pred, per_mask)
            self.conn += self.cal_conn(per_pred, per_mask)
        self.sample_num = self.sample_num + masks.shape[0] - nan_inf_count

    def cal_gradient(self, per_pred, per_mask):
        pd_x = gaussian_filter(per_pred, sigma=1.4, order=[1, 0], output=np.float32)
        pd_y = gaussian_filter(per_pred, sigma=1.4, order=[0, 1], output=np.float32)
        gt_x = gaussian_filter(per_mask, sigma=1.4, order=[1, 0], output=np.float32)
        gt_y = gaussian_filter(per_mask, sigma=1.4, order=[0, 1], output=np.float32)
        error_map = np.square(np.sqrt(pd_x ** 2 + pd_y ** 2) - np.sqrt(gt_x ** 2 + gt_y ** 2))
        return np.sum(error_map) / 10

    def cal_conn(self, per_pred, per_mask):
        pred, true = per_pred, per_mask
        step = 0.1
        thresh_steps = np.arange(0, 1 + step, step)
        round_down_map = -np.ones_like(true)
        for i in range(1, len(thresh_steps)):
            intersection = (true >= thresh_steps[i]) & (pred >= thresh_steps[i])
            # the largest 4-connected component of the intersection; of equally large ones the first label
            output, count = label(intersection, structure=_FOUR_CONNECTED)
            omega = np.zeros_like(true)
            if count != 0:
                size = np.bincount(output.reshape(-1), minlength=count + 1)[1:]
                omega[output == np.argmax(size) + 1] = 1
            mask = (round_down_map == -1) & (omega == 0)
            round_down_map[mask] = thresh_steps[i - 1]
        round_down_map[round_down_map == -1] = 1

        true_diff = true - round_down_map
        pred_diff = pred - round_down_map
        # only differences of at least 0.15 count
        true_phi = 1 - true_diff * (true_diff >= 0.15)
        pred_phi = 1 - pred_diff * (pred_diff >= 0.15)
        return np.sum(np.abs(true_phi - pred_phi)) / 1000

    def compute_all_metrics(self):
        self.precision_list = self.precision_list / self.sample_num
        self.recall_list = self.recall_list / self.sample_num
        self.miou_list = self.miou_list / self.sample_num
        self.f_squared_beta_list = (1 + self.squared_beta) * self.precision_list * self.recall_list / (
            self.squared_beta * self.precision_list + self.recall_list + 1e-4)

        self.f_squared_beta_average = np.mean(self.f_squared_beta_list)
        self.f_squared_beta_max = np.max(self.f_squared_beta_list)
        self.miou_average = np.mean(self.miou_list)
        self.miou_max = np.max(self.miou_list)
        self.precision_average = np.mean(self.precision_list)
        self.precision_max = np.max(self.precision_list)
        self.recall_average = np.mean(self.recall_list)
        self.recall_max = np.max(self.recall_list)

        self.sad = self.sad / self.sample_num
        self.mae = self.mae / self.sample_num
        self.mse = self.mse / self.sample_num
        self.grad = self.grad / self.sample_num
        self.conn = self.conn / self.sample_num


def validate_human_matting(test_loader, model, criterion, config):
    eval_metric = EvalMeter(config)

    def batch_fn(model, data, device):
        images, masks = data['image'].to(device), data['mask'].to(device)
        yield
        outputs = model(images)[2]                      # the fused prediction is what is evaluated
        yield
        eval_metric.add_batch_result(outputs, masks)

    load_ms, inference_ms = timed_eval_pass(test_loader, model, config, batch_fn)
    eval_metric.compute_all_metrics()
    result_dict = collections.OrderedDict()
    result_dict['per_image_load_time'] = f'{load_ms:.3f}ms'
    result_dict['per_image_inference_time'] = f'{inference_ms:.3f}ms'
    result_dict['f_squared_beta_average'] = eval_metric.f_squared_beta_average
    result_dict['f_squared_beta_max'] = eval_metric.f_squared_beta_max
    result_dict['mean_precision'] = eval_metric.precision_average
    result_dict['mean_recall'] = eval_metric.recall_average
    result_dict['max_precision'] = eval_metric.precision_max
    result_dict['max_recall'] = eval_metric.recall_max
    result_dict['miou_average'] = eval_metric.miou_average
    result_dict['miou_max'] = eval_metric.miou_max
    result_dict['sad'] = eval_metric.sad
    result_dict['mae'] = eval_metric.mae
    result_dict['mse'] = eval_metric.mse
    result_dict['grad'] = eval_metric.grad
    result_dict['conn'] = eval_metric.conn
    return result_dict


validate_human_matting_for_all_dataset = for_all_datasets(validate_human_matting)


def matting_losses(criterion, loss_ratio, outputs, images, masks, trimaps, fg_maps, bg_maps):
    """the reference's routing of the criterion dict (tools/human_matting_scripts.py:320-346) -> {name: ratio * loss}"""
    global_preds, local_preds, fused_preds = outputs
    loss_value = {}
    for name in criterion.keys():
        if name in ['GlobalTrimapCELoss', 'GloabelTrimapIouLoss']:
            value = criterion[name](global_preds, trimaps)
        elif name in ['LocalAlphaLoss', 'LocalLaplacianLoss']:
            value = criterion[name](local_preds, masks, trimaps)
        elif name in ['FusionAlphaLoss', 'FusionLaplacianLoss']:
            value = criterion[name](fused_preds, masks)
        elif name in ['CompositionLoss']:
            value = criterion[name](images, masks, fg_maps, bg_maps, fused_preds)
        else:
            raise KeyError(f'train_human_matting: no routing for the loss {name}')
        loss_value[name] = loss_ratio[name] * value
    return loss_value


_KEYS = ('image', 'mask', 'trimap', 'fg_map', 'bg_map')


def train_human_matting(train_loader, model, criterion, optimizer, scheduler, epoch, logger, config):
    '''train human matting model for one epoch (reference tools/human_matting_scripts.py:275-520): `outputs = model(images)`, one
    loss per entry of the criterion dict scaled by config.loss_ratio, and the log line
    `train: epoch 0001, iter [00100, 00937], lr: 0.000100, loss: 6.0674, GlobalTrimapCELoss: 0.6908, GloabelTrimapIouLoss: ..., `.'''
    device, amp = begin_training(model, logger, config)

    def graph_inputs(data):
        return tuple(data[k].to(device, non_blocking=True) for k in _KEYS)

    def step_fn(data):
        images, masks, trimaps, fg_maps, bg_maps = data if isinstance(data, tuple) else graph_inputs(data)
        bad = any_nonfinite(images, masks)
        with amp():
            outputs = model(images)
            loss_value = matting_losses(criterion, config.loss_ratio, outputs, images, masks, trimaps, fg_maps, bg_maps)
        return bad, loss_value, images.size(0)

    return run_epoch(train_loader, model, optimizer, scheduler, epoch, logger, config, step_fn, 'loss', 5, graph_inputs)
