"""Training / evaluation loops of the salient-object-detection family (reference tools/salient_object_detection_scripts.py):

  EvalMeter                                                        (reference :24-88)
  validate_salient_object_detection_segmentation_for_all_dataset   (reference :91-107)
  validate_salient_object_detection_segmentation                   (reference :110-175)
  train_salient_object_detection_segmentation                      (reference :178-368)
  first_dataset_metric: what the entry script checkpoints by       (reference tools/train_salient_object_detection_model.py:215-235)

The training loop is a `step_fn` over tools.loop.run_epoch: the reference's skip / accumulation / clipping / scaler / EMA /
scheduler semantics and its log line.  The iteration has static shapes and no host read (the fused mask statistics take their
gradient as a device tensor), so config.use_step_graph captures it whole, as train_semantic_segmentation does.  Evaluation is
the metric code over tools.loop.timed_eval_pass."""
import collections

import numpy as np
import torch

from ..engine import any_nonfinite
from .loop import begin_training, for_all_datasets, run_epoch, timed_eval_pass


class EvalMeter:
    """The reference's precision / recall / IoU / F-measure accumulator.  The per-threshold foreground counts are taken on the
    tensors' device (three integers per sample and threshold; no full-resolution map travels to the host) and come to the host
    once per batch as a [thresholds, 3, B] integer tensor; everything after them is the reference's numpy code: float64 ratios,
    float32 accumulators, float32 formulas."""

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
        self.sample_num = self.sample_num + masks.shape[0]

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


def validate_salient_object_detection_segmentation(test_loader, model, criterion, config):
    eval_metric = EvalMeter(config)

    def batch_fn(model, data, device):
        images, masks = data['image'].to(device), data['mask'].to(device)
        yield
        outputs = model(images)
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
    return result_dict


validate_salient_object_detection_segmentation_for_all_dataset = for_all_datasets(validate_salient_object_detection_segmentation)


def first_dataset_metric(result_dict, save_model_metric, metric=0, test_loss=0):
    """The entry script judges a checkpoint by the FIRST dataset of the result dict (the config lists the complete validation set
    there): -> (that dataset's result, its `save_model_metric`, its `test_loss`), the last two unchanged where the key is absent."""
    total_result = next(iter(result_dict.values()), None)
    for key, value in (total_result or {}).items():
        if key == save_model_metric:
            metric = value
        elif key == 'test_loss':
            test_loss = value
    return total_result, metric, test_loss


def train_salient_object_detection_segmentation(train_loader, model, criterion, optimizer, scheduler, epoch, logger, config):
    '''train salient object detection segmentation model for one epoch (reference tools/salient_object_detection_scripts.py:178-368):
    `outputs = model(images)`, one loss per entry of the criterion dict scaled by config.loss_ratio, and the log line
    `train: epoch 0001, iter [00100, 00631], lr: 0.000100, loss: 1.2042, BCELoss: 0.6021, BCEIouloss: 0.6021, `.'''
    device, amp = begin_training(model, logger, config)

    def step_fn(data):
        if isinstance(data, tuple):                      # captured step: static device buffers
            images, masks = data
        else:
            images = data['image'].to(device, non_blocking=True)
            masks = data['mask'].to(device, non_blocking=True)
        bad = any_nonfinite(images, masks)
        with amp():
            outputs = model(images)
            loss_value = {name: config.loss_ratio[name] * criterion[name](outputs, masks) for name in criterion.keys()}
        return bad, loss_value, images.size(0)

    def graph_inputs(data):
        return (data['image'].to(device, non_blocking=True), data['mask'].to(device, non_blocking=True))
    return run_epoch(train_loader, model, optimizer, scheduler, epoch, logger, config, step_fn, 'loss', 5, graph_inputs)
