"""Training / evaluation loops of the human-parsing family (reference tools/human_parsing_scripts.py); the face-parsing family
(tools/face_parsing_scripts.py) re-exports them under its names, as the reference's two files differ by names only.

  validate_human_parsing_for_all_dataset    (reference :23-40)
  validate_human_parsing                    (reference :43-204)
  train_human_parsing                       (reference :207-394)
  parsing_metrics: the per-class precision / recall / IoU / Dice arithmetic of validate_human_parsing (:139-203) on its own
  first_dataset_metric: what the entry script checkpoints by (reference tools/train_human_parsing_model.py)

The training loop is a `step_fn` over tools.loop.run_epoch: the reference's skip / accumulation / clipping / scaler / EMA /
scheduler semantics and its log line with one value per loss name.  All losses of the criterion dict read the same prediction, so
on the device they share one pass of ops.pixel_class_terms each way.  The iteration has static shapes and no host read, so
config.use_step_graph captures it whole.  The evaluation pass is the one semantic segmentation makes
(tools.scripts.timed_class_area_pass)."""
import collections

from ..engine import any_nonfinite
from .loop import begin_training, for_all_datasets, run_epoch
from .salient_object_detection_scripts import first_dataset_metric  # noqa: F401  (the same rule, one copy)
from .scripts import timed_class_area_pass


def parsing_metrics(areas):
    """areas: [4][num_classes] = per-class intersection, prediction, ground-truth and union pixel counts.
    -> OrderedDict: exist_num_class, mean_precision / mean_recall / mean_iou / mean_dice (x 100) over the classes that occur in the
    ground truth, then class_i_precision, class_i_recall, class_i_iou, class_i_dice for every class (0 for a class absent from
    the ground truth, and for a ratio whose denominator is 0) -- key order as the reference builds it."""
    intersect, area_pred, area_gt, union = [list(map(float, row)) for row in areas]
    num_classes = len(intersect)
    per_class = [[0.] * num_classes for _ in range(4)]
    exist_num_class, sums = 0., [0., 0., 0., 0.]
    for c, (i, p, g, u) in enumerate(zip(intersect, area_pred, area_gt, union)):
        if g == 0:
            continue
        exist_num_class += 1.
        for j, (num, den) in enumerate(((i, p), (i, g), (i, u), (2. * i, p + g))):
            if den != 0:
                per_class[j][c] = num / den * 100.
            sums[j] += per_class[j][c]
    if exist_num_class > 0:
        sums = [v / exist_num_class for v in sums]
    result = collections.OrderedDict()
    result['exist_num_class'] = exist_num_class
    names = ('precision', 'recall', 'iou', 'dice')
    for name, v in zip(names, sums):
        result[f'mean_{name}'] = v
    for name, values in zip(names, per_class):
        for c, v in enumerate(values):
            result[f'class_{c}_{name}'] = v
    return result


def validate_human_parsing(test_loader, model, criterion, config):
    """reference :43-204: loss by the test criterion, argmax over the classes, the top-left int(size) crop, per-class areas
    accumulated on the device in float64 (tools.scripts.semantic_segmentation_areas), then parsing_metrics."""
    result_dict, areas = timed_class_area_pass(test_loader, model, criterion, config)
    result_dict.update(parsing_metrics(areas))
    return result_dict


validate_human_parsing_for_all_dataset = for_all_datasets(validate_human_parsing)


def train_human_parsing(train_loader, model, criterion, optimizer, scheduler, epoch, logger, config):
    '''train human parsing model for one epoch (reference :207-394): `outputs = model(images)`, one loss per entry of the criterion
    dict scaled by config.loss_ratio, a batch with inf / nan images, masks, loss or gradients skipped, and the log line
    `train: epoch 0001, iter [00100, 00158], lr: 0.000100, loss: 1.9042, CELoss: 1.2042, IoULoss: 0.7000, `.'''
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
