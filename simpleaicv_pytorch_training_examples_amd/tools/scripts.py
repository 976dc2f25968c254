"""Per-iteration train / eval loops of the reference tools/scripts.py on the MI355X engine.

  all_reduce_operation_in_group_for_variables  (reference :26-33)
  test_classification                          (reference :36-113)
  train_classification                         (reference :116-275)
  compute_voc_ap / compute_ious / evaluate_voc_detection / test_detection   (reference :503-739, :884-897; the COCO
                                               variant needs pycocotools, which the bench image does not have)
  train_detection                              (reference :900-1092)
  train_mae_self_supervised_learning           (reference :1774-1934)
  semantic_segmentation_areas / test_semantic_segmentation / train_semantic_segmentation   (reference :1095-1451)

Every train_* function here describes its task -- a `step_fn`, the pieces of its log line, what a captured step takes as inputs --
to the one epoch engine, tools/loop.py (run_epoch), whose module docstring states the skip / accumulation / lag semantics; the timed
evaluation functions are metric code over loop.timed_eval_pass.
"""
import collections
import time

import numpy as np
import torch
import torch.distributed as dist

from ..engine import any_nonfinite
from ..SimpleAICV.classification.common import AccMeter, AverageMeter
from ..SimpleAICV.detection.common import pad_mask_on_device
from .loop import (_device_of, _dist_on, all_ranks_agree, all_reduce_sum_packed, begin_training, run_epoch,  # noqa: F401
                   timed_eval_pass)


def all_reduce_operation_in_group_for_variables(variables, operator, group):
    """python scalars / 0-d tensors -> all-reduced python scalars (blocking; eval path only)."""
    device = 'cuda' if torch.cuda.is_available() else 'cpu'
    for i in range(len(variables)):
        if not torch.is_tensor(variables[i]):
            variables[i] = torch.tensor(variables[i], device=device)
        if _dist_on(group):
            dist.all_reduce(variables[i], op=operator, group=group)
        variables[i] = variables[i].item()
    return variables


def test_classification(test_loader, model, criterion, config):
    losses, accs = AverageMeter(), AccMeter()

    def batch_fn(model, data, device):
        images, labels = data['image'].to(device), data['label'].to(device)
        yield
        outputs = model(images)
        yield
        loss = criterion(outputs, labels)
        _, topk = torch.topk(outputs, k=5, dim=1, largest=True, sorted=True)
        correct = topk.eq(labels.unsqueeze(-1).expand_as(topk)).float()
        # one fused all-reduce instead of the reference's 1 + 3 scalar ones (C8)
        packed = torch.stack([loss.float(), correct[:, :1].sum(), correct[:, :5].sum(),
                              torch.tensor(float(images.size(0)), device=device)])
        all_reduce_sum_packed(packed, model, config.group)
        loss_sum, acc1_n, acc5_n, n = packed.tolist()
        losses.update(loss_sum / float(config.gpus_num), images.size(0))
        accs.update(acc1_n, acc5_n, n)

    load_ms, inference_ms = timed_eval_pass(test_loader, model, config, batch_fn)
    accs.compute()
    return accs.acc1 * 100, accs.acc5 * 100, losses.avg, load_ms, inference_ms


def train_classification(train_loader, model, criterion, optimizer, scheduler, epoch, logger, config):
    '''train classification model for one epoch.  The loss goes to the engine as a bare scalar: the packed vector is [skip, loss] and
    the captured ResNet-50 / ViT step carries no loss-term bookkeeping.'''
    device, amp = begin_training(model, logger, config)

    def graph_inputs(data):
        return (data['image'].to(device, non_blocking=True), data['label'].to(device, non_blocking=True))

    def step_fn(data):
        images, labels = data if isinstance(data, tuple) else graph_inputs(data)      # (a tuple: the captured step's static buffers)
        bad = any_nonfinite(images, labels) if labels.dtype.is_floating_point else any_nonfinite(images)
        with amp():
            loss = criterion(model(images), labels)
        return bad, loss, images.size(0)

    return run_epoch(train_loader, model, optimizer, scheduler, epoch, logger, config, step_fn, 'loss', 5, graph_inputs,
                     log_terms=False)


def train_detection(train_loader, model, criterion, optimizer, scheduler, epoch, logger, config):
    '''train detection model for one epoch (reference tools/scripts.py:900-1092).  DETR-family networks
    ('detr' in config.network) take the padding mask and the normalised cxcywh annotations.'''
    device, amp = begin_training(model, logger, config)
    is_detr = 'detr' in config.network

    static_detr = is_detr and getattr(criterion, 'static_form', False) and getattr(config, 'use_step_graph', False)

    def step_fn(data):
        if isinstance(data, tuple) and static_detr:
            # captured DETR step (r05): fixed shapes and no host read -- the cost matrices, the Hungarian assignment (saicv_detr_assign)
            # and the loss over the padded ground truth all stay on the device
            images, mask, ann = data
            bad = any_nonfinite(images, ann)
            with amp():
                outs = model(images, mask)
                cost, valid = criterion.match_inputs(outs, ann)
                src, tgt, w = criterion.assign_device(cost, valid)
                loss_value = criterion.forward_static(outs, ann, src, tgt, w)
            return bad, loss_value, images.size(0)
        if isinstance(data, tuple):                      # captured step: (images, targets) already on the device, static buffers
            images, targets = data
        else:
            images = data['image'].to(device, non_blocking=True)
            host_targets = data['scaled_annots'] if is_detr else data['annots']
            targets = host_targets.to(device, non_blocking=True)
            if is_detr and not host_targets.is_cuda:
                targets._saicv_host = host_targets       # DETRLoss selects the valid rows on the host (no per-image device sync)
        bad = any_nonfinite(images, targets)
        with amp():
            if not is_detr:
                outs = model(images)
            elif getattr(config, 'device_pad_mask', False):      # f3: the mask from the [B, 2] sizes instead of a [B, S, S] copy
                outs = model(images, pad_mask_on_device(data['scaled_size'], images.shape[-1], device))
            else:
                outs = model(images, data['mask'].to(device, non_blocking=True))
            loss_value = criterion(outs, targets)
        return bad, loss_value, images.size(0)

    # the dense detectors' step has no host read (anchor assignment, focal loss and SmoothL1 are decided on the device): it can be
    # captured whole.  So can DETR's since r05: its Hungarian assignment runs on the device (DETRLoss.assign_device) over the
    # annotations padded (class -1 rows) to config.max_annots rows (default 100 = the reference's query count; a batch with more boxes
    # in one image takes the eager step with the host-side assignment).  Criteria that index by a data-dependent positive mask
    # (`capturable = False`, e.g. the IoU branches) have dynamic shapes and stay eager.
    graph_inputs = None
    if not is_detr and getattr(criterion, 'capturable', False):
        def graph_inputs(data):
            return (data['image'].to(device, non_blocking=True), data['annots'].to(device, non_blocking=True))
    elif static_detr:
        max_annots = int(getattr(config, 'max_annots', 100))

        def graph_inputs(data):
            ann = data['scaled_annots']
            if ann.shape[1] > max_annots:
                if bool((ann[:, max_annots:, 4] >= 0).any()):
                    return None
                ann = ann[:, :max_annots]
            ann = ann.to(device, non_blocking=True).float()
            if ann.shape[1] < max_annots:
                ann = torch.cat([ann, ann.new_full((ann.shape[0], max_annots - ann.shape[1], ann.shape[2]), -1.0)], dim=1)
            if getattr(config, 'device_pad_mask', False):
                mask = pad_mask_on_device(data['scaled_size'], data['image'].shape[-1], device)
            else:
                mask = data['mask'].to(device, non_blocking=True)
            return (data['image'].to(device, non_blocking=True), mask, ann)
        graph_inputs.may_decline = True
    return run_epoch(train_loader, model, optimizer, scheduler, epoch, logger, config, step_fn, 'total_loss', 5, graph_inputs)


def train_mae_self_supervised_learning(train_loader, model, criterion, optimizer, scheduler, epoch, logger, config):
    '''train mae self supervised model for one epoch (reference tools/scripts.py:1774-1934): `outputs, masks = model(images)`,
    `loss = criterion(outputs, labels, masks)` (the per-patch regression target comes from MAESelfSupervisedPretrainCollater),
    the reference's skip / accumulation / clipping / scaler / EMA / scheduler semantics and its log line
    `train: epoch 0001, iter [00100, 01251], lr: 0.000150, loss: 0.7523`.  The iteration has no host read and static shapes
    (the mask is an argsort of device noise, the kept-patch count is fixed by mask_ratio): with config.use_step_graph it is
    captured whole and replayed, as the classification loop is.'''
    device, amp = begin_training(model, logger, config)

    def step_fn(data):
        if isinstance(data, tuple):                      # captured step: static device buffers
            images, labels = data
        else:
            images = data['image'].to(device, non_blocking=True)
            labels = data['label'].to(device, non_blocking=True)
        bad = any_nonfinite(images, labels)
        with amp():
            outputs, masks = model(images)
            loss = criterion(outputs, labels, masks)
        return bad, {'loss': loss}, images.size(0)

    def graph_inputs(data):
        return (data['image'].to(device, non_blocking=True), data['label'].to(device, non_blocking=True))
    return run_epoch(train_loader, model, optimizer, scheduler, epoch, logger, config, step_fn, 'loss', 5, graph_inputs,
                     log_terms=False)


# ---------------------------------------------------------------------------------------------- semantic segmentation
def semantic_segmentation_areas(pred_ids, mask, sizes, num_classes):
    """Per-class pixel counts of one batch, float64 [4, num_classes]: intersection, prediction, ground truth, union -- what the
    reference takes per image with torch.histc(bins=num_classes, min=0, max=num_classes - 1) over the top-left
    int(size[0]) x int(size[1]) crop (reference tools/scripts.py:1138-1171), summed over the batch.  pred_ids [B, H, W] integer class
    ids, mask [B, H, W] class ids (float, as the collater delivers them), sizes [B, 2] (h, w).  Ids outside [0, num_classes) are
    not counted (histc ignores values outside its range).  Pure tensor code: runs on the tensors' device, CPU included."""
    dev = pred_ids.device
    b, h, w = pred_ids.shape
    hw = torch.as_tensor(np.asarray(sizes), dtype=torch.float32).to(dev).long()              # int(size): truncation
    inside = ((torch.arange(h, device=dev).view(1, h, 1) < hw[:, 0].view(b, 1, 1))
              & (torch.arange(w, device=dev).view(1, 1, w) < hw[:, 1].view(b, 1, 1)))
    pred, gt = pred_ids.long(), mask.long()

    def count(ids, select):
        select = select & (ids >= 0) & (ids < num_classes)
        return torch.bincount(ids[select], minlength=num_classes).double()

    area_pred, area_gt = count(pred, inside), count(gt, inside)
    intersect = count(pred, inside & (pred == mask))
    return torch.stack([intersect, area_pred, area_gt, area_pred + area_gt - intersect])


def timed_class_area_pass(test_loader, model, criterion, config):
    """The evaluation pass semantic segmentation and human / face parsing share: loss by the test criterion, argmax over the
    classes, per-class areas accumulated on the device in float64.
    -> (result dict with test_loss and the two per-image times, areas as [4][num_classes] lists)"""
    losses, areas = AverageMeter(), torch.zeros((4, config.num_classes), dtype=torch.float64)

    def batch_fn(model, data, device):
        nonlocal areas
        images, masks, sizes = data['image'].to(device), data['mask'].to(device), data['size']
        yield
        outputs = model(images)
        yield
        losses.update(float(criterion(outputs, masks)), images.size(0))
        areas = areas.to(device) + semantic_segmentation_areas(torch.argmax(outputs, dim=1), masks, sizes, config.num_classes)

    load_ms, inference_ms = timed_eval_pass(test_loader, model, config, batch_fn)
    result_dict = collections.OrderedDict()
    result_dict['test_loss'] = losses.avg
    result_dict['per_image_load_time'] = f'{load_ms:.3f}ms'
    result_dict['per_image_inference_time'] = f'{inference_ms:.3f}ms'
    return result_dict, areas.cpu().tolist()


def test_semantic_segmentation(test_loader, model, criterion, config):
    """reference :1095-1259: loss, argmax over the classes, per-class areas accumulated on the device in float64, then mean
    precision / recall / IoU / Dice over the classes that occur in the ground truth (x 100)."""
    result_dict, (intersect, area_pred, area_gt, union) = timed_class_area_pass(test_loader, model, criterion, config)
    exist_num_class, sums = 0., [0., 0., 0., 0.]
    for i, p, g, u in zip(intersect, area_pred, area_gt, union):
        if g == 0:
            continue
        exist_num_class += 1.
        for j, (num, den) in enumerate(((i, p), (i, g), (i, u), (2. * i, p + g))):
            if den != 0:
                sums[j] += num / den * 100.
    if exist_num_class > 0:
        sums = [v / exist_num_class for v in sums]
    result_dict['exist_num_class'] = exist_num_class
    for name, v in zip(('mean_precision', 'mean_recall', 'mean_iou', 'mean_dice'), sums):
        result_dict[name] = v
    return result_dict


def train_semantic_segmentation(train_loader, model, criterion, optimizer, scheduler, epoch, logger, config):
    '''train semantic segmentation model for one epoch (reference tools/scripts.py:1262-1451): `outputs = model(images)`, one loss
    per entry of the criterion dict scaled by config.loss_ratio, the reference's skip / accumulation / clipping / scaler / EMA /
    scheduler semantics and its log line `train: epoch 0001, iter [00100, 00631], lr: 0.000100, loss: 2.1042, CELoss: 2.1042, `.
    The iteration has static shapes and no host read (the fused loss decides the clamp on the device): with config.use_step_graph
    it is captured whole and replayed.'''
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


# ---------------------------------------------------------------------------------------------- detection evaluation
def compute_voc_ap(recall, precision, use_07_metric=False):
    """area under the precision envelope (VOC >= 2010) or the 11-point average (VOC 2007); reference :503-532"""
    recall, precision = np.asarray(recall, dtype=np.float64), np.asarray(precision, dtype=np.float64)
    if use_07_metric:
        ap = 0.
        for t in np.arange(0., 1.1, 0.1):
            hit = recall >= t
            ap = ap + (np.max(precision[hit]) if hit.any() else 0) / 11.
        return ap
    r = np.concatenate(([0.], recall, [1.]))
    env = np.maximum.accumulate(np.concatenate(([0.], precision, [0.]))[::-1])[::-1]      # precision envelope from the right
    step = np.where(r[1:] != r[:-1])[0]
    return np.sum((r[step + 1] - r[step]) * env[step + 1])


def compute_ious(a, b):
    """[N, 4] x [M, 4] xyxy boxes -> IoU [N, M] (no clamp on degenerate unions, as the reference :535-556)"""
    a, b = np.expand_dims(a, axis=1), np.expand_dims(b, axis=0)
    overlap = np.prod(np.maximum(0.0, np.minimum(a[..., 2:], b[..., 2:]) - np.maximum(a[..., :2], b[..., :2])), axis=-1)
    area_a = np.prod(a[..., 2:] - a[..., :2], axis=-1)
    area_b = np.prod(b[..., 2:] - b[..., :2], axis=-1)
    return overlap / (area_a + area_b - overlap)


def _voc_class_ap(gt_boxes, pred_boxes, pred_scores, threshold):
    """AP of one class at one IoU threshold.  Per image, predictions are visited in the order the decoder emitted them; each
    takes its best-IoU ground-truth box if that box is still free and the IoU reaches the threshold (reference :676-706)."""
    flags, scores, total = [], [], 0
    for boxes, preds, sc in zip(gt_boxes, pred_boxes, pred_scores):
        total += len(boxes)
        if len(preds) == 0:
            continue
        scores.append(sc)
        hit = np.zeros(len(preds))
        if boxes.shape[0] > 0:
            iou = compute_ious(boxes, preds)                              # [gt, pred]
            best = np.argmax(iou, axis=0)
            best_iou = iou[best, np.arange(len(preds))]
            taken = np.zeros(boxes.shape[0], dtype=bool)
            for j in range(len(preds)):
                if best_iou[j] >= threshold and not taken[best[j]]:
                    hit[j] = 1
                    taken[best[j]] = True
        flags.append(hit)
    if not scores:
        tp = fp = np.zeros((0,))
    else:
        order = np.argsort(-np.concatenate(scores))
        hit = np.concatenate(flags)[order]
        tp, fp = np.cumsum(hit), np.cumsum(1 - hit)
    with np.errstate(divide='ignore', invalid='ignore'):
        recall = tp / total
    precision = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    return compute_voc_ap(recall, precision, use_07_metric=False)


def evaluate_voc_detection(test_loader, model, criterion, decoder, config):
    """VOC-style mAP at every threshold of config.eval_voc_iou_threshold_list (reference :559-739): forward + loss + decode per
    batch, boxes back to the original image scale and clipped to it, then per class and threshold the matching above."""
    model.eval()
    batch_time, data_time, losses = AverageMeter(), AverageMeter(), AverageMeter()
    batch_size = int(config.batch_size // config.gpus_num)
    device = _device_of(model)
    on_gpu = device.type == 'cuda'
    is_detr = 'detr' in config.network
    preds, gts = [], []
    with torch.no_grad():
        end = time.time()
        for data in test_loader:
            images, annots, scales, sizes = data['image'].to(device), data['annots'].to(device), data['scale'], data['size']
            if on_gpu:
                torch.cuda.synchronize()
            data_time.update(time.time() - end, images.size(0))
            end = time.time()
            outs = model(images, data['mask'].to(device)) if is_detr else model(images)
            loss = sum(criterion(outs, annots).values())
            losses.update(float(loss), images.size(0))
            pred_scores, pred_classes, pred_boxes = decoder(outs, data['scaled_size']) if is_detr else decoder(outs)
            unscale = np.expand_dims(np.expand_dims(scales, axis=-1), axis=-1)
            pred_boxes = pred_boxes / unscale
            if on_gpu:
                torch.cuda.synchronize()
            batch_time.update(time.time() - end, images.size(0))
            annots = annots.cpu().numpy()
            gt_bboxes, gt_classes = annots[:, :, 0:4] / unscale, annots[:, :, 4]
            for sc, cl, bx, gb, gc, size in zip(pred_scores, pred_classes, pred_boxes, gt_bboxes, gt_classes, sizes):
                live = cl > -1
                sc, cl, bx = sc[live], cl[live], bx[live].copy()
                bx[:, 0:2] = np.maximum(bx[:, 0:2], 0)
                bx[:, 2] = np.minimum(bx[:, 2], size[1])
                bx[:, 3] = np.minimum(bx[:, 3], size[0])
                preds.append([bx, cl, sc])
                gts.append([gb[gc > -1], gc[gc > -1]])
            end = time.time()
    result_dict = collections.OrderedDict()
    result_dict['test_loss'] = losses.avg
    result_dict['per_image_load_time'] = f'{data_time.avg / batch_size * 1000:.3f}ms'
    result_dict['per_image_inference_time'] = f'{batch_time.avg / batch_size * 1000:.3f}ms'
    per_class = collections.OrderedDict()
    for thr in config.eval_voc_iou_threshold_list:
        aps = collections.OrderedDict()
        for c in range(config.num_classes):
            aps[c] = 100 * _voc_class_ap([g[0][g[1] == c] for g in gts], [p[0][p[1] == c] for p in preds],
                                         [p[2][p[1] == c] for p in preds], thr)
        result_dict[f'IoU={thr:.2f},area=all,maxDets=100,mAP'] = sum(float(v) for v in aps.values()) / config.num_classes
        per_class[f'IoU={thr:.2f},area=all,maxDets=100,per_class_ap'] = aps
    result_dict.update(per_class)
    return result_dict


def evaluate_coco_detection(test_loader, model, criterion, decoder, config):
    """COCO-style evaluation (reference :742-881): forward + loss + decode per batch, boxes back to the original image scale,
    clipped, converted to [x, y, w, h], then the twelve COCO summary numbers (x 100) under the reference's keys.  The reference
    hands the detections to pycocotools' COCOeval; here the same protocol runs in numpy (tools/cocoeval_numpy.py).  Ground truth:
    `config.test_dataset.coco.dataset` (a COCO annotation dict, as pycocotools holds it) when the dataset has one, else the
    annotations the loader delivers (un-scaled; every box a regular, non-crowd object with area w * h) -- which is what the
    synthetic benchmark datasets provide."""
    from . import cocoeval_numpy as CE
    model.eval()
    batch_time, data_time, losses = AverageMeter(), AverageMeter(), AverageMeter()
    test_dataset = config.test_dataset
    batch_size = int(config.batch_size // config.gpus_num)
    device = _device_of(model)
    on_gpu = device.type == 'cuda'
    is_detr = 'detr' in config.network
    image_id_of = getattr(test_dataset, 'image_ids', None)
    cat_of = getattr(test_dataset, 'coco_label_to_cat_id', None)
    coco = getattr(test_dataset, 'coco', None)
    results, gts, image_ids = [], [], []
    with torch.no_grad():
        end = time.time()
        for i, data in enumerate(test_loader):
            images, annots, scales, sizes = data['image'].to(device), data['annots'].to(device), data['scale'], data['size']
            if on_gpu:
                torch.cuda.synchronize()
            data_time.update(time.time() - end, images.size(0))
            end = time.time()
            outs = model(images, data['mask'].to(device)) if is_detr else model(images)
            loss = sum(criterion(outs, annots).values())
            losses.update(float(loss), images.size(0))
            scores, classes, boxes = decoder(outs, data['scaled_size']) if is_detr else decoder(outs)
            unscale = np.expand_dims(np.expand_dims(scales, axis=-1), axis=-1)
            boxes = boxes / unscale
            if on_gpu:
                torch.cuda.synchronize()
            batch_time.update(time.time() - end, images.size(0))
            annots_np = annots.cpu().numpy()
            for b in range(images.size(0)):
                index = i * batch_size + b
                img_id = image_id_of[index] if image_id_of is not None else index
                image_ids.append(img_id)
                pb = boxes[b].copy()
                pb[:, 0], pb[:, 1] = np.maximum(pb[:, 0], 0), np.maximum(pb[:, 1], 0)
                pb[:, 2], pb[:, 3] = np.minimum(pb[:, 2], sizes[b][1]), np.minimum(pb[:, 3], sizes[b][0])
                pb[:, 2:] -= pb[:, :2]                                  # COCO boxes are [x_min, y_min, w, h]
                for sc, cl, bx in zip(scores[b], classes[b], pb):
                    if int(cl) == -1:
                        break
                    results.append({'image_id': img_id, 'category_id': cat_of[int(cl)] if cat_of is not None else int(cl),
                                    'score': float(sc), 'bbox': bx.tolist()})
                if coco is None:
                    for row in annots_np[b]:
                        if row[4] < 0:
                            continue
                        x0, y0, x1, y1 = (row[0:4] / float(np.asarray(scales[b]).reshape(-1)[0])).tolist()
                        gts.append({'image_id': img_id, 'category_id': cat_of[int(row[4])] if cat_of is not None else int(row[4]),
                                    'bbox': [x0, y0, x1 - x0, y1 - y0], 'area': (x1 - x0) * (y1 - y0), 'iscrowd': 0})
            end = time.time()
    result_dict = collections.OrderedDict()
    result_dict['test_loss'] = losses.avg
    result_dict['per_image_load_time'] = f'{data_time.avg / batch_size * 1000:.3f}ms'
    result_dict['per_image_inference_time'] = f'{batch_time.avg / batch_size * 1000:.3f}ms'
    if len(results) == 0:
        for name in CE.STAT_NAMES:
            result_dict[name] = 0
        return result_dict
    cats = None
    if coco is not None:
        ds = coco.dataset
        wanted = set(image_ids)
        gts = [dict(a) for a in ds['annotations'] if a['image_id'] in wanted]
        cats = [c['id'] for c in ds['categories']]
    stats, _, _ = CE.evaluate_bbox(gts, results, image_ids=image_ids, category_ids=cats)
    for name, v in zip(CE.STAT_NAMES, stats):
        result_dict[name] = v * 100
    return result_dict


def test_detection(test_loader, model, criterion, decoder, config):
    """reference :884-897"""
    assert config.eval_type in ['COCO', 'VOC']
    if getattr(config, 'use_ema_model', False):
        model = config.ema_model.ema_model
    return {'COCO': evaluate_coco_detection, 'VOC': evaluate_voc_detection}[config.eval_type](test_loader, model, criterion, decoder, config)
