"""Training and validation loops of the reference's text-recognition family (tools/text_scripts.py), for any model that maps
images [B, 3, H, W] to per-frame logits [B, T, num_classes + 1].

train_text_recognition (:894-...): `outputs = model(images)`, the permuted [T, B, C] view goes to the criterion dict
({'CTCLoss': ...} in the reference config, 'ACELoss' also known) scaled by config.loss_ratio; accumulation, skip of a non-finite
batch, scaler, clipping, EMA, scheduler and the reference's log line come from tools.loop.run_epoch.  On the device CTCLoss
is ops.ctc_loss (csrc/ctc.hip): labels are encoded on the host by config.converter and copied over, nothing is read back.  The
iteration has no host read and nn.LSTM captures unchanged, so config.use_step_graph replays it as one hipGraph -- for batches of
ONE width and accumulation_steps 1 (what tools.loop.run_epoch's captured step asks for); the reference config's
accumulation_steps 2 and batches of changing width run eagerly.

test_text_recognition_for_all_dataset (:31-...): one pass per validation set (the reference makes four): test_loss by the test
criterion, greedy decode by ops.ctc_greedy (arg-max class and its softmax probability per frame without a softmax tensor; on CPU
tensors the reference's two expressions) and config.converter.decode, then str_acc, not_included_str_percent,
final_edit_distance (ICDAR2019 normalised edit distance) and lcs_precision / lcs_recall over all characters, x 100.  Levenshtein
distance and LCS are SimpleAICV.text_recognition.common's.  The reference's order precision / recall and the per-table LCS figures
(digits, letters, the three Chinese tables) are not computed, nor its `ignore_threhold` (-1 below 1000 target characters)."""
import collections

import torch
import torch.nn.functional as F

from .. import ops
from ..engine import any_nonfinite
from ..SimpleAICV.classification.common import AverageMeter
from ..SimpleAICV.text_recognition.common import edit_distance, lcs_length
from .loop import begin_training, for_all_datasets, run_epoch, timed_eval_pass
from .salient_object_detection_scripts import first_dataset_metric  # noqa: F401  (checkpoints go by lcs_precision of the first set)
from .scripts import all_reduce_operation_in_group_for_variables


def text_losses(criterion, loss_ratio, outputs, trans_targets, input_lengths, target_lengths):
    """outputs [T, B, C] -> {name: scaled loss} for the criterion dict of the reference configs"""
    loss_value = {}
    for name in criterion.keys():
        if name == 'CTCLoss':
            loss_value[name] = loss_ratio[name] * criterion[name](outputs, trans_targets, input_lengths, target_lengths)
        elif name == 'ACELoss':
            loss_value[name] = loss_ratio[name] * criterion[name](outputs, trans_targets)
        else:
            raise ValueError(f'Unsupport loss: {name}')
    return loss_value


def greedy_decode(outputs, input_lengths):
    """outputs [B, T, C] -> (index [B, T], prob [B, T]) on the host: each frame's arg-max class and its softmax probability"""
    if outputs.is_cuda:
        index, prob = ops.ctc_greedy(outputs.permute(1, 0, 2), input_lengths)
        return index.t().cpu().numpy(), prob.t().cpu().numpy()
    _, index = outputs.max(dim=2)
    prob, _ = F.softmax(outputs.float(), dim=2).max(dim=2)
    return index.numpy(), prob.numpy()


def string_counts(pred_strs, targets, keep_characters, garbage_char, case_insensitive=True):
    """the reference's per-batch bookkeeping (:196-257 and the all-character part of :749-...) -> dict of
    correct / not_included / ne_distance (strings) and lcs / pred_chars / target_chars (characters)"""
    keep = set(keep_characters)
    out = dict(correct=0, not_included=0, ne_distance=0., lcs=0, pred_chars=0, target_chars=0)
    for pred, target in zip(pred_strs, targets):
        if any(ch not in keep for ch in target):
            out['not_included'] += 1
        target = ''.join(ch if ch in keep else garbage_char for ch in target).replace(' ', '')
        pred = pred.replace(' ', '')
        if target == garbage_char or target == '':
            continue
        # LCS over the strings as they are, the string comparison and the edit distance case-folded (as the reference has them)
        if len(pred) and len(target):
            out['lcs'] += lcs_length(pred, target)
        out['pred_chars'] += len(pred)
        out['target_chars'] += len(target)
        if case_insensitive:
            pred, target = pred.lower(), target.lower()
        if pred == target:
            out['correct'] += 1
        if len(pred) and len(target):
            out['ne_distance'] += 1 - edit_distance(pred, target) / max(len(pred), len(target))
    return out


def test_text_recognition_for_all_dataset(val_loader_list, model, criterion, config):
    if getattr(config, 'use_ema_model', False):
        model = config.ema_model.ema_model
    return for_all_datasets(test_text_recognition_for_per_sub_dataset)(val_loader_list, model, criterion, config)


def test_text_recognition_for_per_sub_dataset(val_loader, model, criterion, config):
    losses = AverageMeter()
    converter = config.converter
    keep = ''.join(config.all_char_table)
    total = collections.Counter()
    total_strs = 0

    def batch_fn(model, data, device):
        nonlocal total_strs
        images, targets = data['image'].to(device), data['label']
        trans_targets, target_lengths = converter.encode(targets)
        trans_targets, target_lengths = trans_targets.to(device), target_lengths.to(device)
        yield
        outputs = model(images)
        yield
        input_lengths = torch.full((outputs.shape[0],), outputs.shape[1], dtype=torch.int32, device=device)
        loss = criterion(outputs.permute(1, 0, 2), trans_targets, input_lengths, target_lengths)
        [loss] = all_reduce_operation_in_group_for_variables([loss], torch.distributed.ReduceOp.SUM, getattr(config, 'group', None))
        losses.update(float(loss) / float(config.gpus_num), images.size(0))
        index, _prob = greedy_decode(outputs, input_lengths)
        pred_strs = converter.decode(index, input_lengths.cpu().numpy())
        total.update(string_counts(pred_strs, targets, keep, converter.garbage_char))
        total_strs += images.size(0)

    # (the model is the one the caller hands over: the ..._for_all_dataset wrapper has made the EMA switch)
    load_ms, inference_ms = timed_eval_pass(val_loader, model, config, batch_fn, ema=False)
    keys = ['correct', 'not_included', 'ne_distance', 'lcs', 'pred_chars', 'target_chars']
    values = all_reduce_operation_in_group_for_variables([total[k] for k in keys] + [total_strs], torch.distributed.ReduceOp.SUM,
                                                         getattr(config, 'group', None))
    total, total_strs = dict(zip(keys, values[:-1])), values[-1]
    result = collections.OrderedDict()
    result['per_image_load_time'] = load_ms
    result['per_image_inference_time'] = inference_ms
    result['test_loss'] = losses.avg
    result['str_acc'] = total['correct'] / float(total_strs) * 100 if total_strs else 0
    result['not_included_str_percent'] = total['not_included'] / float(total_strs) * 100 if total_strs else 0
    result['final_edit_distance'] = total['ne_distance'] / float(total_strs) * 100 if total_strs else 0
    result['lcs_precision'] = total['lcs'] / float(total['pred_chars']) * 100 if total['pred_chars'] else 0
    result['lcs_recall'] = total['lcs'] / float(total['target_chars']) * 100 if total['target_chars'] else 0
    return result


def train_text_recognition(train_loader, model, criterion, optimizer, scheduler, epoch, logger, config):
    '''train a text recognition model for one epoch; the log line is
    `train: epoch 0001, iter [00050, 00158], lr: 0.000100, loss: 12.9042, CTCLoss: 12.9042, `.'''
    device, amp = begin_training(model, logger, config)

    def graph_inputs(data):
        trans_targets, target_lengths = config.converter.encode(data['label'])
        return (data['image'].to(device, non_blocking=True), trans_targets.to(device, non_blocking=True),
                target_lengths.to(device, non_blocking=True))

    def step_fn(data):
        # (a tuple: the static device buffers of the captured step)
        images, trans_targets, target_lengths = data if isinstance(data, tuple) else graph_inputs(data)
        bad = any_nonfinite(images)
        with amp():
            outputs = model(images)                                          # [B, T, C]
            input_lengths = torch.full((outputs.shape[0],), outputs.shape[1], dtype=torch.int32, device=device)
            loss_value = text_losses(criterion, config.loss_ratio, outputs.permute(1, 0, 2), trans_targets, input_lengths,
                                     target_lengths)
        return bad, loss_value, images.size(0)

    return run_epoch(train_loader, model, optimizer, scheduler, epoch, logger, config, step_fn, 'loss', 5, graph_inputs)
