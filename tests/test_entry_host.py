"""tools/entry.py on the CPU: `resume()` and `fit()` driven with stand-ins for each of the 12 training tasks, the report step of each of
the 9 test tasks, and the surface of the 21 entry modules.  Every task description comes from its real entry module; only the loop and
evaluation functions are replaced by scripted ones.  The expected log lines are the f-strings of the entry scripts as they were before
the shared driver, written out by hand: nothing here formats a line through the code under test."""
import argparse
import dataclasses
import importlib
import os
import re
import types

import numpy as np
import pytest
import torch

from simpleaicv_pytorch_training_examples_amd import ops  # noqa: F401  (resume() imports it: not on the first test's clock)
from simpleaicv_pytorch_training_examples_amd.tools import entry

PKG = 'simpleaicv_pytorch_training_examples_amd.tools.'
LOSSES = (0.5, 0.25, 0.75, 0.125)               # the scripted training loss of epochs 1..4

# module -> (family, writes epoch_N.pth, checkpoints follow the EMA model)
TRAIN_TASKS = {
    'train_classification_model': ('acc', False, True),
    'train_semantic_segmentation_model': ('percent', False, True),
    'train_salient_object_detection_model': ('list', True, True),
    'train_human_matting_model': ('list', True, True),
    'train_face_parsing_model': ('list', True, True),
    'train_human_parsing_model': ('list', True, True),
    'train_text_recognition_model': ('list', True, True),
    'train_detection_model': ('loss', False, False),
    'train_mae_self_supervised_model': ('loss', False, True),
    'train_interactive_segmentation_model': ('loss', True, False),
    'train_interactive_matting_model': ('loss', True, False),
    'train_universal_segmentation_model': ('loss', True, True),
}

# what the scripted evaluation returns, call by call
EVAL_RESULTS = {
    'acc': [(50.0, 80.0, 1.5, 0.25, 0.5), (60.0, 85.0, 1.25, 0.25, 0.5), (55.0, 82.0, 1.375, 0.25, 0.5), (70.0, 90.0, 1.0, 0.25, 0.5)],
    'percent': [{'test_loss': 0.75, 'per_image_load_time': 0.1, 'm': 40.0}, {'test_loss': 0.5, 'per_image_load_time': 0.1, 'm': 45.5}],
    'list': [{'setA': {'per_image_load_time': 0.1, 'm': np.float32(40.0), 'test_loss': 0.75}, 'setB': {'m': np.float32(99.0)}},
             {'setA': {'per_image_load_time': 0.1, 'm': np.float32(45.5), 'test_loss': 0.5}, 'setB': {'m': np.float32(1.0)}}],
    'loss': [],
}
CALLS_IN_FIRST_RUN = {'acc': 3, 'percent': 1, 'list': 1, 'loss': 0}

FIRST_RUN = {           # epochs 1-3 of 4 (eval_epoch [2]); the run is cut off inside epoch 4's training
    'acc': ['epoch 001 lr: 0.100000',
            'train: epoch 001, train_loss: 0.5000',
            'eval: epoch: 001, acc1: 50.000%, acc5: 80.000%, test_loss: 1.5000, per_image_load_time: 0.250ms, '
            'per_image_inference_time: 0.500ms',
            'until epoch: 001, best_acc1: 50.000%',
            'epoch 002 lr: 0.100000',
            'train: epoch 002, train_loss: 0.2500',
            'eval: epoch: 002, acc1: 60.000%, acc5: 85.000%, test_loss: 1.2500, per_image_load_time: 0.250ms, '
            'per_image_inference_time: 0.500ms',
            'until epoch: 002, best_acc1: 60.000%',
            'epoch 003 lr: 0.100000',
            'train: epoch 003, train_loss: 0.7500',
            'eval: epoch: 003, acc1: 55.000%, acc5: 82.000%, test_loss: 1.3750, per_image_load_time: 0.250ms, '
            'per_image_inference_time: 0.500ms',
            'until epoch: 003, best_acc1: 60.000%',
            'epoch 004 lr: 0.100000'],
    'percent': ['epoch 001 lr: 0.100000',
                'train: epoch 001, train_loss: 0.5000',
                'until epoch: 001, best_metric: 0.000%',
                'epoch 002 lr: 0.100000',
                'train: epoch 002, train_loss: 0.2500',
                'eval: epoch: 002\ntest_loss: 0.75\nper_image_load_time: 0.1\nm: 40.0\n',
                'until epoch: 002, best_metric: 40.000%',
                'epoch 003 lr: 0.100000',
                'train: epoch 003, train_loss: 0.7500',
                'until epoch: 003, best_metric: 40.000%',
                'epoch 004 lr: 0.100000'],
    'list': ['epoch 001 lr: 0.100000',
             'train: epoch 001, train_loss: 0.5000',
             'until epoch: 001, best_metric: 0.000',
             'epoch 002 lr: 0.100000',
             'train: epoch 002, train_loss: 0.2500',
             'eval: epoch: 002\nper_image_load_time: 0.1\nm: 40.0\ntest_loss: 0.75\n',
             'until epoch: 002, best_metric: 40.000',
             'epoch 003 lr: 0.100000',
             'train: epoch 003, train_loss: 0.7500',
             'until epoch: 003, best_metric: 40.000',
             'epoch 004 lr: 0.100000'],
    'loss': ['epoch 001 lr: 0.100000',
             'train: epoch 001, train_loss: 0.5000',
             'until epoch: 001, best_loss: 0.5000',
             'epoch 002 lr: 0.100000',
             'train: epoch 002, train_loss: 0.2500',
             'until epoch: 002, best_loss: 0.2500',
             'epoch 003 lr: 0.100000',
             'train: epoch 003, train_loss: 0.7500',
             'until epoch: 003, best_loss: 0.2500',
             'epoch 004 lr: 0.100000'],
}
SECOND_RUN = {          # resumed from the latest.pth of the first run: epoch 4.  {P} is the path of latest.pth; the last line is a pattern
    'acc': ['resuming model from {P}. resume_epoch: 003, used_time: 0.000 hours, best_acc1: 60.000%, test_loss: 1.3750, lr: 0.100000',
            'using torch version',
            'epoch 004 lr: 0.100000',
            'train: epoch 004, train_loss: 0.1250',
            'eval: epoch: 004, acc1: 70.000%, acc5: 90.000%, test_loss: 1.0000, per_image_load_time: 0.250ms, '
            'per_image_inference_time: 0.500ms',
            'until epoch: 004, best_acc1: 70.000%',
            r'train done\. model: net, train time: \d+\.\d{3} hours, best_acc1: 70\.000%'],
    'percent': ['resuming model from {P}. resume_epoch: 003, used_time: 0.000 hours, best_metric: 40.000%, test_loss: 0.7500, '
                'lr: 0.100000',
                'using torch version',
                'epoch 004 lr: 0.100000',
                'train: epoch 004, train_loss: 0.1250',
                'eval: epoch: 004\ntest_loss: 0.5\nper_image_load_time: 0.1\nm: 45.5\n',
                'until epoch: 004, best_metric: 45.500%',
                r'train done\. model: net, train time: \d+\.\d{3} hours, best_metric: 45\.500%'],
    'list': ['resuming model from {P}. resume_epoch: 003, used_time: 0.000 hours, best_metric: 40.000, test_loss: 0.75, lr: 0.100000',
             'using torch version',
             'epoch 004 lr: 0.100000',
             'train: epoch 004, train_loss: 0.1250',
             'eval: epoch: 004\nper_image_load_time: 0.1\nm: 45.5\ntest_loss: 0.5\n',
             'until epoch: 004, best_metric: 45.500',
             r'train done\. model: net, train time: \d+\.\d{3} hours, best_metric: 45\.500'],
    'loss': ['resuming model from {P}. resume_epoch: 003, used_time: 0.000 hours, best_loss: 0.2500, lr: 0.100000',
             'using torch version',
             'epoch 004 lr: 0.100000',
             'train: epoch 004, train_loss: 0.1250',
             'until epoch: 004, best_loss: 0.1250',
             r'train done\. model: net, train time: \d+\.\d{3} hours, best_loss: 0\.1250'],
}
BEST_FILE = {'acc': 'net-acc70.000.pth', 'percent': 'net-metric45.500.pth', 'list': 'net-metric45.500.pth', 'loss': 'net-loss0.125.pth'}
LATEST_KEYS = {
    'acc': {'epoch', 'time', 'best_acc1', 'test_loss', 'lr', 'model_state_dict', 'optimizer_state_dict', 'scheduler_state_dict'},
    'percent': {'epoch', 'time', 'best_metric', 'test_loss', 'lr', 'model_state_dict', 'optimizer_state_dict', 'scheduler_state_dict'},
    'list': {'epoch', 'time', 'best_metric', 'test_loss', 'lr', 'model_state_dict', 'optimizer_state_dict', 'scheduler_state_dict'},
    'loss': {'epoch', 'time', 'best_loss', 'train_loss', 'lr', 'model_state_dict', 'optimizer_state_dict', 'scheduler_state_dict'},
}
NUMBER_KEYS = {'acc': ('best_acc1', 'test_loss'), 'percent': ('best_metric', 'test_loss'), 'list': ('best_metric', 'test_loss'),
               'loss': ('best_loss', 'train_loss')}
# (best value, the second number) latest.pth holds after the first run and after the second
LATEST_NUMBERS = {'acc': ((60.0, 1.375), (70.0, 1.0)), 'percent': ((40.0, 0.75), (45.5, 0.5)), 'list': ((40.0, 0.75), (45.5, 0.5)),
                  'loss': ((0.25, 0.75), (0.125, 0.125))}


# ------------------------------------------------------------------------------------------------ stand-ins
class Net(torch.nn.Module):
    def __init__(self, value):
        super().__init__()
        self.encoder = torch.nn.Linear(1, 1)                # two parameters; `.encoder` is what the MAE task saves on its own
        with torch.no_grad():
            self.encoder.weight.fill_(value)
            self.encoder.bias.fill_(value)


class Wrapper:
    """the surface of the data-parallel wrapper the driver uses: `.module` and a `module.`-prefixed state dict"""

    def __init__(self, module):
        self.module = module

    def state_dict(self):
        return {'module.' + k: v for k, v in self.module.state_dict().items()}

    def load_state_dict(self, state_dict):
        self.module.load_state_dict({k[len('module.'):]: v for k, v in state_dict.items()})


class SchedulerStub:
    current_lr = 0.1
    loaded = None

    def state_dict(self):
        return {'step': 7}

    def load_state_dict(self, state_dict):
        self.loaded = state_dict


class Interrupted(Exception):
    pass


class Stage:
    """One process's worth of stand-ins around a checkpoint directory; `run()` is what train() does from the resume on."""

    def __init__(self, checkpoint_dir, use_ema_model, epochs=4, eval_epoch=(2, )):
        self.checkpoint_dir = str(checkpoint_dir)
        self.latest = os.path.join(self.checkpoint_dir, 'latest.pth')
        self.model, self.ema = Wrapper(Net(1.0)), Wrapper(Net(2.0))
        self.optimizer = torch.optim.SGD(self.model.module.parameters(), lr=0.1)
        self.scheduler = SchedulerStub()
        self.config = types.SimpleNamespace(epochs=epochs, eval_epoch=list(eval_epoch), save_interval=2, network='net', save_model_metric='m',
                                            use_ema_model=use_ema_model, ema_model=types.SimpleNamespace(ema_model=self.ema))
        self.lines, self.sampler_epochs = [], []
        self.logger = types.SimpleNamespace(info=self.lines.append)
        self.train_loader = types.SimpleNamespace(sampler=types.SimpleNamespace(set_epoch=self.sampler_epochs.append))

    def run(self, task, local_rank=0):
        info = entry.rank0_info(self.logger, local_rank)
        start = entry.resume(task, self.latest, self.model, self.optimizer, self.scheduler, self.config, info)
        info('using torch version')
        entry.fit(task, self.model, self.optimizer, self.scheduler, self.train_loader, 'eval loaders', 'train criterion', 'test criterion',
                  self.logger, self.checkpoint_dir, local_rank, self.config, start)

    def files(self):
        return set(os.listdir(self.checkpoint_dir))


def scripted(module_name, results, stop_at=None):
    """the module's TASK with a scripted loop (the loss of LOSSES; cut off at epoch `stop_at`) and a scripted evaluation"""
    task = importlib.import_module(PKG + module_name).TASK
    results = iter(results)

    def train(train_loader, model, criterion, optimizer, scheduler, epoch, logger, config):
        assert criterion == 'train criterion'
        if epoch == stop_at:
            raise Interrupted
        return LOSSES[epoch - 1]

    def validate(loaders, model, criterion, config):
        assert (loaders, criterion) == ('eval loaders', 'test criterion')
        return next(results)

    return dataclasses.replace(task, train=train, validate=validate if task.validate else None)


def same_lines(lines, expected, path):
    assert len(lines) == len(expected), lines
    for line, want in zip(lines[:-1], expected[:-1]):
        assert line == want.replace('{P}', path)
    return lines[-1], expected[-1]


# ------------------------------------------------------------------------------------------------ the 12 training tasks
@pytest.mark.parametrize('use_ema_model', [False, True])
@pytest.mark.parametrize('module_name', list(TRAIN_TASKS))
def test_fit_and_resume_log_and_write_what_the_entry_script_did(module_name, use_ema_model, tmp_path):
    family, epoch_files, follows_ema = TRAIN_TASKS[module_name]
    encoder = ['best_encoder.pth'] if module_name == 'train_mae_self_supervised_model' else []
    keys = LATEST_KEYS[family] | ({'ema_model_state_dict'} if use_ema_model and follows_ema else set())
    best_key, second_key = NUMBER_KEYS[family]
    cut = CALLS_IN_FIRST_RUN[family]

    first = Stage(tmp_path, use_ema_model)
    with pytest.raises(Interrupted):
        first.run(scripted(module_name, EVAL_RESULTS[family][:cut], stop_at=4))
    assert first.lines == ['using torch version'] + FIRST_RUN[family]
    assert first.sampler_epochs == [1, 2, 3, 4]
    assert first.files() == {'latest.pth', 'best.pth', *encoder, *(['epoch_2.pth'] if epoch_files else [])}
    latest = torch.load(first.latest, weights_only=True)
    assert set(latest) == keys
    assert (latest['epoch'], latest[best_key], latest[second_key], latest['lr']) == (3, *LATEST_NUMBERS[family][0], 0.1)
    assert type(latest[best_key]) is float and latest['scheduler_state_dict'] == {'step': 7}
    assert set(latest['model_state_dict']) == {'module.encoder.weight', 'module.encoder.bias'}

    second = Stage(tmp_path, use_ema_model)
    with torch.no_grad():                                   # the resume has to bring both networks back
        second.model.module.encoder.weight.fill_(5.0)
        second.ema.module.encoder.weight.fill_(6.0)
    second.run(scripted(module_name, EVAL_RESULTS[family][cut:]))
    last, pattern = same_lines(second.lines, SECOND_RUN[family], second.latest)
    assert re.fullmatch(pattern, last), last
    assert second.sampler_epochs == [4] and second.scheduler.loaded == {'step': 7}
    assert float(second.model.module.encoder.weight.detach()) == 1.0
    assert float(second.ema.module.encoder.weight.detach()) == (2.0 if use_ema_model and follows_ema else 6.0)
    best_files = [BEST_FILE[family]] + [BEST_FILE[family][:-len('.pth')] + '_encoder.pth' for _ in encoder]
    assert second.files() == {'latest.pth', *best_files, *(['epoch_2.pth', 'epoch_4.pth'] if epoch_files else [])}
    latest = torch.load(second.latest, weights_only=True)
    assert set(latest) == keys
    assert (latest['epoch'], latest[best_key], latest[second_key]) == (4, *LATEST_NUMBERS[family][1])
    # whose weights the files hold: the EMA network's (filled with 2) where the task follows it, the model's (1) otherwise
    whose = 2.0 if use_ema_model and follows_ema else 1.0
    for name in best_files + (['epoch_2.pth', 'epoch_4.pth'] if epoch_files else []):
        state = torch.load(os.path.join(second.checkpoint_dir, name), weights_only=True)
        assert set(state) == ({'weight', 'bias'} if name.endswith('_encoder.pth') else {'encoder.weight', 'encoder.bias'}), name
        assert all(float(v) == whose for v in state.values()), name


def test_other_ranks_log_nothing_and_write_nothing(tmp_path):
    stage = Stage(tmp_path, False, epochs=2)
    stage.run(scripted('train_human_matting_model', EVAL_RESULTS['list']), local_rank=1)
    assert stage.lines == [] and stage.files() == set() and stage.sampler_epochs == [1, 2]


# ------------------------------------------------------------------------------------------------ the guards of the metric families
METRIC_TASKS = [name for name, (family, _, _) in TRAIN_TASKS.items() if family != 'loss']
ABOVE_100 = {'acc': [(101.0, 80.0, 1.5, 0.25, 0.5)] * 2, 'percent': [{'test_loss': 0.75, 'm': 101.0}],
             'list': [{'setA': {'m': np.float32(101.0), 'test_loss': 0.75}}]}
ABOVE_100_LINES = {
    'acc': ['epoch 001 lr: 0.100000',
            'train: epoch 001, train_loss: 0.5000',
            'eval: epoch: 001, acc1: 101.000%, acc5: 80.000%, test_loss: 1.5000, per_image_load_time: 0.250ms, '
            'per_image_inference_time: 0.500ms',
            'until epoch: 001, best_acc1: 0.000%',
            'epoch 002 lr: 0.100000',
            'train: epoch 002, train_loss: 0.2500',
            'eval: epoch: 002, acc1: 101.000%, acc5: 80.000%, test_loss: 1.5000, per_image_load_time: 0.250ms, '
            'per_image_inference_time: 0.500ms',
            'until epoch: 002, best_acc1: 0.000%',
            r'train done\. model: net, train time: \d+\.\d{3} hours, best_acc1: 0\.000%'],
    'percent': ['epoch 001 lr: 0.100000',
                'train: epoch 001, train_loss: 0.5000',
                'until epoch: 001, best_metric: 0.000%',
                'epoch 002 lr: 0.100000',
                'train: epoch 002, train_loss: 0.2500',
                'eval: epoch: 002\ntest_loss: 0.75\nm: 101.0\n',
                'until epoch: 002, best_metric: 0.000%',
                r'train done\. model: net, train time: \d+\.\d{3} hours, best_metric: 0\.000%'],
    'list': ['epoch 001 lr: 0.100000',
             'train: epoch 001, train_loss: 0.5000',
             'until epoch: 001, best_metric: 0.000',
             'epoch 002 lr: 0.100000',
             'train: epoch 002, train_loss: 0.2500',
             'eval: epoch: 002\nm: 101.0\ntest_loss: 0.75\n',
             'until epoch: 002, best_metric: 0.000',
             r'train done\. model: net, train time: \d+\.\d{3} hours, best_metric: 0\.000'],
}


@pytest.mark.parametrize('module_name', METRIC_TASKS)
def test_a_metric_above_100_does_not_become_the_best(module_name, tmp_path):
    family = TRAIN_TASKS[module_name][0]
    stage = Stage(tmp_path, False, epochs=2, eval_epoch=())
    stage.run(scripted(module_name, ABOVE_100[family]))
    last, pattern = same_lines(stage.lines, ['using torch version'] + ABOVE_100_LINES[family], stage.latest)
    assert re.fullmatch(pattern, last), last
    assert stage.files() == {'latest.pth', *(['epoch_2.pth'] if TRAIN_TASKS[module_name][1] else [])}
    latest = torch.load(stage.latest, weights_only=True)
    assert latest['best_acc1' if family == 'acc' else 'best_metric'] == 0


EMPTY = {'percent': [{'test_loss': 0.75, 'm': 40.0}, {}], 'list': [{'setA': {'m': np.float32(40.0), 'test_loss': 0.75}}, {'setA': {}}]}
EMPTY_LINES = {
    'percent': ['epoch 001 lr: 0.100000',
                'train: epoch 001, train_loss: 0.5000',
                'until epoch: 001, best_metric: 0.000%',
                'epoch 002 lr: 0.100000',
                'train: epoch 002, train_loss: 0.2500',
                'eval: epoch: 002\ntest_loss: 0.75\nm: 40.0\n',
                'until epoch: 002, best_metric: 40.000%',
                'epoch 003 lr: 0.100000',
                'train: epoch 003, train_loss: 0.7500',
                'eval: epoch: 003\n',                      # the flat family logs the head of the block even so, as it did
                'until epoch: 003, best_metric: 40.000%',
                r'train done\. model: net, train time: \d+\.\d{3} hours, best_metric: 40\.000%'],
    'list': ['epoch 001 lr: 0.100000',
             'train: epoch 001, train_loss: 0.5000',
             'until epoch: 001, best_metric: 0.000',
             'epoch 002 lr: 0.100000',
             'train: epoch 002, train_loss: 0.2500',
             'eval: epoch: 002\nm: 40.0\ntest_loss: 0.75\n',
             'until epoch: 002, best_metric: 40.000',
             'epoch 003 lr: 0.100000',
             'train: epoch 003, train_loss: 0.7500',
             'until epoch: 003, best_metric: 40.000',       # no `eval:` block for an empty first dataset
             r'train done\. model: net, train time: \d+\.\d{3} hours, best_metric: 40\.000'],
}


@pytest.mark.parametrize('module_name', [name for name in METRIC_TASKS if TRAIN_TASKS[name][0] != 'acc'])
def test_an_empty_result_leaves_metric_and_test_loss_as_they_were(module_name, tmp_path):
    family = TRAIN_TASKS[module_name][0]
    stage = Stage(tmp_path, False, epochs=3)
    stage.run(scripted(module_name, EMPTY[family]))
    last, pattern = same_lines(stage.lines, ['using torch version'] + EMPTY_LINES[family], stage.latest)
    assert re.fullmatch(pattern, last), last
    assert stage.files() == {'latest.pth', 'net-metric40.000.pth', *(['epoch_2.pth'] if TRAIN_TASKS[module_name][1] else [])}
    latest = torch.load(stage.latest, weights_only=True)
    assert (latest['epoch'], latest['best_metric'], latest['test_loss']) == (3, 40.0, 0.75)


# ------------------------------------------------------------------------------------------------ the 9 test tasks: the report step
DATASETS = {'setA[+]setB': {'per_image_load_time': 0.1, 'miou_average': 40.0}, 'setB': {'miou_average': 1.5}}
DATASET_BLOCKS = ['eval dataset:setA[+]setB\nper_image_load_time: 0.1\nmiou_average: 40.0\n', 'eval dataset:setB\nmiou_average: 1.5\n']
FLAT = {'test_loss': 0.75, 'per_image_load_time': 0.1, 'mean_iou': 40.0}
REPORTS = {
    'test_classification_model': ((60.0, 85.0, 1.25, 0.25, 0.5),
                                  ['acc1: 60.000%, acc5: 85.000%, test_loss: 1.2500, per_image_load_time: 0.250ms, '
                                   'per_image_inference_time: 0.500ms']),
    'test_detection_model': ({'IoU=0.50:0.95,area=all,maxDets=100,mAP': 0.25, 'per_image_load_time': 0.1},
                             ['eval type: VOC\nIoU=0.50:0.95,area=all,maxDets=100,mAP: 0.25\nper_image_load_time: 0.1\n']),
    'test_semantic_segmentation_model': (FLAT, ['eval result:\ntest_loss: 0.75\nper_image_load_time: 0.1\nmean_iou: 40.0\n']),
    'test_universal_segmentation_model_for_semantic_segmentation_dataset':
        (FLAT, ['eval result:\ntest_loss: 0.75\nper_image_load_time: 0.1\nmean_iou: 40.0\n']),
    'test_salient_object_detection_model': (DATASETS, DATASET_BLOCKS),
    'test_human_matting_model': (DATASETS, DATASET_BLOCKS),
    'test_face_parsing_model': (DATASETS, DATASET_BLOCKS),
    'test_human_parsing_model': (DATASETS, DATASET_BLOCKS),
    'test_text_recognition_model': (DATASETS, DATASET_BLOCKS),
}


@pytest.mark.parametrize('module_name', list(REPORTS))
def test_report_of_each_test_task(module_name):
    task = importlib.import_module(PKG + module_name).TASK
    result, expected = REPORTS[module_name]
    lines = []
    task.report(result, types.SimpleNamespace(eval_type='VOC'), lines.append)
    assert lines == expected


def test_what_each_test_task_hands_its_evaluation_function():
    """(model line, arguments between the model and the config) where a task departs from `flops / macs / params` and the test criterion"""
    criterion = types.SimpleNamespace(cuda=lambda: 'criterion on the device')
    config = types.SimpleNamespace(test_criterion=criterion, decoder='decoder')
    args = {name: importlib.import_module(PKG + name).TASK.extra_args(config) for name in REPORTS}
    assert args.pop('test_detection_model') == ('criterion on the device', 'decoder')
    assert args.pop('test_universal_segmentation_model_for_semantic_segmentation_dataset') == ('decoder', )
    assert set(args.values()) == {('criterion on the device', )}
    text = importlib.import_module(PKG + 'test_text_recognition_model').TASK
    assert text.describe(config, Net(0.0)) == 'params: 2'


# ------------------------------------------------------------------------------------------------ the 21 entry modules
DESCRIPTIONS = {
    'train_classification_model': 'PyTorch Classification Training (MI355X engine)',
    'train_detection_model': 'PyTorch Detection Training (MI355X engine)',
    'train_face_parsing_model': 'PyTorch Face Parsing Training (MI355X engine)',
    'train_human_matting_model': 'PyTorch Human Matting Training (MI355X engine)',
    'train_human_parsing_model': 'PyTorch Human Parsing Training (MI355X engine)',
    'train_interactive_matting_model': 'PyTorch Interactive Matting Training (MI355X engine)',
    'train_interactive_segmentation_model': 'PyTorch Interactive Segmentation Training (MI355X engine)',
    'train_mae_self_supervised_model': 'PyTorch MAE Self Supervised Learning Training (MI355X engine)',
    'train_salient_object_detection_model': 'PyTorch Salient Object Detection Training (MI355X engine)',
    'train_semantic_segmentation_model': 'PyTorch Semantic Segmentation Training (MI355X engine)',
    'train_text_recognition_model': 'PyTorch Text Recognition Training (MI355X engine)',
    'train_universal_segmentation_model': 'PyTorch Universal Segmentation Training (MI355X engine)',
    'test_classification_model': 'PyTorch Classification Testing (MI355X engine)',
    'test_detection_model': 'PyTorch Detection Testing (MI355X engine)',
    'test_face_parsing_model': 'PyTorch Face Parsing Testing (MI355X engine)',
    'test_human_matting_model': 'PyTorch Human Matting Testing (MI355X engine)',
    'test_human_parsing_model': 'PyTorch Human Parsing Testing (MI355X engine)',
    'test_salient_object_detection_model': 'PyTorch Salient Object Detection Testing (MI355X engine)',
    'test_semantic_segmentation_model': 'PyTorch Semantic Segmentation Testing (MI355X engine)',
    'test_text_recognition_model': 'PyTorch Text Recognition Testing (MI355X engine)',
    'test_universal_segmentation_model_for_semantic_segmentation_dataset': 'PyTorch Universal Segmentation Testing (MI355X engine)',
}


def test_the_21_entry_modules_keep_their_surface(monkeypatch):
    assert set(DESCRIPTIONS) == set(TRAIN_TASKS) | set(REPORTS) and len(DESCRIPTIONS) == 21
    monkeypatch.setattr(argparse.ArgumentParser, 'parse_args', lambda self: self)           # parse_args() -> its parser
    for name, description in DESCRIPTIONS.items():
        m = importlib.import_module(PKG + name)
        assert importlib.import_module('tools.' + name) is m                                # the reference spelling
        assert callable(m.main) and callable(m.parse_args)
        parser = m.parse_args()
        assert parser.description == description
        assert [a.dest for a in parser._actions] == ['help', 'work_dir']
        assert f'-m {PKG}{name} --work-dir ./' in m.__doc__
        assert isinstance(m.TASK, entry.TrainTask if name.startswith('train_') else entry.TestTask)
