"""tools/text_scripts.py on the GPU: train_text_recognition over tools/loop.py run_epoch with accumulation 1 and 2, fused against composed
CTCLoss trajectories, test_text_recognition_for_all_dataset and its keys, a variable-width batch -- on a stand-in with the
model's contract (images [B, 3, 32, W] -> logits [B, W / 4, C]): two linear layers over groups of four image columns, torch ops
only, so that what is under test is the loops, the CTC loss and the greedy decode, and the two routes can be compared without
BatchNorm and LSTM in between.  tests/test_gpu_text_recognition.py runs the same helpers with CTCModel."""
import logging

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

BATCH, HEIGHT, WIDTH = 8, 32, 96
CHARS = list('0123456789abcdefghijklmnopqrstuvwxyz')


class ColumnModel(nn.Module):

    def __init__(self, num_classes, hidden=128):
        super().__init__()
        self.linear1 = nn.Linear(3 * HEIGHT * 4, hidden)
        self.linear2 = nn.Linear(hidden, num_classes)

    def forward(self, x):
        b, c, h, w = x.shape
        x = x.permute(0, 3, 1, 2).reshape(b, w // 4, 4 * c * h)
        return self.linear2(torch.relu(self.linear1(x)))                     # [B, T, C]


class _Repeat(torch.utils.data.Dataset):
    """the same `period` samples over and over: a batch a model can memorise"""

    def __init__(self, base, length, period):
        self.base, self.length, self.period = base, length, period

    def __len__(self):
        return self.length

    def __getitem__(self, i):
        return self.base[i % self.period]


def _setup(iterations, accumulation_steps=1, route='fused', variable_width=False, lr=3e-3, model_fn=None, **overrides):
    from SimpleAICV.text_recognition import losses
    from SimpleAICV.text_recognition.common import CTCTextLabelConverter, KeepRatioResizeTextRecognitionCollater
    from SimpleAICV.text_recognition.datasets.syntheticdataset import SyntheticTextRecognitionDataset
    from simpleaicv_pytorch_training_examples_amd.tools import utils

    class config:
        pass
    config.all_char_table = CHARS
    config.converter = CTCTextLabelConverter(CHARS, str_max_length=12, garbage_char='㍿')
    config.num_classes = config.converter.num_classes
    config.loss_ratio = {'CTCLoss': 1.0}
    config.train_criterion = {'CTCLoss': losses.CTCLoss(blank_index=config.converter.blank_index)}
    config.test_criterion = losses.CTCLoss(blank_index=config.converter.blank_index)
    config.train_criterion['CTCLoss'].route = config.test_criterion.route = route
    config.optimizer = ('AdamW', {'lr': lr, 'global_weight_decay': False, 'weight_decay': 1e-3, 'no_weight_decay_layer_name_list': []})
    config.scheduler = ('MultiStepLR', {'warm_up_epochs': 0, 'gamma': 0.1, 'milestones': [100]})
    config.epochs, config.batch_size, config.accumulation_steps, config.print_interval = 1, BATCH, accumulation_steps, 1
    config.use_amp, config.use_ema_model, config.local_rank, config.gpus_num, config.group = False, False, 0, 1, None
    config.sync_bn, config.host_sync_lag = False, 2
    for k, v in overrides.items():
        setattr(config, k, v)
    collater = KeepRatioResizeTextRecognitionCollater(resize_h=HEIGHT)
    make = lambda n, seed: SyntheticTextRecognitionDataset(n, CHARS, height=HEIGHT, width=WIDTH, max_length=6, seed=seed,      # noqa: E731
                                                            variable_width=variable_width)
    loader = torch.utils.data.DataLoader(_Repeat(make(BATCH, 0), iterations * BATCH, BATCH), batch_size=BATCH, shuffle=False,
                                         drop_last=True, collate_fn=collater)
    config.val_dataset_name_list = [['synthetic', f'part/{i}'] for i in range(2)]
    config.val_loader_list = [torch.utils.data.DataLoader(make(2 * BATCH, 10 + i), batch_size=BATCH, shuffle=False, collate_fn=collater)
                              for i in range(2)]
    torch.manual_seed(0)
    model = (model_fn or ColumnModel)(config.num_classes + 1).cuda()
    optimizer, _ = utils.build_optimizer(config, model)
    scheduler = utils.Scheduler(config, optimizer)
    model, config.ema_model, config.scaler = utils.build_training_mode(config, model)
    return config, model, optimizer, scheduler, loader


def _train(config, model, optimizer, scheduler, loader):
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.classification import common
    from simpleaicv_pytorch_training_examples_amd.tools import text_scripts
    got, orig = [], common.AverageMeter.update

    def spy(self, val, n=1):
        got.append(float(val))
        return orig(self, val, n)

    common.AverageMeter.update = spy
    try:
        avg = text_scripts.train_text_recognition(loader, model, config.train_criterion, optimizer, scheduler, 1,
                                                  logging.getLogger('saicv_text'), config)
    finally:
        common.AverageMeter.update = orig
    assert np.isfinite(avg) and all(np.isfinite(v) for v in got)
    return got


@pytest.mark.parametrize('accumulation_steps', [1, 2])
def test_three_optimizer_steps_lower_the_loss_on_a_memorisable_batch(accumulation_steps):
    got = _train(*_setup(4 * accumulation_steps, accumulation_steps))
    print('losses', got)
    # the loop's meter takes one entry per OPTIMIZER step, before the step: the fourth has seen three steps
    assert len(got) == 4
    assert got[-1] < 0.9 * got[0], got


def test_fused_and_composed_trajectories_agree():
    """the same six iterations with either route: the kernel differs from the reference formula by fp32 rounding per step (4 x the
    reference's own error, tests/test_gpu_ctc_kernels.py), and six AdamW steps do not amplify that beyond the project's 1e-3"""
    a = _train(*_setup(6, route='fused'))
    b = _train(*_setup(6, route='composed'))
    worst = max(abs(x - y) / abs(y) for x, y in zip(a, b))
    print('fused', a, 'composed', b, f'largest relative difference {worst:.3e}')
    assert len(a) == len(b) == 6
    assert worst < 1e-3


def test_validation_returns_the_six_keys_per_validation_set():
    from simpleaicv_pytorch_training_examples_amd.tools import text_scripts
    config, model, optimizer, scheduler, loader = _setup(40, lr=1e-2)
    before = text_scripts.test_text_recognition_for_all_dataset(config.val_loader_list, model, config.test_criterion, config)
    assert list(before) == ['synthetic[+]part[s]0', 'synthetic[+]part[s]1']
    for r in before.values():
        assert {'test_loss', 'str_acc', 'not_included_str_percent', 'final_edit_distance', 'lcs_precision', 'lcs_recall'} <= set(r)
        assert all(np.isfinite(float(r[k])) for k in r) and r['not_included_str_percent'] == 0
        assert 0 <= r['str_acc'] <= 100 and 0 <= r['lcs_precision'] <= 100 and 0 <= r['lcs_recall'] <= 100
    first = before['synthetic[+]part[s]0']
    assert text_scripts.first_dataset_metric(before, 'lcs_precision') == (first, first['lcs_precision'], first['test_loss'])
    # the training batch, validated before and after the model has seen it 40 times: the loss has fallen, and the figures are
    # those of the reference's own expressions (outputs.max(dim=2), converter.decode) on the same outputs
    config.val_dataset_name_list = [['memorised']]
    one = torch.utils.data.DataLoader(loader.dataset.base, batch_size=BATCH, shuffle=False, collate_fn=loader.collate_fn)
    r0 = text_scripts.test_text_recognition_for_all_dataset([one], model, config.test_criterion, config)['memorised']
    _train(config, model, optimizer, scheduler, loader)
    r = text_scripts.test_text_recognition_for_all_dataset([one], model, config.test_criterion, config)['memorised']
    print(r0, r)
    assert r['test_loss'] < 0.5 * r0['test_loss']
    batch = next(iter(one))
    with torch.no_grad():
        outputs = model(batch['image'].cuda())
    _, index = outputs.max(dim=2)
    strs = config.converter.decode(index.cpu().numpy(), [outputs.shape[1]] * BATCH)
    c = text_scripts.string_counts(strs, batch['label'], ''.join(CHARS), '㍿')
    assert r['str_acc'] == c['correct'] / BATCH * 100 and r['final_edit_distance'] == c['ne_distance'] / BATCH * 100
    assert r['lcs_precision'] == (c['lcs'] / c['pred_chars'] * 100 if c['pred_chars'] else 0)
    assert r['lcs_recall'] == c['lcs'] / c['target_chars'] * 100
    # the composed route on the same model gives the same figures (arg-max and strings are exact)
    config.test_criterion.route = 'composed'
    r2 = text_scripts.test_text_recognition_for_all_dataset([one], model, config.test_criterion, config)['memorised']
    assert r2['str_acc'] == r['str_acc'] and abs(r2['test_loss'] - r['test_loss']) <= 1e-3 * max(r['test_loss'], 1e-3)


def test_variable_width_batches_run():
    got = _train(*_setup(3, variable_width=True))
    assert len(got) == 3
