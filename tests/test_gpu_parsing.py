"""PFAN human and face parsing end to end on the GPU: resnet18_pfan_human_parsing against the fixture the REFERENCE produced
(tests/golden/pfan_parse_r18_tiny.pt: scripts/record_pfan_parsing_golden.py runs SimpleAICV/human_parsing/models/pfan_human_parsing.py
and the reference CELoss + IoULoss('softmax') on the CPU in fp32), the training loop, the captured step and the validation; one
test takes the 19-class face family through a training step and a validation.  Mirrors tests/test_gpu_semseg.py, bounds included.

Same seed => bit-identical initial weights (checked on samples of every tensor).  fp32 parity mode, the bounds of
tests/test_gpu_retinanet.py (a BatchNorm backbone at batch 2): output within 1e-3 of its scale, both losses within 1e-3, gradient
norms within 2e-2, gradient samples within 4e-2 of the tensor's gradient scale (two BatchNorm biases have an exactly zero gradient
and no scale of their own: see the test), BatchNorm buffers within 1e-3.  bf16: output within twice the
reference's own bf16-autocast deviation (stored in the fixture), floor 1e-2."""
import logging
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_err

pytestmark = pytest.mark.gpu


def _sample_idx(numel, k=16):
    return torch.linspace(0, numel - 1, min(k, numel)).long()


def _build():
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.human_parsing import models
    fx = torch.load(os.path.join(GOLDEN, 'pfan_parse_r18_tiny.pt'), weights_only=True)
    torch.manual_seed(0)
    model = models.resnet18_pfan_human_parsing(**fx['config'])
    sd = model.state_dict()
    assert set(fx['init_sample']) == {k for k, v in sd.items() if v.dtype.is_floating_point}
    for k, ref in fx['init_sample'].items():
        assert torch.equal(sd[k].flatten()[_sample_idx(sd[k].numel())], ref), f'initial weights differ: {k}'
    b, c, h, w = fx['input_shape']
    x = torch.randn(b, h, w, c, generator=torch.Generator().manual_seed(1)).permute(0, 3, 1, 2)
    mask = torch.randint(0, fx['config']['num_classes'], (b, h, w), generator=torch.Generator().manual_seed(2)).float()
    return fx, model.cuda().train(), x.cuda(), mask.cuda()


def test_pfan_fp32_matches_reference(deterministic):
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.human_parsing.losses import CELoss, IoULoss
    fx, model, x, mask = _build()
    out = model(x)
    assert tuple(out.shape) == tuple(fx['out'].shape) and out.dtype == torch.float32
    print('output rel_err', rel_err(out.cpu(), fx['out']))
    assert rel_err(out.cpu(), fx['out']) < 1e-3
    loss = {'CELoss': CELoss()(out, mask), 'IoULoss': IoULoss(logit_type='softmax')(out, mask)}
    for name, value in loss.items():
        print(name, float(value.detach()), fx['loss'][name])
        assert abs(float(value.detach()) - fx['loss'][name]) < 1e-3
    sum(loss.values()).backward()
    params = dict(model.named_parameters())
    assert set(fx['grad_norm']) == {k for k, p in params.items() if p.grad is not None}
    # A tensor whose exact gradient is zero (a BatchNorm bias in front of a pointwise convolution + batch-statistics BatchNorm: the
    # next normalisation removes a per-channel shift) has no gradient scale of its own: the reference's fp32 numbers for it are
    # rounding noise (its float64 run gives a norm ten orders of magnitude smaller, recorded in the fixture).  Such a tensor is
    # held to zero within 4e-2 of the scale of its layer's weight gradient; every other tensor to its own scale.
    exact_zero = {k for k, n in fx['grad_norm'].items() if fx['grad_norm64'][k] < 1e-3 * n}
    print('exactly-zero gradients', sorted(exact_zero))
    assert exact_zero == {'high_level_conv.layer.1.bias', 'low_level_conv.layer.1.bias'}      # both feed reduce_conv1 (1x1 conv + BN)
    for k, n in fx['grad_norm'].items():
        g = params[k].grad.float().cpu()
        assert abs(float(g.norm()) - n) <= 2e-2 * max(n, 1e-6), (k, float(g.norm()), n)
        if k in exact_zero:
            scale = float(params[k[:-len('bias')] + 'weight'].grad.abs().max())
            assert float(g.abs().max()) <= 4e-2 * scale, (k, float(g.abs().max()), scale)
            continue
        ref = fx['grad_sample'][k]
        assert float((g.flatten()[_sample_idx(g.numel())] - ref).abs().max()) <= 4e-2 * max(float(g.abs().max()), 1e-12), k
    # The same for a running mean that is exactly zero (reduce_conv1: a pointwise convolution of two zero-mean BatchNorm outputs;
    # upsample_conv1: a bias-free transposed convolution of reduce_conv1's zero-mean output):
    # what the reference's fp32 run holds there is rounding noise, so the value is held to zero within 1e-3 of the scale a mean has
    # inside its normalisation, the standard deviation (sqrt of the layer's running variance).
    sd = model.state_dict()
    zero_stat = {k for k, v in fx['bn_buffers'].items() if fx['bn_absmax64'][k] < 1e-3 * float(v.abs().max())}
    print('exactly-zero statistics', sorted(zero_stat))
    assert zero_stat == {'reduce_conv1.layer.1.running_mean', 'upsample_conv1.layer.1.running_mean'}
    for k, v in fx['bn_buffers'].items():
        if k in zero_stat:
            std = fx['bn_buffers'][k.replace('running_mean', 'running_var')].sqrt()
            assert float(sd[k].float().cpu().abs().max()) <= 1e-3 * float(std.max()), k
            continue
        assert rel_err(sd[k].float().cpu(), v) < 1e-3, k


def test_pfan_bf16_autocast_stays_close():
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.human_parsing.losses import CELoss, IoULoss
    fx, model, x, mask = _build()
    with torch.autocast('cuda', dtype=torch.bfloat16):
        out = model(x)
        loss = CELoss()(out, mask) + IoULoss(logit_type='softmax')(out, mask)
    assert out.dtype == torch.bfloat16
    err = rel_err(out.float().cpu(), fx['out'])
    print('bf16 output rel_err', err, 'reference bf16 deviation', fx['bf16_dev'])
    assert err < max(2 * fx['bf16_dev'], 1e-2)
    loss.backward()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)


# ------------------------------------------------------------------------------------------------ loops
NUM_CLASSES, HEIGHT, WIDTH, BATCH = 20, 64, 96, 4


class _Poisoned(torch.utils.data.Dataset):

    def __init__(self, base, poison):
        self.base, self.poison = base, set(poison)

    def __len__(self):
        return len(self.base)

    def __getitem__(self, i):
        sample = self.base[i]
        if i in self.poison:
            sample['image'][0, 0, 0] = float('nan')
        return sample


def _setup(num_samples, poison=(), use_amp=True, lr=2e-3, family='human', val_sets=1, **overrides):
    import importlib
    from simpleaicv_pytorch_training_examples_amd.tools import utils
    pkg = f'simpleaicv_pytorch_training_examples_amd.SimpleAICV.{family}_parsing'
    losses, models, common = (importlib.import_module(f'{pkg}.{m}') for m in ('losses', 'models', 'common'))
    synthetic = importlib.import_module(f'{pkg}.datasets.syntheticdataset')
    Family = family.capitalize()
    dataset_cls, collater_cls = getattr(synthetic, f'Synthetic{Family}ParsingDataset'), getattr(common, f'{Family}ParsingCollater')
    num_classes = NUM_CLASSES if family == 'human' else 19

    class config:
        pass
    config.network = f'resnet18_pfan_{family}_parsing'
    config.num_classes = num_classes
    config.loss_ratio = {'CELoss': 1.0, 'IoULoss': 1.0}
    config.train_criterion = {'CELoss': losses.CELoss(), 'IoULoss': losses.IoULoss(logit_type='softmax')}
    config.test_criterion = losses.CELoss()
    config.optimizer = ('AdamW', {'lr': lr, 'global_weight_decay': False, 'weight_decay': 1e-3, 'no_weight_decay_layer_name_list': []})
    config.scheduler = ('MultiStepLR', {'warm_up_epochs': 0, 'gamma': 0.1, 'milestones': [100]})
    config.epochs, config.batch_size, config.accumulation_steps, config.print_interval = 1, BATCH, 1, 1
    config.use_amp, config.use_ema_model, config.local_rank, config.gpus_num, config.group = use_amp, False, 0, 1, None
    config.sync_bn, config.host_sync_lag = False, 2
    for k, v in overrides.items():
        setattr(config, k, v)
    collater = collater_cls(resize=WIDTH)
    dataset = _Poisoned(dataset_cls(num_samples, HEIGHT, WIDTH, seed=0), poison)
    assert dataset.base.num_classes == num_classes                  # the family's default
    loader = torch.utils.data.DataLoader(dataset, batch_size=BATCH, shuffle=False, drop_last=True, collate_fn=collater)
    config.val_dataset_name_list = [['synthetic', f'part/{i}'] for i in range(val_sets)]
    config.val_loader_list = [torch.utils.data.DataLoader(dataset_cls(2 * BATCH, HEIGHT, WIDTH, seed=10 + i), batch_size=BATCH,
                                                          shuffle=False, collate_fn=collater) for i in range(val_sets)]
    torch.manual_seed(0)
    model = models.__dict__[config.network]().cuda()
    assert model.pred_conv.out_channels == num_classes
    optimizer, _ = utils.build_optimizer(config, model)
    scheduler = utils.Scheduler(config, optimizer)
    model, config.ema_model, config.scaler = utils.build_training_mode(config, model)
    return config, model, optimizer, scheduler, loader


def _spy_average_meter():
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.classification import common
    got, orig = [], common.AverageMeter.update

    def spy(self, val, n=1):
        got.append(float(val))
        return orig(self, val, n)

    common.AverageMeter.update = spy
    return got, lambda: setattr(common.AverageMeter, 'update', orig)


def test_train_human_parsing_learns_and_logs(caplog):
    from simpleaicv_pytorch_training_examples_amd.tools import human_parsing_scripts as scripts
    steps = 12
    config, model, optimizer, scheduler, loader = _setup(steps * BATCH)
    logger = logging.getLogger('saicv_parsing')
    logger.setLevel(logging.INFO)
    got, restore = _spy_average_meter()
    try:
        with caplog.at_level(logging.INFO, logger='saicv_parsing'):
            avg = scripts.train_human_parsing(loader, model, config.train_criterion, optimizer, scheduler, 1, logger, config)
    finally:
        restore()
    print('losses', got)
    assert len(got) == steps and all(np.isfinite(v) for v in got) and np.isfinite(avg)
    assert sum(got[-4:]) / 4 < sum(got[:4]) / 4, got
    assert 'skip this batch!' not in caplog.text
    lines = re.findall(r'train: epoch 0001, iter \[(\d{5}), 00012\], lr: \d\.\d{6}, loss: (\d+\.\d{4}), CELoss: (\d+\.\d{4}), '
                       r'IoULoss: (\d+\.\d{4}), $', caplog.text, flags=re.M)
    assert [int(i) for i, _, _, _ in lines] == list(range(1, steps + 1)), caplog.text
    assert all(abs(float(total) - float(ce) - float(iou)) <= 1.51e-4 for _, total, ce, iou in lines)      # three values printed with four decimals
    assert all(0. < float(iou) <= 1. for _, _, _, iou in lines)
    for p in model.parameters():
        assert torch.isfinite(p).all()


def test_poisoned_batch_is_skipped_and_leaves_parameters_untouched(caplog):
    from simpleaicv_pytorch_training_examples_amd.tools import human_parsing_scripts as scripts
    config, model, optimizer, scheduler, loader = _setup(BATCH, poison=(2,))
    before = model.arena.flat_param.clone()
    logger = logging.getLogger('saicv_parsing_skip')
    logger.setLevel(logging.INFO)
    with caplog.at_level(logging.INFO, logger='saicv_parsing_skip'):
        scripts.train_human_parsing(loader, model, config.train_criterion, optimizer, scheduler, 1, logger, config)
    assert caplog.text.count('skip this batch!') == 1
    assert torch.equal(before, model.arena.flat_param)


def test_step_graph_replays_the_same_training_as_eager_launches(deterministic):
    """The iteration has static shapes and no host read: config.use_step_graph captures it whole.  One eager warm-up iteration, the
    capture, two replays; deterministic mode: losses and parameters after 3 iterations equal the eager loop's bit for bit."""
    from simpleaicv_pytorch_training_examples_amd.tools import human_parsing_scripts as scripts
    steps = 3

    def run(use_graph):
        config, model, optimizer, scheduler, loader = _setup(steps * BATCH, use_step_graph=use_graph, step_graph_warmup=1)
        got, restore = _spy_average_meter()
        try:
            scripts.train_human_parsing(loader, model, config.train_criterion, optimizer, scheduler, 1,
                                        logging.getLogger('saicv_parsing_graph'), config)
        finally:
            restore()
        torch.cuda.synchronize()
        return got, model.arena.flat_param.clone(), getattr(config, '_saicv_step_graphs', {})

    eager, p_eager, _ = run(False)
    graph, p_graph, graphs = run(True)
    assert len(graphs) == 1 and next(iter(graphs.values())).graph is not None and next(iter(graphs.values())).replays == steps - 1
    print('losses eager', eager, 'graph', graph)
    assert len(eager) == steps and eager == graph
    assert torch.equal(p_eager, p_graph), float((p_eager - p_graph).norm() / p_eager.norm())


def _check_result(result, num_classes):
    head = ['test_loss', 'per_image_load_time', 'per_image_inference_time', 'exist_num_class', 'mean_precision', 'mean_recall',
            'mean_iou', 'mean_dice']
    per_class = [f'class_{i}_{name}' for name in ('precision', 'recall', 'iou', 'dice') for i in range(num_classes)]
    assert list(result) == head + per_class
    assert np.isfinite(result['test_loss']) and result['per_image_load_time'].endswith('ms')
    assert 1 <= result['exist_num_class'] <= num_classes
    for key in head[4:] + per_class:
        assert 0. <= result[key] <= 100., (key, result[key])


def test_validation_returns_the_reference_keys_per_validation_set():
    from simpleaicv_pytorch_training_examples_amd.tools import human_parsing_scripts as scripts
    config, model, _, _, _ = _setup(BATCH, val_sets=2)
    results = scripts.validate_human_parsing_for_all_dataset(config.val_loader_list, model, config.test_criterion, config)
    assert list(results) == ['synthetic[+]part[s]0', 'synthetic[+]part[s]1']
    for result in results.values():
        _check_result(result, NUM_CLASSES)
    total, metric, test_loss = scripts.first_dataset_metric(results, 'mean_iou')
    assert total is results['synthetic[+]part[s]0'] and metric == total['mean_iou'] and test_loss == total['test_loss']


def test_face_parsing_trains_and_validates():
    from simpleaicv_pytorch_training_examples_amd.tools import face_parsing_scripts as scripts
    config, model, optimizer, scheduler, loader = _setup(BATCH, family='face')
    before = model.arena.flat_param.clone()
    avg = scripts.train_face_parsing(loader, model, config.train_criterion, optimizer, scheduler, 1, logging.getLogger('saicv_face'), config)
    assert np.isfinite(avg) and not torch.equal(before, model.arena.flat_param)
    results = scripts.validate_face_parsing_for_all_dataset(config.val_loader_list, model, config.test_criterion, config)
    assert len(results) == 1
    _check_result(next(iter(results.values())), 19)
