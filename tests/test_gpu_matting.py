"""PFAN human matting end to end on the GPU: resnet18_pfan_matting against the fixture the REFERENCE produced
(tests/golden/pfan_mat_r18_tiny.pt: scripts/record_pfan_matting_golden.py runs SimpleAICV/human_matting/models/pfan_matting.py and
the reference losses on the CPU in fp32), the training loop, the captured step and the validation.

Same seed => bit-identical initial weights (tests/test_matting_host.py).  fp32 parity mode, the bounds of tests/test_gpu_salient.py:
global_pred and local_pred within 1e-3 of their scale; fused_pred compared only where the recorded two largest global
probabilities lie at least 2e-3 apart (elsewhere other arithmetic may take the other branch of collaborative_matting; at most 2 %
of the pixels may be left out, the reference's input has 1.35 %); the seven losses on the RECORDED outputs within 1e-3; for the
sum of the four argmax-free losses gradient norms within 2e-2, gradient samples within 4e-2 of the tensor's gradient scale,
BatchNorm buffers within 1e-3; the tensors that are exactly zero by construction (found from the fixture's float64 run) are
treated as that file treats them.  bf16: outputs within twice the reference's own bf16-autocast deviation, floor 1e-2."""
import logging
import os
import re

import numpy as np
import pytest
import torch

import matting_common as M
from conftest import GOLDEN, rel_err

pytestmark = pytest.mark.gpu

NAMES = list(M.LOSS_NAMES)


def _sample_idx(numel, k=16):
    return torch.linspace(0, numel - 1, min(k, numel)).long()


def _build():
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.human_matting import models
    fx = torch.load(os.path.join(GOLDEN, 'pfan_mat_r18_tiny.pt'), weights_only=True)
    torch.manual_seed(0)
    model = models.resnet18_pfan_matting(**fx['config'])
    x, alpha, trimap, fg, bg = M.model_inputs(fx['input_shape'])
    return fx, model.cuda().train(), [t.cuda() for t in (x, alpha, trimap, fg, bg)]


def _criterion():
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.human_matting import losses
    return {name: losses.__dict__[name]() for name in NAMES}


def _losses(names, outs, data):
    from simpleaicv_pytorch_training_examples_amd.tools.human_matting_scripts import matting_losses
    x, alpha, trimap, fg, bg = data
    crit = _criterion()
    return matting_losses({n: crit[n] for n in names}, {n: 1.0 for n in names}, outs, x, alpha, trimap, fg, bg)


def _check_outputs(outs, fx, tol):
    g, l, f = (o.float().cpu() for o in outs)
    errs = {'global': rel_err(g, fx['out'][0]), 'local': rel_err(l, fx['out'][1])}
    top2 = torch.sort(fx['out'][0], dim=1, descending=True)[0]
    clear = ((top2[:, 0] - top2[:, 1]) >= 2e-3).unsqueeze(1)
    left_out = 1. - float(clear.float().mean())
    errs['fused'] = rel_err(f[clear], fx['out'][2][clear])
    print('output rel_err', errs, 'pixels left out of the fused comparison', left_out, 'recorded', fx['tie_share'])
    assert left_out <= 0.02 and abs(left_out - fx['tie_share']) < 1e-6
    for k, e in errs.items():
        assert e < tol, (k, e)


def test_pfan_matting_fp32_matches_reference(deterministic):
    fx, model, data = _build()
    assert model.head_route == 'fused'
    outs = model(data[0])
    assert all(o.dtype == torch.float32 and o.shape == r.shape for o, r in zip(outs, fx['out']))
    _check_outputs(outs, fx, 1e-3)
    recorded = tuple(o.cuda() for o in fx['out'])
    for name, value in _losses(NAMES, recorded, data).items():
        print(name, float(value), fx['losses'][name])
        assert abs(float(value) - fx['losses'][name]) < 1e-3, (name, float(value), fx['losses'][name])
    sum(_losses(M.ARGMAX_FREE, outs, data).values()).backward()
    params = dict(model.named_parameters())
    assert set(fx['grad_norm']) == {k for k, p in params.items() if p.grad is not None}
    exact_zero = {k for k, n in fx['grad_norm'].items() if fx['grad_norm64'][k] < 1e-3 * n}
    print('exactly-zero gradients', sorted(exact_zero))
    assert exact_zero == {f'{d}_{lvl}_level_conv.layer.1.bias' for d in ('global', 'local') for lvl in ('high', 'low')}
    for k, n in fx['grad_norm'].items():
        g = params[k].grad.float().cpu()
        assert abs(float(g.norm()) - n) <= 2e-2 * max(n, 1e-6), (k, float(g.norm()), n)
        if k in exact_zero:
            scale = float(params[k[:-len('bias')] + 'weight'].grad.abs().max())
            assert float(g.abs().max()) <= 4e-2 * scale, (k, float(g.abs().max()), scale)
            continue
        ref = fx['grad_sample'][k]
        assert float((g.flatten()[_sample_idx(g.numel())] - ref).abs().max()) <= 4e-2 * max(float(g.abs().max()), 1e-12), k
    sd = model.state_dict()
    zero_stat = {k for k, v in fx['bn_buffers'].items() if fx['bn_absmax64'][k] < 1e-3 * float(v.abs().max())}
    print('exactly-zero statistics', sorted(zero_stat))
    assert zero_stat == {f'{d}_{m}.layer.1.running_mean' for d in ('global', 'local') for m in ('reduce_conv1', 'upsample_conv1')}
    for k, v in fx['bn_buffers'].items():
        if k in zero_stat:
            std = fx['bn_buffers'][k.replace('running_mean', 'running_var')].sqrt()
            assert float(sd[k].float().cpu().abs().max()) <= 1e-3 * float(std.max()), k
            continue
        assert rel_err(sd[k].float().cpu(), v) < 1e-3, k


def test_pfan_matting_generic_head_route_gives_the_same_probabilities():
    fx, model, data = _build()
    model.head_route = 'generic'
    outs = model(data[0])
    assert all(o.dtype == torch.float32 for o in outs) and outs[1].is_contiguous()
    _check_outputs(outs, fx, 1e-3)


def test_pfan_matting_bf16_autocast_stays_close():
    fx, model, data = _build()
    with torch.autocast('cuda', dtype=torch.bfloat16):
        outs = model(data[0])
        loss = sum(_losses(NAMES, outs, data).values())
    assert all(o.dtype == torch.float32 for o in outs)      # the reference's .float(): probabilities are fp32 under autocast too
    errs = [rel_err(o.cpu(), r) for o, r in zip(outs[:2], fx['out'][:2])]
    print('bf16 output rel_err', errs, 'reference bf16 deviation', fx['bf16_dev'])
    assert max(errs) < max(2 * fx['bf16_dev'], 1e-2)
    loss.backward()
    assert all(p.grad is not None for p in model.parameters())          # every parameter takes part in the seven-loss sum
    assert bool(torch.isfinite(loss)) and all(torch.isfinite(p.grad).all() for p in model.parameters())


# ------------------------------------------------------------------------------------------------ loops
HEIGHT, WIDTH, BATCH = 64, 96, 4
LINE = (r'train: epoch 0001, iter \[(\d{5}), %05d\], lr: \d\.\d{6}, loss: (\d+\.\d{4}), '
        + ''.join(name + r': (\d+\.\d{4}), ' for name in NAMES) + '$')


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


def _setup(num_samples, poison=(), use_amp=True, lr=2e-3, **overrides):
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.human_matting import models
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.human_matting.common import HumanMattingCollater
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.human_matting.datasets.syntheticdataset import SyntheticHumanMattingDataset
    from simpleaicv_pytorch_training_examples_amd.tools import utils

    class config:
        pass
    config.network = 'resnet18_pfan_matting'
    config.loss_ratio = {name: 1.0 for name in NAMES}
    config.train_criterion = _criterion()
    config.test_criterion = config.train_criterion['GlobalTrimapCELoss']
    config.optimizer = ('AdamW', {'lr': lr, 'global_weight_decay': False, 'weight_decay': 1e-3, 'no_weight_decay_layer_name_list': []})
    config.scheduler = ('MultiStepLR', {'warm_up_epochs': 0, 'gamma': 0.1, 'milestones': [100]})
    config.epochs, config.batch_size, config.accumulation_steps, config.print_interval = 1, BATCH, 1, 1
    config.use_amp, config.use_ema_model, config.local_rank, config.gpus_num, config.group = use_amp, False, 0, 1, None
    config.sync_bn, config.host_sync_lag = False, 2
    config.thresh, config.squared_beta, config.save_model_metric = [0.2, 0.5], 0.3, 'miou_average'
    config.val_dataset_name_list = [['P3M-500-NP', 'P3M-500-P/val'], ['AIM']]
    for k, v in overrides.items():
        setattr(config, k, v)
    dataset = _Poisoned(SyntheticHumanMattingDataset(num_samples, HEIGHT, WIDTH, seed=0), poison)
    loader = torch.utils.data.DataLoader(dataset, batch_size=BATCH, shuffle=False, drop_last=True,
                                         collate_fn=HumanMattingCollater(resize=WIDTH))
    torch.manual_seed(0)
    model = models.resnet18_pfan_matting().cuda()
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


def _train(steps, name, **kw):
    from simpleaicv_pytorch_training_examples_amd.tools import human_matting_scripts as scripts
    config, model, optimizer, scheduler, loader = _setup(steps * BATCH, **kw)
    logger = logging.getLogger(name)
    logger.setLevel(logging.INFO)
    got, restore = _spy_average_meter()
    try:
        avg = scripts.train_human_matting(loader, model, config.train_criterion, optimizer, scheduler, 1, logger, config)
    finally:
        restore()
    torch.cuda.synchronize()
    return got, avg, model, config


def test_train_human_matting_learns_and_logs(caplog):
    steps = 16
    with caplog.at_level(logging.INFO, logger='saicv_mat'):
        got, avg, model, _ = _train(steps, 'saicv_mat')
    print('losses', got)
    assert len(got) == steps and all(np.isfinite(v) for v in got) and np.isfinite(avg)
    assert sum(got[-4:]) / 4 < sum(got[:4]) / 4, got
    assert 'skip this batch!' not in caplog.text
    lines = re.findall(LINE % steps, caplog.text, flags=re.M)
    assert [int(line[0]) for line in lines] == list(range(1, steps + 1)), caplog.text
    assert all(abs(float(line[1]) - sum(float(v) for v in line[2:])) <= 4.1e-4 for line in lines)      # seven terms at ratio 1.0
    for p in model.parameters():
        assert torch.isfinite(p).all()


def test_poisoned_batch_is_skipped_and_leaves_parameters_untouched(caplog):
    from simpleaicv_pytorch_training_examples_amd.tools import human_matting_scripts as scripts
    config, model, optimizer, scheduler, loader = _setup(BATCH, poison=(2,))
    before = model.arena.flat_param.clone()
    logger = logging.getLogger('saicv_mat_skip')
    logger.setLevel(logging.INFO)
    with caplog.at_level(logging.INFO, logger='saicv_mat_skip'):
        scripts.train_human_matting(loader, model, config.train_criterion, optimizer, scheduler, 1, logger, config)
    assert caplog.text.count('skip this batch!') == 1
    assert torch.equal(before, model.arena.flat_param)


def test_deterministic_runs_and_the_captured_step_are_bit_equal(deterministic):
    """Deterministic mode: two eager runs give the same losses and weights bit for bit, and so does the run whose iteration -- all
    seven losses included -- is captured whole (config.use_step_graph: one eager warm-up iteration, the capture, two replays)."""
    steps = 3
    eager, _, m1, _ = _train(steps, 'saicv_mat_det')
    again, _, m2, _ = _train(steps, 'saicv_mat_det')
    p_eager, p_again = m1.arena.flat_param.clone(), m2.arena.flat_param.clone()
    assert len(eager) == steps and eager == again and torch.equal(p_eager, p_again)
    graph, _, m3, config = _train(steps, 'saicv_mat_graph', use_step_graph=True, step_graph_warmup=1)
    graphs = getattr(config, '_saicv_step_graphs', {})
    assert len(graphs) == 1 and next(iter(graphs.values())).graph is not None and next(iter(graphs.values())).replays == steps - 1
    print('losses eager', eager, 'graph', graph)
    assert eager == graph
    assert torch.equal(p_eager, m3.arena.flat_param), float((p_eager - m3.arena.flat_param).norm() / p_eager.norm())


def test_validation_returns_the_reference_keys_and_the_checkpoint_metric():
    from simpleaicv_pytorch_training_examples_amd.tools import human_matting_scripts as scripts
    config, model, _, _, loader = _setup(2 * BATCH)
    result = scripts.validate_human_matting_for_all_dataset([loader, loader], model, config.test_criterion, config)
    assert list(result) == ['P3M-500-NP[+]P3M-500-P[s]val', 'AIM']
    for per_dataset in result.values():
        assert list(per_dataset) == ['per_image_load_time', 'per_image_inference_time', 'f_squared_beta_average', 'f_squared_beta_max',
                                     'mean_precision', 'mean_recall', 'max_precision', 'max_recall', 'miou_average', 'miou_max', 'sad',
                                     'mae', 'mse', 'grad', 'conn']
        assert per_dataset['per_image_load_time'].endswith('ms') and per_dataset['per_image_inference_time'].endswith('ms')
        metrics = list(per_dataset)[2:]
        assert len(metrics) == 13 and all(np.isfinite(per_dataset[key]) for key in metrics)
        assert all(0. <= per_dataset[key] <= 1. for key in metrics[:8]) and all(per_dataset[key] >= 0. for key in metrics[8:])
        assert per_dataset['miou_max'] >= per_dataset['miou_average']
    total, metric, test_loss = scripts.first_dataset_metric(result, config.save_model_metric, 0, 0)
    assert total is result['P3M-500-NP[+]P3M-500-P[s]val'] and metric == total['miou_average'] and test_loss == 0
