"""The universal-segmentation family end to end on the GPU: the tiny dinov3_vit_small_patch16_universal_segmentation against one
recorded step of the reference (tests/golden/univseg_tiny.pt: outputs, the three losses and every parameter gradient, with the
reference's own fp32-against-float64 deviations printed beside the measured ones), gradient checkpointing, bf16 autocast, a
second image size, the training loop with accumulation 1 and 2 and its repeat in a second process, the evaluation function and
both entry scripts.  The token counts here (16 + 5 = 21, 64 + 5 = 69) are no multiples of the attention kernel's tile."""
import hashlib
import logging
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import univseg_common as U
from conftest import ROOT, load_golden, rel_err

pytestmark = pytest.mark.gpu

CONFIG_DIR = os.path.join(ROOT, '16.universal_segmentation_training', '16.0.semantic_segmentation_training', 'ade20k',
                          'dinov3_vit_large_patch16_universal_segmentation')
TINY_ENV = dict(SAICV_UNIVSEG_MODEL='dinov3_vit_small_patch16_universal_segmentation', SAICV_UNIVSEG_SIZE='64',
                SAICV_UNIVSEG_QUERIES='5', SAICV_UNIVSEG_TRAIN='4', SAICV_UNIVSEG_TEST='4', SAICV_UNIVSEG_BATCH='2',
                SAICV_UNIVSEG_WORKERS='0', SAICV_UNIVSEG_EPOCHS='2', SAICV_UNIVSEG_PRINT='1')       # (one warm-up epoch, then one of the cosine)


def _pkg():
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.universal_segmentation import models
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.universal_segmentation.segmentation_losses import \
        UniversalSegmentationLoss
    return models, UniversalSegmentationLoss


@pytest.fixture(scope='module')
def fx():
    return load_golden('univseg_tiny')


def _step(rec, autocast=False, **extra):
    """the recorded step on this package: -> model, mask_preds, class_preds, losses, criterion"""
    models, Loss = _pkg()
    torch.manual_seed(0)
    model = models.__dict__[rec['name']](**dict(rec['config'], **extra)).cuda().train()
    crit = Loss(num_classes=rec['config']['num_classes'], **U.LOSS_WEIGHTS).cuda()
    crit.route = 'fused'
    images, masks, labels = U.model_batch()
    torch.manual_seed(1)
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
        mask_preds, class_preds = model(images.cuda())
        losses = crit(mask_preds, class_preds, masks, labels)
    sum(losses.values()).backward()
    return model, mask_preds, class_preds, losses, crit


def test_tiny_model_fp32_matches_the_recorded_reference_step(fx, deterministic):
    rec = fx['model']
    model, mask_preds, class_preds, losses, crit = _step(rec)
    assert mask_preds.dtype == torch.float32 and tuple(mask_preds.shape) == tuple(rec['mask_preds'].shape)
    for name, got in (('mask_preds', mask_preds), ('class_preds', class_preds)):
        e = rel_err(got, rec[name])
        print(f'{name}: deviation {e:.3e} (the reference fp32 against float64: {rec["out_dev64"][name]:.3e})')
        assert e <= 1e-3
    for (qg, tg), (qr, tr) in zip(crit.last_indices, rec['indices']):
        assert np.array_equal(qg, qr.numpy()) and np.array_equal(tg, tr.numpy())
    for k, want in rec['losses'].items():
        got = float(losses[k].detach())
        e = abs(got - want) / abs(want)
        print(f'{k}: {got:.7f} reference {want:.7f} relative {e:.3e} '
              f'(reference float64 {rec["losses64"][k]:.7f})')
        assert e <= 1e-3
    params = dict(model.named_parameters())
    assert sorted(rec['grad_norm']) == sorted(k for k, p in params.items() if p.grad is not None)
    worst = []
    for k, want in rec['grad_sample'].items():
        g = params[k].grad.detach().float().cpu()
        scale = rec['grad_absmax'][k]
        if scale == 0.:
            assert float(g.abs().max()) == 0., k
            continue
        e = float((g.flatten()[U.sample_idx(g.numel())] - want).abs().max()) / scale
        en = abs(float(g.norm()) - rec['grad_norm'][k]) / rec['grad_norm'][k]
        worst.append((max(e, en), k, rec['grad_dev64'].get(k)))
    worst.sort(reverse=True)
    for e, k, dev in worst[:8]:
        print(f'gradient {k}: deviation {e:.3e} (the reference fp32 against float64: {dev:.3e})')
    assert worst[0][0] <= 1e-3, worst[:3]


def test_gradient_checkpoint_gives_the_same_gradients(fx, deterministic):
    rec = fx['model']
    plain = _step(rec)
    ckpt = _step(rec, use_gradient_checkpoint=True)
    assert torch.equal(plain[1], ckpt[1]) and torch.equal(plain[2], ckpt[2])
    same = 0
    for (k, p), (_, q) in zip(plain[0].named_parameters(), ckpt[0].named_parameters()):
        assert q.grad is not None, k
        same += int(torch.equal(p.grad, q.grad))
        # recomputed activations are the same numbers; a gradient may differ by the order of its accumulation only
        assert float((p.grad - q.grad).abs().max()) <= 1e-6 * float(p.grad.abs().max()), k
    print('bit-equal gradients:', same, 'of', len(list(plain[0].parameters())))


def test_bf16_autocast_runs(fx):
    rec = fx['model']
    model, mask_preds, class_preds, losses, _ = _step(rec, autocast=True)
    assert mask_preds.dtype == torch.bfloat16
    for k, v in losses.items():
        assert bool(torch.isfinite(v)), k
        assert abs(float(v) - rec['losses'][k]) <= 0.05 * abs(rec['losses'][k]), (k, float(v))
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)


def test_image_size_128_has_69_tokens():
    models, Loss = _pkg()
    torch.manual_seed(0)
    model = models.dinov3_vit_small_patch16_universal_segmentation(image_size=128, query_num=5, num_classes=7,
                                                                   query_block_nums=2).cuda().eval()
    x = torch.randn(2, 3, 128, 128, device='cuda')
    with torch.no_grad():
        both = model(x)
        single = model(x[1:])
        with torch.autocast('cuda', dtype=torch.bfloat16):
            low = model(x)
    assert tuple(both[0].shape) == (2, 5, 128, 128) and tuple(both[1].shape) == (2, 5, 7)
    assert bool(torch.isfinite(both[0]).all())
    # an image's outputs do not depend on its neighbours in the batch; bf16 stays near fp32
    assert rel_err(both[0][1:], single[0]) <= 1e-5 and rel_err(both[1][1:], single[1]) <= 1e-5
    assert rel_err(low[0].float(), both[0]) <= 5e-2


class _Cfg:
    pass


def _loop_config(acc_steps):
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.universal_segmentation.datasets.syntheticdataset import \
        SyntheticUniversalSegmentationDataset
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.universal_segmentation.semantic_segmentation_common import (
        Normalize, SemanticSegmentationTestCollater, SemanticSegmentationTrainCollater)
    models, Loss = _pkg()
    config = _Cfg()
    config.network = 'dinov3_vit_small_patch16_universal_segmentation'
    config.input_image_size = 64
    config.num_classes = 7
    config.model = models.__dict__[config.network](image_size=64, query_num=5, num_classes=7, query_block_nums=2)
    config.train_criterion = Loss(num_classes=7, **U.LOSS_WEIGHTS)
    config.train_dataset = SyntheticUniversalSegmentationDataset(4 * acc_steps, 64, num_classes=7, max_objects=3, seed=0,
                                                                 transform=Normalize())
    config.test_dataset = SyntheticUniversalSegmentationDataset(4, 64, num_classes=7, max_objects=3, seed=1, transform=Normalize())
    config.train_collater = SemanticSegmentationTrainCollater(resize=64)
    config.test_collater = SemanticSegmentationTestCollater(resize=64)
    config.batch_size = 2
    config.accumulation_steps = acc_steps
    config.optimizer = ('Muon', {'lr': 4e-4, 'weight_decay': 1e-3, 'exclude_muon_layer_name_list': []})
    config.scheduler = ('CosineLR', {'warm_up_epochs': 0, 'min_lr': 1e-6})
    config.epochs = 2
    config.print_interval = 1
    config.use_amp = True
    config.use_ema_model = False
    config.local_rank = 0
    config.group = None
    config.gpus_num = 1
    config.sync_bn = False
    return config


def _run_loop(acc_steps, logger=None):
    """two epochs of train_universal_segmentation under set_seed(0) -> (losses per epoch, sha256 of the parameters, moved, config, model)"""
    from simpleaicv_pytorch_training_examples_amd.tools import universal_segmentation_scripts as uss, utils
    utils.set_seed(0)
    config = _loop_config(acc_steps)
    model = config.model.cuda()
    crit = config.train_criterion.cuda()
    optimizer, _ = utils.build_optimizer(config, model)
    scheduler = utils.Scheduler(config, optimizer)
    model, config.ema_model, config.scaler = utils.build_training_mode(config, model)
    before = {k: p.detach().clone() for k, p in model.module.named_parameters()}
    loader = torch.utils.data.DataLoader(config.train_dataset, batch_size=2, shuffle=False, drop_last=True,
                                         collate_fn=config.train_collater)
    logger = logger or logging.getLogger('saicv_univseg_child')
    losses = [float(uss.train_universal_segmentation(loader, model, crit, optimizer, scheduler, epoch, logger, config))
              for epoch in (1, 2)]
    torch.cuda.synchronize()
    digest = hashlib.sha256()
    moved = {}
    for k, p in model.module.named_parameters():
        digest.update(p.detach().float().cpu().numpy().tobytes())
        moved[k] = not torch.equal(p, before[k])
    return losses, digest.hexdigest(), moved, config, model


@pytest.fixture
def seeded_state(deterministic):
    """tools.utils.set_seed() switches the engine and torch to their deterministic kernels for the process: put both back"""
    prev = torch.backends.cudnn.deterministic
    yield
    torch.backends.cudnn.deterministic = prev


@pytest.mark.parametrize('acc_steps', [1, 2])
def test_train_loop_runs_moves_the_parameters_and_repeats(caplog, seeded_state, acc_steps):
    logger = logging.getLogger('saicv_test_univseg')
    logger.setLevel(logging.INFO)
    with caplog.at_level(logging.INFO, logger='saicv_test_univseg'):
        losses, digest, moved, config, model = _run_loop(acc_steps, logger)
    assert all(v > 0 and np.isfinite(v) for v in losses), losses
    assert 'train: epoch 0002, iter [00002, 00002]' in caplog.text and 'total_loss:' in caplog.text and 'dice_loss:' in caplog.text
    assert 'skip this batch!' not in caplog.text
    for k, p in model.module.named_parameters():
        assert bool(torch.isfinite(p).all()), k
    still = [k for k, m in moved.items() if not m]
    assert not still, still[:8]
    # the same seed in a fresh process: bit for bit
    code = (f"import sys; sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); import test_gpu_univseg as t; "
            f"print('DIGEST', t._run_loop({acc_steps})[1])")
    r = subprocess.run(['timeout', '-k', '10', '240', sys.executable, '-c', code], env=dict(os.environ, PYTHONPATH=str(ROOT)),
                       capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert f'DIGEST {digest}' in r.stdout, (digest, r.stdout[-500:])


def test_evaluation_returns_the_reference_metric_keys():
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.universal_segmentation.segmentation_decode import \
        UniversalSegmentationDecoder
    from simpleaicv_pytorch_training_examples_amd.tools import universal_segmentation_scripts as uss
    torch.manual_seed(0)
    config = _loop_config(1)
    model = config.model.cuda()
    loader = torch.utils.data.DataLoader(config.test_dataset, batch_size=2, shuffle=False, collate_fn=config.test_collater)
    decoder = UniversalSegmentationDecoder(topk=100, min_score_threshold=0.1, mask_threshold=0.5, binary_mask=True)
    out = uss.test_semantic_segmentation_dataset(loader, model, decoder, config)
    assert list(out) == ['per_image_load_time', 'per_image_inference_time', 'exist_num_class', 'mean_precision', 'mean_recall',
                         'mean_iou', 'mean_dice']
    assert out['exist_num_class'] >= 2 and 0. <= float(out['mean_iou']) <= 100.


def _torchrun(module, work, port):
    env = dict(os.environ, PYTHONPATH=str(ROOT), MASTER_ADDR='127.0.0.1', **TINY_ENV)
    cmd = ['timeout', '-k', '10', '300', sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=1',
           '--master-addr', '127.0.0.1', '--master-port', str(port), '-m',
           'simpleaicv_pytorch_training_examples_amd.tools.' + module, '--work-dir', str(work)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=360, cwd=str(ROOT))
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    return out


def test_train_entry_script_runs_from_its_work_dir(tmp_path):
    """tools/train_universal_segmentation_model.py on the benchmark config shortened by SAICV_UNIVSEG_*: the small ViT at 64 x 64 with
    5 queries (21 tokens), 4 images, batch 2, two epochs; a fresh child process"""
    work = tmp_path / 'work'
    shutil.copytree(CONFIG_DIR, work)
    out = _torchrun('train_universal_segmentation_model', work, 29561)
    assert 'train: epoch 002' in out and 'train done. model: dinov3_vit_small_patch16_universal_segmentation' in out
    assert 'total_loss:' in out and 'class_loss:' in out
    ck = torch.load(work / 'checkpoints' / 'latest.pth', map_location='cpu', weights_only=True)
    assert ck['epoch'] == 2 and 'module.upscale_blocks.1.conv2.weight' in ck['model_state_dict']


def test_test_entry_script_runs_from_its_work_dir(tmp_path):
    """tools/test_universal_segmentation_model_for_semantic_segmentation_dataset.py on the same shortened configs (4 images, batch 2)"""
    work = tmp_path / 'work'
    shutil.copytree(CONFIG_DIR, work)
    out = _torchrun('test_universal_segmentation_model_for_semantic_segmentation_dataset', work, 29562)
    assert 'eval result:' in out and 'mean_iou:' in out and 'exist_num_class:' in out
