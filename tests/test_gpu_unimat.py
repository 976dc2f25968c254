"""The universal-matting family end to end on the GPU: UniversalMattingLoss fused against the float64 judge and the composed route
on the recorded loss cases, the tiny dinov3_vit_small_patch16_universal_matting against one recorded step of the reference
(tests/golden/unimat_tiny.pt), the training loop with accumulation 1 and 2 and a skipped NaN batch, validation through the decoder
and both entry scripts.

Bounds.  Losses and loss gradients of the fused route: REF_FACTOR x what the fixture records for the reference's own fp32 run
against float64 (per loss: |loss - loss64| / loss64; per input: 'grad_dev'), the largest over the four cases.  The model step: the
1e-3 that tests/test_gpu_univseg.py applies to its model step."""
import logging
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import unimat_common as U
from conftest import ROOT, load_golden, rel_err

pytestmark = pytest.mark.gpu

CONFIG_DIR = os.path.join(ROOT, '16.universal_segmentation_training', '16.3.human_matting_training',
                          'dinov3_vit_large_patch16_universal_matting')
TINY_ENV = dict(SAICV_UNIMAT_MODEL='dinov3_vit_small_patch16_universal_matting', SAICV_UNIMAT_SIZE='64', SAICV_UNIMAT_QUERIES='5',
                SAICV_UNIMAT_TRAIN='4', SAICV_UNIMAT_TEST='4', SAICV_UNIMAT_BATCH='2', SAICV_UNIMAT_WORKERS='0', SAICV_UNIMAT_EPOCHS='2',
                SAICV_UNIMAT_PRINT='1', SAICV_UNIMAT_ACCUM='1')
GRADS = ('dglobal', 'dlocal', 'dfused', 'dclass')


def _pkg():
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.universal_segmentation import models
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.universal_segmentation.matting_losses import UniversalMattingLoss
    return models.dinov3_universal_matting, UniversalMattingLoss


@pytest.fixture(scope='module')
def fx():
    return load_golden('unimat_tiny')


@pytest.fixture(scope='module')
def bounds(fx):
    cases = fx['loss_cases'].values()
    loss = {k: U.REF_FACTOR * max(abs(r['losses'][k] - r['losses64'][k]) / abs(r['losses64'][k]) for r in cases) for k in U.LOSS_KEYS}
    grad = {k: U.REF_FACTOR * max(r['grad_dev'][k] for r in cases) for k in GRADS}
    return loss, grad


_judged = {}


def _judge(case):
    if U.case_id(case) not in _judged:
        _judged[U.case_id(case)] = (U.loss_inputs(case), U.judge_loss(*U.loss_inputs(case)))
    return _judged[U.case_id(case)]


def _run_loss(case, route, order):
    _, Loss = _pkg()
    (gp, lp, fp, cp, trimaps, alphas, labels), _ = _judge(case)
    place = (lambda x: U.channels_last(x.cuda())) if order == 'channels_last' else (lambda x: x.cuda().contiguous())
    leaves = [place(t).detach().requires_grad_(True) for t in (gp, lp, fp)] + [cp.cuda().requires_grad_(True)]
    crit = Loss(num_classes=U.LOSS_CLASSES, **U.LOSS_WEIGHTS).cuda()
    crit.route = route
    out = crit(*leaves, trimaps, alphas, labels)
    sum(out.values()).backward()
    return crit, out, leaves


@pytest.mark.parametrize('order', ['channels_last', 'contiguous'])
@pytest.mark.parametrize('case', U.LOSS_CASES, ids=U.case_id)
def test_fused_loss_against_judge_and_composed(fx, bounds, case, order):
    loss_bound, grad_bound = bounds
    rec = fx['loss_cases'][U.case_id(case)]
    _, judge = _judge(case)
    crit, out, leaves = _run_loss(case, 'fused', order)
    comp, cout, cleaves = _run_loss(case, 'composed', order)
    assert tuple(out) == U.LOSS_KEYS
    for got, other, (rq, rt) in zip(crit.last_indices, comp.last_indices, rec['indices']):
        assert np.array_equal(got[0], rq.numpy()) and np.array_equal(got[1], rt.numpy())
        assert np.array_equal(other[0], rq.numpy()) and np.array_equal(other[1], rt.numpy())
    for k in U.LOSS_KEYS:
        got, want = float(out[k].detach()), judge['losses'][k]
        e, ec = abs(got - want) / abs(want), abs(float(cout[k].detach()) - want) / abs(want)
        print(f'{U.case_id(case)} {order} {k}: fused {e:.2e} composed {ec:.2e} of the float64 value, bound {loss_bound[k]:.2e}')
        assert e <= loss_bound[k], k
        assert ec <= loss_bound[k], ('composed', k)
    matched = torch.zeros(case[0], case[1], dtype=torch.bool)
    for i, (q, _) in enumerate(crit.last_indices):
        matched[i, torch.as_tensor(q)] = True
    for leaf, cleaf, name in zip(leaves, cleaves, GRADS):
        want = judge[name]
        g = leaf.grad
        assert g.stride() == leaf.stride(), name                                       # the predictions' memory order
        e = float((g.cpu().double() - want).abs().max() / want.abs().max())
        ec = float((cleaf.grad.cpu().double() - want).abs().max() / want.abs().max())
        print(f'{U.case_id(case)} {order} {name}: fused {e:.2e} composed {ec:.2e} of the largest element, bound {grad_bound[name]:.2e}')
        assert e <= grad_bound[name], name
        # the composed route is the reference's two-pyramid Laplacian form in fp32: where a pyramid difference is zero up to its
        # rounding, the L1 gradient's sign is nobody's to decide, and the judge says how far that can move each element
        slack = {'dlocal': judge['slack_local'], 'dfused': judge['slack_fused']}.get(name)
        over = (cleaf.grad.cpu().double() - want).abs() - grad_bound[name] * want.abs().max()
        if slack is not None:
            reached = float((slack > 0).double().mean())
            print(f'{U.case_id(case)} {order} {name}: undecided pyramid entries reach {reached:.2%} of the elements')
            over = over - slack
        assert float(over.max()) <= 0., ('composed', name, float(over.max()))
        if name != 'dclass' and bool((~matched).any()):
            assert float(g.cpu()[~matched].abs().max()) == 0., name                   # exact zeros in the unmatched rows


def test_no_pair_gives_nan_map_terms():
    _, Loss = _pkg()
    gp, lp, fp, cp, trimaps, alphas, labels = U.make_inputs(2, 3, [0, 0], 32, 32, seed=4)
    crit = Loss(num_classes=U.LOSS_CLASSES).cuda()
    crit.route = 'fused'
    out = crit(U.channels_last(gp.cuda()), U.channels_last(lp.cuda()), U.channels_last(fp.cuda()), cp.cuda(), trimaps, alphas, labels)
    assert all(bool(torch.isnan(out[k])) for k in U.LOSS_KEYS[:6]) and bool(torch.isfinite(out['class_loss']))
    assert all(len(q) == 0 for q, _ in crit.last_indices)


def _step(rec, autocast=False, route='fused', **extra):
    M, Loss = _pkg()
    torch.manual_seed(U.MODEL_SEEDS['build'])
    model = M.__dict__[rec['name']](**dict(rec['config'], **extra)).cuda().train()
    crit = Loss(num_classes=rec['config']['num_classes'], **U.LOSS_WEIGHTS).cuda()
    crit.route = route
    images, trimaps, alphas, labels = U.model_batch()
    torch.manual_seed(U.MODEL_SEEDS['run'])
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
        outs = model(images.cuda())
        losses = crit(*outs, trimaps, alphas, labels)
    sum(losses.values()).backward()
    return model, outs, losses, crit


def test_tiny_model_fp32_matches_the_recorded_reference_step(fx, deterministic):
    rec = fx['model']
    model, outs, losses, crit = _step(rec)
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == [(k, tuple(s)) for k, s in rec['keys']]
    und = torch.zeros(rec['fused_preds'].shape, dtype=torch.bool)
    if rec['undecided'].numel():
        und[tuple(rec['undecided'].t())] = True
    for name, got in zip(('global_preds', 'local_preds', 'fused_preds', 'class_preds'), outs):
        assert got.dtype == torch.float32 and tuple(got.shape) == tuple(rec[name].shape), name
        got, want = got.detach().cpu(), rec[name]
        if name == 'fused_preds':
            got, want = got * ~und, want * ~und
        e = rel_err(got, want)
        print(f'{name}: deviation {e:.3e} (the reference fp32 against float64: {rec["out_dev64"][name]:.3e})')
        assert e <= 1e-3, name
    assert outs[0].stride(2) == 1 and outs[0].stride(1) == 3                          # channels-last views
    for (qg, tg), (qr, tr) in zip(crit.last_indices, rec['indices']):
        assert np.array_equal(qg, qr.numpy()) and np.array_equal(tg, tr.numpy())
    for k, want in rec['losses'].items():
        got = float(losses[k].detach())
        e = abs(got - want) / abs(want)
        print(f'{k}: {got:.7f} reference {want:.7f} relative {e:.3e} (reference float64 {rec["losses64"][k]:.7f})')
        assert e <= 1e-3, k
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


@pytest.mark.parametrize('C', [8, 12])
def test_scale_block_in_image_groups_and_on_padded_channels(C, monkeypatch):
    """The two branches of _scale_block every real configuration takes (Q = 100: 100 and 300 channels at batch 8), at a small size:
    the split into image groups (C = 8: groups of 2 + 1 images through ScaleBlock.forward; C = 12: one image per group) and zero-padded
    channels with the fp32 LayerNorm kernel on the real ones (C = 12 -> 16), against the block's own torch modules in float64,
    forward and every gradient, under the model step's 1e-3."""
    import copy
    M, _ = _pkg()
    torch.manual_seed(3)
    block = M.ScaleBlock(C).cuda()
    with torch.no_grad():
        block.norm.weight.uniform_(0.5, 1.5)
        block.norm.bias.uniform_(-0.5, 0.5)
    x = torch.randn(3, 6, 5, C, device='cuda')
    ref = copy.deepcopy(block).double()
    x64 = x.double().requires_grad_(True)
    y64 = ref.norm(ref.conv2(torch.nn.functional.gelu(ref.conv1(x64.permute(0, 3, 1, 2)))).permute(0, 2, 3, 1))
    g = torch.randn_like(y64)
    (y64 * g).sum().backward()
    monkeypatch.setattr(M, '_BLOCK_ELEMENTS', 6 * 5 * 4 * 16)
    xg = x.clone().requires_grad_(True)
    got = M._scale_block(block, xg)
    assert tuple(got.shape) == (3, 12, 10, C) and got.dtype == torch.float32
    (got * g.float()).sum().backward()
    errs = {'output': rel_err(got, y64), 'dx': rel_err(xg.grad, x64.grad)}
    for (k, p), (_, q) in zip(block.named_parameters(), ref.named_parameters()):
        errs['d' + k] = rel_err(p.grad, q.grad)
    print(f'_scale_block C={C}:', {k: f'{v:.2e}' for k, v in errs.items()})
    assert max(errs.values()) <= 1e-3, errs


def test_bf16_autocast_and_checkpointing_run(fx):
    rec = fx['model']
    model, outs, losses, _ = _step(rec, autocast=True, use_gradient_checkpoint=True)
    assert all(o.dtype == torch.float32 for o in outs[:3])
    for k, v in losses.items():
        assert bool(torch.isfinite(v)), k
        assert abs(float(v.detach()) - rec['losses'][k]) <= 0.1 * abs(rec['losses'][k]) + 0.02, (k, float(v.detach()))
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)


class _Cfg:
    pass


def _loop_config(acc_steps):
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.universal_segmentation.datasets.syntheticmattingdataset import \
        SyntheticUniversalMattingDataset
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.universal_segmentation.human_matting_common import (
        HumanMattingTestCollater, HumanMattingTrainCollater, Normalize)
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.universal_segmentation.matting_decode import UniversalMattingDecoder
    M, Loss = _pkg()
    config = _Cfg()
    config.network = 'dinov3_vit_small_patch16_universal_matting'
    config.input_image_size = [64, 64]
    config.num_classes = 2
    config.model = M.__dict__[config.network](image_size=64, query_num=5, num_classes=2, query_block_nums=2)
    config.train_criterion = Loss(num_classes=2, **U.LOSS_WEIGHTS)
    config.train_dataset = SyntheticUniversalMattingDataset(4 * acc_steps, 64, seed=0, transform=Normalize())
    config.val_dataset_name_list = [['synthetic_mattes']]
    config.val_dataset_list = [SyntheticUniversalMattingDataset(4, 64, seed=1, transform=Normalize())]
    config.train_collater = HumanMattingTrainCollater(resize=64)
    config.val_collater = HumanMattingTestCollater(resize=64)
    config.decoder = UniversalMattingDecoder(topk=1, min_score_threshold=0.1)
    config.thresh, config.squared_beta = [0.2], 0.3
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


class _NaNBatch:
    """the loader's batches with the FIRST image of the first batch made NaN"""

    def __init__(self, loader):
        self.loader, self.dataset = loader, loader.dataset

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for i, data in enumerate(self.loader):
            if i == 0:
                data['image'][0, 0, 0, 0] = float('nan')
            yield data


@pytest.fixture
def seeded_state(deterministic):
    prev = torch.backends.cudnn.deterministic
    yield
    torch.backends.cudnn.deterministic = prev


@pytest.mark.parametrize('acc_steps', [1, 2])
def test_train_loop_runs_skips_a_nan_batch_and_validates(caplog, seeded_state, acc_steps):
    from simpleaicv_pytorch_training_examples_amd.tools import universal_matting_scripts as ums, utils
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
    logger = logging.getLogger('saicv_test_unimat')
    logger.setLevel(logging.INFO)
    with caplog.at_level(logging.INFO, logger='saicv_test_unimat'):
        first = float(ums.train_universal_matting(loader, model, crit, optimizer, scheduler, 1, logger, config))
        assert 'skip this batch!' not in caplog.text
        second = float(ums.train_universal_matting(_NaNBatch(loader), model, crit, optimizer, scheduler, 2, logger, config))
    assert first > 0 and np.isfinite(first) and np.isfinite(second)
    assert 'total_loss:' in caplog.text and 'fusion_laplacian_loss:' in caplog.text and 'class_loss:' in caplog.text
    assert 'skip this batch!' in caplog.text
    moved = [k for k, p in model.module.named_parameters() if not torch.equal(p, before[k])]
    assert all(bool(torch.isfinite(p).all()) for p in model.module.parameters()) and len(moved) == len(before)
    if acc_steps == 1:
        val = [torch.utils.data.DataLoader(d, batch_size=2, shuffle=False, collate_fn=config.val_collater) for d in config.val_dataset_list]
        out = ums.validate_human_matting_for_all_dataset(val, model, config.decoder, config)
        assert list(out) == ['synthetic_mattes']
        assert list(out['synthetic_mattes']) == ['per_image_load_time', 'per_image_inference_time', 'f_squared_beta_average',
                                                 'f_squared_beta_max', 'mean_precision', 'mean_recall', 'max_precision', 'max_recall',
                                                 'miou_average', 'miou_max', 'sad', 'mae', 'mse', 'grad', 'conn']
        assert 0. <= float(out['synthetic_mattes']['mae']) <= 1.


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
    """tools/train_universal_matting_model.py on the benchmark config shortened by SAICV_UNIMAT_*: the small ViT at 64 x 64 with 5
    queries, 4 images, batch 2, two epochs; a fresh child process"""
    work = tmp_path / 'work'
    shutil.copytree(CONFIG_DIR, work)
    out = _torchrun('train_universal_matting_model', work, 29571)
    assert 'train: epoch 002' in out and 'train done. model: dinov3_vit_small_patch16_universal_matting' in out
    assert 'total_loss:' in out and 'fusion_alpha_loss:' in out
    ck = torch.load(work / 'checkpoints' / 'latest.pth', map_location='cpu', weights_only=True)
    assert ck['epoch'] == 2 and 'module.global_upscale_blocks.1.conv2.weight' in ck['model_state_dict']


def test_test_entry_script_runs_from_its_work_dir(tmp_path):
    """tools/test_universal_segmentation_model_for_human_matting_dataset.py on the same shortened configs (4 images, batch 2)"""
    work = tmp_path / 'work'
    shutil.copytree(CONFIG_DIR, work)
    out = _torchrun('test_universal_segmentation_model_for_human_matting_dataset', work, 29572)
    assert 'eval dataset:synthetic_mattes' in out and 'miou_average:' in out and 'conn:' in out
