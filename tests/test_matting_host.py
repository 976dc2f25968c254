"""Host-side checks of the human-matting family (no GPU): the float64 judges of tests/matting_common.py -- against the values the
REFERENCE losses produced, against autograd of the reference formulas, the pyramid adjoint by a dot-product test -- the Gaussian
table, the trimap class mapping, the argmax tie rule, EvalMeter against the reference's, the model factories and state_dict
surface, the CPU route of the losses, the collater, the synthetic dataset and the benchmark configs
(tests/golden/pfan_mat_r18_tiny.pt is written by scripts/record_pfan_matting_golden.py)."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import matting_common as M
from conftest import GOLDEN, ROOT


@pytest.fixture(scope='module')
def fx():
    return torch.load(os.path.join(GOLDEN, 'pfan_mat_r18_tiny.pt'), weights_only=True)


def _cpu_losses(outs, x, alpha, trimap, fg, bg):
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.human_matting import losses
    from simpleaicv_pytorch_training_examples_amd.tools.human_matting_scripts import matting_losses
    crit = {name: losses.__dict__[name]() for name in M.LOSS_NAMES}
    return matting_losses(crit, {name: 1.0 for name in M.LOSS_NAMES}, outs, x, alpha, trimap, fg, bg)


def test_judges_reproduce_the_reference_losses_of_the_model_step(fx):
    """pins the judges to the reference, not to the code under test; bound: the project's loss bound (tests/test_gpu_kernels.py)"""
    x, alpha, trimap, fg, bg = M.model_inputs(fx['input_shape'])
    got = M.seven_losses(*fx['out'], x, alpha, trimap, fg, bg)
    assert set(fx['losses']) == set(M.LOSS_NAMES)
    for name in M.LOSS_NAMES:
        print(name, float(got[name]), fx['losses'][name])
        assert abs(float(got[name]) - fx['losses'][name]) <= 1e-5 * max(1., abs(fx['losses'][name])), name


@pytest.mark.parametrize('case', M.PIXEL_CASES)
def test_judges_and_cpu_losses_reproduce_the_reference_loss_cases(fx, case):
    d = M.pixel_inputs(*case)
    fused, _ = M.fuse_judge(d['global_pred'], d['local_pred'])
    ref = fx['loss_cases'][case]
    assert ('LocalLaplacianLoss' in ref) == (min(case[1:]) >= 32)
    judged = M.seven_losses(d['global_pred'], d['local_pred'], fused, d['image'], d['alpha'], d['trimap'], d['fg'], d['bg']) \
        if min(case[1:]) >= 32 else None
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.human_matting import losses
    from simpleaicv_pytorch_training_examples_amd.tools.human_matting_scripts import matting_losses
    crit = {name: losses.__dict__[name]() for name in ref}
    cpu = matting_losses(crit, {name: 1.0 for name in ref}, (d['global_pred'], d['local_pred'], fused), d['image'], d['alpha'],
                         d['trimap'], d['fg'], d['bg'])
    for name, value in ref.items():
        assert abs(float(cpu[name]) - value) <= 1e-6 * max(1., abs(value)), (name, float(cpu[name]), value)      # the same torch ops
        if judged is not None:
            assert abs(float(judged[name]) - value) <= 1e-5 * max(1., abs(value)), (name, float(judged[name]), value)


def test_pixel_judge_gradients_equal_autograd_of_the_reference_formulas():
    d = M.pixel_inputs(2, 7, 9)
    lo, hi = np.float32(M.LO), np.float32(M.HI)
    planted = torch.tensor([lo, hi, np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(1)), 0., 1.])
    d['global_pred'].view(2, 3, -1)[:, 1, :6] = planted
    d['local_pred'].view(2, -1)[:, :6] = planted
    B = 2
    g2 = torch.tensor([[0.7, -0.3], [-0.2, 0.5]], dtype=torch.float64)
    # trimap losses
    j = M.trimap_stats_judge(d['global_pred'], d['trimap'], M.SMOOTH, g2)
    ga = d['global_pred'].double().requires_grad_(True)
    ph = torch.clamp(ga, min=M.LO, max=M.HI).permute(0, 2, 3, 1)
    oh = torch.nn.functional.one_hot(M.trimap_class(d['trimap']), 3).double()
    bce = -(oh * torch.log(ph) + (1. - oh) * torch.log(1. - ph))
    inter = ph * oh
    iou = 1. - (inter.sum(3) + M.SMOOTH) / (ph.sum(3) + oh.sum(3) - inter.sum(3) + M.SMOOTH)
    stats = torch.stack([bce.reshape(B, -1).sum(1), iou.reshape(B, -1).sum(1)], dim=1)
    (stats * g2).sum().backward()
    assert float((stats.detach() - j['stats']).abs().max()) <= 1e-12 * float(j['stats'].abs().max())
    assert float((ga.grad - j['dgp']).abs().max()) <= 1e-12 * float(j['dgp'].abs().max())
    inside = j['inside'].view(B, 3, -1)[:, 1]
    assert inside[:, :2].all() and not inside[:, 2:6].any()                              # the bounds themselves are inside
    assert float(ga.grad[~j['inside']].abs().max()) == 0.0 and float(j['dgp'][~j['inside']].abs().max()) == 0.0
    assert bool((j['dgp_mag'] >= j['dgp'].abs() * (1 - 1e-12)).all())
    # alpha losses, masked and plain
    for trimap in (d['trimap'], None):
        ja = M.alpha_judge(d['local_pred'], d['alpha'], trimap, g2)
        pa = d['local_pred'].double().requires_grad_(True)
        w = torch.ones(B, 7, 9, dtype=torch.float64) if trimap is None else (trimap == 128).double()
        diff = (torch.clamp(pa, min=M.LO, max=M.HI)[:, 0] - d['alpha'].double()) * w
        sums = torch.stack([torch.sqrt(diff ** 2 + M.EPS).reshape(B, -1).sum(1), w.reshape(B, -1).sum(1)], dim=1)
        (sums * g2).sum().backward()
        assert float((sums.detach() - ja['sums']).abs().max()) <= 1e-12 * float(ja['sums'].abs().max())
        assert float((pa.grad.view(B, -1) - ja['dp']).abs().max()) <= 1e-12 * float(ja['dp'].abs().max())
    # composition loss
    g1 = torch.tensor([0.7, -0.3], dtype=torch.float64)
    jc = M.composition_judge(d['local_pred'], d['fg'], d['bg'], d['image'], g1)
    pa = d['local_pred'].double().requires_grad_(True)
    p3 = torch.clamp(pa, min=M.LO, max=M.HI).expand(-1, 3, -1, -1)
    comp = torch.sqrt((p3 * d['fg'].double() + (1. - p3) * d['bg'].double() - d['image'].double()) ** 2 + M.EPS).reshape(B, -1).sum(1)
    (comp * g1).sum().backward()
    assert float((comp.detach() - jc['sums']).abs().max()) <= 1e-12 * float(jc['sums'].abs().max())
    assert float((pa.grad - jc['dp']).abs().max()) <= 1e-12 * float(jc['dp'].abs().max())


@pytest.mark.parametrize('masked', [False, True])
def test_pyramid_judge_equals_the_reference_formula_and_its_autograd(masked):
    """ONE pyramid of (clamp(pred) - alpha) w against the reference's two pyramids, both in float64: the pyramid is linear"""
    pred, alpha, trimap = M.lap_float_inputs(1, 37, 45, masked)
    pred.view(-1)[:4] = torch.tensor([0., 1., M.LO, M.HI])
    loss, grad, _ = M.lap_loss_judge(pred, alpha, trimap)
    leaf = pred.double().requires_grad_(True)
    ref = M.lap_loss_reference_form(leaf, alpha.double(), None if trimap is None else trimap.double())
    ref.backward()
    assert abs(float(loss) - float(ref.detach())) <= 1e-13 * float(loss)
    assert float((grad - leaf.grad).abs().max()) <= 1e-12 * float(grad.abs().max())
    assert float(grad.view(-1)[0]) == 0.0 and float(grad.view(-1)[1]) == 0.0
    if masked:
        assert float(grad[:, 0][trimap != 128].abs().max()) == 0.0


@pytest.mark.parametrize('hw', [(32, 32), (37, 45), (33, 70), (2, 3), (1, 1)])
def test_pyramid_adjoint_passes_the_dot_product_test(hw):
    """<A x, y> = <x, A^T y> in float64 for the two linear pieces (replicate-padded filter, pooling) and for their chain"""
    h, w = hw
    g = torch.Generator().manual_seed(h * 100 + w)
    K = M.gauss_table().double()
    x = torch.randn(2, 1, h, w, dtype=torch.float64, generator=g)
    y = torch.randn(2, 1, h, w, dtype=torch.float64, generator=g)
    a, b = float((M.conv_gauss(x, K) * y).sum()), float((x * M.conv_gauss_T(y, K)).sum())
    assert abs(a - b) <= 1e-12 * max(1., abs(a))
    if h >= 2 and w >= 2:
        z = torch.randn(2, 1, h // 2, w // 2, dtype=torch.float64, generator=g)
        a, b = float((torch.nn.functional.avg_pool2d(x, 2) * z).sum()), float((x * M.pool_T(z, h, w)).sum())
        assert abs(a - b) <= 1e-12 * max(1., abs(a))
        a = float((torch.nn.functional.avg_pool2d(M.conv_gauss(x, K), 2) * z).sum())
        b = float((x * M.conv_gauss_T(M.pool_T(z, h, w), K)).sum())
        assert abs(a - b) <= 1e-12 * max(1., abs(a))


def test_gaussian_table_is_the_recorded_one_and_not_the_product_gaussian(fx):
    from simpleaicv_pytorch_training_examples_amd import ops
    table = torch.tensor(ops.laplacian_gauss_table(), dtype=torch.float32)
    assert torch.equal(table, fx['gauss']) and torch.equal(M.gauss_table().reshape(25), fx['gauss'])
    assert abs(float(table[0]) - 0.0109) < 5e-5 and abs(float(table[12]) - 0.0805) < 5e-5
    assert abs(float(table[0]) - M.product_gauss_corner()) > 5e-3              # the product Gaussian's corner is 0.00297
    assert abs(float(table.double().sum()) - 1.) < 1e-6 and torch.equal(table.view(5, 5), table.view(5, 5).t())


def test_trimap_class_mapping_on_planted_values():
    t = torch.tensor(M.TRIMAP_PLANTED)
    assert M.trimap_class(t).tolist() == M.TRIMAP_PLANTED_CLASS
    # the reference's own lines (losses.py:36-44), run here as they are written
    c = t.clone()
    c[c == 0] = 0
    c[c == 255] = 2
    c[c > 2] = 1
    assert c.long().tolist() == M.TRIMAP_PLANTED_CLASS


def test_argmax_ties_pick_the_first_maximum():
    gp = torch.tensor([[.5, .5, .5], [.2, .7, .7], [.7, .2, .7], [1., 1., 1.], [.1, .8, .3], [.1, .3, .8], [0., 0., 1.]]).t().reshape(1, 3, 1, 7)
    local = torch.full((1, 1, 1, 7), 0.25)
    fused, idx = M.fuse_judge(gp, local)
    assert idx.view(-1).tolist() == [0, 1, 0, 0, 1, 2, 2]
    assert fused.view(-1).tolist() == [0., .25, 0., 0., .25, 1., 1.]
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.human_matting.models.pfan_matting import PFANMatting
    assert torch.equal(PFANMatting.collaborative_matting(None, gp, local), fused)          # the model's CPU route


def test_eval_meter_equals_the_reference_on_cpu_tensors(fx):
    from simpleaicv_pytorch_training_examples_amd.tools.human_matting_scripts import EvalMeter

    class cfg:
        thresh, squared_beta = M.EVAL_THRESH, M.EVAL_SQUARED_BETA
    meter = EvalMeter(cfg)
    for preds, masks in M.eval_inputs():
        meter.add_batch_result(preds, masks)
    meter.compute_all_metrics()
    assert set(fx['eval']) == set(M.EVAL_KEYS)
    for k in M.EVAL_KEYS:
        got = np.asarray(getattr(meter, k))
        assert np.array_equal(got, np.asarray(fx['eval'][k], dtype=got.dtype)), (k, got, fx['eval'][k])


def test_conn_of_two_blobs_by_hand():
    """An 8 x 8 mask with a 3 x 3 blob A and a 2 x 2 blob B, both 1.0; the prediction equals the mask except that B is 0.5.
    At every threshold 0.1 .. 1.0 the intersection holds A (9 pixels) and, up to 0.5, B (4 pixels): the largest component is A
    throughout.  Every pixel outside A is rounded down to 0 at the first threshold; A stays in the component to the end and gets
    1.  Differences to that map: A 0 / 0, background 0 / 0, B mask 1.0 -> phi 0, prediction 0.5 -> phi 0.5.  conn = 4 pixels x
    |0 - 0.5| / 1000 = 0.002.  With B at 1.0 as well both maps agree and conn = 0."""
    from simpleaicv_pytorch_training_examples_amd.tools.human_matting_scripts import EvalMeter

    class cfg:
        thresh, squared_beta = [0.2], 0.3
    mask = np.zeros((8, 8), dtype=np.float32)
    mask[0:3, 0:3] = 1.
    mask[5:7, 5:7] = 1.
    pred = mask.copy()
    pred[5:7, 5:7] = 0.5
    meter = EvalMeter(cfg)
    assert abs(float(meter.cal_conn(pred, mask)) - 0.002) < 1e-9
    assert float(meter.cal_conn(mask.copy(), mask)) == 0.0


def test_factories_state_dict_surface_and_initial_weights_equal_the_reference(fx):
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.human_matting import losses, models
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.human_matting.models import pfan_matting as pfan
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.semantic_segmentation.models import pfan_semantic_segmentation as semseg
    assert pfan.CPFE is semseg.CPFE and pfan.ConvBnActBlock is semseg.ConvBnActBlock                      # reused, not copied
    assert pfan.ConvTransposeBnActBlock is semseg.ConvTransposeBnActBlock
    assert len(pfan.__all__) == 13 and all(name.endswith('_pfan_matting') for name in pfan.__all__)
    for name in pfan.__all__:
        model = models.__dict__[name]()
        assert model.global_pred_conv.weight.shape == (3, 32, 3, 3) and model.local_pred_conv.weight.shape == (1, 32, 3, 3), name
        assert model.head_route == 'fused' and model.local_reduce_conv1.layer[0].in_channels == 128, name
        assert model.global_high_level_cpfe_3.conv_1_1.in_channels == model.backbone.out_channels[2], name
    assert models.resnet18_pfan_matting(cpfe_planes=20).head_route == 'generic'
    assert models.resnet18_pfan_matting(use_gradient_checkpoint=True).backbone.use_gradient_checkpoint is True
    assert losses.__all__ == list(M.LOSS_NAMES)
    for name in losses.__all__:
        assert isinstance(losses.__dict__[name](), torch.nn.Module)
    assert losses.GloabelTrimapIouLoss(smooth=1e-3).smooth == 1e-3
    torch.manual_seed(0)
    model = models.resnet18_pfan_matting(**fx['config'])
    sd = model.state_dict()
    assert len(sd) == 260 and len(fx['keys']) == 260
    assert [(k, tuple(v.shape)) for k, v in sorted(sd.items())] == [(k, tuple(s)) for k, s in fx['keys']]
    assert all(k.split('.')[0].startswith(('backbone', 'global_', 'local_')) for k in sd)
    assert set(fx['init_sample']) == {k for k, v in sd.items() if v.dtype.is_floating_point}
    for k, ref in fx['init_sample'].items():
        idx = torch.linspace(0, sd[k].numel() - 1, min(16, sd[k].numel())).long()
        assert torch.equal(sd[k].flatten()[idx], ref), f'initial weights differ: {k}'
    # every parameter takes part in the reference's step (the fixture holds a gradient for each of them)
    assert set(fx['grad_norm']) == {k for k, _ in model.named_parameters()}


def test_cpu_losses_equal_the_reference_values_and_differentiate(fx):
    x, alpha, trimap, fg, bg = M.model_inputs(fx['input_shape'])
    outs = tuple(o.clone().requires_grad_(True) for o in fx['out'])
    got = _cpu_losses(outs, x, alpha, trimap, fg, bg)
    assert list(got) == list(M.LOSS_NAMES)
    for name, value in got.items():
        assert abs(float(value.detach()) - fx['losses'][name]) <= 1e-6 * max(1., abs(fx['losses'][name])), name
    sum(got.values()).backward()
    assert all(o.grad is not None and bool(torch.isfinite(o.grad).all()) and float(o.grad.abs().max()) > 0 for o in outs)
    with pytest.raises(KeyError):
        from simpleaicv_pytorch_training_examples_amd.tools.human_matting_scripts import matting_losses
        matting_losses({'BCELoss': None}, {'BCELoss': 1.0}, outs, x, alpha, trimap, fg, bg)


def test_collater_and_synthetic_dataset_contract():
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.classification import common as cls_common
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.human_matting.common import HumanMattingCollater, load_state_dict
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.human_matting.datasets.syntheticdataset import SyntheticHumanMattingDataset
    from simpleaicv_pytorch_training_examples_amd.tools import path
    assert load_state_dict is cls_common.load_state_dict and path.human_matting_dataset_path.endswith('human_matting_dataset')
    ds = SyntheticHumanMattingDataset(4, 48, 64, seed=0)
    sample = ds[1]
    assert list(sample) == ['image', 'mask', 'trimap', 'fg_map', 'bg_map', 'size'] and len(ds) == 4
    for k in ('image', 'fg_map', 'bg_map'):
        assert sample[k].shape == (48, 64, 3) and sample[k].dtype == np.float32
    assert sample['mask'].shape == (48, 64) and sample['mask'].dtype == np.float32
    assert sample['mask'].min() >= 0. and sample['mask'].max() <= 1. and ((sample['mask'] > 0) & (sample['mask'] < 1)).any()
    assert sample['trimap'].dtype == np.uint8 and set(np.unique(sample['trimap']).tolist()) == {0, 128, 255}
    soft = (sample['mask'] > 0) & (sample['mask'] < 1)
    assert (sample['trimap'][soft] == 128).all() and (sample['mask'][sample['trimap'] == 255] == 1.).all()
    assert (sample['mask'][sample['trimap'] == 0] == 0.).all()
    m3 = sample['mask'][:, :, None]
    assert np.allclose(sample['image'], m3 * sample['fg_map'] + (1. - m3) * sample['bg_map'], atol=1e-6)
    assert sample['size'].tolist() == [48, 64] and sample['size'].dtype == np.float32
    assert np.array_equal(ds[1]['mask'], sample['mask']) and not np.array_equal(ds[2]['mask'], sample['mask'])
    batch = HumanMattingCollater(resize=80)([ds[0], ds[1]])
    assert list(batch) == ['image', 'mask', 'trimap', 'fg_map', 'bg_map', 'size']
    for k in ('image', 'fg_map', 'bg_map'):
        assert batch[k].shape == (2, 3, 80, 80) and batch[k].dtype == torch.float32
        assert torch.equal(batch[k][1, :, :48, :64], torch.from_numpy(sample[k]).permute(2, 0, 1))
        assert float(batch[k][:, :, 48:].abs().sum()) == 0 and float(batch[k][:, :, :, 64:].abs().sum()) == 0
    for k in ('mask', 'trimap'):
        assert batch[k].shape == (2, 80, 80) and batch[k].dtype == torch.float32
        assert torch.equal(batch[k][1, :48, :64], torch.from_numpy(sample[k].astype(np.float32)))
        assert float(batch[k][:, 48:].abs().sum()) == 0 and float(batch[k][:, :, 64:].abs().sum()) == 0
    assert isinstance(batch['size'], np.ndarray) and batch['size'].dtype == np.float32 and batch['size'].tolist() == [[48, 64], [48, 64]]


def test_benchmark_configs_import_with_the_shorteners(monkeypatch):
    for k, v in dict(SAICV_MAT_TRAIN=8, SAICV_MAT_TEST=4, SAICV_MAT_BATCH=2, SAICV_MAT_WORKERS=0, SAICV_MAT_EPOCHS=2, SAICV_MAT_PRINT=1).items():
        monkeypatch.setenv(k, str(v))
    work_dir = os.path.join(ROOT, '07.human_matting_training', 'resnet50_pfan_matting')
    monkeypatch.syspath_prepend(ROOT)
    configs = {}
    for name in ('train_config', 'test_config'):
        monkeypatch.syspath_prepend(work_dir)
        monkeypatch.delitem(sys.modules, 'train_config', raising=False)
        spec = importlib.util.spec_from_file_location(f'saicv_mat_{name}', os.path.join(work_dir, name + '.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        configs[name] = mod.config
    sys.modules.pop('train_config', None)              # (popped, not monkeypatched away: an undo would put the module back for later tests)
    c = configs['train_config']
    assert c.network == 'resnet50_pfan_matting' and c.input_image_size == [1024, 1024]
    assert list(c.train_criterion) == list(M.LOSS_NAMES) and c.loss_ratio == {name: 1.0 for name in M.LOSS_NAMES}
    assert c.optimizer[0] == 'AdamW' and c.optimizer[1]['lr'] == 1e-4 and c.scheduler[0] == 'CosineLR'
    assert c.thresh == [0.2] and c.squared_beta == 0.3 and c.save_model_metric == 'miou_average' and c.save_interval == 10
    assert (len(c.train_dataset), len(c.val_dataset_list[0]), c.batch_size, c.num_workers, c.epochs, c.print_interval) == (8, 4, 2, 0, 2, 1)
    assert len(c.val_dataset_name_list) == len(c.val_dataset_list) == 1 and c.use_amp is True
    t = configs['test_config']
    assert t.thresh == [0.2] and t.squared_beta == 0.3 and t.batch_size == 2 and len(t.val_dataset_list[0]) == 4
    monkeypatch.delenv('SAICV_MAT_BATCH')
    assert int(os.environ.get('SAICV_MAT_BATCH', 32)) == 32                      # the reference's global batch is the default
