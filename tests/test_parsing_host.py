"""Host-side checks of the human- and face-parsing families (no GPU): the float64 judge of tests/parsing_common.py against torch
autograd of the restated reference formulas and against loss values recorded from the reference's own losses
(tests/golden/pfan_parse_r18_tiny.pt, written by scripts/record_pfan_parsing_golden.py), the conditions the kernel test's inputs
must meet, the four losses on CPU tensors, the model factories and the recorded state_dict surface, the collaters, the synthetic
datasets and the validation arithmetic."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import parsing_common as P
from conftest import GOLDEN, ROOT

PKG = 'simpleaicv_pytorch_training_examples_amd.SimpleAICV'
PREFIXES = ('resnet18', 'resnet34', 'resnet50', 'resnet101', 'resnet152', 'vanb0', 'vanb1', 'vanb2', 'vanb3', 'convformers18',
            'convformers36', 'convformerm36', 'convformerb36')


def _family(family, module):
    import importlib
    return importlib.import_module(f'{PKG}.{family}_parsing.{module}')


@pytest.mark.parametrize('logit_type', P.LOGIT_TYPES)
@pytest.mark.parametrize('C', [2, 19, 20, 33, 151])
def test_judge_gradient_equals_autograd_of_the_restated_formulas(C, logit_type):
    x, label = P.class_terms_inputs(96, C, seed=C, dtype=torch.float64, logit_type=logit_type)
    g = (0.7, -1.3, 0.4)
    j = P.class_terms_judge(x, label, logit_type, g)
    xa = x.clone().requires_grad_(True)
    terms = P.class_terms_restated(xa, label, logit_type)
    (terms * torch.tensor(g, dtype=torch.float64)).sum().backward()
    assert float((terms.detach() - j['terms']).abs().max()) <= 1e-12
    assert float((xa.grad - j['grad']).abs().max()) < 1e-12 * float(xa.grad.abs().max())
    if logit_type == 'sigmoid':                                       # the element mask is the gradient's support
        assert float(xa.grad[~j['mask']].abs().max()) == 0.0 and float(j['grad'][~j['mask']].abs().max()) == 0.0


def test_judge_terms_equal_the_recorded_reference_values():
    """fp32 reference values against the float64 judge on the recorded logits: within 1e-6.  The reference clamps with float32
    constants; the judge is given the same two numbers (at the default 1 - 1e-4 the BCE of every element above the upper bound
    differs by log(1.00017): 1.7e-5 on this tensor's mean, nothing to do with the formulas being pinned)."""
    fx = torch.load(os.path.join(GOLDEN, 'pfan_parse_r18_tiny.pt'), weights_only=True)
    logits, labels = fx['loss_logits'], fx['loss_labels']
    assert tuple(logits.shape) == (1, 20, 8, 12) and logits.dtype == torch.float32
    rows = logits.permute(0, 2, 3, 1).reshape(-1, 20)
    for logit_type in P.LOGIT_TYPES:
        j = P.class_terms_judge(rows, labels.reshape(-1), logit_type, lo=float(np.float32(1e-4)), hi=float(np.float32(1. - 1e-4)))
        clamped = float((~j['mask']).double().mean())
        print(logit_type, [float(v) for v in j['terms']], fx['loss_values'][logit_type], 'clamped share', clamped)
        assert 0.1 <= clamped <= 0.9                                  # the recorded values exercise the clamp
        for got, want in zip(j['terms'], fx['loss_values'][logit_type]):
            assert abs(float(got) - want) <= 1e-6


@pytest.mark.parametrize('logit_type', P.LOGIT_TYPES)
@pytest.mark.parametrize('dtype', P.KERNEL_DTYPES)
@pytest.mark.parametrize('rows', P.KERNEL_ROWS)
@pytest.mark.parametrize('C', P.KERNEL_CLASSES)
def test_kernel_test_inputs_meet_their_conditions(C, rows, dtype, logit_type):
    """conditions on the inputs of tests/test_gpu_parsing_kernels.py, asserted here so that the GPU test cannot hide behind them"""
    x, label = P.class_terms_inputs(rows, C, P.case_seed(C, rows, logit_type), dtype, logit_type)
    assert x.dtype == dtype and x.shape == (rows, C)
    j = P.class_terms_judge(x, label, logit_type, P.KERNEL_G)
    assert int(j['near'].sum()) == 0                                  # no element within relative 1e-3 of a bound
    for regime in range(3):
        assert float((j['regime'] == regime).double().mean()) >= 0.05
    clamped = float((~j['mask']).double().mean())
    assert clamped >= 0.1 and 1. - clamped >= 0.1


@pytest.mark.parametrize('logit_type', P.LOGIT_TYPES)
def test_judge_ignores_labels_outside_the_classes_and_still_counts_them(logit_type):
    x, label = P.class_terms_inputs(12, 7, seed=3, dtype=torch.float64, logit_type=logit_type)
    ref = P.class_terms_judge(x, label, logit_type)
    label2 = label.clone()
    label2[0], label2[1] = -1., 7.
    j = P.class_terms_judge(x, label2, logit_type)
    assert not bool(j['valid'][0]) and not bool(j['valid'][1]) and float(j['grad'][:2].abs().max()) == 0.0
    assert torch.equal(j['grad'][2:], ref['grad'][2:])               # the other rows still divide by all 12 rows
    kept = P.class_terms_judge(x[2:], label[2:], logit_type)
    assert float((j['terms'] * 12 - kept['terms'] * 10).abs().max()) < 1e-12


@pytest.mark.parametrize('family,num_classes', [('human', 20), ('face', 19)])
def test_all_factories_construct(family, num_classes):
    models = _family(family, 'models')
    names = _family(family, f'models.pfan_{family}_parsing').__all__
    assert sorted(names) == sorted(f'{p}_pfan_{family}_parsing' for p in PREFIXES)
    for name in names:
        model = getattr(models, name)()
        assert type(model).__name__ == 'PFANParsing' and model.pred_conv.out_channels == num_classes, name
    assert getattr(models, f'resnet18_pfan_{family}_parsing')(num_classes=5).pred_conv.out_channels == 5


def test_r18_state_dict_surface_equals_the_reference():
    models = _family('human', 'models')
    fx = torch.load(os.path.join(GOLDEN, 'pfan_parse_r18_tiny.pt'), weights_only=True)
    torch.manual_seed(0)
    model = models.resnet18_pfan_human_parsing(**fx['config'])
    assert [(k, tuple(v.shape)) for k, v in sorted(model.state_dict().items())] == [(k, tuple(s)) for k, s in fx['keys']]


def test_config_imports_resolve_through_the_shim():
    from SimpleAICV.face_parsing import losses as face_losses
    from SimpleAICV.human_parsing import losses, models
    assert losses is _family('human', 'losses') and models is _family('human', 'models')
    assert face_losses.CELoss is losses.CELoss and face_losses.IoULoss is losses.IoULoss       # one implementation


@pytest.mark.parametrize('family', ['human', 'face'])
def test_collater_contract_and_synthetic_dataset(family):
    Family = family.capitalize()
    collater = getattr(_family(family, 'common'), f'{Family}ParsingCollater')(resize=32)
    dataset = getattr(_family(family, 'datasets.syntheticdataset'), f'Synthetic{Family}ParsingDataset')(3, 24, 20, seed=4)
    num_classes = 20 if family == 'human' else 19
    assert dataset.num_classes == num_classes and len(dataset) == 3
    a, b = dataset[1], dataset[1]
    assert np.array_equal(a['mask'], b['mask']) and np.array_equal(a['image'], b['image'])           # seeded per index
    assert a['image'].shape == (24, 20, 3) and a['image'].dtype == np.float32 and a['mask'].shape == (24, 20)
    ids = np.unique(a['mask'])
    assert len(ids) >= 2 and ids.min() == 0 and ids.max() < num_classes and np.array_equal(ids, ids.astype(np.int64))
    batch = collater([dataset[i] for i in range(3)])
    assert batch['image'].shape == (3, 3, 32, 32) and batch['image'].dtype == torch.float32
    assert batch['mask'].shape == (3, 32, 32) and batch['mask'].dtype == torch.float32
    assert isinstance(batch['size'], np.ndarray) and batch['size'].dtype == np.float32 and batch['size'].tolist() == [[24., 20.]] * 3
    assert float(batch['image'][:, :, 24:, :].abs().max()) == 0.0 and float(batch['image'][:, :, :, 20:].abs().max()) == 0.0
    assert float(batch['mask'][:, 24:, :].abs().max()) == 0.0 and float(batch['mask'][:, :, 20:].abs().max()) == 0.0
    assert torch.equal(batch['image'][1, :, :24, :20], torch.from_numpy(a['image']).permute(2, 0, 1))


@pytest.mark.parametrize('family', ['human', 'face'])
def test_losses_on_cpu_tensors_follow_the_reference_formulas(family):
    """spot values worked out by hand for two pixels"""
    losses = _family(family, 'losses')
    pred = torch.zeros(1, 2, 1, 2)
    pred[0, :, 0, 1] = torch.tensor([0., 100.])
    label = torch.tensor([[[0., 1.]]])
    # softmax: pixel 0 is (.5, .5); pixel 1 is (0, 1), clamped to (1e-4, 1 - 1e-4)
    ce = losses.CELoss()(pred, label)
    assert abs(float(ce) - (-np.log(.5) - np.log(1 - 1e-4)) / 2) < 1e-6
    iou = losses.IoULoss()(pred, label)
    want_iou = ((1 - .5 / (1. + 1. - .5)) + (1 - (1 - 1e-4) / (1. + 1. - (1 - 1e-4)))) / 2
    assert abs(float(iou) - want_iou) < 1e-6
    dice = losses.DiceLoss(logit_type='softmax')(pred, label)
    want_dice = ((1 - (2 * .5 + 1e-4) / (1. + 1. + 1e-4)) + (1 - (2 * (1 - 1e-4) + 1e-4) / (1. + 1. + 1e-4))) / 2
    assert abs(float(dice) - want_dice) < 1e-6
    # sigmoid: pixel 0 is (.5, .5); pixel 1 is (.5, 1 -> 1 - 1e-4)
    bce = losses.MultiClassBCELoss()(pred, label)
    assert abs(float(bce) - (2 * -np.log(.5) + -np.log(.5) + -np.log(1 - 1e-4)) / 4) < 1e-6
    iou_s = losses.IoULoss(logit_type='sigmoid')(pred, label)
    want = ((1 - .5 / (1. + 1. - .5)) + (1 - (1 - 1e-4) / ((1.5 - 1e-4) + 1. - (1 - 1e-4)))) / 2
    assert abs(float(iou_s) - want) < 1e-6
    dice_s = losses.DiceLoss(logit_type='sigmoid')(pred, label)
    want = ((1 - (2 * .5 + 1e-4) / (1. + 1. + 1e-4)) + (1 - (2 * (1 - 1e-4) + 1e-4) / ((1.5 - 1e-4) + 1. + 1e-4))) / 2
    assert abs(float(dice_s) - want) < 1e-6
    with pytest.raises(AssertionError):
        losses.IoULoss(logit_type='tanh')


def test_validation_arithmetic_on_hand_made_areas():
    from simpleaicv_pytorch_training_examples_amd.tools.human_parsing_scripts import parsing_metrics
    # class 0: 8 of 10 predicted pixels right, 16 in the ground truth; class 1: absent from the ground truth (3 predicted): skipped;
    # class 2: in the ground truth (5 pixels), never predicted; class 3: perfect
    intersect, pred, gt = [8., 0., 0., 4.], [10., 3., 0., 4.], [16., 0., 5., 4.]
    union = [p + g - i for i, p, g in zip(intersect, pred, gt)]
    r = parsing_metrics([intersect, pred, gt, union])
    assert list(r)[:5] == ['exist_num_class', 'mean_precision', 'mean_recall', 'mean_iou', 'mean_dice']
    assert list(r)[5:] == [f'class_{i}_{n}' for n in ('precision', 'recall', 'iou', 'dice') for i in range(4)]
    assert r['exist_num_class'] == 3.
    want = {'precision': [80., 0., 0., 100.], 'recall': [50., 0., 0., 100.], 'iou': [8. / 18 * 100, 0., 0., 100.],
            'dice': [16. / 26 * 100, 0., 0., 100.]}
    for name, values in want.items():
        for i, v in enumerate(values):
            assert abs(r[f'class_{i}_{name}'] - v) < 1e-9, (name, i)
        assert abs(r[f'mean_{name}'] - sum(values) / 3.) < 1e-9
    empty = parsing_metrics([[0.] * 3] * 4)
    assert empty['exist_num_class'] == 0. and empty['mean_iou'] == 0.


def test_validation_on_the_cpu_crops_to_size_and_returns_one_dict_per_set():
    """validate_human_parsing runs on the model's device: a stand-in model that predicts the mask's colour code on the CPU"""
    from simpleaicv_pytorch_training_examples_amd.tools import face_parsing_scripts, human_parsing_scripts
    losses = _family('human', 'losses')

    class Oracle(torch.nn.Module):
        """image channel 0 carries the class id; predicts it everywhere except that class 2 is called class 1"""

        def __init__(self):
            super().__init__()
            self.dummy = torch.nn.Parameter(torch.zeros(1))

        def forward(self, x):
            ids = x[:, 0].long()
            ids = torch.where(ids == 2, torch.ones_like(ids), ids)
            return torch.nn.functional.one_hot(ids, 4).permute(0, 3, 1, 2).float() * 20.

    mask = torch.zeros(2, 6, 6)
    mask[:, :2, :] = 1.
    mask[:, 2:4, :] = 2.
    mask[:, :, 4:] = 3.                         # columns 4, 5 lie outside the 4-wide crop
    image = torch.zeros(2, 3, 6, 6)
    image[:, 0] = mask
    batch = {'image': image, 'mask': mask, 'size': np.array([[6., 4.], [6., 4.]], dtype=np.float32)}

    class config:
        num_classes, batch_size, gpus_num = 4, 2, 1
        val_dataset_name_list = [['a'], ['b', 'c/d']]
    for scripts, name in ((human_parsing_scripts, 'validate_human_parsing_for_all_dataset'),
                          (face_parsing_scripts, 'validate_face_parsing_for_all_dataset')):
        results = getattr(scripts, name)([[batch], [batch, batch]], Oracle(), losses.CELoss(), config)
        assert list(results) == ['a', 'b[+]c[s]d']
        for r in results.values():
            assert r['exist_num_class'] == 3.                         # class 3 lies outside the crop: absent
            assert r['class_0_iou'] == 100. and r['class_2_iou'] == 0. and r['class_3_iou'] == 0.
            assert abs(r['class_1_precision'] - 50.) < 1e-9 and r['class_1_recall'] == 100.
            assert abs(r['mean_iou'] - (100. + 50. + 0.) / 3) < 1e-9 and abs(r['mean_dice'] - (100. + 200. / 3 + 0.) / 3) < 1e-9


@pytest.mark.parametrize('family,env,root,num_classes', [('human', 'SAICV_HP', '12.human_parsing_training/LIP', 20),
                                                         ('face', 'SAICV_FP', '11.face_parsing_training/CelebAMask-HQ', 19)])
def test_benchmark_configs_import_with_the_shorteners(monkeypatch, family, env, root, num_classes):
    for k, v in dict(TRAIN=8, TEST=4, BATCH=2, WORKERS=0, EPOCHS=2, PRINT=1).items():
        monkeypatch.setenv(f'{env}_{k}', str(v))
    work_dir = os.path.join(ROOT, *root.split('/'), f'resnet50_pfan_{family}_parsing')
    monkeypatch.syspath_prepend(ROOT)
    configs = {}
    for name in ('train_config', 'test_config'):
        monkeypatch.syspath_prepend(work_dir)
        monkeypatch.delitem(sys.modules, 'train_config', raising=False)
        spec = importlib.util.spec_from_file_location(f'saicv_{family}_parsing_{name}', os.path.join(work_dir, name + '.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        configs[name] = mod.config
    sys.modules.pop('train_config', None)              # (popped, not monkeypatched away: an undo would put the module back for later tests)
    c = configs['train_config']
    assert c.network == f'resnet50_pfan_{family}_parsing' and c.input_image_size == [512, 512] and c.num_classes == num_classes
    assert c.model.pred_conv.out_channels == num_classes
    assert list(c.train_criterion) == ['CELoss', 'IoULoss'] and c.loss_ratio == {'CELoss': 1.0, 'IoULoss': 1.0}
    assert c.train_criterion['IoULoss'].logit_type == 'softmax' and type(c.test_criterion).__name__ == 'CELoss'
    assert c.optimizer[0] == 'AdamW' and c.optimizer[1]['lr'] == 1e-4 and c.scheduler[0] == 'CosineLR'
    assert c.save_model_metric == 'mean_iou' and c.save_interval == 10 and c.eval_epoch == [2] and c.use_amp is True
    assert (len(c.train_dataset), len(c.val_dataset_list[0]), c.batch_size, c.num_workers, c.epochs, c.print_interval) == (8, 4, 2, 0, 2, 1)
    assert len(c.val_dataset_name_list) == len(c.val_dataset_list) == 1 and c.train_dataset.num_classes == num_classes
    t = configs['test_config']
    assert t.num_classes == num_classes and t.batch_size == 2 and len(t.val_dataset_list[0]) == 4 and type(t.model).__name__ == 'PFANParsing'
    monkeypatch.delenv(f'{env}_BATCH')
    assert int(os.environ.get(f'{env}_BATCH', 192)) == 192                        # the reference's global batch is the default
