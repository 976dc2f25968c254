"""Host-side checks of the universal-matting family: the float64 judges of tests/unimat_common.py pinned to values recorded from the
reference's own classes (tests/golden/unimat_tiny.pt), the composed loss route on CPU tensors against the same, the collaters, the
decoder, the synthetic dataset, the two entry modules and the C-ABI surface of csrc/unimat.hip.  No GPU."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import unimat_common as U
from conftest import ROOT, load_golden

PKG = 'simpleaicv_pytorch_training_examples_amd'
SYMBOLS = ('saicv_unimat_chunk', 'saicv_unimat_pair_ws_floats', 'saicv_unimat_pair_sums', 'saicv_unimat_head_fwd', 'saicv_unimat_head_bwd')


@pytest.fixture(scope='module')
def fx():
    return load_golden('unimat_tiny')


@pytest.mark.parametrize('case', U.LOSS_CASES, ids=U.case_id)
def test_judge_pinned_to_reference(fx, case):
    rec = fx['loss_cases'][U.case_id(case)]
    assert fx['loss_weights'] == U.LOSS_WEIGHTS and fx['loss_classes'] == U.LOSS_CLASSES
    gp, lp, fp, cp, trimaps, alphas, labels = U.loss_inputs(case)
    assert torch.equal(fp, U.fuse(gp, lp))
    judge = U.judge_loss(gp, lp, fp, cp, trimaps, alphas, labels)
    for i, (want, dev) in enumerate(zip(rec['cost'], rec['cost_dev'])):
        got = judge['costs'][i]
        assert got.shape == want.shape and want.numel() > 0
        # the reference's fp32 matrix lies `dev` (of its largest entry) from its own float64 run.  The judge is that run except for
        # the clamp bounds, which it takes as the fp32 tensors hold them: float32(1 - 1e-4) lies up to 2^-25 from 0.9999, and a
        # prediction at the bound moves each of the four map terms (mean slopes <= 1, cost weights 1) by at most that
        assert float((got - want.double()).abs().max()) <= dev * float(want.abs().max()) + 4 * 2.0 ** -25
        assert rec['margin'][i] >= 1e-3 and dev <= 4e-7
        q, t = judge['indices'][i]
        assert np.array_equal(q, rec['indices'][i][0].numpy()) and np.array_equal(t, rec['indices'][i][1].numpy())
    assert tuple(rec['losses']) == U.LOSS_KEYS
    for k in U.LOSS_KEYS:
        # float64 against float64: what is left is the clamp bound again (a mean whose slope in the bound is at most 1)
        assert abs(judge['losses'][k] - rec['losses64'][k]) <= 1e-9 * abs(rec['losses64'][k]) + 2.0 ** -25, (k, judge['losses'][k], rec['losses64'][k])
        assert abs(judge['losses'][k] - rec['losses'][k]) <= 2e-6 * abs(rec['losses'][k]), (k, judge['losses'][k], rec['losses'][k])


@pytest.mark.parametrize('case', U.LOSS_CASES, ids=U.case_id)
def test_composed_route_on_cpu_tensors(fx, case):
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.universal_segmentation.matting_losses import UniversalMattingLoss
    rec = fx['loss_cases'][U.case_id(case)]
    gp, lp, fp, cp, trimaps, alphas, labels = U.loss_inputs(case)
    crit = UniversalMattingLoss(num_classes=U.LOSS_CLASSES, **U.LOSS_WEIGHTS)
    leaves = [t.clone().requires_grad_(True) for t in (gp, lp, fp, cp)]
    out = crit(*leaves, trimaps, alphas, labels)
    assert tuple(out) == U.LOSS_KEYS
    for (q, t), (rq, rt) in zip(crit.last_indices, rec['indices']):
        assert np.array_equal(q, rq.numpy()) and np.array_equal(t, rt.numpy())
    for k in U.LOSS_KEYS:
        assert abs(float(out[k].detach()) - rec['losses'][k]) <= 2e-5 * abs(rec['losses'][k]), (k, float(out[k].detach()), rec['losses'][k])
    sum(out.values()).backward()
    judge = U.judge_loss(gp, lp, fp, cp, trimaps, alphas, labels)
    for leaf, name in zip(leaves, ('dglobal', 'dlocal', 'dfused', 'dclass')):
        want = judge[name]
        assert float((leaf.grad.double() - want).abs().max()) <= 1e-4 * float(want.abs().max()), name


def test_no_object_and_no_pair():
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.universal_segmentation.matting_losses import UniversalMattingLoss
    gp, lp, fp, cp, trimaps, alphas, labels = U.make_inputs(2, 3, [0, 2], 32, 32, seed=4)
    crit = UniversalMattingLoss(num_classes=U.LOSS_CLASSES)
    out = crit(gp, lp, fp, cp, trimaps, alphas, labels)                      # an image without objects contributes no pair
    assert len(crit.last_indices[0][0]) == 0 and len(crit.last_indices[1][0]) == 2 and all(bool(torch.isfinite(v)) for v in out.values())
    want = U.judge_loss(gp, lp, fp, cp, trimaps, alphas, labels)['losses']
    assert all(abs(float(out[k]) - want[k]) <= 2e-5 * abs(want[k]) for k in U.LOSS_KEYS)
    none = crit(gp, lp, fp, cp, [t[:0] for t in trimaps], [a[:0] for a in alphas], [l[:0] for l in labels])
    assert all(bool(torch.isnan(none[k])) for k in U.LOSS_KEYS[:6]) and bool(torch.isfinite(none['class_loss']))
    judged = U.judge_loss(gp, lp, fp, cp, [t[:0] for t in trimaps], [a[:0] for a in alphas], [l[:0] for l in labels])['losses']
    assert all(np.isnan(judged[k]) for k in U.LOSS_KEYS[:6])
    crit.route = 'nonsense'
    os.environ['SAICV_UNIMAT_LOSS'] = 'nonsense'
    try:
        from simpleaicv_pytorch_training_examples_amd.SimpleAICV.universal_segmentation import matting_losses
        with pytest.raises(ValueError):
            matting_losses.default_route()
    finally:
        os.environ.pop('SAICV_UNIMAT_LOSS')


def test_take_rows_keeps_the_memory_order():
    from simpleaicv_pytorch_training_examples_amd import ops
    x = U.channels_last(torch.randn(2, 4, 3, 5, 6)).requires_grad_(True)
    rows = ops.take_rows(x, [1, 0, 1], [3, 0, 1])
    assert rows.is_contiguous() and torch.equal(rows, x.detach()[[1, 0, 1], [3, 0, 1]])
    g = torch.randn_like(rows)
    rows.backward(g)
    assert x.grad.stride() == x.stride() and x.grad.stride(2) == 1
    want = torch.zeros(2, 4, 3, 5, 6)
    want[[1, 0, 1], [3, 0, 1]] = g
    assert torch.equal(x.grad, want)


def _sample(h, w, s=7.):
    alpha = np.zeros((h, w), dtype=np.float32)
    alpha[1:3, 1:4] = 1.
    alpha[3, 1:4] = 0.5
    trimap = np.where(alpha == 1, 255, np.where(alpha == 0, 0, 128)).astype(np.uint8)
    return {'image': np.full((h, w, 3), s, dtype=np.float32), 'mask': alpha, 'trimap': trimap, 'fg_map': np.full((h, w, 3), 2., dtype=np.float32),
            'bg_map': np.full((h, w, 3), 3., dtype=np.float32), 'size': np.array([h, w], dtype=np.float32),
            'origin_size': np.array([h, w], dtype=np.float32)}


def test_collaters_on_hand_made_samples():
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.universal_segmentation import human_matting_common as C
    out = C.HumanMattingTrainCollater(resize=8)([_sample(5, 6), _sample(8, 8)])
    assert tuple(out['image'].shape) == (2, 3, 8, 8) and float(out['image'][0, 0, 4, 5]) == 7. and float(out['image'][0, 0, 5, 0]) == 0.
    assert [tuple(m.shape) for m in out['mask']] == [(1, 8, 8)] * 2 and out['mask'][0].dtype == torch.float32
    assert out['trimap'][0].dtype == torch.float32 and sorted(out['trimap'][0].unique().tolist()) == [0., 128., 255.]
    assert float(out['trimap'][0][0, 3, 2]) == 128. and float(out['mask'][0][0, 3, 2]) == 0.5 and float(out['mask'][0][0, 5:].sum()) == 0.
    assert tuple(out['fg_map'][0].shape) == (1, 3, 8, 8) and float(out['bg_map'][1][0, 2, 7, 7]) == 3.
    assert [l.tolist() for l in out['label']] == [[0], [0]] and out['label'][0].dtype == torch.int64
    assert out['size'].tolist() == [[5., 6.], [8., 8.]]
    empty = _sample(5, 6)
    empty['mask'] = np.zeros((5, 6), dtype=np.float32)
    with pytest.raises(AssertionError):
        C.HumanMattingTrainCollater(resize=8)([empty])
    test = C.HumanMattingTestCollater(resize=8)([_sample(5, 6)])
    assert tuple(test['mask'].shape) == (1, 8, 8) and tuple(test['trimap'].shape) == (1, 8, 8) and tuple(test['fg_map'].shape) == (1, 3, 8, 8)
    assert test['origin_size'].tolist() == [[5., 6.]] and float(test['trimap'][0, 1, 1]) == 255.
    flipped = C.RandomHorizontalFlip(prob=1.)(_sample(5, 6))
    assert float(flipped['mask'][1, 2]) == 1. and float(flipped['mask'][1, 0]) == 0. and float(flipped['trimap'][3, 4]) == 128
    assert float(C.Normalize()(_sample(5, 6, 255.))['image'].max()) == 1.
    assert callable(C.load_state_dict)


def test_decoder_on_a_hand_made_prediction():
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.universal_segmentation.matting_decode import UniversalMattingDecoder
    fused = torch.zeros(2, 3, 1, 4, 4)
    fused[0, 0, 0, :2] = 0.25
    fused[0, 2, 0, :, :2] = 0.75
    class_preds = torch.zeros(2, 3, 2)
    class_preds[0, 0, 0] = 2.                       # query 0: foreground 0.88
    class_preds[0, 1, 1] = 9.                       # query 1: background
    class_preds[0, 2, 0] = 6.                       # query 2: foreground 0.998, sorted first
    class_preds[1, :, 1] = 9.                       # image 1 keeps nothing
    sizes = np.array([[4., 4.], [4., 4.]])
    masks, scores, classes = UniversalMattingDecoder(topk=100, min_score_threshold=0.1)((None, None, fused, class_preds), sizes, sizes)
    assert masks[0].shape == (2, 4, 4) and masks[0].dtype == np.float32 and scores[0][0] > scores[0][1] > 0.8 and classes[0].tolist() == [0, 0]
    assert masks[0][0].tolist() == [[0.75, 0.75, 0., 0.]] * 4 and masks[0][1][0].tolist() == [0.25] * 4
    assert masks[1].shape == (0, 4, 4) and scores[1].shape == (0, ) and classes[1].shape == (0, )
    top1 = UniversalMattingDecoder(topk=1)((None, None, fused, class_preds), np.array([[4., 2.]] * 2), np.array([[8., 4.]] * 2))
    assert top1[0][0].shape == (1, 8, 4) and float(top1[0][0].min()) == 0.75      # cropped to the scaled size, then resized


def test_synthetic_dataset():
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.universal_segmentation.datasets.syntheticmattingdataset import \
        SyntheticUniversalMattingDataset
    ds = SyntheticUniversalMattingDataset(3, image_size=64, seed=2)
    s = ds[1]
    assert len(ds) == 3 and set(s) == {'image', 'mask', 'trimap', 'fg_map', 'bg_map', 'size', 'origin_size'}
    assert s['image'].shape == (64, 64, 3) and s['image'].dtype == np.float32 and s['mask'].shape == (64, 64)
    assert s['trimap'].dtype == np.uint8 and sorted(np.unique(s['trimap']).tolist()) == [0, 128, 255]
    assert np.array_equal(s['trimap'] == 255, s['mask'] == 1.) and np.array_equal(s['trimap'] == 0, s['mask'] == 0.)
    assert 0. <= s['mask'].min() and s['mask'].max() == 1. and np.count_nonzero(s['mask']) > 0
    a = s['mask'][:, :, None]
    assert np.allclose(s['image'], a * s['fg_map'] + (1 - a) * s['bg_map'], atol=1e-3)
    assert np.array_equal(ds[1]['mask'], s['mask']) and not np.array_equal(ds[2]['mask'], s['mask'])
    assert s['size'].tolist() == [64., 64.] and s['origin_size'].tolist() == [64., 64.]


def test_model_keys_match_the_reference(fx):
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.universal_segmentation import models
    M = models.dinov3_universal_matting
    assert len(M.__all__) == 6 and all(n.endswith('_universal_matting') and callable(getattr(M, n)) for n in M.__all__)
    assert M.ScaleBlock is models.dinov3_universal_segmentation.ScaleBlock and models.UniversalMatting is M.UniversalMatting
    rec = fx['model']
    assert rec['config'] == U.MODEL_CFG
    torch.manual_seed(U.MODEL_SEEDS['build'])
    model = M.__dict__[rec['name']](**rec['config'])
    sd = model.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(s)) for k, s in rec['keys']]
    for k, want in rec['init_sample'].items():                        # the same seed draws the reference's initial values
        assert torch.equal(sd[k].flatten()[U.sample_idx(sd[k].numel())], want), k
    heads = [k for k in sd if not k.startswith('backbone.')]
    assert heads[:3] == ['query_embedding.weight', 'class_pred.weight', 'class_pred.bias']
    assert tuple(sd['global_upscale_blocks.1.conv1.weight'].shape) == (15, 15, 2, 2) and tuple(sd['local_upscale_blocks.0.norm.weight'].shape) == (5, )
    assert rec['fused_flipped'] == 0 and rec['undecided'].shape[0] <= U.UNDECIDED_CAP * rec['fused_preds'].numel()


def test_entry_modules_keep_the_surface():
    for name, words in (('train_universal_matting_model', 'Training'), ('test_universal_segmentation_model_for_human_matting_dataset', 'Testing')):
        m = importlib.import_module(f'{PKG}.tools.{name}')
        assert callable(m.main) and callable(m.parse_args) and m.TASK is not None
        assert f'-m {PKG}.tools.{name} --work-dir ./' in m.__doc__
        src = open(m.__file__).read()
        assert f"description='PyTorch Universal Matting {words} (MI355X engine)'" in src
    from simpleaicv_pytorch_training_examples_amd.tools import entry, universal_matting_scripts as S
    train = importlib.import_module(f'{PKG}.tools.train_universal_matting_model').TASK
    test = importlib.import_module(f'{PKG}.tools.test_universal_segmentation_model_for_human_matting_dataset').TASK
    assert train.train is S.train_universal_matting and train.best is entry.BEST_LOSS
    assert test.validate is S.validate_human_matting_for_all_dataset and test.report is entry.report_datasets

    class cfg:
        decoder = object()
    assert test.extra_args(cfg) == (cfg.decoder, )
    for d in ('train_config.py', 'test_config.py'):
        assert os.path.exists(os.path.join(ROOT, '16.universal_segmentation_training', '16.3.human_matting_training',
                                           'dinov3_vit_large_patch16_universal_matting', d))


def test_header_binding_and_guide_name_the_new_symbols():
    from simpleaicv_pytorch_training_examples_amd import _lib
    from ctypes import c_int, c_long, c_size_t, c_void_p
    header = open(os.path.join(ROOT, 'include', 'saicv_hip.h')).read()
    source = open(os.path.join(ROOT, PKG, 'csrc', 'unimat.hip')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', header) and name in _lib.SIGNATURES
        assert len(re.findall(r'^extern "C" (?:int|size_t) ' + name + r'\(', source, flags=re.M)) == 1
    assert 'unimat.hip' in open(os.path.join(ROOT, PKG, 'build.py')).read()
    P = c_void_p
    assert _lib.SIGNATURES['saicv_unimat_pair_sums'] == (c_int, [P] + [c_long] * 4 + [P] + [c_long] * 3 + [P] + [c_long] * 3 + [P, P, P]
                                                         + [c_int] * 4 + [c_size_t, P, P, P])
    assert _lib.SIGNATURES['saicv_unimat_head_fwd'] == (c_int, [c_int, P, P, c_size_t, c_int, P, P, P, P])
    assert _lib.SIGNATURES['saicv_unimat_head_bwd'] == (c_int, [c_int, P, P, P, P, P, c_size_t, c_int, P, P, P])
    assert _lib.SIGNATURES['saicv_unimat_chunk'] == (c_int, []) and _lib.SIGNATURES['saicv_unimat_pair_ws_floats'] == (c_size_t, [c_int] * 3 + [c_size_t])
    for word in ('`saicv_unimat_pair_sums`', '`saicv_unimat_head_fwd / _bwd`', '`SAICV_UNIMAT_LOSS`', 'SAICV_UNIMAT_*', 'train_universal_matting_model'):
        assert word in doc, word
