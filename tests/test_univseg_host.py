"""Host-side checks of the universal-segmentation family: the float64 judges of tests/univseg_common.py pinned to values recorded
from the reference's own classes (tests/golden/univseg_tiny.pt), the collaters, the decoder and the model's key list.  No GPU."""
import numpy as np
import pytest
import torch

import univseg_common as U
from conftest import load_golden


@pytest.fixture(scope='module')
def fx():
    return load_golden('univseg_tiny')


@pytest.mark.parametrize('case', U.LOSS_CASES, ids=U.case_id)
def test_judge_pinned_to_reference(fx, case):
    rec = fx['loss_cases'][U.case_id(case)]
    assert fx['loss_weights'] == U.LOSS_WEIGHTS
    x, cp, targets, labels = U.loss_inputs(case)
    judge = U.judge_loss(x, cp, targets, labels)
    for i, (want, dev) in enumerate(zip(rec['cost'], rec['cost_dev'])):
        got = judge['costs'][i]
        assert got.shape == want.shape
        if want.numel():
            # the reference's fp32 matrix lies `dev` from its own float64 run; the judge is that run up to float64 rounding
            assert float((got - want.double()).abs().max()) <= dev * (1 + 1e-6) + 1e-10
        assert rec['margin'][i] >= 1e-3
        q, t = judge['indices'][i]
        assert np.array_equal(q, rec['indices'][i][0].numpy()) and np.array_equal(t, rec['indices'][i][1].numpy())
    for k, want in rec['losses'].items():
        assert abs(judge['losses'][k] - want) <= 1e-6 * abs(want), (k, judge['losses'][k], want)


def test_judge_no_pair_is_nan():
    x, cp, _, _ = U.make_inputs((2, 3, [0, 0], 4, 4))
    out = U.judge_loss(x, cp, [torch.zeros(0, 4, 4)] * 2, [torch.zeros(0, dtype=torch.int64)] * 2)['losses']
    assert np.isnan(out['mask_loss']) and np.isnan(out['dice_loss']) and np.isfinite(out['class_loss'])


def _sample(mask, size=None):
    h, w = mask.shape
    return {'image': np.full((h, w, 3), 7., dtype=np.float32), 'mask': mask.astype(np.float32),
            'size': np.array(size or [h, w], dtype=np.float32), 'origin_size': np.array([h, w], dtype=np.float32)}


def test_train_collater_on_a_hand_made_label_map():
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.universal_segmentation.semantic_segmentation_common import \
        SemanticSegmentationTrainCollater
    m = np.zeros((4, 6))
    m[0, :3] = 9
    m[1:3, 2:5] = 3
    m[3, 5] = 150
    out = SemanticSegmentationTrainCollater(resize=8)([_sample(m), _sample(np.full((8, 8), 5.))])
    assert tuple(out['image'].shape) == (2, 3, 8, 8) and float(out['image'][0, 0, 3, 5]) == 7. and float(out['image'][0, 0, 4, 0]) == 0.
    assert out['label'][0].tolist() == [2, 8, 149] and out['label'][0].dtype == torch.int64         # sorted, background gone, ids - 1
    masks = out['mask'][0]
    assert tuple(masks.shape) == (3, 8, 8) and masks.dtype == torch.float32
    assert torch.equal(masks[0, :4, :6], torch.from_numpy((m == 3).astype(np.float32)))
    assert torch.equal(masks[1, :4, :6], torch.from_numpy((m == 9).astype(np.float32)))
    assert float(masks[2].sum()) == 1. and float(masks[2, 3, 5]) == 1. and float(masks[:, 4:].sum()) == 0.
    assert out['label'][1].tolist() == [4] and float(out['mask'][1].sum()) == 64.
    assert out['size'].tolist() == [[4., 6.], [8., 8.]]
    with pytest.raises(ValueError):                                   # an all-background map: np.stack of nothing, as in the reference
        SemanticSegmentationTrainCollater(resize=8)([_sample(np.zeros((4, 4)))])


def test_test_collater_keeps_the_label_map():
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.universal_segmentation.semantic_segmentation_common import \
        SemanticSegmentationTestCollater
    m = np.arange(12).reshape(3, 4) % 5
    out = SemanticSegmentationTestCollater(resize=6)([_sample(m)])
    assert tuple(out['mask'].shape) == (1, 6, 6) and torch.equal(out['mask'][0, :3, :4], torch.from_numpy(m.astype(np.float32)))
    assert float(out['mask'][0, 3:].sum()) == 0. and out['size'].tolist() == [[3., 4.]] and out['origin_size'][0].tolist() == [3., 4.]


def test_decoder_on_a_hand_made_prediction():
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.universal_segmentation.segmentation_decode import \
        UniversalSegmentationDecoder
    mask_preds = torch.full((2, 3, 4, 4), -9.)
    mask_preds[0, 0, :2] = 9.                      # query 0: the upper half
    mask_preds[0, 2, :, :2] = 9.                   # query 2: the left half
    class_preds = torch.zeros(2, 3, 4)             # 3 foreground classes + background
    class_preds[0, 0, 1] = 4.                      # query 0 -> class 1, probability 0.948
    class_preds[0, 1, 3] = 9.                      # query 1 -> background: every foreground score below the threshold
    class_preds[0, 2, 2] = 6.                      # query 2 -> class 2, probability 0.993: sorted first
    class_preds[1, :, 3] = 9.                      # image 1: nothing kept
    dec = UniversalSegmentationDecoder(topk=100, min_score_threshold=0.1, mask_threshold=0.5, binary_mask=True)
    masks, scores, classes = dec((mask_preds, class_preds), np.array([[4., 4.], [4., 4.]]), np.array([[4., 4.], [4., 4.]]))
    assert classes[0].tolist() == [2, 0 + 1] and scores[0][0] > scores[0][1] > 0.9
    assert masks[0].dtype == np.uint8 and masks[0].shape == (2, 4, 4)
    assert masks[0][0].tolist() == [[1, 1, 0, 0]] * 4 and masks[0][1].tolist() == [[1] * 4, [1] * 4, [0] * 4, [0] * 4]
    assert masks[1].shape == (0, 4, 4) and scores[1].shape == (0, ) and classes[1].shape == (0, )
    top1 = UniversalSegmentationDecoder(topk=1)((mask_preds, class_preds), np.array([[4., 4.]] * 2), np.array([[8., 8.]] * 2))
    assert top1[2][0].tolist() == [2] and top1[0][0].shape == (1, 8, 8)


def test_model_keys_match_the_reference(fx):
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.universal_segmentation import models
    assert sorted(models.dinov3_universal_segmentation.__all__) == sorted(n for n in dir(models) if n.startswith('dinov3_vit_'))
    assert len(models.dinov3_universal_segmentation.__all__) == 6
    rec = fx['model']
    torch.manual_seed(0)
    model = models.__dict__[rec['name']](**rec['config'])
    sd = model.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(s)) for k, s in rec['keys']]
    for k, want in rec['init_sample'].items():                        # the same seed draws the reference's initial values
        assert torch.equal(sd[k].flatten()[U.sample_idx(sd[k].numel())], want), k
    heads = [k for k in sd if not k.startswith('backbone.')]
    assert heads[:3] == ['query_embedding.weight', 'class_pred.weight', 'class_pred.bias']
    assert [k for k in heads if k.startswith('upscale_blocks.0.')] == ['upscale_blocks.0.' + n for n in (
        'conv1.weight', 'conv1.bias', 'conv2.weight', 'norm.weight', 'norm.bias')]
    assert models.__dict__[rec['name']](use_gradient_checkpoint=True, **rec['config']).use_gradient_checkpoint
