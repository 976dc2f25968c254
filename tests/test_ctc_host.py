"""CPU checks of the text-recognition family: the float64 CTC judge (tests/ctc_common.py) against float64 torch and against values
recorded from the reference's own CTCLoss class (tests/golden/ctc_tiny.pt, scripts/record_ctc_golden.py); the package's CTCLoss
and ACELoss on CPU tensors; converter round trips; edit distance and LCS against hand-worked strings; and the conditions the GPU
tests' input recipes promise, on the same case list."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_common as cc
from conftest import load_golden


def _torch64(case, gamma=None):
    x = case['logits'].double().requires_grad_(True)
    tg = case['targets'].clone()
    for b in range(tg.shape[0]):
        tg[b, int(case['target_lengths'][b]):] = 0
    loss, nll = cc.reference_formula(x, tg, case['input_lengths'].long(), case['target_lengths'].long(), case['blank'], gamma)
    loss.backward()
    return float(loss.detach()), nll.numpy(), x.grad.numpy()


@pytest.mark.parametrize('key', [(3, 2, 3, 'first'), (37, 7, 3, 'c-2'), (65, 33, 3, 'last'), (257, 90, 1, 'first'), 'aa_aba_run5',
                                 'L40_T90', 'L80_T170', 'focal_planted'])
@pytest.mark.parametrize('gamma', [None, 2.0, 1.0])
def test_judge_agrees_with_float64_torch(key, gamma):
    """float64 against float64: 1e-10 (relative to the largest entry)"""
    case, j, _ = cc.case_and_judgement(key, gamma)
    loss, nll, grad = _torch64(case, gamma)
    assert abs(j['loss'] - loss) <= 1e-10 * max(1.0, abs(loss))
    assert np.abs(j['nll'] - nll).max() <= 1e-10 * max(1.0, np.abs(nll).max())
    assert np.abs(j['grad'] - grad).max() <= 1e-10 * max(np.abs(grad).max(), 1e-300)


@pytest.mark.parametrize('name, gamma', [('plain', None), ('focal', 2.0)])
def test_judge_and_cpu_loss_agree_with_the_recorded_reference(name, gamma):
    """the recording is fp32: the float64 judge agrees to fp32 rounding of a 10-frame recursion (1e-5 relative); the package's
    CTCLoss on CPU tensors runs the reference's own operations and reproduces the recorded values"""
    rec = load_golden('ctc_tiny')
    assert rec['blank'] == rec['preds'].shape[2] - 2 and int(rec['targets'].max()) == rec['preds'].shape[2] - 1
    j = cc.judge(rec['preds'].numpy(), rec['targets'].numpy(), rec['input_lengths'].numpy(), rec['target_lengths'].numpy(),
                 rec['blank'], gamma)
    ref_loss, ref_grad = float(rec[name]['loss']), rec[name]['grad'].double().numpy()
    assert abs(j['loss'] - ref_loss) <= 1e-5 * abs(ref_loss)
    assert np.abs(j['grad'] - ref_grad).max() <= 1e-5 * np.abs(ref_grad).max()
    assert abs(float(rec['plain']['loss']) - float(rec['focal']['loss'])) > 0.1          # the focal weight is not a no-op here

    from SimpleAICV.text_recognition.losses import CTCLoss
    x = rec['preds'].clone().requires_grad_(True)
    crit = CTCLoss(blank_index=rec['blank'], use_focal_weight=gamma is not None, gamma=gamma or 2.0)
    loss = crit(x, rec['targets'].float(), rec['input_lengths'], rec['target_lengths'])
    loss.backward()
    torch.testing.assert_close(loss.detach(), rec[name]['loss'], rtol=1e-6, atol=0)
    torch.testing.assert_close(x.grad, rec[name]['grad'], rtol=1e-5, atol=1e-7)
    assert crit.last_nll.shape == (3,)


def test_ace_loss_matches_the_reference_formula():
    """the reference's host loop (losses.py:49-80) written out, against the scatter_add histogram"""
    import collections
    from SimpleAICV.text_recognition.losses import ACELoss
    g = torch.Generator().manual_seed(4)
    t, b, c = 9, 3, 11
    preds = torch.randn(t, b, c, generator=g)
    targets = torch.tensor([[3, 3, 5, 0, 0, 0], [11, 2, 12, 7, 0, 0], [1, 1, 1, 1, 1, 1]])        # 11 and 12 are >= num_classes
    p = F.softmax(preds.float(), dim=2).mean(dim=0)
    want = torch.zeros(b, c)
    for i, row in enumerate(targets.numpy()):
        row = row[row < c]
        for k, v in collections.Counter(row).items():
            want[i][k] = v
        want[i][0] = t - np.sum(row > 0)
    want = want / t
    ref = (-torch.sum(torch.log(p) * want)) / b
    torch.testing.assert_close(ACELoss(blank_index=0)(preds, targets), ref, rtol=1e-6, atol=0)


def test_converter_round_trips():
    from SimpleAICV.text_recognition.char_sets.final_char_table import final_char_table
    from SimpleAICV.text_recognition.common import CTCTextLabelConverter
    conv = CTCTextLabelConverter(final_char_table, str_max_length=80, garbage_char='㍿')
    assert conv.num_classes == 12112 and conv.blank_index == 12111 and len(set(final_char_table)) == 12111
    texts = ['abc', 'hello7', 'aab', '一丁', 'xéy']                           # the last holds a character outside the table
    idx, length = conv.encode(texts)
    assert idx.shape == (5, 80) and idx.dtype == torch.int64 and length.dtype == torch.int32
    assert length.tolist() == [3, 6, 3, 2, 3]
    assert (idx[0, 3:] == conv.blank_index).all() and idx[4, 1] == conv.num_classes
    assert idx[0, :3].tolist() == [final_char_table.index(ch) for ch in 'abc']
    # a frame sequence: every label once, a blank between equal neighbours, each frame doubled
    frames = torch.full((5, 40), conv.blank_index, dtype=torch.long)
    for i in range(5):
        seq = []
        for k in idx[i, :length[i]].tolist():
            seq += [k, k, conv.blank_index]
        frames[i, :len(seq)] = torch.tensor(seq)
    out = conv.decode(frames, [40] * 5)
    assert out[:4] == texts[:4] and out[4] == 'x㍿㍿y'                               # (the reference appends the garbage mark per FRAME)
    assert conv.decode(torch.tensor([[0, 0, -1, -1]]), [4]) == ['0']                   # -1: ops.ctc_greedy beyond the sample's frames


def test_edit_distance_and_lcs_on_hand_worked_strings():
    from SimpleAICV.text_recognition.common import edit_distance, lcs_length
    assert edit_distance('kitten', 'sitting') == 3           # k->s, e->i, +g
    assert edit_distance('', 'abc') == 3 and edit_distance('abc', '') == 3 and edit_distance('abc', 'abc') == 0
    assert edit_distance('flaw', 'lawn') == 2                # -f, +n
    assert edit_distance('你好吗', '他好吗') == 1
    assert lcs_length('ABCBDAB', 'BDCABA') == 4              # BCBA
    assert lcs_length('', 'abc') == 0 and lcs_length('abc', 'abc') == 3
    assert lcs_length('AGGTAB', 'GXTXAYB') == 4              # GTAB
    assert lcs_length('大家都好吗', '大家好') == 3


def test_collater_and_normalize():
    from SimpleAICV.text_recognition.common import KeepRatioResizeTextRecognitionCollater, Normalize
    rng = np.random.default_rng(0)
    data = [Normalize()({'image': rng.uniform(0, 255, (32, w, 3)).astype(np.float32), 'label': 'ab', 'scale': 1.0,
                         'size': np.array([32, w], dtype=np.float32)}) for w in (64, 100)]
    data.append({'image': rng.uniform(0, 1, (16, 40, 3)).astype(np.float32), 'label': 'c', 'scale': 1.0, 'size': None})
    out = KeepRatioResizeTextRecognitionCollater(resize_h=32)(data)
    assert out['image'].shape == (3, 3, 32, 128) and out['label'] == ['ab', 'ab', 'c']
    assert float(out['image'].max()) <= 1.0
    assert torch.equal(out['image'][0, :, :, :64], torch.from_numpy(data[0]['image']).permute(2, 0, 1))
    assert float(out['image'][0, :, :, 64:].abs().max()) == 0 and float(out['image'][2, :, :, 80:].abs().max()) == 0
    assert float(out['image'][2, :, :, :80].abs().min()) > 0


def test_synthetic_dataset_feeds_the_collater_and_the_converter():
    from SimpleAICV.text_recognition.char_sets.final_char_table import final_char_table
    from SimpleAICV.text_recognition.common import CTCTextLabelConverter, KeepRatioResizeTextRecognitionCollater
    from SimpleAICV.text_recognition.datasets.syntheticdataset import SyntheticTextRecognitionDataset
    ds = SyntheticTextRecognitionDataset(6, final_char_table, height=32, width=128, max_length=24, seed=3)
    a, b = ds[2], ds[2]
    assert a['label'] == b['label'] and np.array_equal(a['image'], b['image'])        # a sample is a function of (seed, index)
    assert a['image'].shape == (32, 128, 3) and a['image'].dtype == np.float32
    assert 0.0 <= a['image'].min() and a['image'].max() <= 1.0 and a['size'].tolist() == [32.0, 128.0]
    labels = [ds[i]['label'] for i in range(6)]
    assert all(1 <= len(s) <= 24 for s in labels) and len(set(labels)) == 6
    batch = KeepRatioResizeTextRecognitionCollater(resize_h=32)([ds[i] for i in range(6)])
    assert batch['image'].shape == (6, 3, 32, 160) and batch['label'] == labels      # 128 rounds up to the NEXT multiple of 32
    idx, length = CTCTextLabelConverter(final_char_table).encode(batch['label'])
    assert length.tolist() == [len(s) for s in labels] and int(idx.max()) <= 12111   # no character falls outside the table
    var = SyntheticTextRecognitionDataset(8, final_char_table, height=32, width=128, variable_width=True, seed=1)
    widths = {var[i]['image'].shape[1] for i in range(8)}
    assert len(widths) > 1 and min(widths) >= 64 and max(widths) <= 128
    assert KeepRatioResizeTextRecognitionCollater(32)([var[i] for i in range(8)])['image'].shape[3] % 32 == 0


def test_recipe_conditions():
    """what the GPU tests rely on, asserted on their own case list"""
    for key in cc.grid_cases():
        C, T, B, where = key
        case = cc.make_case(*key)
        blank = case['blank']
        assert blank == {'first': 0, 'c-2': C - 2, 'last': C - 1}[where]
        tg, tl, il = case['targets'], case['target_lengths'], case['input_lengths']
        assert torch.equal(case['logits'], case['logits'].bfloat16().float())                         # bf16-exact: both dtypes judge one input
        for b in range(B):
            lab = tg[b, :tl[b]]
            assert len(lab) >= 1 and int(lab.min()) >= 0 and int(lab.max()) < C and not (lab == blank).any()
            assert (tg[b, tl[b]:] == C + cc.PAD_OFFSET).all() and tg.shape[1] > int(tl[b])              # poisoned padding exists
            need = int(tl[b]) + int((lab[1:] == lab[:-1]).sum())
            assert (need > int(il[b])) == (b == 2), key                                                 # sample 2, and only it, is infeasible
        if B == 3:
            assert int(il[1]) < T or T == 1
            assert int(il[0]) == T and int(il[2]) == T
    # label coverage over the grid, per class count: class 0, class C - 1 and both sides of the loop boundaries below C
    for C in cc.GRID_C:
        seen = set()
        for T in cc.GRID_T:
            for where in cc.BLANKS:
                case = cc.make_case(C, T, 3, where)
                for b in range(2):
                    seen.update(case['targets'][b, :case['target_lengths'][b]].tolist())
        assert {0, C - 1} <= seen, (C, sorted(seen))
        if C == 12113:
            assert {3, 4, 7, 8, 255, 256, 511, 512, 1023, 1024, 2047, 2048, 12111, 12112} <= seen, sorted(seen)   # 12112 = C // 8 * 8
    sp = cc.special_cases()
    assert int(sp['L1']['target_lengths'][0]) == 1
    assert 2 * int(sp['L40_T90']['target_lengths'][0]) + 1 == 81 and sp['L40_T90']['logits'].shape[0] == 90
    assert 2 * int(sp['L80_T170']['target_lengths'][0]) + 1 == 161 and sp['L80_T170']['logits'].shape[0] == 170
    assert sp['aa_aba_run5']['targets'][:, :5].tolist()[0][:2] == [4, 4]
    _, j, _ = cc.case_and_judgement('L80_T170')
    assert j['feasible'].tolist() == [True, False]
    _, j, _ = cc.case_and_judgement('focal_planted', 2.0)
    assert (j['nll'] < 3).all() and (j['nll'] > 0.01).all()                                            # the focal weight is far from 0 and from 1


@pytest.mark.parametrize('C', cc.GRID_C)
def test_greedy_recipe_has_a_unit_gap(C):
    logits, pick = cc.greedy_case(C, 7, 3)
    assert torch.equal(logits, logits.bfloat16().float())
    top2 = logits.topk(2, dim=2).values
    assert (top2[..., 0] - top2[..., 1] >= 1.0).all()
    assert torch.equal(logits.argmax(dim=2), pick)
    edges = cc.boundary_classes(C)
    assert set(pick.view(-1)[:min(21, len(edges))].tolist()) == set(edges[:21])
