"""The judge of tests/detloss_common.py, checked without a GPU: the float64 references agree with the reference project's own code on
the edge inputs (tests/golden/detloss_edges.pt, oracle/make_golden_detloss_edges.py), every planted edge is present in the inputs it
is claimed for, every exactness premise holds in float64, the fp32 emulations meet the bounds and set CONSTANTS, every planted fault
makes at least one case miss, the left-out shares stay within the cap on the reference alone, and the case tables reach every launch
form of csrc/detloss.hip."""
import math
import os

import numpy as np
import pytest
import torch

import detloss_common as D
from conftest import GOLDEN

F64 = torch.float64


@pytest.fixture(scope='module')
def golden():
    return torch.load(os.path.join(GOLDEN, 'detloss_edges.pt'), weights_only=True)


# ------------------------------------------------------------------------------------------------ the clamp and thresholds as the kernel holds them
def test_the_kernels_constants_are_torchs():
    """`1.f - 1e-4f` evaluated in fp32 is the fp32 value of torch.clamp's 0.9999, and 0.4f / 0.5f those of `overlap < 0.4`"""
    assert D.HI == float(np.float32(0.9999)) == float(torch.tensor(1. - 1e-4, dtype=torch.float32))
    assert D.LO == float(torch.tensor(1e-4, dtype=torch.float32))
    assert D.T04 == float(torch.tensor(0.4, dtype=torch.float32)) and float(np.float32(100) / np.float32(250)) == D.T04


# ------------------------------------------------------------------------------------------------ against the reference project's own code
def test_retina_reference_agrees_with_the_reference_project_on_the_edges(golden):
    for case in D.edge_cases()['retina']:
        rec = golden['retina'][case.id]
        spec, _ = D.retina_reference(case, D.retina_inputs(case))
        cls = spec['cls'][1]
        assert torch.equal(cls, rec['cls'].to(F64)), case.id
        assert float(spec['pos'][1]) - D.POS_PREFILL == rec['pos']
        if not case.smoothl1:
            assert torch.equal(spec['box'][1], rec['box'].to(F64)), case.id
        val, bnd = D.edge_focal_scalar(case.id, cls)
        assert abs(val - rec['cls_loss']) <= D.MARGIN * D.CONSTANTS['focal_sum'] * D.UF * bnd, (case.id, val, rec['cls_loss'])
        if case.smoothl1:
            box = torch.cat([spec['box_xy'][1], spec['box_wh'][1]], 2)
            val, bnd = D.edge_smooth_scalar(case.id, cls, box)
            assert abs(val - rec['reg_loss']) <= D.MARGIN * D.CONSTANTS['smoothl1_sum'] * D.UF * bnd, (case.id, val, rec['reg_loss'])


def test_fcos_reference_agrees_with_the_reference_project_on_the_edges(golden):
    for case in D.edge_cases()['fcos']:
        rec = golden['fcos'][case.id]
        spec, _ = D.fcos_reference(case, D.fcos_inputs(case))
        assert torch.equal(spec['cls'][1], rec['cls'].to(F64)), case.id
        assert torch.equal(spec['ltrb'][1], rec['ltrb'].to(F64)), case.id
        assert float(spec['pos'][1]) - D.POS_PREFILL == rec['pos']
        val, bnd = D.edge_focal_scalar(case.id, spec['cls'][1])
        assert abs(val - rec['cls_loss']) <= D.MARGIN * D.CONSTANTS['focal_sum'] * D.UF * bnd, (case.id, val, rec['cls_loss'])


def test_best_class_reference_agrees_with_numpys_argmax_on_the_edges(golden):
    for case in D.edge_cases()['best']:
        spec = D.best_reference(case, D.best_inputs(case))
        assert torch.equal(spec['classes'][1], golden['best'][case.id]['classes'].to(F64)), case.id


# ------------------------------------------------------------------------------------------------ planted edges are present
def _retina_edge_case(smoothl1=0):
    return D._pick(D.RETINA_CASES, A=257, G=37, smoothl1=smoothl1)


def test_retina_planted_edges_are_in_the_inputs_and_decided_as_claimed():
    case = _retina_edge_case()
    inp = D.retina_inputs(case)
    spec, aux = D.retina_reference(case, inp)
    gt = inp['annots'][0]
    valid = gt[gt[:, 4] >= 0]
    want_iou = {'iou_half': 0.5, 'iou_one_tied_classes': 1.0, 'iou_two_fifths': D.T04, 'iou_zero_everywhere': 0.0, 'iou_third_tied_boxes': float(np.float32(1 / 3)),
                'iou_one': 1.0, 'beside_zero_area_box': 0.0}
    for j, (name, (anchor, cls, box)) in enumerate(D.RETINA_PLANTED.items()):
        assert inp['anchors'][j].tolist() == list(map(float, anchor)), name
        assert float(aux['best'][0, j]) == want_iou[name], (name, float(aux['best'][0, j]))
        assert float(spec['cls'][1][0, j]) == cls, name
        assert spec['box'][1][0, j].tolist() == list(map(float, box)), name
    # the exact rationals: 100 / 200 and 100 / 250
    assert D._iou_matrix(inp['anchors'][:3], valid)[0, 0] == 0.5 and D._iou_matrix(inp['anchors'][:3], valid)[2, 0] == 100.0 / 250.0
    # ties: two valid boxes of different class tied for best (the lower valid index wins), with and without a positive IoU
    assert float(aux['second'][0, 1]) == 1.0 and valid[0, 4] != valid[1, 4]
    assert float(aux['second'][0, 4]) == float(np.float32(1 / 3))
    assert float(aux['second'][0, 3]) == 0.0                       # zero against every box: class 0, box of the FIRST valid row
    assert bool(((valid[:, 2] - valid[:, 0]) * (valid[:, 3] - valid[:, 1]) == 0).any())           # a zero-area ground-truth box
    pad = (gt[:, 4] < 0).nonzero()[:, 0].tolist()
    assert pad[0] == 0 and pad[-1] == case.G - 1 and any(0 < p < case.G - 1 and gt[p - 1, 4] >= 0 and gt[p + 1, 4] >= 0 for p in pad)
    b3 = _retina_edge_case(1)
    i3 = D.retina_inputs(b3)
    assert b3.B == 3 and bool((i3['annots'][1][:, 4] < 0).all())   # an image of only padding rows
    s3, _ = D.retina_reference(b3, i3)
    assert bool((s3['cls'][1][1] == -1).all()) and bool((s3['box_xy'][1][1] == -1).all())
    g0 = D._pick(D.RETINA_CASES, A=257, G=0, smoothl1=0)
    i0 = D.retina_inputs(g0)
    assert i0['annots'] is None
    s0, _ = D.retina_reference(g0, i0)
    assert bool((s0['cls'][1] == -1).all()) and bool((s0['box'][1] == -1).all()) and float(s0['pos'][1]) == D.POS_PREFILL
    full = D._pick(D.RETINA_CASES, A=257, G=1024, smoothl1=0)
    assert bool((D.retina_inputs(full)['annots'][:, :, 4] >= 0).all())


def test_fcos_planted_edges_are_in_the_inputs_and_decided_as_claimed():
    for cs in (0, 1):
        case = D._pick(D.FCOS_CASES, P=257, G=37, center_sample=cs, ranges='default')
        inp = D.fcos_inputs(case)
        spec, _ = D.fcos_reference(case, inp)
        pts = inp['points']
        gt = inp['annots'][0]
        valid = gt[gt[:, 4] >= 0]
        for j, (name, (x, y, s, cls)) in enumerate(D.FCOS_PLANTED.items()):
            assert pts[j, :3].tolist() == [x, y, D.FCOS_STRIDES[s]], name
            if name == 'dist_at_radius' and not cs:
                cls = 4                                      # without centre sampling the box simply holds the point
            assert float(spec['cls'][1][0, j]) == cls, (cs, name, float(spec['cls'][1][0, j]))
            if name in D.FCOS_PLANTED_FAULT:                 # and the decision is the edge's: the fault it guards against flips it
                fault, flipped = D.FCOS_PLANTED_FAULT[name]
                if fault == 'radius_nonstrict' and not cs:
                    continue
                f, _ = D.fcos_reference(case, inp, fault=fault)
                assert float(f['cls'][1][0, j]) == flipped, (cs, name, float(f['cls'][1][0, j]))
        l = pts[:, 0, None] - valid[None, :, 0]
        r = valid[None, :, 2] - pts[:, 0, None]
        assert float(l[0, 0]) == 0 and float(r[1, 1]) == 0
        q = D.fcos_quantities(pts, valid, F64)
        assert float(q['dist'][2, 2]) == 12.0 == 8 * D.FCOS_RADIUS
        assert float(l[3, 3]) == 64 and float(l[4, 4]) == 64
        assert float(q['area'][0, 9]) == float(q['area'][0, 10]) == 400
        pad = (gt[:, 4] < 0).nonzero()[:, 0].tolist()
        assert pad[0] == 0 and pad[-1] == case.G - 1 and 8 in pad and gt[8].tolist() == list(map(float, D.FCOS_PADDING_BOX))
        kept, _ = D.fcos_reference(case, inp, fault='padding_kept')
        assert float(kept['ltrb'][1][0, 9, 0]) == 16 and float(spec['ltrb'][1][0, 9, 0]) == 0      # the point inside the padding row's box
    b3 = D._pick(D.FCOS_CASES, P=257, G=37, center_sample=1, ranges='default')
    assert b3.B == 3
    s3, _ = D.fcos_reference(b3, D.fcos_inputs(b3))
    assert bool((s3['cls'][1][1] == 0).all()) and bool((s3['ltrb'][1][1] == 0).all()) and bool((s3['ctr'][1][1] == 0).all())
    g0 = D._pick(D.FCOS_CASES, P=257, G=0, center_sample=1)
    s0, _ = D.fcos_reference(g0, D.fcos_inputs(g0))
    assert D.fcos_inputs(g0)['annots'] is None and bool((s0['cls'][1] == 0).all()) and bool((s0['ctr'][1] == 0).all())


def test_focal_planted_edges_are_in_the_inputs_and_decided_as_claimed():
    case = next(c for c in D.FOCAL_CASES if c.Al >= 12 and c.grad and c.off > 0)
    inp = D.focal_inputs(case)
    terms, grad, bound = D.focal_math(case, inp)
    lo32, hi32 = np.float32(D.LO), np.float32(D.HI)
    for j, (p, hot) in enumerate(D.FOCAL_PLANTED):
        col = j % case.C
        assert float(inp['probs'][0, j, col]) == p
        inside = D.LO <= p <= D.HI
        assert (float(grad[0, j, col]) != 0) == inside, j
        assert float(terms[0, j, col]) > 0, j                  # the loss is counted on either side of the clamp
    assert D.FOCAL_PLANTED[2][0] == float(np.nextafter(lo32, np.float32(0))) < D.LO and D.FOCAL_PLANTED[3][0] == float(np.nextafter(hi32, np.float32(1))) > D.HI
    cls = inp['targets'][0, case.off:case.off + 12, 4].tolist()
    assert {-1.0, 0.0, 1.0, float(case.C)} <= set(cls)
    assert bool((grad[0, 9] == 0).all()) and bool((terms[0, 9] == 0).all())
    assert {c.C for c in D.FOCAL_CASES} >= {1, 7, 80, 91} and {c.gamma for c in D.FOCAL_CASES} == set(D.GAMMAS)
    assert any(not c.grad for c in D.FOCAL_CASES) and any(c.off > 0 and c.At > c.Al for c in D.FOCAL_CASES)
    other = inp['targets'][:, :, 4]
    assert not torch.equal(other[:, :case.Al], other[:, case.off:case.off + case.Al])       # the other levels' rows carry other classes


def test_smoothl1_planted_edges_and_exactness():
    for case in D.SMOOTH_CASES:
        if not case.dyadic:
            continue
        inp = D.smooth_inputs(case)
        terms, grad, _ = D.smooth_math(case, inp)
        assert grad[0, 0].tolist() == [1.0, -1.0, 0.0, 0.5] and terms[0, 0].tolist() == [0.25, 0.25, 0.0, 0.0625], case.id
        if case.Al >= 3:
            assert inp['targets'][0, case.off + 1, 4] == -1 and inp['targets'][0, case.off + 2, 4] == 0
            assert bool((grad[0, 1:3] == 0).all())
        # every term a multiple of 1/64, the whole sum below 2^18: exact in fp32 in any order
        assert torch.equal(terms * 64, (terms * 64).round()) and float(terms.sum()) + D.SUM_PREFILL < 2 ** 18, case.id
        assert torch.equal(D.r32(grad), grad)
        t32, g32, _ = D.smooth_math(case, inp, wd=torch.float32)
        assert torch.equal(t32.double(), terms) and torch.equal(g32.double(), grad)
        if case.rows <= 70000:
            assert D.kernel_order_sum(t32.numpy().reshape(-1), D.SUM_PREFILL, 4) == float(terms.sum()) + D.SUM_PREFILL
    # the neutral fault: `>` at beta changes neither a term nor a gradient element (both branches agree at |d| == beta)
    case = next(c for c in D.SMOOTH_CASES if c.dyadic and c.rows == 3001)
    inp = D.smooth_inputs(case)
    a, b = D.smooth_math(case, inp), D.smooth_math(case, inp, fault='gt_at_beta')
    assert bool((((inp['reg'] - inp['targets'][:, case.off:case.off + case.Al, :4]).abs() == 0.5) & (inp['targets'][:, case.off:case.off + case.Al, 4:5] > 0)).any())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_best_class_planted_edges():
    for case in D.BEST_CASES:
        if case.Al < 3:
            continue
        inp = D.best_inputs(case)
        spec = D.best_reference(case, inp)
        p = inp['probs'][0]
        assert float(spec['classes'][1][0, 0]) == case.C // 3 and int((p[0] == p[0].max()).sum()) == (2 if case.C > 1 else 1)
        assert float(spec['classes'][1][0, 1]) == 0 and bool((p[1] == p[1, 0]).all())
        assert float(spec['classes'][1][0, 2]) == case.C - 1
        if case.C > 1:
            ties = (inp['probs'] == inp['probs'].max(2, keepdim=True)[0]).sum(2) > 1
            assert int(ties.sum()) > 3, case.id                 # ties beyond the planted ones


def test_detr_planted_edges_and_subgradients_against_autograd():
    """on the dyadic inputs float64 autograd over losses._giou makes the subgradient choices csrc/detloss.hip claims: the hand-written
    reverse mode (whose magnitudes are the gradient's bound) equals it to float64 rounding"""
    for case in D.DETR_CASES:
        inp = D.detr_inputs(case)
        for n in ('reg', 'gt'):
            x = inp[n][..., :4] * 64
            keep = torch.isfinite(x) & (inp[n][..., :4] > -0.99)
            if n == 'gt':
                assert torch.equal(x[keep], x[keep].round())
        auto, mine = D.detr_autograd(case, inp), D.detr_math(case, inp)
        for k in ('l1', 'iou', 'dreg'):
            scale = float(auto[k].abs().max()) + 1e-30
            assert float((auto[k] - mine[k]).abs().max()) <= 1e-13 * scale + 1e-15, (case.id, k)
        if case.T < 8:
            continue
        src = inp['src'][0, :8]
        g = mine['dreg'][0, 0, src]
        p = torch.clamp(inp['reg'][0, 0, src], case.lo, case.hi)
        t = inp['gt'][0, :8, :4]
        tape = D.giou_tape(p, t)
        names = {n: i for i, n in enumerate(D.DETR_PLANTED)}
        assert torch.equal(p[names['equal']], t[names['equal']])
        assert float(tape['iw'][names['disjoint']]) < 0 and float(tape['ih'][names['disjoint']]) < 0
        assert float(tape['iw'][names['touching']]) == 0 and float(tape['ih'][names['touching']]) > 0
        raw = inp['reg'][0, 0, src]
        assert float(raw[names['at_lo'], 2]) == float(np.float32(case.lo)) and float(raw[names['at_hi'], 0]) == float(np.float32(case.hi))
        assert float(raw[names['below_lo'], 2]) < float(np.float32(case.lo)) and float(raw[names['above_hi'], 0]) > float(np.float32(case.hi))
        if case.d_l1 or case.d_iou:
            assert float(g[names['at_lo'], 2]) != 0 and float(g[names['at_hi'], 0]) != 0
            assert float(g[names['below_lo'], 2]) == 0 and float(g[names['above_hi'], 0]) == 0
        if case.lo == 0.0:
            assert float(p[names['zero_size'], 2]) == 0 and float(p[names['zero_size'], 3]) == 0
        if case.B > 1:
            assert bool((inp['gt'][1, :, 4] < 0).all()) and bool((mine['dreg'][:, 1] == 0).all())       # an image without boxes
    assert any(not c.d_l1 for c in D.DETR_CASES) and any(not c.d_iou for c in D.DETR_CASES)
    assert {c.L for c in D.DETR_CASES} == {1, 6} and {c.B * c.T for c in D.DETR_CASES} == {1, 255, 256, 257, 513}


# ------------------------------------------------------------------------------------------------ exactness premises
@pytest.mark.parametrize('case', [c for c in D.RETINA_CASES if c.exact and c.G and c.A <= 257], ids=lambda c: c.id)
def test_retina_exact_inputs_are_exact_in_fp32(case):
    inp = D.retina_inputs(case)
    an = inp['anchors']
    assert torch.equal(an, an.round()) and float(an.abs().max()) < 2 ** 11
    for rows in inp['annots']:
        gt = rows[rows[:, 4] >= 0]
        if gt.shape[0] == 0:
            continue
        assert torch.equal(gt, gt.round())
        i64, i32 = D._iou_matrix(an, gt), D._iou_matrix(an, gt, torch.float32)
        assert torch.equal(D.r32(i64), i32.double())        # fp32 arithmetic IS the once-rounded float64 result
        area = (an[:, 2] - an[:, 0]) * (an[:, 3] - an[:, 1])
        assert float(area.max()) + float(((gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])).max()) < 2 ** 24


@pytest.mark.parametrize('case', [c for c in D.FCOS_CASES if c.exact and c.G and c.P <= 257], ids=lambda c: c.id)
def test_fcos_exact_inputs_are_exact_in_fp32(case):
    inp = D.fcos_inputs(case)
    assert float(inp['annots'][:, :, :4].max()) <= 256 and D.fcos_exactness(inp)
    a, _ = D.fcos_reference(case, inp)
    b, _ = D.fcos_reference(case, inp, wd=torch.float32)
    assert torch.equal(a['cls'][1], b['cls'][1]) and torch.equal(a['ltrb'][1], b['ltrb'][1])


# ------------------------------------------------------------------------------------------------ constants
def _measure():
    worst = {}
    for case in D.RETINA_CASES:
        if case.smoothl1 and case.G:
            inp = D.retina_inputs(case)
            spec, _ = D.retina_reference(case, inp)
            emu, _ = D.retina_reference(case, inp, emulate=True)
            D.judge(D.values(emu), {k: v for k, v in spec.items() if k.startswith('box_')}, worst)
    for case in D.FOCAL_CASES:
        inp = D.focal_inputs(case)
        spec = D.focal_reference(case, inp)
        D.judge(D.focal_emulate(case, inp), spec, worst)
        parts = D.workgroup_partials(D.focal_math(case, inp, wd=torch.float32)[0].numpy().reshape(-1))
        for seed in D.ORDER_SEEDS[1:]:
            D.judge(D.focal_emulate(case, inp, seed, parts), {'sum': spec['sum']}, worst)
    for case in D.SMOOTH_CASES:
        if not case.dyadic:
            inp = D.smooth_inputs(case)
            spec = D.smooth_reference(case, inp)
            D.judge(D.smooth_emulate(case, inp), spec, worst)
            parts = D.workgroup_partials(D.smooth_math(case, inp, wd=torch.float32)[0].numpy().reshape(-1), 4)
            for seed in D.ORDER_SEEDS[1:]:
                D.judge(D.smooth_emulate(case, inp, seed, parts), {'sum': spec['sum']}, worst)
    for case in D.DETR_CASES:
        inp = D.detr_inputs(case)
        spec = D.detr_reference(case, inp)
        D.judge(D.detr_emulate(case, inp), {k: v for k, v in spec.items() if v[0] == 'bound'}, worst)
    return worst


@pytest.fixture(scope='module')
def measured():
    """on one thread: the order of torch's fp32 element-wise kernels does not matter, but keep the measurement the same everywhere"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _measure()
    finally:
        torch.set_num_threads(threads)


def test_constants_table_is_what_the_emulations_measure(measured):
    """CONSTANTS is a record of this measurement, not a choice: a quarter of slack either way for another torch build"""
    lines = [f'{n:18} {measured.get(n, float("nan")):9.4g}  (stored {c:g})' for n, c in D.CONSTANTS.items()]
    print('\n'.join(lines))
    assert set(measured) == set(D.CONSTANTS)
    for n, c in D.CONSTANTS.items():
        assert math.isfinite(measured[n]) and c / 1.25 <= measured[n] <= c * 1.25, '\n' + '\n'.join(lines)


def test_emulations_pass_every_bound_with_the_margin(measured):
    for n, c in D.CONSTANTS.items():
        assert measured[n] <= D.MARGIN * c, (n, measured[n])


def test_four_correctly_rounded_operations_stay_within_three_units():
    """the derived bound of the centre-ness chain (divide, divide, multiply, square root): relative error (3 u) / 2 + u <= 3 u, met by an
    fp32 evaluation on random operands"""
    g = torch.Generator().manual_seed(5)
    l, r, t, b = (torch.rand(200000, generator=g) * 200 + 0.01 for _ in range(4))
    c32 = torch.sqrt((torch.minimum(l, r) / torch.maximum(l, r)) * (torch.minimum(t, b) / torch.maximum(t, b))).double()
    l, r, t, b = (v.double() for v in (l, r, t, b))
    c64 = torch.sqrt((torch.minimum(l, r) / torch.maximum(l, r)) * (torch.minimum(t, b) / torch.maximum(t, b)))
    assert float(((c32 - c64).abs() / c64).max()) <= D.FIXED['chain4'] * D.UF


# ------------------------------------------------------------------------------------------------ every fault makes a case miss
def _fault_misses(cases, inputs, reference, fault, pair=False):
    n = 0
    for case in cases:
        inp = inputs(case)
        true, bad = reference(case, inp), reference(case, inp, fault=fault)
        if pair:
            true, bad = true[0], bad[0]
        if bad.keys() != true.keys():
            n += 1
            continue
        n += bool(D.judge(D.values(bad), true))
    return n


@pytest.mark.parametrize('fault', D.RETINA_FAULTS)
def test_every_retina_fault_is_caught(fault):
    cases = [c for c in D.RETINA_CASES if c.A in (257,) or (c.A == 3001 and not c.exact and c.B == 1)]
    assert _fault_misses(cases, D.retina_inputs, D.retina_reference, fault, pair=True) >= 1


@pytest.mark.parametrize('fault', D.FCOS_FAULTS)
def test_every_fcos_fault_is_caught(fault):
    cases = [c for c in D.FCOS_CASES if c.P == 257]
    assert _fault_misses(cases, D.fcos_inputs, D.fcos_reference, fault, pair=True) >= 1


@pytest.mark.parametrize('fault', D.FOCAL_FAULTS)
def test_every_focal_fault_is_caught(fault):
    cases = [c for c in D.FOCAL_CASES if c.total <= 70000 or fault == 'remainder_dropped']
    assert _fault_misses(cases, D.focal_inputs, D.focal_reference, fault) >= 1


@pytest.mark.parametrize('fault', D.SMOOTHL1_FAULTS)
def test_every_smoothl1_fault_is_caught(fault):
    cases = [c for c in D.SMOOTH_CASES if c.rows <= 70000 or fault == 'remainder_dropped']
    assert _fault_misses(cases, D.smooth_inputs, D.smooth_reference, fault) >= 1
    if fault != 'remainder_dropped':                          # and by a dyadic case and an accuracy case alike
        for dy in (True, False):
            assert _fault_misses([c for c in cases if c.dyadic == dy and c.rows <= 70000], D.smooth_inputs, D.smooth_reference, fault) >= 1


@pytest.mark.parametrize('fault', D.BEST_FAULTS)
def test_every_best_class_fault_is_caught(fault):
    cases = [c for c in D.BEST_CASES if c.rows <= 70000 or fault == 'remainder_dropped']
    assert _fault_misses(cases, D.best_inputs, D.best_reference, fault) >= 1


@pytest.mark.parametrize('fault', D.DETR_FAULTS)
def test_every_detr_fault_is_caught(fault):
    assert _fault_misses([c for c in D.DETR_CASES if c.T >= 8], D.detr_inputs, D.detr_reference, fault) >= 1


# ------------------------------------------------------------------------------------------------ left-out shares
def test_left_out_shares_stay_within_the_cap_on_the_reference_alone():
    lines = []
    for table, inputs, reference, n in ((D.RETINA_CASES, D.retina_inputs, D.retina_reference, 'A'), (D.FCOS_CASES, D.fcos_inputs, D.fcos_reference, 'P')):
        for case in table:
            if case.exact:
                continue
            _, aux = reference(case, inputs(case))
            out, total = int(aux['left_out'].sum()), case.B * getattr(case, n)
            err = aux['iou_err'] if 'iou_err' in aux else max(aux['err'].values())
            lines.append(f'{case.id}: left out {out} of {total}, worst fp32 error of a deciding quantity {err:.2f} u')
            assert out <= D.LEFT_OUT_CAP * total, lines[-1]
            assert err < 64, lines[-1]
    print('\n'.join(lines))
    assert len(lines) >= 8


# ------------------------------------------------------------------------------------------------ the tables reach every form
def test_case_tables_reach_every_launch_form():
    cap = D.DL_GRID_CAP * D.DL_THREADS
    assert D.dl_grid(1) == 1 and D.dl_grid(256) == 1 and D.dl_grid(257) == 2 and D.dl_grid(cap) == 4096 and D.dl_grid(cap + 1) == 4096
    for kernel, items in D.looped_items().items():
        assert any(n > cap for n in items), kernel                # the grid-stride form
        assert any(n < D.DL_THREADS for n in items), kernel       # less than one block
        assert any(n % D.DL_THREADS for n in items if n > D.DL_THREADS), kernel
    assert any(c.total > cap and c.gamma == 2.0 for c in D.FOCAL_CASES) and any(c.total > cap and c.gamma != 2.0 for c in D.FOCAL_CASES)
    assert any(c.rows > cap and c.dyadic for c in D.SMOOTH_CASES) and any(c.rows > cap and not c.dyadic for c in D.SMOOTH_CASES)
    assert any(c.rows > cap and c.ctr for c in D.BEST_CASES) and any(c.rows > cap and not c.ctr for c in D.BEST_CASES)
    for table, n in ((D.RETINA_CASES, 'A'), (D.FCOS_CASES, 'P')):
        sizes, gs = {getattr(c, n) for c in table}, {c.G for c in table}
        assert sizes >= {1, 255, 256, 257, 3001} and gs == {0, 1, 37, D.DL_MAX_GT} and {c.B for c in table} == {1, 3}
    assert {c.smoothl1 for c in D.RETINA_CASES} == {0, 1} and {c.center_sample for c in D.FCOS_CASES} == {0, 1}
    assert {c.ranges for c in D.FCOS_CASES} == {'default', 'second'}
    assert {c.C for c in D.BEST_CASES} >= {1, 2, 80, 91} and any(c.off > 0 and c.At > c.Al for c in D.BEST_CASES)
    assert {round(c.beta, 6) for c in D.SMOOTH_CASES} == {0.5, round(1 / 9, 6)} and any(not c.grad for c in D.SMOOTH_CASES)
    assert {c.rows for c in D.SMOOTH_CASES} >= {1, 255, 257, 3001} and any(c.off > 0 for c in D.SMOOTH_CASES)
    ids = [c.id for t in (D.RETINA_CASES, D.FCOS_CASES, D.FOCAL_CASES, D.SMOOTH_CASES, D.BEST_CASES, D.DETR_CASES) for c in t]
    assert len(set(ids)) == len(ids)
