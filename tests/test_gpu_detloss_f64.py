"""Every C-ABI entry point of csrc/detloss.hip but saicv_detr_assign (held to scipy case by case in test_gpu_r05.py) against the float64
references of tests/detloss_common.py, at every launch form: less than a block, the block edges, a ragged tail, the grid-stride loop
beyond dl_grid()'s 4 096 workgroups, G = 0 (a null annotation pointer) to G = 1024 (LDS full), levels in the middle of the pyramid, the
atomic and the deterministic accumulation.  Exact-regime cases are compared with torch.equal, nothing left out; accuracy-regime cases
element by element against MARGIN * CONSTANTS * u * bound, nothing sampled.  Outputs live in guarded allocations pre-filled with NaN
(`+=` targets with a known value) and the guards are compared after every launch.  Reads tests/golden/detloss_edges.pt and
detloss_common only."""
import functools
import os

import pytest
import torch

import detloss_common as D
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
F64 = torch.float64
ids = lambda c: c.id      # noqa: E731


@functools.lru_cache(maxsize=None)
def _retina(case):
    inp = D.retina_inputs(case)
    return inp, D.retina_reference(case, inp)


@functools.lru_cache(maxsize=None)
def _fcos(case):
    inp = D.fcos_inputs(case)
    return inp, D.fcos_reference(case, inp)


@functools.lru_cache(maxsize=None)
def _focal(case):
    inp = D.focal_inputs(case)
    return inp, D.focal_reference(case, inp)


@functools.lru_cache(maxsize=None)
def _smooth(case):
    inp = D.smooth_inputs(case)
    return inp, D.smooth_reference(case, inp)


def _show(case, got, spec):
    worst = {}
    bad = D.judge(got, spec, worst)
    if worst:
        print(case.id, ' '.join(f'{q}={r:.3g} (allowed {D.FIXED.get(q, D.MARGIN * D.CONSTANTS.get(q, 0)):.3g})' for q, r in worst.items()))
    return bad


def _mode(request, mode):
    if mode == 'deterministic':
        request.getfixturevalue('deterministic')


# ------------------------------------------------------------------------------------------------ the assignments
@pytest.mark.parametrize('case', D.RETINA_CASES, ids=ids)
def test_retina_assign(case):
    inp, (spec, aux) = _retina(case)
    got, guards = D.run_retina_assign(case, inp)
    assert not guards, guards
    if not case.exact:
        assert int(aux['left_out'].sum()) <= D.LEFT_OUT_CAP * case.A * case.B
    assert not _show(case, got, spec)


def test_retina_assign_agrees_with_the_reference_project_on_the_edges():
    gold = torch.load(os.path.join(GOLDEN, 'detloss_edges.pt'), weights_only=True)['retina']
    for case in D.edge_cases()['retina']:
        got, guards = D.run_retina_assign(case, _retina(case)[0])
        assert not guards
        assert torch.equal(got['cls'], gold[case.id]['cls'].to(F64)) and float(got['pos']) == gold[case.id]['pos'] + D.POS_PREFILL, case.id
        if not case.smoothl1:
            assert torch.equal(got['box'], gold[case.id]['box'].to(F64)), case.id


@pytest.mark.parametrize('entry', ['retina_assign', 'fcos_assign'])
def test_more_rows_than_lds_holds_are_refused_without_a_launch(entry):
    from simpleaicv_pytorch_training_examples_amd import _lib
    L = _lib.lib()
    G = D.DL_MAX_GT + 1
    tab = torch.zeros(8, 5, device='cuda')
    ann = torch.zeros(1, G, 5, device='cuda')
    g_t = D.Guarded((1, 8, 5), (40, 5, 1), torch.float32, 'cuda')
    g_c = D.Guarded((1, 8), (8, 1), torch.float32, 'cuda')
    pos = torch.full((1,), D.POS_PREFILL, device='cuda')
    if entry == 'retina_assign':
        rc = L.saicv_retina_assign(_lib.ptr(tab), _lib.ptr(ann), _lib.ptr(g_t.view), _lib.ptr(pos), 1, 8, G, 0, _lib.stream())
    else:
        rc = L.saicv_fcos_assign(_lib.ptr(tab), _lib.ptr(ann), _lib.ptr(g_t.view), _lib.ptr(g_c.view), _lib.ptr(pos), 1, 8, G, 1.5, 1, _lib.stream())
    torch.cuda.synchronize()
    assert rc != 0
    msg = L.saicv_last_error_string().decode()
    assert entry in msg and str(G) in msg, msg
    with pytest.raises(RuntimeError, match=entry):
        _lib.check(rc, entry)
    assert bool(torch.isnan(g_t.view).all()) and bool(torch.isnan(g_c.view).all()) and float(pos) == D.POS_PREFILL     # nothing ran


@pytest.mark.parametrize('case', D.FCOS_CASES, ids=ids)
def test_fcos_assign(case):
    inp, (spec, aux) = _fcos(case)
    got, guards = D.run_fcos_assign(case, inp)
    assert not guards, guards
    if not case.exact:
        assert int(aux['left_out'].sum()) <= D.LEFT_OUT_CAP * case.P * case.B
    assert not _show(case, got, spec)


def test_fcos_assign_agrees_with_the_reference_project_on_the_edges():
    gold = torch.load(os.path.join(GOLDEN, 'detloss_edges.pt'), weights_only=True)['fcos']
    for case in D.edge_cases()['fcos']:
        got, guards = D.run_fcos_assign(case, _fcos(case)[0])
        assert not guards
        assert torch.equal(got['cls'], gold[case.id]['cls'].to(F64)) and torch.equal(got['ltrb'], gold[case.id]['ltrb'].to(F64)), case.id
        assert float(got['pos']) == gold[case.id]['pos'] + D.POS_PREFILL


# ------------------------------------------------------------------------------------------------ the level losses
@pytest.mark.parametrize('mode', ['atomic', 'deterministic'])
@pytest.mark.parametrize('case', D.FOCAL_CASES, ids=ids)
def test_focal_loss_level(case, mode, request):
    _mode(request, mode)
    inp, spec = _focal(case)
    got, guards = D.run_focal(case, inp)
    assert not guards, guards
    assert not _show(case, got, spec)
    if mode == 'deterministic':
        again, _ = D.run_focal(case, inp)
        assert all(torch.equal(again[k], got[k]) for k in got)


@pytest.mark.parametrize('mode', ['atomic', 'deterministic'])
@pytest.mark.parametrize('case', D.SMOOTH_CASES, ids=ids)
def test_smoothl1_level(case, mode, request):
    _mode(request, mode)
    inp, spec = _smooth(case)
    got, guards = D.run_smoothl1(case, inp)
    assert not guards, guards
    assert not _show(case, got, spec)
    if mode == 'deterministic':
        again, _ = D.run_smoothl1(case, inp)
        assert all(torch.equal(again[k], got[k]) for k in got)


# ------------------------------------------------------------------------------------------------ the decoder's best class
@pytest.mark.parametrize('case', D.BEST_CASES, ids=ids)
def test_det_best_class(case):
    inp = D.best_inputs(case)
    got, guards = D.run_best_class(case, inp)
    assert not guards, guards                                   # the other levels' slots of scores / classes keep their sentinel
    assert not _show(case, got, D.best_reference(case, inp))


def test_det_best_class_agrees_with_numpys_argmax_on_the_edges():
    gold = torch.load(os.path.join(GOLDEN, 'detloss_edges.pt'), weights_only=True)['best']
    for case in D.edge_cases()['best']:
        got, _ = D.run_best_class(case, D.best_inputs(case))
        assert torch.equal(got['classes'], gold[case.id]['classes'].to(F64)), case.id


# ------------------------------------------------------------------------------------------------ DETR box losses
@pytest.mark.parametrize('case', D.DETR_CASES, ids=ids)
def test_detr_box_loss(case):
    inp = D.detr_inputs(case)
    got, guards = D.run_detr(case, inp)
    assert not guards, guards
    assert not _show(case, got, D.detr_reference(case, inp))


# ------------------------------------------------------------------------------------------------ through the modules: no positives at all
SIZES = [(16, 20), (8, 10), (4, 5), (2, 3), (1, 2)]


def _heads(shape_tail, gen):
    return [(torch.rand(2, h, w, *shape_tail, generator=gen) * 0.9 + 0.05).cuda().requires_grad_(True) for h, w in SIZES]


def _assert_zero(losses, leaves):
    for name, v in losses.items():
        assert float(v.detach()) == 0.0, (name, float(v.detach()))
    total = sum(losses.values())
    grads = torch.autograd.grad(total, leaves, allow_unused=True) if total.requires_grad else [None] * len(leaves)
    for i, g in enumerate(grads):        # a head no loss term reaches has no gradient at all: that is a zero, too
        assert g is None or (bool(torch.isfinite(g).all()) and bool((g == 0).all())), i


@pytest.mark.parametrize('annots', ['no_rows', 'only_padding'])
@pytest.mark.parametrize('box_loss_type', ['SmoothL1', 'GIoU'])
def test_retina_loss_without_any_box_is_exactly_zero(box_loss_type, annots):
    """the inv = 0 path: the reference returns 0 when no anchor is positive"""
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.detection.losses import RetinaLoss
    gen = torch.Generator().manual_seed(3)
    cls, reg = _heads((9, 8), gen), _heads((9, 4), gen)
    ann = torch.zeros(2, 0, 5) if annots == 'no_rows' else torch.full((2, 6, 5), -1.0)
    _assert_zero(RetinaLoss(box_loss_type=box_loss_type)([cls, reg], ann.cuda()), cls + reg)


@pytest.mark.parametrize('annots', ['no_rows', 'only_padding'])
def test_fcos_loss_without_any_box_is_exactly_zero(annots):
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.detection.losses import FCOSLoss
    gen = torch.Generator().manual_seed(4)
    cls, reg, ctr = _heads((8,), gen), _heads((4,), gen), _heads((1,), gen)
    ann = torch.zeros(2, 0, 5) if annots == 'no_rows' else torch.full((2, 6, 5), -1.0)
    _assert_zero(FCOSLoss()([cls, reg, ctr], ann.cuda()), cls + reg + ctr)
