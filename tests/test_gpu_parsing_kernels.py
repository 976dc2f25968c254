"""The parsing loss kernel (csrc/parsing.hip, ops.pixel_class_terms) against its float64 judge (tests/parsing_common.py).

Class counts 2, 19, 20, 32 (lane-per-row form), 33, 64, 65, 151 (wavefront-per-row form; one to three classes per lane); 3 rows
(less than one tile of either form, scalar tail of the span copy) and 700 (whole tiles plus a partial one in both forms); fp32
and bf16 logits; softmax and sigmoid; dL/dterms = (1.25, 0, -0.75).  tests/test_parsing_host.py asserts on the same list that
no element lies within relative 1e-3 of a clamp bound and that every target regime and both clamp states are populated, so the
judge's element masks are the kernel's without exception.  Bounds (those of tests/test_gpu_semseg_kernels.py): each term
|got - ref| <= 1e-5 max(1, |ref|); fp32 gradient rel_err < 1e-5; bf16 gradient per element |g - g64| <= 2^-8 |g64| + 1e-5 max|g64|
against the judge on the same bf16 values; exactly 0 where the judge's gradient is exactly 0.

Measured on one MI355X, worst ratio to each bound over the 64 cases of test_terms_and_gradient_against_float64:
terms 0.017 (fp32 logits) / 0.023 (bf16 logits), fp32 gradient 0.046, bf16 gradient 0.99 (the bf16 bound is one rounding to nearest
of the stored gradient: 2^-8 relative is half a step at the bottom of a binade, so a correct kernel sits just below it)."""
import pytest
import torch

import parsing_common as P
from conftest import rel_err

pytestmark = pytest.mark.gpu


def _ops():
    from simpleaicv_pytorch_training_examples_amd import ops
    return ops


def _losses():
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.human_parsing import losses
    return losses


def _run(x, label, logit_type, g=P.KERNEL_G, form='auto'):
    ops = _ops()
    xd = x.cuda().requires_grad_(True)
    terms = ops.pixel_class_terms(xd, label.cuda(), logit_type, form)
    (terms * torch.tensor(g, device='cuda')).sum().backward()
    return terms.detach(), xd.grad


def _check(terms, grad, j, dtype):
    """-> the worst ratios (terms, gradient) to their bounds, after asserting them"""
    assert terms.dtype == torch.float32 and terms.shape == (3,) and grad.dtype == dtype and grad.shape == j['grad'].shape
    ref_t = j['terms']
    ratios = [abs(float(terms[k]) - float(ref_t[k])) / (1e-5 * max(1.0, abs(float(ref_t[k])))) for k in range(3)]
    got, ref = grad.double().cpu(), j['grad']
    if dtype == torch.float32:
        gratio = rel_err(got, ref) / 1e-5
    else:
        bound = 2. ** -8 * ref.abs() + 1e-5 * float(ref.abs().max())
        gratio = float(((got - ref).abs() / bound).max())
    print('ratio to bound', str(dtype).replace('torch.', ''), 'terms', ['%.3g' % v for v in ratios], 'gradient %.3g' % gratio)
    assert max(ratios) <= 1.0
    zero = ref == 0
    assert float(got[zero].abs().max() if bool(zero.any()) else 0.0) == 0.0       # exactly zero where the judge is
    assert gratio < 1.0 if dtype == torch.float32 else gratio <= 1.0
    return max(ratios), gratio


@pytest.mark.parametrize('logit_type', P.LOGIT_TYPES)
@pytest.mark.parametrize('dtype', P.KERNEL_DTYPES)
@pytest.mark.parametrize('rows', P.KERNEL_ROWS)
@pytest.mark.parametrize('C', P.KERNEL_CLASSES)
def test_terms_and_gradient_against_float64(C, rows, dtype, logit_type):
    x, label = P.class_terms_inputs(rows, C, P.case_seed(C, rows, logit_type), dtype, logit_type)
    j = P.class_terms_judge(x, label, logit_type, P.KERNEL_G)
    assert int(j['near'].sum()) == 0
    terms, grad = _run(x, label, logit_type)
    _check(terms, grad, j, dtype)


@pytest.mark.parametrize('logit_type', P.LOGIT_TYPES)
@pytest.mark.parametrize('C', [19, 20, 32])
def test_both_row_mappings_at_small_class_counts(C, logit_type):
    """the wavefront-per-row form also serves the counts the lane-per-row form takes by default: either side of a moved boundary"""
    x, label = P.class_terms_inputs(700, C, P.case_seed(C, 700, logit_type), torch.bfloat16, logit_type)
    j = P.class_terms_judge(x, label, logit_type, P.KERNEL_G)
    for form in ('lane', 'wave'):
        terms, grad = _run(x, label, logit_type, form=form)
        _check(terms, grad, j, torch.bfloat16)


@pytest.mark.parametrize('logit_type', P.LOGIT_TYPES)
@pytest.mark.parametrize('C', [20, 81])
def test_labels_outside_the_classes(C, logit_type):
    rows = 70
    x, label = P.class_terms_inputs(rows, C, seed=5, logit_type=logit_type)
    label[0], label[1], label[40] = -1., float(C), float(C + 3)
    j = P.class_terms_judge(x, label, logit_type, P.KERNEL_G)
    assert int((~j['valid']).sum()) == 3
    terms, grad = _run(x, label, logit_type)
    _check(terms, grad, j, torch.float32)
    assert float(grad[[0, 1, 40]].abs().max()) == 0.0
    kept = torch.ones(rows, dtype=torch.bool)
    kept[[0, 1, 40]] = False
    # the ignored rows add nothing and still count in the means: the kept rows alone give the same sums
    alone, _ = _run(x[kept], label[kept], logit_type)
    for k in range(3):
        assert abs(float(terms[k]) * rows - float(alone[k]) * (rows - 3)) < 1e-5 * rows * max(1.0, abs(float(j['terms'][k])))


@pytest.mark.parametrize('C', [20, 65])
def test_the_prediction_layouts_are_bit_equal(C):
    """[B, C, H, W] over NHWC memory (what pred_conv produces: used as it is), NCHW-contiguous (copied once), and the [rows, C] view"""
    ops = _ops()
    B, H, W = 2, 5, 6
    x, label = P.class_terms_inputs(B * H * W, C, seed=4)
    g = torch.tensor(P.KERNEL_G, device='cuda')
    ref, gref = _run(x, label, 'softmax')
    for src in (x.view(B, H, W, C).permute(0, 3, 1, 2), x.view(B, H, W, C).permute(0, 3, 1, 2).contiguous()):
        leaf = src.cuda().requires_grad_(True)
        assert leaf.stride() == src.stride()
        terms = ops.pixel_class_terms(leaf, label.view(B, H, W).cuda())
        (terms * g).sum().backward()
        assert torch.equal(terms, ref) and leaf.grad.shape == (B, C, H, W)
        assert torch.equal(leaf.grad.permute(0, 2, 3, 1).reshape(-1, C), gref)


@pytest.mark.parametrize('logit_type', P.LOGIT_TYPES)
def test_upstream_scales_the_gradient_exactly(logit_type):
    x, label = P.class_terms_inputs(100, 20, seed=9, logit_type=logit_type)
    _, g1 = _run(x, label, logit_type)
    _, g4 = _run(x, label, logit_type, g=tuple(4.0 * v for v in P.KERNEL_G))
    # a power of two: exact wherever the smaller gradient is a normal fp32 number.  A subnormal result (a_j down to e^-100 in the
    # widest rows) was rounded to a multiple of 2^-149, and four times it need not be the rounding of the four times larger value:
    # there the two may differ by that one rounding, scaled
    normal = g1.abs() >= 2. ** -126
    assert bool(normal.any()) and torch.equal(g4[normal], g1[normal] * 4.0)
    assert float((g4.double() - 4.0 * g1.double()).abs().max()) <= 4.0 * 2. ** -149


@pytest.mark.parametrize('dtype', P.KERNEL_DTYPES)
@pytest.mark.parametrize('C', [20, 151])
def test_results_repeat_bit_for_bit(C, dtype):
    ops = _ops()
    x, label = P.class_terms_inputs(700, C, seed=2, dtype=dtype)
    runs = []
    for det in (False, True, False):
        prev = ops.set_deterministic(det)
        try:
            runs.append(_run(x, label, 'softmax'))
        finally:
            ops.set_deterministic(prev)
    for terms, grad in runs[1:]:
        assert torch.equal(terms, runs[0][0]) and torch.equal(grad, runs[0][1])


def test_losses_over_one_prediction_share_both_passes():
    ops, L = _ops(), _losses()
    B, C, H, W = 2, 20, 6, 7
    x, label = P.class_terms_inputs(B * H * W, C, seed=3)
    pred = x.view(B, H, W, C).permute(0, 3, 1, 2).cuda().requires_grad_(True)
    lab = label.view(B, H, W).cuda()
    first = ops.pixel_class_terms(pred, lab, 'softmax')
    assert ops.pixel_class_terms(pred, lab, 'softmax') is first
    ce, iou = L.CELoss()(pred, lab), L.IoULoss('softmax')(pred, lab)
    assert ce._base is first and iou._base is first
    (ce + iou).backward()
    j = P.class_terms_judge(x, label, 'softmax', (1., 1., 0.))
    assert rel_err(pred.grad.permute(0, 2, 3, 1).reshape(-1, C), j['grad']) < 1e-5
    assert abs(float(ce) - float(j['terms'][0])) <= 1e-5 * max(1.0, abs(float(j['terms'][0])))
    assert abs(float(iou) - float(j['terms'][1])) <= 1e-5
    # another logit type, another label object, or a changed prediction: a pass of their own
    assert ops.pixel_class_terms(pred, lab, 'sigmoid') is not first
    again = ops.pixel_class_terms(pred, lab, 'softmax')
    assert again is not first and torch.equal(again, first)          # (only the last call is remembered)
    other = ops.pixel_class_terms(pred, lab.clone(), 'softmax')
    assert other is not again
    with torch.no_grad():
        p2 = pred.detach()
        a = ops.pixel_class_terms(p2, lab, 'softmax')
        assert ops.pixel_class_terms(p2, lab, 'softmax') is a
        p2.add_(1.0)                                                 # bumps _version
        assert ops.pixel_class_terms(p2, lab, 'softmax') is not a


@pytest.mark.parametrize('logit_type', P.LOGIT_TYPES)
@pytest.mark.parametrize('dtype', P.KERNEL_DTYPES)
def test_composed_route_agrees_with_the_fused_one(dtype, logit_type):
    """Each loss on its own, both routes, against the judge with dL/dterms = e_k.  One loss per backward because the bf16 bound
    allows ONE rounding of the gradient to bf16: the composed route hands autograd one bf16 gradient per loss and autograd adds
    them in bf16, so the sum of three composed losses carries five roundings where the fused route has one (measured 1.5 to 1.8
    times the bound on these inputs; the fp32 sum of all three is within 0.04 of its bound on both routes)."""
    L = _losses()
    B, C, H, W = 2, 20, 9, 11
    x, label = P.class_terms_inputs(B * H * W, C, seed=6, dtype=dtype, logit_type=logit_type)
    lab = label.view(B, H, W).cuda()
    first = L.CELoss() if logit_type == 'softmax' else L.MultiClassBCELoss()
    for k, loss in enumerate((first, L.IoULoss(logit_type), L.DiceLoss(logit_type))):
        g = tuple(1. if i == k else 0. for i in range(3))
        j = P.class_terms_judge(x, label, logit_type, g)
        for route in ('fused', 'composed'):
            loss.route = route
            pred = x.view(B, H, W, C).permute(0, 3, 1, 2).cuda().requires_grad_(True)
            value = loss(pred, lab)
            value.backward()
            print(type(loss).__name__, route)
            terms = j['terms'].clone().float()
            terms[k] = value.detach().float().cpu()
            _check(terms, pred.grad.permute(0, 2, 3, 1).reshape(-1, C), j, dtype)


def test_rejects_too_many_classes_and_cpu_tensors():
    ops = _ops()
    with pytest.raises(RuntimeError, match='257 classes'):
        ops.pixel_class_terms(torch.zeros(4, 257, device='cuda'), torch.zeros(4, device='cuda'))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.pixel_class_terms(torch.zeros(4, 5), torch.zeros(4))
