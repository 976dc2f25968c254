"""The two salient-object-detection kernels (csrc/salient.hip) against their float64 judges (tests/salient_common.py, themselves
pinned to the reference by tests/test_salient_host.py).  The kernels are called through the C-ABI on buffers that are NaN-filled and
fenced by guard elements, and through ops for the autograd surface and the sharing of one statistics pass between losses.

Tolerances.  Head, random operands: TOL of tests/test_gpu_kernels.py (fp32 1e-4, bf16 2e-2, relative to the tensor's scale); integer
operands: bit-exact (every sum is an integer below 2^24).  Statistics: 1e-5 of the sum of the terms' magnitudes, per statistic and
per gradient element -- the project's loss bound; a handful of fp32 roundings per term and a tree sum sit two orders below it.
Measured worst ratios to those bounds are printed by the tests and recorded in DESIGN.md section 3n."""
import numpy as np
import pytest
import torch

import salient_common as S
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-4, torch.bfloat16: 2e-2}
GUARD, FENCE = 64, 12288.0            # (exact in bf16)


def _ops():
    from simpleaicv_pytorch_training_examples_amd import _lib, ops
    return ops, _lib


def _fenced(shape, dtype):
    """-> (flat buffer, view): the view is NaN, GUARD elements of FENCE lie on either side of it"""
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), FENCE, dtype=dtype, device='cuda')
    flat[GUARD:GUARD + n] = float('nan')
    return flat, flat[GUARD:GUARD + n].view(*shape)


def _check_fence(flat, name):
    assert bool((flat[:GUARD] == FENCE).all()) and bool((flat[-GUARD:] == FENCE).all()), f'{name}: guard elements were written'
    assert not bool(torch.isnan(flat).any()), f'{name}: an element was left unwritten'


# ------------------------------------------------------------------------------------------------ head
HEAD_HW = [(1, 1), (3, 5), (17, 33), (64, 96)]
HEAD_C = [8, 32, 64]


def _head_call(x, w, b, dout, sigmoid):
    """one forward and one backward through the C-ABI on fenced buffers -> out [N, 1, H, W], dx (NCHW view), dw, db"""
    ops, _lib = _ops()
    L, st = _lib.lib(), _lib.stream()
    N, C, H, W = x.shape
    xd = x.cuda()
    assert xd.permute(0, 2, 3, 1).is_contiguous()
    wd, bd, dd = w.cuda(), b.cuda(), dout.cuda().contiguous()
    code = _lib.dtype_code(x.dtype)
    fo, out = _fenced((N, H, W), torch.float32)
    _lib.check(L.saicv_conv3x3_c1_fwd(code, xd.data_ptr(), wd.data_ptr(), 9, 1, bd.data_ptr(), out.data_ptr(), N, H, W, C,
                                      int(sigmoid), st), 'conv3x3_c1_fwd')
    fx_, dx = _fenced((N, H, W, C), x.dtype)
    fw, dw = _fenced((1, C, 3, 3), torch.float32)
    fb, db = _fenced((1,), torch.float32)
    fs, ws = _fenced((L.saicv_conv3x3_c1_ws_floats(N, H, W, C),), torch.float32)
    _lib.check(L.saicv_conv3x3_c1_bwd(code, xd.data_ptr(), wd.data_ptr(), 9, 1, out.data_ptr(), dd.data_ptr(), dx.data_ptr(),
                                      dw.data_ptr(), db.data_ptr(), ws.data_ptr(), N, H, W, C, int(sigmoid), 0, st), 'conv3x3_c1_bwd')
    torch.cuda.synchronize()
    for flat, name in ((fo, 'out'), (fx_, 'dx'), (fw, 'dw'), (fb, 'db'), (fs, 'workspace')):
        _check_fence(flat, name)
    return out.view(N, 1, H, W).cpu(), dx.permute(0, 3, 1, 2).float().cpu(), dw.cpu(), db.cpu()


@pytest.fixture(scope='module')
def head_refs():
    """float64 judge results, computed once per (shape, dtype, integer, sigmoid) and left unchanged"""
    cache = {}

    def get(N, C, H, W, dtype, integer, sigmoid):
        key = (N, C, H, W, dtype, integer, sigmoid)
        if key not in cache:
            operands = S.head_operands(N, C, H, W, seed=H * 100 + C, integer=integer, dtype=dtype)
            cache[key] = (operands, S.head_judge(*operands, sigmoid))
        return cache[key]
    return get


@pytest.mark.parametrize('det', [False, True])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('C', HEAD_C)
@pytest.mark.parametrize('hw', HEAD_HW)
def test_head_integer_operands_are_bit_exact(head_refs, hw, C, dtype, det):
    ops, _ = _ops()
    (x, w, b, dout), j = head_refs(2, C, hw[0], hw[1], dtype, True, False)
    prev = ops.set_deterministic(det)
    try:
        out, dx, dw, db = _head_call(x, w, b, dout, False)
    finally:
        ops.set_deterministic(prev)
    assert torch.equal(out.double(), j['out']) and torch.equal(dx.double(), j['dx'])
    assert torch.equal(dw.double(), j['dw']) and torch.equal(db.double(), j['db'])


@pytest.mark.parametrize('sigmoid', [True, False])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('C', HEAD_C)
@pytest.mark.parametrize('hw', HEAD_HW)
def test_head_random_operands_match_float64_and_repeat_bit_for_bit(head_refs, hw, C, dtype, sigmoid):
    (x, w, b, dout), j = head_refs(2, C, hw[0], hw[1], dtype, False, sigmoid)
    first = _head_call(x, w, b, dout, sigmoid)
    errs = {k: rel_err(got, j[k]) for k, got in zip(('out', 'dx', 'dw', 'db'), first)}
    print('head', hw, C, dtype, 'sigmoid' if sigmoid else 'logit', errs)
    for k, e in errs.items():
        assert e < TOL[dtype], (k, e)
    second = _head_call(x, w, b, dout, sigmoid)
    for a, c in zip(first, second):
        assert torch.equal(a, c)


@pytest.mark.parametrize('channels_last_weight', [False, True])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_ops_conv3x3_c1_autograd_surface(head_refs, dtype, channels_last_weight):
    """through ops: NCHW-shaped NHWC input, fp32 [N, 1, H, W] output, gradients for input, weight and bias; a channels-last
    weight is read in place through its strides"""
    ops, _ = _ops()
    (x, w, b, dout), j = head_refs(2, 32, 17, 33, dtype, False, True)
    xd = x.cuda().requires_grad_(True)
    wd = w.cuda().contiguous(memory_format=torch.channels_last) if channels_last_weight else w.cuda()
    wd, bd = wd.requires_grad_(True), b.cuda().requires_grad_(True)
    out = ops.conv3x3_c1(xd, wd, bd, sigmoid=True)
    assert out.dtype == torch.float32 and tuple(out.shape) == (2, 1, 17, 33) and out.is_contiguous()
    out.backward(dout.cuda())
    assert xd.grad.dtype == dtype and wd.grad.dtype == torch.float32 and wd.grad.shape == wd.shape
    for got, k in ((out, 'out'), (xd.grad, 'dx'), (wd.grad, 'dw'), (bd.grad, 'db')):
        assert rel_err(got.float().cpu(), j[k]) < TOL[dtype], k
    with pytest.raises(ValueError):
        ops.conv3x3_c1(torch.zeros(1, 20, 4, 4, device='cuda'), torch.zeros(1, 20, 3, 3, device='cuda'), bd)


# ------------------------------------------------------------------------------------------------ mask statistics
STATS_CASES = S.LOSS_CASES + [(2, 1048583)]


def _stats_call(p, label, g):
    ops, _lib = _ops()
    L, st = _lib.lib(), _lib.stream()
    B, P = p.shape
    pd, ld, gd = p.cuda().contiguous(), label.cuda().contiguous(), g.float().cuda().contiguous()
    fs, stats = _fenced((B, 4), torch.float32)
    fp_, part = _fenced((L.saicv_binary_seg_stats_ws_floats(B, P),), torch.float32)
    _lib.check(L.saicv_binary_seg_stats_fwd(pd.data_ptr(), ld.data_ptr(), B, P, part.data_ptr(), stats.data_ptr(), st), 'stats_fwd')
    fd, dp = _fenced((B, P), torch.float32)
    _lib.check(L.saicv_binary_seg_stats_bwd(pd.data_ptr(), ld.data_ptr(), gd.data_ptr(), B, P, dp.data_ptr(), st), 'stats_bwd')
    torch.cuda.synchronize()
    for flat, name in ((fs, 'stats'), (fp_, 'workspace'), (fd, 'dprob')):
        _check_fence(flat, name)
    return stats.cpu(), dp.cpu()


def _upstream(B):
    return torch.randn(B, 4, generator=torch.Generator().manual_seed(B)) * torch.tensor([1., 0.5, 7., 2.])


@pytest.mark.parametrize('det', [False, True])
@pytest.mark.parametrize('case', S.LOSS_CASES)
def test_stats_exact_operands_are_bit_exact(case, det):
    """p in {k / 64}, label in {0, 1/4, 1/2, 1}: sum ph, sum l and sum ph * l are multiples of 2^-8 below 2^14 (P <= 9100), exact in
    fp32 in any order; the bce sum is held to its bound"""
    ops, _ = _ops()
    B, P = case
    gen = torch.Generator().manual_seed(P)
    p = torch.randint(1, 64, (B, P), generator=gen).float() / 64.
    label = torch.tensor([0., 0.25, 0.5, 1.])[torch.randint(0, 4, (B, P), generator=gen)]
    g = _upstream(B)
    j = S.stats_judge(p, label, g)
    assert bool(j['inside'].all())
    prev = ops.set_deterministic(det)
    try:
        stats, dp = _stats_call(p, label, g)
        again, dp2 = _stats_call(p, label, g)
    finally:
        ops.set_deterministic(prev)
    assert torch.equal(stats[:, 1:].double(), j['stats'][:, 1:])
    assert bool(((stats[:, 0].double() - j['stats'][:, 0]).abs() <= 1e-5 * j['mag'][:, 0]).all())
    assert torch.equal(stats, again) and torch.equal(dp, dp2)


@pytest.mark.parametrize('det', [False, True])
@pytest.mark.parametrize('case', S.ORDER_CASES)
def test_stats_sums_follow_the_stated_order_bit_for_bit(case, det):
    """sum clamp(p) and sum label are pure fp32 additions: the kernel's bits equal the NumPy emulation of the ordered sum
    (S.ordered_stats_emulation; tests/test_salient_host.py shows that a sequential sum gives other bits at these sizes)"""
    ops, _ = _ops()
    B, P = case
    p, label = S.order_inputs(B, P)
    want = torch.from_numpy(S.ordered_stats_emulation(p, label))
    prev = ops.set_deterministic(det)
    try:
        stats, _ = _stats_call(p, label, _upstream(B))
    finally:
        ops.set_deterministic(prev)
    assert torch.equal(stats[:, 1:3], want), (stats[:, 1:3], want)


@pytest.mark.parametrize('case', STATS_CASES)
def test_stats_regimes_and_gradient_bounds(case):
    B, P = case
    p, label = (S.loss_inputs(B, P) if case in S.LOSS_CASES else
                (lambda gen: (torch.sigmoid(6. * torch.randn(B, P, generator=gen)), torch.rand(B, P, generator=gen)))(
                    torch.Generator().manual_seed(P)))
    lo, hi = np.float32(S.LO), np.float32(S.HI)
    if P >= 4099:                 # a few elements exactly at the bounds, one step outside each, and at 0 and 1
        planted = torch.tensor([lo, hi, np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(1)), 0., 1.], dtype=torch.float32)
        p[:, 100:106] = planted
        p[-1, P - 6:] = planted
    g = _upstream(B)
    j = S.stats_judge(p, label, g)
    if P >= 4099:
        # (7 elements cannot hold 5 % of anything: the regime fractions are asserted where the sample is large enough to have them)
        for name in ('below', 'above'):
            frac = float(j[name].float().mean())
            assert 0.05 <= frac, (name, frac)
        assert float(j['inside'].float().mean()) >= 0.5
        assert j['inside'][0, 100] and j['inside'][0, 101] and not j['inside'][0, 102:106].any()
    stats, dp = _stats_call(p, label, g)
    ratio = ((stats.double() - j['stats']).abs() / (1e-5 * j['mag']).clamp_min(1e-300)).max(dim=0).values
    outside = ~j['inside']
    if bool(outside.any()):
        assert float(dp[outside].abs().max()) == 0.0                       # exactly zero outside the clamp
    err = (dp.double() - j['dp']).abs()[j['inside']]
    gratio = float((err / (1e-5 * j['dp_mag'][j['inside']])).max()) if err.numel() else 0.0
    print('stats', case, 'worst ratio to the bound per statistic', [round(float(r), 4) for r in ratio], 'gradient', round(gratio, 4))
    assert bool((ratio <= 1.0).all()), ratio
    assert gratio <= 1.0, gratio


class _Recorder:
    """Stands in for ops.lib(): notes the name of every entry point fetched for a call and hands out the real function."""

    def __init__(self, real):
        self._real, self.names = real, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._real, name)


def test_two_losses_on_one_prediction_share_one_statistics_pass(monkeypatch):
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.salient_object_detection import losses
    ops, _ = _ops()
    rec = _Recorder(ops.lib())
    monkeypatch.setattr(ops, 'lib', lambda: rec)
    p, label = S.loss_inputs(2, 4099)
    label = label.view(2, 4099, 1).cuda()
    j = S.stats_judge(p, label.view(2, -1).cpu())['stats']

    def run(touch):
        leaf = p.view(2, 1, 4099, 1).cuda().requires_grad_(True)
        pred = leaf * 1.0
        rec.names = []
        bce = losses.BCELoss()(pred, label)
        if touch:
            with torch.no_grad():
                pred.mul_(1.0)                      # same values, a new version of the tensor
        iou = losses.BCEIouloss()(pred, label)
        # (autograd refuses to run the backward of a node whose saved input was changed in place: the touched run differentiates
        # the second loss only)
        (iou if touch else bce + iou).backward()
        torch.cuda.synchronize()
        return bce, iou, leaf.grad, [n for n in rec.names if n.startswith('saicv_binary_seg_stats_') and not n.endswith('ws_floats')]

    bce, iou, grad, names = run(False)
    assert names == ['saicv_binary_seg_stats_fwd', 'saicv_binary_seg_stats_bwd'], names
    assert abs(float(bce.detach()) - float(S.loss_from_stats(j, 4099, 'BCELoss'))) <= 1e-5
    assert abs(float(iou.detach()) - float(S.loss_from_stats(j, 4099, 'BCEIouloss'))) <= 1e-5
    pa = p.double().requires_grad_(True)
    ph = torch.clamp(pa, min=S.LO, max=S.HI)
    l = label.view(2, -1).cpu().double()
    st64 = torch.stack([(-(l * torch.log(ph) + (1. - l) * torch.log(1. - ph))).sum(1), ph.sum(1), l.sum(1), (ph * l).sum(1)], dim=1)
    (S.loss_from_stats(st64, 4099, 'BCELoss') + S.loss_from_stats(st64, 4099, 'BCEIouloss')).backward()
    assert rel_err(grad.view(2, -1).cpu(), pa.grad) < 1e-4
    bce2, iou2, _, names2 = run(True)
    assert names2 == ['saicv_binary_seg_stats_fwd', 'saicv_binary_seg_stats_fwd', 'saicv_binary_seg_stats_bwd'], names2
    assert float(bce2.detach()) == float(bce.detach()) and float(iou2.detach()) == float(iou.detach())


def test_dice_loss_and_non_contiguous_predictions():
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.salient_object_detection import losses
    p, label = S.loss_inputs(2, 9100)
    j = S.stats_judge(p, label)['stats']
    pred = p.view(2, 1, 91, 100).cuda()
    lab = label.view(2, 91, 100).cuda()
    assert abs(float(losses.BCEDiceLoss()(pred, lab)) - float(S.loss_from_stats(j, 9100, 'BCEDiceLoss'))) <= 1e-5
    assert abs(float(losses.BCEDiceLoss()(pred.bfloat16().float().double(), lab))
               - float(S.loss_from_stats(S.stats_judge(p.bfloat16().float(), label)['stats'], 9100, 'BCEDiceLoss'))) <= 1e-5
    wide = torch.zeros(2, 1, 91, 128, device='cuda')
    wide[..., :100] = pred
    assert float(losses.BCELoss()(wide[..., :100], lab)) == float(losses.BCELoss()(pred, lab))
