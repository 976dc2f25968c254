"""CPU proof that the off-centre builder and the bounds of tests/norm_stats_common.py mean something (no GPU):

  * every class of the builder realises its |mean| / std within 25 %, in fp32 and in bf16, at a count of 8 and at 4096;
  * PyTorch's own fp32 batch_norm / group_norm / layer_norm, judged exactly as the HIP kernels are in
    tests/test_gpu_norm_stats.py, stay inside every asserted bound with a margin of 3 -- the bounds are attainable;
  * a float64 model of the kernels' route (partial rows -> finalize -> scale / shift -> apply) passes, and each of five faults
    planted into it breaks at least one assertion: a dropped partial row, the biased variance in running_var at a count of 8,
    statistics taken before the bf16 rounding at class 32, the mean folded into an fp32 `shift` on a constant nonzero channel,
    a finalize that ignores partial rows >= 32.
"""
import pytest
import torch
import torch.nn.functional as F

import norm_stats_common as N

DTYPES = [torch.float32, torch.bfloat16]
IDS = ['fp32', 'bf16']


@pytest.mark.parametrize('dt', DTYPES, ids=IDS)
@pytest.mark.parametrize('length', [8, 32, 4096])
def test_builder_realises_every_class_ratio(dt, length):
    x, x64 = N.build_slabs(4 * N.NCLS, length, dt, seed=length)
    N.assert_ratios(x64, 'float64')
    N.assert_ratios(x, str(dt))
    assert set(N.slab_classes(4 * N.NCLS)) == set(N.GROUPS)
    centred = torch.randn(4 * N.NCLS, length).to(dt)
    with pytest.raises(AssertionError):            # the assertion notices inputs that drifted back to centred
        N.assert_ratios(centred, 'centred')


def _torch_bn(x, gamma, beta, rm, rv):
    """torch's fp32 BatchNorm on x [M][C] -> the dict judge_* take"""
    xt = x.float().t().contiguous()[None]                                    # [1][C][M]
    out, mean, invstd = torch.native_batch_norm(xt, gamma, beta, rm, rv, True, 0.1, N.EPS)
    return {'mean': mean, 'invstd': invstd, 'out': out[0].t(), 'running_mean': rm, 'running_var': rv}


@pytest.mark.parametrize('count', [8, 4096, 50176])
def test_torch_fp32_batch_norm_holds_every_bound_with_margin(count):
    C = 4 * N.NCLS
    g = torch.Generator().manual_seed(count)
    x = N.build_slabs(C, count, torch.float32, seed=count)[0].t().contiguous()          # [M][C]
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5
    rm0, rv0 = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) * 0.1 + 0.05
    ref = N.bn_ref(x, gamma, beta, running_mean=rm0, running_var=rv0)
    got = _torch_bn(x, gamma, beta, rm0.clone(), rv0.clone())
    led, cls = N.Ledger(), N.slab_classes(C)
    N.judge_stats(led, 'torch', torch.float32, cls, ref, got)
    N.judge_out(led, 'torch', torch.float32, cls, ref['out'], got['out'], beta)
    # backward: torch's autograd in fp32 against the float64 formula fed torch's saved statistics
    dz = torch.randn(count, C, generator=g)
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    F.batch_norm(xr.t()[None], None, None, gr, br, True, 0.1, N.EPS).backward(dz.t()[None])
    refb = N.bn_bwd_ref(x, dz, gamma, got['mean'], got['invstd'])
    N.judge_grads(led, 'torch', torch.float32, cls, refb, {'dx': xr.grad, 'dgamma': gr.grad, 'dbeta': br.grad})
    led.check()
    for route, group, qty, err, bound in led.rows:
        if bound is not None and group != 'dead':
            assert 3 * err <= bound, (group, qty, err, bound)


def test_torch_fp32_group_norm_and_layer_norm_hold_every_bound_with_margin():
    led = N.Ledger()
    # GroupNorm(32, 256) on a 16 x 16 map, the offset per (sample, group)
    n, c, G, hw = 2, 256, 32, 256
    cpg = c // G
    x = N.build_slabs(n * G, hw * cpg, torch.float32, seed=5)[0].view(n, G, cpg, hw).reshape(n, c, hw)
    got = F.group_norm(x, G, None, None, N.EPS)
    ref = F.group_norm(x.double(), G, None, None, N.EPS)
    cls = N.slab_classes(n * G)
    N.judge_out(led, 'torch_gn', torch.float32, cls, ref.view(n * G, -1), got.view(n * G, -1), slab_dim=0)
    # LayerNorm over rows of 768
    x = N.build_slabs(4 * N.NCLS, 768, torch.float32, seed=6)[0]
    got = F.layer_norm(x, (768,), None, None, N.EPS)
    ref = F.layer_norm(x.double(), (768,), None, None, N.EPS)
    N.judge_out(led, 'torch_ln', torch.float32, N.slab_classes(4 * N.NCLS), ref, got, slab_dim=0)
    led.check()
    for route, group, qty, err, bound in led.rows:
        if bound is not None:
            assert 3 * err <= bound, (route, group, qty, err, bound)


# ------------------------------------------------------------------------------ a float64 model of the kernels' route, with faults
def _route_model(x, x_unrounded, gamma, beta, rm0, rv0, tile=4, fault=None):
    """Partial rows of `tile` pixels -> finalize -> (scale, shift) -> apply, as csrc/bn.hip arranges it, in float64."""
    xs = (x_unrounded if fault == 'stats_before_rounding' else x).double()
    M, C = xs.shape
    rows_s = xs.view(M // tile, tile, C).sum(1)
    rows_q = xs.pow(2).view(M // tile, tile, C).sum(1)
    if fault == 'row_dropped':
        rows_s, rows_q = rows_s[:-1], rows_q[:-1]
    if fault == 'rows_from_32_ignored':
        rows_s, rows_q = rows_s[:32], rows_q[:32]
    mean = rows_s.sum(0) / M
    var = (rows_q.sum(0) / M - mean * mean).clamp_min(0)
    invstd = (var + N.EPS).rsqrt()
    unbiased = var if fault == 'biased_running_var' else var * M / (M - 1)
    scale = gamma.double() * invstd
    if fault == 'fp32_shift':
        shift = (beta.double() - (mean * scale).float().double()).float().double()
        out = (x.double() * scale.float().double()).float().double() + shift
    else:
        out = (x.double() - mean) * scale + beta.double()
    return {'mean': mean, 'invstd': invstd, 'out': out, 'running_mean': 0.9 * rm0.double() + 0.1 * mean,
            'running_var': 0.9 * rv0.double() + 0.1 * unbiased}


FAULTS = [('row_dropped', torch.float32, 4096, 0.0), ('biased_running_var', torch.float32, 8, 0.0),
          ('stats_before_rounding', torch.bfloat16, 4096, 0.0), ('fp32_shift', torch.float32, 4096, 3.0),
          ('rows_from_32_ignored', torch.float32, 4096, 0.0)]


@pytest.mark.parametrize('fault,dt,count,dead_value', FAULTS, ids=[f[0] for f in FAULTS])
def test_each_planted_fault_breaks_an_assertion(fault, dt, count, dead_value):
    C = 2 * N.NCLS
    g = torch.Generator().manual_seed(11)
    x, x64 = N.build_slabs(C, count, dt, seed=count + 1, dead_value=dead_value)
    N.assert_ratios(x, fault, dead_value)
    x, x64 = x.t().contiguous(), x64.t().contiguous()
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5
    rm0, rv0 = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) * 0.1 + 0.05
    ref = N.bn_ref(x, gamma, beta, running_mean=rm0, running_var=rv0)
    cls = N.slab_classes(C)

    def judged(f):
        got = _route_model(x, x64, gamma, beta, rm0, rv0, fault=f)
        led = N.Ledger()
        N.judge_stats(led, f or 'faithful', dt, cls, ref, got)
        # (the model's output is not rounded to dt: the fp32 bounds apply to it)
        N.judge_out(led, f or 'faithful', torch.float32, cls, ref['out'], got['out'], beta)
        return led

    judged(None).check()                                   # the faithful route passes on the same inputs
    led = judged(fault)
    assert led.bad, f'{fault} went unnoticed'
    expect = {'row_dropped': 'mean', 'biased_running_var': 'running_var', 'stats_before_rounding': '[c32] var',
              'fp32_shift': '[dead] out-beta', 'rows_from_32_ignored': 'mean'}[fault]
    assert any(expect in b for b in led.bad), (fault, led.bad)
    if fault == 'biased_running_var':                      # ... and only there: the saved statistics are untouched
        assert all('running_var' in b for b in led.bad), led.bad
    if fault == 'stats_before_rounding':                   # the rounding is resolvable off-centre only
        assert not any('[c0]' in b or '[tiny]' in b for b in led.bad), led.bad
