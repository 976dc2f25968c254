"""saicv_c3_bwd_stream (csrc/c3bwd.hip): BatchNorm-backward apply + data gradient + weight gradient of a bottleneck block's third
1 x 1 convolution as one kernel, judged in float64 against the three kernels it replaces.

Judge: float64 on the CPU from the bf16 inputs and from dy AS ROUNDED BY saicv_bn_act_bwd_from_partials (its bits are the
specification: the fused kernel forms the same expression with the same rounding and never stores it):
    dx = dy wd^T, dW = dW0 + dy^T x, sum_g = sum [bs_mask] dx, sum_gx = sum [bs_mask] dx (bs_y - mean) invstd.
Tolerance for each of them: the largest error of today's path (saicv_bn_act_bwd_from_partials -> saicv_conv2d_dgrad_fused ->
saicv_conv2d_wgrad) on the same inputs against the same reference, times 2 -- same operands and precision, another association of
two sums (the K slices of dx, the pixel order of dW) -- with a floor of one bf16 (dx) / fp32 (dW, sums) ulp of the result's largest
magnitude.

Shapes: M = 98 (2 x 7 x 7: no multiple of 16 or 32, four workgroups), 2304, 39200 (8 x 70 x 70: 245 workgroups of five tiles, the
last one short); both (CO, CI); with and without the bs_* sums (partial rows in deterministic mode, pooled rows with atomics
otherwise); random masks, off-centre y, dW pre-filled.  At M = 65536 (16 x 64 x 64, the smallest size at which the data gradient
of the three-kernel path is the streaming kernel whose additions the fused launch repeats) dx, dW and the partial rows are
bit-equal to the three kernels' in deterministic mode: a training step amplifies any other association of these sums.  Today's path is measured in the mode under test: the
weight gradient's error depends on it (ordered partials or atomics).

Largest errors of today's path measured with this file on an MI355X (max |error| at M = 98 / 2304 / 39200; the fused kernel's
were 0.7 ... 1.4 of them):
    (256, 64)   dx 1.2e-4 / 1.2e-4 / 2.4e-4   dW 7.1e-8 / 5.6e-7 / 5.4e-6 (atomics 7.0e-8 / 8.4e-7 / 7.2e-6)
                sum_g 3.6e-4 / 2.1e-3 / 6.4e-3   sum_gx 4.7e-4 / 2.3e-3 / 9.8e-3
    (512, 128)  dx 2.4e-4 / 2.4e-4 / 2.4e-4   dW 9.5e-8 / 5.1e-7 / 5.3e-6 (atomics 9.8e-8 / 1.2e-6 / 7.0e-6)
                sum_g 5.5e-4 / 3.5e-3 / 1.2e-2   sum_gx 5.5e-4 / 3.1e-3 / 1.1e-2
(the test prints both paths' figures on every run)."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = {98: (2, 7, 7), 2304: (4, 24, 24), 39200: (8, 70, 70), 65536: (16, 64, 64)}
JUDGED = (98, 2304, 39200)
_cache = {}


def _lib():
    from simpleaicv_pytorch_training_examples_amd import _lib as L
    return L


def _case(co, ci, m, mode):
    """Inputs, dy of the existing apply kernel, today's results IN THE SAME MODE (ordered partials or atomics: the weight gradient's
    error depends on it) and the float64 references: made once per shape and mode, never modified."""
    key = (co, ci, m, mode)
    if key in _cache:
        return _cache[key]
    L = _lib()
    lib = L.lib()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device='cuda').manual_seed(1000 * co + m)
    dev = 'cuda'
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)      # noqa: E731
    c = {}
    c['dz'] = (rn(m, co) * 0.02).bfloat16()
    c['y'] = (rn(m, co) * (0.5 + torch.rand(co, device=dev, generator=g)) + rn(co) * 2.0 + 1.5).bfloat16()     # off-centre
    c['mask'] = torch.randint(0, 256, (m * co // 8,), device=dev, generator=g, dtype=torch.uint8)
    c['gamma'] = 1.0 + 0.2 * rn(co)
    yf = c['y'].float()
    c['mean'] = yf.mean(0)
    c['invstd'] = 1.0 / (yf.var(0, unbiased=False) + 1e-5).sqrt()
    bits = ((c['mask'].view(m, co // 8, 1) >> torch.arange(8, device=dev, dtype=torch.uint8)) & 1).reshape(m, co).bool()
    gm = torch.where(bits, c['dz'].float(), torch.zeros((), device=dev))
    c['part_g'] = gm.sum(0, keepdim=True).contiguous()
    c['part_gx'] = (gm * (yf - c['mean']) * c['invstd']).sum(0, keepdim=True).contiguous()
    c['x'] = torch.relu(rn(m, ci) + 0.3).bfloat16()
    c['wd'] = (rn(ci, co) * 0.05).bfloat16()
    c['bs_y'] = (rn(m, ci) * 0.7 + rn(ci) + 1.0).bfloat16()
    c['bs_mask'] = torch.randint(0, 256, (m * ci // 8,), device=dev, generator=g, dtype=torch.uint8)
    c['bs_mean'] = c['bs_y'].float().mean(0)
    c['bs_invstd'] = 1.0 / (c['bs_y'].float().var(0, unbiased=False) + 1e-5).sqrt()
    c['dw0'] = rn(co, ci) * 0.1

    # ---- today's path
    dy = torch.empty(m, co, dtype=torch.bfloat16, device=dev)
    c['dgamma'] = torch.empty(co, device=dev)
    c['dbeta'] = torch.empty(co, device=dev)
    ws = torch.empty(lib.saicv_bn_bwd_ws_floats(m, co, L.BF16), device=dev)
    L.check(lib.saicv_bn_act_bwd_from_partials(L.BF16, L.ptr(c['dz']), L.ptr(c['mask']), L.ptr(c['y']), L.ptr(c['gamma']), L.ptr(c['mean']),
                                               L.ptr(c['invstd']), L.ptr(c['part_g']), L.ptr(c['part_gx']), 1, L.ptr(dy), 0,
                                               L.ptr(c['dgamma']), L.ptr(c['dbeta']), m, co, 1, 0, L.ptr(ws), st), 'from_partials')
    n, h, w = SHAPES[m]
    d = L.ConvDesc(n, h, w, ci, co, 1, 1, 1, 0, h, w, L.BF16)
    rows = lib.saicv_conv2d_dgrad_stat_rows(ctypes.byref(d))
    part = torch.zeros(2, rows, ci, device=dev)
    fuse = L.DgradFuse()
    fuse.bn_y, fuse.bn_mask, fuse.bn_mean, fuse.bn_invstd = L.ptr(c['bs_y']), L.ptr(c['bs_mask']), L.ptr(c['bs_mean']), L.ptr(c['bs_invstd'])
    fuse.part_g, fuse.part_gx = L.ptr(part[0]), L.ptr(part[1])
    dx_old = torch.empty(m, ci, dtype=torch.bfloat16, device=dev)
    L.check(lib.saicv_conv2d_dgrad_fused(ctypes.byref(d), L.ptr(dy), L.ptr(c['wd']), ctypes.byref(fuse), L.ptr(dx_old), st), 'dgrad_fused')
    dw_old = c['dw0'].clone()
    L.check(lib.saicv_conv2d_wgrad(ctypes.byref(d), L.ptr(dy), L.ptr(c['x']), L.ptr(dw_old), st), 'wgrad')
    torch.cuda.synchronize()

    # ---- float64 on the CPU
    dy64 = dy.cpu().double()
    ref = {'dx': dy64 @ c['wd'].cpu().double().t(), 'dw': c['dw0'].cpu().double() + dy64.t() @ c['x'].cpu().double()}
    bb = ((c['bs_mask'].cpu().view(m, ci // 8, 1) >> torch.arange(8, dtype=torch.uint8)) & 1).reshape(m, ci).bool()
    g64 = torch.where(bb, ref['dx'], torch.zeros((), dtype=torch.float64))
    ref['sg'] = g64.sum(0)
    ref['sgx'] = (g64 * (c['bs_y'].cpu().double() - c['bs_mean'].cpu().double()) * c['bs_invstd'].cpu().double()).sum(0)
    old = {'dx': dx_old.cpu().double(), 'dw': dw_old.cpu().double(), 'sg': part[0].cpu().double().sum(0), 'sgx': part[1].cpu().double().sum(0)}
    c['ref'] = ref
    c['err_old'] = {k: float((old[k] - ref[k]).abs().max()) for k in ref}
    c['dy'] = dy
    c['old'] = (dx_old, dw_old, part)
    _cache[key] = c
    return c


def _ulp(scale, mant):
    return 2.0 ** (math.floor(math.log2(max(scale, 1e-30))) - mant)


def _run_fused(c, co, ci, m, with_bs, pooled_rows):
    """-> dict of the fused entry's results (dx, dw, and the sums summed over their rows in float64 / as rows for bit comparisons)"""
    L = _lib()
    lib = L.lib()
    st = torch.cuda.current_stream().cuda_stream
    dev = 'cuda'
    dx = torch.full((m, ci), float('nan'), dtype=torch.bfloat16, device=dev)
    dw = c['dw0'].clone()
    dgamma, dbeta = torch.empty(co, device=dev), torch.empty(co, device=dev)
    ws = torch.empty(lib.saicv_c3_bwd_stream_ws_floats(m, co, ci), device=dev)
    fuse, part = None, None
    if with_bs:
        rows = pooled_rows or lib.saicv_c3_bwd_stream_rows(m, co, ci)
        assert rows > 0
        part = torch.zeros(2, rows, ci, device=dev) if pooled_rows else torch.full((2, rows, ci), float('nan'), device=dev)
        fuse = L.DgradFuse()
        fuse.bn_y, fuse.bn_mask, fuse.bn_mean, fuse.bn_invstd = L.ptr(c['bs_y']), L.ptr(c['bs_mask']), L.ptr(c['bs_mean']), L.ptr(c['bs_invstd'])
        fuse.part_g, fuse.part_gx, fuse.part_rows = L.ptr(part[0]), L.ptr(part[1]), pooled_rows
    L.check(lib.saicv_c3_bwd_stream(L.BF16, L.ptr(c['dz']), L.ptr(c['mask']), L.ptr(c['y']), L.ptr(c['gamma']), L.ptr(c['mean']),
                                    L.ptr(c['invstd']), L.ptr(c['part_g']), L.ptr(c['part_gx']), 1, L.ptr(dgamma), L.ptr(dbeta), 0,
                                    L.ptr(ws), L.ptr(c['x']), L.ptr(c['wd']), ctypes.byref(fuse) if fuse is not None else None,
                                    L.ptr(dx), L.ptr(dw), m, co, ci, st), 'c3_bwd_stream')
    torch.cuda.synchronize()
    out = {'dx': dx, 'dw': dw, 'dgamma': dgamma, 'dbeta': dbeta, 'part': part}
    return out


@pytest.fixture(params=['deterministic', 'atomics'])
def mode(request):
    lib = _lib().lib()
    prev = lib.saicv_set_deterministic(1 if request.param == 'deterministic' else 0)
    if request.param == 'deterministic':
        assert lib.saicv_deterministic_prepare(torch.cuda.current_stream().cuda_stream) == 0
    yield request.param
    lib.saicv_set_deterministic(prev)


@pytest.mark.parametrize('m', JUDGED)
@pytest.mark.parametrize('co, ci', [(256, 64), (512, 128)])
def test_fused_against_float64(mode, co, ci, m):
    c = _case(co, ci, m, mode)
    ref, err_old = c['ref'], c['err_old']
    det = mode == 'deterministic'
    for with_bs in (False, True):
        got = _run_fused(c, co, ci, m, with_bs, 0 if det else 4)
        assert torch.equal(got['dgamma'], c['dgamma']) and torch.equal(got['dbeta'], c['dbeta'])      # the same finalize launch
        res = {'dx': got['dx'].cpu().double(), 'dw': got['dw'].cpu().double()}
        if with_bs:
            res['sg'], res['sgx'] = got['part'][0].cpu().double().sum(0), got['part'][1].cpu().double().sum(0)
        for k, v in res.items():
            assert bool(torch.isfinite(v).all()), k
            err = float((v - ref[k]).abs().max())
            floor = _ulp(float(ref[k].abs().max()), 7 if k == 'dx' else 23)
            tol = max(2.0 * err_old[k], floor)
            print(f'({co}, {ci}) M={m} {mode} bs={with_bs} {k}: fused {err:.3e}  three kernels {err_old[k]:.3e}  tolerance {tol:.3e}')
            assert err <= tol, (k, err, err_old[k], tol)
        if det:
            again = _run_fused(c, co, ci, m, with_bs, 0)
            assert torch.equal(again['dx'], got['dx']) and torch.equal(again['dw'], got['dw'])
            if with_bs:
                assert torch.equal(again['part'], got['part'])


def test_bit_equal_to_the_three_kernels_at_streaming_size():
    lib = _lib().lib()
    prev = lib.saicv_set_deterministic(1)
    try:
        assert lib.saicv_deterministic_prepare(torch.cuda.current_stream().cuda_stream) == 0
        c = _case(256, 64, 65536, 'deterministic')
        dx_old, dw_old, part_old = c['old']
        got = _run_fused(c, 256, 64, 65536, True, 0)
        assert got['part'].shape == part_old.shape
        assert torch.equal(got['dx'], dx_old)
        assert torch.equal(got['dw'], dw_old)
        assert torch.equal(got['part'], part_old)
    finally:
        lib.saicv_set_deterministic(prev)


def test_unsupported_shapes_are_errors():
    L = _lib()
    lib = L.lib()
    assert lib.saicv_c3_bwd_stream_rows(1024, 256, 128) == 0 and lib.saicv_c3_bwd_stream_rows(0, 256, 64) == 0
    t = torch.zeros(16, device='cuda')
    rc = lib.saicv_c3_bwd_stream(L.BF16, L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), 1, L.ptr(t),
                                 L.ptr(t), 0, L.ptr(t), L.ptr(t), L.ptr(t), None, L.ptr(t), L.ptr(t), 1024, 256, 128,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and b'no form' in lib.saicv_last_error_string()
    rc = lib.saicv_c3_bwd_stream(L.F32, L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), 1, L.ptr(t),
                                 L.ptr(t), 0, L.ptr(t), L.ptr(t), L.ptr(t), None, L.ptr(t), L.ptr(t), 1024, 256, 64,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc != 0
