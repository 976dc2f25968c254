"""Oracle comparison AT BASELINE.json's shapes: every distinct ResNet-50 convolution at per-GPU batch 256 (the 23 shapes
of SURVEY.md 8d: forward + BN partial statistics, data gradient, weight gradient) and the four ViT-B/16 GEMM shapes at
M = 197 x 256 tokens, each against a plain PyTorch fp32 CPU computation on the same bf16-rounded operands.

The model-level fixtures (tests/test_gpu_models.py) run at batch 2-8, where the tile picker chooses other geometries
and the weight-gradient kernel other split counts than at batch 256; tests/test_gpu_fullsize.py checks batch 256 only
against itself.  Here the 256 x 128 / 256 x 256 tile paths, the real reduction splits and the stride-2 parity classes
are checked against the oracle.  Reference ops: F.conv2d / its autograd (reference resnet.py:33-43), F.linear.

Tolerance: bf16 outputs 2e-2 of the tensor's scale (storage rounding 2^-8 of an element; conftest.rel_err is scale-
relative), fp32 weight gradients 4e-3 (fp32 accumulation of bf16 products in another order), BN statistics 1e-3."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err


@pytest.fixture(autouse=True)
def _restore_threads():
    """The oracle's thread count must not outlive the test: later CPU tests compare fp32 sums whose order depends on it."""
    n = torch.get_num_threads()
    yield
    torch.set_num_threads(n)

pytestmark = pytest.mark.gpu

BATCH = int(os.environ.get('SAICV_TEST_BATCH', '256'))

# (Cin, Cout, k, stride, Hin): the 23 distinct ResNet-50 convolutions at 224 x 224 input (stem: input packed to 8 channels), each with
# the kernel family saicv_igemm_plan must give its forward (+ statistics), data gradient and weight gradient at batch 256:
# 'tiled BMxBN [kc8]' igemm_nt1_kernel, 'pw B' / 'pw3 B' the streaming kernels with B workgroups, 'tn BAxBB dma|reg xS' igemm_tn with S splits
R50_PLANS = [
    ((8, 64, 7, 2, 224), 'tiled 128x64', 'tiled 128x64', 'tn 64x128 dma x128'),
    ((64, 64, 1, 1, 56), 'pw 512', 'pw 512', 'tn 64x64 dma x502'),
    ((64, 64, 3, 1, 56), 'pw3 256', 'pw3 256', 'tn 64x128 dma x102'),
    ((64, 256, 1, 1, 56), 'pw 512', 'tiled 128x64', 'tn 128x64 dma x256'),
    ((256, 64, 1, 1, 56), 'tiled 128x64', 'pw 512', 'tn 64x128 dma x256'),
    ((256, 128, 1, 1, 56), 'tiled 256x128', 'pw 512', 'tn 128x128 dma x256'),
    ((128, 128, 3, 2, 56), 'tiled 256x128', 'tiled 256x128', 'tn 128x128 dma x56'),
    ((128, 512, 1, 1, 28), 'pw 256', 'tiled 256x128', 'tn 128x128 dma x126'),
    ((256, 512, 1, 2, 56), 'tiled 256x128', 'tiled 256x128', 'tn 128x128 dma x64'),
    ((512, 128, 1, 1, 28), 'tiled 256x128', 'pw 256', 'tn 128x128 dma x126'),
    ((128, 128, 3, 1, 28), 'tiled 256x128', 'tiled 256x128', 'tn 128x128 dma x56'),
    ((512, 256, 1, 1, 28), 'tiled 256x128', 'tiled 256x128', 'tn 128x128 dma x64'),
    ((256, 256, 3, 2, 28), 'tiled 256x128', 'tiled 256x128', 'tn 128x128 dma x14'),
    ((256, 1024, 1, 1, 14), 'tiled 256x128', 'tiled 256x128', 'tn 128x128 dma x32'),
    ((512, 1024, 1, 2, 28), 'tiled 256x128', 'tiled 256x128', 'tn 128x128 dma x16'),
    ((1024, 256, 1, 1, 14), 'tiled 256x128', 'tiled 256x128', 'tn 128x128 dma x32'),
    ((256, 256, 3, 1, 14), 'tiled 256x128', 'tiled 256x128', 'tn 128x128 dma x14'),
    ((1024, 512, 1, 1, 14), 'tiled 256x128', 'tiled 256x128', 'tn 128x128 dma x16'),
    ((512, 512, 3, 2, 14), 'tiled 128x128', 'tiled 128x128', 'tn 128x128 dma x3'),
    ((512, 2048, 1, 1, 7), 'tiled 256x128', 'tiled 128x128', 'tn 128x128 dma x8'),
    ((1024, 2048, 1, 2, 14), 'tiled 256x128', 'tiled 256x128', 'tn 128x128 dma x4'),
    ((2048, 512, 1, 1, 7), 'tiled 128x128', 'tiled 256x128', 'tn 128x128 dma x8'),
    ((512, 512, 3, 1, 7), 'tiled 128x128', 'tiled 128x128', 'tn 128x128 dma x3')]
R50 = [r[0] for r in R50_PLANS]
PLANS = {r[0]: r[1:] for r in R50_PLANS}


def _plan_name(op, d):
    """The kernel family the library plans for this product under the current switches, in the table's words."""
    from simpleaicv_pytorch_training_examples_amd import _lib
    q, pl = _lib.PlanQuery(), _lib.Plan()
    q.op, q.conv, q.stats = op, d, int(op == _lib.PLAN_CONV_FWD)
    _lib.check(_lib.lib().saicv_igemm_plan(ctypes.byref(q), ctypes.byref(pl)), 'plan')
    if pl.route == _lib.ROUTE_TILED:
        return f'tiled {pl.bm}x{pl.bn}' + (' kc8' if pl.kc8 else '')
    if pl.route == _lib.ROUTE_TN:
        return f'tn {pl.bm}x{pl.bn} {"dma" if pl.dma else "reg"} x{pl.splits}'
    return f'{"pw" if pl.route == _lib.ROUTE_PW_STREAM else "pw3"} {pl.blocks}'


def _bf(t):
    return t.to(torch.bfloat16).float()


@pytest.mark.timeout(900)
@pytest.mark.parametrize('shape', R50, ids=[f'{ci}to{co}_k{k}s{s}_{h}' for ci, co, k, s, h in R50])
def test_resnet50_conv_shapes_at_batch_256_match_cpu_fp32(shape):
    _conv_case(shape)


# kernels behind a switch (off by default because they measured level or slower, profiles/r03_lds_fill_and_kc8.md): the
# switches are read per call, so the same oracle comparison covers them
SWITCHED = [('SAICV_TN_DMA', '0', (256, 256, 3, 1, 14)), ('SAICV_TN_DMA', '0', (1024, 256, 1, 1, 14)),
            ('SAICV_NT_KC8', '1', (1024, 512, 1, 1, 14)), ('SAICV_NT_KC8', '1', (256, 128, 1, 1, 56))]
# what the switch must change in the plans of PLANS (forward, data gradient, weight gradient)
SWITCHED_PLANS = [('tiled 256x128', 'tiled 256x128', 'tn 128x128 reg x14'), ('tiled 256x128', 'tiled 256x128', 'tn 128x128 reg x32'),
                  ('tiled 256x128 kc8', 'tiled 256x128 kc8', 'tn 128x128 dma x16'), ('tiled 256x128 kc8', 'pw 512', 'tn 128x128 dma x256')]


@pytest.mark.timeout(900)
@pytest.mark.parametrize('var,val,shape', SWITCHED, ids=[f'{v}={x}_{c[0]}to{c[1]}_k{c[2]}_{c[4]}' for v, x, c in SWITCHED])
def test_switched_kernel_paths_at_batch_256_match_cpu_fp32(var, val, shape, monkeypatch):
    """The register-staged weight-gradient kernel and the 128-byte-K-slice forward / data-gradient kernel on every eligible launch: same oracle, same tolerances."""
    monkeypatch.setenv(var, val)
    _conv_case(shape, SWITCHED_PLANS[SWITCHED.index((var, val, shape))])


def _conv_case(shape, plans=None):
    from simpleaicv_pytorch_training_examples_amd import _lib, ops
    from simpleaicv_pytorch_training_examples_amd._lib import check, lib, ptr
    ci, co, k, s, h = shape
    pad = k // 2
    dt = torch.bfloat16
    L, st = lib(), _lib.stream()
    g = torch.Generator().manual_seed(ci * 7 + co * 3 + k + s + h)
    x = _bf(torch.randn(BATCH, ci, h, h, generator=g)).contiguous(memory_format=torch.channels_last)
    if ci == 8:
        x[:, 3:] = 0            # the stem sees a 3-channel image padded to 8
    w = _bf(torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5)
    d = ops._desc(BATCH, h, h, ci, co, k, k, s, pad, dt)
    oh, ow = d.OH, d.OW
    dy = _bf(torch.randn(BATCH, co, oh, ow, generator=g)).contiguous(memory_format=torch.channels_last)
    if BATCH == 256:            # which kernel family this comparison certifies (the table is written for BASELINE.json's batch)
        planned = tuple(_plan_name(op, d) for op in (_lib.PLAN_CONV_FWD, _lib.PLAN_CONV_DGRAD, _lib.PLAN_CONV_WGRAD))
        assert planned == tuple(plans or PLANS[shape]), (shape, planned)

    # ---- CPU fp32 oracle
    torch.set_num_threads(min(os.cpu_count() or 8, 64))
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    y_ref = F.conv2d(xr, wr, None, s, pad)
    y_ref.backward(dy)
    yq = _bf(y_ref.detach())                                   # what the kernel stores and sums
    sum_ref = yq.double().sum((0, 2, 3))
    sq_ref = (yq.double() ** 2).sum((0, 2, 3))

    # ---- device, through the C-ABI
    xd = x.to(dt).cuda()                                       # NHWC memory
    wf = w.permute(0, 2, 3, 1).contiguous().to(dt).cuda()      # [Cout][R][S][Cin]
    wdg = w.permute(1, 2, 3, 0).contiguous().to(dt).cuda()     # [Cin][R][S][Cout]
    y = torch.empty((BATCH, oh, ow, co), dtype=dt, device='cuda')
    rows = L.saicv_conv2d_stat_rows(ctypes.byref(d))
    stats = torch.zeros((2, rows, co), dtype=torch.float32, device='cuda')
    check(L.saicv_conv2d_fwd(ctypes.byref(d), ptr(xd), ptr(wf), 0, ptr(y), 0, ptr(stats[0]), ptr(stats[1]), st), 'fwd')
    dyd = dy.to(dt).cuda()
    dx = torch.empty((BATCH, h, h, ci), dtype=dt, device='cuda')
    check(L.saicv_conv2d_dgrad(ctypes.byref(d), ptr(dyd), ptr(wdg), ptr(dx), st), 'dgrad')
    dw = torch.zeros((co, k, k, ci), dtype=torch.float32, device='cuda')
    check(L.saicv_conv2d_wgrad(ctypes.byref(d), ptr(dyd), ptr(xd), ptr(dw), st), 'wgrad')
    torch.cuda.synchronize()

    tag = str(shape)
    assert rel_err(y.permute(0, 3, 1, 2).float(), y_ref) < 2e-2, 'forward ' + tag
    assert rel_err(stats[0].double().sum(0), sum_ref) < 1e-3, 'BN partial sums ' + tag
    assert rel_err(stats[1].double().sum(0), sq_ref) < 1e-3, 'BN partial sums of squares ' + tag
    if ci != 8:                                                # the network input needs no gradient (stem dgrad never runs)
        assert rel_err(dx.permute(0, 3, 1, 2).float(), xr.grad) < 2e-2, 'data gradient ' + tag
    gw = wr.grad
    if ci == 8:
        gw = gw[:, :3]
        dw = dw[..., :3]
    assert rel_err(dw.permute(0, 3, 1, 2), gw) < 4e-3, 'weight gradient ' + tag


@pytest.mark.timeout(900)
@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_s2d_stem_at_batch_256_matches_cpu_fp32(dt):
    """The stem the benchmark actually runs since the space-to-depth change: saicv_pack_input_s2d + the 4 x 4 x 16
    stride-1 convolution + BatchNorm + ReLU (ops.pack_stem_input / ops.conv_bn_act) at 256 x 3 x 224 x 224, forward and weight
    gradient, against F.conv2d(7 x 7, stride 2, padding 3) + batch_norm + relu in fp32 on the CPU on the same bf16-rounded
    operands (reference resnet.py:172-174).  fp32 parity mode pins the arithmetic (1e-3); in bf16 the conv output, the
    BatchNorm backward and its input gradient are STORED in bf16, which the 3.2 M-pixel weight-gradient sums feel at the
    percent level (4e-2; the small-size test of tests/test_gpu_kernels.py allows 3e-2 for the same reason)."""
    import torch.nn as nn
    from simpleaicv_pytorch_training_examples_amd import ops
    g = torch.Generator().manual_seed(224)
    x = _bf(torch.randn(BATCH, 224, 224, 3, generator=g)).permute(0, 3, 1, 2)          # NHWC memory, NCHW shape (the collater's form)
    w = _bf(torch.randn(64, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5)
    gamma = torch.rand(64, generator=g) + 0.5
    beta = torch.randn(64, generator=g) * 0.1
    dz = _bf(torch.randn(BATCH, 112, 112, 64, generator=g)).permute(0, 3, 1, 2)
    torch.set_num_threads(min(os.cpu_count() or 8, 64))
    wr = w.clone().requires_grad_(True)
    y_ref = F.conv2d(x, wr, None, 2, 3)
    z_ref = F.relu(F.batch_norm(y_ref, None, None, gamma, beta, True, 0.1, 1e-5))
    z_ref.backward(dz)
    conv, bn = nn.Conv2d(3, 64, 7, 2, 3, bias=False).cuda(), nn.BatchNorm2d(64).cuda()
    with torch.no_grad():
        conv.weight.copy_(w)
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    conv.weight.data = conv.weight.data.contiguous(memory_format=torch.channels_last)
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=dt == torch.bfloat16):
        xp = ops.pack_stem_input(x.cuda(), conv, dt)
        assert getattr(xp, '_saicv_s2d', None) is not None and xp.shape[1] == 16
        z = ops.conv_bn_act(xp, conv.weight, bn, 2, 3, True)
    z.backward(dz.cuda().to(z.dtype).contiguous(memory_format=torch.channels_last))
    torch.cuda.synchronize()
    assert tuple(z.shape) == (BATCH, 64, 112, 112)
    f32 = dt == torch.float32
    assert rel_err(z.float(), z_ref) < (1e-3 if f32 else 2e-2)
    mean_ref = y_ref.detach().transpose(0, 1).flatten(1).double().mean(1)
    var_ref = y_ref.detach().transpose(0, 1).flatten(1).double().var(1)
    assert rel_err(bn.running_mean, 0.1 * mean_ref) < (1e-4 if f32 else 2e-3)     # bf16: statistics of the rounded, stored y
    assert rel_err(bn.running_var, 0.9 + 0.1 * var_ref) < (1e-4 if f32 else 2e-3)
    assert rel_err(conv.weight.grad, wr.grad) < (1e-3 if f32 else 4e-2)
    dgamma_ref, dbeta_ref = _bn_grads(y_ref.detach(), dz, z_ref.detach())
    # bf16: the ReLU gate is taken from the bf16-rounded y -- a few thousand of the 3.2 M pixels per channel sit within that
    # rounding of zero and flip, each moving the sum by its whole dz (measured 2.0e-2 of the largest dbeta)
    assert rel_err(bn.weight.grad, dgamma_ref) < (1e-3 if f32 else 4e-2)
    assert rel_err(bn.bias.grad, dbeta_ref) < (1e-3 if f32 else 4e-2)


def _bn_grads(y, dz, z):
    """dgamma / dbeta of relu(batch_norm(y)) in fp64 on the CPU."""
    yd = y.double().transpose(0, 1).flatten(1)
    g = (dz.double() * (z > 0)).transpose(0, 1).flatten(1)
    xhat = (yd - yd.mean(1, keepdim=True)) / (yd.var(1, unbiased=False, keepdim=True) + 1e-5).sqrt()
    return (g * xhat).sum(1), g.sum(1)


VIT = [(768, 2304, 'qkv'), (768, 768, 'proj'), (768, 3072, 'fc1'), (3072, 768, 'fc2')]


@pytest.mark.timeout(900)
@pytest.mark.parametrize('kn', VIT, ids=[v[2] for v in VIT])
def test_vit_base_gemm_shapes_at_batch_256_match_cpu_fp32(kn):
    from simpleaicv_pytorch_training_examples_amd import _lib
    from simpleaicv_pytorch_training_examples_amd._lib import check, lib, ptr
    K, N, name = kn
    M = 197 * BATCH
    L, st = lib(), _lib.stream()
    g = torch.Generator().manual_seed(K + N)
    x = _bf(torch.randn(M, K, generator=g))
    w = _bf(torch.randn(N, K, generator=g) * K ** -0.5)
    b = torch.randn(N, generator=g) * 0.1
    dy = _bf(torch.randn(M, N, generator=g))
    torch.set_num_threads(min(os.cpu_count() or 8, 64))
    y_ref = F.linear(x, w, b)
    dx_ref = dy @ w
    dw_ref = dy.t() @ x
    db_ref = dy.sum(0)

    dt = torch.bfloat16
    xd, wf, wd, dyd = x.to(dt).cuda(), w.to(dt).cuda(), w.t().contiguous().to(dt).cuda(), dy.to(dt).cuda()
    y = torch.empty((M, N), dtype=dt, device='cuda')
    bd = b.cuda()
    check(L.saicv_linear_fwd(0, ptr(xd), ptr(wf), ptr(bd), ptr(y), M, K, N, 0, 0, 0, 1, st), 'linear_fwd')
    dx = torch.empty((M, K), dtype=dt, device='cuda')
    check(L.saicv_linear_dgrad(0, ptr(dyd), ptr(wd), ptr(dx), M, K, N, 0, st), 'linear_dgrad')
    dw = torch.zeros((N, K), dtype=torch.float32, device='cuda')
    db = torch.zeros(N, dtype=torch.float32, device='cuda')
    check(L.saicv_linear_wgrad(0, ptr(dyd), ptr(xd), ptr(dw), ptr(db), M, K, N, st), 'linear_wgrad')
    torch.cuda.synchronize()
    assert rel_err(y.float(), y_ref) < 2e-2, name
    assert rel_err(dx.float(), dx_ref) < 2e-2, name
    assert rel_err(dw, dw_ref) < 4e-3, name
    assert rel_err(db, db_ref) < 4e-3, name


INLINE_SHAPES = [(64, 256, 1, 1, 56), (128, 128, 3, 2, 56), (256, 256, 3, 1, 14), (512, 2048, 1, 1, 7)]


@pytest.mark.timeout(900)
@pytest.mark.parametrize('shape', INLINE_SHAPES, ids=[f'{ci}to{co}_k{k}s{s}_{h}' for ci, co, k, s, h in INLINE_SHAPES])
def test_batchnorm_statistics_through_atomic_rows_at_batch_256(shape):
    """The default training path of a conv + BatchNorm + ReLU layer at BASELINE.json's batch: saicv_conv2d_fwd_stats adds
    the per-tile sums into a few rows with fp32 atomics, saicv_bn_act_fwd_stats finalises them in-kernel (mean, invstd,
    running statistics, z = relu(bn(y)) + sign mask).  Against F.batch_norm on the CPU over the conv output the device
    stored (bf16), and the backward pair saicv_conv2d_dgrad_fused(part_rows) -> saicv_bn_act_bwd_inline against the three-pass
    saicv_bn_act_bwd on the same tensors."""
    from simpleaicv_pytorch_training_examples_amd import _lib, ops
    from simpleaicv_pytorch_training_examples_amd._lib import check, lib, ptr
    ci, co, k, s, h = shape
    pad = k // 2
    dt = torch.bfloat16
    L, st = lib(), _lib.stream()
    g = torch.Generator().manual_seed(ci + co + k + s + h)
    x = _bf(torch.randn(BATCH, ci, h, h, generator=g)).contiguous(memory_format=torch.channels_last)
    w = _bf(torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5)
    gamma, beta = torch.rand(co, generator=g) + 0.5, torch.randn(co, generator=g) * 0.2
    d = ops._desc(BATCH, h, h, ci, co, k, k, s, pad, dt)
    oh, ow = d.OH, d.OW
    M = BATCH * oh * ow
    xd = x.to(dt).cuda()
    wf = w.permute(0, 2, 3, 1).contiguous().to(dt).cuda()
    y = torch.empty((BATCH, oh, ow, co), dtype=dt, device='cuda')
    rows = ops._stat_rows(L.saicv_conv2d_stat_rows(ctypes.byref(d)))
    stats = torch.zeros((2, rows, co), dtype=torch.float32, device='cuda')
    check(L.saicv_conv2d_fwd_stats(ctypes.byref(d), ptr(xd), ptr(wf), ptr(y), ptr(stats[0]), ptr(stats[1]), rows, st), 'fwd_stats')
    z = torch.empty_like(y)
    mask = torch.empty(M * co // 8, dtype=torch.uint8, device='cuda')
    mean, invstd = torch.empty(co, device='cuda'), torch.empty(co, device='cuda')
    rm, rv = torch.zeros(co, device='cuda'), torch.ones(co, device='cuda')
    nbt = torch.zeros((), dtype=torch.int64, device='cuda')
    gd, bd = gamma.cuda(), beta.cuda()
    check(L.saicv_bn_act_fwd_stats(0, ptr(y), 0, ptr(z), ptr(stats[0]), ptr(stats[1]), rows, float(M), ptr(gd), ptr(bd), ptr(rm),
                                   ptr(rv), 0.1, 1e-5, ptr(nbt), ptr(mean), ptr(invstd), M, co, 1, ptr(mask), st), 'bn_act_fwd_stats')
    torch.cuda.synchronize()
    yc = y.float().cpu().permute(0, 3, 1, 2)                       # what the device stored; its statistics are the truth
    mu = yc.double().mean((0, 2, 3))
    var = yc.double().var((0, 2, 3), unbiased=False)
    assert rel_err(mean.double().cpu(), mu) < 1e-4
    assert rel_err(invstd.double().cpu(), (var + 1e-5).rsqrt()) < 1e-4
    assert rel_err(rm.double().cpu(), 0.1 * mu) < 1e-4
    assert rel_err(rv.double().cpu(), 0.9 + 0.1 * var * M / (M - 1)) < 1e-4 and int(nbt) == 1
    z_ref = F.relu(F.batch_norm(yc, None, None, gamma, beta, True, 0.1, 1e-5))
    assert rel_err(z.float().cpu().permute(0, 3, 1, 2), z_ref) < 2e-2

    # ---- backward: a following 1x1 convolution's data gradient leaves this layer's sums in atomic rows
    k2 = 64
    d2 = ops._desc(BATCH, oh, ow, co, k2, 1, 1, 1, 0, dt)
    w2 = (torch.randn(co, 1, 1, k2, generator=g) * 0.05).to(dt).cuda()        # [Cin][R][S][Cout] for the data gradient
    dy2 = _bf(torch.randn(BATCH, oh, ow, k2, generator=g)).to(dt).cuda()
    rows_b = ops._stat_rows(L.saicv_conv2d_dgrad_stat_rows(ctypes.byref(d2)))
    part = torch.zeros((2, rows_b, co), dtype=torch.float32, device='cuda')
    dz = torch.empty_like(z)
    f = _lib.DgradFuse()
    f.bn_y, f.bn_mask, f.bn_mean, f.bn_invstd = ptr(y), ptr(mask), ptr(mean), ptr(invstd)
    f.part_g, f.part_gx, f.part_rows = ptr(part[0]), ptr(part[1]), rows_b
    check(L.saicv_conv2d_dgrad_fused(ctypes.byref(d2), ptr(dy2), ptr(w2), ctypes.byref(f), ptr(dz), st), 'dgrad_fused')
    out = []
    ws = torch.empty(L.saicv_bn_bwd_ws_floats(M, co, 0), device='cuda')
    for inline in (False, True):
        dyb = torch.empty_like(y)
        dgam, dbet = torch.empty(co, device='cuda'), torch.empty(co, device='cuda')
        if inline:
            check(L.saicv_bn_act_bwd_inline(0, ptr(dz), ptr(mask), ptr(y), ptr(gd), ptr(mean), ptr(invstd), ptr(part[0]), ptr(part[1]),
                                            rows_b, ptr(dyb), 0, ptr(dgam), ptr(dbet), M, co, 1, 0, st), 'bn_bwd_inline')
        else:
            check(L.saicv_bn_act_bwd(0, ptr(dz), 0, ptr(mask), ptr(y), ptr(gd), ptr(mean), ptr(invstd), ptr(dyb), 0, ptr(dgam),
                                     ptr(dbet), M, co, 1, 0, ptr(ws), st), 'bn_bwd')
        torch.cuda.synchronize()
        out.append((dyb.float(), dgam.clone(), dbet.clone()))
    assert rel_err(out[1][1], out[0][1]) < 1e-4 and rel_err(out[1][2], out[0][2]) < 1e-4
    assert rel_err(out[1][0], out[0][0]) < 8e-3
