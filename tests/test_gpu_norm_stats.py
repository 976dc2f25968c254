"""BatchNorm / GroupNorm / LayerNorm statistics OFF-CENTRE and at every reduction route, through the C-ABI, against float64.

The kernels take var = E[x^2] - E[x]^2 in fp32 (csrc/bn.hip finalize kernels and the in-kernel finalize of bn_act_fwd_kernel<SELF>,
csrc/groupnorm.hip gn_coeffs_kernel) from fp32 partial sums; csrc/tfm.hip's LayerNorm is two-pass and serves as the control.  Every
other test feeds zero-centred data (|mean| / std <= 0.2); here the channels (groups, rows) carry |mean| / std = 0, 2, 8, 32, 128 in
both signs plus a dead and a tiny-variance class (tests/norm_stats_common.py: builder, float64 references, bounds, judge;
tests/test_norm_stats_host.py proves on the CPU that the bounds are attainable and that planted faults break them).

The reference is float64 arithmetic on the CPU over the values the device holds: for a BatchNorm behind a convolution that is the
STORED y read back, so the statistics path is judged apart from the GEMM (tests/test_gpu_igemm_exact.py has that).  In bf16 the saved
statistics must be those of the stored tensor and, where the two are resolvably apart, not those of the unrounded product.
Each launch form is asserted from saicv_igemm_plan before it runs.  Every backward route is fed the saved mean / invstd of its own
forward; the ReLU decisions of the reference are the device's (its sign mask), as in __graft_entry__.smoke().

SAICV_NORM_STATS_REPORT=<file>: every (route, class, quantity, error, bound) is appended there (DESIGN.md section 4b is that table).
"""
import ctypes
import math
import os

import pytest
import torch
import torch.nn.functional as F

import norm_stats_common as N

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ['fp32', 'bf16']
MOM = 0.1


def _L():
    from simpleaicv_pytorch_training_examples_amd import _lib
    return _lib, _lib.lib(), _lib.stream()


def _finish(led):
    torch.cuda.synchronize()
    path = os.environ.get('SAICV_NORM_STATS_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write(led.report() + '\n')
    led.check()


def _tag(dt):
    return 'fp32' if dt == torch.float32 else 'bf16'


def _gate(mask, M, C, dt):
    """the sign mask of saicv_bn_act_fwd (one byte per 16-byte chunk, bit j = element j) -> 0/1 [M][C] on the CPU"""
    n = 8 if dt == torch.bfloat16 else 4
    m = mask.cpu().to(torch.int32)
    return ((m[:, None] >> torch.arange(n, dtype=torch.int32)[None]) & 1).reshape(M, C).double()


def _affine(C, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5, torch.randn(C, generator=g) * 0.1,
            torch.rand(C, generator=g) * 0.1 + 0.05)


def _plan(d, stats=1, op=None, bn_sums=0):
    _lib, L, _ = _L()
    q, pl = _lib.PlanQuery(), _lib.Plan()
    q.op, q.conv, q.stats, q.bn_sums = _lib.PLAN_CONV_FWD if op is None else op, d, stats, bn_sums
    _lib.check(L.saicv_igemm_plan(ctypes.byref(q), ctypes.byref(pl)), 'plan')
    return pl


def _conv_operands(dt, n, h, w, cin, K, k, seed):
    """x [n][h][w][cin] and wf [K][k][k][cin] whose convolution has the builder's per-output-channel offsets: input channel 0 is the
    constant 1 and carries the mean through the centre tap; the other input channels are unit-variance noise and carry the std.
    -> x, wf (dtype dt, CPU), the bound class of each output channel"""
    g = torch.Generator().manual_seed(seed)
    M = n * h * w
    x = torch.randn(M, cin, dtype=torch.float64, generator=g)
    x -= x.mean(0)
    x /= x.pow(2).mean(0).sqrt()
    x[:, 0] = 1.0
    mean, std = N.slab_params(K)
    wn = torch.randn(K, k, k, cin, dtype=torch.float64, generator=g)
    wn[..., 0] = 0.0
    wn = wn / wn.flatten(1).norm(dim=1).view(K, 1, 1, 1) * std.view(K, 1, 1, 1)
    wn[:, k // 2, k // 2, 0] = mean
    return x.view(n, h, w, cin).to(dt), wn.to(dt), N.slab_classes(K)


def _stats_of_stored(led, route, dt, y, yu, got_var):
    """bf16: the statistics describe the stored tensor.  yu: the unrounded float64 product of the same operands (or None)."""
    if yu is None or dt != torch.bfloat16:
        return
    _, vs = N.realised(y.double().t())
    _, vu = N.realised(yu.t())
    C = y.shape[1]
    cls = N.slab_classes(C)
    seen = 0
    for c in range(C):
        b = N.bounds(cls[c], dt)
        if b is None:
            continue
        apart = abs(float(vu[c] - vs[c])) / (float(vs[c]) + N.EPS)
        if apart > 2 * b['var']:              # resolvable: no variance is within the bound of both, and the device's must be the stored one's
            seen += 1
            d = abs(float(got_var[c] - vu[c])) / (float(vu[c]) + N.EPS)
            led.require(d > b['var'], f'{route} channel {c} [{cls[c]}]: variance matches the unrounded product ({d:.2e})')
    led.require(seen > 0, f'{route}: no channel where stored and unrounded statistics are resolvably apart')


# ------------------------------------------------------------------------------ the BatchNorm chain
def _bn_chain(led, route, dt, y, classes, stat, rows, fwd, bwd, seed, yu=None, dgrad=None, relu=1, slices=None, with_res=True):
    """y [M][C] on the device with its statistics `stat` [2][rows][C]; fwd in {'finalize', 'inline', 'join'}; bwd in {None, 'reduce',
    'inline', 'partials'} ('inline' / 'partials' take their sums from saicv_conv2d_dgrad_fused of a following 1 x 1 convolution
    dgrad = K2).  slices: judge the output on these row ranges only (big cases)."""
    _lib, L, st = _L()
    check, ptr, code = _lib.check, _lib.ptr, _lib.dtype_code(dt)
    M, C = y.shape
    n = 8 if dt == torch.bfloat16 else 4
    gamma, beta, rm0, rv0 = _affine(C, seed)
    g = torch.Generator().manual_seed(seed + 1)
    dev = y.device
    gm, bt, rm, rv = gamma.cuda(), beta.cuda(), rm0.cuda(), rv0.cuda()
    nbt = torch.tensor([41], dtype=torch.int64, device=dev)
    mean, invstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
    z = torch.empty_like(y)
    mask = torch.empty(M * C // n, dtype=torch.uint8, device=dev) if relu else None
    res = None
    if fwd in ('finalize', 'inline') and slices is None and with_res:
        res = torch.randn(M, C, generator=g).to(dt).cuda()
    rs = rsh = None
    if fwd == 'finalize':
        scale, shift = torch.empty(C, device=dev), torch.empty(C, device=dev)
        ws = torch.empty(L.saicv_bn_ws_floats(C), device=dev)
        check(L.saicv_bn_finalize_fwd(ptr(stat[0]), ptr(stat[1]), rows, C, float(M), ptr(gm), ptr(bt), ptr(rm), ptr(rv), MOM, N.EPS,
                                      ptr(mean), ptr(invstd), ptr(scale), ptr(shift), ptr(ws), ptr(nbt), st), 'finalize')
        check(L.saicv_bn_act_fwd(code, ptr(y), ptr(res), ptr(z), ptr(scale), ptr(shift), M, C, relu, ptr(mask), st), 'bn_act_fwd')
    elif fwd == 'inline':
        check(L.saicv_bn_act_fwd_stats(code, ptr(y), ptr(res), ptr(z), ptr(stat[0]), ptr(stat[1]), rows, float(M), ptr(gm), ptr(bt), ptr(rm),
                                       ptr(rv), MOM, N.EPS, ptr(nbt), ptr(mean), ptr(invstd), M, C, relu, ptr(mask), st), 'bn_act_fwd_stats')
    else:
        res = torch.randn(M, C, generator=g).to(dt).cuda()
        rs, rsh = (torch.rand(C, generator=g) + 0.5).cuda(), (torch.randn(C, generator=g) * 0.3).cuda()
        check(L.saicv_bn_act_fwd_join(code, ptr(y), ptr(res), ptr(rs), ptr(rsh), ptr(z), 0, 0, ptr(stat[0]), ptr(stat[1]), rows, float(M),
                                      ptr(gm), ptr(bt), ptr(rm), ptr(rv), MOM, N.EPS, ptr(nbt), ptr(mean), ptr(invstd), M, C, relu,
                                      ptr(mask), st), 'bn_act_fwd_join')
    torch.cuda.synchronize()
    assert int(nbt) == 42, f'{route}: num_batches_tracked {int(nbt)}, expected 41 + 1'

    # ---- float64 over the stored y
    yc = y.cpu()
    if slices is None:
        N.assert_ratios(yc.t(), route)
        resc = None if res is None else (res.cpu().double() if rs is None else res.cpu().double() * rs.cpu().double() + rsh.cpu().double())
        gate = _gate(mask, M, C, dt) if relu else None
        ref = N.bn_ref(yc, gamma, beta, N.EPS, MOM, rm0, rv0, resc, gate)
        N.judge_out(led, route, dt, classes, ref['out'], z, beta if (res is None and not relu) else None)
    else:
        s = torch.zeros(C, dtype=torch.float64)
        q = torch.zeros(C, dtype=torch.float64)
        step = 1 << 20
        for r0 in range(0, M, step):
            blk = yc[r0:r0 + step].double()
            s += blk.sum(0)
            q += (blk * blk).sum(0)
        mu = s / M
        d2 = torch.zeros(C, dtype=torch.float64)
        for r0 in range(0, M, step):              # two-pass variance in float64
            d2 += (yc[r0:r0 + step].double() - mu).pow(2).sum(0)
        var = d2 / M
        r = torch.sqrt(mu.abs().pow(2) / var.clamp_min(1e-300))
        for c in range(C):
            name, ratio, _ = N.CLASSES[c % N.NCLS]
            if ratio:
                assert 0.75 * ratio <= float(r[c]) <= 1.25 * ratio, (route, c, name, float(r[c]))
        ref = {'mean': mu, 'var': var, 'invstd': (var + N.EPS).rsqrt(), 'running_mean': (1 - MOM) * rm0.double() + MOM * mu,
               'running_var': (1 - MOM) * rv0.double() + MOM * var * M / (M - 1)}
        for a, b in slices:
            blk = yc[a:b].double()
            out = (blk - mu) * ref['invstd'] * gamma.double() + beta.double()
            if relu:
                out = out * _gate(mask[a * C // n:b * C // n], b - a, C, dt)
            N.judge_out(led, route, dt, classes, out, z[a:b])
    got = {'mean': mean, 'invstd': invstd, 'running_mean': rm, 'running_var': rv}
    N.judge_stats(led, route, dt, classes, ref, got)
    _stats_of_stored(led, route, dt, yc, yu, invstd.double().cpu().pow(-2) - N.EPS)
    if bwd is None:
        return

    # ---- backward
    dres = torch.empty_like(y)
    dx = torch.empty_like(y)
    dgamma, dbeta = torch.full((C,), float('nan'), device=dev), torch.full((C,), float('nan'), device=dev)
    broute = f'{route}>{bwd}'
    if bwd == 'reduce':
        dz = torch.randn(M, C, generator=g).to(dt).cuda()
        ws = torch.empty(L.saicv_bn_bwd_ws_floats(M, C, code), device=dev)
        check(L.saicv_bn_act_bwd(code, ptr(dz), 0, ptr(mask), ptr(y), ptr(gm), ptr(mean), ptr(invstd), ptr(dx), ptr(dres), ptr(dgamma),
                                 ptr(dbeta), M, C, relu, 0, ptr(ws), st), 'bn_act_bwd')
    else:
        from simpleaicv_pytorch_training_examples_amd import ops
        K2 = dgrad
        d2 = ops._desc(1, 1, M, C, K2, 1, 1, 1, 0, dt)                    # the convolution that consumes z: [M][C] -> [M][K2]
        dy2 = torch.randn(M, K2, generator=g).to(dt).cuda()
        wd = (torch.randn(C, K2, generator=g) / math.sqrt(K2)).to(dt).cuda()
        dz = torch.empty_like(y)
        prow = L.saicv_conv2d_dgrad_stat_rows(ctypes.byref(d2))
        assert prow == _plan(d2, 0, _lib.PLAN_CONV_DGRAD, 1).stat_rows
        arows = 0 if bwd == 'partials' else min(8, max(1, prow))
        nrow = prow if bwd == 'partials' else arows
        parts = torch.zeros(2, nrow, C, device=dev)
        f = _lib.DgradFuse(0, 0, ptr(y), ptr(mask), ptr(mean), ptr(invstd), ptr(parts[0]), ptr(parts[1]), arows, 0)
        check(L.saicv_conv2d_dgrad_fused(ctypes.byref(d2), ptr(dy2), ptr(wd), ctypes.byref(f), ptr(dz), st), 'dgrad_fused')
        if bwd == 'inline':
            check(L.saicv_bn_act_bwd_inline(code, ptr(dz), ptr(mask), ptr(y), ptr(gm), ptr(mean), ptr(invstd), ptr(parts[0]), ptr(parts[1]),
                                            nrow, ptr(dx), ptr(dres), ptr(dgamma), ptr(dbeta), M, C, relu, 0, st), 'bn_act_bwd_inline')
        else:
            ws = torch.empty(L.saicv_bn_bwd_ws_floats(M, C, code), device=dev)
            check(L.saicv_bn_act_bwd_from_partials(code, ptr(dz), ptr(mask), ptr(y), ptr(gm), ptr(mean), ptr(invstd), ptr(parts[0]),
                                                   ptr(parts[1]), nrow, ptr(dx), ptr(dres), ptr(dgamma), ptr(dbeta), M, C, relu, 0,
                                                   ptr(ws), st), 'bn_act_bwd_from_partials')
    torch.cuda.synchronize()
    refb = N.bn_bwd_ref(yc, dz.cpu(), gamma, mean.cpu(), invstd.cpu(), _gate(mask, M, C, dt) if relu else None)
    N.judge_grads(led, broute, dt, classes, refb, {'dx': dx, 'dres': dres, 'dgamma': dgamma, 'dbeta': dbeta})


@pytest.mark.parametrize('dt', DTYPES, ids=IDS)
@pytest.mark.parametrize('det', [False, True], ids=['atomic', 'deterministic'])
@pytest.mark.parametrize('count', [8, 4096])
def test_bn_stats_finalize_act_route(dt, det, count):
    """saicv_bn_stats -> saicv_bn_finalize_fwd (1 row) -> saicv_bn_act_fwd -> saicv_bn_act_bwd: ops.batch_norm2d's path.  A count of 8
    separates the biased from the unbiased variance by 12 %."""
    from simpleaicv_pytorch_training_examples_amd import ops
    _lib, L, st = _L()
    C = 8 * N.NCLS
    y = N.build_slabs(C, count, dt, seed=count)[0].t().contiguous().cuda()
    prev = ops.set_deterministic(det)
    try:
        assert bool(L.saicv_get_deterministic()) == det
        stat = torch.zeros(2, 1, C, device='cuda')
        _lib.check(L.saicv_bn_stats(_lib.dtype_code(dt), _lib.ptr(y), count, C, _lib.ptr(stat[0]), _lib.ptr(stat[1]), st), 'bn_stats')
    finally:
        ops.set_deterministic(prev)
    led = N.Ledger()
    _bn_chain(led, f'bn_stats/{_tag(dt)}', dt, y, N.slab_classes(C), stat, 1, 'finalize', 'reduce', seed=count + 3)
    # the dead class without a residual or a ReLU: the output IS beta
    _bn_chain(led, f'bn_stats/{_tag(dt)}', dt, y, N.slab_classes(C), stat, 1, 'finalize', None, seed=count + 4, relu=0, with_res=False)
    _finish(led)


# (n, h, w, cin, K, k, pad), the route and statistics rows saicv_igemm_plan must give per dtype (fp32, bf16), what consumes them
CONV_ROWS = [
    ((2, 32, 32, 16, 88, 1, 0), ('tiled', 'tiled'), 'P <= 32'),
    ((16, 64, 64, 16, 88, 1, 0), ('tiled', 'tiled'), 'P <= 1024'),
    ((16, 64, 64, 64, 64, 1, 0), ('tiled', 'pw'), 'P <= 1024'),
    ((16, 64, 64, 64, 64, 3, 1), ('tiled', 'pw3'), 'P <= 1024'),
]


def _conv_fwd(dt, shape, seed, atomic_rows=0):
    """-> y [M][K] (device), stat [2][rows][K], rows, classes, the plan, the unrounded float64 product (1 x 1 only)"""
    from simpleaicv_pytorch_training_examples_amd import ops
    _lib, L, st = _L()
    n, h, w, cin, K, k, pad = shape
    x, wf, classes = _conv_operands(dt, n, h, w, cin, K, k, seed)
    d = ops._desc(n, h, w, cin, K, k, k, 1, pad, dt)
    pl = _plan(d)
    M = n * h * w
    yu = x.double().view(M, cin) @ wf.double().view(K, cin).t() if k == 1 and M <= (1 << 17) else None
    xd, wd = x.cuda(), wf.cuda()
    y = torch.empty(M, K, dtype=dt, device='cuda')
    if atomic_rows:
        rows = atomic_rows
        stat = torch.zeros(2, rows, K, device='cuda')
        _lib.check(L.saicv_conv2d_fwd_stats(ctypes.byref(d), _lib.ptr(xd), _lib.ptr(wd), _lib.ptr(y), _lib.ptr(stat[0]), _lib.ptr(stat[1]), rows,
                                            st), 'conv2d_fwd_stats')
    else:
        rows = L.saicv_conv2d_stat_rows(ctypes.byref(d))
        assert rows == pl.stat_rows
        stat = torch.full((2, rows + 1, K), float('nan'), device='cuda')            # one guard row
        _lib.check(L.saicv_conv2d_fwd(ctypes.byref(d), _lib.ptr(xd), _lib.ptr(wd), 0, _lib.ptr(y), 0, _lib.ptr(stat[0]), _lib.ptr(stat[1]), st),
                   'conv2d_fwd')
        torch.cuda.synchronize()
        assert bool(torch.isnan(stat[:, rows]).all()) and bool(torch.isfinite(stat[:, :rows]).all()), 'partial rows / guard row'
        stat = stat[:, :rows].contiguous()
    return y, stat, rows, classes, pl, yu


def _route_name(pl):
    _lib = _L()[0]
    return {_lib.ROUTE_TILED: 'tiled', _lib.ROUTE_PW_STREAM: 'pw', _lib.ROUTE_PW3_STREAM: 'pw3'}[pl.route]


@pytest.mark.parametrize('dt', DTYPES, ids=IDS)
@pytest.mark.parametrize('case', CONV_ROWS, ids=[f'{c[0][3]}to{c[0][4]}_k{c[0][5]}_m{c[0][0] * c[0][1] * c[0][2]}' for c in CONV_ROWS])
def test_conv_partial_rows_finalize_route(dt, case):
    """saicv_conv2d_fwd, one statistics row per tile row (per workgroup on the streaming forms) -> saicv_bn_finalize_fwd -> saicv_bn_act_fwd,
    backward through saicv_conv2d_dgrad_fused's partial rows -> saicv_bn_act_bwd_from_partials."""
    shape, routes, regime = case
    y, stat, rows, classes, pl, yu = _conv_fwd(dt, shape, seed=shape[0] + shape[4] + shape[5])
    assert _route_name(pl) == routes[DTYPES.index(dt)], (_route_name(pl), pl.stat_rows)
    assert (rows <= 32) if regime == 'P <= 32' else (32 < rows <= 1024), (rows, regime)
    led = N.Ledger()
    _bn_chain(led, f'conv_rows:{_route_name(pl)}/{_tag(dt)}', dt, y, classes, stat, rows, 'finalize', 'partials', seed=rows, yu=yu, dgrad=64)
    _finish(led)


@pytest.mark.parametrize('dt', DTYPES, ids=IDS)
@pytest.mark.parametrize('rows', [1, 2, 4, 8])
@pytest.mark.parametrize('fwd', ['inline', 'join'])
def test_conv_atomic_rows_inline_route(dt, rows, fwd):
    """saicv_conv2d_fwd_stats (1, 2, 4, 8 atomically accumulated rows) -> saicv_bn_act_fwd_stats / saicv_bn_act_fwd_join, backward through
    saicv_conv2d_dgrad_fused's atomic rows -> saicv_bn_act_bwd_inline.  The tile rows exceed the atomic rows: every row is shared."""
    shape = (4, 32, 32, 16, 88, 1, 0)
    y, stat, _, classes, pl, yu = _conv_fwd(dt, shape, seed=rows + 17, atomic_rows=rows)
    assert _route_name(pl) == 'tiled' and pl.stat_rows >= 2 * rows, (pl.route, pl.stat_rows)
    led = N.Ledger()
    _bn_chain(led, f'conv_atomic{rows}>{fwd}/{_tag(dt)}', dt, y, classes, stat, rows, fwd, 'inline', seed=rows + 5, yu=yu, dgrad=64)
    _finish(led)


@pytest.mark.parametrize('dt', [torch.bfloat16], ids=['bf16'])
@pytest.mark.parametrize('form', ['pw', 'pw3'])
def test_streaming_forms_with_atomic_rows(dt, form):
    """pw_stream / pw3_stream (bf16 only; tests/test_gpu_layers_b256.py has their fp32 twins on the tiled kernel) adding their
    per-workgroup sums into 8 atomic rows -> saicv_bn_act_fwd_stats."""
    shape = (16, 64, 64, 64, 64, 1, 0) if form == 'pw' else (16, 64, 64, 64, 64, 3, 1)
    y, stat, _, classes, pl, yu = _conv_fwd(dt, shape, seed=29, atomic_rows=8)
    assert _route_name(pl) == form, _route_name(pl)
    led = N.Ledger()
    _bn_chain(led, f'{form}_atomic8>inline/bf16', dt, y, classes, stat, 8, 'inline', 'inline', seed=31, yu=yu, dgrad=64)
    _finish(led)


BIG = [('stage', (256, 56, 56, 16, 64, 1, 0)), ('stem', (256, 112, 112, 16, 64, 1, 0))]


@pytest.mark.timeout(600)
@pytest.mark.parametrize('dt', DTYPES, ids=IDS)
@pytest.mark.parametrize('name,shape', BIG, ids=[b[0] for b in BIG])
def test_resnet_sized_counts(dt, name, shape):
    """A stage-sized count (256 x 56 x 56 pixels x 64 channels) through the production default -- ops._stat_rows atomic rows, finalised
    inside saicv_bn_act_fwd_stats -- and the stem's count (256 x 112 x 112 x 64, bf16) through one row per tile row, the two-kernel finalize
    (P > 1024) and saicv_bn_act_fwd.  Statistics over the whole stored tensor, the output on its first and last 4096 rows."""
    if name == 'stem' and dt == torch.float32:
        shape = (64,) + shape[1:]                 # the fp32 twin keeps P > 1024 at a quarter of the bytes
    M = shape[0] * shape[1] * shape[2]
    led = N.Ledger()
    if name == 'stage':
        from simpleaicv_pytorch_training_examples_amd import ops
        n, h, w, cin, K, k, pad = shape
        arows = ops._stat_rows(_plan(ops._desc(n, h, w, cin, K, k, k, 1, pad, dt)).stat_rows)          # what ops.conv_bn_act takes
        y, stat, rows, classes, pl, _ = _conv_fwd(dt, shape, seed=56, atomic_rows=arows)
        assert pl.stat_rows == 6272
        _bn_chain(led, f'stage_count_atomic{arows}>inline/{_tag(dt)}', dt, y, classes, stat, arows, 'inline', None, seed=57,
                  slices=[(0, 4096), (M - 4096, M)])
    else:
        y, stat, rows, classes, pl, _ = _conv_fwd(dt, shape, seed=112)
        assert rows > 1024, rows
        _bn_chain(led, f'stem_count_rows{rows}>finalize/{_tag(dt)}', dt, y, classes, stat, rows, 'finalize', None, seed=113,
                  slices=[(0, 4096), (M - 4096, M)])
    _finish(led)


@pytest.mark.parametrize('dt', DTYPES, ids=IDS)
@pytest.mark.parametrize('det', [False, True], ids=['atomic', 'deterministic'])
def test_stem_bn_relu_maxpool_route(dt, det):
    """saicv_bn_stats -> saicv_bn_finalize_fwd -> saicv_bn_relu_maxpool_fwd / _bwd (the stem: BatchNorm + ReLU + MaxPool2d(3, 2, 1) in one
    pass each way; the backward's channel sums are fp32 atomics, ordered in deterministic mode)."""
    from simpleaicv_pytorch_training_examples_amd import ops
    _lib, L, st = _L()
    check, ptr, code = _lib.check, _lib.ptr, _lib.dtype_code(dt)
    n, h, w, C = 4, 16, 16, 64
    oh, ow = h // 2, w // 2
    M = n * h * w
    classes = N.slab_classes(C)
    y = N.build_slabs(C, M, dt, seed=77)[0].t().contiguous().cuda()                  # [n * h * w][C]
    gamma, beta, rm0, rv0 = _affine(C, 78)
    g = torch.Generator().manual_seed(79)
    dout = torch.randn(n * oh * ow, C, generator=g).to(dt)
    gm, bt = gamma.cuda(), beta.cuda()
    stat = torch.zeros(2, 1, C, device='cuda')
    mean, invstd, scale, shift = (torch.empty(C, device='cuda') for _ in range(4))
    ws = torch.empty(L.saicv_bn_ws_floats(C), device='cuda')
    out = torch.empty(n * oh * ow, C, dtype=dt, device='cuda')
    idx = torch.empty(n * oh * ow, C, dtype=torch.uint8, device='cuda')
    dy = torch.empty_like(y)
    dgamma, dbeta = torch.full((C,), float('nan'), device='cuda'), torch.full((C,), float('nan'), device='cuda')
    ws2 = torch.empty(L.saicv_bn_relu_maxpool_bwd_ws_floats(C), device='cuda')
    dd = dout.cuda()
    prev = ops.set_deterministic(det)
    try:
        check(L.saicv_bn_stats(code, ptr(y), M, C, ptr(stat[0]), ptr(stat[1]), st), 'bn_stats')
        check(L.saicv_bn_finalize_fwd(ptr(stat[0]), ptr(stat[1]), 1, C, float(M), ptr(gm), ptr(bt), 0, 0, MOM, N.EPS, ptr(mean), ptr(invstd),
                                      ptr(scale), ptr(shift), ptr(ws), 0, st), 'finalize')
        check(L.saicv_bn_relu_maxpool_fwd(code, ptr(y), ptr(scale), ptr(shift), ptr(out), ptr(idx), n, h, w, C, oh, ow, 3, 2, 1, st), 'pool_fwd')
        check(L.saicv_bn_relu_maxpool_bwd(code, ptr(dd), ptr(idx), ptr(y), ptr(gm), ptr(mean), ptr(invstd), ptr(scale), ptr(shift), ptr(dy),
                                          ptr(dgamma), ptr(dbeta), 0, ptr(ws2), n, h, w, C, oh, ow, 3, 2, 1, st), 'pool_bwd')
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(prev)
    route = f'stem_pool/{_tag(dt)}'
    yc = y.cpu()
    N.assert_ratios(yc.t(), route)
    ref = N.bn_ref(yc, gamma, beta)
    pre = ref['out'].view(n, h, w, C).permute(0, 3, 1, 2).clone().requires_grad_(True)
    pooled = F.max_pool2d(F.relu(pre), 3, 2, 1)
    pooled.backward(dout.double().view(n, oh, ow, C).permute(0, 3, 1, 2))
    gflow = pre.grad.permute(0, 2, 3, 1).reshape(M, C)                                # the gradient reaching the BatchNorm output
    led = N.Ledger()
    N.judge_stats(led, route, dt, classes, ref, {'mean': mean, 'invstd': invstd})
    N.judge_out(led, route, dt, classes, pooled.detach().permute(0, 2, 3, 1).reshape(-1, C), out)
    refb = N.bn_bwd_ref(yc, gflow, gamma, mean.cpu(), invstd.cpu())
    N.judge_grads(led, route + '>pool_bwd', dt, classes, refb, {'dx': dy, 'dgamma': dgamma, 'dbeta': dbeta})
    _finish(led)


# ------------------------------------------------------------------------------ GroupNorm, LayerNorm
GN_CASES = [(2, 2, 2, 256, 32), (2, 16, 16, 256, 32), (3, 8, 8, 64, 8)]


@pytest.mark.parametrize('dt', DTYPES, ids=IDS)
@pytest.mark.parametrize('det', [False, True], ids=['atomic', 'deterministic'])
@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('case', GN_CASES, ids=[f'n{c[0]}_{c[1]}x{c[2]}_c{c[3]}g{c[4]}' for c in GN_CASES])
def test_groupnorm_routes(dt, det, relu, case):
    """saicv_groupnorm_fwd / _bwd with the offset per (sample, group): the FCOS head's GroupNorm(32, 256), on a 2 x 2 map too."""
    from simpleaicv_pytorch_training_examples_amd import ops
    _lib, L, st = _L()
    check, ptr, code = _lib.check, _lib.ptr, _lib.dtype_code(dt)
    n, h, w, C, G = case
    hw, cpg = h * w, C // G
    # slab (sample, group) has class group % NCLS in every sample: lay the slabs out group-major so that slab index % NCLS follows the group
    # slab (sample i, group g) takes the class of g in every sample (dgamma / dbeta of a channel then sum over one class)
    xs = torch.stack([N.build_slabs(G, hw * cpg, dt, seed=hw + C + i)[0] for i in range(n)])      # [n][G][hw * cpg]
    for i in range(n):
        N.assert_ratios(xs[i], 'groupnorm')
    x = xs.view(n, G, hw, cpg).permute(0, 2, 1, 3).reshape(n, hw, C).contiguous()     # NHWC
    g = torch.Generator().manual_seed(C + hw)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5
    dyh = torch.randn(n, hw, C, generator=g).to(dt)
    xd, dyd, gm, bt = x.cuda(), dyh.cuda(), gamma.cuda(), beta.cuda()
    y = torch.empty_like(xd)
    dx = torch.empty_like(xd)
    mean_rstd = torch.empty(2, n, G, device='cuda')
    ab = torch.empty(2, n, C, device='cuda')
    ws = torch.empty(L.saicv_groupnorm_ws_floats(n, C), device='cuda')
    dgamma, dbeta = torch.zeros(C, device='cuda'), torch.zeros(C, device='cuda')
    prev = ops.set_deterministic(det)
    try:
        check(L.saicv_groupnorm_fwd(code, ptr(xd), ptr(gm), ptr(bt), ptr(y), ptr(mean_rstd), ptr(ab), ptr(ws), n, hw, C, G, N.EPS, relu, st), 'gn_fwd')
        check(L.saicv_groupnorm_bwd(code, ptr(dyd), ptr(xd), ptr(gm), ptr(mean_rstd), ptr(ab), ptr(dx), ptr(dgamma), ptr(dbeta), ptr(ws), n, hw, C,
                                    G, relu, st), 'gn_bwd')
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(prev)
    route = f'groupnorm{"+relu" if relu else ""}/{_tag(dt)}'
    # float64: per (sample, group) slab [hw * cpg]
    s64 = xs.double().view(n * G, hw * cpg)
    mu, var = N.realised(s64)
    rstd = (var + N.EPS).rsqrt()
    gam_s = gamma.double().view(G, 1, cpg).expand(G, hw, cpg).reshape(G, -1).repeat(n, 1)      # per-slab element gamma / beta
    bet_s = beta.double().view(G, 1, cpg).expand(G, hw, cpg).reshape(G, -1).repeat(n, 1)
    pre = (s64 - mu[:, None]) * rstd[:, None] * gam_s + bet_s
    ys = y.cpu().view(n, hw, G, cpg).permute(0, 2, 1, 3).reshape(n * G, -1)
    gate = (ys.double() > 0).double() if relu else torch.ones_like(pre)
    slab_cls = [N.group_of(i % G) for i in range(n * G)]
    led = N.Ledger()
    N.judge_stats(led, route, dt, slab_cls, {'mean': mu, 'var': var}, {'mean': mean_rstd[0].flatten(), 'invstd': mean_rstd[1].flatten()})
    N.judge_out(led, route, dt, slab_cls, pre * gate, ys, slab_dim=0)
    # backward from the saved statistics
    md, rd = mean_rstd[0].flatten().double().cpu(), mean_rstd[1].flatten().double().cpu()
    gs = dyh.double().view(n, hw, G, cpg).permute(0, 2, 1, 3).reshape(n * G, -1) * gate
    xh = (s64 - md[:, None]) * rd[:, None]
    gg = gs * gam_s
    dxs = rd[:, None] * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
    dxd = dx.cpu().view(n, hw, G, cpg).permute(0, 2, 1, 3).reshape(n * G, -1)
    N.judge_grads(led, route, dt, slab_cls, {'dx': dxs}, {'dx': dxd}, slab_dim=0)
    # dgamma / dbeta per channel (sums over samples): the channel's class is its group's
    dg = (gs * xh).view(n, G, hw, cpg).sum((0, 2)).flatten()
    db = gs.view(n, G, hw, cpg).sum((0, 2)).flatten()
    ch_cls = [N.group_of(c // cpg) for c in range(C)]
    N.judge_grads(led, route, dt, ch_cls, {'dgamma': dg, 'dbeta': db}, {'dgamma': dgamma, 'dbeta': dbeta})
    _finish(led)


@pytest.mark.parametrize('dt', DTYPES, ids=IDS)
@pytest.mark.parametrize('C', [256, 768])
@pytest.mark.parametrize('fused', [False, True], ids=['layernorm', 'dropout_add_layernorm_p0'])
def test_layernorm_two_pass_control(dt, C, fused):
    """saicv_layernorm_fwd / _bwd and saicv_dropout_add_layernorm_fwd at p = 0 with the row offset swept like the channels above: the
    two-pass kernels must hold the class-0 bounds at every class (c128 included, recorded)."""
    _lib, L, st = _L()
    check, ptr, code = _lib.check, _lib.ptr, _lib.dtype_code(dt)
    M = 4 * N.NCLS
    x = N.build_slabs(M, C, dt, seed=C)[0]
    g = torch.Generator().manual_seed(C + 1)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5
    dyh = torch.randn(M, C, generator=g).to(dt)
    gm, bt = gamma.cuda(), beta.cuda()
    xd = x.cuda()
    y = torch.empty_like(xd)
    mean, rstd = torch.empty(M, device='cuda'), torch.empty(M, device='cuda')
    cls = N.slab_classes(M)
    route = f'{"dropout_add_" if fused else ""}layernorm/{_tag(dt)}'
    if fused:
        zero = torch.zeros_like(xd)
        summed = torch.empty_like(xd)
        check(L.saicv_dropout_add_layernorm_fwd(code, ptr(xd), ptr(zero), 0.0, 7, 0, ptr(gm), ptr(bt), ptr(summed), ptr(y), ptr(mean), ptr(rstd),
                                                M, C, N.EPS, st), 'dropout_add_layernorm_fwd')
        torch.cuda.synchronize()
        assert torch.equal(summed.cpu(), x), 'x + 0 at p = 0 must be x'
    else:
        check(L.saicv_layernorm_fwd(code, ptr(xd), ptr(gm), ptr(bt), ptr(y), ptr(mean), ptr(rstd), M, C, N.EPS, st), 'layernorm_fwd')
    N.assert_ratios(x, route)
    mu, var = N.realised(x)
    r = (var + N.EPS).rsqrt()
    ref = (x.double() - mu[:, None]) * r[:, None] * gamma.double() + beta.double()
    led = N.Ledger()
    N.judge_stats(led, route, dt, cls, {'mean': mu, 'var': var}, {'mean': mean, 'invstd': rstd})
    N.judge_out(led, route, dt, cls, ref, y, slab_dim=0)
    # two-pass: the class-0 bound holds at EVERY class, c128 included
    b0 = N.bounds('c0', dt)
    for (rt, group, qty, err, _) in list(led.rows):
        if group in ('c32', 'c128') and qty in ('mean', 'var', 'out'):
            led.add(rt + ' (two-pass control)', group, qty, err, b0['out'] if qty == 'out' else b0[qty])
    if not fused:
        dx = torch.empty_like(xd)
        dgamma, dbeta = torch.full((C,), float('nan'), device='cuda'), torch.full((C,), float('nan'), device='cuda')
        ws = torch.empty(L.saicv_layernorm_bwd_ws_floats(M, C), device='cuda')
        dyd = dyh.cuda()
        check(L.saicv_layernorm_bwd(code, ptr(dyd), ptr(xd), ptr(gm), ptr(mean), ptr(rstd), 0, ptr(dx), ptr(dgamma), ptr(dbeta), ptr(ws), M, C, 0,
                                    st), 'layernorm_bwd')
        torch.cuda.synchronize()
        md, rd = mean.double().cpu(), rstd.double().cpu()
        xh = (x.double() - md[:, None]) * rd[:, None]
        gg = dyh.double() * gamma.double()
        dxr = rd[:, None] * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
        N.judge_grads(led, route, dt, cls, {'dx': dxr}, {'dx': dx}, slab_dim=0)
        # dgamma / dbeta sum over rows of every class: one bound, the dtype's gradient tolerance
        from conftest import rel_err
        led.add(route, 'all', 'dgamma', rel_err(dgamma, (dyh.double() * xh).sum(0)), b0['grad'])
        led.add(route, 'all', 'dbeta', rel_err(dbeta, dyh.double().sum(0)), b0['grad'])
    _finish(led)


# ------------------------------------------------------------------------------ the finalize kernels, directly
FIN_P = [1, 4, 31, 32, 33, 100, 1023, 1024, 1025, 3136, 6272, 6273]
FIN_C = [4, 60, 64, 72, 200, 2048, 2056]
GUARD = 64


def _synthetic_rows(P, C, count, seed):
    """fp32 partial rows [P][C] of sum and sum of squares whose float64 column sums belong to channels of the builder's classes"""
    g = torch.Generator().manual_seed(seed)
    mean, std = N.slab_params(C)
    var = std * std if count > 1 else torch.zeros(C, dtype=torch.float64)
    S, Q = count * mean, count * (var + mean * mean)
    wgt = torch.rand(P, C, dtype=torch.float64, generator=g) + 0.5
    wgt = wgt / wgt.sum(0)
    a, b = (S * wgt).float(), (Q * wgt).float()
    return a, b


def _guarded(C, fill=None):
    """-> (buffer with GUARD NaN floats either side, the [C] view between them)"""
    buf = torch.full((C + 2 * GUARD,), float('nan'), device='cuda')
    if fill is not None:
        buf[GUARD:GUARD + C] = fill.cuda()
    return buf, buf[GUARD:GUARD + C]


def _guards_intact(buf, C):
    return bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + C:]).all())


@pytest.mark.parametrize('P', FIN_P)
@pytest.mark.parametrize('single', [False, True], ids=['count256P', 'count1'])
def test_bn_finalize_fwd_directly(P, single):
    """saicv_bn_finalize_fwd on synthetic partial rows: P on both sides of 32 (one batch of the four-wave kernel), of 1024 (the
    sixteen-wave kernel) and beyond (bn_reduce_partials_kernel with ragged rows_per); C below, at and off the 64-channel block and
    on both sides of 2048; gamma / beta and the running statistics present and NULL; a count of 1 (the variance is exactly 0 whatever the
    mean: with fp32 q / n - mean^2 the rounding of mean^2 alone is up to 70 x eps at |mean| = 64) and a count above it.  Outputs,
    running buffers and the workspace tail carry NaN guard bands."""
    _lib, L, st = _L()
    check, ptr = _lib.check, _lib.ptr
    led = N.Ledger()
    for C in FIN_C:
        for count in ((1,) if single else (P * 256,)):
            a, b = _synthetic_rows(P, C, count, seed=P * 7 + C)
            ad, bd = a.cuda(), b.cuda()
            s64, q64 = a.double().sum(0), b.double().sum(0)
            mean_r = s64 / count
            var_r = (q64 / count - mean_r * mean_r).clamp_min(0)
            if count == 1:
                # one sample per channel has variance 0 by definition; q - s^2 of the fp32-ROUNDED rows is their rounding (up to
                # 1e-7 * mean^2, either sign), not a property of the channel
                var_r = torch.zeros_like(var_r)
            classes = N.slab_classes(C)
            for affine in (True, False):
                for running in (True, False):
                    gamma, beta, rm0, rv0 = _affine(C, C + P)
                    bufs = {k: _guarded(C) for k in ('mean', 'invstd', 'scale', 'shift')}
                    rmb, rm = _guarded(C, rm0)
                    rvb, rv = _guarded(C, rv0)
                    nws = L.saicv_bn_ws_floats(C)
                    ws = torch.full((nws + GUARD,), float('nan'), device='cuda')
                    nbt = torch.tensor([6], dtype=torch.int64, device='cuda')
                    gm, bt = (gamma.cuda(), beta.cuda()) if affine else (None, None)
                    check(L.saicv_bn_finalize_fwd(ptr(ad), ptr(bd), P, C, float(count), ptr(gm), ptr(bt), ptr(rm) if running else 0,
                                                  ptr(rv) if running else 0, MOM, N.EPS, ptr(bufs['mean'][1]), ptr(bufs['invstd'][1]),
                                                  ptr(bufs['scale'][1]), ptr(bufs['shift'][1]), ptr(ws), ptr(nbt) if running else 0, st), 'finalize')
                    torch.cuda.synchronize()
                    route = f'finalize_fwd P={P} C={C} count={count} affine={int(affine)} running={int(running)}'
                    for k, (buf, _) in bufs.items():
                        led.require(_guards_intact(buf, C), f'{route}: guard band of {k} overwritten')
                    led.require(bool(torch.isnan(ws[nws:]).all()), f'{route}: workspace tail overwritten')
                    led.require(int(nbt) == (7 if running else 6), f'{route}: num_batches_tracked {int(nbt)}')
                    ref = {'mean': mean_r, 'var': var_r}
                    got = {'mean': bufs['mean'][1], 'invstd': bufs['invstd'][1]}
                    if running:
                        led.require(_guards_intact(rmb, C) and _guards_intact(rvb, C), f'{route}: guard band of the running statistics overwritten')
                        unb = var_r * count / (count - 1) if count > 1 else var_r
                        ref['running_mean'] = (1 - MOM) * rm0.double() + MOM * mean_r
                        ref['running_var'] = (1 - MOM) * rv0.double() + MOM * unb
                        got['running_mean'], got['running_var'] = rm, rv
                    else:
                        led.require(torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0), f'{route}: running statistics touched')
                    N.judge_stats(led, 'finalize_fwd_direct', torch.float32, classes, ref, got)
                    # scale / shift from the device's own mean / invstd (fp32 roundings of two products)
                    md, iv = got['mean'].double().cpu(), got['invstd'].double().cpu()
                    g64 = gamma.double() if affine else torch.ones(C, dtype=torch.float64)
                    b64 = beta.double() if affine else torch.zeros(C, dtype=torch.float64)
                    sc, sh = bufs['scale'][1].double().cpu(), bufs['shift'][1].double().cpu()
                    led.require(bool(((sc - g64 * iv).abs() <= 1e-6 * (g64 * iv).abs()).all()), f'{route}: scale != gamma * invstd')
                    shr = b64 - md * g64 * iv
                    led.require(bool(((sh - shr).abs() <= 1e-6 * (b64.abs() + (md * g64 * iv).abs()) + 1e-30).all()), f'{route}: shift != beta - mean * scale')
            led.require(torch.equal(ad.cpu(), a) and torch.equal(bd.cpu(), b), f'finalize_fwd P={P} C={C} count={count}: partial rows modified')
    _finish(led)


@pytest.mark.parametrize('P', FIN_P)
@pytest.mark.parametrize('dt', DTYPES, ids=IDS)
def test_bn_act_bwd_from_partials_directly(P, dt):
    """The same row counts through saicv_bn_act_bwd_from_partials: dgamma / dbeta are the float64 column sums of the rows it is given,
    dx follows from them; outputs and the workspace tail carry NaN guard bands."""
    _lib, L, st = _L()
    check, ptr, code = _lib.check, _lib.ptr, _lib.dtype_code(dt)
    led = N.Ledger()
    M = 64
    for C in (64, 200):
        g = torch.Generator().manual_seed(P + C)
        y = N.build_slabs(C, M, dt, seed=P + C)[0].t().contiguous()
        mu, var = N.realised(y.t())
        mean, invstd = mu.float(), (var + N.EPS).rsqrt().float()
        dz = torch.randn(M, C, generator=g).to(dt)
        gamma = torch.rand(C, generator=g) + 0.5
        wgt = torch.rand(P, C, dtype=torch.float64, generator=g) + 0.5
        wgt = wgt / wgt.sum(0)
        ref0 = N.bn_bwd_ref(y, dz, gamma, mean, invstd)
        pg, pgx = (ref0['dbeta'] * wgt).float(), (ref0['dgamma'] * wgt).float()
        sg, sx = pg.double().sum(0), pgx.double().sum(0)
        xhat = (y.double() - mean.double()) * invstd.double()
        dxr = gamma.double() * invstd.double() * (dz.double() - sg / M - xhat * sx / M)
        nws = L.saicv_bn_bwd_ws_floats(M, C, code)
        ws = torch.full((nws + GUARD,), float('nan'), device='cuda')
        dgb, dgamma = _guarded(C)
        dbb, dbeta = _guarded(C)
        dx = torch.full((M + 2, C), float('nan'), dtype=dt, device='cuda')
        yd, dzd, gm, md, ivd, pgd, pgxd = y.cuda(), dz.cuda(), gamma.cuda(), mean.cuda(), invstd.cuda(), pg.cuda(), pgx.cuda()
        check(L.saicv_bn_act_bwd_from_partials(code, ptr(dzd), 0, ptr(yd), ptr(gm), ptr(md), ptr(ivd), ptr(pgd), ptr(pgxd), P, ptr(dx[1]), 0,
                                               ptr(dgamma), ptr(dbeta), M, C, 0, 0, ptr(ws), st), 'from_partials')
        torch.cuda.synchronize()
        route = f'bwd_from_partials_direct/{_tag(dt)}'
        what = f'{route} P={P} C={C}'
        led.require(_guards_intact(dgb, C) and _guards_intact(dbb, C), f'{what}: guard band of dgamma / dbeta overwritten')
        led.require(bool(torch.isnan(dx[0]).all() and torch.isnan(dx[M + 1]).all()), f'{what}: guard rows of dx overwritten')
        led.require(bool(torch.isnan(ws[nws:]).all()), f'{what}: workspace tail overwritten')
        led.require(torch.equal(pgd.cpu(), pg) and torch.equal(pgxd.cpu(), pgx), f'{what}: partial rows modified')
        # the sums are plain fp32 column sums of fp32 rows: the fp32 gradient tolerance whatever the activations' dtype
        cls = N.slab_classes(C)
        N.judge_grads(led, route, torch.float32, cls, {'dgamma': sx, 'dbeta': sg}, {'dgamma': dgamma, 'dbeta': dbeta})
        N.judge_grads(led, route, dt, cls, {'dx': dxr}, {'dx': dx[1:M + 1]})
    _finish(led)


def test_bn_act_fwd_stats_channel_limit():
    """The in-kernel finalize holds its coefficients in LDS: C = 2048 runs (64 statistics rows, the most it accepts), C = 2056 is
    refused with its error text."""
    _lib, L, st = _L()
    check, ptr = _lib.check, _lib.ptr
    dt = torch.float32
    M, rows = 16, 64
    led = N.Ledger()
    for C in (2048, 2056):
        y = N.build_slabs(C, M, dt, seed=C)[0].t().contiguous()
        a, b = torch.zeros(rows, C, dtype=torch.float64), torch.zeros(rows, C, dtype=torch.float64)
        a[torch.arange(M) % rows] += y.double()                  # row m of y lands in statistics row m % rows
        b[torch.arange(M) % rows] += y.double() ** 2
        a, b = a.float(), b.float()
        gamma, beta, rm0, rv0 = _affine(C, C)
        yd, ad, bd, gm, bt, rm, rv = (t.cuda() for t in (y, a, b, gamma, beta, rm0, rv0))
        z = torch.full((M + 2, C), float('nan'), device='cuda')
        mean, invstd = torch.full((C,), float('nan'), device='cuda'), torch.full((C,), float('nan'), device='cuda')
        nbt = torch.tensor([0], dtype=torch.int64, device='cuda')
        rc = L.saicv_bn_act_fwd_stats(1, ptr(yd), 0, ptr(z[1]), ptr(ad), ptr(bd), rows, float(M), ptr(gm), ptr(bt), ptr(rm), ptr(rv), MOM, N.EPS,
                                      ptr(nbt), ptr(mean), ptr(invstd), M, C, 0, 0, st)
        torch.cuda.synchronize()
        if C > 2048:
            assert rc != 0
            msg = L.saicv_last_error_string().decode()
            assert 'bn_act_fwd_stats: C=2056 must be a multiple of 4 and <= 2048' in msg, msg
            assert bool(torch.isnan(z).all() and torch.isnan(mean).all()) and int(nbt) == 0 and torch.equal(rm.cpu(), rm0)
            continue
        check(rc, 'bn_act_fwd_stats')
        assert int(nbt) == 1 and bool(torch.isnan(z[0]).all() and torch.isnan(z[M + 1]).all())
        s64, q64 = a.double().sum(0), b.double().sum(0)
        mr = s64 / M
        vr = (q64 / M - mr * mr).clamp_min(0)
        ref = N.bn_ref(y, gamma, beta, N.EPS, MOM, rm0, rv0)
        ref.update({'mean': mr, 'var': vr, 'invstd': (vr + N.EPS).rsqrt(), 'running_mean': (1 - MOM) * rm0.double() + MOM * mr,
                    'running_var': (1 - MOM) * rv0.double() + MOM * vr * M / (M - 1)})
        ref['out'] = (y.double() - mr) * ref['invstd'] * gamma.double() + beta.double()
        cls = N.slab_classes(C)
        N.judge_stats(led, 'fwd_stats_C2048_rows64', dt, cls, ref, {'mean': mean, 'invstd': invstd, 'running_mean': rm, 'running_var': rv})
        N.judge_out(led, 'fwd_stats_C2048_rows64', dt, cls, ref['out'], z[1:M + 1], beta)
    _finish(led)
