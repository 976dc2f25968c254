"""The human-matting kernels (csrc/matting.hip) against their float64 judges (tests/matting_common.py, themselves pinned to the
reference by tests/test_matting_host.py).  The kernels are called through the C-ABI on buffers that are NaN-filled and fenced by
guard elements, and through ops for the autograd surface.

Tolerances.  Pixel kernels: 1e-5 of the sum of the terms' magnitudes, per sum and per gradient element -- the project's bound for
such sums (tests/test_gpu_salient_kernels.py).  matting_fuse: bit-exact.  Pyramid, integer d0 and a dyadic table: bit-exact (every
entry is a multiple of 2^-20 that fp32 holds, the test asserts it on the judge).  Pyramid, float inputs: 8 x the deviation of the
REFERENCE's own fp32 run from the float64 judge for that case (recorded in the fixture), floor 16 fp32 epsilons, loss relative to
the loss and gradient relative to its largest element; the margin covers the other summation order (25 fused taps, one pyramid
of the difference, five chained levels).  Worst ratios are printed and recorded in DESIGN.md section 3p."""
import os

import numpy as np
import pytest
import torch

import matting_common as M
from conftest import ROOT

pytestmark = pytest.mark.gpu

GUARD, FENCE = 64, 12288.0
EPS32 = float(np.finfo(np.float32).eps)
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'pfan_mat_r18_tiny.pt')


def _ops():
    from simpleaicv_pytorch_training_examples_amd import _lib, ops
    return ops, _lib


def _fenced(shape, dtype=torch.float32):
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), FENCE, dtype=dtype, device='cuda')
    flat[GUARD:GUARD + n] = float('nan')
    return flat, flat[GUARD:GUARD + n].view(*shape)


def _check_fences(pairs):
    torch.cuda.synchronize()
    for flat, name in pairs:
        assert bool((flat[:GUARD] == FENCE).all()) and bool((flat[-GUARD:] == FENCE).all()), f'{name}: guard elements were written'
        assert not bool(torch.isnan(flat).any()), f'{name}: an element was left unwritten'


def _upstream(B, n):
    return torch.randn(B, n, generator=torch.Generator().manual_seed(B + n)) * torch.tensor([1., 3.][:n])


def _lo_hi():
    lo, hi = np.float32(M.LO), np.float32(M.HI)
    return torch.tensor([lo, hi, np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(1)), 0., 1.], dtype=torch.float32)


@pytest.fixture(scope='module')
def px_inputs():
    """the seeded inputs of every pixel case with the planted values, computed once and left unchanged"""
    cache = {}

    def get(case):
        if case not in cache:
            B, H, W = case
            d = M.pixel_inputs(B, H, W)
            if H * W >= 16:
                planted = _lo_hi()
                gp, local, trimap = d['global_pred'].view(B, 3, -1), d['local_pred'].view(B, -1), d['trimap'].view(B, -1)
                for i in range(6):                      # bounds, one ulp outside, 0 and 1: in channel i % 3 and in the local map
                    gp[:, i % 3, i] = planted[i]
                    local[:, i] = planted[i]
                trimap[:, 6:14] = torch.tensor(M.TRIMAP_PLANTED)
                gp[:, :, 14] = 0.5                      # ties: all three, the last two, the outer two; and saturated sigmoids
                gp[:, :, 15] = torch.tensor([0.2, 0.7, 0.7])
                if H * W >= 18:
                    gp[:, :, 16] = torch.tensor([0.7, 0.2, 0.7])
                    gp[:, :, 17] = 1.0
                # (the image stays 0.01 .. 0.5 away from the composition of the planted local map)
                ph = torch.clamp(d['local_pred'], min=M.LO, max=M.HI)
                comp = ph * d['fg'] + (1. - ph) * d['bg']
                old = torch.clamp(M.pixel_inputs(B, H, W)['local_pred'], min=M.LO, max=M.HI)
                d['image'] = d['image'] - (old * d['fg'] + (1. - old) * d['bg']) + comp
            if B >= 2:
                d['trimap'][0][d['trimap'][0] == 128] = 255.      # a sample with no 128 pixel: sum w = 0
            cache[case] = d
        return cache[case]
    return get


def _tri_buffers(gp, channels_last):
    """-> device global_pred in the memory format asked for, (sb, sc, sp), and a fenced gradient buffer with the same strides"""
    B, _, H, W = gp.shape
    P = H * W
    if channels_last:
        gd = gp.permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2)
        flat, buf = _fenced((B, H, W, 3))
        return gd, (3 * P, 1, 3), flat, buf.permute(0, 3, 1, 2)
    flat, buf = _fenced((B, 3, H, W))
    return gp.contiguous().cuda(), (3 * P, P, 1), flat, buf


def _ratio(got, want, mag):
    return float(((got.double() - want).abs() / (1e-5 * mag).clamp_min(1e-300)).max())


@pytest.mark.parametrize('channels_last', [False, True])
@pytest.mark.parametrize('case', M.PIXEL_CASES)
def test_trimap_stats_both_memory_formats(px_inputs, case, channels_last):
    _, _lib = _ops()
    L, st = _lib.lib(), _lib.stream()
    B, H, W = case
    P = H * W
    d = px_inputs(case)
    g = _upstream(B, 2)
    j = M.trimap_stats_judge(d['global_pred'], d['trimap'], M.SMOOTH, g)
    gd, (sb, sc, sp), fgrad, dgp = _tri_buffers(d['global_pred'], channels_last)
    td, gsd = d['trimap'].cuda().contiguous(), g.float().cuda()
    fs, stats = _fenced((B, 2))
    fp_, part = _fenced((L.saicv_matting_ws_floats(B, P),))
    _lib.check(L.saicv_trimap_stats_fwd(gd.data_ptr(), sb, sc, sp, td.data_ptr(), B, P, M.SMOOTH, part.data_ptr(), stats.data_ptr(),
                                        st), 'trimap_stats_fwd')
    _lib.check(L.saicv_trimap_stats_bwd(gd.data_ptr(), sb, sc, sp, td.data_ptr(), gsd.data_ptr(), B, P, M.SMOOTH, dgp.data_ptr(), st),
               'trimap_stats_bwd')
    _check_fences(((fs, 'stats'), (fp_, 'workspace'), (fgrad, 'dglobal')))
    got = dgp.cpu()
    outside = ~j['inside']
    if P >= 16:
        assert bool(j['inside'].view(B, 3, -1)[:, 0, 0].all()) and bool(j['inside'].view(B, 3, -1)[:, 1, 1].all())
        assert not bool(j['inside'].view(B, 3, -1)[:, 2, 2].any()) and int(outside.sum()) >= 4 * B
    assert float(got[outside].abs().max() if bool(outside.any()) else 0.) == 0.0
    rs = _ratio(stats.cpu(), j['stats'], j['mag'])
    rg = _ratio(got[j['inside']], j['dgp'][j['inside']], j['dgp_mag'][j['inside']])
    print('trimap_stats', case, 'channels_last' if channels_last else 'nchw', 'worst ratio: sums', round(rs, 4), 'gradient', round(rg, 4))
    assert rs <= 1.0 and rg <= 1.0, (rs, rg)


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('case', M.PIXEL_CASES)
def test_alpha_l1(px_inputs, case, masked):
    _, _lib = _ops()
    L, st = _lib.lib(), _lib.stream()
    B, H, W = case
    P = H * W
    d = px_inputs(case)
    trimap = d['trimap'] if masked else None
    g = _upstream(B, 2)
    j = M.alpha_judge(d['local_pred'], d['alpha'], trimap, g)
    pd, ad, gd = d['local_pred'].cuda().contiguous(), d['alpha'].cuda().contiguous(), g.float().cuda()
    td = trimap.cuda().contiguous() if masked else None
    fs, sums = _fenced((B, 2))
    fp_, part = _fenced((L.saicv_matting_ws_floats(B, P),))
    fd, dp = _fenced((B, P))
    _lib.check(L.saicv_alpha_l1_fwd(pd.data_ptr(), ad.data_ptr(), _lib.ptr(td), B, P, part.data_ptr(), sums.data_ptr(), st), 'alpha_l1_fwd')
    _lib.check(L.saicv_alpha_l1_bwd(pd.data_ptr(), ad.data_ptr(), _lib.ptr(td), gd.data_ptr(), B, P, dp.data_ptr(), st), 'alpha_l1_bwd')
    _check_fences(((fs, 'sums'), (fp_, 'workspace'), (fd, 'dpred')))
    sums, got = sums.cpu(), dp.cpu()
    assert torch.equal(sums[:, 1].double(), j['sums'][:, 1])                  # counts are exact
    if masked and B >= 2:
        assert float(sums[0, 1]) == 0.0                                       # no 128 pixel: the loss's denominator is 0 + 1
        assert float(got[0].abs().max()) == 0.0
    outside = ~j['inside']
    assert float(got[outside].abs().max() if bool(outside.any()) else 0.) == 0.0
    if P >= 16:
        assert bool(j['inside'][:, :2].all()) and not bool(j['inside'][:, 2:6].any())
    rs = _ratio(sums[:, 0], j['sums'][:, 0], j['mag'][:, 0])
    ins = j['inside'] & (j['dp_mag'] > 0)
    rg = _ratio(got[ins], j['dp'][ins], j['dp_mag'][ins]) if bool(ins.any()) else 0.
    print('alpha_l1', case, 'masked' if masked else 'plain', 'worst ratio: sum', round(rs, 4), 'gradient', round(rg, 4))
    assert rs <= 1.0 and rg <= 1.0, (rs, rg)
    zero = j['inside'] & (j['dp_mag'] == 0)
    assert float(got[zero].abs().max() if bool(zero.any()) else 0.) == 0.0


@pytest.mark.parametrize('case', M.PIXEL_CASES)
def test_composition_l1(px_inputs, case):
    _, _lib = _ops()
    L, st = _lib.lib(), _lib.stream()
    B, H, W = case
    P = H * W
    d = px_inputs(case)
    g = _upstream(B, 1)[:, 0]
    j = M.composition_judge(d['local_pred'], d['fg'], d['bg'], d['image'], g)
    assert float(j['e'].abs().min()) >= 5e-3              # the recipe keeps every residual away from the kink of sqrt(e^2 + 1e-12)
    dev = [d[k].cuda().contiguous() for k in ('local_pred', 'fg', 'bg', 'image')]
    gd = g.float().cuda()
    fs, sums = _fenced((B,))
    fp_, part = _fenced((L.saicv_matting_ws_floats(B, P),))
    fd, dp = _fenced((B, 1, H, W))
    _lib.check(L.saicv_composition_l1_fwd(*[t.data_ptr() for t in dev], B, P, part.data_ptr(), sums.data_ptr(), st), 'composition_l1_fwd')
    _lib.check(L.saicv_composition_l1_bwd(*[t.data_ptr() for t in dev], gd.data_ptr(), B, P, dp.data_ptr(), st), 'composition_l1_bwd')
    _check_fences(((fs, 'sums'), (fd, 'dpred')))
    got = dp.cpu()
    outside = ~j['inside']
    assert float(got[outside].abs().max() if bool(outside.any()) else 0.) == 0.0
    rs = _ratio(sums.cpu(), j['sums'], j['mag'])
    rg = _ratio(got[j['inside']], j['dp'][j['inside']], j['dp_mag'][j['inside']])
    print('composition_l1', case, 'worst ratio: sum', round(rs, 4), 'gradient', round(rg, 4))
    assert rs <= 1.0 and rg <= 1.0, (rs, rg)


@pytest.mark.parametrize('channels_last', [False, True])
@pytest.mark.parametrize('case', M.PIXEL_CASES)
def test_matting_fuse_is_bit_exact(px_inputs, case, channels_last):
    _, _lib = _ops()
    L, st = _lib.lib(), _lib.stream()
    B, H, W = case
    P = H * W
    d = px_inputs(case)
    fused_j, idx = M.fuse_judge(d['global_pred'], d['local_pred'])
    if P >= 18:
        flat = idx.view(B, -1)
        assert flat[:, 14].tolist() == [0] * B and flat[:, 15].tolist() == [1] * B and flat[:, 16].tolist() == [0] * B
        assert flat[:, 17].tolist() == [0] * B
    dfused = torch.randn(B, 1, H, W, generator=torch.Generator().manual_seed(P))
    gd, (sb, sc, sp), _, _ = _tri_buffers(d['global_pred'], channels_last)
    ld, dd = d['local_pred'].cuda().contiguous(), dfused.cuda()
    ff, fused = _fenced((B, 1, H, W))
    fd, dlocal = _fenced((B, 1, H, W))
    _lib.check(L.saicv_matting_fuse_fwd(gd.data_ptr(), sb, sc, sp, ld.data_ptr(), B, P, fused.data_ptr(), st), 'matting_fuse_fwd')
    _lib.check(L.saicv_matting_fuse_bwd(gd.data_ptr(), sb, sc, sp, dd.data_ptr(), B, P, dlocal.data_ptr(), st), 'matting_fuse_bwd')
    _check_fences(((ff, 'fused'), (fd, 'dlocal')))
    assert torch.equal(fused.cpu(), fused_j)
    assert torch.equal(dlocal.cpu(), dfused * (idx == 1).float())


@pytest.mark.parametrize('channels_last', [False, True])
def test_ops_autograd_surface(px_inputs, channels_last):
    """through ops: the five functions under autograd at 33 x 70, global_pred in both memory formats, gradients against the judges"""
    ops, _ = _ops()
    case = (3, 33, 70)
    B, H, W = case
    d = px_inputs(case)
    gp = d['global_pred'].cuda()
    if channels_last:
        gp = gp.contiguous(memory_format=torch.channels_last)
    gp.requires_grad_(True)
    local = d['local_pred'].cuda().requires_grad_(True)
    alpha, trimap = d['alpha'].cuda(), d['trimap'].cuda()
    g2 = _upstream(B, 2)
    stats = ops.trimap_stats(gp, trimap, M.SMOOTH)
    fused = ops.collaborative_matting(gp, local)
    la = ops.alpha_l1(local, alpha, trimap)
    fa = ops.alpha_l1(fused, alpha)
    co = ops.composition_l1(fused, d['fg'].cuda(), d['bg'].cuda(), d['image'].cuda())
    lap = ops.laplacian_l1(local, alpha, trimap)
    assert tuple(stats.shape) == (B, 2) and tuple(la.shape) == (B, 2) and tuple(co.shape) == (B,) and lap.dim() == 0
    assert fused.dtype == torch.float32 and tuple(fused.shape) == (B, 1, H, W)
    ((stats * g2.cuda()).sum() + (la * g2.cuda()).sum() + (fa * g2.cuda()).sum() + co.sum() + lap).backward()
    assert gp.grad.stride() == gp.stride()
    jt = M.trimap_stats_judge(d['global_pred'], d['trimap'], M.SMOOTH, g2)
    ins = jt['inside']
    assert _ratio(gp.grad.cpu()[ins], jt['dgp'][ins], jt['dgp_mag'][ins]) <= 1.0          # fuse sends nothing to global_pred
    fused_j, idx = M.fuse_judge(d['global_pred'], d['local_pred'])
    assert torch.equal(fused.detach().cpu(), fused_j)
    ja = M.alpha_judge(d['local_pred'], d['alpha'], d['trimap'], g2)
    jf = M.alpha_judge(fused_j, d['alpha'], None, g2)
    jc = M.composition_judge(fused_j, d['fg'], d['bg'], d['image'], torch.ones(B))
    loss64, dlap, _ = M.lap_loss_judge(d['local_pred'], d['alpha'], d['trimap'])
    on = (idx == 1).double()
    want = ja['dp'].view(B, 1, H, W) + on * (jf['dp'].view(B, 1, H, W) + jc['dp']) + dlap
    err = float((local.grad.cpu().double() - want).abs().max() / want.abs().max())
    print('ops surface', 'channels_last' if channels_last else 'nchw', 'local gradient error relative to its largest element', err)
    assert err <= 1e-5
    assert abs(float(lap) - float(loss64)) <= 1e-5 * abs(float(loss64))


@pytest.mark.parametrize('masked', [False, True])
def test_alpha_loss_node_is_the_reference_ratio_of_the_sums(px_inputs, masked):
    """ops.alpha_loss (what LocalAlphaLoss / FusionAlphaLoss call): sum / (sum w + 1) with a trimap, sum / pixels without; held to
    the bound of the sums it is made of"""
    ops, _ = _ops()
    B, H, W = case = (3, 33, 70)
    d = px_inputs(case)
    trimap = d['trimap'] if masked else None
    j = M.alpha_judge(d['local_pred'], d['alpha'], trimap)
    den = float(j['sums'][:, 1].sum()) + 1. if masked else float(B * H * W)
    j = M.alpha_judge(d['local_pred'], d['alpha'], trimap, torch.full((B, 2), 2.5 / den, dtype=torch.float64))
    leaf = d['local_pred'].cuda().requires_grad_(True)
    loss = ops.alpha_loss(leaf, d['alpha'].cuda(), None if trimap is None else trimap.cuda())
    (2.5 * loss).backward()
    assert loss.dim() == 0 and abs(float(loss.detach()) - float(j['sums'][:, 0].sum()) / den) <= 1e-5 * float(j['mag'][:, 0].sum()) / den
    got, ins = leaf.grad.cpu().view(B, -1), j['inside'] & (j['dp_mag'] > 0)
    assert _ratio(got[ins], j['dp'][ins], j['dp_mag'][ins]) <= 1.0 and float(got[~ins].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ pyramid
def _lap_level(cur, alpha, trimap, level0, table, gnext=None, topcur=None, gs=None, gtop=None):
    """one level forward (and, with gs, backward) through the C-ABI on fenced buffers; every argument a CPU tensor or None
    -> next [B, h/2, w/2], sum_e [B], sum_next [B], gcur [B, h, w] or None"""
    _, _lib = _ops()
    L, st = _lib.lib(), _lib.stream()
    import ctypes
    B, h, w = cur.shape
    tab = (ctypes.c_float * 25)(*[float(v) for v in table.reshape(-1).tolist()])
    dev = [None if t is None else t.float().contiguous().cuda() for t in (cur, alpha, trimap, gnext, topcur, gs, gtop)]
    cd, ad, td, gnd, tcd, gsd, gtd = dev
    fn, nxt = _fenced((B, h // 2, w // 2)) if (h // 2) * (w // 2) else (None, None)
    fp_, part = _fenced((L.saicv_lap_level_ws_floats(B, h, w),))
    fs, se = _fenced((B,))
    fs2, sn = _fenced((B,))
    p = _lib.ptr
    _lib.check(L.saicv_lap_level_fwd(p(cd), p(ad), p(td), int(level0), B, h, w, tab, p(nxt), p(part), p(se), p(sn), st), 'lap_level_fwd')
    pairs = [(fp_, 'workspace'), (fs, 'sum_e'), (fs2, 'sum_next')] + ([(fn, 'next')] if fn is not None else [])
    gcur = None
    if gs is not None:
        fg_, gcur = _fenced((B, h, w))
        _lib.check(L.saicv_lap_level_bwd(p(cd), p(ad), p(td), int(level0), B, h, w, tab, p(gnd), p(tcd), p(gsd), p(gtd), p(gcur), st),
                   'lap_level_bwd')
        pairs.append((fg_, 'gcur'))
    _check_fences(pairs)
    return (nxt.cpu() if nxt is not None else torch.zeros(B, h // 2, w // 2)), se.cpu(), sn.cpu(), (None if gcur is None else gcur.cpu())


def _lap_chain(pred, alpha, trimap, table, gs):
    """the five levels forward and backward through the C-ABI -> levels (cur1 .. cur5), sums [6, B], dpred [B, h, w]"""
    B, _, h, w = pred.shape
    maps, sums = [pred[:, 0]], []
    for l in range(M.LEVELS):
        nxt, se, sn, _ = _lap_level(maps[l], alpha if l == 0 else None, trimap if l == 0 else None, l == 0, table)
        maps.append(nxt)
        sums.append(se)
    sums.append(sn)
    g = None
    for l in range(M.LEVELS - 1, -1, -1):
        top = l == M.LEVELS - 1
        _, _, _, g = _lap_level(maps[l], alpha if l == 0 else None, trimap if l == 0 else None, l == 0, table, gnext=g if not top else None,
                                topcur=maps[l + 1] if top else None, gs=gs[l], gtop=gs[M.LEVELS] if top else None)
    return maps[1:], torch.stack(sums), g


def _representable(x, frac_bits):
    """x (float64) is held by fp32 exactly and |x| 2^frac_bits stays below 2^24: sums of such terms in any order are exact"""
    return bool((x.float().double() == x).all()) and float(x.abs().max() if x.numel() else 0.) * 2. ** frac_bits < 2. ** 24


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('case', M.LAP_CASES)
def test_lap_levels_integer_inputs_are_bit_exact(case, masked):
    B, H, W = case
    pred, alpha, trimap = M.lap_integer_inputs(B, H, W, masked)
    table = M.dyadic_table(H * 1000 + W)
    gs = (torch.randint(0, 2, (M.LEVELS + 1, B), generator=torch.Generator().manual_seed(H + W)) * 2 - 1).double()
    d0, wgt = M.lap_d0(pred, alpha, trimap)
    j = M.lap_judge(d0, table, gs)
    for l in range(M.LEVELS):
        # forward: the map is a multiple of 2^-4l, G * cur and e of 2^-(4l + 2); the sums of |e| stay below 2^24 such units
        assert _representable(j['curs'][l], 4 * l + 2) and _representable(j['es'][l], 4 * l + 2)
        assert _representable(j['es'][l].abs().sum((1, 2, 3)), 4 * l + 2)
        # backward: gF is a multiple of 2^-(18 - 4l), g_cur of 2^-(20 - 4l); G^T |gF| + 1 bounds every partial sum of a pixel
        assert _representable(j['gcurs'][l], 20 - 4 * l)
        assert _representable(M.conv_gauss_T(j['gfs'][l].abs(), table.double()) + 1., 20 - 4 * l)
    assert _representable(j['curs'][M.LEVELS], 20) and _representable(j['sums'][M.LEVELS], 20)
    assert bool((j['sums'].float().double() == j['sums']).all())
    levels, sums, dpred = _lap_chain(pred, alpha, trimap, table, gs.float())
    for l in range(M.LEVELS):
        assert torch.equal(levels[l].double(), j['curs'][l + 1][:, 0]), f'level {l + 1}'
    assert torch.equal(sums.double(), j['sums'])
    assert torch.equal(dpred.double(), (j['g0'] * wgt)[:, 0])
    assert float(j['g0'].abs().max()) > 0 and float(j['sums'][M.LEVELS].min()) >= 0


@pytest.mark.parametrize('shape', [(1, 1, 1), (1, 2, 3), (2, 1, 5), (1, 3, 2)])
def test_lap_level_tiny_maps_are_bit_exact(shape):
    """one level on maps smaller than the replicate pad: integer map, dyadic table, +-1 / small-integer upstream gradients"""
    B, h, w = shape
    g = torch.Generator().manual_seed(h * 10 + w)
    cur = torch.randint(-2, 3, (B, h, w), generator=g).double()
    K = M.dyadic_table(h * 7 + w).double()
    gs = (torch.randint(0, 2, (B,), generator=g) * 2 - 1).double()
    gnext = torch.randint(-2, 3, (B, h // 2, w // 2), generator=g).double()
    f = M.conv_gauss(cur[:, None], K)
    e = cur[:, None] - f
    nxt_j = torch.nn.functional.avg_pool2d(f, 2) if (h // 2) * (w // 2) else torch.zeros(B, 1, h // 2, w // 2, dtype=torch.float64)
    s = gs.view(B, 1, 1, 1) * torch.sign(e)
    want = s + M.conv_gauss_T(M.pool_T(gnext[:, None], h, w) - s, K)
    nxt, se, sn, gcur = _lap_level(cur, None, None, False, K, gnext=gnext if gnext.numel() else None, gs=gs)
    assert torch.equal(nxt.double(), nxt_j[:, 0]) and torch.equal(se.double(), e.abs().sum((1, 2, 3)))
    assert torch.equal(sn.double(), nxt_j.abs().sum((1, 2, 3))) and torch.equal(gcur.double(), want[:, 0])


@pytest.fixture(scope='module')
def fixture():
    return torch.load(FIXTURE, map_location='cpu', weights_only=True)


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('case', M.LAP_CASES)
def test_lap_float_inputs_match_float64_and_repeat_bit_for_bit(fixture, case, masked):
    ops, _ = _ops()
    B, H, W = case
    pred, alpha, trimap = M.lap_float_inputs(B, H, W, masked)
    loss64, grad64, j = M.lap_loss_judge(pred, alpha, trimap)
    smallest = min(float(e[e != 0].abs().min()) for e in j['es'] + [j['curs'][M.LEVELS]] if bool((e != 0).any()))
    assert smallest >= 1e-6, smallest                   # no sign of a pyramid entry is ambiguous in fp32
    dev = fixture['lap_dev'][(B, H, W, masked)]

    def run():
        leaf = pred.cuda().requires_grad_(True)
        loss = ops.laplacian_l1(leaf, alpha.cuda(), None if trimap is None else trimap.cuda())
        loss.backward()
        return loss.detach().cpu(), leaf.grad.cpu()

    loss, grad = run()
    err_l = abs(float(loss) - float(loss64)) / abs(float(loss64))
    err_g = float((grad.double() - grad64).abs().max() / grad64.abs().max())
    lim_l, lim_g = max(8. * dev['loss'], 16. * EPS32), max(8. * dev['grad'], 16. * EPS32)
    print('laplacian', case, 'masked' if masked else 'plain', 'smallest entry', smallest, 'loss', err_l, 'limit', lim_l, 'ratio',
          round(err_l / lim_l, 4), 'gradient', err_g, 'limit', lim_g, 'ratio', round(err_g / lim_g, 4))
    if masked:
        assert float(grad[:, 0][trimap != 128].abs().max()) == 0.0
    assert err_l <= lim_l and err_g <= lim_g
    loss2, grad2 = run()
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


def test_a_side_below_32_raises_before_any_launch():
    ops, _ = _ops()
    pred, alpha = torch.rand(1, 1, 31, 64, device='cuda'), torch.rand(1, 31, 64, device='cuda')
    with pytest.raises(ValueError):
        ops.laplacian_l1(pred, alpha)
    with pytest.raises(ValueError):
        ops.laplacian_l1(pred.transpose(2, 3), alpha.transpose(1, 2))
    assert float(ops.laplacian_l1(torch.rand(1, 1, 32, 32, device='cuda'), torch.rand(1, 32, 32, device='cuda'))) > 0
