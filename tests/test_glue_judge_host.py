"""Proves the judge of tests/test_gpu_glue_f64.py on the host, without a GPU: the float64 references of tests/glue_common.py agree with
torch's own CPU operators and autograd (and, for RoPE, with the reference project's function through tests/golden/glue_edges.pt), the
exact-regime inputs are exact, the planted edges are in the inputs and decided as claimed, CONSTANTS is what the fp32 emulations
measure, every planted fault makes at least one named case miss, and the case tables reach every launch form of csrc/elemwise.hip and
csrc/pool.hip (ew_grid, col_geom and sgrid restated)."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import glue_common as G
from conftest import GOLDEN

F32, F64 = torch.float32, torch.float64
SMALL = 400000                                              # elements of the largest tensor a case may have to go through torch's operators


def _accuracy_cases(family):
    cases = G.FAMILIES[family][0]
    return [c for c in cases if not G.is_exact(c)]


def _close(a, b, tol=1e-13):
    return bool(((a - b).abs() <= tol * (1 + b.abs())).all())


# ------------------------------------------------------------------------------------------------ the references against torch
def test_activation_references_agree_with_torch_and_its_autograd():
    x = torch.cat([torch.tensor(G.SILU_PLANTED, dtype=F64), torch.linspace(-30, 30, 4001, dtype=F64)])
    x = x[x != 0].clone().requires_grad_(True)            # relu's derivative at 0 is a convention, held below
    dy = torch.linspace(-2, 2, x.numel(), dtype=F64)
    for op, fn in (('relu', F.relu), ('leaky', lambda t: F.leaky_relu(t, G.LEAKY_SLOPE)), ('silu', F.silu)):
        y = fn(x)
        (gx,) = torch.autograd.grad(y, x, dy)
        v, d = G.silu_math(x.detach())[:2] if op == 'silu' else G.act_math(op, x.detach())
        assert _close(v, y.detach()) and _close(dy * d, gx), op
    z = torch.zeros(3, dtype=F64)
    assert torch.equal(G.act_math('relu', z)[1], z) and torch.equal(G.act_math('leaky', z)[1], torch.full_like(z, G.LEAKY_SLOPE))
    # the stated bounds dominate the values they bound
    v, d, bv, bd = G.silu_math(x.detach())
    assert bool((bv >= v.abs()).all()) and bool((bd >= d.abs()).all())


def test_swiglu_reference_agrees_with_autograd():
    case = next(c for c in G.STREAM_CASES if c.op == 'swiglu' and c.chunks == 257 and c.dt == 'f32')
    inp = G.stream_inputs(case)
    x1, x2 = inp['x'].clone().requires_grad_(True), inp['x2'].clone().requires_grad_(True)
    out = F.silu(x1) * x2
    g1, g2 = torch.autograd.grad(out, (x1, x2), inp['dy'])
    spec = G.stream_reference(case, inp)
    assert _close(spec['out'][1], out.detach()) and _close(spec['dx1'][1], g1) and _close(spec['dx2'][1], g2)


def _window_positions(flat, case):
    """ATen's flat input indices [N, C, OH, OW] -> window positions kh * K + kw"""
    ih, iw = flat // case.W, flat % case.W
    oh = torch.arange(case.OH).view(1, 1, -1, 1) * case.stride - case.pad
    ow = torch.arange(case.OW).view(1, 1, 1, -1) * case.stride - case.pad
    return (ih - oh) * case.K + (iw - ow)


@pytest.mark.parametrize('case', [c for c in G.MAXPOOL_CASES if c.dt == 'f32' and c.H * c.W < SMALL], ids=lambda c: c.id)
def test_maxpool_reference_is_atens_cpu_operator(case):
    """values, the index plane (ties, NaN, +-inf and the all -inf window included) and the gradient"""
    inp = G.maxpool_inputs(case)
    spec = G.maxpool_reference(case, inp)
    x = inp['x'].permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    out, flat = F.max_pool2d(x, case.K, case.stride, case.pad, return_indices=True)
    (gx,) = torch.autograd.grad(out, x, inp['dout'].permute(0, 3, 1, 2).contiguous())
    ref_out = spec['out'][1].permute(0, 3, 1, 2)
    assert bool(((out.detach() == ref_out) | (torch.isnan(out.detach()) & torch.isnan(ref_out))).all())
    assert torch.equal(_window_positions(flat, case).to(F64), spec['idx'][1].permute(0, 3, 1, 2))
    assert torch.equal(gx, spec['dx'][1].permute(0, 3, 1, 2))


@pytest.mark.parametrize('case', [c for c in G.RESIZE_CASES if c.N * c.H * c.W * c.C < SMALL], ids=lambda c: c.id)
def test_resize_reference_follows_atens_tap_specification(case):
    """F.interpolate(mode='bilinear') run in fp32, forward and autograd: equal on the exact geometries, inside the judge elsewhere"""
    inp = G.resize_inputs(case)
    top = inp['top'].to(F32).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    out = F.interpolate(top, size=(case.H, case.W), mode='bilinear', align_corners=False)
    (gt,) = torch.autograd.grad(out, top, inp['dout'].to(F32).permute(0, 3, 1, 2).contiguous())
    got = {'out': out.detach().permute(0, 2, 3, 1).to(F64) + (0.0 if inp['lat'] is None else inp['lat']), 'dtop': G.rdt(gt.permute(0, 2, 3, 1).to(F64), case.tt)}
    assert not G.judge(got, G.resize_reference(case, inp)), case.id


@pytest.mark.parametrize('case', [c for c in G.AVGPOOL_CASES if c.fwd and c.dt == 'f32' and c.N * c.HW * c.C < SMALL], ids=lambda c: c.id)
def test_avgpool_reference_agrees_with_torch_and_its_autograd(case):
    inp = G.avgpool_inputs(case)
    x = inp['x'].permute(0, 2, 1).reshape(case.N, case.C, case.HW, 1).contiguous().requires_grad_(True)
    out = F.adaptive_avg_pool2d(x, 1)
    (gx,) = torch.autograd.grad(out, x, inp['dout'].view(case.N, case.C, 1, 1))
    spec = G.avgpool_reference(case, inp)
    assert _close(spec['out'][1], out.detach().view(case.N, case.C))
    assert _close(spec['dx'][1], gx.view(case.N, case.C, case.HW).permute(0, 2, 1))


def test_rope_reference_agrees_with_the_reference_project():
    gold = torch.load(os.path.join(GOLDEN, 'glue_edges.pt'), weights_only=True)['rope']
    cases = G.rope_edge_cases()
    assert cases and set(gold) == {c.id for c in cases}
    assert {c.prefix for c in cases} == {0, 1, 5, 7}
    for case in cases:
        inp = G.rope_inputs(case)
        out = G.rope_reference(case, inp)['out'][1]
        assert torch.equal(out[:, :, 0], gold[case.id]['q'].to(F64)) and torch.equal(out[:, :, 1], gold[case.id]['k'].to(F64)), case.id
        assert torch.equal(out[:, :, 2], inp['qkv'][:, :, 2])


def test_rope_transpose_is_the_adjoint():
    """<rope(x), g> == <x, rope^T(g)> on the float64 reference, untied halves"""
    for case in [c for c in G.ROPE_CASES if not c.exact and not c.transpose]:
        inp = G.rope_inputs(case)
        g = torch.randn(inp['qkv'].shape, generator=torch.Generator().manual_seed(7), dtype=F64)
        lhs = (G.rope_math(inp['qkv'], inp['sin'], inp['cos'], case.prefix, 0) * g).sum()
        rhs = (inp['qkv'] * G.rope_math(g, inp['sin'], inp['cos'], case.prefix, 1)).sum()
        assert abs(float(lhs - rhs)) <= 1e-12 * float((inp['qkv'] * g).abs().sum()), case.id


# ------------------------------------------------------------------------------------------------ the exact regime is exact
def _exact_candidates(family, case, inp):
    if family == 'resize':
        return [G.resize_emulate(case, inp, fused=False, bwd=case.bwd_items < 10000)]
    if family == 'colred':
        return G.emulate(family, case, inp)[:3]
    return G.emulate(family, case, inp)


def _input_dtype(family, case, name):
    if family == 'resize':
        return {'top': case.tt, 'lat': case.tl, 'dout': 'f32'}[name]
    return 'f32' if name in ('s', 'sin', 'cos') else case.dt


@pytest.mark.parametrize('family', ['stream', 'colred', 'rope', 'resize', 'avgpool'])
def test_exact_regime_inputs_are_exact_in_the_working_precision(family):
    """the fp32 (and bf16) evaluation of the kernel's arithmetic equals the float64 one bit for bit; for the column sums in the
    deterministic fold and in two random arrival orders"""
    cases, inputs, reference, _ = G.FAMILIES[family]
    n = 0
    for case in cases:
        if not G.is_exact(case) or (family == 'stream' and case.op in ('relu', 'leaky')):
            continue
        inp = inputs(case)
        spec = reference(case, inp)
        assert all(s[0] == 'equal' for s in spec.values())
        for got in _exact_candidates(family, case, inp):
            sub = {k: v for k, v in spec.items() if k in got}
            assert sub and not G.judge(got, sub), case.id
        for name, t in inp.items():                        # the inputs themselves are exact in their dtype
            if t is not None:
                assert torch.equal(G.rdt(t, _input_dtype(family, case, name)), t), (case.id, name)
        n += 1
    assert n


def test_exact_relu_and_leaky_outputs_are_bf16_values():
    for case in [c for c in G.STREAM_CASES if c.op in ('relu', 'leaky') and c.chunks <= 257]:
        inp = G.stream_inputs(case)
        v, d = G.act_math(case.op, inp['x'])
        assert torch.equal(G.rdt(v, 'bf16'), v) and torch.equal(G.rdt(inp['dy'] * d, 'bf16'), inp['dy'] * d)


# ------------------------------------------------------------------------------------------------ the planted edges
def test_planted_activation_edges_are_in_the_inputs():
    for case in G.STREAM_CASES:
        inp = G.stream_inputs(case) if case.chunks <= 257 else None
        if inp is None:
            continue
        if case.op in ('relu', 'leaky'):
            assert float(inp['x'][0]) == 0.0 and bool((inp['dy'][inp['x'] == 0] != 0).all())
            assert bool((inp['x'] > 0).any()) and bool((inp['x'] < 0).any())
        if case.op in ('silu', 'swiglu') and case.n >= len(G.SILU_PLANTED):
            assert torch.equal(inp['x'][:12], G.rdt(torch.tensor(G.SILU_PLANTED, dtype=F64), case.dt))
            s = torch.sigmoid(inp['x'][:12])
            assert bool((s[:3] < G.TINY).all()) and float(s[3]) > G.TINY                  # -120, -100, -88 underflow; -87 does not
            assert bool((inp['dy'][:12] != 0).all())


def test_planted_maxpool_edges_are_decided_as_claimed():
    case = next(c for c in G.MAXPOOL_CASES if c.id.startswith('f32-k3s2p1-16x16') and c.cpr == 1)
    inp = G.maxpool_inputs(case)
    spec = G.maxpool_reference(case, inp)
    out, idx, dx = spec['out'][1], spec['idx'][1], spec['dx'][1]
    assert bool((out[0, 0, 0] == -math.inf).all()) and bool((idx[0, 0, 0] == 4).all())      # all -inf: the first VALID element, (1, 1)
    # window (2, 2) covers rows 3..5, columns 3..5: NaN at (4, 3) and (4, 4) on the even channels -> the LAST NaN, position 1 * 3 + 1
    assert math.isnan(float(out[0, 2, 2, 0])) and float(idx[0, 2, 2, 0]) == 4.0
    assert math.isnan(float(out[0, 2, 1, 0])) and float(idx[0, 2, 1, 0]) == 5.0             # columns 1..3: only (4, 3), position 1 * 3 + 2
    assert bool((out[0, 3, 2] == math.inf).all())                                           # +inf at (6, 4)
    assert float(dx[0, 4, 4, 0]) == float(inp['dout'][0, 2, 2, 0])                          # the NaN takes the window's gradient
    ties = 0
    for c in G.MAXPOOL_CASES:
        if c.H * c.W < SMALL:
            i = G.maxpool_inputs(c)
            a, b = G.maxpool_reference(c, i), G.maxpool_reference(c, i, 'tie_last')
            ties += int((a['idx'][1] != b['idx'][1]).sum())
    assert ties > 1000
    odd = next(c for c in G.MAXPOOL_CASES if c.id.startswith('bf16-k2s2p0-7x9'))
    d = G.maxpool_reference(odd, G.maxpool_inputs(odd))['dx'][1]
    assert bool((d[:, 6] == 0).all()) and bool((d[:, :, 8] == 0).all()) and bool((d[:, :6, :8] != 0).any())


def test_resize_taps_are_clamped_at_both_ends_in_the_table():
    low = high = 0
    for case in G.RESIZE_CASES:
        for n_in, n_out in ((case.h, case.H), (case.w, case.W)):
            t = G.resize_taps(n_in, n_out)
            raw = G.resize_taps(n_in, n_out, 'no_low_clamp')
            low += int((raw['w1'] < 0).sum())
            high += int(((t['i0'] == n_in - 1) & (t['w1'] > 0)).sum())
            assert int(t['i1'].max()) <= n_in - 1 and int(t['i0'].min()) >= 0
    assert low > 10 and high > 10


def test_rope_tables_have_independent_halves():
    for case in G.ROPE_CASES[:16]:
        inp = G.rope_inputs(case)
        half = case.D // 2
        if inp['sin'].numel():
            assert not torch.equal(inp['sin'][:, :half], inp['sin'][:, half:]) and not torch.equal(inp['cos'][:, :half], inp['cos'][:, half:])


def test_accumulating_destinations_hold_a_nonzero_prefill():
    assert bool((G.col_prefill(16, 0) >= G.SUM_PREFILL).all()) and not torch.equal(G.col_prefill(16, 0), G.col_prefill(16, 1))


# ------------------------------------------------------------------------------------------------ the constants
@pytest.fixture(scope='module')
def measured():
    """the worst ratio of every emulation to its float64 reference over the accuracy cases, on one thread"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    worst, left_out = {}, 0
    try:
        for family in ('stream', 'colred', 'resize', 'avgpool', 'rope'):
            _, inputs, reference, _ = G.FAMILIES[family]
            for case in _accuracy_cases(family):
                inp = inputs(case)
                spec = reference(case, inp)
                for got in G.emulate(family, case, inp):
                    G.judge(got, {k: v for k, v in spec.items() if k in got}, worst)
    finally:
        torch.set_num_threads(threads)
    return worst


def test_constants_table_is_what_the_emulations_measure(measured):
    """CONSTANTS is a record of this measurement, not a choice: a quarter of slack either way for another torch build"""
    lines = [f'{n:14} {measured.get(n, float("nan")):9.4g}  (stored {c:g})' for n, c in G.CONSTANTS.items()]
    print('\n'.join(lines))
    assert set(G.CONSTANTS) <= set(measured)
    for n, c in G.CONSTANTS.items():
        assert math.isfinite(measured[n]) and c / 1.25 <= measured[n] <= c * 1.25, '\n' + '\n'.join(lines)


def test_emulations_pass_every_bound_with_the_margin(measured):
    for n, r in measured.items():
        assert r <= G.allowed_ratio(n), (n, r)


def test_no_case_leaves_an_element_out():
    """no spec carries a keep mask: every element of every output is judged, so the cap LEFT_OUT_CAP is never drawn on -- shown on the
    reference alone, which passes its own spec whole"""
    assert G.LEFT_OUT_CAP == 0.005
    for family, (cases, inputs, reference, _) in G.FAMILIES.items():
        for case in cases:
            if 'big' in case.id or getattr(case, 'chunks', 0) > 257 or getattr(case, 'M', 0) > 65:
                continue
            spec = reference(case, inputs(case))
            for kind, ref, *rest in spec.values():
                assert kind in ('equal', 'bound', 'fixed') and len(rest) in (0, 3)
                assert rest == [] or rest[0].shape == ref.shape                    # a bound for every element
            assert not G.judge(G.values(spec), spec), case.id


# ------------------------------------------------------------------------------------------------ every fault makes a case miss
def _catching_cases(family, fault, stop=3):
    cases, inputs, reference, _ = G.FAMILIES[family]
    hits = []
    for case in sorted(cases, key=lambda c: getattr(c, 'chunks', 0) > 257 or 'big' in c.id):       # the small ones first
        inp = inputs(case)
        true, bad = reference(case, inp), reference(case, inp, fault)
        if G.judge(G.values(bad), true):
            hits.append(case.id)
            if len(hits) >= stop:
                break
    return hits


ALL_FAULTS = [(family, fault) for family, spec in G.FAMILIES.items() for fault in spec[3]]


@pytest.mark.parametrize('family,fault', ALL_FAULTS, ids=[f'{a}-{b}' for a, b in ALL_FAULTS])
def test_every_planted_fault_is_caught(family, fault):
    hits = _catching_cases(family, fault)
    print(family, fault, '->', hits)
    assert hits


def test_required_faults_are_all_listed():
    listed = {f for spec in G.FAMILIES.values() for f in spec[3]} | set(G.NEUTRAL_FAULTS)
    assert listed >= {'sin_halves_shared', 'cos_halves_shared', 'prefix_rotated', 'v_rotated', 'transpose_sign', 'align_corners', 'no_low_clamp',
                      'edge_tap_dropped', 'bwd_window_one_short', 'scale_in_float64', 'tie_last', 'nan_ignored', 'padding_as_zero',
                      'uncovered_pixel_not_zeroed', 'index_plane_transposed', 'last_row_range_dropped', 'second_column_group_dropped',
                      'assign_not_add', 'tail_beyond_grid_dropped', 'scale_index_not_wrapped', 'relu_grad_one_at_zero',
                      'leaky_slope_on_positive', 'silu_derivative_without_x_term', 'swiglu_gradients_swapped', 'divide_by_hw_minus_one',
                      'accumulate_in_bf16'}


def test_the_neutral_fault_changes_nothing_observable():
    """scale_in_float64: not a bit on the exact geometries (dyadic ratios); elsewhere inside the allowance every tap already has"""
    assert G.NEUTRAL_FAULTS == ('scale_in_float64',)
    for case in G.RESIZE_CASES:
        if 'big' in case.id:
            assert case.h / case.H == 0.5
            continue
        inp = G.resize_inputs(case)
        true, bad = G.resize_reference(case, inp), G.resize_reference(case, inp, 'scale_in_float64')
        if case.exact:
            assert all(torch.equal(true[k][1], bad[k][1]) for k in true), case.id
        else:
            assert not G.judge(G.values(bad), true), case.id


# ------------------------------------------------------------------------------------------------ the tables reach every launch form
def test_restated_launch_geometry():
    assert [G.ew_grid(n) for n in (0, 1, 256, 257, 2048 * 256, 2048 * 256 + 1)] == [1, 1, 1, 2, 2048, 2048]
    assert [G.ew_trips(n) for n in (1, 2048 * 256, 2048 * 256 + 1)] == [1, 1, 2]
    assert [G.sgrid(n) for n in (1, 257, 4096 * 256 + 1)] == [1, 2, 4096] and G.pool_trips(4096 * 256 + 1) == 2
    assert G.col_geom(65537, 1) == (1, 1, 1009, 65) and G.col_geom(65, 63) == (32, 2, 2, 64) and G.col_geom(64, 65) == (64, 2, 1, 64)
    assert G.col_geom(3, 2)[0] == 2 and G.col_geom(1, 64) == (64, 1, 1, 64)


def test_streaming_tables_reach_every_form():
    for dt in G.DTYPES:
        for op in ('relu', 'leaky', 'silu', 'swiglu', 'mul', 'scale_add'):
            mine = [c for c in G.STREAM_CASES if c.op == op and c.dt == dt]
            chunks = {c.chunks for c in mine}
            if op != 'scale_add':
                assert chunks >= {1, 255, 256, 257, G.BIG_CHUNKS}
            big = [c for c in mine if G.ew_trips(c.chunks) == 2]
            assert big and all((c.chunks - G.EW_CAP * G.EW_THREADS) % G.EW_THREADS for c in big)      # second trip, ragged tail
            assert {G.ew_grid(c.chunks) for c in mine} >= {1, 2, G.EW_CAP}
        mul = [c for c in G.STREAM_CASES if c.op == 'mul' and c.dt == dt]
        assert {c.variant for c in mul} == {'both', 'da_null', 'db_null'}
        sa = [c for c in G.STREAM_CASES if c.op == 'scale_add' and c.dt == dt]
        assert {(c.cpr, c.variant) for c in sa} >= {(p, v) for p in (1, 65) for v in ('full', 'x_null', 's_null')}
        assert any(c.cpr == 65 and c.chunks > 256 and 256 % 65 for c in sa)                           # the channel index wraps mid-workgroup
        assert any(c.cpr == 65 and G.ew_trips(c.chunks) == 2 for c in sa) and any(c.cpr == 1 and G.ew_trips(c.chunks) == 2 for c in sa)
        assert any(not c.exact for c in sa) and any(not c.exact for c in mul)


def test_column_reduction_tables_reach_every_form():
    for dt in G.DTYPES:
        for op in ('bn_stats', 'scale_bwd'):
            mine = [c for c in G.COL_CASES if c.op == op and c.dt == dt]
            geoms = {(c.cpr, c.M): G.col_geom(c.M, c.cpr) for c in mine}
            assert {c.cpr for c in mine} >= {1, 2, 63, 64, 65} and {c.M for c in mine} >= {1, 3, 64, 65, 65537}
            assert {g[0] for g in geoms.values()} >= {1, 2, 32, 64}                                   # cw below 64 and at it
            assert geoms[(63, 65)] == (32, 2, 2, 64) and geoms[(65, 65)][1:3] == (2, 2)               # ragged second group, two row ranges
            assert geoms[(1, 65537)][3] == 65 and any(g[3] == 64 for g in geoms.values())             # rows_per_block above its floor
            assert any(M < G.EW_THREADS // g[0] for (cpr, M), g in geoms.items())                     # fewer rows than row lanes
            assert any(not c.exact for c in mine)
        sb = [c for c in G.COL_CASES if c.op == 'scale_bwd' and c.dt == dt]
        assert {c.variant for c in sb} == {'both', 'dy_only', 'ds_only', 's_null'}
        for v in ('both', 'dy_only', 'ds_only', 's_null'):
            assert any(c.variant == v and G.col_geom(c.M, c.cpr)[2] > 1 and G.col_geom(c.M, c.cpr)[1] > 1 for c in sb), v


def test_rope_table_reaches_every_form():
    for dt in G.DTYPES:
        mine = [c for c in G.ROPE_CASES if c.dt == dt]
        assert {c.D for c in mine} == {2 * G.EPC[dt], 32, 64, 96}
        assert {c.heads for c in mine} == {1, 3} and {c.B for c in mine} == {1, 2}
        for tr in (0, 1):
            assert {c.prefix for c in mine if c.transpose == tr and c.N == 7} == {0, 1, 5, 7}
            assert any(G.ew_trips(c.items) == 2 for c in mine if c.transpose == tr)
            assert any(not c.exact for c in mine if c.transpose == tr)
        assert all(G.ew_trips(c.items) == 1 for c in mine if 'big' not in c.id)


def test_resize_table_reaches_every_form():
    assert {((c.h, c.w), (c.H, c.W)) for c in G.RESIZE_CASES} >= set(G.RESIZE_GEOMS)
    assert {(c.tt, c.tl) for c in G.RESIZE_CASES} == {(a, b) for a in G.DTYPES for b in G.DTYPES + ('none',)}
    assert {c.C for c in G.RESIZE_CASES} == {4, 12} and {c.N for c in G.RESIZE_CASES} == {1, 2}
    for tt in G.DTYPES:
        big = [c for c in G.RESIZE_CASES if c.tt == tt and G.ew_trips(c.fwd_items) >= 2 and G.ew_trips(c.bwd_items) >= 2]
        assert big and all(c.exact for c in big)
        assert any(c.exact for c in G.RESIZE_CASES if c.tt == tt) and any(not c.exact for c in G.RESIZE_CASES if c.tt == tt)
    assert {(c.h / c.H) for c in G.RESIZE_CASES if c.exact} == set(G.RESIZE_EXACT_RATIOS)
    assert any(c.h / c.H >= 8 for c in G.RESIZE_CASES) and any(c.H / c.h >= 8 for c in G.RESIZE_CASES) and any(c.h == 1 for c in G.RESIZE_CASES)


def test_pooling_tables_reach_every_form():
    for dt in G.DTYPES:
        mine = [c for c in G.MAXPOOL_CASES if c.dt == dt]
        assert {(c.K, c.stride, c.pad) for c in mine} == {(3, 2, 1), (2, 2, 0), (2, 1, 0), (3, 1, 1), (5, 1, 2), (1, 2, 0)}
        assert {c.cpr for c in mine} == {1, 3}
        small = [c for c in mine if c.H * c.W < SMALL]
        br = {c.id: G.maxpool_bwd_branches(c) for c in small}
        by_geom = lambda K, s, p: [b for c, b in ((c, br[c.id]) for c in small) if (c.K, c.stride, c.pad) == (K, s, p)]      # noqa: E731
        assert all(b['loop'] == 0 and b['uncovered'] == 0 and b['quad'] > 0 for b in by_geom(3, 2, 1))
        assert any(b['uncovered'] > 0 for b in by_geom(2, 2, 0)) and any(b['uncovered'] == 0 for b in by_geom(2, 2, 0))
        assert all(b['quad'] > 0 and b['loop'] == 0 for b in by_geom(2, 1, 0))
        assert all(b['loop'] > 0 for b in by_geom(3, 1, 1)) and all(b['loop'] > 0 for b in by_geom(5, 1, 2))
        assert all(b['uncovered'] > 0 and b['quad'] > 0 for b in by_geom(1, 2, 0))
        big = [c for c in mine if c.H * c.W >= SMALL]
        assert len(big) == 1 and G.pool_trips(big[0].N * big[0].OH * big[0].OW * big[0].cpr) == 2
        assert G.pool_trips(big[0].N * big[0].H * big[0].W * big[0].cpr) == 2
        assert all(G.pool_trips(c.N * c.H * c.W * c.cpr) == 1 for c in small)
        avg = [c for c in G.AVGPOOL_CASES if c.dt == dt and c.fwd]
        assert {c.HW for c in avg} == {1, 49, 64, 3136} and {c.N * c.cpr for c in avg} == {1, 256, 257}
    big = [c for c in G.AVGPOOL_CASES if not c.fwd]
    assert len(big) == 1 and (big[0].N, big[0].C, big[0].dt) == (2, 8, 'f32') and G.pool_trips(big[0].N * big[0].HW * big[0].cpr) == 2
