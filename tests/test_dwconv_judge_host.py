"""Proves the judge of tests/test_gpu_dwconv_f64.py on the host, without a GPU: the two float64 formulations of tests/dwconv_common.py
agree with each other and with float64 autograd on every case, the exact-regime inputs are exact in fp32 and in bf16, every planted fault
makes at least one exact and one accuracy case miss, the unfaulted fp32 emulation passes everywhere with nothing left out, CONSTANTS is
what the emulations measure, and the case tables reach every template instantiation and launch form of csrc/dwconv.hip (dw_grid, the
route predicates, the tiling and the weight gradient's launch quantities restated)."""
import math
import os
import re
import sys

import pytest
import torch

import dwconv_common as D
from conftest import ROOT

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
ids = lambda c: c.id      # noqa: E731


def _close(a, b, scale, tol=1e-13):
    return bool(((a - b).abs() <= tol * (1 + scale)).all())


# ------------------------------------------------------------------------------------------------ the references against each other
def test_the_two_float64_formulations_agree_with_each_other_and_with_autograd():
    """F.conv2d(groups=C) + autograd against the tap-shifted formulation, and the kernels' gather form against both, on every case"""
    for case in D.ALL_CASES:
        inp = D.inputs(case)
        a, b, m = D.conv_f64(case, inp), D.direct(case, inp), D.direct(case, inp, mag=True)
        assert a.keys() == b.keys() == m.keys() == {'y', 'dx', 'dw', 'db'}
        for k in a:
            assert a[k].shape == b[k].shape == m[k].shape, (case.id, k)
            assert _close(a[k], b[k], m[k]), (case.id, k)
            assert bool((m[k] >= b[k].abs() - 1e-12 * (1 + m[k])).all()), (case.id, k)     # the magnitude sums dominate the values
        assert _close(D.gather_form(case, inp['x'], inp['w'], inp['b'], False), a['y'], m['y']), case.id
        assert _close(D.gather_form(case, inp['dy'], inp['w'], None, True), a['dx'], m['dx']), case.id


def test_big_reference_is_the_general_one_at_a_small_height():
    """the three shifted products of the second-trip cases against F.conv2d on the same geometry with 37 rows"""
    for big in D.BIG_CASES:
        case = D.DwCase(big.id + '-small', 'walk', big.dt, 2, 37, 1, 1, big.K, 1, big.pad, 1, True)
        inp = D.big_inputs(case)
        ref = D.conv_f64(case, {k: v.to(F64) for k, v in inp.items()})
        got = D.big_reference(case, inp)
        assert torch.equal(got['y'].to(F64), ref['y']) and torch.equal(got['dx'].to(F64), ref['dx']), big.id
        assert float(got['y'].abs().max()) <= 256 and float(got['dx'].abs().max()) <= 256                      # exact in bf16


# ------------------------------------------------------------------------------------------------ the exact regime is exact
def test_exact_regime_inputs_are_exact_in_the_working_precision():
    """an fp32 and a bf16 evaluation of forward and data gradient equal the float64 one; the weight-gradient sums are exact in the fp32
    emulation of the kernel's partition, in the deterministic fold and in two arrival orders"""
    n = 0
    for case in D.ALL_CASES:
        if not case.exact:
            continue
        inp = D.inputs(case)
        spec = D.reference(case, inp)
        assert all(s[0] == 'equal' for s in spec.values())
        for name, t in inp.items():
            if t is not None:
                assert torch.equal(D.rdt(t, 'bf16'), t), (case.id, name)
        if case.table == 'wgrad':
            for got in D.emulate(case, inp)[:3]:
                assert not D.judge(got, spec), case.id
            assert float(D.direct(case, inp, mag=True)['dw'].max()) + 8 < 2 ** 24
        else:
            for wd, store in ((F32, 'f32'), (BF16, 'bf16')):
                assert not D.judge(D.emulate_conv(case, inp, wd, store), spec), (case.id, wd)
            assert float(max(spec['y'][1].abs().max(), spec['dx'][1].abs().max())) <= 132
        n += 1
    assert n > 300


def test_exact_weights_have_no_symmetry_a_wrong_kernel_could_hide_behind():
    for case in D.ALL_CASES:
        if case.exact and case.K >= 2:
            w = D.inputs(case)['w'][:, 0]
            for other in (w.flip(1), w.flip(2), w.flip(1, 2), w.transpose(1, 2)):
                assert bool((other != w).flatten(1).any(1).all()), case.id                # in every channel
    for big in D.BIG_CASES:
        if big.K >= 2:
            col = D.big_inputs(D.DwCase('w', 'big', 'bf16', 1, 4, 1, 1, big.K, 1, big.pad, 1))['w'][:, 0, :, big.pad]
            assert bool((col.flip(1) != col).any(1).all())


def test_accumulating_destinations_hold_a_nonzero_prefill():
    case = next(c for c in D.WGRAD_CASES if c.K == 3 and c.cpr == 3)
    pw, pb = D.dw_prefill(case)
    assert bool((pw >= 3).all()) and bool((pb >= 3).all()) and pw.unique().numel() == 5 and not torch.equal(pw.reshape(-1)[:case.C], pb)


def test_unread_rows_and_columns_are_exact_zeros_in_the_reference():
    hit = 0
    for case in D.CONV_CASES:
        rows, cols = D.unread(case)
        if bool(rows.any()) or bool(cols.any()):
            dx = D.reference(case, D.inputs(case))['dx'][1]
            assert bool((dx[:, rows] == 0).all()) and bool((dx[:, :, cols] == 0).all()), case.id
            live = dx[:, ~rows][:, :, ~cols]
            assert bool((live != 0).any()), case.id
            hit += bool(rows.any()) and bool(cols.any())
    assert hit >= 4


# ------------------------------------------------------------------------------------------------ the constants
@pytest.fixture(scope='module')
def measured():
    """the worst ratio of every emulation to its float64 reference over the accuracy cases, on one thread"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    worst, missed = {}, []
    try:
        for case in D.ALL_CASES:
            if case.exact:
                continue
            inp = D.inputs(case)
            spec = D.reference(case, inp)
            for got in D.emulate(case, inp):
                assert got.keys() == spec.keys()
                missed += [(case.id, m) for m in D.judge(got, spec, worst)]
    finally:
        torch.set_num_threads(threads)
    return worst, missed


def test_constants_table_is_what_the_emulations_measure(measured):
    """CONSTANTS is a record of this measurement, not a choice: a quarter of slack either way for another torch build"""
    worst, _ = measured
    lines = [f'{n:6} {worst.get(n, float("nan")):9.4g}  (stored {c:g})' for n, c in D.CONSTANTS.items()]
    print('\n'.join(lines))
    assert set(D.CONSTANTS) == {'dw', 'db'} and set(D.CONSTANTS) <= set(worst) and D.CONSTANTS_MEASURED_WITH.startswith('torch ')
    for n, c in D.CONSTANTS.items():
        assert math.isfinite(worst[n]) and c / 1.25 <= worst[n] <= c * 1.25, '\n' + '\n'.join(lines)


def test_the_unfaulted_emulation_passes_everywhere(measured):
    """forward and data gradient inside the DERIVED K * K + 1, the weight gradient inside MARGIN times its measured constant"""
    worst, missed = measured
    assert not missed, missed[:5]
    assert D.MARGIN == 4.0 and D.UF == 2.0 ** -24
    assert D.FIXED == {f'chain_k{K}': K * K + 1.0 for K in range(1, 9)}
    assert set(worst) == set(D.CONSTANTS) | {f'chain_k{K}' for K in (1, 2, 3, 4, 5, 6, 7, 8)}
    for n, r in worst.items():
        assert r <= D.allowed_ratio(n), (n, r)


def test_no_case_leaves_an_element_out():
    """no spec carries a keep mask: every element of every output is judged, so the cap LEFT_OUT_CAP is never drawn on -- shown on the
    reference alone, which passes its own spec whole"""
    assert D.LEFT_OUT_CAP == 0.005
    for case in D.ALL_CASES:
        spec = D.reference(case, D.inputs(case))
        assert set(spec) == ({'y', 'dx'} if case.table != 'wgrad' else ({'dw', 'db'} if case.bias else {'dw'}))
        for kind, ref, *rest in spec.values():
            assert kind in ('equal', 'bound') and len(rest) in (0, 3)
            assert rest == [] or rest[0].shape == ref.shape                                # a bound for every element
            assert not bool(torch.isnan(ref).any())
        assert not D.judge(D.values(spec), spec), case.id


# ------------------------------------------------------------------------------------------------ every fault makes a case miss
def _catching_cases(fault, exact, stop=3):
    hits = []
    for case in D.ALL_CASES:
        if case.exact != exact:
            continue
        inp = D.inputs(case)
        if D.judge(D.values(D.reference(case, inp, fault)), D.reference(case, inp)):
            hits.append(case.id)
            if len(hits) >= stop:
                break
    return hits


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'accuracy'])
@pytest.mark.parametrize('fault', D.FAULTS)
def test_every_planted_fault_is_caught(fault, exact):
    hits = _catching_cases(fault, exact)
    print(fault, '->', hits)
    assert hits


def test_required_faults_are_all_listed():
    assert set(D.FAULTS) == {'unmirrored_dgrad', 'taps_transposed', 'pad_off_by_one', 'row_wrap', 'last_tile_dropped', 'inexact_quotient_kept',
                             'dilation_ignored_in_dgrad', 'bias_per_tap', 'bias_per_kernel_row', 'assign_not_add', 'last_range_dropped',
                             'image_seam_ignored'}


def test_the_direct_formulation_without_a_fault_is_the_reference():
    case = next(c for c in D.GATHER_CASES if 'k3s3' in c.id and not c.exact)
    inp = D.inputs(case)
    assert not D.judge(D.direct(case, inp), D.reference(case, inp))


def test_a_border_tap_the_tensor_scale_bound_would_not_see_is_caught():
    """one tap of one border pixel of a 7 x 7 bf16 layer read one column off: under the 2e-2 of the tensor's maximum that
    tests/test_gpu_dwconv.py allows, outside the judge"""
    case = next(c for c in D.WALK_CASES if c.K == 7 and c.pad == 3 and c.dt == 'bf16' and not c.exact and c.W >= 7)
    inp = D.inputs(case)
    spec = D.reference(case, inp)
    top = float(spec['y'][1].abs().max())
    # output (0, 0, 0) reads x[0, r - 3, c - 3]: the candidates are its valid taps, each moved one column to the right
    moves = torch.stack([(inp['x'][0, r - 3, c - 2] - inp['x'][0, r - 3, c - 3]) * inp['w'][:, 0, r, c] for r in range(3, 6) for c in range(3, 6)])
    small = torch.where(moves.abs() < 0.9 * 2e-2 * top, moves.abs(), torch.zeros(()))
    k, ch = divmod(int(small.argmax()), case.C)
    y = spec['y'][1].clone()
    y[0, 0, 0, ch] += moves[k, ch]
    got = {'y': D.rdt(y, 'bf16'), 'dx': D.rdt(spec['dx'][1], 'bf16')}
    assert 0 < float((got['y'] - spec['y'][1]).abs().max()) / top < 2e-2
    assert D.judge(got, spec) and not D.judge({'y': D.rdt(spec['y'][1], 'bf16'), 'dx': got['dx']}, spec)


# ------------------------------------------------------------------------------------------------ the tables reach every launch form
def test_restated_launch_geometry():
    assert [D.dw_grid(n) for n in (0, 1, 256, 257, 16384 * 256, 16384 * 256 + 1)] == [1, 1, 1, 2, 16384, 16384]
    assert [D.dw_trips(n) for n in (1, 16384 * 256, 16384 * 256 + 1)] == [1, 1, 2]
    assert [D.out_extent(*a) for a in ((5, 3, 1, 1, 1), (5, 3, 2, 1, 1), (6, 3, 3, 1, 1), (11, 7, 1, 9, 3), (1, 3, 1, 0, 1), (2, 3, 2, 0, 1))] == [5, 3, 2, 11, 0, 0]
    assert D.fwd_route(3, 1, 9, 1) == 'walk' and D.fwd_route(3, 2, 1, 1) == 'gather' and D.fwd_route(7, 1, 9, 3) == 'gather' and D.fwd_route(4, 1, 2, 1) == 'gather'
    assert D.dgrad_route(3, 1, 2, 1) == 'walk' and D.dgrad_route(3, 1, 3, 1) == 'gather' and D.dgrad_route(5, 1, 4, 1) == 'walk'
    assert D.conv_items(2, 3, 17, 3, 'walk') == 2 * 3 * 3 * 3 and D.conv_items(2, 3, 17, 3, 'gather') == 2 * 3 * 5 * 3
    g = D.wgrad_geom(256, 1, 7)                             # K = 7 with one chunk: 36 sub-ranges of 8 pixels for 256
    assert (g['cpb'], g['lanes_per_ps'], g['nps'], g['sub'], g['ppb'], g['ranges']) == (1, 7, 36, 8, 256, 1)
    assert g['subs_behind_the_block'] == 4 and g['dead_threads'] == 4 and not g['ordered'] and g['fold'] is None
    g = D.wgrad_geom(2 * 64 * 65, 1, 3)
    assert (g['ranges'], g['ppb'], g['last'], g['fold']) == (33, 256, 128, 'det_fold4_coop_kernel')
    g = D.wgrad_geom(257, 3, 5)
    assert (g['cpb'], g['groups'], g['dead_chunk_lanes'], g['ranges'], g['last'], g['fold']) == (2, 2, 1, 2, 1, 'det_fold4_kernel')
    assert [D.smallest_cpr_with_one_sub_range(K) for K in (3, 7, 8)] == [64, 32, 32]
    assert [D.smallest_cpr_with_a_live_last_sub_range(K) for K in range(1, 9)] == [1, 1, 8, 1, 4, 4, 2, 1]
    g = D.wgrad_geom(25, 32, 7)
    assert (g['cpb'], g['nps'], g['dead_threads'], g['sub']) == (32, 1, 32, 256)
    assert D.wgrad_geom(10 ** 6, 64, 3)['ranges'] == 512 and D.wgrad_geom(10 ** 6, 1, 3)['ranges'] == 512
    assert D.wgrad_lds_bytes(8, 'bf16') == 73728 and D.wgrad_lds_bytes(8, 'f32') == 36864 and D.wgrad_lds_bytes(7, 'bf16') == 65536


def test_every_template_instantiation_is_reached():
    R = D.REACHED
    assert set(R['gather']) == {(dt, flip) for dt in D.DTYPES for flip in (False, True)}
    assert set(R['s1']) == {(dt, K, flip) for dt in D.DTYPES for K in D.WALK_K for flip in (False, True)}
    assert set(R['wgrad']) == {(dt, K) for dt in D.DTYPES for K in range(1, 9)}
    # the LDS sum over the sub-ranges has a last term that holds pixels, at every K (every small case leaves it empty)
    assert set(R['last_sub_range_live']) == {(dt, K) for dt in D.DTYPES for K in range(1, 9)}
    known = {c.id for c in D.ALL_CASES + D.BIG_CASES}
    assert all(v in known for group in R.values() for v in group.values())


def test_every_launch_form_is_reached():
    flags = D.REACHED['flags']
    assert set(flags) >= {'nps==1', 'nps>1', 'dead_chunk_lanes', 'dead_threads', 'dead_threads_at_nps==1', 'sub_ranges_behind_the_block',
                          'ragged_last_range', 'ranges==1', 'ranges==2', 'ranges>=32', 'det_fold4_kernel', 'det_fold4_coop_kernel', 'dbias_null',
                          'dbias', 'dbias_null_ordered', 'lds_above_64KiB', 'skipped_rows', 'dgrad_falls_back_to_gather', 'inexact_quotients',
                          'unread_rows_and_columns', 'second_trip_gather_fwd', 'second_trip_gather_dgrad', 'second_trip_walk_fwd',
                          'second_trip_walk_dgrad'}, sorted(flags)
    assert all(D.dw_trips(max(c.fwd_items, c.dgrad_items)) == 1 for c in D.CONV_CASES)      # the second trip is the BIG cases' alone
    assert all(D.dw_trips(c.fwd_items) == 2 and D.dw_trips(c.dgrad_items) == 2 and (c.dt, c.W, c.C) == ('bf16', 1, 8) for c in D.BIG_CASES)


def test_walk_table_covers_the_paddings_and_the_tile_edges():
    for dt in D.DTYPES:
        mine = [c for c in D.WALK_CASES if c.dt == dt]
        assert all(c.N == 2 and c.fwd_route == 'walk' for c in mine)
        for K in D.WALK_K:
            for pad in (0, (K - 1) // 2, K - 1):
                at = [c for c in mine if c.K == K and c.pad == pad and c.exact]
                assert all(c.dgrad_route == 'walk' for c in at)
                assert {c.W for c in at} >= {t for t in D.WALK_WIDTHS if D.out_extent(t, K, 1, pad, 1) >= 1}, (K, pad)                  # the data gradient's destination width
                assert {c.OW for c in at} >= {t for t in D.WALK_WIDTHS if t - 2 * pad + K - 1 >= 1}, (K, pad)
                assert {c.cpr for c in at} == {1, 3} and {c.bias for c in at} == {True, False}
                assert any(not c.exact for c in mine if c.K == K and c.pad == pad)
            over = [c for c in mine if c.K == K and c.pad == K + 1]
            assert over and all(c.dgrad_route == 'gather' for c in over) and {c.OW for c in over} & set(D.WALK_WIDTHS)
        assert {c.OW for c in mine if c.pad == 0} >= set(D.WALK_WIDTHS)                  # every source column inside, a narrower output


def test_gather_table_covers_the_strides_dilations_and_even_kernels():
    for dt in D.DTYPES:
        mine = [c for c in D.GATHER_CASES if c.dt == dt]
        assert {c.geom for c in mine} == {(1, 1, 0, 1), (2, 1, 1, 1), (4, 1, 2, 1), (6, 1, 3, 1), (8, 1, 4, 1), (3, 2, 1, 1), (3, 3, 1, 1), (7, 1, 9, 3),
                                          (3, 2, 2, 2), (3, 1, 3, 1)}
        for geom in {c.geom for c in mine}:
            at = [c for c in mine if c.geom == geom]
            assert {c.W for c in at if c.exact} >= set(D.GATHER_WIDTHS), geom
            assert {c.OW for c in at if c.exact} >= set(D.GATHER_WIDTHS) - ({1} if geom[0] in (2, 4, 6, 8) else set()) - ({1, 3, 4} if geom == (3, 1, 3, 1) else set()), geom
            assert {c.bias for c in at} == {True, False} and any(not c.exact for c in at)
            assert all(c.dgrad_route == 'gather' for c in at) and all((c.fwd_route == 'walk') == (geom == (3, 1, 3, 1)) for c in at)
        s3 = [c for c in mine if c.geom == (3, 3, 1, 1)]
        assert any((c.H + 2 - 2 - 1) % 3 and bool(D.unread(c)[0].any()) and bool(D.unread(c)[1].any()) for c in s3)
        assert any((c.H, c.W) == (11, 13) for c in mine if c.geom == (7, 1, 9, 3))
        assert max(c.K ** 2 for c in mine) == 64


def test_weight_gradient_table_covers_the_launch_quantities():
    for dt in D.DTYPES:
        mine = [c for c in D.WGRAD_CASES if c.dt == dt]
        for K in range(1, 9):
            assert {c.cpr for c in mine if c.K == K} >= {1, 3, 16}
        assert {c.npix for c in mine if c.cpr == 1 and c.K in (3, 7)} >= {256, 257, 2 * 64 * 65}
        for n, ranges in ((256, 1), (257, 2), (2 * 64 * 65, 33)):
            at = [c for c in mine if c.npix == n and c.cpr == 1]
            assert at and all(c.wgrad['ranges'] == ranges for c in at) and {c.bias for c in at} == {True, False}
            assert any(not c.exact for c in at)
        for K in (3, 7, 8):
            at = [c for c in mine if c.K == K and c.wgrad['nps'] == 1]
            assert at and all((c.N, c.H, c.W) == (1, 5, 5) and c.cpr == D.smallest_cpr_with_one_sub_range(K) for c in at)
        assert {(c.stride, c.dil) for c in mine} >= {(1, 1), (2, 1), (3, 1), (1, 3), (2, 2)} and {c.pad for c in mine} >= {0, 1, 3, 9}
        assert any(not c.exact and c.wgrad['nps'] == 1 for c in mine) and any(not c.exact and c.wgrad['dead_chunk_lanes'] for c in mine)


def test_the_instantiation_set_of_the_table_is_the_set_in_the_assembly():
    """the kernel symbols the compiler emits for csrc/dwconv.hip are exactly the instantiations REACHED names"""
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import check_fragment_regs as A
    names = set(re.findall(r'^\s*\.amdhsa_kernel _ZN12_GLOBAL__N_1\d+(dwconv_\w+?_kernelI\S+)$', A.assembly('dwconv.hip'), re.M))
    t = {'f32': 'f', 'bf16': 'DF16b'}
    table = {f'dwconv_gather_kernelI{t[dt]}Lb{int(flip)}EE' for dt, flip in D.REACHED['gather']}
    table |= {f'dwconv_s1_kernelI{t[dt]}Li{K}ELb{int(flip)}EE' for dt, K, flip in D.REACHED['s1']}
    table |= {f'dwconv_wgrad_kernelI{t[dt]}Li{K}EE' for dt, K in D.REACHED['wgrad']}
    got = {re.match(r'(dwconv_\w+?_kernelI(?:f|DF16b)(?:L[ib]\d+E)*E)', n).group(1) for n in names}
    assert got == table, (sorted(got - table), sorted(table - got))
