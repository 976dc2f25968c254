"""The attention judge of tests/attn_common.py, checked without a GPU: the working-precision emulations pass every bound over the
whole case table (and set the constants), every planted fault breaks the quantity it should, the hand-written gradients agree with
float64 autograd, and the case table covers every kernel form the dispatch can select."""
import math

import pytest
import torch

import attn_common as A

DTYPES = (torch.float32, torch.bfloat16)
HOST_SEED = 20261017            # effective dropout seed of the host runs (the GPU test derives its own at launch time)


@pytest.fixture(scope='module')
def measured():
    """-> {dtype: {quantity: (worst ratio, case id)}} of emulate() against the float64 reference, over every case.
    On one thread: the order of torch's fp32 sums, and with it a worst-case ratio, otherwise moves with the machine's core count."""
    worst = {dt: {n: (0.0, None) for n in A.QUANTITIES} for dt in DTYPES}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        _measure(worst)
    finally:
        torch.set_num_threads(threads)
    return worst


def _measure(worst):
    for case in A.STREAM_CASES + A.WHOLE_CASES:
        inp = A.build_inputs(case)
        for dt in DTYPES:
            if A.DT_NAME[dt] not in case.dtypes:
                continue
            x = A.rounded(inp, dt)
            # the float64 reference depends on the dtype only through the rounded inputs
            ref, bnd = A.reference(case, x, HOST_SEED)
            rat = A.ratios(A.emulate(case, x, dt, HOST_SEED), ref, bnd, dt)
            for n, r in rat.items():
                assert math.isfinite(r), (case.id, A.DT_NAME[dt], n)
                if r > worst[dt][n][0]:
                    worst[dt][n] = (r, case.id)


def test_constants_table_is_what_the_emulations_measure(measured):
    """CONSTANTS is a record of this measurement, not a choice.  A quarter of slack either way, for a torch build whose fp32 sums run in
    another order than those of the build the table was measured with."""
    lines = []
    for dt in DTYPES:
        for n in A.QUANTITIES:
            r, cid = measured[dt][n]
            lines.append(f"{A.DT_NAME[dt]:>5} {n:12} {r:8.3f}  ({cid})")
    print('\n'.join(lines))
    for dt in DTYPES:
        for n in A.QUANTITIES:
            r, c = measured[dt][n][0], A.CONSTANTS[dt][n]
            assert c / 1.25 <= r <= c * 1.25, (A.DT_NAME[dt], n, r, c, '\n' + '\n'.join(lines))


def test_emulations_pass_every_bound_with_the_margin(measured):
    for dt in DTYPES:
        for n in A.QUANTITIES:
            assert measured[dt][n][0] <= A.MARGIN * A.CONSTANTS[dt][n], (A.DT_NAME[dt], n, measured[dt][n])


def _case(cid):
    return next(c for c in A.STREAM_CASES if c.id == cid)


# (fault, case id, the quantities that must break)
PLANTED = [
    # (one key of 65 moves lse by about 1 / 65: the fp32 unit sees that, the bf16 unit of 2^-9 (1 + |lse|) does not -- out does)
    ('skip_last_key_in_one_row', 'plain-d64-q127-k65', ('out', 'lse@f32')),
    ('bias_ignored_in_partial_chunk', 'layout-seqfirst-d32-kb', ('out', 'lse')),
    ('mask_without_bh_for_one_head', 'layout-packed-d32-drop', ('out', 'dq', 'dk', 'dv')),
    ('mask_seed_plus_1_in_dkv', 'layout-packed-d32-drop', ('dk', 'dv')),
    ('lse_from_dropped', 'layout-packed-d32-drop', ('lse',)),
    ('dsum_from_undropped_out', 'layout-packed-d32-drop', ('dq', 'dk')),
    ('dk_without_keep_scale', 'layout-packed-d32-drop', ('dk',)),
    ('dk_without_scale', 'layout-wide-d64', ('dk',)),
    ('stale_row_of_a_tile', 'layout-wide-d64', ('out',)),
    ('rel_w_indexed_by_kh', 'rel1-4x20', ('out', 'lse', 'dq', 'dk', 'dv', 'd_rel_h', 'd_rel_w')),
]


@pytest.mark.parametrize('fault,cid,broken', PLANTED, ids=[p[0] for p in PLANTED])
@pytest.mark.parametrize('dt', DTYPES, ids=['f32', 'bf16'])
def test_planted_fault_breaks_its_quantity(fault, cid, broken, dt):
    """The fault goes into the float64 candidate: everything else about it is exact, so whatever fails is the fault's doing.
    Judged with the bf16 unit too -- a fault must not hide inside the wider bound."""
    case = _case(cid)
    x = A.rounded(A.build_inputs(case), dt)
    ref, bnd = A.reference(case, x, HOST_SEED)
    clean = A.misses(A.ratios(ref, ref, bnd, dt), dt)
    assert not clean
    cand, _ = A.reference(case, x, HOST_SEED, fault=fault)
    failed = {n for n in A.misses(A.ratios(cand, ref, bnd, dt), dt)}
    failed = {n.split('@')[0] for n in failed}          # a quantity has to hold both of its bounds
    print(fault, A.DT_NAME[dt], 'misses:', sorted(failed))
    for n in broken:
        if '@' in n:
            n, only = n.split('@')
            if only != A.DT_NAME[dt]:
                continue
        assert n in failed, f'{fault}: {n} should have missed its bound on {cid} ({A.DT_NAME[dt]}); misses: {sorted(failed)}'
    untouched = set(ref) - set(broken)
    if fault in ('dk_without_scale', 'dk_without_keep_scale', 'lse_from_dropped', 'mask_seed_plus_1_in_dkv'):
        assert not (set(failed) & untouched), (fault, sorted(failed))          # these touch nothing else


def test_planted_faults_are_the_issue_list():
    assert [p[0] for p in PLANTED] == list(A.FAULTS)


def _autograd(case, x, M):
    """the same attention through float64 autograd; M: the pinned keep mask multiplied into P inside the graph (or None)"""
    H, scale = case.H, case.scale
    leaves = {n: x[n].clone().requires_grad_(True) for n in ('q', 'k', 'v')}
    rel = {n: x[n].clone().requires_grad_(True) for n in ('rel_h', 'rel_w') if x[n] is not None}
    q, k, v = (A._heads(leaves[n], H) for n in ('q', 'k', 'v'))
    s = q @ k.transpose(1, 2) * scale
    if x['key_bias'] is not None:
        s = s + x['key_bias'].repeat_interleave(H, 0)[:, None, :]
    if rel:
        sh, sw = case.rel
        s = (s.view(-1, case.Nq, sh, sw) + rel['rel_h'][..., None] + rel['rel_w'][:, :, None, :]).view(-1, case.Nq, case.Nk)
    P = s.softmax(-1)
    if M is not None:
        P = P * M.double() / A.keep_prob(case.p)
    out = A._unheads(P @ v, case.B)
    out.backward(x['dout'])
    res = {'out': out.detach(), 'lse': torch.logsumexp(s, -1).detach(), 'dq': leaves['q'].grad, 'dk': leaves['k'].grad, 'dv': leaves['v'].grad}
    if rel:
        res['d_rel_h'], res['d_rel_w'] = rel['rel_h'].grad, rel['rel_w'].grad
    return res


@pytest.mark.parametrize('cid', ['rel1-4x20', 'rel2-1x64', 'rel3-20x20', 'layout-seqfirst-d32-kb', 'layout-packed-d32-drop', 'dropkb-d32-q17-k5'])
def test_hand_written_gradients_equal_float64_autograd(cid):
    """rel-pos cases, a key-bias case, and dropout cases with the pinned mask multiplied into P inside the autograd graph"""
    case = _case(cid)
    x = A.rounded(A.build_inputs(case), torch.float32)
    ref, bnd = A.reference(case, x, HOST_SEED)
    M = A.keep_mask(HOST_SEED, case.B * case.H, case.Nq, case.Nk, case.p) if case.p > 0 else None
    auto = _autograd(case, x, M)
    assert set(auto) == set(ref)
    for n, r in ref.items():
        # two float64 evaluations of one expression: within 1e-12 of its magnitude sum
        assert bool(((auto[n] - r).abs() <= 1e-12 * bnd[n] + 1e-300).all()), (cid, n)


def test_mask_restatement_keep_rates_and_wrapping():
    for p in (0.1, 0.3, 0.5):
        M = A.keep_mask(12345, 4, 300, 257, p)
        assert abs(float(M.double().mean()) - (1 - p)) < 0.01, p
    # wrapping: q * Nk + key and bh * 0x9E3779B9 exceed 2^32 here; the restatement must still be a function of the low 32 bits
    a = A.keep_mask(0xfffffff0, 3, 70000, 3, 0.5)[2, 69990:, :]
    assert 0.2 < float(a.double().mean()) < 0.8
    assert A.drop_threshold(0.5) == 2 ** 31 and A.drop_threshold(0.0) == 0
    assert A.effective_seed(0xffffffff, 2) == 1 and A.effective_seed(5, -3) == 2
    # a row whose keys are all dropped exists at Nk = 5, p = 0.5 somewhere in a few hundred rows: its bound is 0 and out must be 0
    M = A.keep_mask(7, 2, 400, 5, 0.5)
    assert bool((~M.any(-1)).any())


def test_every_kernel_form_has_a_case():
    """The template combinations of sa_dispatch / sa_launch and of the whole-head dispatch against the table.  The two
    SAICV_SA_FWD2 children (tests/attn_fwd2_worker.py) count: they run the bf16 forward rows under the other two settings."""
    covered = set()
    for case in A.STREAM_CASES:
        for dt in case.dtypes:
            covered |= A.case_forms(case, dt)
        if A.fwd2_eligible(case):
            for env in (0, 2):
                covered |= A.case_forms(case, 'bf16', whiches=(0,), fwd2_env=env)
    missing = A.all_stream_forms() - covered
    assert not missing, sorted(missing)
    assert len(A.all_stream_forms()) == 3 * 12 * 2 + 4 + 1 + 1         # + sa_fwd2 REL 0 (D x KB), REL 2, REL 1
    whole = {f'attention_fwd<{dt}>' for dt in ('f32', 'bf16')} | {A.whole_bwd_form(dt, m) for dt in ('f32', 'bf16') for m in (None, '1', '2')}
    assert whole == set(A.WHOLE_FORMS)
    # the cases the forms must appear at
    ids = {c.id: c for c in A.STREAM_CASES}
    assert {c.rel for c in A.STREAM_CASES if c.rel_mode == 1} >= {(14, 14), (16, 16)} and any(c.rel_mode == 1 and c.rel[0] != c.rel[1] for c in A.STREAM_CASES)
    assert {c.rel[0] for c in A.STREAM_CASES if c.rel_mode == 2} >= {1, 3, 5, 64}
    assert (20, 20) in {c.rel for c in A.STREAM_CASES if c.rel_mode == 3}
    for D in (32, 64):
        for form in ('plain', 'kb', 'drop', 'dropkb'):
            mine = [c for c in A.STREAM_CASES if c.id.startswith(f'{form}-d{D}-')]
            assert {c.Nq for c in mine} >= set(A.NQ_SWEEP) and {c.Nk for c in mine} >= set(A.NK_SWEEP), (form, D)
            assert all(c.B * c.H <= 4 for c in mine)
            if 'drop' in form:
                assert {c.p for c in mine} == set(A.DROP_VALUES)
            if 'kb' in form:
                assert {c.bias for c in mine} == set(A.BIAS_VALUES)
    assert ids['detr-self-1764x1764'].D == 32 and ids['vit-197-12heads'].H == 12
