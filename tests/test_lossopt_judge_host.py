"""Proves the judge of tests/test_gpu_lossopt_f64.py on the host, without a GPU: the float64 references of tests/lossopt_common.py agree
with F.cross_entropy, torch.optim.SGD / AdamW, clip_grad_norm_, clip_grad_value_ and ATen's _amp_update_scale_ run on the CPU on the
cases those can express, every fp32 emulation passes the judge on every case with nothing left out, CONSTANTS is what the emulations
measure, every planted fault makes at least one named case miss, and the case tables reach every launch form of csrc/loss.hip and
csrc/optim.hip (the grid arithmetic restated in lossopt_common read back from the sources)."""
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import lossopt_common as Lc

F32, F64 = torch.float32, torch.float64
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'simpleaicv_pytorch_training_examples_amd', 'csrc')
ids = lambda c: c.id      # noqa: E731


def _close(a, b, tol=1e-12):
    same = (a == b) | (torch.isnan(a) & torch.isnan(b))
    return bool((same | ((a - b).abs() <= tol * (1e-300 + a.abs() + b.abs()))).all())


def _inputs(family):
    return Lc.opt_inputs if family in Lc.OPT_FAMILIES else Lc.FAMILIES[family][1]


def _cases(family):
    return Lc.OPT_FAMILIES[family][0] if family in Lc.OPT_FAMILIES else Lc.FAMILIES[family][0]


ALL_FAMILIES = tuple(Lc.FAMILIES) + tuple(Lc.OPT_FAMILIES)


# ------------------------------------------------------------------------------------------------ the references against torch
@pytest.mark.parametrize('case', Lc.CE_CASES, ids=ids)
def test_ce_reference_is_f_cross_entropy_in_float64(case):
    """rows: every family (a label outside [0, C) is what ignore_index expresses: no loss, no gradient; +inf and NaN rows as torch has
    them); the gradient through autograd of sum / B on the families without -inf logits"""
    inp = Lc.ce_inputs(case)
    x = inp['x'].clone().requires_grad_(case.logits != 'neginf')
    if case.soft:
        rows = F.cross_entropy(x, inp['label'], reduction='none')
    else:
        lab = inp['label']
        rows = F.cross_entropy(x, torch.where((lab >= 0) & (lab < case.C), lab, torch.full_like(lab, -100)), reduction='none', ignore_index=-100)
    spec = Lc.ce_reference(case, inp, {'row_loss': rows.detach()})
    ref, bound, got = spec['row_loss'][1], spec['row_loss'][2], rows.detach()                           # both sides cancel at |lse|: 1e-12 of the bound
    assert bool((((ref == got) | (torch.isnan(ref) & torch.isnan(got))) | ((ref - got).abs() <= 1e-12 * bound)).all()), case.id
    assert _close(spec['loss'][1], (rows.detach().sum() / case.B).reshape(1))
    if case.logits != 'neginf':
        (gx,) = torch.autograd.grad(rows.sum() / case.B, x)
        assert bool(((spec['dlogits'][1] - gx).abs() <= 1e-12 * spec['dlogits'][2] + 1e-300).all()), case.id
        assert bool((spec['dlogits'][2] >= spec['dlogits'][1].abs() * (1 - 1e-12)).all())              # the bound dominates what it bounds


def _torch_step(case, inp, state, g):
    """one torch.optim step in float64, one parameter per updated block with its state preloaded -> {name: [n]} of the new state"""
    out = {k: v.clone() for k, v in state.items()}
    upd = Lc.opt_updated(case, inp)
    inv = 1.0 if inp['inv'] is None else inp['inv']
    for b in torch.nonzero(upd).flatten().tolist():
        sl = slice(b * Lc.BLOCK, (b + 1) * Lc.BLOCK)
        h = case.groups[int(inp['bg'][b])]
        p = state['p'][sl].clone().requires_grad_(True)
        p.grad = g[sl] * inv
        if case.kind == 'sgd':
            opt = torch.optim.SGD([p], lr=h['lr'], weight_decay=h['wd'], momentum=h['mu'], nesterov=h['nesterov'] and h['mu'] != 0)
            if h['mu'] != 0:
                opt.state[p]['momentum_buffer'] = state['m'][sl].clone()
            opt.step()
            if h['mu'] != 0:
                out['m'][sl] = opt.state[p]['momentum_buffer']
        else:
            opt = torch.optim.AdamW([p], lr=h['lr'], weight_decay=h['wd'], betas=(h['b1'], h['b2']), eps=h['eps'])
            opt.state[p].update(step=torch.tensor(float(state['step'][b])), exp_avg=state['m'][sl].clone(), exp_avg_sq=state['v'][sl].clone())
            opt.step()
            out['m'][sl], out['v'][sl], out['step'][b] = opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq'], float(opt.state[p]['step'])
        out['p'][sl] = p.detach()
    return out


@pytest.mark.parametrize('case', Lc.SGD_CASES + Lc.ADAMW_CASES, ids=ids)
def test_optimizer_references_are_torch_optim_in_float64(case):
    """a skipped block (found_inf, no gradient, nobody's) is one torch.optim never sees: its state stays what it was"""
    inp = Lc.opt_inputs(case)
    state, g = inp['state'], inp['grads'][0]
    spec = Lc.opt_step_reference(case, inp, state, g)
    want = _torch_step(case, inp, state, g)
    for k in spec:
        assert _close(spec[k][1], want[k], 1e-11), (case.id, k)
    skipped = ~Lc.opt_updated(case, inp).repeat_interleave(Lc.BLOCK)
    for k in ('p', 'm', 'v'):
        if k in spec and spec[k][0] == 'bound':
            assert bool((spec[k][2][skipped] == 0).all())                                               # bound 0: held to equality


@pytest.mark.parametrize('case', [c for c in Lc.CLIP_SCALE_CASES if c.n <= 1028], ids=ids)
def test_clip_scale_reference_is_clip_grad_norm(case):
    """clip_grad_norm_ takes the norm from the gradients themselves; the kernel is handed sum g^2 rounded to fp32 (one part in 2^24)"""
    inp = Lc.clip_scale_inputs(case)
    if case.norm == 'zero':
        return
    p = torch.zeros(case.n, dtype=F64, requires_grad=True)
    p.grad = inp['g'] * (1.0 if inp['inv'] is None else inp['inv'])
    torch.nn.utils.clip_grad_norm_([p], inp['max_norm'])
    assert _close(Lc.clip_scale_reference(case, inp)['g'][1], p.grad, 2.0 ** -22), case.id


@pytest.mark.parametrize('case', [c for c in Lc.CLIP_VALUE_CASES if c.n <= 1028], ids=ids)
def test_clip_value_reference_is_clip_grad_value(case):
    """GradScaler.unscale_ then clip_grad_value_ in fp32, as the training loops run them: the same bits"""
    inp = Lc.clip_value_inputs(case)
    p = torch.zeros(case.n, dtype=F32, requires_grad=True)
    p.grad = inp['g'].to(F32) * torch.tensor(1.0 if inp['inv'] is None else inp['inv'], dtype=F32)
    torch.nn.utils.clip_grad_value_([p], case.value)
    ref = Lc.clip_value_reference(case, inp)['g'][1]
    assert _close(ref, p.grad.to(F64), 0.0), case.id
    assert math.isnan(float(ref[0])) and float(ref[1]) == Lc.f32v(case.value) and float(ref[-1]) == -Lc.f32v(case.value)


@pytest.mark.parametrize('case', Lc.SCALER_CASES, ids=ids)
def test_scaler_reference_is_atens_amp_update_scale(case):
    scale, tracker = torch.tensor([case.scale], dtype=F32), torch.tensor([int(case.tracker)], dtype=torch.int32)
    torch._amp_update_scale_(scale, tracker, torch.tensor([case.found], dtype=F32), case.growth, case.backoff, case.interval)
    ref = Lc.scaler_reference(case, Lc.scaler_inputs(case))['state'][1]
    assert float(ref[0]) == float(scale) and float(ref[1]) == float(tracker) and float(ref[2]) == float(torch.tensor(1.0) / scale), case.id


def test_scaler_table_has_the_rows_it_claims():
    c = Lc.SCALER_CASES
    assert len(c) >= 12 and any(k.interval == 1 for k in c) and any(k.found not in (0.0, 1.0) for k in c)
    assert any(k.found == 0 and k.tracker + 1 == k.interval for k in c) and any(k.found == 0 and k.tracker + 2 == k.interval for k in c)
    assert any(k.scale * k.growth > Lc.FLT_MAX for k in c)


# ------------------------------------------------------------------------------------------------ the planted edges are in the inputs
def test_cross_entropy_tables_hold_the_stated_cases():
    assert {(c.B, c.C) for c in Lc.CE_CASES} == set(Lc.CE_SHAPES) and {c.logits for c in Lc.CE_CASES} == set(Lc.CE_LOGITS)
    assert {c.soft for c in Lc.CE_CASES} == {False, True}
    assert any(c.B > 256 for c in Lc.CE_CASES) and {c.C for c in Lc.CE_CASES} >= {63, 64, 65} and sum(c.B % 4 != 0 for c in Lc.CE_CASES) > 40
    for B, C in Lc.CE_SHAPES:
        hard = [c for c in Lc.CE_CASES if (c.B, c.C) == (B, C) and not c.soft]
        bad = {v for c in hard for v in Lc.ce_invalid_rows(c).values()}
        assert bad == ({-1, -100, C, 2 ** 40} if B >= 3 else set()), (B, C)
        for c in hard:
            lab = Lc.ce_inputs(c)['label']
            assert lab.dtype == torch.int64 and all(int(lab[r]) == v for r, v in Lc.ce_invalid_rows(c).items())
            assert bool(((lab >= 0) & (lab < C)).any())
        kinds = set()
        for c in (k for k in Lc.CE_CASES if (k.B, k.C) == (B, C) and k.soft):
            kinds |= {Lc.SOFT_KINDS[(r + Lc.CE_LOGITS.index(c.logits)) % 7] for r in range(B)}
        assert kinds == set(Lc.SOFT_KINDS) or B < 3
    soft = Lc.ce_inputs(next(c for c in Lc.CE_CASES if c.soft and c.B == 9 and c.logits == 'randn3'))['label']
    sums = sorted(round(float(s), 4) for s in soft.sum(1))
    assert sums[0] == 0.0 and 0.5 in sums and 2.0 in sums and bool((soft.max(1).values == 1.0).any())
    dom = Lc.ce_inputs(next(c for c in Lc.CE_CASES if not c.soft and c.B == 9 and c.logits == 'dominant'))['x']
    p = torch.softmax(dom, 1)
    assert bool((p.min(1).values < 2.0 ** -149).all())                                                  # the rivals' softmax underflows fp32
    assert float(Lc.ce_inputs(next(c for c in Lc.CE_CASES if c.logits == 'shifted' and c.B == 9))['x'].min()) > 9000
    for c in (k for k in Lc.CE_CASES if k.logits == 'neginf' and k.C > 1):
        inp = Lc.ce_inputs(c)
        assert bool(torch.isinf(inp['x']).any()) and bool(torch.isfinite(inp['x']).any(1).all())
        if not c.soft:
            lab = inp['label']
            ok = (lab >= 0) & (lab < c.C)
            assert bool(torch.isfinite(inp['x'][ok].gather(1, lab[ok][:, None])).all())                 # never the labelled one


def test_gradient_utility_tables_hold_the_stated_cases():
    assert Lc.UTIL_SIZES == (4, 1020, 1024, 1028, 2097152, 2097156, 4194312) and [Lc.stats_sweeps(n) for n in Lc.UTIL_SIZES] == [1, 1, 1, 1, 1, 2, 3]
    st = Lc.STATS_CASES
    for n in Lc.UTIL_SIZES:
        for det in (False, True):
            assert {c.which for c in st if c.n == n and c.det == det and not c.poison} >= {'sumsq', 'both'}
            assert any(c.data == 'ints' and c.n == n and c.det == det for c in st)
        assert any(c.which == 'found' and c.n == n and c.data == 'edges' for c in st)
    spots = {(c.poison[0], c.poison[1]) for c in st if c.poison}
    assert {e for e, _ in spots} >= {0, 255, Lc.SWEEP, 2 * Lc.SWEEP} and len(spots) == 15 and {k for _, k in spots} == set(Lc.POISON)
    assert any(c.poison and c.poison[0] == c.n - 1 for c in st)
    assert {c.found_prefill for c in st if c.poison} == {0.0, 0.25} == {c.found_prefill for c in st if c.data == 'edges'}
    for c in (k for k in st if k.data == 'edges' and k.n <= 1028):
        x = Lc.stats_inputs(c)['g']
        assert float(x.abs().max()) == Lc.FLT_MAX and bool(torch.isfinite(x).all()) and 0 < float(x[1]) < 2.0 ** -126
    for c in (k for k in st if k.data == 'ints'):
        assert c.n + Lc.SUMSQ_PREFILL < 2 ** 24                                                        # every partial sum is an exact integer
    cs = Lc.CLIP_SCALE_CASES
    assert {(c.n, c.inv, c.norm) for c in cs} >= {(n, i, m) for n in Lc.UTIL_SIZES for i in Lc.INV_SCALES for m in ('above', 'below')}
    assert any(c.norm == 'zero' for c in cs) and any(c.tiny for c in cs)
    assert {(c.n, c.inv) for c in Lc.CLIP_VALUE_CASES} == {(n, i) for n in Lc.UTIL_SIZES for i in Lc.INV_SCALES}
    assert Lc.INV_SCALES['p2'] == 2.0 ** -16 and Lc.OPT_INV['p2'] == 2.0 ** -10
    assert {c.n for c in Lc.SCALE_CASES} == {1, 255, 256, 257, 524288, 524289, 1100003} and {c.dt for c in Lc.SCALE_CASES} == {'f32', 'bf16'}
    assert max(c.n for c in Lc.STATS_CASES) * 4 < 17e6                                                  # the largest buffer, bytes


def test_optimizer_tables_hold_the_stated_cases():
    for kind, cases, groups in (('sgd', Lc.SGD_CASES, Lc.SGD_GROUPS), ('adamw', Lc.ADAMW_CASES, Lc.ADAMW_GROUPS)):
        assert {c.blocks for c in cases} == {1, 2, 37} and len(groups) >= 4 and len({tuple(g.values()) for g in groups}) == len(groups)
        assert {c.has_grad for c in cases} == {'null', 'ones', 'mixed'} and {c.found for c in cases} == {'null', 'zero', 'one'}
        assert {c.inv for c in cases} == {'null', 'p2', 'third'} and {c.pscale for c in cases} >= {1.0, 1e-3}
        assert any(c.steps == 3 and c.zero_state for c in cases) and any(c.lone_group == -1 for c in cases)
        big = Lc.opt_block_group(next(c for c in cases if c.blocks == 37))
        assert set(big.tolist()) == {-1, 0, 1, 2, 3} and bool((big[1:] != big[:-1]).all())            # interleaved: a neighbour's row differs
        inp = Lc.opt_inputs(next(c for c in cases if c.blocks == 37 and c.has_grad == 'mixed'))
        assert 0 < int((inp['hg'] == 0).sum()) < 37 and int(inp['hg'].max()) > 1
        pad = torch.arange(37 * Lc.BLOCK) % Lc.BLOCK >= Lc.BLOCK - Lc.PAD
        assert all(bool((t[pad] == 0).all()) for t in list(inp['state'].values())[:2] + inp['grads'])
        small = Lc.opt_inputs(next(c for c in cases if c.pscale == 1e-3 and c.blocks == 37))['state']['p']
        assert 4e-4 < float(small[~pad].abs().min()) and float(small.abs().max()) < 1.6e-3              # of the order of lr
    assert any(g['mu'] == 0 for g in Lc.SGD_GROUPS) and any(g['wd'] == 0 for g in Lc.SGD_GROUPS) and {g['nesterov'] for g in Lc.SGD_GROUPS} == {False, True}
    assert {(g['b1'], g['b2']) for g in Lc.ADAMW_GROUPS} == {(0.9, 0.999), (0.9, 0.95), (0.0, 0.9999)} and {g['eps'] for g in Lc.ADAMW_GROUPS} == {1e-8, 1e-6}
    steps = Lc.opt_inputs(next(c for c in Lc.ADAMW_CASES if c.blocks == 37 and not c.zero_state))['state']['step']
    assert set(steps.tolist()) == {0.0, 1.0, 9.0, 999.0, 99999.0}
    assert any(c.exact for c in Lc.SGD_CASES)
    for c in (k for k in Lc.SGD_CASES if k.exact):                                                     # dyadic everything: every fma is exact
        inp = Lc.opt_inputs(c)
        for t in (inp['state']['p'], inp['state']['m'], inp['grads'][0] * inp['inv'] if inp['inv'] else inp['grads'][0]):
            assert torch.equal(t * 4, (t * 4).round())
        assert all(math.frexp(v)[0] in (0.0, 0.5) for g in c.groups for v in (g['lr'], g['wd'], g['mu']))


# ------------------------------------------------------------------------------------------------ the emulations and the constants
@pytest.fixture(scope='module')
def measured():
    """every emulated form of every case through the judge, on one thread -> (worst ratio per quantity, cases with a complaint)"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    worst, failed = {}, []
    try:
        for family in ALL_FAMILIES:
            for case in _cases(family):
                for bad in Lc.complaints(family, case, _inputs(family)(case), None, worst):
                    if bad:
                        failed.append((family, case.id, bad))
    finally:
        torch.set_num_threads(threads)
    return worst, failed


def test_every_emulation_passes_the_judge_on_every_case(measured):
    worst, failed = measured
    assert not failed, failed[:5]
    for q, r in worst.items():
        assert r <= Lc.allowed_ratio(q), (q, r)


def test_constants_table_is_what_the_emulations_measure(measured):
    """CONSTANTS is a record of this measurement, not a choice: a quarter of slack either way for another torch build"""
    worst, _ = measured
    lines = [f'{n:14} {worst.get(n, float("nan")):9.4g}  (stored {c:g}, the GPU is allowed {Lc.MARGIN:g} x)' for n, c in Lc.CONSTANTS.items()]
    print('\n'.join(lines), '\nmeasured with', Lc.CONSTANTS_MEASURED_WITH)
    assert set(Lc.CONSTANTS) | set(Lc.FIXED) == set(worst) and Lc.MARGIN == 4.0
    for n, c in Lc.CONSTANTS.items():
        assert math.isfinite(worst[n]) and c / 1.25 <= worst[n] <= c * 1.25, '\n' + '\n'.join(lines)
    assert worst['prod'] <= Lc.FIXED['prod']


def _expected_non_finite(family, case, name):
    """where the definition itself gives +inf or NaN: soft labels over -inf logits (as torch), sum g^2 of a poisoned gradient, the
    NaN that grad_clip_value keeps"""
    return ((family == 'ce' and case.soft and case.logits == 'neginf' and name in ('row_loss', 'loss'))
            or (family == 'stats' and case.poison is not None and name == 'sumsq') or family == 'clip_value')


def test_no_case_leaves_an_element_out():
    """no spec carries a keep mask: every element of every output has a reference and a bound of its own shape, the reference is finite
    wherever the kernel's result is meant to be, and it passes its own spec whole -- the cap LEFT_OUT_CAP is never drawn on"""
    assert Lc.LEFT_OUT_CAP == 0.005
    for family in tuple(Lc.FAMILIES):
        _, inputs, reference, candidates, _ = Lc.FAMILIES[family]
        for case in _cases(family):
            if Lc.case_size(case) > 1100:
                continue
            inp = inputs(case)
            spec = reference(case, inp, candidates(case, inp)[0])
            if family == 'ce':
                spec = reference(case, inp, {'row_loss': spec['row_loss'][1]})
            for name, (kind, ref, *rest) in spec.items():
                assert kind in ('equal', 'bound') and len(rest) in (0, 3) and (rest == [] or rest[0].shape == ref.shape)
                assert bool(torch.isfinite(ref).all()) or _expected_non_finite(family, case, name), (case.id, name)
            assert not Lc.judge({n: s[1] for n, s in spec.items()}, spec), case.id
    for family, (cases, _) in Lc.OPT_FAMILIES.items():
        for case in cases:
            inp = Lc.opt_inputs(case)
            spec = Lc.opt_step_reference(case, inp, inp['state'], inp['grads'][0])
            assert all(bool(torch.isfinite(s[1]).all()) and s[1].shape == inp['state'][n].shape for n, s in spec.items()), case.id
            assert not Lc.judge({n: s[1] for n, s in spec.items()}, spec), case.id


# ------------------------------------------------------------------------------------------------ every fault makes a case miss
def _catching_cases(family, fault, stop=3):
    hits = []
    for case in sorted(_cases(family), key=Lc.case_size):                                               # the small ones first
        if all(Lc.complaints(family, case, _inputs(family)(case), fault)):                              # every emulated form misses
            hits.append(case.id)
            if len(hits) >= stop:
                break
    return hits


ALL_FAULTS = [(family, fault) for family, faults in Lc.FAULTS.items() for fault in faults]


@pytest.mark.parametrize('family,fault', ALL_FAULTS, ids=[f'{a}-{b}' for a, b in ALL_FAULTS])
def test_every_planted_fault_is_caught(family, fault):
    hits = _catching_cases(family, fault)
    print(f'\n{family}: {fault} -> caught by {hits}')
    assert hits


def test_required_faults_are_all_listed():
    listed = {(family, fault) for family, fault in ALL_FAULTS}
    assert len(listed) == len(ALL_FAULTS) and not set(Lc.NEUTRAL_FAULTS) & {f for _, f in listed}
    want = {'ce': 8, 'stats': 5, 'clip_scale': 5, 'clip_value': 2, 'scale': 1, 'scaler': 3, 'sgd': 6, 'adamw': 7}
    assert all(len(Lc.FAULTS[f]) >= k for f, k in want.items())
    assert {'bc2_from_powf', 'one_minus_beta2_subtracted_in_fp32'} <= set(Lc.ADAMW_FAULTS)


def test_neutral_faults_change_nothing_observable():
    """every entry (none is listed: see the module's docstring) must leave every emulated output of every case bit-identical"""
    for fault, reason in Lc.NEUTRAL_FAULTS.items():
        assert reason
        family = next(f for f in Lc.FAMILIES if fault.startswith(f))
        _, inputs, _, candidates, _ = Lc.FAMILIES[family]
        for case in _cases(family):
            inp = inputs(case)
            for a, b in zip(candidates(case, inp), candidates(case, inp, fault)):
                assert all(torch.equal(a[k], b[k]) for k in a), (fault, case.id)


def test_what_the_rounded_lse_costs_the_gradient_is_recorded():
    """the kernels' exp(x - lse) against exp((x - max) - log(sum)) on the shifted family: the first pays u |lse| = 1e4 u per probability
    and sets the @shifted constants; the second would stay inside the allowance of the ordinary families.  Changing the kernels changes
    the bits of every training run, so it is recorded here for whoever takes that decision, not done."""
    for case in (c for c in Lc.CE_CASES if c.logits == 'shifted' and c.C > 1):
        inp = Lc.ce_inputs(case)
        q = ('ce_soft_grad' if case.soft else 'ce_hard_grad')
        ratios = []
        for shift_first in (False, True):
            worst = {}
            got = Lc.ce_emulate(case, inp, shift_first=shift_first)
            Lc.judge(got, Lc.ce_reference(case, inp, got), worst)
            ratios.append(worst[q + '@shifted'])
        print(f'\n{case.id}: exp(x - lse) {ratios[0]:.4g} u*bound, exp((x - max) - log(sum)) {ratios[1]:.4g}')
        assert ratios[1] <= Lc.allowed_ratio(q) < ratios[0]


# ------------------------------------------------------------------------------------------------ the launch geometry, from the sources
def test_restated_launch_geometry_is_the_sources():
    loss, optim = open(os.path.join(CSRC, 'loss.hip')).read(), open(os.path.join(CSRC, 'optim.hip')).read()
    assert len(re.findall(r'size_t b = \(n / 4 \+ 255\) / 256;\s+if \(b > 2048\) b = 2048;', optim)) == 3            # stats, clip_scale, clip_value
    assert len(re.findall(r'dim3\(\(unsigned\)\(n / 1024\)\), dim3\(256\)', optim)) == 2                              # sgd_flat, adamw_flat
    assert re.search(r'const int grid = \(B \+ 3\) / 4;', loss) and re.search(r'size_t b = \(n \+ 255\) / 256;\s+if \(b > 2048\) b = 2048;', loss)
    assert re.search(r'mean_rows_kernel, dim3\(1\), dim3\(256\)', loss) and 'threadIdx.x) * 4; i < n; i += gstride' in optim
    assert [Lc.stats_grid(n) for n in (4, 1020, 1024, 1028, Lc.SWEEP, Lc.SWEEP + 4)] == [1, 1, 1, 2, 2048, 2048]
    assert [Lc.scale_grid(n) for n in (1, 256, 257, Lc.SCALE_SWEEP + 1)] == [1, 1, 2, 2048] and Lc.SWEEP == 2097152 and Lc.SCALE_SWEEP == 524288
    assert [Lc.ce_grid(B) for B in (1, 4, 5, 600)] == [1, 1, 2, 150] and Lc.opt_grid(37 * 1024) == 37 and Lc.BLOCK == 1024
    assert -(-1100003 // (Lc.scale_grid(1100003) * 256)) == 3                                                        # scale_by_scalar: three sweeps
