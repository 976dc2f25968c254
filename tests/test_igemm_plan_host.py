"""Host-side checks of the implicit-GEMM launch plans (no GPU): saicv_igemm_plan answers from the same plan functions the launches
ask, so which kernel form a shape takes, and what cannot be allocated in a test, can be checked here.

  closure      the case table of tests/test_gpu_igemm_exact.py reaches EVERY compiled form of igemm_nt1_kernel, igemm_tn_kernel,
               igemm_tn_dma_kernel (tests/test_kernel_asm.py pins that set against the generated assembly) and pw_stream_kernel;
  boundaries   operands at the 4 GiB buffer-addressing guards, the partial-statistics row queries, the split invariant of the
               weight gradient's deterministic fold;
  generator    the exactness bounds and the no-zero-chunk condition of every case of the table, before a GPU is used."""
import ctypes
import os
import random
import re
import sys

import pytest
import torch

from conftest import ROOT
from simpleaicv_pytorch_training_examples_amd import _lib, ops
from simpleaicv_pytorch_training_examples_amd._lib import lib
import test_gpu_igemm_exact as E

sys.path.insert(0, os.path.join(ROOT, 'scripts'))

NT_WAVES = {(256, 256): (2, 4), (256, 128): (4, 2), (128, 128): (2, 2), (128, 64): (2, 2)}
PW_NSPLIT = {(64, 64): 1, (64, 256): 4, (256, 64): 1, (128, 128): 2, (128, 512): 8, (128, 256): 4}

# Compiled forms the table does not reach: name -> why no public entry point can request it.  Empty: the forms that were unreachable
# (bf16 data gradients with an fp32 output; the K = 256 streaming forms other than the fused data gradient) are no longer compiled.
UNREACHABLE = {}


def kernel_form(case, pl):
    """The (demangled-prefix-free) name of the kernel instantiation a plan launches, as the assembly spells it."""
    t = 'DF16b' if case.dt == torch.bfloat16 else 'f'
    mode = int(case.op.endswith('dgrad'))
    if pl['route'] == E.TILED:
        tile = (pl['bm'], pl['bn'])
        return 'igemm_nt1_kernelI{}Li{}ELi{}ELi{}ELi{}ELi{}ELb{:d}ELb{:d}ELi{}EEEvNS_8NTParamsE'.format(
            t, *tile, *NT_WAVES[tile], mode, pl['out_f32'], pl['plain'], 8 if pl['kc8'] else 4)
    if pl['route'] == E.TN:
        g = (pl['bm'], pl['bn'], 2, 4 if pl['bm'] == 256 else 2)
        if pl['dma']:
            return 'igemm_tn_dma_kernelILi{}ELi{}ELi{}ELi{}ELb{:d}EEEvNS_8TNParamsE'.format(*g, pl['plain'])
        return 'igemm_tn_kernelI{}Li{}ELi{}ELi{}ELi{}EEEvNS_8TNParamsE'.format(t, *g)
    f = case.flags
    stats = bool(f.get('stats'))
    extras = bool(f.get('addend') or f.get('bn'))
    n, h, w, ci, co, k, s, p = case.shape
    kd, nd = (ci, co) if mode == 0 else (co, ci)
    taps = 9 if pl['route'] == E.PW3 else 1
    return 'pw_stream_kernelILi{}ELi{}ELi{}ELb{:d}ELb{:d}ELi{}EEEvNS_8PWParamsE'.format(kd, nd, PW_NSPLIT[(kd, nd)], stats, extras and not stats, taps)


@pytest.mark.timeout(1200)
def test_the_exact_sweep_reaches_every_compiled_igemm_and_streaming_form():
    import check_fragment_regs as F
    from test_kernel_asm import _igemm_kernels_expected
    compiled = set(_igemm_kernels_expected())
    pw = set(re.findall(r'^\s*\.amdhsa_kernel _ZN12_GLOBAL__N_1\d+(pw_stream_kernel\S+)$', F.assembly('pwstream.hip'), re.M))
    assert len(pw) == 5 * 3 + 1 + 3, sorted(pw)          # five (K, N) forms x {plain, statistics, fused dgrad}, K = 256 fused dgrad, nine taps x 3
    compiled |= pw
    reached = {}
    for c in E.CASES:
        reached.setdefault(kernel_form(c, E.plan_of(c)), c.id)
    assert set(reached) <= compiled, sorted(set(reached) - compiled)          # a plan can only name a form that exists
    missing = compiled - set(reached)
    assert missing == set(UNREACHABLE), (sorted(missing - set(UNREACHABLE)), sorted(set(UNREACHABLE) - missing))


@pytest.mark.parametrize('case', E.CASES, ids=[c.id for c in E.CASES])
def test_every_case_gets_the_plan_it_was_written_for(case):
    """Route, tile, 128-byte K slices, splits ... as the table states them, and the no-empty-split property of every weight gradient."""
    E.assert_plan(case)


def test_the_sweep_covers_every_tile_edge_and_reduction_length():
    """The coverage the table promises, counted from the plans: per tiled geometry a ragged case (M % bm and N % bn both non-zero),
    M < bm and exactly one full tile; per weight-gradient kernel and tile a reduction below one step; a last split of one step."""
    seen = {}
    for c in E.CASES:
        pl = E.plan_of(c)
        if pl['route'] == E.TILED and c.op.startswith('conv') and c.shape[6] == 1:
            n, h, w, ci, co, k, s, p = c.shape
            m, nn = n * h * w, (co if c.op == 'conv_fwd' else ci)
            kind = ('ragged' if m > pl['bm'] and m % pl['bm'] and nn % pl['bn'] else 'below' if m < pl['bm'] else
                    'one' if (m, nn) == (pl['bm'], pl['bn']) else None)
            seen.setdefault(('nt', pl['tile'], c.dt, c.op, pl['plain']), set()).add(kind)
        if pl['route'] == E.TN:
            key = ('tn', pl['bm'], pl['bn'], c.dt, pl['dma'])
            if pl['total_rt'] == 1:
                seen.setdefault(key, set()).add('below-one-step')
            if (pl['splits'] - 1) * pl['rt_per'] == pl['total_rt'] - 1 and pl['splits'] > 1:
                seen.setdefault(('tn-last-split', c.dt, pl['dma']), set()).add('one-step')
            seen.setdefault(key, set()).add('plain' if pl['plain'] else 'gathered')
    for t in range(4):
        for dt in (torch.bfloat16, torch.float32):
            if dt == torch.float32 and t == 0:
                continue
            for op in ('conv_fwd', 'conv_dgrad'):
                for plain in (0, 1):
                    assert {'ragged', 'below', 'one'} <= seen.get(('nt', t, dt, op, plain), set()), (t, dt, op, plain)
    for dt, dma in ((torch.bfloat16, 1), (torch.bfloat16, 0), (torch.float32, 0)):
        for tile in ((64, 64), (64, 128), (128, 64), (128, 128)):
            assert {'below-one-step', 'plain', 'gathered'} <= seen.get(('tn', *tile, dt, dma), set()), (tile, dt, dma)
        assert {'plain', 'gathered'} <= seen.get(('tn', 256, 256, dt, dma), set()), (dt, dma)
        assert seen.get(('tn-last-split', dt, dma)) == {'one-step'}, (dt, dma)


# ---------------------------------------------------------------------------------------------------------------- boundaries
def _query(op, dt=torch.bfloat16, conv=None, lin=None, **flags):
    q = _lib.PlanQuery()
    q.op = op
    if conv:
        q.conv = _lib.ConvDesc(*conv, _lib.dtype_code(dt))
    else:
        q.M, q.K, q.N = lin
        q.dtype = _lib.dtype_code(dt)
    for k, v in flags.items():
        setattr(q, k, v)
    pl = _lib.Plan()
    rc = lib().saicv_igemm_plan(ctypes.byref(q), ctypes.byref(pl))
    return rc, {n: getattr(pl, n) for n, _ in pl._fields_}


def _conv(n, h, w, c, k, r, stride, pad):
    return (n, h, w, c, k, r, r, stride, pad, (h + 2 * pad - r) // stride + 1, (w + 2 * pad - r) // stride + 1)


def test_operands_at_the_4gib_guards_are_never_streamed_and_are_refused_beyond(monkeypatch):
    """pw_stream addresses its source through a 32-bit buffer offset: at M K 2 >= 0xfffffff0 bytes the plan must fall back to the
    tiled kernel, which refuses the same operand (and the nine-tap form at M 128 >= 0xffffff00 - 256 bytes); one row below, it streams."""
    monkeypatch.delenv('SAICV_PW_MIN_ROWS', raising=False)
    # K = 128 (N = 128): 256 bytes per row; the guard is at 16 777 216 rows (0xfffffff0 / 256 rounded up)
    edge = -(-0xfffffff0 // 256)
    below = (edge - 1, 1, 1, 128, 128, 1, 1, 0)
    rc, pl = _query(_lib.PLAN_CONV_FWD, conv=_conv(*below), stats=1)
    assert rc == 0 and pl['route'] == E.PW, pl
    # at the guard the output tensor (M x 128 elements) already exceeds the descriptor's 2^31-element limit: refused outright
    at = (edge, 1, 1, 128, 128, 1, 1, 0)
    rc, pl = _query(_lib.PLAN_CONV_FWD, conv=_conv(*at), stats=1)
    assert rc == -1 and b'2^31' in lib().saicv_last_error_string()
    # the fused data gradient K = 256 -> N = 64: 512 bytes per source row; through a descriptor the 2^31-element limit still comes first
    edge = -(-0xfffffff0 // 512)
    rc, pl = _query(_lib.PLAN_CONV_DGRAD, conv=_conv(edge - 1, 1, 1, 64, 256, 1, 1, 0), bn_sums=1)
    assert rc == 0 and pl['route'] == E.PW, pl
    rc, pl = _query(_lib.PLAN_CONV_DGRAD, conv=_conv(edge, 1, 1, 64, 256, 1, 1, 0), bn_sums=1)
    assert rc == -1, pl
    # fp32 data passes the element limit at twice the bytes: the tiled kernel's own guard refuses a 4 GiB source
    rc, pl = _query(_lib.PLAN_CONV_FWD, torch.float32, conv=_conv(1 << 23, 1, 1, 128, 8, 1, 1, 0))
    assert rc == -1 and b'4 GiB' in lib().saicv_last_error_string(), pl
    rc, pl = _query(_lib.PLAN_CONV_FWD, torch.float32, conv=_conv((1 << 23) - 1, 1, 1, 128, 8, 1, 1, 0))
    assert rc == 0 and pl['route'] == E.TILED, pl
    # a linear product of a streamed shape has no descriptor in front of it: one row below the guard it streams, at the guard it is
    # not streamed, and the tiled kernel it falls back to refuses the operand
    edge = -(-0xfffffff0 // 256)
    rc, pl = _query(_lib.PLAN_LINEAR_FWD, lin=(edge - 1, 128, 128))
    assert rc == 0 and pl['route'] == E.PW, pl
    rc, pl = _query(_lib.PLAN_LINEAR_FWD, lin=(edge, 128, 128))
    assert rc == -1 and b'4 GiB' in lib().saicv_last_error_string(), pl
    edge = -(-0xfffffff0 // 512)
    # ... and so does a product that never streams, forward and weight gradient
    rc, pl = _query(_lib.PLAN_LINEAR_FWD, lin=(edge, 256, 64))
    assert rc == -1 and b'4 GiB' in lib().saicv_last_error_string()
    rc, pl = _query(_lib.PLAN_LINEAR_FWD, lin=(edge - 1, 256, 64))
    assert rc == 0 and pl['route'] == E.TILED
    rc, pl = _query(_lib.PLAN_LINEAR_WGRAD, lin=(edge, 256, 64))
    assert rc == -1 and b'4 GiB' in lib().saicv_last_error_string()
    rc, pl = _query(_lib.PLAN_LINEAR_WGRAD, lin=(edge - 1, 256, 64))
    assert rc == 0 and pl['route'] == E.TN and (pl['splits'] - 1) * pl['rt_per'] < pl['total_rt']
    # nine taps, 64 channels: 128 bytes per row; guard at 0xffffff00 - 256
    edge3 = -(-(0xffffff00 - 256) // 128)
    h = 4096
    n_at = -(-edge3 // (h * h))
    rc, pl = _query(_lib.PLAN_CONV_FWD, conv=_conv(n_at, h, h, 64, 64, 3, 1, 1), stats=1)
    assert rc == -1 or pl['route'] == E.TILED, pl
    rc, pl = _query(_lib.PLAN_CONV_FWD, conv=_conv(1, h, h, 64, 64, 3, 1, 1), stats=1)
    assert rc == 0 and pl['route'] == E.PW3, pl


def _random_desc(rng):
    dt = rng.choice([torch.bfloat16, torch.float32])
    epc = 8 if dt == torch.bfloat16 else 4
    k, stride = rng.choice([(1, 1), (1, 2), (3, 1), (3, 2), (7, 2), (5, 1)])
    pad = rng.choice([0, k // 2])
    c = rng.choice([8, 24, 40, 64, 128, 256, 512, 1024]) // 8 * 8
    co = rng.choice([8, 40, 64, 72, 128, 256, 264, 512, 2048])
    h, w = rng.randint(k, 80), rng.randint(k, 80)
    n = rng.choice([1, 2, 3, 32, 256])
    assert c % epc == 0 and co % epc == 0
    return dt, _conv(n, h, w, c, co, k, stride, pad)


def test_stat_rows_of_the_query_equal_the_row_queries_on_a_seeded_sample(monkeypatch):
    rng = random.Random(20260)
    L = lib()
    streamed = 0
    for i in range(3000):
        dt, cv = _random_desc(rng)
        if i % 3 == 0:
            monkeypatch.setenv('SAICV_PW_MIN_ROWS', str(rng.choice([1, 1024, 65536])))
        d = _lib.ConvDesc(*cv, _lib.dtype_code(dt))
        if d.N * d.H * d.W * d.C >= 1 << 31 or d.N * d.OH * d.OW * d.K >= 1 << 31:
            continue
        rc, pl = _query(_lib.PLAN_CONV_FWD, dt, conv=cv, stats=1)
        if rc == -1:                          # the launch would refuse it too: an fp32 operand of 4 GiB
            assert dt == torch.float32 and b'4 GiB' in L.saicv_last_error_string(), cv
            continue
        assert rc == 0 and pl['stat_rows'] == L.saicv_conv2d_stat_rows(ctypes.byref(d)), (cv, pl)
        streamed += pl['route'] != E.TILED
        rc, pl = _query(_lib.PLAN_CONV_DGRAD, dt, conv=cv, bn_sums=1)
        if rc == -1:
            assert dt == torch.float32 and b'4 GiB' in L.saicv_last_error_string(), cv
            continue
        assert rc == 0 and pl['stat_rows'] == L.saicv_conv2d_dgrad_stat_rows(ctypes.byref(d)), (cv, pl)
        streamed += pl['route'] != E.TILED
    assert streamed > 20


def test_no_planned_split_of_a_weight_gradient_is_empty(monkeypatch):
    """(splits - 1) * rt_per < total_rt: the deterministic fold sums `splits` parked tiles without zeroing them, so every split must
    own at least one reduction step -- over a seeded sample of descriptors and linear shapes, at both slot percentages."""
    rng = random.Random(7)
    n = 0
    for pct in (None, '85', '100', '37'):
        if pct is None:
            monkeypatch.delenv('SAICV_TN_SLOTS_PCT', raising=False)
        else:
            monkeypatch.setenv('SAICV_TN_SLOTS_PCT', pct)
        for _ in range(1500):
            if rng.random() < 0.5:
                dt, cv = _random_desc(rng)
                d = _lib.ConvDesc(*cv, _lib.dtype_code(dt))
                if d.N * d.H * d.W * d.C >= 1 << 31 or d.N * d.OH * d.OW * d.K >= 1 << 31:
                    continue
                rc, pl = _query(_lib.PLAN_CONV_WGRAD, dt, conv=cv)
                if rc == -1 and dt == torch.float32 and b'4 GiB' in lib().saicv_last_error_string():
                    continue
            else:
                dt = rng.choice([torch.bfloat16, torch.float32])
                m = rng.choice([1, 31, 32, 33, 63, 64, 65, rng.randint(1, 70000), 50432, 32 * 512 + 1, 64 * 512 + 1])
                rc, pl = _query(_lib.PLAN_LINEAR_WGRAD, dt, lin=(m, rng.choice([8, 64, 72, 768, 3072]), rng.choice([8, 64, 264, 768, 1024])))
            assert rc == 0
            assert pl['splits'] >= 1 and pl['rt_per'] >= 1 and (pl['splits'] - 1) * pl['rt_per'] < pl['total_rt'] <= pl['splits'] * pl['rt_per'], pl
            n += 1
    assert n > 4000


def test_the_query_refuses_what_the_entry_points_refuse():
    L = lib()
    assert L.saicv_igemm_plan(None, None) == -1
    rc, _ = _query(_lib.PLAN_CONV_FWD, conv=_conv(2, 8, 8, 8, 8, 1, 1, 0), stats=1, out_f32=1)
    assert rc == -1 and b'out_f32' in L.saicv_last_error_string()
    rc, _ = _query(_lib.PLAN_CONV_FWD, conv=_conv(2, 8, 8, 12, 8, 1, 1, 0))
    assert rc == -1 and b'multiple of 8' in L.saicv_last_error_string()
    rc, _ = _query(9, lin=(8, 8, 8))
    assert rc == -1


# ------------------------------------------------------------------------------------------------------ generator conditions
SMALL = [c for c in E.CASES if (c.shape[0] * c.shape[1] * c.shape[2] if len(c.shape) == 3 else
                                c.shape[0] * c.shape[1] * c.shape[2] * max(c.shape[3], c.shape[4]) * c.shape[5] ** 2 * max(c.shape[3], c.shape[4])) < 2e9]


@pytest.mark.timeout(1800)
def test_bounds_and_no_zero_chunk_hold_for_every_case_of_the_table():
    """make_problem() asserts the no-zero-chunk condition itself; the bounds it returns are what the GPU runner asserts before it
    launches.  Run here so that a bad case is found before a GPU is used."""
    threads = torch.get_num_threads()
    torch.set_num_threads(min(os.cpu_count() or 8, 16))
    try:
        for c in E.CASES:
            prob = E.make_problem(c)
            for name, value, limit in prob.bounds:
                assert value < limit, (c.id, name, value, limit)
            if c.regime == 'wide':          # used only where the checked result is the output tensor itself
                assert set(prob.expected) == {'out'}, c.id
            if c.flags.get('rounding'):     # the bf16 store is exercised: outputs pass 256, odd ones (ties) round to even neighbours both ways
                y, out = prob.exact, prob.expected['out'].double()
                tie = (y.abs() > 256) & (y.abs() < 512) & (y % 2 == 1)
                assert int(tie.sum()) > 100 and bool((out[tie] > y[tie]).any()) and bool((out[tie] < y[tie]).any()), c.id
                assert bool(((out[tie] / 2) % 2 == 0).all()), c.id          # ... each to the neighbour with an even mantissa
    finally:
        torch.set_num_threads(threads)


def _first(id_):
    return next(c for c in E.CASES if c.id == id_)


def test_the_faults_the_tolerances_absorbed_change_the_reference():
    """The three localised faults a 2e-2 / 4e-3 / 1e-3 budget absorbs, applied to the REFERENCE of a table case: each makes
    torch.equal false, so the same fault in a kernel fails the sweep.  (No kernel is edited to fail.)"""
    # 1. a weight gradient that loses the last 32 rows of its reduction
    c = _first('r50-1024to256-wgrad-bf16')
    prob = E.make_problem(c)
    x, dy = prob.inputs['x'].reshape(-1, 1024), prob.inputs['dy'].reshape(-1, 256)
    faulty = (prob.inputs['dw0'].reshape(256, 1024) + dy[:-32].t() @ x[:-32]).float()
    assert not torch.equal(faulty, prob.expected['dw'].reshape(256, 1024))
    assert torch.equal((prob.inputs['dw0'].reshape(256, 1024) + dy.t() @ x).float(), prob.expected['dw'].reshape(256, 1024))
    # 2. a forward launch that leaves the last 256-row tile out of the partial sums of squares
    c = _first('r50-1024to256-fwd-stats-bf16')
    prob = E.make_problem(c)
    y = prob.expected['out'].double()
    assert torch.equal((y * y).sum(0), prob.expected['stat_sq'])
    assert not torch.equal((y[:-256] * y[:-256]).sum(0), prob.expected['stat_sq'])
    assert not torch.equal(y[:-256].sum(0), prob.expected['stat_sum'])
    # 3. one output element that misses one 16-byte K chunk of K = 4608.  Where the stored value is exact (fp32 output; bf16 output of the
    # narrow regime, all below 256) every chunk with a non-zero partial product changes it.  (A bf16 output ABOVE 256 can round a
    # change of +-1 away: the wide bf16 cases are there for the store, the narrow and fp32 ones for the sums.)
    for cid in ('deep-k-fwd-stats-bf16', 'deep-k-fwd-fp32'):
        c = _first(cid)
        prob = E.make_problem(c)
        x, wf = prob.inputs['x'], prob.inputs['wf']
        epc = 8 if c.dt == torch.bfloat16 else 4
        col = 17                                                        # pixel (3, 3) of image 0: an interior pixel, no tap is padding
        patch = x[0, 2:5, 2:5, :].reshape(-1)                           # (r, s, c) order, as the weights
        partial = (patch * wf[col].reshape(-1)).reshape(-1, epc).sum(1)
        assert float(partial.sum()) == float(prob.exact[3 * 7 + 3, col])
        hit = partial.nonzero().squeeze(1)
        assert len(hit) >= len(partial) // 16, (cid, len(hit), len(partial))
        for ch in hit[:8].tolist():
            faulty = prob.exact.clone()
            faulty[3 * 7 + 3, col] -= partial[ch]
            stored = faulty.float() if c.dt == torch.float32 else faulty.to(torch.bfloat16)
            assert not torch.equal(stored, prob.expected['out']), (cid, ch)
