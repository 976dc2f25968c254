"""SAM's own kernels (csrc/sam.hip, csrc/samtail.hip, csrc/maskloss.hip) at every dispatch form, through the C-ABI with outputs inside
sentinel guards: structure bit for bit on operands every precision holds exactly, accuracy element by element against the float64
references of tests/sam_common.py, in atomic and in deterministic mode, and the argument checks.  The judge, its bounds and its
constants are sam_common's; tests/test_sam_judge_host.py shows what they catch."""
import math

import pytest
import torch

import sam_common as S

pytestmark = pytest.mark.gpu

DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16}
MODES = ('atomic', 'deterministic')
LEDGER = {}                     # (family, dtype name, quantity) -> (worst ratio / allowed, case id)
_CACHE = {}                     # key -> inputs and float64 reference of a case: computed once, never modified


def _cached(key, make):
    if key not in _CACHE:
        if len(_CACHE) >= 2:    # the 128 x 64 reference and its bounds are 200 MB
            _CACHE.clear()
        _CACHE[key] = make()
    return _CACHE[key]


def _enter(mode, request):
    from simpleaicv_pytorch_training_examples_amd._lib import lib
    if mode == 'deterministic':
        request.getfixturevalue('deterministic')
    assert bool(lib().saicv_get_deterministic()) == (mode == 'deterministic')


def _judge(family, cid, dt, got, ref, bnd, problems):
    rat = S.ratios(got, ref, bnd, DTYPES[dt])
    for n, r in rat.items():
        allowed = S.MARGIN * S.constant(n, DTYPES[dt])
        rel = r / allowed if allowed > 0 else (0.0 if r == 0 else math.inf)
        if rel >= LEDGER.get((family, dt, n), (-1.0, None))[0]:
            LEDGER[(family, dt, n)] = (rel, cid)
    print(cid, dt, ' '.join(f'{n}={r:.3g}' for n, r in rat.items()))
    for n, (r, lim) in S.misses(rat, DTYPES[dt]).items():
        problems.append(f'{cid} [{dt}] {n}: worst |got - ref| is {r:.4g} u*bound, allowed {lim:.4g}')


def _same(name, got, ref, problems):
    g = got.double().reshape(ref.shape)
    if not torch.equal(g, ref):
        bad = g != ref
        i = int(bad.flatten().nonzero()[0])
        problems.append(f'{name}: {int(bad.sum())} of {ref.numel()} elements differ from float64, first at flat index {i} '
                        f'(got {float(g.flatten()[i])}, expected {float(ref.flatten()[i])})')


# ------------------------------------------------------------------------------------------------ relpos
def _relpos_exact(case):
    def make():
        x = S.relpos_inputs(case, torch.float32, exact=True)
        ref, _ = S.relpos_math(case, x)
        lim = S.relpos_exact_limits(case)
        for n, r in ref.items():            # every result is an integer the formats hold
            assert torch.equal(r, r.round()) and float(r.abs().max()) <= lim[n], (case.id, n)
        assert torch.equal(ref['dq'].to(torch.bfloat16).double(), ref['dq'])
        return x, ref
    return _cached((case.id, 'exact'), make)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('case', S.RELPOS_CASES, ids=lambda c: c.id)
def test_relpos_structure_bit_for_bit(case, dt, mode, request):
    """entries in {-1, 0, 1}: rel_h, rel_w, prior dq + increment and prior table gradients + increment equal the integer einsums"""
    _enter(mode, request)
    x, ref = _relpos_exact(case)
    got, problems = S.run_relpos(case, x, DTYPES[dt])
    for n in S.RELPOS_Q:
        _same(f'{case.id} [{dt}, {mode}] {n}', got[n], ref[n], problems)
    assert not problems, '\n'.join(problems)


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('case', [c for c in S.RELPOS_CASES if (c.Sh, c.Sw, c.heads) in ((14, 14, 3), (32, 32, 3), (64, 64, 3), (128, 64, 3))
                                  and not c.contiguous], ids=lambda c: c.id)
def test_relpos_without_table_gradients(case, dt):
    """dtab = NULL (the recomputing backward of a checkpointed block asks for dq alone): the same dq, nothing else written"""
    x, ref = _relpos_exact(case)
    got, problems = S.run_relpos(case, x, DTYPES[dt], tables=False)
    for n in ('rel_h', 'rel_w', 'dq'):
        _same(f'{case.id} [{dt}] {n}', got[n], ref[n], problems)
    assert not problems, '\n'.join(problems)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('case', S.RELPOS_ACCURACY_CASES, ids=lambda c: c.id)
def test_relpos_against_float64(case, dt, mode, request):
    _enter(mode, request)

    def make():
        x = S.relpos_inputs(case, DTYPES[dt], exact=False)
        return (x,) + S.relpos_math(case, x, bounds=True)
    x, ref, bnd = _cached((case.id, dt), make)
    got, problems = S.run_relpos(case, x, DTYPES[dt])
    _judge(f'relpos {mode}', case.id, dt, got, ref, bnd, problems)
    assert not problems, '\n'.join(problems)


# ------------------------------------------------------------------------------------------------ windows
@pytest.mark.parametrize('shape', S.WINDOW_CASES, ids=lambda s: 'x'.join(str(v) for v in s[:5]))
def test_window_kernels_move_every_element_and_add_once(shape):
    B, H, W, C, ws, dts = shape
    for dt in dts:
        g = torch.Generator().manual_seed(H * 7 + ws + C)
        x = torch.randn(B, H, W, C, generator=g).to(DTYPES[dt])
        add = torch.randn(B, H, W, C, generator=g).to(DTYPES[dt])
        win, back, fused, problems = S.run_window(x, add, ws)
        ref = S.window_reference(x, ws)
        if not torch.equal(win, ref):
            problems.append(f'[{dt}] window_partition differs from pad + view + permute in {int((win != ref).sum())} elements')
        if not torch.equal(back, x):
            problems.append(f'[{dt}] window_unpartition does not return the input in {int((back != x).sum())} elements')
        want = (x.float() + add.float()).to(DTYPES[dt])
        if not torch.equal(fused, want):
            problems.append(f'[{dt}] the fused residual add differs from one rounded addition in {int((fused != want).sum())} elements')
        assert not problems, '\n'.join(problems)


# ------------------------------------------------------------------------------------------------ x4 bilinear
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('planes', S.UP4_PLANES)
@pytest.mark.parametrize('hw', S.UP4_HW, ids=lambda s: f'{s[0]}x{s[1]}')
def test_upsample4_structure_bit_for_bit(hw, planes, dt):
    """multiples of 1/8: fp32 equals float64 in every bit, bf16 equals float64 rounded once"""
    low, dhi = S.up4_exact_inputs(planes, *hw)
    out, dlow = S.up4(low), S.up4_adjoint(dhi)
    assert torch.equal(out.float().double(), out) and torch.equal(dlow.float().double(), dlow)      # exact in fp32
    got, problems = S.run_up4(low, dhi, DTYPES[dt])
    _same(f'{hw} x{planes} [{dt}] out', got['out'], out.to(DTYPES[dt]).double(), problems)
    _same(f'{hw} x{planes} [{dt}] dlow', got['dlow'], dlow.to(DTYPES[dt]).double(), problems)
    assert not problems, '\n'.join(problems)


# ------------------------------------------------------------------------------------------------ hyper-network product
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('case', S.HYPER_CASES, ids=lambda c: c.id)
def test_hyper_product_structure_and_accuracy(case, dt, mode, request):
    _enter(mode, request)
    x = S.hyper_inputs(case, DTYPES[dt], exact=True)
    ref, _ = S.hyper_math(case, x)
    assert all(torch.equal(r, r.round()) for r in ref.values())
    assert float(ref['hp_out'].abs().max()) <= 32 and float(ref['hp_dx'].abs().max()) <= 8
    assert float(ref['hp_dhyper'].abs().max()) <= (256 if dt == 'bf16' else 2 ** 24)
    got, problems = S.run_hyper(case, x, DTYPES[dt])
    for n in S.HYPER_Q:
        _same(f'{case.id} [{dt}, {mode}] {n}', got[n], ref[n], problems)
    x = S.hyper_inputs(case, DTYPES[dt], exact=False)
    ref, bnd = S.hyper_math(case, x, bounds=True)
    got, bad = S.run_hyper(case, x, DTYPES[dt])
    problems += bad
    _judge(f'hyper {mode}', case.id, dt, got, ref, bnd, problems)
    assert not problems, '\n'.join(problems)


# ------------------------------------------------------------------------------------------------ mask loss
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('thr', [0.0, 0.5])
@pytest.mark.parametrize('route,hw', [('plain', s) for s in S.PLAIN_HW] + [('up4', s) for s in S.UP4_HW],
                         ids=lambda v: v if isinstance(v, str) else f'{v[0]}x{v[1]}')
def test_iou_counts_are_exact_and_a_logit_at_the_threshold_is_not_above_it(route, hw, thr, dt, mode, request):
    _enter(mode, request)
    x, t = S.count_inputs(route, *hw, thr, DTYPES[dt])
    xf = S.up4(x) if route == 'up4' else x
    assert torch.equal(xf.float().double(), xf) and bool((xf == thr).any())
    case = S.Mask(route, hw[0], hw[1], x.shape[0], x.shape[1], 2.0, 1.0, (1, 1, 1))
    coef = torch.ones(x.shape[0], x.shape[1], 3, dtype=torch.float64)
    ref, _ = S.mask_reference(case, x, t, coef, thr=thr)
    got, problems = S.run_mask(route, x, t, coef, 2.0, thr, DTYPES[dt])
    _same(f'{route} {hw} thr={thr} [{dt}, {mode}] stats[4]', got['count_and'], ref['count_and'], problems)
    _same(f'{route} {hw} thr={thr} [{dt}, {mode}] stats[5]', got['count_or'], ref['count_or'], problems)
    assert not problems, '\n'.join(problems)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('route,hw', [('plain', s) for s in S.PLAIN_HW] + [('up4', s) for s in S.UP4_HW],
                         ids=lambda v: v if isinstance(v, str) else f'{v[0]}x{v[1]}')
def test_mask_loss_against_float64(route, hw, dt, mode, request):
    """the nine (gamma, logit scale) pairs of the size; deterministic mode: the same judge, and a second run bit-identical"""
    _enter(mode, request)
    table = S.MASK_UP4_CASES if route == 'up4' else S.MASK_PLAIN_CASES
    problems = []
    for case in (c for c in table if (c.h, c.w) == hw):
        def make():
            x, t, coef = S.mask_inputs(case, DTYPES[dt])
            return (x, t, coef) + S.mask_reference(case, x, t, coef)
        x, t, coef, ref, bnd = _cached((case.id, dt), make)
        got, bad = S.run_mask(route, x, t, coef, case.gamma, 0.0, DTYPES[dt], raw=True)
        problems += [f'{case.id} [{dt}] {m}' for m in bad]
        _judge(f'mask {mode}', case.id, dt, got, ref, bnd, problems)
        _same(f'{case.id} [{dt}] stats[4]', got['count_and'], ref['count_and'], problems)
        _same(f'{case.id} [{dt}] stats[5]', got['count_or'], ref['count_or'], problems)
        if mode == 'deterministic':
            again, _ = S.run_mask(route, x, t, coef, case.gamma, 0.0, DTYPES[dt], raw=True)
            if not (torch.equal(again['raw_stats'], got['raw_stats']) and torch.equal(again['raw_grad'], got['raw_grad'])):
                problems.append(f'{case.id} [{dt}] two deterministic runs differ')
    assert not problems, '\n'.join(problems)


# ------------------------------------------------------------------------------------------------ argument checks
def _rejected(rc, *words):
    msg = S.last_error()
    assert rc != 0, 'the call was accepted'
    assert msg and all(w in msg for w in words), msg
    torch.cuda.synchronize()


def test_argument_checks_return_an_error_and_a_message():
    """no launch: every output still holds what it was pre-filled with"""
    from simpleaicv_pytorch_training_examples_amd._lib import dtype_code, lib, ptr, stream
    L, dev = lib(), 'cuda'
    out = torch.full((1 << 16,), S.SENTINEL, dtype=torch.float32, device=dev)
    buf = torch.zeros(1 << 22, dtype=torch.float32, device=dev)         # every input pointer: large enough for each call below
    for dt in (torch.float32, torch.bfloat16):
        dc, n = dtype_code(dt), (8 if dt == torch.bfloat16 else 4)
        for sh, sw, words in ((129, 8, ('Sh=129',)), (8, 65, ('Sw=65',))):
            _rejected(L.saicv_relpos_fwd(dc, ptr(buf), 192, 192 * sh * sw, ptr(buf), ptr(buf), ptr(out), ptr(out), 1, 3, sh, sw, stream()), *words)
            _rejected(L.saicv_relpos_bwd(dc, ptr(buf), ptr(out), 192, 192 * sh * sw, ptr(buf), ptr(buf), ptr(buf), ptr(buf), ptr(out), ptr(out),
                                         ptr(out), 1, 3, sh, sw, stream()), *words)
        rs = 192 + n // 2                                                # a multiple of 4 and not of 8 in bf16, of 2 and not of 4 in fp32
        _rejected(L.saicv_relpos_fwd(dc, ptr(buf), rs, rs * 64, ptr(buf), ptr(buf), ptr(out), ptr(out), 1, 3, 8, 8, stream()), 'strides')
        _rejected(L.saicv_relpos_bwd(dc, ptr(buf), ptr(out), rs, rs * 64, ptr(buf), ptr(buf), ptr(buf), ptr(buf), ptr(out), ptr(out), ptr(out),
                                     1, 3, 8, 8, stream()), 'strides')
        _rejected(L.saicv_hyper_product_fwd(dc, ptr(buf), ptr(buf), ptr(out), 1, 4, 100, 16, stream()), 'C=16')
        _rejected(L.saicv_hyper_product_bwd(dc, ptr(buf), ptr(buf), ptr(buf), ptr(out), ptr(out), 1, 4, 100, 16, stream()), 'C=16')
        _rejected(L.saicv_hyper_product_fwd(dc, ptr(buf), ptr(buf), ptr(out), 1, 9, 100, 32, stream()), 'T=9')
        _rejected(L.saicv_hyper_product_bwd(dc, ptr(buf), ptr(buf), ptr(buf), ptr(out), ptr(out), 1, 9, 100, 32, stream()), 'T=9')
    bf = dtype_code(torch.bfloat16)
    _rejected(L.saicv_mask_loss_stats(bf, ptr(buf), ptr(buf), ptr(out), 1, 1, 12, 0.25, 2.0, 0.0, stream()), 'H*W=12', 'multiple of 8')
    _rejected(L.saicv_mask_loss_grad(bf, ptr(buf), ptr(buf), ptr(buf), ptr(out), 1, 1, 12, 0.25, 2.0, stream()), 'H*W=12', 'multiple of 8')
    assert bool((out == S.SENTINEL).all())
    # what the size check says is what it admits
    _rejected(L.saicv_relpos_fwd(dtype_code(torch.float32), ptr(buf), 192, 192 * 129, ptr(buf), ptr(buf), ptr(out), ptr(out), 1, 3, 129, 1, stream()),
              'Sh <= 128', 'Sw <= 64')


@pytest.fixture(scope='module', autouse=True)
def _ledger():
    """Not a check: after the module's last test prints, per kernel family, mode, dtype and quantity, the worst observed error as a
    fraction of what the judge allows (run with -s), and names what came within a factor of two."""
    yield
    for key in sorted(LEDGER):
        rel, cid = LEDGER[key]
        print(f'LEDGER {key[0]:22} {key[1]:5} {key[2]:10} {rel:6.3f} of allowed  ({cid}){"   <-- within 2x" if rel > 0.5 else ""}')
