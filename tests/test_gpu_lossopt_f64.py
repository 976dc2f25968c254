"""The eight C-ABI entry points every training iteration ends in -- saicv_softmax_ce_fwd and saicv_scale_by_scalar of csrc/loss.hip,
saicv_grad_stats, saicv_grad_clip_scale, saicv_grad_clip_value, saicv_scaler_update, saicv_sgd_flat and saicv_adamw_flat of
csrc/optim.hip -- against the float64 references of tests/lossopt_common.py: every class count around the 64-lane row, labels outside
[0, C), -inf and shifted logits, a NULL dlogits, the second and third sweep of every grid-stride loop, NaN / +inf / -inf at the first and
last element and at the head of a later sweep, both accumulation modes, hyper-parameter rows interleaved over the blocks, skipped blocks
and padding left bit-identical, parameters of the order of the learning rate, step counters up to 99 999.  Exact-regime outputs are
compared with torch.equal, nothing left out; the rest element by element against allowed * u * bound.  Outputs and in-place arenas live
in guarded allocations and the guards are compared after every launch.  Reads lossopt_common only."""
import functools

import pytest

import lossopt_common as Lc

pytestmark = pytest.mark.gpu
ids = lambda c: c.id      # noqa: E731


@functools.lru_cache(maxsize=2)
def _inputs(family, case):
    return Lc.FAMILIES[family][1](case)


def _show(case, worst):
    if worst:
        print(case.id, ' '.join(f'{q}={r:.3g} (allowed {Lc.allowed_ratio(q):.3g})' for q, r in worst.items()))


def _run(family, case):
    inp = _inputs(family, case)
    got, guards = Lc.RUNNERS[family](case, inp)
    assert not guards, guards
    spec = Lc.FAMILIES[family][2](case, inp, got)
    assert got.keys() == spec.keys()
    worst = {}
    bad = Lc.judge(got, spec, worst)
    _show(case, worst)
    assert not bad, bad
    return inp, got


@pytest.mark.parametrize('case', Lc.CE_CASES, ids=ids)
def test_softmax_ce_fwd(case):
    """row losses, the gradient, the mean of the rows the kernel wrote, and the call without dlogits bit-identical to the one with.
    Printed, never asserted: the soft row loss lse * sum(y) - sum(x y) against the reference formulation's own bound
    sum|y| |x - lse| -- what the cancellation at |lse| costs on shifted logits."""
    inp, got = _run('ce', case)
    if case.soft and case.logits == 'shifted':
        print(f'{case.id} soft-loss error / (u * sum|y||x - lse|), rows with a loss of order 1 or more = {Lc.ce_soft_tight_ratio(case, inp, got):.4g} (recorded, not asserted)')


@pytest.mark.parametrize('case', Lc.SCALE_CASES, ids=ids)
def test_scale_by_scalar(case):
    _run('scale', case)


@pytest.mark.parametrize('case', Lc.STATS_CASES, ids=ids)
def test_grad_stats(case):
    """the case's accumulation mode is set for the launch and the previous one put back; in deterministic mode a second launch gives the
    same bits"""
    from simpleaicv_pytorch_training_examples_amd import _lib
    before = _lib.lib().saicv_get_deterministic()
    inp, got = _run('stats', case)
    if case.det:
        again, guards = Lc.run_stats(case, inp)
        assert not guards and all(Lc.judge(again, {k: ('equal', v)}) == [] for k, v in got.items())
    assert _lib.lib().saicv_get_deterministic() == before


@pytest.mark.parametrize('case', Lc.CLIP_SCALE_CASES, ids=ids)
def test_grad_clip_scale(case):
    _run('clip_scale', case)


@pytest.mark.parametrize('case', Lc.CLIP_VALUE_CASES, ids=ids)
def test_grad_clip_value(case):
    _run('clip_value', case)


@pytest.mark.parametrize('case', Lc.SCALER_CASES, ids=ids)
def test_scaler_update(case):
    _run('scaler', case)


def _run_opt(case):
    inp = Lc.opt_inputs(case)
    guards, worst = [], {}
    bad = Lc.opt_check(case, inp, Lc.opt_device_stepper(case, inp, guards), worst)
    _show(case, worst)
    assert not guards, guards
    assert not bad, bad


@pytest.mark.parametrize('case', Lc.SGD_CASES, ids=ids)
def test_sgd_flat(case):
    _run_opt(case)


@pytest.mark.parametrize('case', Lc.ADAMW_CASES, ids=ids)
def test_adamw_flat(case):
    _run_opt(case)
