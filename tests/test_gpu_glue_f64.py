"""The 16 C-ABI entry points of csrc/elemwise.hip and of the stand-alone pooling kernels of csrc/pool.hip against the float64 references
of tests/glue_common.py, at every launch form: one chunk, the workgroup edges, the second trip of every grid-stride loop with a ragged
tail, every NULL form, every column geometry of the reductions in the atomic and the deterministic accumulation, the three branches of the
max-pool gradient, resize up, down, by 1 and from one pixel in the four dtype pairings.  Exact-regime cases are compared with torch.equal,
nothing left out; accuracy-regime cases element by element against allowed * u * bound, nothing sampled.  Outputs live in guarded
allocations pre-filled with NaN (`+=` targets with known integers) and the guards are compared after every launch.  Reads
tests/golden/glue_edges.pt and glue_common only."""
import functools
import os

import pytest
import torch

import glue_common as G
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
ids = lambda c: c.id      # noqa: E731


@functools.lru_cache(maxsize=4)
def _case(family, case):
    _, inputs, reference, _ = G.FAMILIES[family]
    inp = inputs(case)
    return inp, reference(case, inp)


def _show(case, got, spec):
    worst = {}
    bad = G.judge(got, spec, worst)
    if worst:
        print(case.id, ' '.join(f'{q}={r:.3g} (allowed {G.allowed_ratio(q):.3g})' for q, r in worst.items()))
    return bad


def _run(family, case):
    inp, spec = _case(family, case)
    got, guards = G.RUNNERS[family](case, inp)
    assert not guards, guards
    assert got.keys() == spec.keys()
    assert not _show(case, got, spec)
    return got


def _of(cases, *ops):
    return [c for c in cases if c.op in ops]


# ------------------------------------------------------------------------------------------------ streaming kernels
@pytest.mark.parametrize('case', _of(G.STREAM_CASES, 'relu', 'leaky', 'silu'), ids=ids)
def test_act_fwd_bwd(case):
    _run('stream', case)


@pytest.mark.parametrize('case', _of(G.STREAM_CASES, 'mul'), ids=ids)
def test_mul_fwd_bwd(case):
    _run('stream', case)


@pytest.mark.parametrize('case', _of(G.STREAM_CASES, 'swiglu'), ids=ids)
def test_swiglu_fwd_bwd(case):
    _run('stream', case)


@pytest.mark.parametrize('case', _of(G.STREAM_CASES, 'scale_add'), ids=ids)
def test_channel_scale_add_fwd(case):
    _run('stream', case)


# ------------------------------------------------------------------------------------------------ column reductions
def _mode(request, mode):
    if mode == 'deterministic':
        request.getfixturevalue('deterministic')


@pytest.mark.parametrize('mode', ['atomic', 'deterministic'])
@pytest.mark.parametrize('case', _of(G.COL_CASES, 'bn_stats'), ids=ids)
def test_bn_stats(case, mode, request):
    _mode(request, mode)
    got = _run('colred', case)
    if mode == 'deterministic':
        again, _ = G.run_colred(case, _case('colred', case)[0])
        assert all(torch.equal(again[k], got[k]) for k in got)


@pytest.mark.parametrize('mode', ['atomic', 'deterministic'])
@pytest.mark.parametrize('case', _of(G.COL_CASES, 'scale_bwd'), ids=ids)
def test_channel_scale_add_bwd(case, mode, request):
    _mode(request, mode)
    got = _run('colred', case)
    if mode == 'deterministic':
        again, _ = G.run_colred(case, _case('colred', case)[0])
        assert all(torch.equal(again[k], got[k]) for k in got)


# ------------------------------------------------------------------------------------------------ RoPE
@pytest.mark.parametrize('case', G.ROPE_CASES, ids=ids)
def test_rope_apply(case):
    _run('rope', case)


def test_rope_apply_agrees_with_the_reference_project_on_untied_tables():
    gold = torch.load(os.path.join(GOLDEN, 'glue_edges.pt'), weights_only=True)['rope']
    for case in G.rope_edge_cases():
        got, guards = G.run_rope(case, G.rope_inputs(case))
        assert not guards, guards
        assert torch.equal(got['out'][:, :, 0], gold[case.id]['q'].to(F64)) and torch.equal(got['out'][:, :, 1], gold[case.id]['k'].to(F64)), case.id


# ------------------------------------------------------------------------------------------------ bilinear resize
@pytest.mark.parametrize('case', G.RESIZE_CASES, ids=ids)
def test_resize_bilinear_add_fwd_and_bwd(case):
    _run('resize', case)


# ------------------------------------------------------------------------------------------------ pooling
@pytest.mark.parametrize('case', G.MAXPOOL_CASES, ids=ids)
def test_maxpool_fwd_bwd(case):
    """values, the recorded index plane and the gradient, ties, NaN, +-inf and uncovered pixels included"""
    _run('maxpool', case)


@pytest.mark.parametrize('case', G.AVGPOOL_CASES, ids=ids)
def test_avgpool_fwd_bwd(case):
    _run('avgpool', case)


# ------------------------------------------------------------------------------------------------ refusals, without a launch
def _refused(rc, entry, outs):
    from simpleaicv_pytorch_training_examples_amd import _lib
    torch.cuda.synchronize()
    assert rc != 0
    msg = _lib.lib().saicv_last_error_string().decode()
    assert entry in msg, msg
    with pytest.raises(RuntimeError, match=entry):
        _lib.check(rc, entry)
    for g in outs:                                          # nothing ran: every output is still NaN, every guard intact
        assert bool(torch.isnan(g.view).all()) and not [m for m in g.check('out') if 'never written' not in m]


@pytest.mark.parametrize('dt', G.DTYPES)
@pytest.mark.parametrize('entry', ['act_fwd', 'act_bwd', 'mul_fwd', 'mul_bwd', 'swiglu_fwd', 'swiglu_bwd', 'channel_scale_add_fwd',
                                   'channel_scale_add_bwd', 'bn_stats'])
def test_an_element_count_that_is_not_whole_chunks_is_refused(entry, dt):
    from simpleaicv_pytorch_training_examples_amd import _lib
    L, P, st = _lib.lib(), _lib.ptr, _lib.stream()
    code = _lib.dtype_code(G.TD[dt])
    n = 3 * G.EPC[dt] + 2
    a, b, c = (torch.ones(4 * n, dtype=G.TD[dt], device='cuda') for _ in range(3))
    s = torch.ones(4 * n, device='cuda')
    o0, o1 = G.Guarded((4 * n,), (1,), G.TD[dt], 'cuda'), G.Guarded((4 * n,), (1,), G.TD[dt], 'cuda')
    f0, f1 = G.Guarded((n,), (1,), F32, 'cuda'), G.Guarded((n,), (1,), F32, 'cuda')
    rc = {'act_fwd': lambda: L.saicv_act_fwd(code, 2, 0.0, P(a), P(o0.view), n, st),
          'act_bwd': lambda: L.saicv_act_bwd(code, 2, 0.0, P(a), P(b), P(o0.view), n, st),
          'mul_fwd': lambda: L.saicv_mul_fwd(code, P(a), P(b), P(o0.view), n, st),
          'mul_bwd': lambda: L.saicv_mul_bwd(code, P(a), P(b), P(c), P(o0.view), P(o1.view), n, st),
          'swiglu_fwd': lambda: L.saicv_swiglu_fwd(code, P(a), P(b), P(o0.view), n, st),
          'swiglu_bwd': lambda: L.saicv_swiglu_bwd(code, P(a), P(b), P(c), P(o0.view), P(o1.view), n, st),
          'channel_scale_add_fwd': lambda: L.saicv_channel_scale_add_fwd(code, P(a), P(b), P(s), P(o0.view), 4, n, st),
          'channel_scale_add_bwd': lambda: L.saicv_channel_scale_add_bwd(code, P(a), P(b), P(s), P(o0.view), P(f0.view), 4, n, st),
          'bn_stats': lambda: L.saicv_bn_stats(code, P(a), 4, n, P(f0.view), P(f1.view), st)}[entry]()
    _refused(rc, entry, [o0, o1, f0, f1])


@pytest.mark.parametrize('entry', ['resize_bilinear_add_fwd', 'resize_bilinear_bwd'])
def test_resize_refuses_channels_that_are_no_multiple_of_four(entry):
    from simpleaicv_pytorch_training_examples_amd import _lib
    L, P, st = _lib.lib(), _lib.ptr, _lib.stream()
    C = 6
    top, dout = torch.ones(1, 3, 3, C, device='cuda'), torch.ones(1, 6, 6, C, device='cuda')
    o, dtop = G.Guarded((1 * 6 * 6 * C,), (1,), F32, 'cuda'), G.Guarded((1 * 3 * 3 * C,), (1,), F32, 'cuda')
    if entry == 'resize_bilinear_add_fwd':
        rc = L.saicv_resize_bilinear_add_fwd(_lib.F32, _lib.F32, P(top), None, P(o.view), 1, 3, 3, 6, 6, C, st)
    else:
        rc = L.saicv_resize_bilinear_bwd(_lib.F32, P(dout), P(dtop.view), 1, 3, 3, 6, 6, C, st)
    _refused(rc, entry, [o, dtop])


@pytest.mark.parametrize('dt,D', [('f32', 12), ('bf16', 24), ('bf16', 8)])
def test_rope_refuses_a_head_dim_that_is_not_two_whole_chunks(dt, D):
    from simpleaicv_pytorch_training_examples_amd import _lib
    L, P = _lib.lib(), _lib.ptr
    qkv = torch.ones(1, 4, 3, 2, D, dtype=G.TD[dt], device='cuda')
    sin, cos = torch.zeros(4, D, device='cuda'), torch.ones(4, D, device='cuda')
    o = G.Guarded((qkv.numel(),), (1,), G.TD[dt], 'cuda')
    rc = L.saicv_rope_apply(_lib.dtype_code(G.TD[dt]), P(qkv), P(sin), P(cos), P(o.view), 1, 4, 2, D, 0, 0, _lib.stream())
    _refused(rc, 'rope_apply', [o])


@pytest.mark.parametrize('entry', ['maxpool_fwd', 'maxpool_bwd'])
def test_maxpool_refuses_a_window_the_index_plane_cannot_hold(entry):
    """K * K > 255 does not fit the uint8 plane: the forward and the backward both say so"""
    from simpleaicv_pytorch_training_examples_amd import _lib
    L, P, st = _lib.lib(), _lib.ptr, _lib.stream()
    K, H, C = 16, 16, 4
    x, dout = torch.ones(1, H, H, C, device='cuda'), torch.ones(1, 1, 1, C, device='cuda')
    idx = torch.zeros(1, 1, 1, C, dtype=torch.uint8, device='cuda')
    o, dx = G.Guarded((C,), (1,), F32, 'cuda'), G.Guarded((H * H * C,), (1,), F32, 'cuda')
    if entry == 'maxpool_fwd':
        rc = L.saicv_maxpool_fwd(_lib.F32, P(x), P(o.view), P(idx), 1, H, H, C, 1, 1, K, 1, 0, st)
    else:
        rc = L.saicv_maxpool_bwd(_lib.F32, P(dout), P(idx), P(dx.view), 1, H, H, C, 1, 1, K, 1, 0, st)
    _refused(rc, entry, [o, dx])
    assert bool((idx == 0).all())
