"""saicv_dwconv2d_fwd, saicv_dwconv2d_dgrad and saicv_dwconv2d_wgrad of csrc/dwconv.hip against the float64 references of
tests/dwconv_common.py, at every launch form: the walk kernel (K = 3, 5, 7) at pad 0, "same", K - 1 and beyond it, the gather kernel at
even kernel sizes, strides 2 and 3, dilation and the data-gradient fallback, destination widths around the eight- and four-pixel tiles,
the weight gradient at every K with dead chunk lanes, the 256-lane cap, one, two and 33 pixel ranges, with and without a bias gradient, in
the atomic and the deterministic accumulation, and the second trip of both grid-stride loops.  Exact-regime cases are compared with
torch.equal, nothing left out; accuracy-regime cases element by element against allowed * u * bound, nothing sampled.  Outputs live in
guarded allocations pre-filled with NaN (`+=` targets with known integers) and the guards are compared after every launch."""
import functools

import pytest
import torch

import dwconv_common as D
from test_gpu_glue_f64 import _refused

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
ids = lambda c: c.id      # noqa: E731


@functools.lru_cache(maxsize=4)
def _case(case):
    inp = D.inputs(case)
    return inp, D.reference(case, inp)


def _show(case, got, spec):
    worst = {}
    bad = D.judge(got, spec, worst)
    if worst:
        print(case.id, ' '.join(f'{q}={r:.3g} (allowed {D.allowed_ratio(q):.3g})' for q, r in worst.items()))
    return bad


def _run(runner, case):
    inp, spec = _case(case)
    got, guards = runner(case, inp)
    assert not guards, guards
    assert got.keys() == spec.keys()
    assert not _show(case, got, spec)
    return got


def _zeros_where_nothing_reads(case, got):
    rows, cols = D.unread(case)
    dx = got['dx'].view(case.N, case.H, case.W, case.C)
    assert bool((dx[:, rows] == 0).all()) and bool((dx[:, :, cols] == 0).all())      # exact zeros, not NaN


# ------------------------------------------------------------------------------------------------ forward and data gradient
@pytest.mark.parametrize('case', D.WALK_CASES, ids=ids)
def test_walk_fwd_and_dgrad(case):
    _zeros_where_nothing_reads(case, _run(D.run_conv, case))


@pytest.mark.parametrize('case', D.GATHER_CASES, ids=ids)
def test_gather_fwd_and_dgrad(case):
    _zeros_where_nothing_reads(case, _run(D.run_conv, case))


@pytest.mark.parametrize('case', D.BIG_CASES, ids=ids)
def test_second_trip_of_the_grid_stride_loop(case):
    """more than 16384 x 256 one-pixel items: bf16, exact regime, against shifted elementwise products"""
    from simpleaicv_pytorch_training_examples_amd import _lib
    L, P, st = _lib.lib(), _lib.ptr, _lib.stream()
    assert D.dw_trips(case.fwd_items) == 2 and D.dw_trips(case.dgrad_items) == 2
    inp = D.big_inputs(case)
    ref = D.big_reference(case, inp)
    dev = lambda t: t.to(torch.bfloat16).cuda()      # noqa: E731
    x, dy, wt, b = dev(inp['x']), dev(inp['dy']), D.tap_major(inp['w'], 'bf16', 'cuda'), inp['b'].cuda()
    shape = (case.N, case.H, 1, case.C)
    y, dx = D._guard(shape, 'bf16', 'cuda'), D._guard(shape, 'bf16', 'cuda')
    _lib.check(L.saicv_dwconv2d_fwd(_lib.BF16, P(x), P(wt), P(b), P(y.view), *D._args(case), st), 'dwconv2d_fwd')
    _lib.check(L.saicv_dwconv2d_dgrad(_lib.BF16, P(dy), P(wt), P(dx.view), *D._args(case), st), 'dwconv2d_dgrad')
    torch.cuda.synchronize()
    assert not y.check('y') and not dx.check('dx')
    assert torch.equal(y.view.float().cpu(), ref['y']) and torch.equal(dx.view.float().cpu(), ref['dx'])


# ------------------------------------------------------------------------------------------------ weight gradient
@pytest.mark.parametrize('mode', ['atomic', 'deterministic'])
@pytest.mark.parametrize('case', D.WGRAD_CASES, ids=ids)
def test_wgrad(case, mode, request):
    """both accumulation modes against the same reference, pre-fill included; the ordered result is the same bits on a second launch"""
    if mode == 'deterministic':
        request.getfixturevalue('deterministic')
    got = _run(D.run_wgrad, case)
    if mode == 'deterministic':
        again, _ = D.run_wgrad(case, _case(case)[0])
        assert all(torch.equal(again[k], got[k]) for k in got)


# ------------------------------------------------------------------------------------------------ refusals, without a launch
def _entries(dt, N, H, W, C, OH, OW, K, stride, pad, dil, code=None):
    """-> {entry: (call, outputs)} on valid operands sized for the largest extent either side claims"""
    from simpleaicv_pytorch_training_examples_amd import _lib
    L, P, st = _lib.lib(), _lib.ptr, _lib.stream()
    code = _lib.dtype_code(D.TD[dt]) if code is None else code
    n = max(N, 1) * max(H, OH, 1) * max(W, OW, 1) * max(C, 8)
    x, dy = torch.ones(n, dtype=D.TD[dt], device='cuda'), torch.ones(n, dtype=D.TD[dt], device='cuda')
    wt, b = torch.ones(81 * max(C, 8), dtype=D.TD[dt], device='cuda'), torch.ones(max(C, 8), device='cuda')
    y, dx = D.Guarded((n,), (1,), D.TD[dt], 'cuda'), D.Guarded((n,), (1,), D.TD[dt], 'cuda')
    dw, db = D.Guarded((81 * max(C, 8),), (1,), F32, 'cuda'), D.Guarded((max(C, 8),), (1,), F32, 'cuda')
    a = (N, H, W, C, OH, OW, K, stride, pad, dil)
    return {'dwconv2d_fwd': (lambda: L.saicv_dwconv2d_fwd(code, P(x), P(wt), P(b), P(y.view), *a, st), [y]),
            'dwconv2d_dgrad': (lambda: L.saicv_dwconv2d_dgrad(code, P(dy), P(wt), P(dx.view), *a, st), [dx]),
            'dwconv2d_wgrad': (lambda: L.saicv_dwconv2d_wgrad(code, P(dy), P(x), P(dw.view), P(db.view), *a, st), [dw, db])}


ENTRIES = ('dwconv2d_fwd', 'dwconv2d_dgrad', 'dwconv2d_wgrad')
# what: (C as chunks + elements, K, stride, pad, dil, dtype code or None) on a 6 x 6 image
REFUSED = {'c_not_whole_chunks': (1, 2, 3, 1, 1, 1, None), 'k0': (1, 0, 0, 1, 0, 1, None), 'k9': (1, 0, 9, 1, 4, 1, None), 'stride0': (1, 0, 3, 0, 1, 1, None),
           'dilation0': (1, 0, 3, 1, 1, 0, None), 'negative_pad': (1, 0, 3, 1, -1, 1, None), 'unknown_dtype': (1, 0, 3, 1, 1, 1, 7)}


@pytest.mark.parametrize('dt', D.DTYPES)
@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('what', sorted(REFUSED))
def test_a_geometry_the_kernels_do_not_have_is_refused(what, entry, dt):
    chunks, extra, K, stride, pad, dil, code = REFUSED[what]
    call, outs = _entries(dt, 2, 6, 6, chunks * D.EPC[dt] + extra, 6, 6, K, stride, pad, dil, code)[entry]
    _refused(call(), entry, outs)


@pytest.mark.parametrize('dt', D.DTYPES)
@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('oh,ow', [(7, 6), (6, 5), (5, 6), (6, 7), (0, 6)])
def test_an_output_extent_that_does_not_match_the_geometry_is_refused(oh, ow, entry, dt):
    """3 x 3, stride 1, pad 1 on 6 x 6 gives 6 x 6 and nothing else"""
    call, outs = _entries(dt, 2, 6, 6, D.EPC[dt], oh, ow, 3, 1, 1, 1)[entry]
    _refused(call(), entry, outs)


@pytest.mark.parametrize('dt', D.DTYPES)
@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('empty', ['no_image', 'kernel_does_not_fit'])
def test_an_empty_problem_is_no_launch_and_no_error(empty, entry, dt):
    """N == 0, or a 3 x 3 kernel on a 2 x 6 image without padding (OH == 0): 0 is returned, nothing is written"""
    N, H, OH, OW = (0, 6, 4, 4) if empty == 'no_image' else (2, 2, 0, 4)
    call, outs = _entries(dt, N, H, 6, D.EPC[dt], OH, OW, 3, 1, 0, 1)[entry]
    assert call() == 0
    torch.cuda.synchronize()
    for g in outs:
        assert bool(torch.isnan(g.view).all()) and not [m for m in g.check('out') if 'never written' not in m]


# ------------------------------------------------------------------------------------------------ the wrapper
@pytest.mark.parametrize('dt', D.DTYPES)
def test_ops_depthwise_conv2d_layouts_and_frozen_operands(dt):
    """what the C-ABI cases cannot reach: an NCHW-contiguous input, a non-contiguous dy, bias=None, and the three needs_input_grad
    combinations (input frozen; weight frozen with a trainable bias; everything frozen but the input), judged by the same judge"""
    from simpleaicv_pytorch_training_examples_amd import ops
    nchw = lambda t: t.permute(0, 3, 1, 2).contiguous()      # noqa: E731
    for bias in (True, False):
        case = D.DwCase(f'wrapper-{dt}-k3s2-{"b" if bias else "nob"}', 'gather', dt, 2, 7, 9, 3, 3, 2, 1, 1, bias, False)
        inp = D.inputs(case)
        wcase = D.DwCase(case.id, 'wgrad', dt, case.N, case.H, case.W, case.cpr, case.K, case.stride, case.pad, case.dil, bias, False)
        spec = {**D.reference(case, inp), **D.reference(wcase, inp)}
        pw, pb = D.dw_prefill(case)                        # the wrapper accumulates into zeros: the pre-fill is taken off again below
        x = nchw(inp['x']).to(D.TD[dt]).cuda()
        assert x.is_contiguous() and not x.is_contiguous(memory_format=torch.channels_last)
        dy_wide = torch.zeros((case.N, case.C, case.OH, 2 * case.OW), dtype=D.TD[dt], device='cuda')
        dy_wide[..., ::2] = nchw(inp['dy']).to(D.TD[dt]).cuda()
        dy = dy_wide[..., ::2]
        assert not dy.is_contiguous() and not dy.is_contiguous(memory_format=torch.channels_last)
        w, b = inp['w'].float().cuda(), (inp['b'].float().cuda() if bias else None)
        combos = [(False, True, True), (True, False, True), (True, False, False)] if bias else [(False, True, False), (True, False, False), (True, True, False)]
        for need_x, need_w, need_b in combos:
            xi, wi = x.clone().requires_grad_(need_x), w.clone().requires_grad_(need_w)
            bi = b.clone().requires_grad_(need_b) if bias else None
            y = ops.depthwise_conv2d(xi, wi, bi, case.stride, case.pad, case.dil)
            assert tuple(y.shape) == (case.N, case.C, case.OH, case.OW) and y.dtype == D.TD[dt]
            y.backward(dy)
            torch.cuda.synchronize()
            got, sub = {'y': y.detach().permute(0, 2, 3, 1)}, {'y': spec['y']}
            assert (xi.grad is not None) == need_x and (wi.grad is not None) == need_w and (bi is None or (bi.grad is not None) == need_b)
            if need_x:
                got['dx'], sub['dx'] = xi.grad.permute(0, 2, 3, 1), spec['dx']
            if need_w:
                got['dw'], sub['dw'] = wi.grad[:, 0].permute(1, 2, 0).reshape(case.K ** 2, case.C).double().cpu() + pw, spec['dw']
            if need_b:
                got['db'], sub['db'] = bi.grad.double().cpu() + pb, spec['db']
            assert not _show(case, got, sub), (bias, need_x, need_w, need_b)
