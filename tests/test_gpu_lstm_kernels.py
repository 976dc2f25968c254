"""ops.lstm (csrc/lstm.hip + the implicit-GEMM kernels) against the float64 judge of tests/lstm_common.py, in fp32 and bf16, at the
smallest shapes at which each mechanism can break.  Bound for every output (y, dx and the eight parameter gradients):

    |kernel - judge|_max <= 4 x yardstick error + floor

with the yardstick and the floor of lstm_common (fp32: torch.nn.LSTM on the CPU; bf16: the fp32 recursion with bf16-rounded matrix
operands, the judge on the same bf16-rounded inputs).  Every figure is printed before it is asserted (`pytest -s`); with
SAICV_LSTM_RATIOS_OUT=<file> the last test writes the worst error / bound per tensor and dtype under the key `accuracy` of that
JSON file (profiles/ocr_lstm.json holds them beside the timings of scripts/probes/lstm_bench.py)."""
import json
import os

import pytest
import torch

import lstm_common as lc

pytestmark = pytest.mark.gpu

TILE = 16                     # batch rows of a workgroup (csrc/lstm.hip)
RECORD = {'fp32': {}, 'bf16': {}}

# name -> (B, T, I, H, parameter scale, dy kind, input layout)
CASES = {
    'T1_no_recurrence': (2, 1, 32, 32, 1.0, 'dense', 'dense'),
    'T2_one_carry': (2, 2, 32, 32, 1.0, 'dense', 'dense'),
    'T5_B3_partial_tile': (3, 5, 32, 32, 1.0, 'dense', 'dense'),
    'B1': (1, 3, 32, 32, 1.0, 'dense', 'dense'),
    'B_tile_plus_one': (TILE + 1, 2, 32, 32, 1.0, 'dense', 'dense'),
    'H96': (3, 16, 96, 96, 1.0, 'dense', 'dense'),
    'H512_streamed_weights': (2, 3, 512, 512, 1.0, 'dense', 'dense'),
    'H640_eight_slices_per_wave': (1, 2, 64, 640, 1.0, 'dense', 'dense'),     # fp32: dgates read back from global; bf16: one LDS tile
    'I48_H32': (2, 3, 48, 32, 1.0, 'dense', 'dense'),
    'T64_carry_growth': (2, 64, 32, 32, 1.0, 'dense', 'dense'),
    'saturated_x4': (3, 16, 96, 96, 4.0, 'dense', 'dense'),
    'row_strided_input': (3, 5, 32, 32, 1.0, 'dense', 'strided'),
    'dy_first_frame_only': (3, 5, 32, 32, 1.0, 'first_frame', 'dense'),
    'dy_last_frame_only': (3, 5, 32, 32, 1.0, 'last_frame', 'dense'),
    'dy_forward_half_only': (3, 5, 32, 32, 1.0, 'forward_half', 'dense'),
    'dy_reverse_half_only': (3, 5, 32, 32, 1.0, 'reverse_half', 'dense'),
}


def _run(x, w, dy, dtype, layout='dense'):
    """ops.lstm forward + backward on the GPU -> dict(y, dx, <the eight names>) on the CPU"""
    from simpleaicv_pytorch_training_examples_amd import ops
    b, t, i = x.shape
    if layout == 'strided':                       # what linear_frames returns when the out-features were padded
        base = torch.zeros(b * t, i + 8, dtype=dtype, device='cuda')
        base[:, :i] = x.reshape(b * t, i).to(dtype)
        leaf = base.requires_grad_(True)
        xin = leaf.as_strided((b, t, i), (t * (i + 8), i + 8, 1), 0)
        assert not xin.is_contiguous()
    else:
        leaf = x.to(dtype).cuda().requires_grad_(True)
        xin = leaf
    params = {n: v.clone().cuda().requires_grad_(True) for n, v in w.items()}
    y = ops.lstm(xin, params)
    y.backward(dy.to(dtype).cuda())
    torch.cuda.synchronize()
    out = {n: p.grad.detach().cpu() for n, p in params.items()}
    out['y'] = y.detach().cpu()
    out['dx'] = leaf.grad.detach().cpu().view(b, t, -1)[:, :, :i]
    assert out['y'].dtype == dtype and out['dx'].dtype == dtype
    assert all(out[n].dtype == torch.float32 for n in lc.NAMES)
    return out


_yard_cache = {}


def _yard(name, bf16):
    key = (name, bf16)
    if key not in _yard_cache:
        b, t, i, h, scale, dy_kind, _ = CASES[name]
        x, w, dy = lc.make_case(b, t, i, h, seed=len(name), scale=scale, bf16=bf16, dy_kind=dy_kind)
        ref, yard = lc.yardstick(x, w, dy, bf16)
        _yard_cache[key] = (x, w, dy, ref, yard, lc.bounds(ref, yard, bf16))
    return _yard_cache[key]


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('name', list(CASES))
def test_against_the_float64_judge(name, dtype):
    bf16 = dtype == 'bf16'
    x, w, dy, ref, yard, bound = _yard(name, bf16)
    got = _run(x, w, dy, torch.bfloat16 if bf16 else torch.float32, CASES[name][6])
    err = lc.errors(got, ref)
    for k in sorted(err):
        print(f'{name} {dtype} {k}: error {err[k]:.3e} yardstick {yard[k]:.3e} bound {bound[k]:.3e} '
              f'largest {float(ref[k].abs().max()):.3e}')
    for k in err:
        if bound[k] > 0:
            cur = RECORD[dtype].get(k, (0.0, ''))
            RECORD[dtype][k] = max(cur, (err[k] / bound[k], name))
    assert all(torch.isfinite(v).all() for v in got.values())
    bad = {k: (err[k], bound[k]) for k in err if not err[k] <= bound[k]}
    assert not bad, bad


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_two_runs_are_bit_equal(deterministic, dtype):
    x, w, dy = lc.make_case(TILE + 1, 5, 96, 96, seed=5, bf16=dtype == torch.bfloat16)
    a, b = _run(x, w, dy, dtype), _run(x, w, dy, dtype)
    assert set(a) == set(b) == set(lc.NAMES) | {'y', 'dx'}
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_unsupported_shapes_raise_before_any_launch():
    from simpleaicv_pytorch_training_examples_amd import ops, _lib
    torch.cuda.synchronize()

    def reject(x, w):
        with pytest.raises(ValueError):
            ops.lstm(x.cuda(), {n: v.cuda() for n, v in w.items()})

    x, w, _ = lc.make_case(2, 3, 32, 40)                       # H no multiple of 32
    reject(x, w)
    x, w, _ = lc.make_case(2, 3, 36, 32)                       # 36 bf16 are no whole number of 16-byte chunks
    reject(x.bfloat16(), w)
    x, w, _ = lc.make_case(2, 3, 32, 32)
    reject(x.half(), w)
    reject(x.transpose(1, 2).contiguous().transpose(1, 2), w)  # the feature axis is not the dense one
    reject(x, dict(w, weight_hh_l0=w['weight_hh_l0'][:, :16]))
    with pytest.raises(ValueError):
        ops.lstm(x.cuda(), {n: v.cuda() for n, v in w.items()}, bidirectional=False)
    # the C entry point refuses the same without a launch: an error code and a readable message, no fault
    L = _lib.lib()
    assert L.saicv_lstm_fwd(_lib.F32, 0, 0, 0, 0, 2, 3, 40, 0) != 0 and b'hidden size' in L.saicv_last_error_string()
    assert L.saicv_lstm_bwd(_lib.F32, 0, 0, 0, 0, 0, 2, 0, 32, 0) != 0
    torch.cuda.synchronize()


def test_zz_record_the_worst_ratios():
    """last in the module: with SAICV_LSTM_RATIOS_OUT set, the worst error / bound per tensor and dtype of this run go to that file"""
    out = os.environ.get('SAICV_LSTM_RATIOS_OUT')
    worst = {dt: {k: {'error_over_bound': round(v[0], 4), 'case': v[1]} for k, v in sorted(r.items())} for dt, r in RECORD.items()}
    if out and any(worst.values()):
        doc = {}
        if os.path.exists(out):
            with open(out) as f:
                doc = json.load(f)
        doc['accuracy'] = {'bound': '4 x yardstick error + floor (tests/lstm_common.py)', 'worst': worst}
        with open(out, 'w') as f:
            json.dump(doc, f, indent=1)
    assert all(v['error_over_bound'] <= 1 for r in worst.values() for v in r.values())
