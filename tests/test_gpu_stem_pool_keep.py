"""saicv_bn_relu_maxpool_fwd_keep / saicv_bn_relu_maxpool_bwd_sums / saicv_bn_relu_maxpool_bwd_apply (csrc/pool.hip): the pooled
stem's forward also stores the raw y at each recorded maximum (ya), the backward's two per-channel sums come from dout and ya alone
-- no pass over y --, and the second pass of the backward runs from them.

Shapes are those of the convolution output, C = 64, pool (3, 2, 1): (2, 17, 24) and (3, 25, 35) have odd extents (border windows, a
last window of two rows / columns), (4, 32, 32) is even.  Channel NEG is negative everywhere behind the BatchNorm (gate closed at the
maximum), channel TIE ties in every window (stem_bwd_common.py).

Atomics mode: the sums from ya are the same addends as the existing pass's, added by the same atomics in whatever order the
workgroups finish -- either differs from run to run in its last bits.  Both are held against a float64 sum of those addends; the new
sums may be 2 x as far from it as the existing pass's own error on the same inputs, with a floor of one fp32 ulp of the largest sum
of that kind.  An error that changes from run to run is taken as the largest of RUNS launches, for the existing pass and for the
new one alike (a single launch of each met the bound in most runs and missed it by 3 % in one: 2.96e-5 against 2 x 1.43e-5)."""
import pytest
import torch

import stem_bwd_common as S

pytestmark = pytest.mark.gpu

SHAPES = [(2, 17, 24), (3, 25, 35), (4, 32, 32)]
RUNS = 5


def _sums(t, ya):
    _lib, lib, st = S.L()
    ptr = _lib.ptr
    sums = torch.full((2 * S.C,), float('nan'), device='cuda')
    _lib.check(lib.saicv_bn_relu_maxpool_bwd_sums(0, ptr(t['dout']), ptr(ya), ptr(t['mean']), ptr(t['invstd']), ptr(t['scale']),
                                                  ptr(t['shift']), ptr(sums), t['n'], t['ph'], t['pw'], S.C, st), 'sums')
    torch.cuda.synchronize()
    return sums


def _apply(t, idx, sums):
    _lib, lib, st = S.L()
    ptr = _lib.ptr
    n, h, w, ph, pw = t['n'], t['h'], t['w'], t['ph'], t['pw']
    dy = torch.full((n, h, w, S.C), float('nan'), dtype=torch.bfloat16, device='cuda')
    dg, db = torch.full((S.C,), float('nan'), device='cuda'), torch.full((S.C,), float('nan'), device='cuda')
    _lib.check(lib.saicv_bn_relu_maxpool_bwd_apply(0, ptr(t['dout']), ptr(idx), ptr(t['y']), ptr(t['gamma']), ptr(t['mean']), ptr(t['invstd']),
                                                   ptr(t['scale']), ptr(t['shift']), ptr(sums), ptr(dy), ptr(dg), ptr(db), 0, n, h, w, S.C, ph, pw,
                                                   *S.POOL, st), 'apply')
    torch.cuda.synchronize()
    return dy, dg, db


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_keeping_forward(shape):
    t = S.case(*shape)
    n, h, w, ph, pw = t['n'], t['h'], t['w'], t['ph'], t['pw']
    out0, idx0, _ = S.forward(t, keep=False)
    out1, idx1, ya = S.forward(t, keep=True)
    assert torch.equal(out0.view(torch.int16), out1.view(torch.int16)) and torch.equal(idx0, idx1)
    assert int(idx1.max()) <= 8
    # y gathered at the recorded positions: window (oh, ow) starts at (2 oh - 1, 2 ow - 1), position = kh * 3 + kw
    pos = idx1.long()
    oh = torch.arange(ph, device='cuda').view(1, ph, 1, 1)
    ow = torch.arange(pw, device='cuda').view(1, 1, pw, 1)
    ih, iw = 2 * oh - 1 + pos // 3, 2 * ow - 1 + pos % 3
    assert bool(((ih >= 0) & (ih < h) & (iw >= 0) & (iw < w)).all())
    img = torch.arange(n, device='cuda').view(n, 1, 1, 1).expand_as(pos)
    ch = torch.arange(S.C, device='cuda').view(1, 1, 1, S.C).expand_as(pos)
    want = t['y'][img, ih.expand_as(pos), iw.expand_as(pos), ch]
    assert torch.equal(ya.view(torch.int16), want.view(torch.int16))
    # the closed channel: every maximum is the ReLU's zero, kept y is negative behind the BatchNorm
    assert bool((out1[..., S.NEG] == 0).all())
    assert bool((t['scale'][S.NEG] * ya[..., S.NEG].float() + t['shift'][S.NEG] < 0).all())


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_sums_deterministic_bit_equal(shape):
    from simpleaicv_pytorch_training_examples_amd import ops
    t = S.case(*shape)
    prev = ops.set_deterministic(True)
    try:
        _, idx, ya = S.forward(t, keep=True)
        dg, db = torch.empty(S.C, device='cuda'), torch.empty(S.C, device='cuda')
        dy_old, old = S.backward_two_kernels(t, idx, dg, db, 0)
        new = _sums(t, ya)
        again = _sums(t, ya)
        dy_new, dg2, db2 = _apply(t, idx, new)
    finally:
        ops.set_deterministic(prev)
    assert bool(torch.isfinite(new).all())
    assert torch.equal(new.view(torch.int32), old.view(torch.int32))
    assert torch.equal(new.view(torch.int32), again.view(torch.int32))
    assert float(new[S.NEG]) == 0.0 and float(new[S.C + S.NEG]) == 0.0
    # the second pass alone, from these sums: the two-kernel entry's dy, dgamma and dbeta
    assert torch.equal(dy_new.view(torch.int16), dy_old.view(torch.int16))
    assert torch.equal(dg2.view(torch.int32), dg.view(torch.int32)) and torch.equal(db2.view(torch.int32), db.view(torch.int32))


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_sums_atomics_against_float64(shape):
    from simpleaicv_pytorch_training_examples_amd import ops
    t = S.case(*shape)
    prev = ops.set_deterministic(False)
    try:
        _, idx, ya = S.forward(t, keep=True)
        dg, db = torch.empty(S.C, device='cuda'), torch.empty(S.C, device='cuda')
        old = [S.backward_two_kernels(t, idx, dg, db, 0)[1] for _ in range(RUNS)]
        new = [_sums(t, ya) for _ in range(RUNS)]
    finally:
        ops.set_deterministic(prev)
    # float64 sums of the addends the kernels form: g = dout * [fmaf(scale, ya, shift) > 0] in fp32, g * ((ya - mean) * invstd) exact
    yaf, d = ya.float().view(-1, S.C), t['dout'].float().view(-1, S.C)
    gate = (t['scale'].double() * yaf.double() + t['shift'].double()) > 0          # the sign of the fused multiply-add is the exact sum's
    g = torch.where(gate, d, torch.zeros_like(d)).double()
    xhat = ((yaf - t['mean']) * t['invstd']).double()
    ref = torch.cat([g.sum(0), (g * xhat).sum(0)])
    for which, sl in (('sum g', slice(0, S.C)), ('sum g xhat', slice(S.C, 2 * S.C))):
        err_old = max(float((o[sl].double() - ref[sl]).abs().max()) for o in old)
        err_new = max(float((o[sl].double() - ref[sl]).abs().max()) for o in new)
        bound = max(2 * err_old, S.ulp32(ref[sl].abs().max()))
        print(f'{shape} {which}: existing pass {err_old:.3e}  from ya {err_new:.3e}  bound {bound:.3e}')
        assert err_new <= bound, (which, err_new, err_old)
