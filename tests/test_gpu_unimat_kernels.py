"""csrc/unimat.hip against the float64 judges of tests/unimat_common.py: the matcher's pair sums and cost matrix in both memory orders
at every chunk edge, query-tile edge and target pattern, and the head forward and backward in bf16 and fp32.

Bound of the sums: REF_FACTOR x the deviation tests/golden/unimat_tiny.pt records for the reference's own fp32 cost matrices from
float64, relative to each sum's magnitude (all terms are non-negative).  The tests print what they measure."""
import pytest
import torch

import unimat_common as U
from conftest import load_golden

pytestmark = pytest.mark.gpu

PLANES = ('ce_pos', 'ce_neg', 'intersection', 'local_l1', 'fused_l1')


@pytest.fixture(scope='module')
def ops():
    from simpleaicv_pytorch_training_examples_amd import ops
    return ops


@pytest.fixture(scope='module')
def bound():
    fx = load_golden('unimat_tiny')
    dev = max(max(rec['cost_dev']) for rec in fx['loss_cases'].values())
    assert 0 < dev < 1e-5
    return U.REF_FACTOR * dev


def _chunk():
    from simpleaicv_pytorch_training_examples_amd import ops
    return ops.matting_pair_chunk()


def _cases():
    c = 4096                                            # asserted against the exported chunk in test_chunk_is_what_the_cases_assume
    cases = [(Q, [0, 4, 1], P) for P in (63, c - 1, c, c + 1, 2 * c + 5) for Q in (5, )]
    cases += [(Q, [1], c + 1) for Q in (1, 17, 65)]
    cases += [(5, [0], 63), (5, [1], 63), (17, [17], 63), (65, [17], c + 1), (4, [6, 1], 63), (4, [6, 1], c + 1)]
    # the order and shape the model produces: channels-last memory takes 16-byte loads only where Q is a multiple of 4; Q = 100 is
    # four query tiles, the last one partial (q0 = 96), Q = 36 two; P a multiple of 4 and not of the 32-pixel tile
    cases += [(100, [2, 1], c + 4), (36, [9], 68)]
    return cases


CASES = _cases()
_inputs = {}


def _case_inputs(case, seed=0, planted=True):
    """inputs of a case on the CPU with their judged sums: computed once, shared by both memory orders, never changed"""
    key = (case[0], tuple(case[1]), case[2], seed, planted)
    if key not in _inputs:
        Q, Ts, P = case
        gp, lp, fp, cp, trimaps, alphas, labels = U.make_inputs(len(Ts), Q, Ts, 1, P, seed=seed, planted=planted)
        want = [U.judge_pair_sums(gp[i].flatten(2), lp[i, :, 0].flatten(1), fp[i, :, 0].flatten(1), trimaps[i].flatten(1),
                                  alphas[i].flatten(1)) for i in range(len(Ts))]
        _inputs[key] = (gp, lp, fp, cp, trimaps, alphas, labels, want)
    return _inputs[key]


def _run(ops, gp, lp, fp, trimaps, alphas, order):
    off = U.offsets_of(trimaps)
    dev = 'cuda'
    place = (lambda x: U.channels_last(x.to(dev))) if order == 'channels_last' else (lambda x: x.to(dev).contiguous())
    g, l, f = place(gp), place(lp), place(fp)
    if order == 'channels_last' and g.shape[1] > 1:                   # (the stride of a one-element axis is anything)
        assert g.stride(2) == 1 and g.stride(1) == 3 and l.stride(1) == 1
    tri = torch.cat(trimaps).to(dev)
    alp = torch.cat(alphas).to(dev)
    planes, gsum, wsum = ops.matting_pair_sums(g, l, f, tri, alp, off)
    torch.cuda.synchronize()
    return planes.cpu(), gsum.cpu(), wsum.cpu(), off, (g, l, f, tri, alp)


def _worst(got, want):
    """largest |got - want| in units of want (a sum of non-negative terms: its own magnitude); an exact zero must be met exactly"""
    got, want = got.double(), want.double()
    zero = want == 0
    assert bool((got[zero] == 0).all())
    return float(((got - want).abs() / want.clamp_min(1e-300))[~zero].max()) if bool((~zero).any()) else 0.


def test_chunk_is_what_the_cases_assume(ops):
    assert ops.matting_pair_chunk() == 4096


@pytest.mark.parametrize('order', ['contiguous', 'channels_last'])
@pytest.mark.parametrize('case', CASES, ids=U.case_id)
def test_pair_sums_against_judge(ops, bound, case, order):
    gp, lp, fp, cp, trimaps, alphas, labels, want = _case_inputs(case)
    planes, gsum, wsum, off, _ = _run(ops, gp, lp, fp, trimaps, alphas, order)
    worst = 0.
    for i, w in enumerate(want):
        for j, name in enumerate(PLANES):
            worst = max(worst, _worst(planes[j][:, off[i]:off[i + 1]], w[name]))
        worst = max(worst, _worst(gsum[i], w['global_sum']), _worst(wsum[off[i]:off[i + 1]], w['weight_sum']))
    print(f'pair sums {U.case_id(case)} {order}: worst {worst:.3e} of the magnitude, bound {bound:.3e}')
    assert worst <= bound


@pytest.mark.parametrize('order', ['contiguous', 'channels_last'])
def test_cost_against_judge(ops, bound, order):
    case = (5, [0, 4, 1], 4097)
    gp, lp, fp, cp, trimaps, alphas, labels, _ = _case_inputs(case)
    _, _, _, off, (g, l, f, tri, alp) = _run(ops, gp, lp, fp, trimaps, alphas, order)
    weights = dict(U.LOSS_WEIGHTS, global_trimap_ce_cost=2.0, global_trimap_iou_cost=0.5, local_alpha_cost=3.0, fusion_alpha_cost=1.5,
                   class_cost=0.7)
    cost = ops.matting_match_cost(g, l, f, cp.cuda(), tri, alp, off, torch.cat(labels).cuda(), 2.0, 0.5, 3.0, 1.5, 0.7).cpu()
    assert tuple(cost.shape) == (5, 5) and cost.dtype == torch.float32
    for i in range(3):
        want, lim = U.judge_cost(gp[i].flatten(2), lp[i, :, 0].flatten(1), fp[i, :, 0].flatten(1), cp[i], trimaps[i].flatten(1),
                                 alphas[i].flatten(1), labels[i], weights, tol=bound)
        got = cost[:, off[i]:off[i + 1]].double()
        if want.numel():
            print(f'cost image {i} {order}: worst {float(((got - want).abs() / lim).max()):.3f} of its bound')
            assert bool(((got - want).abs() <= lim).all())


@pytest.mark.parametrize('order', ['contiguous', 'channels_last'])
def test_dyadic_inputs_are_bit_exact(ops, order):
    """probabilities and alphas that are multiples of 1/256 in [1/256, 255/256]: I, L, F, G, W are exact in any order of addition"""
    Q, Ts, P = 5, [0, 4, 1], 2 * 4096 + 5
    g = torch.Generator().manual_seed(5)
    dy = lambda *shape: torch.randint(1, 256, shape, generator=g).float() / 256     # noqa: E731
    gp, lp, fp = dy(3, Q, 3, 1, P), dy(3, Q, 1, 1, P), dy(3, Q, 1, 1, P)
    alphas = [dy(t, 1, P) for t in Ts]
    trimaps = [torch.tensor([0., 128., 255.])[torch.randint(0, 3, (t, 1, P), generator=g)] for t in Ts]
    planes, gsum, wsum, off, _ = _run(ops, gp, lp, fp, trimaps, alphas, order)
    for i in range(3):
        w = U.judge_pair_sums(gp[i].flatten(2), lp[i, :, 0].flatten(1), fp[i, :, 0].flatten(1), trimaps[i].flatten(1), alphas[i].flatten(1))
        for j, name in ((2, 'intersection'), (3, 'local_l1'), (4, 'fused_l1')):
            assert torch.equal(planes[j][:, off[i]:off[i + 1]].double(), w[name]), name
        assert torch.equal(gsum[i].double(), w['global_sum']) and torch.equal(wsum[off[i]:off[i + 1]].double(), w['weight_sum'])


@pytest.mark.parametrize('order', ['contiguous', 'channels_last'])
def test_saturated_inputs_hit_the_clamp(ops, bound, order):
    Q, Ts, P = 5, [3], 4097
    g = torch.Generator().manual_seed(6)
    gp = torch.randint(0, 2, (1, Q, 3, 1, P), generator=g).float()
    lp = torch.randint(0, 2, (1, Q, 1, 1, P), generator=g).float()
    fp = torch.randint(0, 2, (1, Q, 1, 1, P), generator=g).float()
    alpha, trimap = U.make_targets(3, 1, P, g)
    planes, gsum, wsum, off, _ = _run(ops, gp, lp, fp, [trimap], [alpha], order)
    w = U.judge_pair_sums(gp[0].flatten(2), lp[0, :, 0].flatten(1), fp[0, :, 0].flatten(1), trimap.flatten(1), alpha.flatten(1))
    worst = max(max(_worst(planes[j], w[name]) for j, name in enumerate(PLANES)), _worst(gsum[0], w['global_sum']))
    print(f'saturated {order}: worst {worst:.3e}, bound {bound:.3e}')
    assert worst <= bound and bool(torch.isfinite(planes).all())


def test_two_calls_give_the_same_bits(ops):
    gp, lp, fp, cp, trimaps, alphas, labels, _ = _case_inputs((17, [17], 63))
    a = _run(ops, gp, lp, fp, trimaps, alphas, 'channels_last')
    b = _run(ops, gp, lp, fp, trimaps, alphas, 'channels_last')
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))


@pytest.mark.parametrize('order', ['contiguous', 'channels_last'])
def test_an_image_alone_or_in_a_batch(ops, order):
    """the bits of an image's cost columns depend on its own (Q, T_i, P): alone (one target group of its size) or next to an image
    with many more targets (another group size)"""
    Q, Ts, P = 5, [2, 9, 0, 1], 4096 + 37
    gp, lp, fp, cp, trimaps, alphas, labels, _ = _case_inputs((Q, Ts, P), seed=3)
    _, _, _, off, (g, l, f, tri, alp) = _run(ops, gp, lp, fp, trimaps, alphas, order)
    lab = torch.cat(labels).cuda()
    batch = ops.matting_match_cost(g, l, f, cp.cuda(), tri, alp, off, lab).cpu()
    for i in range(len(Ts)):
        alone = ops.matting_match_cost(g[i:i + 1], l[i:i + 1], f[i:i + 1], cp[i:i + 1].cuda(), tri[off[i]:off[i + 1]],
                                       alp[off[i]:off[i + 1]], [0, Ts[i]], lab[off[i]:off[i + 1]]).cpu()
        assert torch.equal(alone, batch[:, off[i]:off[i + 1]]), i


# ---------------------------------------------------------------------------------------------- head
# fp32 sigmoid through one exp and one division: a few ulps of a value below 1
HEAD_TOL = 16 * U.EPS32


def _head_inputs(Q, dtype, seed):
    g = torch.Generator().manual_seed(900 + seed + Q)
    B, H, W = 2, 3, 7                                    # 21 pixels per image: no multiple of a vector
    gl = (3 * torch.randn(B, 3 * Q, H, W, generator=g)).to(dtype)
    ll = (3 * torch.randn(B, Q, H, W, generator=g)).to(dtype)
    gl[0, 0:3, 0, 0] = 0.75                              # an exact tie of all three -> class 0
    gl[1, 3 * (Q - 1):3 * Q, 2, 6] = torch.tensor([40., 50., 10.]).to(dtype)     # both probabilities are exactly 1.0f -> class 0
    return gl, ll


@pytest.mark.parametrize('memory', ['channels_last', 'contiguous'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('Q', [1, 5, 100])
def test_head_forward_and_backward(ops, Q, dtype, memory):
    gl, ll = _head_inputs(Q, dtype, 0)
    B, _, H, W = gl.shape
    gen = torch.Generator().manual_seed(77)
    dG, dL, dF = torch.randn(B, Q, 3, H, W, generator=gen), torch.randn(B, Q, 1, H, W, generator=gen), torch.randn(B, Q, 1, H, W, generator=gen)
    want = U.judge_head(gl, ll, dG, dL, dF)
    und = want['undecided']
    planted = torch.zeros_like(und)
    planted[0, 0, 0, 0, 0] = True
    planted[1, Q - 1, 0, 2, 6] = True
    assert not bool(und[planted].any()) and float(und.float().mean()) <= U.UNDECIDED_CAP      # exact ties are decided: class 0
    assert bool((want['argmax'][planted] == 0).all())
    fmt = torch.channels_last if memory == 'channels_last' else torch.contiguous_format
    a = gl.cuda().contiguous(memory_format=fmt).requires_grad_(True)
    b = ll.cuda().contiguous(memory_format=fmt).requires_grad_(True)
    g, l, f = ops.matting_head(a, b)
    assert g.dtype == l.dtype == f.dtype == torch.float32
    assert tuple(g.shape) == (B, Q, 3, H, W) and tuple(l.shape) == tuple(f.shape) == (B, Q, 1, H, W)
    assert g.stride(2) == 1 and g.stride(4) == 3 * Q and f.stride(4) == Q and (Q == 1 or (g.stride(1) == 3 and l.stride(1) == 1))
    eg = float((g.detach().cpu().double() - want['global_preds']).abs().max())
    el = float((l.detach().cpu().double() - want['local_preds']).abs().max())
    ef = float(((f.detach().cpu().double() - want['fused_preds']).abs() * ~und).max())
    print(f'head Q={Q} {dtype} {memory}: global {eg:.2e} local {el:.2e} fused {ef:.2e} (bound {HEAD_TOL:.2e})')
    assert max(eg, el, ef) <= HEAD_TOL
    assert float(f.detach().cpu()[planted].abs().max()) == 0.                       # both planted ties resolve to class 0
    (g * dG.cuda()).sum().add((l * dL.cuda()).sum()).add((f * dF.cuda()).sum()).backward()
    keep3 = ~und.expand(B, Q, 3, H, W).reshape(B, 3 * Q, H, W)
    keep1 = ~und.reshape(B, Q, H, W)
    # a gradient element is incoming x p (1 - p): three fp32 factors, rounded to the logits' dtype (relative part), and p itself
    # lies within HEAD_TOL of float64, which moves p (1 - p) by at most that (absolute part, times the incoming gradient)
    rel = 2.0 ** -8 if dtype == torch.bfloat16 else 32 * U.EPS32
    inc3 = dG.double().abs().reshape(B, 3 * Q, H, W)
    inc1 = (dL.double().abs() + dF.double().abs()).reshape(B, Q, H, W)
    for got, ref, keep, inc in ((a.grad, want['dglobal_logits'], keep3, inc3), (b.grad, want['dlocal_logits'], keep1, inc1)):
        assert got.dtype == dtype and got.shape == ref.shape
        err = ((got.cpu().double() - ref).abs() - rel * ref.abs() - HEAD_TOL * inc) * keep
        assert float(err.max()) <= 0., float(err.max())
    # dF alone: the local gradient is exactly zero wherever the argmax is not class 1, the global one everywhere
    a.grad = b.grad = None
    g, l, f = ops.matting_head(a, b)
    (f * dF.cuda()).sum().backward()
    off1 = ((want['argmax'] != 1) & ~und).reshape(B, Q, H, W)
    assert float(b.grad.cpu().float()[off1].abs().max()) == 0. and float(a.grad.float().abs().max()) == 0.
    assert float(b.grad.float().abs().max()) > 0.
