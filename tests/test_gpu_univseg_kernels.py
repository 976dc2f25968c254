"""csrc/univseg.hip against the float64 judges of tests/univseg_common.py: the pair sums of the matcher, the cost matrix and the
assignment it gives, the matched-pair statistics and their backward (unmatched rows exactly zero in a poisoned buffer), bit
repeatability, and UniversalSegmentationLoss by its fused route against the judge and the composed route."""
import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import univseg_common as U

pytestmark = pytest.mark.gpu

DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16}
SENTINEL = 12345.0


def _ops():
    from simpleaicv_pytorch_training_examples_amd import ops
    return ops


def _loss_cls():
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.universal_segmentation.segmentation_losses import \
        UniversalSegmentationLoss
    return UniversalSegmentationLoss


def _device_inputs(case, kind, target_kind, dtype, seed=0):
    x, cp, targets, labels = U.make_inputs(case, kind, target_kind, seed=seed)
    xd = x.cuda().to(dtype)
    seen = xd.float().cpu()                       # what the kernels read: the judge reads the rounded values too
    packed = torch.cat(targets) if sum(case[2]) else torch.zeros((0, case[3], case[4]))
    return xd, seen, cp, targets, labels, packed


def _within(got, want, mag, tol, what):
    got, want, mag = got.detach().double().cpu(), want.double(), mag.double()
    err = (got - want).abs()
    worst = float((err / mag.clamp_min(1e-300)).max()) if err.numel() else 0.
    print(f'{what}: worst error / term magnitude {worst:.3e} (bound {tol:.1e})')
    assert bool((err <= tol * mag).all()), (what, worst)


def test_chunk_case_spans_three_chunks():
    chunk = _ops().mask_pair_chunk()
    hw = U.KERNEL_CASES[-1][3] * U.KERNEL_CASES[-1][4]
    assert hw >= 2 * chunk + 1 and hw % chunk != 0, (hw, chunk)
    assert all(c[3] * c[4] < chunk for c in U.KERNEL_CASES[:-1])


@pytest.mark.parametrize('dtype', list(DTYPES), ids=list(DTYPES))
@pytest.mark.parametrize('kind', U.KINDS)
@pytest.mark.parametrize('case', U.KERNEL_CASES, ids=U.case_id)
def test_pair_sums_cost_and_assignment(case, kind, dtype):
    ops = _ops()
    B, Q, Ts, H, W = case
    w = U.LOSS_WEIGHTS
    for target_kind in U.TARGET_KINDS:
        xd, seen, cp, targets, labels, packed = _device_inputs(case, kind, target_kind, DTYPES[dtype])
        off = U.offsets_of(targets)
        pos, neg, inter, pred_sum, target_sum = ops.mask_pair_sums(xd, packed.cuda(), off)
        cost = ops.mask_match_cost(xd, cp.cuda(), packed.cuda(), off, torch.cat(labels), w['mask_cost'], w['dice_cost'],
                                   w['class_cost']).cpu()
        assert tuple(cost.shape) == (Q, off[-1])
        for i in range(B):
            cols = slice(off[i], off[i + 1])
            j = U.judge_pair_sums(seen[i].flatten(1), targets[i].flatten(1))
            tag = f'{U.case_id(case)} {kind} {target_kind} {dtype} image {i}'
            _within(pos[:, cols], *j['pos'], U.TOL, tag + ' pos')
            _within(neg[:, cols], *j['neg'], U.TOL, tag + ' neg')
            _within(inter[:, cols], *j['inter'], U.TOL, tag + ' inter')
            _within(pred_sum[i], *j['pred_sum'], U.TOL, tag + ' pred_sum')
            _within(target_sum[cols], *j['target_sum'], U.TOL, tag + ' target_sum')
            if target_kind == 'binary':
                assert torch.equal(target_sum[cols].cpu().double(), j['target_sum'][0])
            want, bound = U.judge_cost(seen[i].flatten(1), cp[i], targets[i].flatten(1), labels[i], w['mask_cost'], w['dice_cost'],
                                       w['class_cost'])
            err = (cost[:, cols].double() - want).abs()
            print(tag, 'cost: worst error / bound', float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.)
            assert bool((err <= bound).all())
            if Ts[i] == 0:
                continue
            qg, tg = linear_sum_assignment(cost[:, cols].numpy())
            qj, tj = U.judge_assignment(want)
            slack = 2 * float(bound.sum())
            margin = U.assignment_margin(want) * abs(float(want[qj, tj].sum()))
            if margin > slack:            # decided beyond what the bound lets the costs move: the assignment is the judge's
                assert np.array_equal(qg, qj) and np.array_equal(tg, tj), tag
            else:                         # a near tie: any assignment within the bound of the optimum is a right answer
                assert float(want[qg, tg].sum()) <= float(want[qj, tj].sum()) + slack, tag


def _pairs(case, targets, seed=0):
    """a pair list as a matcher would give it: per image min(Q, T_i) distinct queries against distinct targets (packed rows)"""
    B, Q, Ts = case[:3]
    rng = np.random.default_rng(seed)
    pb, pq, pt = [], [], []
    off = U.offsets_of(targets)
    for i, t in enumerate(Ts):
        n = min(Q, t)
        pb += [i] * n
        pq += sorted(rng.permutation(Q)[:n].tolist())
        pt += (off[i] + rng.permutation(t)[:n]).tolist()
    return torch.tensor(pb), torch.tensor(pq), torch.tensor(pt)


@pytest.mark.parametrize('dtype', list(DTYPES), ids=list(DTYPES))
@pytest.mark.parametrize('kind', U.KINDS)
@pytest.mark.parametrize('case', U.KERNEL_CASES, ids=U.case_id)
def test_matched_stats_forward_and_backward(case, kind, dtype):
    ops = _ops()
    B, Q, Ts, H, W = case
    for target_kind in U.TARGET_KINDS:
        xd, seen, cp, targets, labels, packed = _device_inputs(case, kind, target_kind, DTYPES[dtype])
        pb, pq, pt = _pairs(case, targets)
        m = pb.numel()
        g = torch.Generator().manual_seed(5)
        gs = torch.randn(m, 4, generator=g)
        leaf = xd.clone().requires_grad_(True)
        stats = ops.matched_mask_stats(leaf, packed.cuda(), pb, pq, pt)
        assert tuple(stats.shape) == (m, 4) and stats.dtype == torch.float32
        # the gradient buffer comes out of the caching allocator: give it the block a sentinel-filled tensor just left
        poison = torch.full_like(xd, SENTINEL)
        torch.cuda.synchronize()
        del poison
        stats.backward(gs.cuda())
        grad = leaf.grad
        assert grad.dtype == xd.dtype and grad.shape == xd.shape
        xr = seen.flatten(2)[pb, pq]
        yr = packed.flatten(1)[pt]
        want, mags, gwant, gmag = U.judge_matched(xr, yr, gs)
        tag = f'{U.case_id(case)} {kind} {target_kind} {dtype}'
        _within(stats, want, mags, U.TOL, tag + ' stats')
        if target_kind == 'binary':
            assert torch.equal(stats[:, 3].cpu().double(), want[:, 3])
        got = grad.float().cpu().flatten(2)
        matched = torch.zeros(B, Q, dtype=torch.bool)
        matched[pb, pq] = True
        assert bool((got[~matched] == 0).all()), tag + ': an unmatched row is not exactly zero'
        bound = U.TOL * gmag + (2.0 ** -8 * gwant.abs() if dtype == 'bf16' else 0.)
        err = (got[pb, pq].double() - gwant).abs()
        print(tag, 'gradient: worst error / bound', float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.)
        assert bool((err <= bound).all())


@pytest.mark.parametrize('dtype', list(DTYPES), ids=list(DTYPES))
@pytest.mark.parametrize('case', [U.KERNEL_CASES[2], U.KERNEL_CASES[5], U.KERNEL_CASES[6]], ids=U.case_id)
def test_repeatable_and_independent_of_batch_order(case, dtype):
    ops = _ops()
    B, Q, Ts, H, W = case
    xd, seen, cp, targets, labels, packed = _device_inputs(case, 'randn', 'soft', DTYPES[dtype])
    off = U.offsets_of(targets)
    pb, pq, pt = _pairs(case, targets)
    gs = torch.randn(pb.numel(), 4, generator=torch.Generator().manual_seed(5)).cuda()

    def run(x, pk, off_, pb_, pq_, pt_, g_):
        sums = [t.clone() for t in ops.mask_pair_sums(x, pk, off_)]
        leaf = x.clone().requires_grad_(True)
        stats = ops.matched_mask_stats(leaf, pk, pb_, pq_, pt_)
        stats.backward(g_)
        return sums, stats.detach().clone(), leaf.grad.clone()

    a = run(xd, packed.cuda(), off, pb, pq, pt, gs)
    b = run(xd, packed.cuda(), off, pb, pq, pt, gs)
    for s, t in zip(a[0], b[0]):
        assert torch.equal(s, t)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    # the images in reverse order: every image's sums, statistics and gradients keep their bits
    perm = list(range(B))[::-1]
    targets_p = [targets[i] for i in perm]
    off_p = U.offsets_of(targets_p)
    packed_p = torch.cat(targets_p) if sum(Ts) else packed
    new_of = {old: new for new, old in enumerate(perm)}
    order = sorted(range(pb.numel()), key=lambda k: (new_of[int(pb[k])], int(pq[k])))
    pb_p = torch.tensor([new_of[int(pb[k])] for k in order], dtype=torch.int64)
    pq_p = torch.tensor([int(pq[k]) for k in order], dtype=torch.int64)
    pt_p = torch.tensor([int(pt[k]) - off[int(pb[k])] + off_p[new_of[int(pb[k])]] for k in order], dtype=torch.int64)
    c = run(xd[perm].contiguous(), packed_p.cuda(), off_p, pb_p, pq_p, pt_p, gs[order])
    for i in range(B):
        n = new_of[i]
        old, new = slice(off[i], off[i + 1]), slice(off_p[n], off_p[n + 1])
        for k in range(3):
            assert torch.equal(a[0][k][:, old], c[0][k][:, new])
        assert torch.equal(a[0][3][i], c[0][3][n]) and torch.equal(a[0][4][old], c[0][4][new])
        assert torch.equal(a[2][i], c[2][n])
    assert torch.equal(a[1][order], c[1])


@pytest.mark.parametrize('dtype', list(DTYPES), ids=list(DTYPES))
@pytest.mark.parametrize('case', U.LOSS_CASES, ids=U.case_id)
def test_loss_fused_against_judge_and_composed(case, dtype):
    x, cp, targets, labels = U.loss_inputs(case)
    C = case[5]
    xd = x.cuda().to(DTYPES[dtype])
    seen = xd.float().cpu()
    judge = U.judge_loss(seen, cp, targets, labels)
    Loss = _loss_cls()
    results = {}
    for route in ('fused', 'composed'):
        crit = Loss(num_classes=C, **U.LOSS_WEIGHTS).cuda()
        crit.route = route
        leaf = xd.clone().requires_grad_(True)
        cleaf = cp.cuda().requires_grad_(True)
        out = crit(leaf, cleaf, [t.cuda() for t in targets], [l.cuda() for l in labels])
        sum(out.values()).backward()
        results[route] = (out, crit.last_indices, leaf.grad, cleaf.grad)
    out, indices, dmask, dclass = results['fused']
    for (qf, tf), (qc, tc), (qj, tj) in zip(indices, results['composed'][1], judge['indices']):
        assert np.array_equal(qf, qc) and np.array_equal(tf, tc)
        assert np.array_equal(qf, qj) and np.array_equal(tf, tj)
    for k, want in judge['losses'].items():
        rel = abs(float(out[k].detach()) - want) / abs(want)
        print(U.case_id(case), dtype, k, 'fused', float(out[k].detach()), 'judge', want, 'relative', rel)
        assert rel <= 1e-5
    # d mask_preds: the kernel's own bound (TOL of the term magnitudes) plus the coefficients' -- each is a ratio of sums that are
    # within TOL of their magnitudes, 2 TOL relative -- so 3 TOL of the magnitudes with the judge's coefficients, and the bf16
    # rounding of the stored value.  d class_preds comes from fp32 torch ops: 1e-5 of the largest element.
    assert dmask.dtype == xd.dtype
    B, Q = case[0], case[1]
    hw = case[3] * case[4]
    m = sum(len(qi) for qi, _ in judge['indices'])
    w = U.LOSS_WEIGHTS
    got = dmask.float().cpu().double()
    matched = torch.zeros(B, Q, dtype=torch.bool)
    for i, (qi, ti) in enumerate(judge['indices']):
        for q, t in zip(qi, ti):
            matched[i, q] = True
            xr, yr = seen[i, q].flatten()[None], targets[i][t].flatten()[None]
            st, _ = U.judge_matched(xr, yr)
            den = st[0, 2] + st[0, 3] + 1
            g = torch.tensor([[w['mask_loss_weight'] / (m * hw), -w['dice_loss_weight'] * 2 / den / m,
                               w['dice_loss_weight'] * (2 * st[0, 1] + 1) / den ** 2 / m, 0.]], dtype=torch.float64)
            _, _, gwant, gmag = U.judge_matched(xr, yr, g)
            assert float((gwant[0] - judge['dmask'][i, q].flatten()).abs().max()) <= 1e-12 * float(gmag.max())
            bound = 3 * U.TOL * gmag[0] + (2.0 ** -8 * gwant[0].abs() if dtype == 'bf16' else 0.)
            assert bool(((got[i, q].flatten() - gwant[0]).abs() <= bound).all()), (i, q)
    assert bool((got[~matched] == 0).all())
    assert float((dclass.cpu().double() - judge['dclass']).abs().max()) <= 1e-5 * float(judge['dclass'].abs().max())


def test_no_matched_pair_gives_nan_mask_terms():
    Loss = _loss_cls()
    crit = Loss(num_classes=7, **U.LOSS_WEIGHTS).cuda()
    x = torch.randn(2, 4, 8, 8, device='cuda', requires_grad=True)
    cp = torch.randn(2, 4, 7, device='cuda', requires_grad=True)
    empty = [torch.zeros(0, 8, 8), torch.zeros(0, 8, 8)]
    for route in ('fused', 'composed'):
        crit.route = route
        out = crit(x, cp, empty, [torch.zeros(0, dtype=torch.int64)] * 2)
        assert torch.isnan(out['mask_loss']) and torch.isnan(out['dice_loss']) and torch.isfinite(out['class_loss'])


def test_duplicate_prediction_row_is_refused():
    ops = _ops()
    x = torch.randn(2, 3, 8, 8, device='cuda')
    y = torch.rand(4, 8, 8, device='cuda')
    with pytest.raises(RuntimeError):
        ops.matched_mask_stats(x, y, torch.tensor([0, 1, 1]), torch.tensor([2, 1, 1]), torch.tensor([0, 2, 3]))
