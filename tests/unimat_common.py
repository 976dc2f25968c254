"""Float64 judges of universal matting (csrc/unimat.hip, universal_segmentation/matting_losses.py, models/dinov3_universal_matting.py)
and the seeded input recipes its tests share.  tests/test_unimat_host.py pins the judges to values recorded from the reference's own
classes (tests/golden/unimat_tiny.pt).  The judges restate, on float64 tensors, the reference's
SimpleAICV/universal_segmentation/matting_losses.py -- the matcher's four pair-wise costs (:106-246: trimap BCE and IoU against the
one-hot class, masked local L1, fused L1) with its epilogue (:85-94), and the seven losses (:385-541: trimap BCE and IoU, the two
sqrt(d^2 + 1e-12) alpha losses, the two five-level Laplacian-pyramid L1 losses, the weighted class cross entropy) -- and the end of
models/dinov3_universal_matting.py's predict (:182-219: two sigmoids, collaborative_matting over torch.max).  Nothing calls the package.

Bound.  The fixture records how far the reference's own fp32 run lies from the same code in float64 (cost matrices: 'cost_dev').
An implementation that adds the same fp32 terms in another order is allowed REF_FACTOR = 4 times that, relative to the magnitude of
each sum (every term of the five pair sums is non-negative, so a sum is its own magnitude)."""
import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

REF_FACTOR = 4.0
EPS32 = 2.0 ** -24
LO32, HI32 = float(np.float32(1e-4)), float(np.float32(1.) - np.float32(1e-4))
UNDECIDED = 1e-5                        # two largest float64 global probabilities closer than this: the pixel's class is not judged
UNDECIDED_CAP = 1e-3                    # at most this share of the pixels may be undecided

# (B, Q, [T_i], H, W) recorded from the reference, with its default weights and num_classes = LOSS_CLASSES
LOSS_CASES = [
    (2, 6, [2, 3], 32, 32),
    (1, 5, [5], 40, 32),
    (2, 4, [6, 1], 32, 32),             # more targets than queries in one image
    (1, 3, [1], 64, 64),
]
LOSS_CLASSES = 3
LOSS_WEIGHTS = dict(global_trimap_ce_cost=1.0, global_trimap_iou_cost=1.0, local_alpha_cost=1.0, fusion_alpha_cost=1.0, class_cost=1.0,
                    global_trimap_ce_loss_weight=1.0, global_trimap_iou_loss_weight=1.0, local_alpha_loss_weight=1.0,
                    local_laplacian_loss_weight=1.0, fusion_alpha_loss_weight=1.0, fusion_laplacian_loss_weight=1.0,
                    class_loss_weight=1.0, no_object_class_weight=0.1)
LOSS_KEYS = ('global_trimap_ce_loss', 'global_trimap_iou_loss', 'local_alpha_loss', 'local_laplacian_loss', 'fusion_alpha_loss',
             'fusion_laplacian_loss', 'class_loss')
# a case whose assignment the recording finds decided by less than 1e-3 of its total gets another seed here (none is dropped)
LOSS_SEEDS = {}
MODEL_CFG = dict(image_size=64, query_num=5, num_classes=2, query_block_nums=2)
MODEL_BATCH = 2
MODEL_SEEDS = dict(build=0, data=10, run=1)


def case_id(case):
    return '-'.join(str(v).replace(' ', '') for v in case)


def offsets_of(targets):
    off = [0]
    for t in targets:
        off.append(off[-1] + int(t.shape[0]))
    return off


# ---------------------------------------------------------------------------------------------- recipes
def make_targets(t, h, w, g):
    """-> alpha [t, h, w] in [0, 1] (multiples of 1/256, flat regions of 0 and 1 around a soft band), trimap in {0, 128, 255}"""
    ch, cw = max(1, (h + 3) // 4), max(1, (w + 3) // 4)
    coarse = torch.rand(t, ch, cw, generator=g).repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :h, :w]
    alpha = torch.round(((coarse - 0.3) / 0.4).clamp(0, 1) * 256) / 256
    trimap = torch.where(alpha == 0, 0., torch.where(alpha == 1, 255., 128.))
    return alpha.contiguous(), trimap.contiguous()


def fuse(global_preds, local_preds):
    """collaborative_matting on [..., 3, H, W] / [..., 1, H, W]: the first maximum of the three probabilities"""
    idx = torch.max(global_preds, dim=-3, keepdim=True)[1]
    return local_preds * (idx == 1) + (idx == 2).to(local_preds.dtype)


def make_preds(B, Q, trimaps, alphas, H, W, g, planted=True):
    """-> global [B, Q, 3, H, W], local [B, Q, 1, H, W], fused [B, Q, 1, H, W] fp32 probabilities.  planted: a random permutation gives
    min(Q, T_i) queries a noisy copy of a target -- global softmax(3 onehot + randn), local clamp(alpha + 0.1 randn); the other
    queries are random; fused is recomputed from the two."""
    gp = torch.softmax(torch.randn(B, Q, 3, H, W, generator=g), dim=2)
    lp = torch.rand(B, Q, 1, H, W, generator=g)
    if planted:
        for b in range(B):
            t = trimaps[b].shape[0]
            perm = torch.randperm(Q, generator=g)[:min(Q, t)]
            for j, q in enumerate(perm.tolist()):
                k = judge_class(trimaps[b][j])
                onehot = torch.nn.functional.one_hot(k, 3).permute(2, 0, 1).float()
                gp[b, q] = torch.softmax(3 * onehot + torch.randn(3, H, W, generator=g), dim=0)
                lp[b, q, 0] = (alphas[b][j] + 0.1 * torch.randn(H, W, generator=g)).clamp(0, 1)
    return gp, lp, fuse(gp, lp)


def make_inputs(B, Q, Ts, H, W, seed=0, classes=LOSS_CLASSES, planted=True):
    """-> global_preds, local_preds, fused_preds, class_preds [B, Q, C], trimaps, alphas (lists of [T_i, H, W]), labels (list)"""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * B + 104729 * Q + 31 * H + W + 17 * sum(Ts) + len(Ts))
    alphas, trimaps, labels = [], [], []
    for t in Ts:
        a, tri = make_targets(t, H, W, g)
        alphas.append(a)
        trimaps.append(tri)
        labels.append(torch.randint(0, classes - 1, (t, ), generator=g))
    gp, lp, fp = make_preds(B, Q, trimaps, alphas, H, W, g, planted)
    class_preds = 2 * torch.randn(B, Q, classes, generator=g)
    return gp, lp, fp, class_preds, trimaps, alphas, labels


def loss_inputs(case):
    B, Q, Ts, H, W = case
    return make_inputs(B, Q, Ts, H, W, seed=100 + LOSS_SEEDS.get(case_id(case), 0))


def channels_last(x):
    """[B, Q, C, H, W] -> the same values as a view of [B, H, W, Q * C] memory (channel q * C + c): the order the model's head writes"""
    B, Q, C, H, W = x.shape
    return x.permute(0, 3, 4, 1, 2).contiguous().view(B, H, W, Q, C).permute(0, 3, 4, 1, 2)


# ---------------------------------------------------------------------------------------------- judges
def judge_class(trimap):
    """255 -> 2, else anything > 2 -> 1, else the integer part"""
    k = torch.where(trimap == 255, torch.full_like(trimap, 2), torch.where(trimap > 2, torch.ones_like(trimap), trimap.trunc()))
    return k.long()


def clamp32(x):
    """the clamp to [float32(1e-4), float32(1 - 1e-4)] of an fp32 tensor, as float64"""
    return x.double().clamp(LO32, HI32)


def judge_pair_sums(g, l, f, trimap, alpha):
    """One image: g [Q, 3, P], l, f [Q, P], trimap, alpha [T, P] -> float64 dict: ce_pos, ce_neg, intersection, local_l1, fused_l1
    [Q, T]; global_sum [Q]; weight_sum [T].  Every term is non-negative: a sum is its own magnitude."""
    gc, lc, fc = clamp32(g), clamp32(l), clamp32(f)
    onehot = torch.nn.functional.one_hot(judge_class(trimap), 3).double()                      # [T, P, 3]
    nl, nm = -torch.log(gc), -torch.log1p(-gc)                                                   # [Q, 3, P]
    w = (trimap == 128).double()
    a = alpha.double()
    out = {'ce_pos': torch.einsum('qcp,tpc->qt', nl, onehot), 'ce_neg': torch.einsum('qcp,tpc->qt', nm, 1 - onehot),
           'intersection': torch.einsum('qcp,tpc->qt', gc, onehot),
           'local_l1': ((lc[:, None, :] - a[None]).abs() * w[None]).sum(-1), 'fused_l1': (fc[:, None, :] - a[None]).abs().sum(-1),
           'global_sum': gc.sum(dim=(1, 2)), 'weight_sum': w.sum(-1)}
    return out


def judge_cost(g, l, f, class_pred, trimap, alpha, labels, weights=LOSS_WEIGHTS, tol=0.):
    """One image's cost matrix [Q, T] in float64 and, per entry, the bound of an implementation whose pair sums each lie within `tol`
    of their magnitudes: first-order propagation through
        ce (Cpos + Cneg) / (3 P) + iou (1 - (I + 1e-4) / (G + P - I + 1e-4)) + local L / (W + 1) + fusion F / P - class prob
    (the ratio of two sums that are each within tol is within 2 tol), plus the fp32 rounding of the epilogue's dozen operations
    (16 half-ulps of the magnitudes of the five terms) and of an fp32 softmax (2e-6 relative)."""
    s = judge_pair_sums(g, l, f, trimap, alpha)
    P = g.shape[-1]
    ce = (s['ce_pos'] + s['ce_neg']) / (3 * P)
    ratio = (s['intersection'] + 1e-4) / (s['global_sum'][:, None] + P - s['intersection'] + 1e-4)
    local = s['local_l1'] / (s['weight_sum'][None, :] + 1)
    fusion = s['fused_l1'] / P
    prob = class_pred.double().softmax(-1)[:, labels]
    wc, wi, wl, wf, wk = (abs(weights[k]) for k in ('global_trimap_ce_cost', 'global_trimap_iou_cost', 'local_alpha_cost',
                                                    'fusion_alpha_cost', 'class_cost'))
    cost = (weights['global_trimap_ce_cost'] * ce + weights['global_trimap_iou_cost'] * (1 - ratio) + weights['local_alpha_cost'] * local
            + weights['fusion_alpha_cost'] * fusion - weights['class_cost'] * prob)
    cost = torch.nan_to_num(cost.clamp(-1e10, 1e10), 0)
    mag = wc * ce + wi * (1 + ratio) + wl * local + wf * fusion + wk * prob
    bound = tol * (wc * ce + 2 * wi * ratio + wl * local + wf * fusion) + wk * 2e-6 * prob + 16 * EPS32 * mag
    return cost, bound


def assignment_margin(cost):
    """how far the optimal assignment's total lies below the best assignment that differs from it, relative to its magnitude
    (inf when no other assignment exists): each matched pair is forbidden in turn and the problem solved again"""
    cost = cost.double().numpy()
    q, t = linear_sum_assignment(cost)
    best = cost[q, t].sum()
    other = np.inf
    for qi, ti in zip(q, t):
        c = cost.copy()
        c[qi, ti] = 1e18
        q2, t2 = linear_sum_assignment(c)
        v = c[q2, t2].sum()
        if v < 1e17:
            other = min(other, v)
    return (other - best) / max(abs(best), 1e-30)


def gauss_table64():
    """build_gauss_kernel(size=5, sigma=1.0): the SUM of the two axis Gaussians over the grid, normalised, as the reference's numpy
    code leaves it in float32"""
    grid = np.float32(np.mgrid[0:5, 0:5].T)
    kernel = np.sum(np.exp(-((grid - 2) ** 2) / 2.), axis=2)
    kernel /= np.sum(kernel)
    return torch.from_numpy(np.float32(kernel)).double()


def judge_laplacian(pred, alpha, weight=None):
    """pred [M, 1, H, W] clamped probabilities, alpha [M, H, W], float64 -> the sum over the six pyramid entries of the mean absolute
    difference of the two pyramids (both maps times `weight` first)"""
    F = torch.nn.functional
    kernel = gauss_table64()[None, None]
    a, p = alpha[:, None], pred
    if weight is not None:
        a, p = a * weight[:, None], p * weight[:, None]

    def pyramid(cur):
        out = []
        for _ in range(5):
            filtered = F.conv2d(F.pad(cur, (2, 2, 2, 2), mode='replicate'), kernel)
            out.append(cur - filtered)
            cur = F.avg_pool2d(filtered, 2)
        return out + [cur]

    return sum((x - y).abs().mean() for x, y in zip(pyramid(a), pyramid(p)))


# An L1 loss has the gradient sign(d), which no precision decides where d is zero up to rounding.  The reference's form (two
# pyramids, then their difference) leaves such d: an fp32 pyramid entry carries up to 27 roundings per level (25 filter taps, the
# difference, the pooling) of values of magnitude <= 1, over 5 levels and 2 pyramids.
LAP_DELTA = 2 * 5 * 27 * EPS32


def laplacian_flip_slack(pred, alpha, weight=None, delta=LAP_DELTA):
    """How far, element by element, the gradient of judge_laplacian with respect to pred can move when every pyramid difference
    smaller than delta takes the other sign: each such entry changes dL/d(entry) by at most 2 / (entries of its level), carried back
    to pred through the pyramid with |I - G| replaced by I + G (every weight non-negative).  float64 [M, 1, H, W]; zero where no
    undecided entry reaches."""
    F = torch.nn.functional
    kernel = gauss_table64()[None, None]
    w = 1. if weight is None else weight[:, None]

    def pyramid(cur, sign):
        out = []
        for _ in range(5):
            filtered = F.conv2d(F.pad(cur, (2, 2, 2, 2), mode='replicate'), kernel)
            out.append(cur + sign * filtered)
            cur = F.avg_pool2d(filtered, 2)
        return out + [cur]

    p = pred.detach().clone().requires_grad_(True)
    diffs = [x - y for x, y in zip(pyramid(alpha[:, None] * w, -1.), pyramid(pred.detach() * w, -1.))]
    total = sum((2. / d.numel()) * (e * (d.abs() < delta)).sum() for e, d in zip(pyramid(p * w, 1.), diffs))
    total.backward()
    return p.grad


def judge_loss(gp, lp, fp, class_preds, trimaps, alphas, labels, weights=LOSS_WEIGHTS, indices=None):
    """The seven losses of UniversalMattingLoss in float64 from the formulas (its own assignment unless one is given), with leaves
    for the gradients: -> dict(losses, indices, costs, dglobal, dlocal, dfused, dclass)"""
    B, Q = gp.shape[:2]
    H, W = gp.shape[3], gp.shape[4]
    costs = [judge_cost(gp[i].flatten(2), lp[i, :, 0].flatten(1), fp[i, :, 0].flatten(1), class_preds[i], trimaps[i].flatten(1),
                        alphas[i].flatten(1), labels[i], weights)[0] for i in range(B)]
    if indices is None:
        indices = [linear_sum_assignment(c.numpy()) for c in costs]
    leaves = [t.detach().double().clone().requires_grad_(True) for t in (gp, lp, fp, class_preds)]
    g, l, f, c = leaves
    rows, tri, alp = [], [], []
    cls_t = torch.full((B, Q), c.shape[-1] - 1, dtype=torch.int64)
    for i, (qi, ti) in enumerate(indices):
        for q, t in zip(qi, ti):
            rows.append((i, int(q)))
            tri.append(trimaps[i][t].double())
            alp.append(alphas[i][t].double())
            cls_t[i, q] = labels[i][t]
    m = len(rows)
    nan = torch.tensor(float('nan'), dtype=torch.float64)
    if m:
        pb, pq = torch.tensor([r[0] for r in rows]), torch.tensor([r[1] for r in rows])
        tri, alp = torch.stack(tri), torch.stack(alp)
        mg, ml, mf = (t[pb, pq].clamp(LO32, HI32) for t in (g, l, f))                           # [M, 3 | 1, H, W]
        onehot = torch.nn.functional.one_hot(judge_class(tri), 3).double().permute(0, 3, 1, 2)  # [M, 3, H, W]
        ce = (-(onehot * torch.log(mg) + (1 - onehot) * torch.log1p(-mg))).mean()
        inter = (mg * onehot).sum(1)
        iou = (1 - (inter + 1e-4) / (mg.sum(1) + 1 - inter + 1e-4)).mean()
        w = (tri == 128).double()
        local_alpha = torch.sqrt(((ml[:, 0] - alp) * w) ** 2 + 1e-12).sum() / (w.sum() + 1)
        fusion_alpha = torch.sqrt((mf[:, 0] - alp) ** 2 + 1e-12).sum() / alp.numel()
        terms = [ce, iou, local_alpha, judge_laplacian(ml, alp, w), fusion_alpha, judge_laplacian(mf, alp)]
    else:
        terms = [nan] * 6
    cw = torch.ones(c.shape[-1], dtype=torch.float64)
    cw[-1] = weights['no_object_class_weight']
    terms.append(torch.nn.functional.cross_entropy(c.reshape(B * Q, -1), cls_t.reshape(-1), weight=cw))
    losses = {k: weights[k + '_weight'] * v for k, v in zip(LOSS_KEYS, terms)}
    out = dict(losses={k: float(v.detach()) for k, v in losses.items()}, indices=indices, costs=costs, dglobal=None, dlocal=None,
               dfused=None, dclass=None)
    if m:
        sum(losses.values()).backward()
        out['dglobal'], out['dlocal'], out['dfused'], out['dclass'] = (t.grad for t in leaves)
        # what an implementation of the reference's two-pyramid form may differ by (laplacian_flip_slack), on the leaves' shapes
        # (an element outside the clamp has the gradient zero whatever the signs are)
        for name, leaf, rows, wgt, key in (('slack_local', l, ml, w, 'local_laplacian_loss_weight'),
                                           ('slack_fused', f, mf, None, 'fusion_laplacian_loss_weight')):
            inside = ((leaf.detach()[pb, pq] >= LO32) & (leaf.detach()[pb, pq] <= HI32)).double()
            slack = torch.zeros(l.shape, dtype=torch.float64)
            slack[pb, pq] = abs(weights[key]) * laplacian_flip_slack(rows.detach(), alp, wgt) * inside
            out[name] = slack
    return out


def judge_head(global_logits, local_logits, dG=None, dL=None, dF=None):
    """global_logits [B, 3Q, H, W] (channel 3 q + c), local_logits [B, Q, H, W] -> float64 global_preds [B, Q, 3, H, W], local_preds,
    fused_preds [B, Q, 1, H, W], undecided [B, Q, 1, H, W] (the two largest probabilities differ, by less than UNDECIDED), and with the three
    incoming gradients the two logit gradients"""
    B, C3, H, W = global_logits.shape
    Q = C3 // 3
    g = torch.sigmoid(global_logits.double()).view(B, Q, 3, H, W)
    l = torch.sigmoid(local_logits.double()).view(B, Q, 1, H, W)
    idx = torch.max(g, dim=2, keepdim=True)[1]
    f = l * (idx == 1) + (idx == 2).double()
    top = torch.topk(g, 2, dim=2)[0]
    # an exact tie is decided: equal logits, or two that saturate to 1.0 in float64 and so in fp32, give equal probabilities in
    # both precisions, and both take the first maximum
    gap = top[:, :, 0:1] - top[:, :, 1:2]
    undecided = (gap > 0) & (gap < UNDECIDED)
    out = dict(global_preds=g, local_preds=l, fused_preds=f, undecided=undecided, argmax=idx)
    if dG is not None:
        out['dglobal_logits'] = (dG.double() * g * (1 - g)).reshape(B, C3, H, W)
        out['dlocal_logits'] = ((dL.double() + dF.double() * (idx == 1)) * l * (1 - l)).reshape(B, Q, H, W)
    return out


def sample_idx(numel, k=16):
    return torch.linspace(0, numel - 1, min(k, numel)).long()


def model_batch():
    """the recorded step's inputs under manual_seed(MODEL_SEEDS['data']): images [2, 3, 64, 64], per image alphas and trimaps
    [T_i, 64, 64] and labels"""
    g = torch.Generator().manual_seed(MODEL_SEEDS['data'])
    s = MODEL_CFG['image_size']
    images = torch.randn(MODEL_BATCH, 3, s, s, generator=g)
    alphas, trimaps, labels = [], [], []
    for t in (2, 1):
        a, tri = make_targets(t, s, s, g)
        alphas.append(a)
        trimaps.append(tri)
        labels.append(torch.zeros(t, dtype=torch.int64))
    return images, trimaps, alphas, labels
