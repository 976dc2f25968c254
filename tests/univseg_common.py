"""Float64 judges of the universal-segmentation set loss (csrc/univseg.hip, universal_segmentation/segmentation_losses.py) and the
seeded input recipes its tests share.  tests/test_univseg_host.py pins the judges to values recorded from the reference's own
classes (tests/golden/univseg_tiny.pt).

Every judge returns, with a sum, the sum of the magnitudes of its terms.  The GPU kernels add fp32 terms in a fixed order (lane
sums or MFMA accumulators, then a tree); the error of such a sum is bounded by a multiple of sum |term|, and TOL = 1e-5 of that
magnitude is the bound tests/test_gpu_matting_kernels.py holds the same kind of ordered fp32 pixel sum to."""
import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

TOL = 1e-5
EPS32 = 2.0 ** -24

# (B, Q, [T_i], H, W)
KERNEL_CASES = [
    (1, 1, [1], 1, 1),                  # the smallest shape
    (2, 3, [1, 2], 7, 9),               # nothing a multiple of a vector
    (3, 5, [0, 3, 1], 16, 16),          # an image without targets, first
    (3, 5, [2, 0, 1], 16, 16),          # ... and in the middle
    (1, 100, [33], 24, 40),             # Q and T one past a 32-wide tile
    (2, 17, [150, 2], 8, 8),            # T as large as ADE20K allows, the pixel axis shorter than T
    (2, 3, [2, 1], 97, 130),            # at least three pixel chunks with a ragged last one (asserted from the exported chunk)
]
KINDS = ('randn', 'confident', 'saturating')
TARGET_KINDS = ('binary', 'soft')
# the loss cases recorded from the reference: (B, Q, [T_i], H, W, C) with the reference's default weights
LOSS_CASES = [
    (2, 6, [2, 3], 16, 16, 7),
    (3, 8, [0, 4, 1], 12, 20, 5),
    (1, 5, [5], 9, 7, 4),
    (2, 4, [6, 1], 8, 8, 9),            # more targets than queries in one image
]
LOSS_WEIGHTS = dict(mask_cost=5.0, dice_cost=5.0, class_cost=2.0, mask_loss_weight=5.0, dice_loss_weight=5.0, class_loss_weight=2.0,
                    no_object_class_weight=0.1)
MODEL_CFG = dict(image_size=64, query_num=5, num_classes=7, query_block_nums=2)
MODEL_BATCH = 2


def case_id(case):
    return '-'.join(str(v).replace(' ', '') for v in case)


def make_inputs(case, kind='randn', target_kind='binary', seed=0, classes=7):
    """-> mask_preds [B, Q, H, W] fp32, class_preds [B, Q, C], targets (list of [T_i, H, W] fp32), labels (list of int64 [T_i])"""
    B, Q, Ts, H, W = case[:5]
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * B + 104729 * Q + 31 * H + W + 17 * sum(Ts) + len(kind))
    targets, labels = [], []
    for t in Ts:
        if target_kind == 'binary':
            y = (torch.rand(t, H, W, generator=g) < 0.4).float()
        else:
            y = torch.rand(t, H, W, generator=g)
        targets.append(y)
        labels.append(torch.randint(0, classes - 1, (t, ), generator=g))
    x = 4 * torch.randn(B, Q, H, W, generator=g)
    if kind == 'confident':
        # every query follows one target of its image (where it has any) with 1 % of the pixels flipped
        for b, t in enumerate(Ts):
            for q in range(Q):
                if t:
                    y = targets[b][q % t]
                    flip = torch.rand(H, W, generator=g) < 0.01
                    x[b, q] = 25 * (2 * torch.where(flip, 1 - y, y) - 1)
    elif kind == 'saturating':
        flat = x.view(B, Q, -1)
        n = flat.shape[-1]
        flat[:, :, 0] = 80.
        flat[:, :, n // 2] = -80.
        flat[:, :, n - 1] = 80. if n > 1 else flat[:, :, n - 1]
    class_preds = 2 * torch.randn(B, Q, classes, generator=g)
    return x, class_preds, targets, labels


# a case whose assignment the recording finds decided by less than 1e-3 of its total gets another seed here (none is dropped)
LOSS_SEEDS = {}


def loss_inputs(case):
    B, Q, Ts, H, W, C = case
    return make_inputs((B, Q, Ts, H, W), 'randn', 'binary', seed=100 + LOSS_SEEDS.get(case_id(case), 0), classes=C)


def offsets_of(targets):
    off = [0]
    for t in targets:
        off.append(off[-1] + int(t.shape[0]))
    return off


# ---------------------------------------------------------------------------------------------- judges
def soft_terms(x):
    """float64: softplus(-x), softplus(x), sigmoid(x)"""
    x = x.double()
    return torch.nn.functional.softplus(-x), torch.nn.functional.softplus(x), torch.sigmoid(x)


def judge_pair_sums(x, y):
    """x [Q, P] logits, y [T, P] in [0, 1] -> dict name -> (sum, sum of |terms|), float64.  pos, neg, inter [Q, T]; pred_sum [Q];
    target_sum [T].  (Every term is non-negative for y in [0, 1]; the magnitudes are computed all the same.)"""
    spn, spp, sig = soft_terms(x)
    y = y.double()
    out = {}
    out['pos'] = (spn @ y.T, spn.abs() @ y.abs().T)
    out['neg'] = (spp @ (1 - y).T, spp.abs() @ (1 - y).abs().T)
    out['inter'] = (sig @ y.T, sig.abs() @ y.abs().T)
    out['pred_sum'] = (sig.sum(-1), sig.abs().sum(-1))
    out['target_sum'] = (y.sum(-1), y.abs().sum(-1))
    return out


def judge_cost(x, class_pred, y, labels, mask_cost, dice_cost, class_cost, tol=TOL):
    """One image's cost matrix [Q, T] in float64 and, per entry, the bound an implementation lies within whose five pixel sums
    each lie within tol of their term magnitudes: the first-order propagation of those errors through
        mask_cost (P + N) / HW + dice_cost (1 - (2 S + 1) / (D + 1)) - class_cost prob,   D = sum sigmoid + sum y,
    plus the fp32 rounding of the epilogue itself (a dozen operations: 16 half-ulps of the magnitudes of the three terms, the
    dice term counted as 1 + ratio) and of an fp32 softmax (2e-6 relative: exp and the normalising sum)."""
    s = judge_pair_sums(x, y)
    hw = x.shape[1]
    pos, neg, inter = s['pos'], s['neg'], s['inter']
    den = s['pred_sum'][0][:, None] + s['target_sum'][0][None, :] + 1
    ratio = (2 * inter[0] + 1) / den
    prob = class_pred.double().softmax(-1)[:, labels]
    mask_term = mask_cost * (pos[0] + neg[0]) / hw
    cost = mask_term + dice_cost * (1 - ratio) - class_cost * prob
    cost = torch.nan_to_num(cost.clamp(-1e10, 1e10), 0)
    bound = (abs(mask_cost) * tol * (pos[1] + neg[1]) / hw
             + abs(dice_cost) * (2 * tol * inter[1] / den + ratio / den * tol * (s['pred_sum'][1][:, None] + s['target_sum'][1][None, :]))
             + abs(class_cost) * 2e-6 * prob
             + 16 * EPS32 * (mask_term.abs() + abs(dice_cost) * (1 + ratio) + abs(class_cost) * prob))
    return cost, bound


def judge_assignment(cost):
    q, t = linear_sum_assignment(cost.numpy())
    return q, t


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


def judge_matched(x_rows, y_rows, g=None):
    """x_rows, y_rows [M, P] -> stats [M, 4] float64 = (sum bce, sum sigmoid y, sum sigmoid, sum y), their term magnitudes, and with
    g [M, 4] the gradient [M, P] of sum(g * stats) with ITS term magnitudes |g0| (s + y) + s (1 - s)(|g1| y + |g2|)"""
    x, y = x_rows.double(), y_rows.double()
    spn, spp, sig = soft_terms(x)
    # BCEWithLogits as its two non-negative terms: softplus(x) - x y cancels, in float64 too, where x is large and right
    bce = y * spn + (1 - y) * spp
    stats = torch.stack([bce.sum(-1), (sig * y).sum(-1), sig.sum(-1), y.sum(-1)], dim=-1)
    mags = torch.stack([((y * spn).abs() + ((1 - y) * spp).abs()).sum(-1), (sig * y).abs().sum(-1), sig.abs().sum(-1),
                        y.abs().sum(-1)], dim=-1)
    if g is None:
        return stats, mags
    g = g.double()
    g0, g1, g2 = g[:, 0:1], g[:, 1:2], g[:, 2:3]
    grad = g0 * (sig - y) + sig * (1 - sig) * (g1 * y + g2)
    gmag = g0.abs() * (sig + y.abs()) + sig * (1 - sig) * (g1.abs() * y.abs() + g2.abs())
    return stats, mags, grad, gmag


def judge_loss(mask_preds, class_preds, targets, labels, weights=LOSS_WEIGHTS, indices=None):
    """The three losses of UniversalSegmentationLoss in float64 from the judges above (its own assignment unless one is given), with
    leaves for the gradients: -> dict(losses, indices, costs, dmask, dclass)"""
    B, Q = mask_preds.shape[:2]
    hw = mask_preds.shape[2] * mask_preds.shape[3]
    x = mask_preds.detach().double().clone().requires_grad_(True)
    c = class_preds.detach().double().clone().requires_grad_(True)
    costs = [judge_cost(mask_preds[i].flatten(1), class_preds[i], targets[i].flatten(1), labels[i], weights['mask_cost'],
                        weights['dice_cost'], weights['class_cost'])[0] for i in range(B)]
    if indices is None:
        indices = [judge_assignment(cm) for cm in costs]
    xs, ys, cls_t = [], [], torch.full((B, Q), c.shape[-1] - 1, dtype=torch.int64)
    for i, (qi, ti) in enumerate(indices):
        for q, t in zip(qi, ti):
            xs.append(x[i, q].flatten())
            ys.append(targets[i][t].flatten().double())
            cls_t[i, q] = labels[i][t]
    m = len(xs)
    if m:
        xr, yr = torch.stack(xs), torch.stack(ys)
        sig = torch.sigmoid(xr)
        bce = yr * torch.nn.functional.softplus(-xr) + (1 - yr) * torch.nn.functional.softplus(xr)
        mask_loss = bce.sum() / (m * hw)
        dice_loss = (1 - (2 * (sig * yr).sum(-1) + 1) / (sig.sum(-1) + yr.sum(-1) + 1)).mean()
    else:
        mask_loss = dice_loss = torch.tensor(float('nan'), dtype=torch.float64)
    w = torch.ones(c.shape[-1], dtype=torch.float64)
    w[-1] = weights['no_object_class_weight']
    class_loss = torch.nn.functional.cross_entropy(c.reshape(B * Q, -1), cls_t.reshape(-1), weight=w)
    losses = {'mask_loss': weights['mask_loss_weight'] * mask_loss, 'dice_loss': weights['dice_loss_weight'] * dice_loss,
              'class_loss': weights['class_loss_weight'] * class_loss}
    out = dict(losses={k: float(v.detach()) for k, v in losses.items()}, indices=indices, costs=costs, dmask=None, dclass=None)
    if m:
        sum(losses.values()).backward()
        out['dmask'], out['dclass'] = x.grad, c.grad
    return out


def sample_idx(numel, k=16):
    return torch.linspace(0, numel - 1, min(k, numel)).long()


def model_batch(seed=0):
    """the recorded step's inputs: images [2, 3, 64, 64], per image binary masks [T_i, 64, 64] of distinct classes and their labels"""
    g = torch.Generator().manual_seed(4242 + seed)
    s = MODEL_CFG['image_size']
    images = torch.randn(MODEL_BATCH, 3, s, s, generator=g)
    masks, labels = [], []
    for t in (3, 2):
        label_map = torch.randint(0, t, (s // 8, s // 8), generator=g).repeat_interleave(8, 0).repeat_interleave(8, 1)
        masks.append(torch.stack([(label_map == k).float() for k in range(t)]))
        labels.append(torch.randperm(MODEL_CFG['num_classes'] - 1, generator=g)[:t])
    return images, masks, labels
