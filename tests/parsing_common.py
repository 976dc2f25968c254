"""Float64 judges of the parsing loss kernel (csrc/parsing.hip, ops.pixel_class_terms), in plain torch on the CPU, and the input
recipe of its tests.  tests/test_parsing_host.py checks the judge against torch autograd of the restated reference formulas and
against values recorded from the reference's own losses (tests/golden/pfan_parse_r18_tiny.pt)."""
import math

import torch

LO = 1e-4
HI = 1. - 1e-4
EPS = 1e-4
NEAR = 1e-3              # an element is "near a bound" when a or 1 - a lies within this RELATIVE distance of 1e-4
NUDGE_WITHIN = 1e-2      # the recipe moves every logit whose probability lies within this relative distance of a bound

# what tests/test_gpu_parsing_kernels.py parametrizes; tests/test_parsing_host.py asserts the input conditions on the same list
KERNEL_CLASSES = (2, 19, 20, 32, 33, 64, 65, 151)
KERNEL_ROWS = (3, 700)
KERNEL_DTYPES = (torch.float32, torch.bfloat16)
LOGIT_TYPES = ('softmax', 'sigmoid')
KERNEL_G = (1.25, 0.0, -0.75)          # dL/dterms: one zero and one negative component


def case_seed(C, rows, logit_type):
    return 1000 * C + rows + (7 if logit_type == 'sigmoid' else 0)


def _probabilities(x, logit_type):
    """a and 1 - a in float64, the latter without cancellation near a = 1 up to the float64 rounding of a sum of C terms"""
    if logit_type == 'softmax':
        a = torch.softmax(x, dim=1)
        na = a.sum(dim=1, keepdim=True) - a
        # the one class that can come close to 1: sum the others directly
        big = a.argmax(dim=1)
        rest = a.clone()
        rest[torch.arange(x.shape[0]), big] = 0.
        na[torch.arange(x.shape[0]), big] = rest.sum(dim=1)
        return a, na
    return torch.sigmoid(x), torch.sigmoid(-x)


def class_terms_judge(x, label, logit_type='softmax', g=(1., 1., 1.), lo=LO, hi=HI):
    """The analytic terms of ops.pixel_class_terms and the gradient of sum_k g_k terms_k in float64.
    x [rows, C] (any float dtype: taken as it is, upcast), label [rows] float class ids (outside [0, C): ignored, still counted).
    -> dict: terms [3], grad [rows, C], mask [rows, C] (element inside the clamp), near [rows, C], valid [rows],
       a, q, regime [rows] (0: a_t < lo, 1: inside, 2: a_t > hi; -1 on ignored rows)
    lo / hi: the clamp bounds, 1e-4 and 1 - 1e-4 -- the kernel's.  The reference holds them as float32 constants, and its
    log(1 - pred) at the upper bound reads 1 - float32(1 - 1e-4) = 1.00017e-4: the test that pins this judge to values recorded
    from the reference passes those constants."""
    x = x.detach().double().cpu()
    label = label.detach().double().cpu().reshape(-1)
    g = [float(v) for v in g]
    rows, C = x.shape
    valid = (label >= 0) & (label < C)
    t = torch.where(valid, label, torch.zeros_like(label)).long()
    ar = torch.arange(rows)
    y = torch.zeros_like(x)
    y[ar, t] = 1.
    a, na = _probabilities(x, logit_type)
    low, high = a < lo, na < 1. - hi
    mask = ~low & ~high
    q = torch.where(low, torch.full_like(a, lo), torch.where(high, torch.full_like(a, hi), a))
    nq = torch.where(low, torch.full_like(a, 1. - lo), torch.where(high, torch.full_like(a, 1. - hi), na))
    near = ((a - LO).abs() <= NEAR * LO) | ((na - LO).abs() <= NEAR * LO)
    I = q[ar, t]
    S = q.sum(dim=1)
    U = torch.clamp(S + 1. - I, min=EPS)
    D = S + 1. + EPS
    vf = valid.double()
    if logit_type == 'softmax':
        term0 = (-torch.log(I) * vf).sum() / rows
        d0 = -y / q / rows
    else:
        term0 = ((-(y * torch.log(q) + (1. - y) * torch.log(nq))).sum(dim=1) * vf).sum() / (rows * C)
        d0 = (-y / q + (1. - y) / nq) / (rows * C)
    term1 = ((1. - I / U) * vf).sum() / rows
    term2 = ((1. - (2. * I + EPS) / D) * vf).sum() / rows
    d1 = -(y * U[:, None] - I[:, None] * (1. - y)) / (U * U)[:, None] / rows
    d2 = -(2. * y * D[:, None] - (2. * I + EPS)[:, None]) / (D * D)[:, None] / rows
    h = mask.double() * (g[0] * d0 + g[1] * d1 + g[2] * d2)
    if logit_type == 'softmax':
        grad = a * (h - (h * a).sum(dim=1, keepdim=True))
    else:
        grad = h * a * na
    grad = grad * vf[:, None]
    at, nat = a[ar, t], na[ar, t]
    regime = torch.where(at < lo, 0, torch.where(nat < 1. - hi, 2, 1))
    regime = torch.where(valid, regime, torch.full_like(regime, -1))
    return {'terms': torch.stack([term0, term1, term2]), 'grad': grad, 'mask': mask, 'near': near, 'valid': valid, 'a': a, 'q': q,
            'regime': regime}


def class_terms_restated(x, label, logit_type='softmax'):
    """The reference formulas (human_parsing/losses.py: softmax or sigmoid, clamp, one-hot, sums, means) restated in float64 torch
    ops under autograd -> [3] = (CELoss or MultiClassBCELoss, IoULoss, DiceLoss).  Labels must lie in [0, C)."""
    C = x.shape[1]
    x = x.double()
    pr = torch.softmax(x, dim=-1) if logit_type == 'softmax' else torch.sigmoid(x)
    pr = torch.clamp(pr, min=LO, max=HI)
    y = torch.nn.functional.one_hot(label.reshape(-1).long(), num_classes=C).double()
    if logit_type == 'softmax':
        t0 = ((-torch.log(pr)) * y).sum(dim=-1).mean()
    else:
        t0 = (-(y * torch.log(pr) + (1. - y) * torch.log(1. - pr))).mean()
    inter = (pr * y).sum(dim=1)
    t1 = (1. - inter / torch.clamp(pr.sum(dim=1) + y.sum(dim=1) - inter, min=EPS)).mean()
    t2 = (1. - (2 * inter + EPS) / (pr.sum(dim=1) + y.sum(dim=1) + EPS)).mean()
    return torch.stack([t0, t1, t2])


def class_terms_inputs(rows, C, seed, dtype=torch.float32, logit_type='softmax'):
    """In the style of semseg_common.pixel_ce_inputs: x = randn * s, s from {1, 6, 14}; the target's logit is then set so that its
    probability lands in the regime r % 3 (0: a_t < 1e-4, 1: inside the clamp, 2: a_t > 1 - 1e-4) with a margin of at least 2 in
    the logit.  Unlike there, s is not drawn but cycles as (14, 1, 6)[(r + r // 3) % 3]: nine consecutive rows hold every (regime,
    scale) pair, and already three rows hold clamped and unclamped elements.  Under sigmoid the logits are scaled by 0.8 (more
    elements inside |z| < 9.21) and the target's logit is the regime's logit itself.
    The gradient jumps at a clamp bound, so no element may sit on one: every logit whose probability (or its complement) lies
    within relative 1e-2 of a bound is moved by max(0.1, 2^-6 |z|) -- at least two steps of `dtype` -- away from zero, and the
    values are rounded to `dtype` before they are looked at again.  Returned in `dtype`: what the kernel and the judge both read."""
    g = torch.Generator().manual_seed(seed)
    r = torch.arange(rows)
    s = torch.tensor([14., 1., 6.], dtype=torch.float64)[(r + r // 3) % 3]
    x = torch.randn(rows, C, generator=g, dtype=torch.float64) * s[:, None]
    label = torch.randint(0, C, (rows,), generator=g)
    regime = r % 3
    u = torch.rand(rows, generator=g, dtype=torch.float64)
    u[:3] = 0.45               # the first three rows sit mid-regime: a three-row case then has a row whose classes are all unclamped
    edge = math.log(1. / LO - 1.)                                    # logit(a_t) at the bounds is -edge / +edge
    delta = torch.where(regime == 0, -edge - 2. - 8. * u, torch.where(regime == 1, -(edge - 2.) + 2. * (edge - 2.) * u, edge + 2. + 8. * u))
    if logit_type == 'softmax':
        others = x.clone()
        others[r, label] = -float('inf')
        x[r, label] = torch.logsumexp(others, dim=1) + delta         # logit(a_t) = x_t - lse(others) = delta
    else:
        x = x * 0.8
        x[r, label] = delta
    x = x.to(dtype)
    for _ in range(20):
        a, na = _probabilities(x.double(), logit_type)
        close = ((a - LO).abs() <= NUDGE_WITHIN * LO) | ((na - LO).abs() <= NUDGE_WITHIN * LO)
        if not bool(close.any()):
            break
        xd = x.double()
        step = torch.clamp(xd.abs() * 2. ** -6, min=0.1)
        x = torch.where(close, xd + torch.where(xd >= 0, step, -step), xd).to(dtype)
    return x, label.float()
