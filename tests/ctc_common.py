"""The float64 judge of the CTC loss and the input recipes shared by tests/test_ctc_host.py (CPU) and tests/test_gpu_ctc_kernels.py.

The judge is a plain alpha-beta dynamic program in numpy float64 (log space, np.logaddexp); it does not call F.ctc_loss.  It follows
the reference's CTCLoss (SimpleAICV/text_recognition/losses.py:21-46): log-softmax, per-sample negative log-likelihood with
zero_infinity, optional focal weight (1 - exp(-nll)) ** gamma, / target length / batch, sum.  The gradient with respect to the
logits is written out analytically from the state occupancies -- no autograd.

The yardstick every kernel error is measured against is the reference formula in fp32 on the CPU for the same inputs
(`yardstick`)."""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

NEG = -np.inf


def _sample(lp, labels, blank):
    """lp [Tin, C] float64 log-probabilities, labels [L] -> (nll, occupancy-over-y [Tin, C] = sum_{s: l'_s = c} alpha beta / y / P,
    the largest |log-probability| of a class of the sample)"""
    tin, c = lp.shape
    L = len(labels)
    ext = np.full(2 * L + 1, blank, dtype=np.int64)
    ext[1::2] = labels
    ns = len(ext)
    skip = np.zeros(ns, dtype=bool)                 # state s may be entered from s - 2
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    e = lp[:, ext]                                  # [Tin, ns]
    alpha = np.full((tin, ns), NEG)
    alpha[0, 0] = e[0, 0]
    if ns > 1:
        alpha[0, 1] = e[0, 1]
    with np.errstate(invalid='ignore'):
        for t in range(1, tin):
            a = alpha[t - 1]
            v = a.copy()
            v[1:] = np.logaddexp(v[1:], a[:-1])
            v[2:] = np.where(skip[2:], np.logaddexp(v[2:], a[:-2]), v[2:])
            alpha[t] = v + e[t]
        ll = alpha[-1, -1] if ns == 1 else np.logaddexp(alpha[-1, -1], alpha[-1, -2])
        if not np.isfinite(ll):
            return np.inf, None, 0.0
        beta = np.full((tin, ns), NEG)
        beta[-1, -1] = e[-1, -1]
        if ns > 1:
            beta[-1, -2] = e[-1, -2]
        skipf = np.zeros(ns, dtype=bool)            # state s may go on to s + 2
        skipf[:-2] = skip[2:]
        for t in range(tin - 2, -1, -1):
            b = beta[t + 1]
            v = b.copy()
            v[:-1] = np.logaddexp(v[:-1], b[1:])
            v[:-2] = np.where(skipf[:-2], np.logaddexp(v[:-2], b[2:]), v[:-2])
            beta[t] = v + e[t]
    post = np.exp(alpha + beta - e - ll)            # alpha beta / y / P per state: the state posteriors
    occ = np.zeros((tin, c))
    for s in range(ns):                             # index order
        occ[:, ext[s]] += post[:, s]
    return -ll, occ, float(np.abs(e).max())


def judge(logits, targets, input_lengths, target_lengths, blank, gamma=None, gout=1.0):
    """logits [T, B, C] (anything np.asarray takes; computed in float64), targets [B, S] (entries at or beyond a sample's length
    are not looked at), lengths [B].  -> dict(nll [B], loss, grad [T, B, C], feasible [B], exponent).  nll of an infeasible sample
    is 0.  exponent: the largest of nll_b + max |lp| over the feasible samples -- the size of the log-domain terms whose sum the
    posterior exp(occ + nll - lp) is the exponential of (tests/test_gpu_ctc_kernels.py takes its gradient floor from it)."""
    x = np.asarray(logits, dtype=np.float64)
    T, B, C = x.shape
    targets = np.asarray(targets).astype(np.int64)
    nll = np.zeros(B)
    grad = np.zeros_like(x)
    feas = np.zeros(B, dtype=bool)
    loss = 0.0
    exponent = 0.0
    for b in range(B):
        tin, L = int(input_lengths[b]), int(target_lengths[b])
        labels = targets[b, :L]
        if tin <= 0:
            continue
        xb = x[:tin, b]
        m = xb.max(axis=1, keepdims=True)
        lp = xb - (m + np.log(np.exp(xb - m).sum(axis=1, keepdims=True)))
        n, occ, emax = _sample(lp, labels, blank)
        if not np.isfinite(n):
            continue
        feas[b] = True
        nll[b] = n
        exponent = max(exponent, abs(n) + emax)
        w, dw = 1.0, 1.0
        if gamma is not None:
            p = np.exp(-n)
            w = (1.0 - p) ** gamma
            dw = w + gamma * n * p * (1.0 - p) ** (gamma - 1.0)
        loss += w * n / L / B
        grad[:tin, b] = gout * dw / L / B * (np.exp(lp) - occ)
    return {'nll': nll, 'loss': loss, 'grad': grad, 'feasible': feas, 'exponent': exponent}


def reference_formula(preds, trans_targets, input_lengths, target_lengths, blank, gamma=None):
    """the reference's CTCLoss.forward as torch ops, in the dtype preds arrive in (the class itself calls preds.float() first)"""
    batch = preds.shape[1]
    lp = F.log_softmax(preds, dim=2)
    loss = F.ctc_loss(lp, trans_targets, input_lengths, target_lengths, blank=blank, reduction='none', zero_infinity=True)
    nll = loss.detach().clone()
    if gamma is not None:
        loss = torch.pow(1. - torch.exp(-loss), gamma) * loss
    return (loss / target_lengths / batch).sum(), nll


def yardstick(logits, targets, input_lengths, target_lengths, blank, gamma=None):
    """the reference formula in fp32 on the CPU -> dict(nll, loss, grad) as float64 numpy"""
    x = logits.detach().cpu().float().requires_grad_(True)
    safe = targets.cpu().long().clone()
    for b in range(safe.shape[0]):                  # F.ctc_loss on the CPU validates nothing beyond the length, but be explicit
        safe[b, int(target_lengths[b]):] = 0
    loss, nll = reference_formula(x, safe, input_lengths.cpu().long(), target_lengths.cpu().long(), blank, gamma)
    loss.backward()
    return {'nll': nll.double().numpy(), 'loss': float(loss.detach()), 'grad': x.grad.double().numpy()}


# ------------------------------------------------------------------------------------------------------------------ recipes
GRID_C = (3, 37, 64, 65, 257, 12113)
GRID_T = (1, 2, 7, 33, 90)
GRID_B = (1, 3)
BLANKS = ('first', 'c-2', 'last')
PAD_OFFSET = 5                                      # padding entries hold C + 5: reading one would be an out-of-range class


def blank_index(C, where):
    return {'first': 0, 'c-2': C - 2, 'last': C - 1}[where]


def boundary_classes(C):
    """classes on both sides of every boundary of the kernels' row loop: the 16-byte chunks (4 fp32 / 8 bf16 elements), the lane
    wrap (64 chunks), the four-chunk unroll (256 chunks) and the scalar tail (C // 4 * 4, C // 8 * 8), plus 0 and C - 1"""
    edges = {0, C - 1}
    for e in (4, 8, 256, 512, 1024, 2048, 4096, 8192, C // 4 * 4, C // 8 * 8, C // 1024 * 1024, C // 2048 * 2048):
        edges.update((e - 1, e))
    return sorted(k for k in edges if 0 <= k < C)


def make_case(C, T, B, blank_where, seed=0, S=None):
    """-> dict(logits fp32 [T, B, C] (bf16-exact values), targets int64 [B, S], input_lengths, target_lengths int32 [B], blank).
    Sample 0: full length, labels drawn from boundary_classes first.  With B == 3: sample 1 has input_length < T (when T > 1) and
    a repeated character; sample 2 is infeasible (a run of one character that needs 2 L - 1 > input_length frames)."""
    blank = blank_index(C, blank_where)
    g = torch.Generator().manual_seed(1000 * C + 10 * T + B + seed)
    logits = (torch.randn(T, B, C, generator=g) * 2).bfloat16().float()
    usable = [k for k in boundary_classes(C) if k != blank]
    L_need = [0] * B
    labels = []
    for b in range(B):
        if b == 2:                                  # infeasible: L = T // 2 + 2 equal characters need 2 L - 1 >= T + 1 frames
            L = T // 2 + 2
            lab = [usable[0]] * L
        elif b == 1:
            tin = max(1, T - 2)
            L = max(1, min(tin // 2, 12))
            lab = [usable[(i // 2) % len(usable)] for i in range(L)]      # pairs of repeats: aabb... needs L + L // 2 frames
            while L + sum(lab[i] == lab[i - 1] for i in range(1, L)) > tin:
                L -= 1
                lab = lab[:L]
        else:
            L = max(1, min(T // 2, len(usable) + 4))
            lab = [usable[i % len(usable)] for i in range(L)]
            while L + sum(lab[i] == lab[i - 1] for i in range(1, L)) > T:
                L -= 1
                lab = lab[:L]
        labels.append(lab)
        L_need[b] = len(lab)
    S = S or max(L_need) + 2
    targets = torch.full((B, S), C + PAD_OFFSET, dtype=torch.int64)
    for b, lab in enumerate(labels):
        targets[b, :len(lab)] = torch.tensor(lab)
    in_len = torch.full((B,), T, dtype=torch.int32)
    if B > 1:
        in_len[1] = max(1, T - 2)
    return {'logits': logits, 'targets': targets, 'input_lengths': in_len,
            'target_lengths': torch.tensor(L_need, dtype=torch.int32), 'blank': blank}


def special_cases():
    """name -> case: the target shapes the issue names beyond the grid"""
    out = {}

    def one(name, C, T, labs, blank, in_lens=None, seed=0, plant=0.0):
        g = torch.Generator().manual_seed(zlib.crc32(name.encode()) % 1000 + seed)
        B = len(labs)
        S = max(len(x) for x in labs) + 1
        targets = torch.full((B, S), C + PAD_OFFSET, dtype=torch.int64)
        logits = torch.randn(T, B, C, generator=g) * 2
        for b, lab in enumerate(labs):
            targets[b, :len(lab)] = torch.tensor(lab)
            path = [k for c in lab for k in (c, blank)]           # plant > 0 raises one alignment: nll of order 1
            for t in range(T):
                logits[t, b, path[t] if t < len(path) else blank] += plant
        out[name] = {'logits': logits.bfloat16().float(), 'targets': targets,
                     'input_lengths': torch.tensor(in_lens or [T] * B, dtype=torch.int32),
                     'target_lengths': torch.tensor([len(x) for x in labs], dtype=torch.int32), 'blank': blank}

    one('L1', 37, 7, [[5]], 0)
    one('aa_aba_run5', 37, 12, [[4, 4], [4, 9, 4], [6, 6, 6, 6, 6]], 35, in_lens=[12, 9, 12])
    one('focal_planted', 37, 12, [[4, 4], [4, 9, 4], [6, 6, 6, 6, 6]], 35, in_lens=[12, 9, 12], plant=11.0)
    one('L40_T90', 65, 90, [[1 + (i * 7) % 63 for i in range(40)]], 0)                       # 81 states: more than a wavefront
    one('L80_T170', 257, 170, [[(i * 11) % 255 for i in range(80)], [3] * 80], 255,
        in_lens=[170, 150])                         # 161 states; sample 1 needs 159 frames and has 150
    one('L80_T170_big', 12113, 170, [[(i * 151) % 12111 for i in range(80)]], 12111)
    return out


def grid_cases():
    return [(C, T, B, w) for C in GRID_C for T in GRID_T for B in GRID_B for w in BLANKS]


@functools.lru_cache(maxsize=None)
def case_and_judgement(key, gamma=None):
    """key: a grid tuple (C, T, B, blank_where) or a special-case name.  -> (case, judge result, yardstick result), computed once"""
    case = special_cases()[key] if isinstance(key, str) else make_case(*key)
    args = (case['logits'], case['targets'], case['input_lengths'], case['target_lengths'], case['blank'])
    return case, judge(args[0].numpy(), args[1].numpy(), args[2].numpy(), args[3].numpy(), args[4], gamma), yardstick(*args, gamma)


def greedy_case(C, T, B, seed=0):
    """logits with a planted maximum 1.0 above the runner-up in every row -> (logits [T, B, C], index [T, B]).  Every value is a
    multiple of 1/16 in [-3, 4]: exact in bf16, and so is the planted one"""
    g = torch.Generator().manual_seed(77 * C + T + B + seed)
    logits = (torch.randn(T, B, C, generator=g).clamp_(-3, 3) * 16).round() / 16
    pick = torch.randint(0, C, (T, B), generator=g)
    edges = boundary_classes(C)
    for i in range(min(T * B, len(edges))):         # the first rows put the maximum on the loop's boundaries
        pick.view(-1)[i] = edges[i]
    top = logits.max(dim=2).values
    logits.scatter_(2, pick.unsqueeze(2), (top + 1.0).unsqueeze(2))
    return logits, pick


def softmax_max64(logits):
    x = logits.double()
    return torch.softmax(x, dim=2).max(dim=2).values
