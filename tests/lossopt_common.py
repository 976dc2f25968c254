"""What tests/test_lossopt_judge_host.py (no GPU) and tests/test_gpu_lossopt_f64.py (MI355X) share for the kernels every training
iteration ends in: saicv_softmax_ce_fwd and saicv_scale_by_scalar of csrc/loss.hip, saicv_grad_stats, saicv_grad_clip_scale,
saicv_grad_clip_value, saicv_scaler_update, saicv_sgd_flat and saicv_adamw_flat of csrc/optim.hip.  The case tables, the input builders,
the float64 references written from each operation's definition (hyper-parameters as Python doubles, what torch.optim receives), the fp32
emulations of the kernels' arithmetic that set the constants and carry the planted faults, the judge and the launchers (C-ABI, outputs
and in-place arenas in guarded allocations).

Two regimes, as in glue_common.
  exact     torch.equal, nothing left out: SGD on dyadic operands (every fma exact), grad_clip_value (one rounded product and a clamp; NaN
            stays NaN, +-inf becomes +-value), grad_clip_scale when the coefficient clamps to 1 and inv_scale is a power of two, sumsq of
            gradients in {-1, 0, 1} (total below 2^24) in both accumulation modes with the pre-fill kept, found_inf (exactly 1 for any NaN,
            +inf or -inf wherever it lies, its pre-fill otherwise with FLT_MAX and denormals present), every word of the scaler state
            against torch's _amp_update_scale_ rule with each operation rounded to fp32, the AdamW step counters, every skipped block
            (found_inf, has_grad == 0, block_group < 0), the momentum arena when momentum == 0, padding elements that are 0 everywhere,
            invalid-label and all-zero-label rows of the cross-entropy, and row_loss / loss of a call without dlogits against the call
            that had one.  An element whose bound is 0 is held to equality in the accuracy regime too, which is how most of these are said.
  accuracy  |got - ref| <= allowed * u * bound (+ an absolute allowance where one is derived), u = 2^-24, bound the float64 magnitude sum
            of the element's own expression; `allowed` is FIXED[q] where the kernel is one correctly rounded operation and
            MARGIN * CONSTANTS[q] otherwise, CONSTANTS[q] the worst ratio of the fp32 emulation over the whole table (contracted and
            uncontracted forms, every arrival order of ORDER_SEEDS for the atomic sum).  Where the float64 reference is not finite (a
            soft label on a -inf logit: +inf, or 0 * -inf = NaN, as torch has it) the kernel must give the same non-finite value.

Bounds.
  CE gradient   (p (1 + |x - lse|) sum|y| + |y|) / B, p the softmax: (1 + |x - lse|) is the rounding of the exponent's argument.  Plus
                the absolute floor 2^-126 sum|y| / B where the softmax is below the smallest normal: flushing and not flushing both pass.
                The kernels' exp(x - lse) also pays u |lse| for the rounding of lse itself, which this bound does not grant: the
                constants carry it, and the shifted family (|lse| = 1e4) has constants of its own (GRAD_SUFFIX), 8e3 against 10.
  hard loss     |lse| + |x_t|              soft loss   |lse| sum|y| + sum|y x|
  loss          judged as the float64 mean of the row losses THE KERNEL WROTE, bound sum|row| / B: this isolates the fold
  sumsq         sum g^2 + the pre-fill; the fast mode's order is undefined: fold_partials over ORDER_SEEDS, as detloss_common does
  clip          |g| times the float64 coefficient
  SGD           m: mu |m| + |g is| + wd |p|;  p: |p| + lr (that, or with nesterov |g is| + wd |p| + mu (that))
  AdamW         p: |p| + (lr / bc1) |m'| / denom;  m: |m| + (1 - b1)(|g is| + |m|);  v: b2 v + (1 - b2)(g is)^2
The AdamW bound of p carries |m'|, not the magnitude sum behind it, so parameters are drawn with |p| >= scale / 2 (scale 1, or the
learning rate's order 1e-3, or 0.02 where three steps follow one another): an element where both p and m' cancel to nothing would
otherwise set the constant for the whole table.  With p of the order of lr the update is not hidden beneath u |p|, which is what makes the bias-correction faults visible.

No listed fault is without an observable value: NEUTRAL_FAULTS is empty.  (The clip coefficient without its + 1e-6 would be one on norms
above 2^24 * 1e-6 alone; the table has norms of order 1 and gradients of order 1e-6, where it shows.)
"""
import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

from attn_common import GUARD, MARGIN, SENTINEL, U, Guarded      # noqa: F401  (re-exported for the tests)
from detloss_common import ORDER_SEEDS, fold_partials
from glue_common import FILL_F, GuardedFill, _fma32, _gen, bf16_half_ulp

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
TD = {'f32': F32, 'bf16': BF16}
UF = U[F32]
TINY = 2.0 ** -126
FLT_MAX = 3.4028234663852886e38
LEFT_OUT_CAP = 0.005                                        # no case of these tables leaves an element out (the host test asserts it)
BLOCK = 1024                                                # elements of an optimizer block (one workgroup)
SWEEP = 2048 * 256 * 4                                      # elements one sweep of the capped gradient-utility grid covers
SCALE_SWEEP = 2048 * 256

# Worst ratio of the fp32 emulations to the float64 references over every case of the tables, in units of u * bound.  Measured by
# tests/test_lossopt_judge_host.py::test_constants_table_is_what_the_emulations_measure (which fails if a row drifts by more than a
# quarter, on one thread); the judge allows MARGIN times these.  Never raised by hand.
CONSTANTS = {
    'ce_hard_loss': 1.99, 'ce_soft_loss': 2.95, 'ce_hard_grad': 9.34, 'ce_soft_grad': 9.65, 'ce_hard_grad@shifted': 8180.0,
    'ce_soft_grad@shifted': 8110.0, 'ce_mean': 1.85, 'sumsq': 39.0, 'clip_coef': 3.02,
    'sgd_p': 3.16, 'sgd_m': 2.58, 'adamw_p': 3.37, 'adamw_m': 2.32, 'adamw_v': 4.33,
}
CONSTANTS_MEASURED_WITH = 'torch 2.10.0+rocm7.0 (CPU, one thread), 2026-10-21'
# derived: one correctly rounded product is within u |ref| (scale_by_scalar; grad_clip_scale whose coefficient clamped to 1 * inv_scale)
FIXED = {'prod': 1.0}


# ------------------------------------------------------------------------------------------------ launch geometry, restated
def stats_grid(n):
    """saicv_grad_stats / _grad_clip_scale / _grad_clip_value of csrc/optim.hip: (n / 4 + 255) / 256 capped at 2048"""
    return int(min(max((n // 4 + 255) // 256, 1), 2048))


def scale_grid(n):
    """saicv_scale_by_scalar of csrc/loss.hip: (n + 255) / 256 capped at 2048"""
    return int(min(max((n + 255) // 256, 1), 2048))


def ce_grid(B):
    """saicv_softmax_ce_fwd: four rows (one wavefront each) per workgroup"""
    return (B + 3) // 4


def opt_grid(n):
    """saicv_sgd_flat / _adamw_flat: one workgroup per 1024-element block"""
    return n // BLOCK


def stats_sweeps(n):
    return -(-n // (stats_grid(n) * 1024))


def d64(t):
    return t.to(F64)


def r32(t):
    return t.to(F32).to(F64)


def f32v(x):
    """a Python double rounded to fp32, as a double"""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ the judge
def allowed_ratio(q):
    return FIXED[q] if q in FIXED else MARGIN * CONSTANTS[q]


def judge(got, spec, worst=None):
    """spec: {name: ('equal', ref) | ('bound', ref, bound, quantity, extra)} -> list of complaints; glue_common.judge with one more rule:
    where the reference is not finite the value must be the same non-finite one.  An element whose bound is 0 must be exact."""
    bad = []
    for name, (kind, ref, *rest) in spec.items():
        g = got[name].detach().to(F64).cpu().reshape(ref.shape)
        same = (g == ref) | (torch.isnan(g) & torch.isnan(ref))
        if kind == 'equal':
            if not bool(same.all()):
                bad.append(f'{name}: {int((~same).sum())} of {ref.numel()} elements differ (exact comparison)')
            continue
        bnd, q, extra = rest
        finite = torch.isfinite(ref)
        b = torch.where(finite, torch.as_tensor(bnd, dtype=F64).expand(ref.shape), torch.zeros_like(ref)).abs() * UF
        err = torch.where(finite, (g - ref).abs(), torch.zeros_like(ref))
        if extra is not None:
            err = (err - torch.where(finite, torch.as_tensor(extra, dtype=F64).expand(ref.shape), torch.zeros_like(ref))).clamp_min(0.0)
        ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
        ratio = torch.where(torch.isnan(g) | torch.isnan(err), torch.full_like(ratio, math.inf), ratio)
        ratio = torch.where(finite, ratio, torch.where(same, torch.zeros_like(ratio), torch.full_like(ratio, math.inf)))
        r = float(ratio.max()) if ratio.numel() else 0.0
        if worst is not None:
            worst[q] = max(worst.get(q, 0.0), r)
        allowed = allowed_ratio(q)
        if not r <= allowed:
            bad.append(f'{name}: worst ratio {r:.4g} u*bound > {allowed:.4g} ({q}), {int((ratio > allowed).sum())} elements')
    return bad


def wave_tree(v):
    """wave_sum of csrc/common.h over the last axis (64 lanes): xor 1, xor 2, half mirror, mirror, xor 16, xor 32 -- a balanced tree over
    neighbouring lanes, the same bits in every lane because fp32 addition commutes"""
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def block_tree(w):
    """ordered_sum.h: the four wavefront sums as ((w0 + w1) + w2) + w3"""
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


# ================================================================================================ softmax cross-entropy
CE_SHAPES = ((1, 1), (3, 7), (5, 63), (4, 64), (6, 65), (9, 1000), (257, 100), (600, 10))
CE_LOGITS = ('randn3', 'shifted', 'dominant', 'equal', 'neginf')
CE_INVALID = (-1, -100, 'C', 2 ** 40)
# The kernels form the softmax as expf(x - lse) with lse = max + log(sum) already rounded: every probability pays u |lse| on top of the
# u |x - lse| the bound grants, 1e4 u on the shifted family.  That family's gradients are a quantity of their own, so that logits of
# the size 1e4 do not set the allowance of the ordinary ones (one constant over the whole table would be 8e3 for all of them).
GRAD_SUFFIX = {'shifted': '@shifted'}
SOFT_KINDS = ('onehot', 'twohot', 'smooth', 'softmax', 'half', 'double', 'zero')
CE_FAULTS = ('mean_over_valid_rows', 'invalid_row_gradient_not_zeroed', 'soft_gradient_without_label_sum', 'max_over_first_64_classes',
             'no_max_shift', 'idle_lanes_add_exp0', 'partial_last_workgroup_dropped', 'rows_beyond_256_dropped_from_mean')


@dataclass(frozen=True)
class CECase:
    id: str
    B: int
    C: int
    soft: bool
    logits: str


CE_CASES = tuple(CECase(f'{"soft" if s else "hard"}-b{B}-c{C}-{f}', B, C, s, f) for s in (False, True) for B, C in CE_SHAPES for f in CE_LOGITS)


def ce_invalid_rows(case):
    """{row: label} of the hard labels outside [0, C): odd rows, the four values rotating with the logit family"""
    if case.soft or case.B < 3:
        return {}
    k = CE_LOGITS.index(case.logits)
    out = {}
    for j in range(min(4, case.B // 2)):
        v = CE_INVALID[(j + k) % 4]
        out[2 * j + 1] = case.C if v == 'C' else v
    return out


def ce_inputs(case):
    """logits [B, C] (fp32 values), label int64 [B] or soft labels [B, C] (fp32 values)"""
    g = _gen(case.id)
    B, C, fam = case.B, case.C, case.logits
    k = CE_LOGITS.index(fam)
    x = torch.randn((B, C), generator=g, dtype=F64)
    hot = torch.randint(0, C, (B,), generator=g)
    other = (hot + 1 + torch.randint(0, max(C - 1, 1), (B,), generator=g)) % C
    rows = torch.arange(B)
    if fam == 'randn3':
        x = x * 3
    elif fam == 'shifted':
        x = x * 30 + 1e4
    elif fam == 'dominant':
        x[rows, torch.randint(0, C, (B,), generator=g)] += 200.0
    elif fam == 'equal':
        x = ((rows % 5).to(F64)[:, None] - 2) * 1.5 + torch.zeros_like(x)
    x = r32(x)
    if case.soft:
        y = torch.zeros((B, C), dtype=F64)
        sm = torch.softmax(torch.randn((B, C), generator=g, dtype=F64), 1)
        for r in range(B):
            kind = SOFT_KINDS[(r + k) % len(SOFT_KINDS)]
            if kind == 'onehot':
                y[r, hot[r]] = 1.0
            elif kind == 'twohot':
                y[r, hot[r]] += 0.7
                y[r, other[r]] += 0.3
            elif kind == 'smooth':
                y[r] = 0.1 / C
                y[r, hot[r]] += 0.9
            elif kind != 'zero':
                y[r] = sm[r] * {'softmax': 1.0, 'half': 0.5, 'double': 2.0}[kind]
        lab = r32(y)
        keep = lab > 0
    else:
        lab = hot.clone()
        for r, v in ce_invalid_rows(case).items():
            lab[r] = v
        keep = torch.zeros((B, C), dtype=torch.bool)
        keep[rows, hot] = True
    if fam == 'neginf' and C > 1:                           # some -inf entries; the hard label's class and one more stay finite
        drop = torch.rand((B, C), generator=g) < 0.3
        drop[rows, hot] = False
        drop[rows, other] = False
        if case.soft:                                       # a soft label may sit on one (+inf) and a zero label on another (NaN): see above
            drop[0::2] &= ~keep[0::2]
        x = torch.where(drop, torch.full_like(x, -math.inf), x)
    return {'x': x, 'label': lab}


def ce_reference(case, inp, got):
    """float64: logsumexp, row losses, the gradient (softmax * sum(y) - y) / B; `loss` from the rows the kernel wrote"""
    x, lab, B, C = inp['x'], inp['label'], case.B, case.C
    lse = torch.logsumexp(x, 1)
    dist = torch.where(torch.isinf(x), torch.zeros_like(x), (x - lse[:, None]).abs())
    p = torch.exp(x - lse[:, None])
    if case.soft:
        y = lab
        sy, say = y.sum(1), y.abs().sum(1)
        row = -(y * (x - lse[:, None])).sum(1)
        brow = lse.abs() * say + torch.where(y == 0, torch.zeros_like(x), (y * x).abs()).sum(1)
        grad = (p * sy[:, None] - y) / B
        bgrad = (p * (1 + dist) * say[:, None] + y.abs()) / B
        floor = (TINY * say / B)[:, None].expand(B, C)
        qs = ('ce_soft_loss', 'ce_soft_grad' + GRAD_SUFFIX.get(case.logits, ''))
    else:
        valid = (lab >= 0) & (lab < C)
        t = lab.clamp(0, C - 1)
        xt = x.gather(1, t[:, None])[:, 0]
        hot = torch.zeros_like(x).scatter_(1, t[:, None], 1.0)
        row = torch.where(valid, lse - xt, torch.zeros_like(lse))
        brow = torch.where(valid, lse.abs() + xt.abs(), torch.zeros_like(lse))
        v = valid.to(F64)[:, None]
        grad = (p - hot) / B * v
        bgrad = (p * (1 + dist) + hot) / B * v
        floor = (TINY / B) * v.expand(B, C)
        qs = ('ce_hard_loss', 'ce_hard_grad' + GRAD_SUFFIX.get(case.logits, ''))
    wrote = got['row_loss'].detach().to(F64).cpu().reshape(B)
    spec = {'row_loss': ('bound', row, brow, qs[0], None), 'dlogits': ('bound', grad, bgrad, qs[1], floor),
            'loss': ('bound', (wrote.sum() / B).reshape(1), (wrote.abs().sum() / B).reshape(1), 'ce_mean', None)}
    if 'row_loss_null' in got:                              # the call without dlogits: the same bits as the call that had one
        spec['row_loss_null'] = ('equal', wrote)
        spec['loss_null'] = ('equal', got['loss'].detach().to(F64).cpu().reshape(1))
    return spec


def ce_soft_tight_ratio(case, inp, got):
    """recorded, never asserted: the soft row loss against the reference formulation's own bound sum|y| |x - lse|, in units of u, over
    the rows where that bound is at least 1 (a one-hot row whose label dominates has a loss and a bound of 1e-9: any ratio)"""
    x, y = inp['x'], inp['label']
    lse = torch.logsumexp(x, 1)
    row = -(y * (x - lse[:, None])).sum(1)
    tight = (y.abs() * (x - lse[:, None]).abs()).sum(1)
    ok = torch.isfinite(row) & (tight >= 1.0)
    if not bool(ok.any()):
        return 0.0
    err = (got['row_loss'].detach().to(F64).cpu().reshape(-1) - row).abs()
    return float((err[ok] / (tight[ok] * UF)).max())


def _lanes(t):
    """[B, C] -> [B, K, 64]: class c in lane c % 64 on trip c / 64, zeros behind C"""
    B, C = t.shape
    K = -(-C // 64)
    pad = torch.zeros((B, K * 64), dtype=t.dtype)
    pad[:, :C] = t
    return pad.view(B, K, 64)


def fold_mean32(rows, B, limit=None):
    """mean_rows_kernel: lane t adds rows t, t + 256, ... to +0, wave_sum, the four wavefronts in order, one division by (float)B"""
    v = rows.to(F32).clone()
    if limit is not None:
        v[limit:] = 0.0
    K = -(-v.numel() // 256)
    pad = torch.zeros(K * 256, dtype=F32)
    pad[:v.numel()] = v
    acc = torch.zeros(256, dtype=F32)
    for k in range(K):
        acc = acc + pad[k * 256:(k + 1) * 256]
    return block_tree(wave_tree(acc.view(4, 64)))


def ce_emulate(case, inp, fault=None, fused=True, shift_first=False):
    """the kernels' fp32 arithmetic; fused: the contracted forms of sxy += y x, lse sy - sxy and p sy - y.  shift_first: NOT what the
    kernels do -- the softmax as exp((x - max) - log(sum)), which never rounds at |lse|; the host test records what it would buy"""
    B, C = case.B, case.C
    x = inp['x'].to(F32)
    mx = x.max(1).values
    if fault == 'max_over_first_64_classes':
        mx = x[:, :64].max(1).values
    if fault == 'no_max_shift':
        mx = torch.zeros_like(mx)
    sh = x - mx[:, None]
    e = _lanes(torch.exp(sh))
    if fault == 'idle_lanes_add_exp0' and C < 64:
        e[:, 0, C:] = 1.0
    acc = torch.zeros((B, 64), dtype=F32)
    for k in range(e.shape[1]):
        acc = acc + e[:, k]
    lg = torch.log(wave_tree(acc))
    lse = mx + lg
    pr = torch.exp(sh - lg[:, None]) if shift_first else torch.exp(x - lse[:, None])
    invB = torch.tensor(1.0, dtype=F32) / torch.tensor(float(B), dtype=F32)
    denom = float(B)
    if case.soft:
        y = inp['label'].to(F32)
        yl, xl = _lanes(y), _lanes(x)
        sy, sxy = torch.zeros((B, 64), dtype=F32), torch.zeros((B, 64), dtype=F32)
        for k in range(yl.shape[1]):
            sy = sy + yl[:, k]
            sxy = _fma32(yl[:, k], xl[:, k], sxy) if fused else sxy + yl[:, k] * xl[:, k]
        sy, sxy = wave_tree(sy), wave_tree(sxy)
        row = _fma32(lse, sy, -sxy) if fused else lse * sy - sxy
        if fault == 'soft_gradient_without_label_sum':
            grad = (pr - y) * invB
        else:
            grad = (_fma32(pr, sy[:, None].expand(B, C), -y) if fused else pr * sy[:, None] - y) * invB
    else:
        lab = inp['label']
        valid = (lab >= 0) & (lab < C)
        t = lab.clamp(0, C - 1)
        row = torch.where(valid, lse - x.gather(1, t[:, None])[:, 0], torch.zeros_like(lse))
        hot = torch.zeros_like(x).scatter_(1, t[:, None], 1.0) * valid.to(F32)[:, None]
        scale = invB.expand(B).clone()
        if fault != 'invalid_row_gradient_not_zeroed':
            scale = scale * valid.to(F32)
        grad = (pr - hot) * scale[:, None]
        if fault == 'mean_over_valid_rows':
            denom = float(max(int(valid.sum()), 1))
    if fault == 'partial_last_workgroup_dropped' and B % 4:
        row, grad = row.clone(), grad.clone()
        row[B // 4 * 4:] = math.nan
        grad[B // 4 * 4:] = math.nan
    total = fold_mean32(row, B, 256 if fault == 'rows_beyond_256_dropped_from_mean' else None)
    loss = (total / torch.tensor(denom, dtype=F32)).reshape(1)
    return {'row_loss': row.to(F64), 'dlogits': grad.to(F64), 'loss': loss.to(F64)}


def ce_candidates(case, inp, fault=None):
    return [ce_emulate(case, inp, fault, True), ce_emulate(case, inp, fault, False)] if case.soft else [ce_emulate(case, inp, fault)]


# ================================================================================================ scale_by_scalar
SCALE_SIZES = (1, 255, 256, 257, SCALE_SWEEP, SCALE_SWEEP + 1, 1100003)
SCALES = {'one': 1.0, 'pow2': 2.0 ** -7, 'seven': 7.0, 'third': f32v(1 / 3), 'zero': 0.0}
SCALE_FAULTS = ('beyond_first_sweep_untouched',)


@dataclass(frozen=True)
class ScaleCase:
    id: str
    n: int
    dt: str
    scale: str

    @property
    def exact(self):
        return self.scale in ('one', 'pow2', 'zero')


SCALE_CASES = tuple(ScaleCase(f'{dt}-n{n}-{s}', n, dt, s) for dt in ('f32', 'bf16') for n in SCALE_SIZES for s in SCALES)


def scale_inputs(case):
    return {'in': r32(torch.randn(case.n, generator=_gen(f'scale{case.n}'), dtype=F64)), 's': SCALES[case.scale]}


def scale_reference(case, inp, got=None):
    ref = inp['in'] * inp['s']
    if case.exact:
        return {'out': ('equal', ref.to(TD[case.dt]).to(F64))}
    return {'out': ('bound', ref, ref.abs(), 'prod', bf16_half_ulp(ref) if case.dt == 'bf16' else None)}


def scale_candidates(case, inp, fault=None):
    out = (inp['in'].to(F32) * torch.tensor(inp['s'], dtype=F32)).to(TD[case.dt]).to(F64)
    if fault == 'beyond_first_sweep_untouched':
        out[SCALE_SWEEP:] = math.nan
    return [{'out': out}]


# ================================================================================================ grad_stats
UTIL_SIZES = (4, 1020, 1024, 1028, SWEEP, SWEEP + 4, 2 * SWEEP + 8)
POISON = {'nan': math.nan, 'pinf': math.inf, 'ninf': -math.inf}
SUMSQ_PREFILL = 3.0
STATS_FAULTS = ('beyond_first_sweep_unsummed', 'found_inf_from_isinf_only', 'found_inf_misses_negative_inf', 'found_inf_flags_flt_max',
                'sumsq_overwritten')


@dataclass(frozen=True)
class StatsCase:
    id: str
    n: int
    det: bool
    which: str                  # sumsq | found | both
    data: str                   # randn | ints | edges (FLT_MAX, -FLT_MAX and denormals, all finite)
    poison: tuple = None        # (element, kind)
    found_prefill: float = 0.0


def _stats_table():
    c = []
    for i, n in enumerate(UTIL_SIZES):
        for det in (False, True):
            m = 'det' if det else 'fast'
            for which in ('sumsq', 'both'):
                c.append(StatsCase(f'randn-n{n}-{m}-{which}', n, det, which, 'randn'))
            c.append(StatsCase(f'ints-n{n}-{m}-both', n, det, 'both', 'ints', found_prefill=0.25 * det))
        c.append(StatsCase(f'edges-n{n}-{"det" if i % 2 else "fast"}-found', n, bool(i % 2), 'found', 'edges', found_prefill=0.25 * (i % 2 == 0)))
    spots = (('first', lambda n: 0, (4, 4, 1028)), ('last', lambda n: n - 1, (1028, SWEEP + 4, 2 * SWEEP + 8)),
             ('lane63', lambda n: 255, (1020, 1024, 1028)), ('sweep2', lambda n: SWEEP, (SWEEP + 4, SWEEP + 4, 2 * SWEEP + 8)),
             ('sweep3', lambda n: 2 * SWEEP, (2 * SWEEP + 8,) * 3))
    j = 0
    for name, at, sizes in spots:
        for kind, n in zip(POISON, sizes):
            det, which = bool(j % 2), ('found', 'both')[(j // 2) % 2]
            c.append(StatsCase(f'{kind}-{name}-n{n}-{"det" if det else "fast"}-{which}', n, det, which, 'randn', (at(n), kind), 0.25 * (j % 3 == 0)))
            j += 1
    return tuple(c)


STATS_CASES = _stats_table()


@functools.lru_cache(maxsize=4)
def _drawn(n, data, name):
    g = _gen(f'{name}{n}{data}')
    if data == 'ints':
        return torch.randint(-1, 2, (n,), generator=g).to(F64)
    return r32(torch.randn(n, generator=g, dtype=F64))


def _grads(n, data, name):
    x = _drawn(n, data, name).clone()
    if data == 'edges':
        x[0], x[1], x[2], x[n - 1] = FLT_MAX, 1e-40, -1e-45, -FLT_MAX
        x = r32(x)
    return x


def stats_inputs(case):
    x = _grads(case.n, case.data, 'stats')
    if case.poison:
        x[case.poison[0]] = POISON[case.poison[1]]
    return {'g': x}


def stats_reference(case, inp, got=None):
    x = inp['g']
    spec = {}
    if case.which != 'sumsq':
        bad = not bool(torch.isfinite(x).all())
        spec['found_inf'] = ('equal', torch.tensor([1.0 if bad else case.found_prefill], dtype=F64))
    if case.which != 'found':
        total = (x * x).sum().reshape(1) + SUMSQ_PREFILL
        spec['sumsq'] = ('equal', total) if case.data == 'ints' else ('bound', total, total.clone(), 'sumsq', None)
    return spec


def stats_partials(x, fault=None):
    """one fp32 partial per wavefront: a thread's quads of sweep 0, 1, ... through fma in element order, then wave_sum"""
    n = x.numel()
    grid = stats_grid(n)
    span = grid * 1024
    K = -(-n // span)
    pad = torch.zeros(K * span, dtype=F32)
    pad[:n] = x.to(F32)
    pad = pad.view(K, grid * 256, 4)
    acc = torch.zeros(grid * 256, dtype=F32)
    for k in range(1 if fault == 'beyond_first_sweep_unsummed' else K):
        for j in range(4):
            acc = _fma32(pad[k, :, j], pad[k, :, j], acc)
    return wave_tree(acc.view(grid * 4, 64)).numpy()


def stats_candidates(case, inp, fault=None):
    x = inp['g']
    got = {}
    if case.which != 'sumsq':
        seen = x if fault != 'beyond_first_sweep_unsummed' else x[:stats_grid(case.n) * 1024]
        bad = ~(seen.abs() <= FLT_MAX)
        if fault == 'found_inf_from_isinf_only':
            bad = torch.isinf(seen)
        if fault == 'found_inf_misses_negative_inf':
            bad = ~(seen <= FLT_MAX)
        if fault == 'found_inf_flags_flt_max':
            bad = ~(seen.abs() < FLT_MAX)
        got['found_inf'] = torch.tensor([1.0 if bool(bad.any()) else case.found_prefill], dtype=F64)
    if case.which == 'found':
        return [got]
    parts = stats_partials(x, fault)
    pre = 0.0 if fault == 'sumsq_overwritten' else SUMSQ_PREFILL
    with np.errstate(all='ignore'):
        return [{**got, 'sumsq': torch.tensor([fold_partials(parts, pre, seed)], dtype=F64)} for seed in ((None,) if case.det else ORDER_SEEDS)]


# ================================================================================================ grad_clip_scale, grad_clip_value
INV_SCALES = {'null': None, 'p2': 2.0 ** -16, 'third': f32v(1 / 3)}
CLIP_SCALE_FAULTS = ('beyond_first_sweep_untouched', 'coef_without_eps', 'coef_not_clamped_at_1', 'unscale_applied_twice', 'unscale_not_applied')
CLIP_VALUE_FAULTS = ('beyond_first_sweep_untouched', 'clamp_before_unscale', 'nan_clamped_to_value')
NEUTRAL_FAULTS = {}                                         # fault -> the reason it changes nothing observable: none is listed


@dataclass(frozen=True)
class ClipScaleCase:
    id: str
    n: int
    inv: str
    norm: str                   # above (max_norm above the norm: the coefficient clamps to 1) | below | zero (sumsq == 0)
    tiny: bool = False          # gradients of the order 1e-6: the + 1e-6 of the coefficient decides

    @property
    def exact(self):
        return self.norm != 'below' and self.inv != 'third'


def _clip_scale_table():
    c = [ClipScaleCase(f'n{n}-{inv}-{norm}', n, inv, norm) for n in UTIL_SIZES for inv in INV_SCALES for norm in ('above', 'below')]
    c += [ClipScaleCase(f'n{n}-{inv}-zero', n, inv, 'zero') for n, inv in ((4, 'null'), (1028, 'p2'), (SWEEP + 4, 'third'))]
    c += [ClipScaleCase(f'n{n}-{inv}-below-tiny', n, inv, 'below', True) for n, inv in ((4, 'null'), (1020, 'null'), (1028, 'third'))]
    return tuple(c)


CLIP_SCALE_CASES = _clip_scale_table()


def clip_scale_inputs(case):
    x = _grads(case.n, 'randn', 'clip')
    inv = INV_SCALES[case.inv]
    if case.tiny:
        x = x * 2.0 ** -20
    if inv is not None and not case.tiny:
        x = r32(x / inv)                                    # scaled gradients, as a GradScaler leaves them
    sumsq = 0.0 if case.norm == 'zero' else f32v(float((x * x).sum()))
    norm = math.sqrt(sumsq) * (1.0 if inv is None else inv)
    max_norm = {'above': 2.0 * norm + 1.0, 'below': 0.37 * norm, 'zero': 1.0}[case.norm]
    return {'g': x, 'sumsq': sumsq, 'inv': inv, 'max_norm': max_norm}


def clip_scale_reference(case, inp, got=None):
    x, inv = inp['g'], 1.0 if inp['inv'] is None else inp['inv']
    coef = min(1.0, inp['max_norm'] / (math.sqrt(inp['sumsq']) * inv + 1e-6)) * inv
    ref = x * coef
    if case.exact:
        return {'g': ('equal', ref)}
    return {'g': ('bound', ref, ref.abs(), 'prod' if case.norm != 'below' else 'clip_coef', None)}


def clip_scale_candidates(case, inp, fault=None):
    x = inp['g'].to(F32)
    f = lambda v: torch.tensor(v, dtype=F32)      # noqa: E731
    inv, eps = f(1.0 if inp['inv'] is None else inp['inv']), f(1e-6)
    out, last = [], None
    for fused in (True, False):
        root = torch.sqrt(f(inp['sumsq']))
        total = _fma32(root, inv, eps) if fused else root * inv + eps
        if fault == 'coef_without_eps':
            total = root * inv
        coef = f(inp['max_norm']) / total
        if fault != 'coef_not_clamped_at_1':
            coef = torch.minimum(coef, f(1.0))
        if fault != 'unscale_not_applied':
            coef = coef * inv
        if fault == 'unscale_applied_twice':
            coef = coef * inv
        if fused or float(coef) != last:                    # the two forms differ in the coefficient alone
            g = x * coef
            if fault == 'beyond_first_sweep_untouched':
                g[SWEEP:] = x[SWEEP:]
            out.append({'g': g.to(F64)})
        last = float(coef)
    return out


@dataclass(frozen=True)
class ClipValueCase:
    id: str
    n: int
    inv: str
    value: float


CLIP_VALUE_CASES = tuple(ClipValueCase(f'n{n}-{inv}-v{v:g}', n, inv, v) for n in UTIL_SIZES for inv in INV_SCALES
                         for v in ((0.3, 1e9) if n in (1028, SWEEP + 4) else (0.3,)))


def clip_value_inputs(case):
    """scaled gradients with NaN, +inf and -inf planted: at the front, and at the first element of every later sweep"""
    x = _grads(case.n, 'randn', 'value')
    inv = INV_SCALES[case.inv]
    if inv is not None:
        x = r32(x / inv)
    x[0], x[1], x[case.n - 1] = math.nan, math.inf, -math.inf
    for s, v in ((SWEEP, math.inf), (SWEEP + 1, math.nan), (2 * SWEEP, -math.inf), (2 * SWEEP + 1, math.nan)):
        if s < case.n - 1:
            x[s] = v
    return {'g': x, 'inv': inv}


def clip_value_reference(case, inp, got=None):
    """clamp(fp32(g * inv_scale), -fp32(value), fp32(value)), NaN kept: one rounded product and a clamp, so the comparison is exact"""
    u = r32(inp['g'] * (1.0 if inp['inv'] is None else inp['inv']))
    v = f32v(case.value)
    return {'g': ('equal', torch.where(torch.isnan(u), u, u.clamp(-v, v)))}


def clip_value_candidates(case, inp, fault=None):
    x = inp['g'].to(F32)
    inv, v = torch.tensor(1.0 if inp['inv'] is None else inp['inv'], dtype=F32), f32v(case.value)
    if fault == 'clamp_before_unscale':
        g = torch.where(torch.isnan(x), x, x.clamp(-v, v)) * inv
    else:
        u = x * inv
        g = torch.where(torch.isnan(u), torch.full_like(u, v) if fault == 'nan_clamped_to_value' else u, u.clamp(-v, v))
    if fault == 'beyond_first_sweep_untouched':
        g[SWEEP:] = x[SWEEP:]
    return [{'g': g.to(F64)}]


# ================================================================================================ scaler_update
SCALER_FAULTS = ('tracker_not_reset_on_growth', 'growth_one_step_late', 'reciprocal_not_refreshed')
SCALER_INV_PREFILL = 77.0


@dataclass(frozen=True)
class ScalerCase:
    id: str
    scale: float
    tracker: float
    found: float
    growth: float = 2.0
    backoff: float = 0.5
    interval: int = 2000


SCALER_CASES = (
    ScalerCase('clean-first', 65536.0, 0.0, 0.0), ScalerCase('clean-one-before-the-interval', 65536.0, 1997.0, 0.0),
    ScalerCase('clean-reaches-the-interval', 65536.0, 1999.0, 0.0), ScalerCase('overflow', 65536.0, 5.0, 1.0),
    ScalerCase('overflow-flag-3', 1024.0, 0.0, 3.0), ScalerCase('overflow-flag-half', 1024.0, 7.0, 0.5),
    ScalerCase('overflow-flag-negative', 1024.0, 1.0, -1.0), ScalerCase('interval-1', 1024.0, 0.0, 0.0, interval=1),
    ScalerCase('growth-1.5-reaches', 1000.0, 2.0, 0.0, 1.5, 0.3, 3), ScalerCase('backoff-0.3', 1000.0, 2.0, 1.0, 1.5, 0.3, 3),
    ScalerCase('scale-3-reciprocal', 3.0, 0.0, 0.0, interval=2), ScalerCase('scale-1-reaches-8', 1.0, 7.0, 0.0, interval=8),
    ScalerCase('growth-would-overflow', 2.0 ** 126, 0.0, 0.0, growth=4.0, interval=1),
)


def scaler_inputs(case):
    return {'state': torch.tensor([case.scale, case.tracker, SCALER_INV_PREFILL], dtype=F64), 'found': case.found}


def scaler_reference(case, inp, got=None):
    """torch.amp.GradScaler's update rule (ATen's _amp_update_scale_: grow when the tracker reaches the interval, never into inf), each
    operation rounded to fp32"""
    scale, tracker = case.scale, case.tracker
    if case.found != 0:
        scale, tracker = f32v(scale * f32v(case.backoff)), 0.0
    else:
        tracker += 1
        if tracker == case.interval:
            grown = scale * f32v(case.growth)
            scale = f32v(grown) if abs(grown) <= FLT_MAX else scale
            tracker = 0.0
    return {'state': ('equal', torch.tensor([scale, tracker, f32v(1.0 / scale)], dtype=F64))}


def scaler_candidates(case, inp, fault=None):
    f = np.float32
    s, t = f(case.scale), f(case.tracker)
    with np.errstate(all='ignore'):
        if case.found != 0:
            s, t = f(s * f(case.backoff)), f(0)
        else:
            t = f(t + f(1))
            if (int(t) > case.interval) if fault == 'growth_one_step_late' else (int(t) >= case.interval):
                grown = f(s * f(case.growth))
                s = grown if np.isfinite(grown) else s
                t = t if fault == 'tracker_not_reset_on_growth' else f(0)
        inv = f(SCALER_INV_PREFILL) if fault == 'reciprocal_not_refreshed' else f(f(1) / s)
    return [{'state': torch.tensor([float(s), float(t), float(inv)], dtype=F64)}]


# ================================================================================================ the flat optimizers
SGD_GROUPS = (dict(lr=0.1, wd=5e-4, mu=0.9, nesterov=False), dict(lr=0.03, wd=0.0, mu=0.9, nesterov=True),
              dict(lr=1e-3, wd=1e-2, mu=0.0, nesterov=False), dict(lr=0.5, wd=1e-4, mu=0.5, nesterov=True))
SGD_DYADIC = (dict(lr=0.5, wd=0.25, mu=0.5, nesterov=False), dict(lr=0.25, wd=0.0, mu=0.5, nesterov=True),
              dict(lr=0.125, wd=0.5, mu=0.0, nesterov=False), dict(lr=1.0, wd=0.125, mu=0.25, nesterov=True))
ADAMW_GROUPS = (dict(lr=1e-3, wd=0.05, b1=0.9, b2=0.999, eps=1e-8), dict(lr=1e-4, wd=0.0, b1=0.9, b2=0.95, eps=1e-6),
                dict(lr=5e-4, wd=0.1, b1=0.0, b2=0.9999, eps=1e-8), dict(lr=2e-3, wd=0.01, b1=0.9, b2=0.999, eps=1e-6))
STEP_PREFILLS = (0.0, 1.0, 9.0, 999.0, 99999.0)
PAD = 24                                                    # the last elements of every block: p = g = m = v = 0, as arena padding is
OPT_COMBOS = (   # has_grad, found_inf, inv_scale, parameter scale, exact (SGD only)
    ('null', 'null', 'null', 1.0, False), ('ones', 'zero', 'p2', 1e-3, False), ('mixed', 'null', 'third', 1.0, False),
    ('mixed', 'zero', 'null', 1e-3, False), ('null', 'one', 'p2', 1.0, False), ('ones', 'null', 'third', 1e-3, False),
    ('mixed', 'null', 'p2', 1.0, True), ('null', 'zero', 'null', 1.0, True))
OPT_INV = {'null': None, 'p2': 2.0 ** -10, 'third': f32v(1 / 3)}
SGD_FAULTS = ('group_0_row_for_every_block', 'nesterov_ignored', 'momentum_written_when_mu_is_0', 'momentum_decayed_on_block_without_grad',
              'stepping_despite_found_inf', 'weight_decay_on_scaled_gradient')
ADAMW_FAULTS = ('bc2_from_powf', 'one_minus_beta2_subtracted_in_fp32', 'eps_inside_bias_corrected_root', 'coupled_l2_decay',
                'decay_after_update', 'counter_advanced_on_skipped_step', 'block_0_counter_for_every_block')


@dataclass(frozen=True)
class OptCase:
    id: str
    kind: str                   # sgd | adamw
    blocks: int
    has_grad: str               # null | ones | mixed
    found: str                  # null | zero | one
    inv: str
    pscale: float
    exact: bool = False
    steps: int = 1
    zero_state: bool = False
    lone_group: int = 0         # the group of a one-block arena (-1: a block that belongs to nobody)

    @property
    def groups(self):
        return ADAMW_GROUPS if self.kind == 'adamw' else SGD_DYADIC if self.exact else SGD_GROUPS


def _opt_table(kind):
    c = []
    for blocks in (1, 2, 37):
        for i, (hg, fi, inv, ps, ex) in enumerate(OPT_COMBOS):
            if ex and kind == 'adamw':
                continue
            c.append(OptCase(f'{kind}-blk{blocks}-hg_{hg}-fi_{fi}-is_{inv}-p{ps:g}{"-exact" if ex else ""}', kind, blocks, hg, fi, inv, ps, ex,
                             lone_group=(i + 1) % 4))
    c.append(OptCase(f'{kind}-blk1-nobody', kind, 1, 'null', 'null', 'null', 1.0, lone_group=-1))
    # |p| >= 0.01 here: three AdamW steps move a parameter by up to 3 lr = 6e-3, and one that lands on 0 would lose the floor under |p|
    for blocks, ps, inv in ((2, 0.02, 'null'), (37, 0.02, 'p2'), (37, 1.0, 'third')):
        c.append(OptCase(f'{kind}-blk{blocks}-three-steps-from-zero-is_{inv}-p{ps:g}', kind, blocks, 'ones', 'zero', inv, ps, steps=3, zero_state=True))
    return tuple(c)


SGD_CASES, ADAMW_CASES = _opt_table('sgd'), _opt_table('adamw')


def opt_block_group(case):
    """groups interleaved over the blocks (a neighbour's row is a different row); every fifth block belongs to nobody"""
    if case.blocks == 1:
        return torch.tensor([case.lone_group], dtype=torch.int32)
    b = torch.arange(case.blocks)
    return torch.where(b % 5 == 3, torch.full_like(b, -1), (b * 3 + 1) % 4).to(torch.int32)


def opt_hyper_table(case):
    """the device table as engine.py fills it: doubles rounded to fp32, 8 floats per group"""
    if case.kind == 'sgd':
        rows = [[g['lr'], g['wd'], g['mu'], 0, 0, 0, 0, 1.0 if g['nesterov'] else 0.0] for g in case.groups]
    else:
        rows = [[g['lr'], g['wd'], g['b1'], g['b2'], g['eps'], 1 - g['b1'], 1 - g['b2'], 0] for g in case.groups]
    return torch.tensor(rows, dtype=F32)


def opt_inputs(case):
    """-> {'state': {p, m, (v, step)}, 'grads': [g per step], bg, hg, found, inv}; fp32 values held in float64 (bg int32, hg uint8)"""
    gen = _gen(case.id)
    n = case.blocks * BLOCK
    rn = lambda s=1.0: torch.randn(n, generator=gen, dtype=F64) * s      # noqa: E731
    inv = OPT_INV[case.inv]
    if case.exact:
        ri = lambda lo, hi: torch.randint(lo, hi, (n,), generator=gen).to(F64) / 4      # noqa: E731
        p, m, grads = ri(-8, 9), ri(-8, 9), [ri(-8, 9) / (1.0 if inv is None else inv)]
    else:
        sign = torch.where(torch.rand(n, generator=gen, dtype=F64) < 0.5, -1.0, 1.0)
        p = r32(sign * case.pscale * (0.5 + torch.rand(n, generator=gen, dtype=F64)))
        m = r32(rn(0.5))
        grads = [r32(rn() / (1.0 if inv is None else inv)) for _ in range(case.steps)]
    v = r32((0.5 + torch.rand(n, generator=gen, dtype=F64)) ** 2)       # sqrt(v) of the gradient's order, as a running average is
    live = (torch.arange(n) % BLOCK < BLOCK - PAD).to(F64)
    if case.zero_state:
        m, v = torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    state = {'p': p * live, 'm': m * live}
    if case.kind == 'adamw':
        state['v'] = v * live
        state['step'] = torch.zeros(case.blocks, dtype=F64) if case.zero_state else torch.tensor(STEP_PREFILLS, dtype=F64)[(torch.arange(case.blocks) + case.lone_group) % 5]
    hg = {'null': None, 'ones': torch.ones(case.blocks, dtype=torch.uint8),
          'mixed': (torch.arange(case.blocks) % 3 != 1).to(torch.uint8) if case.blocks > 1 else torch.zeros(1, dtype=torch.uint8)}[case.has_grad]
    if case.has_grad == 'mixed' and case.blocks > 1:
        hg[0] = 200                                         # any non-zero byte means "has a gradient"
    return {'state': state, 'grads': [g * live for g in grads], 'bg': opt_block_group(case), 'hg': hg,
            'found': {'null': None, 'zero': 0.0, 'one': 1.0}[case.found], 'inv': inv}


def opt_updated(case, inp, fault=None):
    """bool [blocks]: the blocks a step updates"""
    upd = inp['bg'] >= 0
    if inp['hg'] is not None:
        upd = upd & (inp['hg'] != 0)
    if inp['found'] is not None and inp['found'] != 0 and fault != 'stepping_despite_found_inf':
        upd = upd & False
    return upd


def _per_element(case, inp, dtype, rows=None):
    """the hyper-parameters of every element's group -> dict of [n] tensors (dtype F64: the Python doubles; F32: the device table)"""
    grp = inp['bg'].long().clamp_min(0) if rows is None else rows
    if dtype == F64:
        names = [k for k in case.groups[0]]
        tab = {k: torch.tensor([float(g[k]) for g in case.groups], dtype=F64) for k in names}
    else:
        t = opt_hyper_table(case)
        cols = dict(lr=0, wd=1, mu=2, nesterov=7) if case.kind == 'sgd' else dict(lr=0, wd=1, b1=2, b2=3, eps=4, omb1=5, omb2=6)
        tab = {k: t[:, c] for k, c in cols.items()}
    return {k: v[grp].repeat_interleave(BLOCK) for k, v in tab.items()}


def opt_step_reference(case, inp, state, g):
    """float64 from the fp32 state the kernel starts from: torch.optim.SGD (dampening 0) / torch.optim.AdamW, one step"""
    h = _per_element(case, inp, F64)
    upd = opt_updated(case, inp).repeat_interleave(BLOCK)
    p, m = state['p'], state['m']
    d = g * (1.0 if inp['inv'] is None else inp['inv'])
    zero = torch.zeros_like(p)
    if case.kind == 'sgd':
        mu, nes = h['mu'], h['nesterov'] != 0
        e = d + h['wd'] * p
        be = d.abs() + h['wd'] * p.abs()
        m2 = torch.where(mu != 0, mu * m + e, m)
        bm = mu * m.abs() + be
        step = torch.where(mu != 0, torch.where(nes, e + mu * m2, m2), e)
        bstep = torch.where(mu != 0, torch.where(nes, be + mu * bm, bm), be)
        p2, bp = p - h['lr'] * step, p.abs() + h['lr'] * bstep
        bm = torch.where(mu != 0, bm, zero)
        new = {'p': (p2, bp, 'sgd_p'), 'm': (m2, bm, 'sgd_m')}
    else:
        v = state['v']
        t = (state['step'] + 1).repeat_interleave(BLOCK)
        b1, b2 = h['b1'], h['b2']
        pd = p * (1 - h['lr'] * h['wd'])
        m2 = m + (1 - b1) * (d - m)
        v2 = b2 * v + (1 - b2) * d * d
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        denom = v2.sqrt() / bc2.sqrt() + h['eps']
        p2 = pd - (h['lr'] / bc1) * m2 / denom
        bp = p.abs() + (h['lr'] / bc1) * m2.abs() / denom
        new = {'p': (p2, bp, 'adamw_p'), 'm': (m2, m.abs() + (1 - b1) * (d.abs() + m.abs()), 'adamw_m'), 'v': (v2, v2.clone(), 'adamw_v')}
    spec = {}
    for k, (ref, bnd, q) in new.items():
        ref, bnd = torch.where(upd, ref, state[k]), torch.where(upd, bnd, zero)
        spec[k] = ('equal', ref) if case.exact else ('bound', ref, bnd, q, None)
    if case.kind == 'adamw':
        spec['step'] = ('equal', state['step'] + opt_updated(case, inp).to(F64))
    return spec


def opt_step_emulate(case, inp, state, g, fault=None, fused=True):
    """one launch in the kernel's fp32 arithmetic; fused: the contracted forms of 1 - lr wd and sqrt(v) rs2 + eps"""
    rows = None
    if fault == 'group_0_row_for_every_block':
        rows = torch.zeros(case.blocks, dtype=torch.long)
    h = _per_element(case, inp, F32, rows)
    updb = opt_updated(case, inp, fault)
    upd = updb.repeat_interleave(BLOCK)
    p, m, g32 = state['p'].to(F32), state['m'].to(F32), g.to(F32)
    inv = torch.tensor(1.0 if inp['inv'] is None else inp['inv'], dtype=F32)
    d = g32 * inv
    out = {}
    if case.kind == 'sgd':
        mu, lr, wd = h['mu'], h['lr'], h['wd']
        e = (_fma32(wd, p, g32) * inv) if fault == 'weight_decay_on_scaled_gradient' else _fma32(wd, p, d)
        m2 = _fma32(mu, m, e)
        nes = (h['nesterov'] != 0) & (fault != 'nesterov_ignored')
        step = torch.where(mu != 0, torch.where(nes, _fma32(mu, m2, e), m2), e)
        keep_m = mu == 0 if fault != 'momentum_written_when_mu_is_0' else torch.zeros_like(upd)
        new = {'p': _fma32(-lr, step, p), 'm': torch.where(keep_m, m, torch.where(mu != 0, m2, e))}
        if fault == 'momentum_decayed_on_block_without_grad' and inp['hg'] is not None:
            idle = ((inp['bg'] >= 0) & (inp['hg'] == 0)).repeat_interleave(BLOCK)
            m = torch.where(idle, mu * m, m)
        old = {'p': p, 'm': m}
    else:
        v = state['v'].to(F32)
        s0 = state['step'].to(F32)
        tb = (s0[0].expand(case.blocks) if fault == 'block_0_counter_for_every_block' else s0) + 1
        omb1, omb2, b2 = h['omb1'], h['omb2'], h['b2']
        if fault == 'one_minus_beta2_subtracted_in_fp32':
            omb2 = 1 - b2
        t = tb.repeat_interleave(BLOCK)
        bc1 = -torch.expm1(t * torch.log1p(-h['omb1']))
        bc2 = (1 - torch.pow(b2, t)) if fault == 'bc2_from_powf' else -torch.expm1(t * torch.log1p(-omb2))
        step, rs2 = h['lr'] / bc1, torch.rsqrt(bc2)
        one = torch.ones((), dtype=F32)
        decay = _fma32(-h['lr'], h['wd'], one) if fused else 1 - h['lr'] * h['wd']
        if fault == 'coupled_l2_decay':
            d = _fma32(h['wd'], p, d)
        pd = p if fault in ('coupled_l2_decay', 'decay_after_update') else p * decay
        m2 = _fma32(omb1, d - m, m)
        v2 = _fma32(omb2 * d, d, b2 * v)
        root = torch.sqrt(v2)
        if fault == 'eps_inside_bias_corrected_root':
            denom = (root + h['eps']) * rs2
        else:
            denom = _fma32(root, rs2, h['eps']) if fused else root * rs2 + h['eps']
        p2 = _fma32(-step, m2 / denom, pd)
        if fault == 'decay_after_update':
            p2 = p2 * decay
        new, old = {'p': p2, 'm': m2, 'v': v2}, {'p': p, 'm': m, 'v': v}
        out['step'] = torch.where(torch.ones_like(updb) if fault == 'counter_advanced_on_skipped_step' else updb, tb, s0).to(F64)
    for k in new:
        out[k] = torch.where(upd, new[k], old[k]).to(F64)
    return out


def opt_check(case, inp, stepper, worst=None):
    """runs the case's steps through `stepper(state, g) -> new state` (an emulation or the launcher), each step judged against the float64
    reference that starts from the state the stepper was given -> complaints.  The state a step wrote is what the next one reads."""
    state, bad = inp['state'], []
    for k, g in enumerate(inp['grads']):
        spec = opt_step_reference(case, inp, state, g)
        new = stepper(state, g)
        bad += [f'step {k}: {msg}' for msg in judge(new, spec, worst)]
        state = {name: new[name].detach().to(F64).cpu() for name in spec}
    return bad


def opt_steppers(case, inp, fault=None):
    forms = (True, False) if case.kind == 'adamw' else (True,)
    return [lambda s, g, f=f: opt_step_emulate(case, inp, s, g, fault, f) for f in forms]


# ================================================================================================ the families
FAMILIES = {
    'ce': (CE_CASES, ce_inputs, ce_reference, ce_candidates, CE_FAULTS),
    'scale': (SCALE_CASES, scale_inputs, scale_reference, scale_candidates, SCALE_FAULTS),
    'stats': (STATS_CASES, stats_inputs, stats_reference, stats_candidates, STATS_FAULTS),
    'clip_scale': (CLIP_SCALE_CASES, clip_scale_inputs, clip_scale_reference, clip_scale_candidates, CLIP_SCALE_FAULTS),
    'clip_value': (CLIP_VALUE_CASES, clip_value_inputs, clip_value_reference, clip_value_candidates, CLIP_VALUE_FAULTS),
    'scaler': (SCALER_CASES, scaler_inputs, scaler_reference, scaler_candidates, SCALER_FAULTS),
}
OPT_FAMILIES = {'sgd': (SGD_CASES, SGD_FAULTS), 'adamw': (ADAMW_CASES, ADAMW_FAULTS)}
FAULTS = {**{f: spec[4] for f, spec in FAMILIES.items()}, **{f: spec[1] for f, spec in OPT_FAMILIES.items()}}


def case_size(case):
    return getattr(case, 'n', 0) or getattr(case, 'blocks', 0) * BLOCK or getattr(case, 'B', 0) * getattr(case, 'C', 0)


def complaints(family, case, inp, fault=None, worst=None):
    """every emulated form of a case (with `fault` planted) through the judge -> list of complaint lists, one per form"""
    if family in OPT_FAMILIES:
        return [opt_check(case, inp, st, worst) for st in opt_steppers(case, inp, fault)]
    _, _, reference, candidates, _ = FAMILIES[family]
    return [judge(got, reference(case, inp, got), worst) for got in candidates(case, inp, fault)]


# ================================================================================================ device side (needs a GPU)
def _L():
    from simpleaicv_pytorch_training_examples_amd import _lib
    return _lib, _lib.lib()


def _filled(t, dtype=F32, device='cuda', written=False):
    """an in-place arena: the values of t inside an allocation of sentinel elements"""
    return GuardedFill(tuple(t.shape), dtype, device, t, written=written)


def _out(shape, device='cuda'):
    """an output that may legitimately hold NaN: pre-filled with a value no result takes"""
    return GuardedFill(tuple(shape), F32, device, FILL_F)


def _finish(outs):
    torch.cuda.synchronize()
    return {n: g.view.to(F64).cpu() for n, g in outs}, [m for n, g in outs for m in g.check(n)]


def _scalar(v, device):
    return None if v is None else torch.tensor([v], dtype=F32, device=device)


def run_ce(case, inp, device='cuda'):
    """-> (got, complaints of the guards): the call with dlogits, then the call without"""
    _lib, L = _L()
    P, st = _lib.ptr, _lib.stream()
    B, C = case.B, case.C
    x = inp['x'].to(F32).to(device)
    lab = inp['label'].to(F32 if case.soft else torch.int64).contiguous().to(device)
    row, loss = _out((B,), device), _out((1,), device)
    d = Guarded((B, C), (C, 1), F32, device)
    _lib.check(L.saicv_softmax_ce_fwd(P(x), P(lab), int(case.soft), B, C, P(row.view), P(loss.view), P(d.view), st), 'softmax_ce_fwd')
    row0, loss0 = _out((B,), device), _out((1,), device)
    _lib.check(L.saicv_softmax_ce_fwd(P(x), P(lab), int(case.soft), B, C, P(row0.view), P(loss0.view), None, st), 'softmax_ce_fwd')
    return _finish([('row_loss', row), ('loss', loss), ('dlogits', d), ('row_loss_null', row0), ('loss_null', loss0)])


def run_scale(case, inp, device='cuda'):
    _lib, L = _L()
    x, s = inp['in'].to(F32).to(device), _scalar(inp['s'], device)
    o = Guarded((case.n,), (1,), TD[case.dt], device)
    _lib.check(L.saicv_scale_by_scalar(_lib.dtype_code(TD[case.dt]), _lib.ptr(x), _lib.ptr(s), _lib.ptr(o.view), case.n, _lib.stream()), 'scale_by_scalar')
    return _finish([('out', o)])


def run_stats(case, inp, device='cuda'):
    """flips saicv_set_deterministic to the case's mode and puts it back"""
    _lib, L = _L()
    x = inp['g'].to(F32).to(device)
    outs = []
    found = sumsq = None
    if case.which != 'sumsq':
        found = _filled(torch.tensor([case.found_prefill]), device=device)
        outs.append(('found_inf', found))
    if case.which != 'found':
        sumsq = _filled(torch.tensor([SUMSQ_PREFILL]), device=device)
        outs.append(('sumsq', sumsq))
    prev = L.saicv_set_deterministic(int(case.det))
    try:
        _lib.check(L.saicv_grad_stats(_lib.ptr(x), case.n, _lib.ptr(found.view) if found else None, _lib.ptr(sumsq.view) if sumsq else None,
                                      _lib.stream()), 'grad_stats')
        return _finish(outs)
    finally:
        L.saicv_set_deterministic(prev)


def run_clip_scale(case, inp, device='cuda'):
    _lib, L = _L()
    g = _filled(inp['g'], device=device)
    sumsq, inv = _scalar(inp['sumsq'], device), _scalar(inp['inv'], device)
    _lib.check(L.saicv_grad_clip_scale(_lib.ptr(g.view), case.n, _lib.ptr(sumsq), _lib.ptr(inv), float(inp['max_norm']), _lib.stream()), 'grad_clip_scale')
    return _finish([('g', g)])


def run_clip_value(case, inp, device='cuda'):
    _lib, L = _L()
    g = _filled(inp['g'], device=device)
    inv = _scalar(inp['inv'], device)
    _lib.check(L.saicv_grad_clip_value(_lib.ptr(g.view), case.n, _lib.ptr(inv), float(case.value), _lib.stream()), 'grad_clip_value')
    return _finish([('g', g)])


def run_scaler(case, inp, device='cuda'):
    _lib, L = _L()
    state = _filled(inp['state'], device=device)
    found = _scalar(inp['found'], device)
    _lib.check(L.saicv_scaler_update(_lib.ptr(state.view), _lib.ptr(found), case.growth, case.backoff, case.interval, _lib.stream()), 'scaler_update')
    return _finish([('state', state)])


RUNNERS = {'ce': run_ce, 'scale': run_scale, 'stats': run_stats, 'clip_scale': run_clip_scale, 'clip_value': run_clip_value, 'scaler': run_scaler}


def opt_device_stepper(case, inp, guards, device='cuda'):
    """-> stepper(state, g) for opt_check: one launch of saicv_sgd_flat / saicv_adamw_flat on guarded arenas holding `state`; the guards'
    complaints are appended to `guards` after every launch"""
    _lib, L = _L()
    P, st = _lib.ptr, _lib.stream()
    n = case.blocks * BLOCK
    bg = inp['bg'].to(device)
    hyper = opt_hyper_table(case).reshape(-1).to(device)
    hg = None if inp['hg'] is None else inp['hg'].to(device)
    inv, found = _scalar(inp['inv'], device), _scalar(inp['found'], device)

    def stepper(state, g):
        arenas = {k: _filled(state[k], device=device) for k in state}
        gd = g.to(F32).to(device)
        if case.kind == 'sgd':
            rc = L.saicv_sgd_flat(P(arenas['p'].view), P(gd), P(arenas['m'].view), P(bg), P(hyper), P(inv), P(found), P(hg), n, st)
        else:
            rc = L.saicv_adamw_flat(P(arenas['p'].view), P(gd), P(arenas['m'].view), P(arenas['v'].view), P(bg), P(hyper), P(inv), P(found), P(hg),
                                    P(arenas['step'].view), n, st)
        _lib.check(rc, f'{case.kind}_flat')
        got, bad = _finish(list(arenas.items()))
        guards.extend(bad)
        return got

    return stepper
