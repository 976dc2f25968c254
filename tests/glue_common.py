"""What tests/test_glue_judge_host.py (no GPU) and tests/test_gpu_glue_f64.py (MI355X) share for the streaming kernels of
csrc/elemwise.hip and the stand-alone pooling kernels of csrc/pool.hip: the case tables of saicv_act_fwd / _bwd, saicv_mul_fwd / _bwd,
saicv_channel_scale_add_fwd / _bwd, saicv_bn_stats, saicv_rope_apply, saicv_swiglu_fwd / _bwd, saicv_resize_bilinear_add_fwd / _bwd,
saicv_maxpool_fwd / _bwd and saicv_avgpool_fwd / _bwd, the input builders, the float64 references with hand-written gradients and planted
faults, the working-precision emulations that set the constants, the judge, and the launchers (C-ABI, outputs in guarded allocations).

Two regimes, as in detloss_common.
  exact     inputs on which fp32 (and bf16 where the tensor is bf16) holds every intermediate exactly: small integers and dyadic scales,
            dyadic RoPE tables with independent halves, resize ratios x2, x4, /2 and 1, pooled sums of dyadic values over a power of two.
            Compared with torch.equal, nothing left out; a bf16 output is compared with the float64 reference rounded once to bf16.
  accuracy  random inputs; an element passes when |got - ref| <= allowed * u * bound (+ half a bf16 unit in the last place at |ref|, between
            2^-9 |ref| and 2^-8 |ref|, for the one rounding of a stored bf16 value: a flat 2^-9 |ref| is less than a correct rounding to
            8 significant bits may cost just above a power of two), u = 2^-24, bound the magnitude sum of the element's own expression
            in float64.  `allowed` is derived (FIXED) where the kernel is a short chain of correctly rounded operations and
            MARGIN * CONSTANTS[quantity] otherwise: the worst ratio of a CPU fp32 emulation of the kernel's arithmetic over the whole
            case table, which the host test measures and holds.

Bounds.   SiLU x s(x): |x| s (1 + |x|); its derivative s (1 + x (1 - s)): s (1 + |x| (1 - s)) (1 + |x|).  The factor (1 + |x|) is the
rounding of the exponent's argument -log2(e) x, an absolute error of u |x| log2(e) that becomes a relative one of the exponential.  Where
the sigmoid falls below 2^-126 the hardware may return zero: SiLU-family values and derivatives get the absolute floor |x| 2^-126 (times
|x2| or |dy| as the expression has it), derived, so that flushing and not flushing both pass.  Resize: (1 + src_y + src_x) * sum of |the
four taps| (+ |lateral|), the taps unweighted: a weight is src - int(src) and carries the absolute error u src of the fp32 source position;
the gradient likewise sums (1 + src_y + src_x) |dout| over every destination pixel one of whose taps is the source pixel.  Sums: the sum of
the magnitudes plus the pre-fill.

One listed fault has no observable value: `scale_in_float64` of the resize (the ratio in / out not rounded to fp32).  On the exact
geometries the ratio is dyadic and nothing changes at all; elsewhere the source position moves by at most u src, which is the very error
the bound grants every tap.  It is kept in NEUTRAL_FAULTS and the host test asserts both halves of that sentence.
"""
import math
from dataclasses import dataclass

import numpy as np
import torch

from attn_common import GUARD, MARGIN, SENTINEL, U, Guarded
from detloss_common import ORDER_SEEDS, fold_partials

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
TD = {'f32': F32, 'bf16': BF16}
DTYPES = ('f32', 'bf16')
EPC = {'f32': 4, 'bf16': 8}                                 # elements of a 16-byte chunk
UF, UB = U[F32], U[BF16]
EW_THREADS, EW_CAP, POOL_CAP = 256, 2048, 4096
TINY = 2.0 ** -126
LEFT_OUT_CAP = 0.005                                        # no case of these tables leaves an element out (the host test asserts it)
LOG2E32 = np.float32(1.4426950408889634)
SUM_PREFILL = 3.0

# Worst ratio of the fp32 emulations to the float64 references over every accuracy case of the tables, in units of u * bound.
# Measured by tests/test_glue_judge_host.py::test_constants_table_is_what_the_emulations_measure (which fails if a row drifts by more
# than a quarter, on one thread); the judge allows MARGIN times these.  Never raised by hand.
CONSTANTS = {
    'silu_val': 2.62, 'silu_der': 4.14, 'swiglu_out': 3.27, 'swiglu_dx1': 4.39, 'swiglu_dx2': 3.25, 'resize_fwd': 1.14, 'resize_bwd': 0.662,
    'avgpool_sum': 28.9, 'bn_sum': 4.52, 'bn_sq': 21.1, 'ds_sum': 1.30,
}
CONSTANTS_MEASURED_WITH = 'torch 2.10.0+rocm7.0 (CPU, one thread), 2026-10-19'
# derived: one correctly rounded product is within u |ref|; two correctly rounded operations on magnitudes p and q (p the product that
# is rounded first) are within u p + u (p + q) (1 + u) <= 2 u (p + q) (1 + u), fused or not; 2^-20 absorbs the second-order term
FIXED = {'prod': 1.0, 'chain2': 2.0 * (1.0 + 2.0 ** -20)}


def ew_grid(items):
    """ew_grid() of csrc/elemwise.hip restated"""
    return int(min(max((items + EW_THREADS - 1) // EW_THREADS, 1), EW_CAP))


def ew_trips(items):
    """trips of the longest-running thread through a grid-stride loop of elemwise.hip"""
    return -(-items // (ew_grid(items) * EW_THREADS))


def sgrid(total):
    """sgrid() of csrc/pool.hip restated"""
    return int(min(max((total + 255) // 256, 1), POOL_CAP))


def pool_trips(total):
    return -(-total // (sgrid(total) * 256))


def col_geom(M, cpr):
    """col_geom() of csrc/elemwise.hip restated -> (cw, column groups, row ranges, rows per range)"""
    cw = 1
    while cw * 2 <= cpr and cw * 2 <= 64:
        cw *= 2
    groups = (cpr + cw - 1) // cw
    ranges = min((2048 + groups - 1) // groups, 1024)
    rpb = max((M + ranges - 1) // ranges, 64)
    return cw, groups, (M + rpb - 1) // rpb, rpb


def rdt(x, dt):
    """one rounding to the dtype `dt` ('f32' | 'bf16'), kept as float64"""
    return x.to(TD[dt]).to(F64)


def r32(x):
    return x.to(F32).to(F64)


def _gen(name):
    return torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31))


def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi, shape, generator=g).to(F64)


def _randn(g, shape, scale=1.0):
    return torch.randn(shape, generator=g, dtype=F64) * scale


def _fma32(a, b, c):
    """fp32 fma(a, b, c) of float32 tensors: the product is exact in float64, the sum rounded there and once more to fp32"""
    return (a.to(F64) * b.to(F64) + c.to(F64)).to(F32)


# ------------------------------------------------------------------------------------------------ the judge
def judge(got, spec, worst=None):
    """spec: {name: ('equal', ref) | ('bound', ref, bound, quantity, extra) | ('fixed', ref, bound, key, extra)} -> list of complaints.
    'equal' is torch.equal with NaN equal to NaN; for 'bound' / 'fixed' the error beyond the absolute allowance `extra` (None: none) is
    held to allowed * u * bound, an element whose bound is 0 must be exact and a NaN never passes.  worst: receives the worst ratios."""
    bad = []
    for name, (kind, ref, *rest) in spec.items():
        g = got[name].detach().to(F64).cpu().reshape(ref.shape)
        if kind == 'equal':
            differ = (g != ref) & ~(torch.isnan(g) & torch.isnan(ref))
            if bool(differ.any()):
                bad.append(f'{name}: {int(differ.sum())} of {ref.numel()} elements differ (exact comparison)')
            continue
        bnd, q, extra = rest
        b = bnd.abs() * UF
        err = (g - ref).abs()
        if extra is not None:
            err = (err - extra).clamp_min(0.0)
        ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
        ratio = torch.where(torch.isnan(g) | torch.isnan(err), torch.full_like(ratio, math.inf), ratio)
        r = float(ratio.max()) if ratio.numel() else 0.0
        if worst is not None:
            worst[q] = max(worst.get(q, 0.0), r)
        allowed = allowed_ratio(q)
        if not r <= allowed:
            bad.append(f'{name}: worst ratio {r:.4g} u*bound > {allowed:.4g} ({q}), {int((ratio > allowed).sum())} elements')
    return bad


def allowed_ratio(q):
    return FIXED[q] if q in FIXED else MARGIN * CONSTANTS[q]


def values(spec):
    """the reference values of a spec as a `got` dict (a planted fault's candidate)"""
    return {n: s[1] for n, s in spec.items()}


def bf16_half_ulp(ref):
    """the one rounding of a stored bf16 value: half a unit in the last of bf16's 8 significant bits at |ref|, 2^(floor(log2 |ref|) - 8),
    between 2^-9 |ref| and 2^-8 |ref| (0 at 0)"""
    _, e = torch.frexp(ref.abs())
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.ones_like(ref), e - 9))


def _entry(ref, dt, exact, bound=None, q=None, floor=None):
    """one spec entry for an output stored in the dtype dt"""
    if exact:
        return ('equal', rdt(ref, dt))
    extra = floor
    if dt == 'bf16':
        extra = bf16_half_ulp(ref) + (0.0 if floor is None else floor)
    return ('fixed' if q in FIXED else 'bound', ref, bound, q, extra)


def _lose(spec, lost):
    """the entries of a spec with the elements `lost` (bool, flat or shaped) never written"""
    out = {}
    for n, (kind, ref, *rest) in spec.items():
        out[n] = (kind, torch.where(lost.reshape(ref.shape), torch.full_like(ref, math.nan), ref), *rest)
    return out


# ================================================================================================ streaming kernels
STREAM_FAULTS = ('tail_beyond_grid_dropped', 'scale_index_not_wrapped', 'relu_grad_one_at_zero', 'leaky_slope_on_positive',
                 'silu_derivative_without_x_term', 'swiglu_gradients_swapped')
SILU_PLANTED = (-120.0, -100.0, -88.0, -87.0, -20.0, -1e-3, 0.0, 1e-3, 20.0, 88.0, 100.0, 120.0)
LEAKY_SLOPE = 0.125
ACT_KIND = {'relu': 0, 'leaky': 1, 'silu': 2}
BIG_CHUNKS = EW_CAP * EW_THREADS + 257


@dataclass(frozen=True)
class StreamCase:
    id: str
    op: str                     # relu | leaky | silu | swiglu | mul | scale_add
    dt: str
    chunks: int
    cpr: int = 1                # chunks per row (scale_add)
    variant: str = 'full'       # mul: both | da_null | db_null; scale_add: full | x_null | s_null
    exact: bool = True

    @property
    def n(self):
        return self.chunks * EPC[self.dt]


def _stream_table():
    c = []
    sizes = (1, 255, 256, 257, BIG_CHUNKS)
    for dt in DTYPES:
        for op in ('relu', 'leaky', 'silu', 'swiglu'):
            ex = op in ('relu', 'leaky')
            c += [StreamCase(f'{op}-{dt}-ch{ch}', op, dt, ch, exact=ex) for ch in sizes]
        for i, ch in enumerate(sizes):
            v = ('both', 'da_null', 'db_null', 'both', 'both')[i]
            c.append(StreamCase(f'mul-{dt}-ch{ch}-{v}-exact', 'mul', dt, ch, variant=v))
        c += [StreamCase(f'mul-{dt}-ch257-da_null-exact', 'mul', dt, 257, variant='da_null'),
              StreamCase(f'mul-{dt}-ch255-db_null-exact', 'mul', dt, 255, variant='db_null'),
              StreamCase(f'mul-{dt}-ch1-both-random', 'mul', dt, 1, variant='both', exact=False),
              StreamCase(f'mul-{dt}-ch257-both-random', 'mul', dt, 257, variant='both', exact=False),
              StreamCase(f'mul-{dt}-ch{BIG_CHUNKS}-both-random', 'mul', dt, BIG_CHUNKS, variant='both', exact=False)]
        geoms = [(1, 1), (1, 255), (1, 256), (1, 257), (1, BIG_CHUNKS), (65, 1), (65, 4), (65, 8071)]
        for i, (cpr, M) in enumerate(geoms):
            v = ('full', 'x_null', 's_null')[i % 3]
            c.append(StreamCase(f'scale_add-{dt}-cpr{cpr}-m{M}-{v}-exact', 'scale_add', dt, cpr * M, cpr=cpr, variant=v))
        for cpr, M, v in ((65, 4, 'x_null'), (65, 4, 's_null'), (1, 257, 'full'), (65, 8071, 'x_null')):
            c.append(StreamCase(f'scale_add-{dt}-cpr{cpr}-m{M}-{v}-exact2', 'scale_add', dt, cpr * M, cpr=cpr, variant=v))
        for cpr, M, v in ((1, 257, 'full'), (65, 4, 'full'), (65, 4, 'x_null'), (65, 8071, 'full'), (1, 256, 's_null')):
            c.append(StreamCase(f'scale_add-{dt}-cpr{cpr}-m{M}-{v}-random', 'scale_add', dt, cpr * M, cpr=cpr, variant=v, exact=False))
    return tuple(c)


STREAM_CASES = _stream_table()


def stream_inputs(case):
    g = _gen(case.id)
    n, dt, op = case.n, case.dt, case.op
    if op in ('relu', 'leaky', 'silu', 'swiglu'):
        if case.exact:
            x = _randint(g, -8, 9, (n,))
            x[::7] = 0.0                                    # exact zeros, the first element among them
            dy = _randint(g, -8, 9, (n,))
            dy[dy == 0] = 3.0
        else:
            x = _randn(g, (n,), 3.0)
            k = min(n, len(SILU_PLANTED))
            x[:k] = torch.tensor(SILU_PLANTED[:k], dtype=F64)
            x, dy = rdt(x, dt), rdt(_randn(g, (n,)), dt)
            dy[:k] = rdt(torch.tensor([1.5, -0.75] * 6, dtype=F64)[:k], dt)
        inp = {'x': x, 'dy': dy}
        if op == 'swiglu':
            x2 = rdt(_randn(g, (n,), 2.0), dt)
            x2[:min(n, 12)] = rdt(torch.tensor([1.25, -2.5] * 6, dtype=F64)[:min(n, 12)], dt)
            inp['x2'] = x2
        return inp
    if op == 'mul':
        if case.exact:
            return {'a': _randint(g, -8, 9, (n,)), 'b': _randint(g, -16, 17, (n,)) / 4, 'dy': _randint(g, -4, 5, (n,))}
        return {'a': rdt(_randn(g, (n,)), dt), 'b': rdt(_randn(g, (n,)), dt), 'dy': rdt(_randn(g, (n,)), dt)}
    C = case.cpr * EPC[dt]
    M = case.chunks // case.cpr
    if case.exact:
        return {'x': _randint(g, -8, 9, (M, C)), 'y': _randint(g, -8, 9, (M, C)), 's': _randint(g, -8, 9, (C,)) / 4}
    return {'x': rdt(_randn(g, (M, C)), dt), 'y': rdt(_randn(g, (M, C)), dt), 's': r32(_randn(g, (C,)))}


def silu_math(x):
    """float64 -> (value, derivative, value bound, derivative bound) of x * sigmoid(x), hand-written"""
    s = torch.sigmoid(x)
    ax = x.abs()
    return x * s, s * (1 + x * (1 - s)), ax * s * (1 + ax), s * (1 + ax * (1 - s)) * (1 + ax)


def act_math(op, x, fault=None):
    """-> (value, derivative) of relu / leaky in float64"""
    zero, one = torch.zeros_like(x), torch.ones_like(x)
    pos = (x >= 0) if fault == 'relu_grad_one_at_zero' and op == 'relu' else (x > 0)
    if op == 'relu':
        return torch.where(x > 0, x, zero), torch.where(pos, one, zero)
    if fault == 'leaky_slope_on_positive':
        return x * LEAKY_SLOPE, torch.full_like(x, LEAKY_SLOPE)
    return torch.where(x > 0, x, x * LEAKY_SLOPE), torch.where(x > 0, one, LEAKY_SLOPE * one)


def stream_reference(case, inp, fault=None):
    dt, op, ex = case.dt, case.op, case.exact
    if op in ('relu', 'leaky'):
        v, d = act_math(op, inp['x'], fault)
        spec = {'y': _entry(v, dt, True), 'dx': _entry(inp['dy'] * d, dt, True)}
    elif op == 'silu':
        x, dy = inp['x'], inp['dy']
        v, d, bv, bd = silu_math(x)
        if fault == 'silu_derivative_without_x_term':
            d = torch.sigmoid(x)
        spec = {'y': _entry(v, dt, False, bv, 'silu_val', x.abs() * TINY),
                'dx': _entry(dy * d, dt, False, dy.abs() * bd, 'silu_der', (x * dy).abs() * TINY)}
    elif op == 'swiglu':
        x, x2, dy = inp['x'], inp['x2'], inp['dy']
        v, d, bv, bd = silu_math(x)
        d1, d2 = dy * x2 * d, dy * v
        b1, b2 = (dy * x2).abs() * bd, dy.abs() * bv
        f1, f2 = (x * dy * x2).abs() * TINY, (x * dy).abs() * TINY
        if fault == 'swiglu_gradients_swapped':
            d1, d2 = d2, d1
        spec = {'out': _entry(v * x2, dt, False, bv * x2.abs(), 'swiglu_out', (x * x2).abs() * TINY),
                'dx1': _entry(d1, dt, False, b1, 'swiglu_dx1', f1), 'dx2': _entry(d2, dt, False, b2, 'swiglu_dx2', f2)}
    elif op == 'mul':
        a, b, dy = inp['a'], inp['b'], inp['dy']
        spec = {'out': _entry(a * b, dt, ex, (a * b).abs(), 'prod')}
        if case.variant != 'da_null':
            spec['da'] = _entry(dy * b, dt, ex, (dy * b).abs(), 'prod')
        if case.variant != 'db_null':
            spec['db'] = _entry(dy * a, dt, ex, (dy * a).abs(), 'prod')
    else:
        x, y, s = inp['x'], inp['y'], inp['s']
        M, C = y.shape
        if fault == 'scale_index_not_wrapped':              # the chunk's own index instead of index % chunks-per-row, held inside s
            e = EPC[dt]
            chunk = torch.arange(M * case.cpr).clamp_max(case.cpr - 1)
            s = s[(chunk[:, None] * e + torch.arange(e)[None, :]).reshape(M, C)]
        sy = y if case.variant == 's_null' else s * y
        ref = sy if case.variant == 'x_null' else x + sy
        bnd = sy.abs() if case.variant == 'x_null' else x.abs() + sy.abs()
        spec = {'out': _entry(ref, dt, ex, bnd, 'chain2')}
    if fault == 'tail_beyond_grid_dropped':
        lost = torch.arange(case.n) >= EW_CAP * EW_THREADS * EPC[dt]
        spec = _lose(spec, lost)
    return spec


def _sigmoid32(x):
    """the sigmoid of act_val / act_der in fp32: 1 / (1 + exp2(-log2e * x))"""
    return 1.0 / (1.0 + torch.exp2(torch.tensor(-LOG2E32) * x))


def stream_emulate(case, inp):
    """the kernel's arithmetic in fp32 on the CPU, the stored value rounded to the case's dtype (accuracy cases)"""
    dt, op = case.dt, case.op
    f = {k: v.to(F32) for k, v in inp.items()}
    one = torch.ones((), dtype=F32)
    if op in ('silu', 'swiglu'):
        x = f['x']
        s = _sigmoid32(x)
        val, der = x * s, s * _fma32(x, one - s, one)
        if op == 'silu':
            got = {'y': val, 'dx': f['dy'] * der}
        else:
            got = {'out': val * f['x2'], 'dx1': f['dy'] * f['x2'] * der, 'dx2': f['dy'] * val}
    elif op == 'mul':
        got = {'out': f['a'] * f['b'], 'da': f['dy'] * f['b'], 'db': f['dy'] * f['a']}
        got = {k: v for k, v in got.items() if k != {'da_null': 'da', 'db_null': 'db'}.get(case.variant)}
    elif op == 'scale_add':
        sy = f['y'] if case.variant == 's_null' else f['y'] * f['s']
        got = {'out': sy if case.variant == 'x_null' else f['x'] + sy}
    else:
        v, d = act_math(op, inp['x'])
        got = {'y': v, 'dx': inp['dy'] * d}
    return {k: rdt(v.to(F64), dt) for k, v in got.items()}


# ================================================================================================ column reductions
COLRED_FAULTS = ('last_row_range_dropped', 'second_column_group_dropped', 'assign_not_add')


@dataclass(frozen=True)
class ColCase:
    id: str
    op: str                     # bn_stats | scale_bwd
    dt: str
    M: int
    cpr: int
    variant: str = 'both'       # scale_bwd: both | dy_only | ds_only | s_null
    exact: bool = True

    @property
    def C(self):
        return self.cpr * EPC[self.dt]


def _col_table():
    c = []
    geoms = [(cpr, M) for cpr in (1, 2, 63, 64, 65) for M in (1, 3, 64, 65)] + [(1, 65537)]
    variants = ('both', 'dy_only', 'ds_only', 's_null')
    for dt in DTYPES:
        for i, (cpr, M) in enumerate(geoms):
            c.append(ColCase(f'bn_stats-{dt}-cpr{cpr}-m{M}-exact', 'bn_stats', dt, M, cpr))
            v = variants[(i + i // 4) % 4]
            c.append(ColCase(f'scale_bwd-{dt}-cpr{cpr}-m{M}-{v}-exact', 'scale_bwd', dt, M, cpr, v))
        for v in variants[1:]:
            c.append(ColCase(f'scale_bwd-{dt}-cpr65-m65-{v}-exact2', 'scale_bwd', dt, 65, 65, v))
            c.append(ColCase(f'scale_bwd-{dt}-cpr1-m65537-{v}-exact2', 'scale_bwd', dt, 65537, 1, v))
        for cpr, M in ((63, 3), (63, 65), (65, 65), (2, 64), (1, 65537)):
            c.append(ColCase(f'bn_stats-{dt}-cpr{cpr}-m{M}-random', 'bn_stats', dt, M, cpr, exact=False))
            c.append(ColCase(f'scale_bwd-{dt}-cpr{cpr}-m{M}-both-random', 'scale_bwd', dt, M, cpr, 'both', exact=False))
    return tuple(c)


COL_CASES = _col_table()


def col_prefill(C, which=0):
    """the known integers an accumulating destination holds before the launch"""
    return SUM_PREFILL + ((torch.arange(C) + which) % 5).to(F64)


def col_inputs(case):
    g = _gen(case.id)
    M, C, dt = case.M, case.C, case.dt
    if case.exact:
        a, b, s = _randint(g, -8, 9, (M, C)), _randint(g, -8, 9, (M, C)), _randint(g, -8, 9, (C,)) / 4
    else:
        a, b, s = rdt(_randn(g, (M, C)) + 0.25, dt), rdt(_randn(g, (M, C)), dt), r32(_randn(g, (C,)))
    if case.op == 'bn_stats':
        return {'x': a}
    return {'dout': a, 'y': b, 's': s}


def _col_lost(case, fault):
    """-> (rows lost, columns lost) under a fault, as bool vectors"""
    cw, groups, ranges, rpb = col_geom(case.M, case.cpr)
    rows, cols = torch.zeros(case.M, dtype=torch.bool), torch.zeros(case.C, dtype=torch.bool)
    if fault == 'last_row_range_dropped' and ranges > 1:
        rows[(ranges - 1) * rpb:] = True
    if fault == 'second_column_group_dropped' and groups > 1:
        cols[cw * EPC[case.dt]:2 * cw * EPC[case.dt]] = True
    return rows, cols


def col_reference(case, inp, fault=None):
    M, C, dt, ex = case.M, case.C, case.dt, case.exact
    rows, cols = _col_lost(case, fault)
    keep = (~rows)[:, None] & (~cols)[None, :]
    pre = 0.0 if fault == 'assign_not_add' else 1.0

    def total(terms, which, q):
        ref = torch.where(keep, terms, torch.zeros_like(terms)).sum(0) + pre * col_prefill(C, which)
        if ex:
            return ('equal', ref)
        return ('bound', ref, terms.abs().sum(0) + col_prefill(C, which), q, None)

    if case.op == 'bn_stats':
        x = inp['x']
        return {'sum': total(x, 0, 'bn_sum'), 'sq': total(x * x, 1, 'bn_sq')}
    dout, y, s = inp['dout'], inp['y'], inp['s']
    spec = {}
    if case.variant != 'ds_only':
        dy = dout if case.variant == 's_null' else s * dout
        spec['dy'] = _entry(torch.where(keep, dy, torch.full_like(dy, math.nan)), dt, ex, dy.abs(), 'prod')
    if case.variant != 'dy_only':
        spec['ds'] = total(dout * y, 0, 'ds_sum')
    return spec


def colred_partials(p, q, M, cpr, fma):
    """fp32 partial sums of colred_kernel, one row per row range: a lane adds its rows m0 + rl, m0 + rl + nrl, ... one after the other
    (p alone, or fma(p, q, acc)), then lane 0 adds the row lanes' partials in order.  p, q: float32 torch [M, C]"""
    cw, _, ranges, rpb = col_geom(M, cpr)
    nrl = EW_THREADS // cw
    C = p.shape[1]
    steps = -(-rpb // nrl)

    def lay(t):
        pad = torch.zeros((ranges * rpb, C), dtype=F32)
        pad[:M] = t
        blk = torch.zeros((ranges, steps * nrl, C), dtype=F32)
        blk[:, :rpb] = pad.view(ranges, rpb, C)
        return blk.view(ranges, steps, nrl, C)

    P, Q = lay(p), (lay(q) if q is not None else None)
    acc = torch.zeros((ranges, nrl, C), dtype=F32)
    for k in range(steps):
        if Q is None:
            acc = acc + P[:, k]
        elif fma:
            acc = _fma32(P[:, k], Q[:, k], acc)
        else:
            acc = acc + P[:, k] * Q[:, k]
    t = torch.zeros((ranges, C), dtype=F32)
    for l in range(nrl):
        t = t + acc[:, l]
    return t.numpy()


def col_emulate(case, inp, seed=None, parts=None):
    """-> (got, parts): the sums folded in the order `seed` (None: the deterministic fold; else a seeded random arrival order of the
    atomic form), dy in fp32.  parts: the partials of an earlier call, to fold them again."""
    M, C, dt = case.M, case.C, case.dt
    f = {k: v.to(F32) for k, v in inp.items()}
    if parts is None:
        if case.op == 'bn_stats':
            parts = {'sum': (colred_partials(f['x'], None, M, case.cpr, False), 0), 'sq': (colred_partials(f['x'], f['x'], M, case.cpr, True), 1)}
        else:
            parts = {} if case.variant == 'dy_only' else {'ds': (colred_partials(f['dout'], f['y'], M, case.cpr, True), 0)}
    got = {}
    for name, (pt, which) in parts.items():
        pre = col_prefill(C, which).numpy()
        got[name] = torch.tensor([fold_partials(pt[:, c], pre[c], seed) for c in range(C)], dtype=F64)
    if case.op == 'scale_bwd' and case.variant != 'ds_only':
        dy = f['dout'] if case.variant == 's_null' else f['dout'] * f['s']
        got['dy'] = rdt(dy.to(F64), dt)
    return got, parts


# ================================================================================================ RoPE
ROPE_FAULTS = ('sin_halves_shared', 'cos_halves_shared', 'prefix_rotated', 'v_rotated', 'transpose_sign')


@dataclass(frozen=True)
class RopeCase:
    id: str
    dt: str
    D: int
    heads: int
    B: int
    N: int
    prefix: int
    transpose: int
    exact: bool = True

    @property
    def items(self):
        return self.B * self.N * 3 * self.heads * (self.D // 2 // EPC[self.dt])


def _rope_table():
    c = []
    for dt in DTYPES:
        dims = (2 * EPC[dt], 32, 64, 96)
        i = 0
        for D in dims:
            for prefix in (0, 1, 5, 7):
                for tr in (0, 1):
                    heads, B = (1, 3)[(i // 2 + i) % 2], (1, 2)[(i // 4 + i // 2) % 2]
                    c.append(RopeCase(f'{dt}-d{D}-h{heads}-b{B}-n7-p{prefix}-t{tr}-exact', dt, D, heads, B, 7, prefix, tr))
                    i += 1
        for j, D in enumerate(dims):
            for tr in (0, 1):
                c.append(RopeCase(f'{dt}-d{D}-h{(3, 1)[j % 2]}-b2-n9-p1-t{tr}-random', dt, D, (3, 1)[j % 2], 2, 9, 1, tr, exact=False))
        rows = -(-(EW_CAP * EW_THREADS + 257) // (3 * 3 * (64 // 2 // EPC[dt])))
        for tr in (0, 1):
            c.append(RopeCase(f'{dt}-d64-h3-b2-n{-(-rows // 2)}-p1-t{tr}-exact-big', dt, 64, 3, 2, -(-rows // 2), 1, tr))
    return tuple(c)


ROPE_CASES = _rope_table()


def rope_inputs(case):
    """qkv [B, N, 3, heads, D]; sin, cos [N - prefix, D] fp32 with INDEPENDENT lower and upper halves"""
    g = _gen(case.id)
    n = case.N - case.prefix
    shape = (case.B, case.N, 3, case.heads, case.D)
    if case.exact:
        return {'qkv': _randint(g, -16, 17, shape), 'sin': _randint(g, -8, 9, (n, case.D)) / 8, 'cos': _randint(g, -8, 9, (n, case.D)) / 8}
    ang = torch.rand((n, case.D), generator=g, dtype=F64) * 2 * math.pi
    ang2 = torch.rand((n, case.D), generator=g, dtype=F64) * 2 * math.pi
    return {'qkv': rdt(_randn(g, shape), case.dt), 'sin': r32(torch.sin(ang)), 'cos': r32(torch.cos(ang2))}


def rope_math(x, sin, cos, prefix, transpose, fault=None, bounds=False):
    """x [B, N, 3, heads, D] float64 -> rotated copy (and the magnitude sums): y = x cos + rot(x) sin on the q and k thirds of the
    tokens n >= prefix, rot(x) = [-x2, x1]; transpose: dx = g cos + rot^T(g sin), rot^T(u) = [u2, -u1]"""
    B, N, _, heads, D = x.shape
    half = D // 2
    out, bnd = x.clone(), torch.zeros_like(x)
    parts = 3 if fault == 'v_rotated' else 2
    if fault == 'prefix_rotated' and prefix and sin.shape[0]:      # the prefix tokens rotated with the first table row
        sin = torch.cat([sin[:1].expand(prefix, D), sin], 0)
        cos = torch.cat([cos[:1].expand(prefix, D), cos], 0)
        prefix = 0
    if sin.shape[0] == 0:
        return (out, bnd) if bounds else out
    rot = x[:, prefix:, :parts]
    a, b = rot[..., :half], rot[..., half:]
    sh = lambda t: t[None, :, None, None, :]      # noqa: E731
    s1, s2, c1, c2 = sh(sin[:, :half]), sh(sin[:, half:]), sh(cos[:, :half]), sh(cos[:, half:])
    if fault == 'sin_halves_shared':
        s2 = s1
    if fault == 'cos_halves_shared':
        c2 = c1
    if transpose and fault != 'transpose_sign':
        o1, o2 = a * c1 + b * s2, b * c2 - a * s1
        b1, b2 = (a * c1).abs() + (b * s2).abs(), (b * c2).abs() + (a * s1).abs()
    elif transpose:                                           # the forward's signs on the transposed taps
        o1, o2 = a * c1 - b * s2, b * c2 + a * s1
        b1, b2 = (a * c1).abs() + (b * s2).abs(), (b * c2).abs() + (a * s1).abs()
    else:
        o1, o2 = a * c1 - b * s1, b * c2 + a * s2
        b1, b2 = (a * c1).abs() + (b * s1).abs(), (b * c2).abs() + (a * s2).abs()
    out[:, prefix:, :parts] = torch.cat([o1, o2], -1)
    bnd[:, prefix:, :parts] = torch.cat([b1, b2], -1)
    return (out, bnd) if bounds else out


def rope_reference(case, inp, fault=None):
    out = rope_math(inp['qkv'], inp['sin'], inp['cos'], case.prefix, case.transpose, fault)
    _, bnd = rope_math(inp['qkv'], inp['sin'], inp['cos'], case.prefix, case.transpose, bounds=True)
    if case.exact:
        return {'out': ('equal', rdt(out, case.dt))}
    # copied elements (v, the prefix) have bound 0: they must be the same bits
    return {'out': _entry(out, case.dt, False, bnd, 'chain2')}


def rope_copied(case):
    """bool [B, N, 3, heads, D]: the elements that are copied, not rotated"""
    m = torch.ones((case.B, case.N, 3, case.heads, case.D), dtype=torch.bool)
    m[:, case.prefix:, :2] = False
    return m


def rope_emulate(case, inp):
    """fp32 products and sum, unfused, rounded to the dtype; copies stay copies"""
    x, s, c = inp['qkv'].to(F32), inp['sin'].to(F32), inp['cos'].to(F32)
    out = rope_math(x, s, c, case.prefix, case.transpose)
    return {'out': rdt(out.to(F64), case.dt)}


def rope_edge_cases():
    """the exact-regime cases oracle/make_golden_glue_edges.py runs the reference project's rope_apply / apply_rope on"""
    return tuple(c for c in ROPE_CASES if c.exact and c.dt == 'f32' and c.D == 8 and not c.transpose)


# ================================================================================================ bilinear resize
RESIZE_FAULTS = ('align_corners', 'no_low_clamp', 'edge_tap_dropped', 'bwd_window_one_short')
NEUTRAL_FAULTS = ('scale_in_float64',)
RESIZE_GEOMS = (((5, 7), (10, 14)), ((3, 4), (12, 16)), ((16, 12), (8, 6)), ((6, 6), (6, 6)), ((1, 3), (2, 6)), ((2, 1), (8, 4)),
                ((7, 10), (13, 19)), ((16, 16), (5, 7)), ((3, 5), (96, 160)), ((33, 17), (4, 3)), ((5, 5), (1, 1)))
RESIZE_EXACT_RATIOS = (0.25, 0.5, 1.0, 2.0)                # in / out of the exact regime: x4, x2, identity and /2


@dataclass(frozen=True)
class ResizeCase:
    id: str
    tt: str
    tl: str                     # 'f32' | 'bf16' | 'none' (lateral NULL)
    N: int
    C: int
    h: int
    w: int
    H: int
    W: int

    @property
    def exact(self):
        return (self.h / self.H) in RESIZE_EXACT_RATIOS and (self.w / self.W) in RESIZE_EXACT_RATIOS

    @property
    def fwd_items(self):
        return self.N * self.H * self.W * (self.C // 4)

    @property
    def bwd_items(self):
        return self.N * self.h * self.w * (self.C // 4)


def _resize_table():
    c = []
    combos = (('f32', 'f32'), ('bf16', 'bf16'), ('f32', 'bf16'), ('bf16', 'f32'), ('f32', 'none'), ('bf16', 'none'))
    for i, ((h, w), (H, W)) in enumerate(RESIZE_GEOMS):
        for j in range(3):                                  # every geometry in three of the six dtype forms, rotating
            tt, tl = combos[(i + 2 * j) % 6] if j else combos[i % 6]
            C, N = (4, 12)[(i + j) % 2], (1, 2)[(i + j // 2) % 2]
            cid = f'{tt}-{tl}-n{N}-c{C}-{h}x{w}-{H}x{W}'
            if all(k.id != cid for k in c):
                c.append(ResizeCase(cid, tt, tl, N, C, h, w, H, W))
    for tt, tl in combos[:4]:                               # the four TT x TL forms on one exact and one inexact geometry each
        for (h, w), (H, W) in (RESIZE_GEOMS[0], RESIZE_GEOMS[6]):
            cid = f'{tt}-{tl}-n2-c12-{h}x{w}-{H}x{W}'
            if all(k.id != cid for k in c):
                c.append(ResizeCase(cid, tt, tl, 2, 12, h, w, H, W))
    c += [ResizeCase(f'{tt}-{tl}-n1-c4-726x726-1452x1452-big', tt, tl, 1, 4, 726, 726, 1452, 1452) for tt, tl in combos[:2]]
    return tuple(c)


RESIZE_CASES = _resize_table()


def resize_inputs(case):
    """top [N, h, w, C], lateral [N, H, W, C] or None, dout [N, H, W, C] (fp32)"""
    g = _gen(case.id)
    N, C, h, w, H, W = case.N, case.C, case.h, case.w, case.H, case.W
    if case.exact:
        top, lat, dout = _randint(g, -64, 65, (N, h, w, C)), _randint(g, -64, 65, (N, H, W, C)), _randint(g, -8, 9, (N, H, W, C))
    else:
        top, lat, dout = rdt(_randn(g, (N, h, w, C)), case.tt), _randn(g, (N, H, W, C)), r32(_randn(g, (N, H, W, C)))
        lat = rdt(lat, case.tl) if case.tl != 'none' else lat
    return {'top': top, 'lat': None if case.tl == 'none' else lat, 'dout': dout}


def resize_taps(n_in, n_out, fault=None, wd=F64, fused=False):
    """the taps of one axis -> dict of [n_out] tensors i0, i1 (long), w0, w1, src (wd).  The positions follow the kernel's stated
    specification: scale = fp32(in) / fp32(out) rounded to fp32, src = max(scale * (d + 0.5) - 0.5, 0), i0 = int(src),
    i1 = i0 + (i0 < in - 1), weights (1 - frac, frac).  wd = F64: everything after the fp32 scale in float64 (the reference);
    wd = F32: the kernel's fp32 arithmetic, `fused` choosing the contracted form of src."""
    scale = float(np.float32(n_in) / np.float32(n_out))
    if fault == 'scale_in_float64':
        scale = n_in / n_out
    d = torch.arange(n_out, dtype=F64)
    if fault == 'align_corners':
        src = d * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
    elif wd == F64:
        src = scale * (d + 0.5) - 0.5
    elif fused:
        src = (scale * (d + 0.5) - 0.5).to(F32).to(F64)    # fma: one rounding (the product of two fp32 values is exact in float64)
    else:
        src = ((scale * (d + 0.5)).to(F32).to(F64) - 0.5).to(F32).to(F64)
    if fault != 'no_low_clamp':
        src = src.clamp_min(0.0)
    i0 = torch.trunc(src).to(torch.long)                    # int(): towards zero
    i1 = i0 + (i0 < n_in - 1).to(torch.long)
    w1 = src - i0.to(F64)
    if wd == F32:
        w1 = w1.to(F32).to(F64)
        w0 = (1.0 - w1).to(F32).to(F64)
    else:
        w0 = 1.0 - w1
    if fault == 'edge_tap_dropped':                         # i1 not clamped at the last source pixel: the tap beyond it reads nothing
        w1 = torch.where(i0 >= n_in - 1, torch.zeros_like(w1), w1)
    return {'i0': i0, 'i1': i1, 'w0': w0, 'w1': w1, 'src': src.clamp_min(0.0)}


def _interp_axis(x, dim, t, fac=None):
    """x gathered along `dim` by the taps t (optionally with a per-destination factor on the weights)"""
    shape = [1] * x.dim()
    shape[dim] = -1
    w0, w1 = (t['w0'], t['w1']) if fac is None else (t['w0'] * fac, t['w1'] * fac)
    return x.index_select(dim, t['i0']) * w0.view(shape).to(x.dtype) + x.index_select(dim, t['i1']) * w1.view(shape).to(x.dtype)


def _scatter_axis(g, dim, t, n_in, fac=None):
    """the transpose of _interp_axis"""
    shape = [1] * g.dim()
    shape[dim] = -1
    w0, w1 = (t['w0'], t['w1']) if fac is None else (t['w0'] * fac, t['w1'] * fac)
    size = list(g.shape)
    size[dim] = n_in
    out = torch.zeros(size, dtype=g.dtype)
    out.index_add_(dim, t['i0'], g * w0.view(shape).to(g.dtype))
    out.index_add_(dim, t['i1'], g * w1.view(shape).to(g.dtype))
    return out


def _one_short(t, n_in):
    """taps of the gather whose window ends one destination row early: every source row loses the last destination row that touches it"""
    w0, w1 = t['w0'].clone(), t['w1'].clone()
    for y in range(n_in):
        touch = ((t['i0'] == y) & (w0 != 0)) | ((t['i1'] == y) & (w1 != 0))
        if bool(touch.any()):
            d = int(touch.nonzero().max())
            if int(t['i0'][d]) == y:
                w0[d] = 0.0
            if int(t['i1'][d]) == y:
                w1[d] = 0.0
    return {**t, 'w0': w0, 'w1': w1}


def resize_reference(case, inp, fault=None):
    top, lat, dout = inp['top'], inp['lat'], inp['dout']
    tf = None if fault == 'bwd_window_one_short' else fault
    ty, tx = resize_taps(case.h, case.H, tf), resize_taps(case.w, case.W, tf)
    out = _interp_axis(_interp_axis(top, 1, ty), 2, tx)
    if lat is not None:
        out = out + lat
    by, bx = (_one_short(ty, case.h), tx) if fault == 'bwd_window_one_short' else (ty, tx)
    dtop = _scatter_axis(_scatter_axis(dout, 2, bx, case.w), 1, by, case.h)
    if case.exact:
        return {'out': ('equal', out), 'dtop': ('equal', rdt(dtop, case.tt))}
    # the bounds: every tap that is touched counts with its whole magnitude, whatever its weight -- a weight carries an ABSOLUTE error
    # of u * src, so a tap whose weight is (nearly) zero in float64 may get one of u * src in fp32 and the other way round
    ones = lambda t: {**t, 'w0': torch.ones_like(t['w0']), 'w1': torch.ones_like(t['w1'])}      # noqa: E731
    ny, nx = ones(resize_taps(case.h, case.H)), ones(resize_taps(case.w, case.W))
    a = top.abs()
    one_y = torch.ones(case.H, dtype=F64)
    bo = (_interp_axis(_interp_axis(a, 1, ny, one_y + ny['src']), 2, nx) + _interp_axis(_interp_axis(a, 1, ny), 2, nx, nx['src'])
          + (lat.abs() if lat is not None else 0.0))
    g = dout.abs()
    bd = (_scatter_axis(_scatter_axis(g, 2, nx, case.w), 1, ny, case.h, one_y + ny['src'])
          + _scatter_axis(_scatter_axis(g, 2, nx, case.w, nx['src']), 1, ny, case.h))
    return {'out': _entry(out, 'f32', False, bo, 'resize_fwd'), 'dtop': _entry(dtop, case.tt, False, bd, 'resize_bwd')}


def resize_emulate(case, inp, fused=False, bwd=True):
    """the kernels' fp32 arithmetic: the blend ty.w0 * (tx.w0 * v00 + tx.w1 * v01) + ty.w1 * (...) operation by operation; the gather
    adds (wy * wx) * dout over the destination pixels in (oy, ox) order"""
    top, dout = inp['top'].to(F32), inp['dout'].to(F32)
    ty, tx = resize_taps(case.h, case.H, None, F32, fused), resize_taps(case.w, case.W, None, F32, fused)
    f = lambda t: t.to(F32)      # noqa: E731
    r0, r1 = top.index_select(1, ty['i0']), top.index_select(1, ty['i1'])
    wx0, wx1 = f(tx['w0']).view(1, 1, -1, 1), f(tx['w1']).view(1, 1, -1, 1)
    wy0, wy1 = f(ty['w0']).view(1, -1, 1, 1), f(ty['w1']).view(1, -1, 1, 1)
    row = lambda r: wx0 * r.index_select(2, tx['i0']) + wx1 * r.index_select(2, tx['i1'])      # noqa: E731
    out = wy0 * row(r0) + wy1 * row(r1)
    if inp['lat'] is not None:
        out = out + inp['lat'].to(F32)
    if not bwd:
        return {'out': out.to(F64)}

    def dense(t, n_in):                                     # [n_out, n_in]: (i0 == y ? w0 : 0) + (i1 == y ? w1 : 0) in fp32
        m0, m1 = torch.zeros((t['i0'].numel(), n_in), dtype=F32), torch.zeros((t['i0'].numel(), n_in), dtype=F32)
        ar = torch.arange(t['i0'].numel())
        m0[ar, t['i0']] = f(t['w0'])
        m1[ar, t['i1']] = f(t['w1'])
        return m0 + m1

    Wy, Wx = dense(ty, case.h), dense(tx, case.w)
    acc = torch.zeros((case.N, case.h, case.w, case.C), dtype=F32)
    for oy in range(case.H):
        for ox in range(case.W):
            wgt = (Wy[oy][:, None] * Wx[ox][None, :])[None, :, :, None]
            acc = acc + wgt * dout[:, oy, ox][:, None, None, :]
    return {'out': out.to(F64), 'dtop': rdt(acc.to(F64), case.tt)}


# ================================================================================================ max pooling
MAXPOOL_FAULTS = ('tie_last', 'nan_ignored', 'padding_as_zero', 'uncovered_pixel_not_zeroed', 'index_plane_transposed')
MAXPOOL_VALUES = (0.0, 0.0, 0.0, 0.5, 1.0, 1.5, -1.0, -2.5)        # post-ReLU zeros and a few repeated bf16 values: ties everywhere


@dataclass(frozen=True)
class MaxPoolCase:
    id: str
    dt: str
    N: int
    H: int
    W: int
    cpr: int
    K: int
    stride: int
    pad: int

    @property
    def C(self):
        return self.cpr * EPC[self.dt]

    @property
    def OH(self):
        return (self.H + 2 * self.pad - self.K) // self.stride + 1

    @property
    def OW(self):
        return (self.W + 2 * self.pad - self.K) // self.stride + 1


def _maxpool_table():
    c = []
    geoms = [((3, 2, 1), (16, 16)), ((3, 2, 1), (15, 17)), ((3, 2, 1), (1, 1)), ((2, 2, 0), (8, 8)), ((2, 2, 0), (7, 9)), ((2, 1, 0), (9, 6)),
             ((3, 1, 1), (9, 7)), ((5, 1, 2), (11, 9)), ((1, 2, 0), (7, 8))]
    for dt in DTYPES:
        for i, ((K, s, p), (H, W)) in enumerate(geoms):
            for cpr in (1, 3):
                N = (1, 2)[(i + cpr) % 2]
                c.append(MaxPoolCase(f'{dt}-k{K}s{s}p{p}-{H}x{W}-n{N}-cpr{cpr}', dt, N, H, W, cpr, K, s, p))
        c.append(MaxPoolCase(f'{dt}-k2s1p0-1026x1026-n1-cpr1-big', dt, 1, 1026, 1026, 1, 2, 1, 0))
    return tuple(c)


MAXPOOL_CASES = _maxpool_table()


def maxpool_inputs(case):
    """x [N, H, W, C] and dout [N, OH, OW, C].  Planted where the extent allows: an all -inf block at the top-left corner (with padding
    the first window's maximum is then NOT at window position 0), NaN twice in one window, +inf, -inf alone"""
    g = _gen(case.id)
    N, H, W, C = case.N, case.H, case.W, case.C
    vals = torch.tensor(MAXPOOL_VALUES, dtype=F64)
    x = vals[torch.randint(0, len(MAXPOOL_VALUES), (N, H, W, C), generator=g)]
    if H >= 7 and W >= 6:
        k = min(case.K + 1, 3)
        x[0, :k, :k, :] = -math.inf
        x[0, 4, 3, 0::2] = math.nan
        x[0, 4, 4, 0::2] = math.nan
        x[0, 5, 1, 1] = math.nan
        x[0, 6, 4, :] = math.inf
        x[0, 6, 5, 1::2] = math.inf
        x[0, 3, 1, :] = -math.inf
        x[-1, H - 1, W - 1, :] = -1.0                       # a negative corner: padding must not win as a zero
        x[-1, H - 2:, W - 2:, 1] = -2.5
    elif H == 1 and W == 1:
        x[0, 0, 0, :] = -1.0
        x[0, 0, 0, 1] = -math.inf
    dout = _randint(g, -8, 9, (N, case.OH, case.OW, C))
    dout[dout == 0] = 2.0
    return {'x': x, 'dout': dout}


def _win(n_out, n_in, stride, pad, k):
    i = torch.arange(n_out) * stride - pad + k
    return i, (i >= 0) & (i < n_in)


def maxpool_reference(case, inp, fault=None):
    """the window scanned in (kh, kw) order, a later element replacing the best only if strictly greater or NaN (ATen's CPU rule);
    idx = kh * K + kw of the winner; dx[h, w] = the sum of dout over the windows whose winner sits at (h, w)"""
    x, dout = inp['x'], inp['dout']
    N, H, W, C, K, s, p, OH, OW = case.N, case.H, case.W, case.C, case.K, case.stride, case.pad, case.OH, case.OW
    best = torch.full((N, OH, OW, C), -math.inf, dtype=F64)
    bi = torch.zeros((N, OH, OW, C), dtype=torch.long)
    first = torch.ones((OH, OW), dtype=torch.bool)
    code = (lambda kh, kw: kw * K + kh) if fault == 'index_plane_transposed' else (lambda kh, kw: kh * K + kw)
    for kh in range(K):
        ih, vh = _win(OH, H, s, p, kh)
        for kw in range(K):
            iw, vw = _win(OW, W, s, p, kw)
            valid = vh[:, None] & vw[None, :]
            v = x[:, ih.clamp(0, H - 1)][:, :, iw.clamp(0, W - 1)]
            if fault == 'padding_as_zero':
                v = torch.where(valid[None, :, :, None], v, torch.zeros_like(v))
                valid = torch.ones_like(valid)
            better = (v >= best) if fault == 'tie_last' else (v > best)
            if fault != 'nan_ignored':
                better = better | torch.isnan(v)
            take = valid[None, :, :, None] & (first[None, :, :, None] | better)
            best = torch.where(take, v, best)
            bi = torch.where(take, torch.full_like(bi, code(kh, kw)), bi)
            first = first & ~valid
    dx = torch.zeros((N, H, W, C), dtype=F64)
    cover_h, cover_w = torch.zeros(H, dtype=torch.bool), torch.zeros(W, dtype=torch.bool)
    for kh in range(K):
        ih, vh = _win(OH, H, s, p, kh)
        cover_h[ih[vh]] = True
        for kw in range(K):
            iw, vw = _win(OW, W, s, p, kw)
            cover_w[iw[vw]] = True
            hit = torch.where(bi == code(kh, kw), dout, torch.zeros_like(dout))[:, vh][:, :, vw]
            dx[:, ih[vh][:, None], iw[vw][None, :]] += hit
    if fault == 'uncovered_pixel_not_zeroed':
        covered = cover_h[:, None] & cover_w[None, :]
        dx = torch.where(covered[None, :, :, None], dx, torch.full_like(dx, math.nan))
    return {'out': ('equal', best), 'idx': ('equal', bi.to(F64)), 'dx': ('equal', dx)}


def _cdiv(a, b):
    """C's integer division (towards zero)"""
    return -((-a) // b) if a < 0 else a // b


def maxpool_bwd_branches(case):
    """-> {branch: pixels} of maxpool_bwd_kernel: 'uncovered' (no window), 'quad' (at most 2 x 2 windows), 'loop' (the general gather)"""
    K, s, p = case.K, case.stride, case.pad
    count = {'uncovered': 0, 'quad': 0, 'loop': 0}

    def span(i, n_out):
        return max(0, _cdiv(i + p - (K - 1) + s - 1, s)), min(n_out - 1, (i + p) // s)

    for h in range(case.H):
        lo_h, hi_h = span(h, case.OH)
        for w in range(case.W):
            lo_w, hi_w = span(w, case.OW)
            if hi_h < lo_h or hi_w < lo_w:
                count['uncovered'] += 1
            elif hi_h - lo_h <= 1 and hi_w - lo_w <= 1:
                count['quad'] += 1
            else:
                count['loop'] += 1
    return count


# ================================================================================================ average pooling
AVGPOOL_FAULTS = ('divide_by_hw_minus_one', 'accumulate_in_bf16')


@dataclass(frozen=True)
class AvgPoolCase:
    id: str
    dt: str
    N: int
    HW: int
    cpr: int
    fwd: bool = True

    @property
    def C(self):
        return self.cpr * EPC[self.dt]

    @property
    def exact(self):
        return self.HW & (self.HW - 1) == 0


def _avgpool_table():
    c = []
    for dt in DTYPES:
        for HW in (1, 49, 64, 3136):
            for N, cpr in ((1, 1), (4, 64), (1, 257)):
                c.append(AvgPoolCase(f'{dt}-n{N}-hw{HW}-cpr{cpr}', dt, N, HW, cpr))
    c.append(AvgPoolCase('f32-n2-hw262200-cpr2-bwd-big', 'f32', 2, 262200, 2, fwd=False))
    return tuple(c)


AVGPOOL_CASES = _avgpool_table()


def avgpool_inputs(case):
    g = _gen(case.id)
    N, HW, C = case.N, case.HW, case.C
    inp = {}
    if case.exact:
        if case.fwd:
            inp['x'] = _randint(g, -64, 65, (N, HW, C)) / 8
        inp['dout'] = _randint(g, -64, 65, (N, C)) / 8
    else:
        if case.fwd:
            inp['x'] = rdt(_randn(g, (N, HW, C)) + 0.5, case.dt)
        inp['dout'] = rdt(_randn(g, (N, C)), case.dt)
    return inp


def avgpool_reference(case, inp, fault=None):
    N, HW, C, dt, ex = case.N, case.HW, case.C, case.dt, case.exact
    div = HW - 1 if fault == 'divide_by_hw_minus_one' and HW > 1 else HW
    spec = {}
    if case.fwd:
        x = inp['x']
        if fault == 'accumulate_in_bf16' and dt == 'bf16':
            acc = torch.zeros((N, C), dtype=BF16)
            for p in range(HW):
                acc = acc + x[:, p].to(BF16)
            mean = acc.to(F64) / div
        else:
            mean = x.sum(1) / div
        spec['out'] = _entry(mean, dt, ex, x.abs().sum(1) / HW, 'avgpool_sum')
    dx = (inp['dout'] / div)[:, None, :].expand(N, HW, C)
    spec['dx'] = _entry(dx, dt, ex, dx.abs(), 'chain2')
    return spec


def avgpool_emulate(case, inp):
    """the sequential fp32 sum over the pixels, times fp32(1 / HW)"""
    inv = torch.tensor(np.float32(1.0) / np.float32(case.HW))
    got = {}
    if case.fwd:
        x = inp['x'].to(F32)
        acc = torch.zeros((case.N, case.C), dtype=F32)
        for p in range(case.HW):
            acc = acc + x[:, p]
        got['out'] = rdt((acc * inv).to(F64), case.dt)
    dx = (inp['dout'].to(F32) * inv)[:, None, :].expand(case.N, case.HW, case.C)
    got['dx'] = rdt(dx.to(F64), case.dt)
    return got


# ================================================================================================ what the tables reach
FAMILIES = {
    'stream': (STREAM_CASES, stream_inputs, stream_reference, STREAM_FAULTS),
    'colred': (COL_CASES, col_inputs, col_reference, COLRED_FAULTS),
    'rope': (ROPE_CASES, rope_inputs, rope_reference, ROPE_FAULTS),
    'resize': (RESIZE_CASES, resize_inputs, resize_reference, RESIZE_FAULTS),
    'maxpool': (MAXPOOL_CASES, maxpool_inputs, maxpool_reference, MAXPOOL_FAULTS),
    'avgpool': (AVGPOOL_CASES, avgpool_inputs, avgpool_reference, AVGPOOL_FAULTS),
}


def is_exact(case):
    return True if isinstance(case, MaxPoolCase) else case.exact


def emulate(family, case, inp):
    """the working-precision candidates of an accuracy case -> list of `got` dicts (every form the constants are measured over)"""
    if family == 'stream':
        return [stream_emulate(case, inp)]
    if family == 'rope':
        return [rope_emulate(case, inp)]
    if family == 'resize':
        return [resize_emulate(case, inp, fused=False), resize_emulate(case, inp, fused=True)]
    if family == 'avgpool':
        return [avgpool_emulate(case, inp)]
    if family == 'colred':
        first, parts = col_emulate(case, inp)
        return [first] + [col_emulate(case, inp, seed, parts)[0] for seed in ORDER_SEEDS[1:]]
    raise KeyError(family)


# ================================================================================================ device side (needs a GPU)
FILL_F, FILL_U8, SENTINEL_U8 = -24576.0, 255, 201           # never results of these inputs (-24576 = -3 * 2^13 is exact in bf16)


class GuardedFill:
    """Guarded for an output that may legitimately hold NaN, for a uint8 plane and for an accumulating destination: the contiguous view
    pre-filled with `fill` inside an allocation of sentinel elements.  written=True: an element still equal to `fill` was never
    written (fill is then a value no result takes); written=False: a known pre-fill the kernel adds into."""

    def __init__(self, shape, dtype, device, fill, written=True):
        n = int(np.prod(shape))
        self.sentinel = SENTINEL_U8 if dtype == torch.uint8 else SENTINEL
        self.flat = torch.full((2 * GUARD + n,), self.sentinel, dtype=dtype, device=device)
        self.view = self.flat[GUARD:GUARD + n].view(tuple(shape))
        if torch.is_tensor(fill):
            self.view.copy_(fill.to(dtype).to(device).view(tuple(shape)))
        else:
            self.view.fill_(fill)
        self.fill, self.written = fill, written

    def check(self, name):
        bad = []
        if self.written and bool((self.view == self.fill).any()):
            bad.append(f'{name}: {int((self.view == self.fill).sum())} elements were never written')
        outside = torch.cat([self.flat[:GUARD], self.flat[-GUARD:]])
        if not bool((outside == self.sentinel).all()):
            bad.append(f'{name}: {int((outside != self.sentinel).sum())} sentinel elements outside the view were overwritten')
        return bad


def _L():
    from simpleaicv_pytorch_training_examples_amd import _lib
    return _lib, _lib.lib()


def _dev(t, dt, device):
    return None if t is None else t.to(TD[dt]).contiguous().to(device)


def _guard(shape, dt, device):
    shape = tuple(shape)
    strides = tuple(int(np.prod(shape[i + 1:])) for i in range(len(shape)))
    return Guarded(shape, strides, TD[dt], device)


def _finish(outs):
    """outs: [(name, guard)] -> (got, complaints) after the stream has drained"""
    torch.cuda.synchronize()
    got = {n: g.view.to(F64).cpu() for n, g in outs}
    return got, [m for n, g in outs for m in g.check(n)]


def run_stream(case, inp, device='cuda'):
    """-> (got for judge(), complaints of the guards)"""
    _lib, L = _L()
    dt, op, n = case.dt, case.op, case.n
    code, st, P = _lib.dtype_code(TD[dt]), _lib.stream(), _lib.ptr
    d = {k: _dev(v, 'f32' if k == 's' else dt, device) for k, v in inp.items()}
    if op in ACT_KIND:
        y, dx = _guard((n,), dt, device), _guard((n,), dt, device)
        _lib.check(L.saicv_act_fwd(code, ACT_KIND[op], LEAKY_SLOPE, P(d['x']), P(y.view), n, st), 'act_fwd')
        _lib.check(L.saicv_act_bwd(code, ACT_KIND[op], LEAKY_SLOPE, P(d['dy']), P(d['x']), P(dx.view), n, st), 'act_bwd')
        return _finish([('y', y), ('dx', dx)])
    if op == 'swiglu':
        o, d1, d2 = (_guard((n,), dt, device) for _ in range(3))
        _lib.check(L.saicv_swiglu_fwd(code, P(d['x']), P(d['x2']), P(o.view), n, st), 'swiglu_fwd')
        _lib.check(L.saicv_swiglu_bwd(code, P(d['dy']), P(d['x']), P(d['x2']), P(d1.view), P(d2.view), n, st), 'swiglu_bwd')
        return _finish([('out', o), ('dx1', d1), ('dx2', d2)])
    if op == 'mul':
        o = _guard((n,), dt, device)
        da = None if case.variant == 'da_null' else _guard((n,), dt, device)
        db = None if case.variant == 'db_null' else _guard((n,), dt, device)
        _lib.check(L.saicv_mul_fwd(code, P(d['a']), P(d['b']), P(o.view), n, st), 'mul_fwd')
        _lib.check(L.saicv_mul_bwd(code, P(d['dy']), P(d['a']), P(d['b']), P(da.view) if da else None, P(db.view) if db else None, n, st), 'mul_bwd')
        return _finish([('out', o)] + ([('da', da)] if da else []) + ([('db', db)] if db else []))
    M, C = inp['y'].shape
    o = _guard((M, C), dt, device)
    x = None if case.variant == 'x_null' else d['x']
    s = None if case.variant == 's_null' else d['s']
    _lib.check(L.saicv_channel_scale_add_fwd(code, P(x), P(d['y']), P(s), P(o.view), M, C, st), 'channel_scale_add_fwd')
    return _finish([('out', o)])


def run_colred(case, inp, device='cuda'):
    """the engine's current accumulation mode (atomic, or ordered under the `deterministic` fixture)"""
    _lib, L = _L()
    dt, M, C = case.dt, case.M, case.C
    code, st, P = _lib.dtype_code(TD[dt]), _lib.stream(), _lib.ptr
    if case.op == 'bn_stats':
        x = _dev(inp['x'], dt, device)
        g0 = GuardedFill((C,), F32, device, col_prefill(C, 0), written=False)
        g1 = GuardedFill((C,), F32, device, col_prefill(C, 1), written=False)
        _lib.check(L.saicv_bn_stats(code, P(x), M, C, P(g0.view), P(g1.view), st), 'bn_stats')
        return _finish([('sum', g0), ('sq', g1)])
    dout, y, s = _dev(inp['dout'], dt, device), _dev(inp['y'], dt, device), _dev(inp['s'], 'f32', device)
    outs = []
    dy = ds = None
    if case.variant != 'ds_only':
        dy = _guard((M, C), dt, device)
        outs.append(('dy', dy))
    if case.variant != 'dy_only':
        ds = GuardedFill((C,), F32, device, col_prefill(C, 0), written=False)
        outs.append(('ds', ds))
    if case.variant == 'dy_only':
        y = None                                            # the branch output is read for ds alone
    _lib.check(L.saicv_channel_scale_add_bwd(code, P(dout), P(y), None if case.variant == 's_null' else P(s), P(dy.view) if dy else None,
                                             P(ds.view) if ds else None, M, C, st), 'channel_scale_add_bwd')
    return _finish(outs)


def run_rope(case, inp, device='cuda'):
    _lib, L = _L()
    qkv = _dev(inp['qkv'], case.dt, device)
    rows = max(case.N - case.prefix, 1)                     # prefix == N: the tables are never read, the pointers must still be valid
    sin, cos = torch.zeros((rows, case.D), device=device), torch.zeros((rows, case.D), device=device)
    if case.N > case.prefix:
        sin, cos = _dev(inp['sin'], 'f32', device), _dev(inp['cos'], 'f32', device)
    o = _guard(tuple(inp['qkv'].shape), case.dt, device)
    _lib.check(L.saicv_rope_apply(_lib.dtype_code(TD[case.dt]), _lib.ptr(qkv), _lib.ptr(sin), _lib.ptr(cos), _lib.ptr(o.view), case.B, case.N,
                                  case.heads, case.D, case.prefix, case.transpose, _lib.stream()), 'rope_apply')
    got, bad = _finish([('out', o)])
    copied = rope_copied(case)
    if not torch.equal(o.view.cpu()[copied], qkv.cpu()[copied]):
        bad.append('out: v or the prefix tokens are not the copied bits')
    return got, bad


def run_resize(case, inp, device='cuda'):
    _lib, L = _L()
    N, C, h, w, H, W = case.N, case.C, case.h, case.w, case.H, case.W
    top, dout = _dev(inp['top'], case.tt, device), _dev(inp['dout'], 'f32', device)
    lat = None if inp['lat'] is None else _dev(inp['lat'], case.tl, device)
    o, dtop = _guard((N, H, W, C), 'f32', device), _guard((N, h, w, C), case.tt, device)
    ct = _lib.dtype_code(TD[case.tt])
    cl = _lib.dtype_code(TD[case.tl]) if lat is not None else ct
    _lib.check(L.saicv_resize_bilinear_add_fwd(ct, cl, _lib.ptr(top), _lib.ptr(lat), _lib.ptr(o.view), N, h, w, H, W, C, _lib.stream()),
               'resize_bilinear_add_fwd')
    _lib.check(L.saicv_resize_bilinear_bwd(ct, _lib.ptr(dout), _lib.ptr(dtop.view), N, h, w, H, W, C, _lib.stream()), 'resize_bilinear_bwd')
    return _finish([('out', o), ('dtop', dtop)])


def run_maxpool(case, inp, device='cuda'):
    """the backward reads the index plane the forward has just recorded"""
    _lib, L = _L()
    N, H, W, C, OH, OW = case.N, case.H, case.W, case.C, case.OH, case.OW
    code, st, P = _lib.dtype_code(TD[case.dt]), _lib.stream(), _lib.ptr
    x, dout = _dev(inp['x'], case.dt, device), _dev(inp['dout'], case.dt, device)
    o = GuardedFill((N, OH, OW, C), TD[case.dt], device, FILL_F)
    idx = GuardedFill((N, OH, OW, C), torch.uint8, device, FILL_U8)
    dx = _guard((N, H, W, C), case.dt, device)
    _lib.check(L.saicv_maxpool_fwd(code, P(x), P(o.view), P(idx.view), N, H, W, C, OH, OW, case.K, case.stride, case.pad, st), 'maxpool_fwd')
    _lib.check(L.saicv_maxpool_bwd(code, P(dout), P(idx.view), P(dx.view), N, H, W, C, OH, OW, case.K, case.stride, case.pad, st), 'maxpool_bwd')
    return _finish([('out', o), ('idx', idx), ('dx', dx)])


def run_avgpool(case, inp, device='cuda'):
    _lib, L = _L()
    N, HW, C = case.N, case.HW, case.C
    code, st, P = _lib.dtype_code(TD[case.dt]), _lib.stream(), _lib.ptr
    outs = []
    if case.fwd:
        x = _dev(inp['x'], case.dt, device)
        o = _guard((N, C), case.dt, device)
        _lib.check(L.saicv_avgpool_fwd(code, P(x), P(o.view), N, HW, C, st), 'avgpool_fwd')
        outs.append(('out', o))
    dout = _dev(inp['dout'], case.dt, device)
    dx = _guard((N, HW, C), case.dt, device)
    _lib.check(L.saicv_avgpool_bwd(code, P(dout), P(dx.view), N, HW, C, st), 'avgpool_bwd')
    outs.append(('dx', dx))
    return _finish(outs)


RUNNERS = {'stream': run_stream, 'colred': run_colred, 'rope': run_rope, 'resize': run_resize, 'maxpool': run_maxpool, 'avgpool': run_avgpool}
