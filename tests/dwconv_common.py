"""What tests/test_dwconv_judge_host.py (no GPU) and tests/test_gpu_dwconv_f64.py (MI355X) share for the depthwise convolution kernels of
csrc/dwconv.hip: the launch geometry restated, the case tables of saicv_dwconv2d_fwd / _dgrad / _wgrad, the input builders, the float64
references (F.conv2d(groups=C) with autograd, and an independent tap-shifted formulation that also yields the magnitude sums and takes
planted faults), the fp32 emulations of the kernels' own order, the judge, and the launchers (C-ABI, outputs in guarded allocations).

Two regimes, as in glue_common.
  exact     x and dy integers in [-2, 2], weights in {-1, 0, 1} (asymmetric in both axes and under transposition), bias integers in
            [-4, 4], accumulation targets pre-filled with known integers.  With at most 64 taps every forward / data-gradient value is an
            integer of magnitude <= 132 (exact in fp32 and in bf16), every weight-gradient sum far below 2^24.  torch.equal, nothing left out.
  accuracy  random operands rounded once to the compute dtype; an element passes when |got - ref| <= allowed * u * bound (+ the house
            half-unit term for the one rounding of a stored bf16 value), u = 2^-24, bound the same convolution applied to magnitudes
            (|x| with |w| plus |b|; |dy| with |w|; |dy| with |x| plus the pre-fill).  Forward and data gradient are a chain of at most
            K * K fused multiply-adds that starts from the bias: each term passes through at most K * K roundings, so
            allowed = K * K + 1 (FIXED, derived; the + 1 absorbs the second-order terms).  The weight gradient is a sum of up to thousands
            of terms in the kernel's own partition: allowed = MARGIN * CONSTANTS[...], the worst ratio of a CPU fp32 emulation of that
            partition (per-thread chain over its pixel sub-range, the LDS sum over the sub-ranges, the pixel ranges through
            detloss_common.fold_partials over ORDER_SEEDS), which the host test measures and holds.

Tensors here are NHWC ([N, H, W, C]) in float64 unless said otherwise; the weight is PyTorch's [C, 1, K, K] and the launcher makes it
tap-major ([K * K][C]) itself, independently of ops.py.
"""
import math
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from attn_common import GUARD, MARGIN, SENTINEL, U, Guarded      # noqa: F401  (GUARD, SENTINEL, Guarded: for the tests that import this module)
from detloss_common import ORDER_SEEDS, fold_partials
from glue_common import GuardedFill, _dev, _finish, _fma32, _gen, _guard, _L, _randint, _randn, bf16_half_ulp, col_prefill, r32, rdt

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
TD = {'f32': F32, 'bf16': BF16}
DTYPES = ('f32', 'bf16')
EPC = {'f32': 4, 'bf16': 8}                                 # elements of a 16-byte chunk
UF = U[F32]
LEFT_OUT_CAP = 0.005                                        # no case of these tables leaves an element out (the host test asserts it)
DW_TW, S1_TW, DW_THREADS, DW_CAP = 4, 8, 256, 16384        # DW_TW, TW of dwconv_s1_kernel, the block, the cap of dw_grid()
WALK_K = (3, 5, 7)                                          # the instantiations of dwconv_s1_kernel
COOP_CH = 32                                                # det.hip: from this many parts the cooperative fold runs
MAX_K = 8

# Worst ratio of the fp32 emulation of dwconv_wgrad_kernel (+ the fold over ORDER_SEEDS) to the float64 reference over every accuracy case
# of WGRAD_CASES, in units of u * bound.  Measured by tests/test_dwconv_judge_host.py::test_constants_table_is_what_the_emulations_measure
# (which fails if a row drifts by more than a quarter, on one thread); the judge allows MARGIN times these.  Never raised by hand.
CONSTANTS = {'dw': 2.66, 'db': 1.34}
CONSTANTS_MEASURED_WITH = 'torch 2.10.0+rocm7.0 (CPU, one thread), 2026-10-20'
# derived: a chain of K * K fused multiply-adds from the bias (docstring)
FIXED = {f'chain_k{K}': float(K * K + 1) for K in range(1, MAX_K + 1)}


# ================================================================================================ launch geometry, restated
def dw_grid(items):
    """dw_grid() of csrc/dwconv.hip restated"""
    return int(min(max((items + DW_THREADS - 1) // DW_THREADS, 1), DW_CAP))


def dw_trips(items):
    """trips of the longest-running thread through the grid-stride loop of dwconv_gather_kernel / dwconv_s1_kernel"""
    return -(-items // (dw_grid(items) * DW_THREADS))


def out_extent(n_in, K, stride, pad, dil):
    """dw_out() of csrc/dwconv.hip restated: the output extent of one axis, 0 where the kernel does not fit"""
    span = n_in + 2 * pad - dil * (K - 1) - 1
    return 0 if span < 0 else span // stride + 1


def fwd_route(K, stride, pad, dil):
    """the route predicate of saicv_dwconv2d_fwd: 'walk' (dwconv_s1_kernel) | 'gather' (dwconv_gather_kernel)"""
    return 'walk' if stride == 1 and dil == 1 and K in WALK_K else 'gather'


def dgrad_route(K, stride, pad, dil):
    """the route predicate of saicv_dwconv2d_dgrad: the walk kernel needs its mirrored padding K - 1 - pad >= 0"""
    return 'walk' if fwd_route(K, stride, pad, dil) == 'walk' and K - 1 - pad >= 0 else 'gather'


def tile_width(route):
    """output pixels of one row per thread: TW = 8 of the walk kernel, DW_TW = 4 of the gather kernel"""
    return S1_TW if route == 'walk' else DW_TW


def conv_items(N, DH, DW, cpr, route):
    """work items of a forward / data-gradient launch over a destination of N x DH x DW pixels"""
    return N * DH * (-(-DW // tile_width(route))) * cpr


def wgrad_geom(npix, cpr, K):
    """the launch quantities of saicv_dwconv2d_wgrad and dwconv_wgrad_kernel restated -> dict"""
    cpb = 1
    while cpb * 2 * K <= 256 and cpb * 2 <= cpr:
        cpb *= 2
    groups = (cpr + cpb - 1) // cpb
    ranges = max(min((1024 + groups - 1) // groups, 512), 1)
    ppb = max((npix + ranges - 1) // ranges, 256)
    ranges = (npix + ppb - 1) // ppb
    lanes_per_ps = cpb * K
    nps = 256 // lanes_per_ps
    sub = (ppb + nps - 1) // nps
    last = npix - (ranges - 1) * ppb                        # pixels of the last range
    ordered = ranges > 1                                    # DetParts::begin takes the workspace for more than one part only
    fold = None if not ordered else ('det_fold4_coop_kernel' if ranges >= COOP_CH else 'det_fold4_kernel')
    return {'cpb': cpb, 'groups': groups, 'lanes_per_ps': lanes_per_ps, 'nps': nps, 'sub': sub, 'ppb': ppb, 'ranges': ranges, 'last': last,
            'dead_threads': 256 - nps * lanes_per_ps, 'dead_chunk_lanes': groups * cpb - cpr,
            'subs_behind_the_block': sum(1 for ps in range(nps) if ps * sub >= ppb),
            'subs_behind_the_last_range': sum(1 for ps in range(nps) if ps * sub >= last), 'ordered': ordered, 'fold': fold}


def wgrad_lds_bytes(K, dt):
    """dynamic LDS of dwconv_wgrad_kernel<T, K>: 256 threads x (K + 1) sums x one chunk of fp32"""
    return 256 * (K + 1) * EPC[dt] * 4


# ================================================================================================ the case tables
@dataclass(frozen=True)
class DwCase:
    id: str
    table: str                  # walk | gather | wgrad | big
    dt: str
    N: int
    H: int
    W: int
    cpr: int
    K: int
    stride: int = 1
    pad: int = 0
    dil: int = 1
    bias: bool = True           # forward: a bias is passed; weight gradient: dbias is not NULL
    exact: bool = True

    @property
    def C(self):
        return self.cpr * EPC[self.dt]

    @property
    def OH(self):
        return out_extent(self.H, self.K, self.stride, self.pad, self.dil)

    @property
    def OW(self):
        return out_extent(self.W, self.K, self.stride, self.pad, self.dil)

    @property
    def npix(self):
        return self.N * self.OH * self.OW

    @property
    def geom(self):
        return (self.K, self.stride, self.pad, self.dil)

    @property
    def fwd_route(self):
        return fwd_route(*self.geom)

    @property
    def dgrad_route(self):
        return dgrad_route(*self.geom)

    @property
    def fwd_items(self):
        return conv_items(self.N, self.OH, self.OW, self.cpr, self.fwd_route)

    @property
    def dgrad_items(self):
        return conv_items(self.N, self.H, self.W, self.cpr, self.dgrad_route)

    @property
    def wgrad(self):
        return wgrad_geom(self.npix, self.cpr, self.K)


def _cid(table, dt, tag, N, H, W, cpr, bias, exact):
    return f'{table}-{dt}-{tag}-n{N}-{H}x{W}-cpr{cpr}-{"b" if bias else "nob"}-{"exact" if exact else "random"}'


WALK_WIDTHS = (1, 7, 8, 9, 17)                              # destination widths around the eight-pixel tile
WALK_RANDOM_WIDTHS = (7, 17)


def _walk_table():
    """K x pad x destination width, the width once as the forward's (OW) and once as the data gradient's (W); pad K + 1 is the forward's
    alone: its data gradient is the gather kernel's"""
    c, seen, i = [], set(), 0
    for K in WALK_K:
        for pad in (0, (K - 1) // 2, K - 1, K + 1):
            for t in WALK_WIDTHS:
                for which in ('ow', 'w'):
                    W = t - 2 * pad + K - 1 if which == 'ow' else t
                    H = max(3, K - 2 * pad + 1)
                    if W < 1 or out_extent(W, K, 1, pad, 1) < 1 or (K, pad, W) in seen:
                        continue
                    seen.add((K, pad, W))
                    cpr, bias = (1, 3)[i % 2], i % 3 != 0
                    i += 1
                    for dt in DTYPES:
                        c.append(DwCase(_cid('walk', dt, f'k{K}p{pad}', 2, H, W, cpr, bias, True), 'walk', dt, 2, H, W, cpr, K, 1, pad, 1, bias))
                        if t in WALK_RANDOM_WIDTHS:
                            c.append(DwCase(_cid('walk', dt, f'k{K}p{pad}', 2, H, W, cpr, bias, False), 'walk', dt, 2, H, W, cpr, K, 1, pad, 1, bias, False))
    return tuple(c)


# (tag, K, stride, pad, dil, remainder): `remainder` more rows and columns than the last output reads
GATHER_GEOMS = (('k1', 1, 1, 0, 1, 0), ('k2', 2, 1, 1, 1, 0), ('k4', 4, 1, 2, 1, 0), ('k6', 6, 1, 3, 1, 0), ('k8', 8, 1, 4, 1, 0),
                ('k3s2', 3, 2, 1, 1, 0), ('k3s3', 3, 3, 1, 1, 2), ('k7d3', 7, 1, 9, 3, 0), ('k3s2d2', 3, 2, 2, 2, 0), ('k3p3', 3, 1, 3, 1, 0))
GATHER_WIDTHS = (1, 3, 4, 5, 9)                             # destination widths around the four-pixel tile
GATHER_RANDOM_WIDTHS = (5, 9)


def _gather_table():
    c, seen, i = [], set(), 0
    for tag, K, s, p, d, rem in GATHER_GEOMS:
        base = d * (K - 1) + 1 - 2 * p + rem                # the input extent of ONE output
        H = max(2, base + s)                                # two output rows
        if tag == 'k3s3':
            H = base + s
        geoms = []
        for t in GATHER_WIDTHS:
            geoms += [(t, (t - 1) * s + base, H), (t, t, H)]
        if tag == 'k7d3':
            geoms.append((9, 13, 11))                       # the VAN layer at 11 x 13
        for t, W, h in geoms:
            if W < 1 or out_extent(W, K, s, p, d) < 1 or out_extent(h, K, s, p, d) < 1 or (tag, W, h) in seen:
                continue
            seen.add((tag, W, h))
            cpr, bias = (1, 3)[i % 2], i % 3 != 1
            i += 1
            for dt in DTYPES:
                c.append(DwCase(_cid('gather', dt, tag, 2, h, W, cpr, bias, True), 'gather', dt, 2, h, W, cpr, K, s, p, d, bias))
                if t in GATHER_RANDOM_WIDTHS:
                    c.append(DwCase(_cid('gather', dt, tag, 2, h, W, cpr, bias, False), 'gather', dt, 2, h, W, cpr, K, s, p, d, bias, False))
    return tuple(c)


def smallest_cpr_with_one_sub_range(K):
    """the smallest channel-chunk count at which the 256-lane cap leaves nps == 1"""
    return next(cpr for cpr in range(1, 257) if wgrad_geom(256, cpr, K)['nps'] == 1)


def last_sub_range_live(g, npix):
    """whether the last pixel sub-range of the first block holds pixels (the last term of the LDS sum is not zero)"""
    return g['nps'] > 1 and (g['nps'] - 1) * g['sub'] < min(g['ppb'], npix)


def smallest_cpr_with_a_live_last_sub_range(K):
    """sub = ceil(256 / nps) leaves the trailing sub-ranges empty for most (K, chunks): K = 3 needs 8 chunks, K = 7 two"""
    return next(cpr for cpr in range(1, 257) if last_sub_range_live(wgrad_geom(256, cpr, K), 256))


def _wgrad_table():
    c = []

    def add(tag, N, H, W, cpr, K, s, p, d, bias, random=False):
        for dt in DTYPES:
            c.append(DwCase(_cid('wgrad', dt, tag, N, H, W, cpr, bias, True), 'wgrad', dt, N, H, W, cpr, K, s, p, d, bias))
            if random:
                c.append(DwCase(_cid('wgrad', dt, tag, N, H, W, cpr, bias, False), 'wgrad', dt, N, H, W, cpr, K, s, p, d, bias, False))

    i = 0
    for K in range(1, MAX_K + 1):                           # every instantiation at 1, 3 (dead chunk lanes) and 16 chunks
        for cpr in (1, 3, 16):
            add(f'k{K}p{K // 2}', 2, 5, 6, cpr, K, 1, K // 2, 1, i % 2 == 0, random=cpr == 3 and K in (1, 4, 5, 8))
            i += 1
    for K in range(1, MAX_K + 1):                           # 256 pixels at the fewest chunks that leave the LAST sub-range of the block pixels
        H, W = (8, 16) if K % 2 else (7, 15)
        add(f'k{K}p{K // 2}-lastsub', 2, H, W, smallest_cpr_with_a_live_last_sub_range(K), K, 1, K // 2, 1, K % 2 == 1, random=K in (2, 3, 5, 7, 8))
    for K in (3, 7, 8):                                     # the 256-lane cap: nps == 1 (and dead threads behind it for K = 3 and 7)
        add(f'k{K}p{K // 2}-nps1', 1, 5, 5, smallest_cpr_with_one_sub_range(K), K, 1, K // 2, 1, K != 7, random=True)
    for K in (3, 7):                                        # npix 256 (one range), 257 (a second range of one pixel), 8320 (33 ranges)
        for N, H, W in ((2, 8, 16), (1, 1, 257), (2, 64, 65)):
            for bias in (True, False):
                add(f'k{K}p{K // 2}', N, H, W, 1, K, 1, K // 2, 1, bias, random=bias == (K == 3))
    add('k5p2', 1, 1, 257, 3, 5, 1, 2, 1, True, random=True)                       # two ranges with dead chunk lanes
    add('k3s2', 2, 9, 9, 1, 3, 2, 1, 1, False)                                   # skipped rows and columns under stride, dilation, padding
    add('k3s3', 2, 6, 9, 3, 3, 3, 1, 1, True, random=True)
    add('k7d3', 2, 11, 13, 1, 7, 1, 9, 3, True, random=True)
    add('k3s2d2', 2, 7, 9, 3, 3, 2, 2, 2, False)
    add('k3p3', 2, 3, 4, 1, 3, 1, 3, 1, True)
    add('k3p0', 2, 5, 6, 1, 3, 1, 0, 1, False)
    return tuple(c)


BIG_ROWS = 2097152 + 129                                    # per image; N = 2: just above 16384 x 256 one-pixel items


def _big_table():
    """the second trip of the grid-stride loops: bf16, exact regime, W = 1, C = 8, one pixel per item"""
    return (DwCase('big-bf16-k1-gather', 'big', 'bf16', 2, BIG_ROWS, 1, 1, 1, 1, 0, 1, True),
            DwCase('big-bf16-k3p1-walk', 'big', 'bf16', 2, BIG_ROWS, 1, 1, 3, 1, 1, 1, True))


WALK_CASES, GATHER_CASES, WGRAD_CASES, BIG_CASES = _walk_table(), _gather_table(), _wgrad_table(), _big_table()
CONV_CASES = WALK_CASES + GATHER_CASES
ALL_CASES = CONV_CASES + WGRAD_CASES


def unread(case):
    """-> (rows, columns) of x that no output reads, as bool vectors: their data gradient is an exact zero"""
    out = []
    for n_in, n_out in ((case.H, case.OH), (case.W, case.OW)):
        read = torch.zeros(n_in, dtype=torch.bool)
        for k in range(case.K):
            i = torch.arange(n_out) * case.stride - case.pad + k * case.dil
            read[i[(i >= 0) & (i < n_in)]] = True
        out.append(~read)
    return tuple(out)


def _reached():
    """which case first reaches each template instantiation and launch form, from the restated geometry alone"""
    r = {'gather': {}, 's1': {}, 'wgrad': {}, 'last_sub_range_live': {}, 'flags': {}}

    def flag(name, on, case):
        if on:
            r['flags'].setdefault(name, case.id)

    for case in CONV_CASES + BIG_CASES:
        for flip, route, items in ((False, case.fwd_route, case.fwd_items), (True, case.dgrad_route, case.dgrad_items)):
            if route == 'walk':
                r['s1'].setdefault((case.dt, case.K, flip), case.id)
            else:
                r['gather'].setdefault((case.dt, flip), case.id)
            flag(f'second_trip_{route}_{"dgrad" if flip else "fwd"}', dw_trips(items) >= 2, case)
        flag('dgrad_falls_back_to_gather', case.fwd_route == 'walk' and case.dgrad_route == 'gather', case)
        flag('inexact_quotients', case.stride > 1, case)
        flag('unread_rows_and_columns', bool(unread(case)[0].any()) and bool(unread(case)[1].any()), case)
    for case in WGRAD_CASES:
        g = case.wgrad
        r['wgrad'].setdefault((case.dt, case.K), case.id)
        flag('nps==1', g['nps'] == 1, case)
        flag('nps>1', g['nps'] > 1, case)
        flag('dead_chunk_lanes', g['dead_chunk_lanes'] > 0, case)
        flag('dead_threads', g['dead_threads'] > 0, case)
        flag('dead_threads_at_nps==1', g['dead_threads'] > 0 and g['nps'] == 1, case)
        flag('sub_ranges_behind_the_block', g['subs_behind_the_block'] > 0, case)
        if last_sub_range_live(g, case.npix):
            r['last_sub_range_live'].setdefault((case.dt, case.K), case.id)
        flag('ragged_last_range', g['ranges'] > 1 and g['last'] < g['ppb'], case)
        flag('ranges==1', g['ranges'] == 1, case)
        flag('ranges==2', g['ranges'] == 2, case)
        flag('ranges>=32', g['ranges'] >= 32, case)
        for fold in ('det_fold4_kernel', 'det_fold4_coop_kernel'):
            flag(fold, g['fold'] == fold, case)
        flag('dbias_null', not case.bias, case)
        flag('dbias', case.bias, case)
        flag('dbias_null_ordered', not case.bias and g['ordered'], case)
        flag('lds_above_64KiB', wgrad_lds_bytes(case.K, case.dt) > 65536, case)
        flag('skipped_rows', case.pad > 0 or case.dil > 1, case)
    return r


REACHED = _reached()


# ================================================================================================ inputs
def inputs(case):
    """x [N, H, W, C], w [C, 1, K, K], b [C] (None: no bias), dy [N, OH, OW, C], float64 holding values of the case's dtype (b: fp32)"""
    g = _gen(case.id)
    N, H, W, C, K, OH, OW = case.N, case.H, case.W, case.C, case.K, case.OH, case.OW
    if case.exact:
        x, dy = _randint(g, -2, 3, (N, H, W, C)), _randint(g, -2, 3, (N, OH, OW, C))
        w, b = _randint(g, -1, 2, (C, 1, K, K)), _randint(g, -4, 5, (C,))
        if K >= 2:                                          # no mirror image and no transpose of the kernel equals it
            w[:, 0, 0, 0], w[:, 0, 0, K - 1], w[:, 0, K - 1, 0], w[:, 0, K - 1, K - 1] = 1.0, -1.0, 0.0, -1.0
        b[b == 0] = 3.0
    else:
        x, dy = rdt(_randn(g, (N, H, W, C)), case.dt), rdt(_randn(g, (N, OH, OW, C)), case.dt)
        w, b = rdt(_randn(g, (C, 1, K, K)) / K, case.dt), r32(_randn(g, (C,), 0.5))
    return {'x': x, 'w': w, 'b': b if case.bias and case.table != 'wgrad' else None, 'dy': dy}


def big_inputs(case):
    """the inputs of a BIG case as float32 (integers, exact in bf16), drawn as int8"""
    g = _gen(case.id)
    ri = lambda lo, hi, shape: torch.randint(lo, hi, shape, generator=g, dtype=torch.int8).to(F32)      # noqa: E731
    x, dy = ri(-2, 3, (case.N, case.H, 1, case.C)), ri(-2, 3, (case.N, case.OH, 1, case.C))
    w, b = ri(-1, 2, (case.C, 1, case.K, case.K)), ri(-4, 5, (case.C,))
    if case.K >= 2:
        w[:, 0, 0, case.pad], w[:, 0, case.K - 1, case.pad] = 1.0, -1.0       # the acting column is not its own mirror image
    return {'x': x, 'w': w, 'b': b, 'dy': dy}


def big_reference(case, inp):
    """W = 1, pad = K // 2: only the kernel column `pad` acts.  K shifted elementwise products in torch, float32 (integers: exact)"""
    assert case.W == 1 and case.OW == 1 and case.stride == 1 and case.dil == 1 and case.OH == case.H and case.pad == case.K // 2
    x, dy, w, b = inp['x'], inp['dy'], inp['w'], inp['b']
    H, p = case.H, case.pad
    y = b.view(1, 1, 1, -1).expand_as(x).clone()
    dx = torch.zeros_like(x)
    for r in range(case.K):
        o = r - p                                           # y[h] += x[h + o] w[r]; dx[h + o] += dy[h] w[r]
        lo, hi = max(0, -o), min(H, H - o)
        wr = w[:, 0, r, p].view(1, 1, 1, -1)
        y[:, lo:hi] += x[:, lo + o:hi + o] * wr
        dx[:, lo + o:hi + o] += dy[:, lo:hi] * wr
    return {'y': y, 'dx': dx}


# ================================================================================================ the float64 references
FAULTS = ('unmirrored_dgrad', 'taps_transposed', 'pad_off_by_one', 'row_wrap', 'last_tile_dropped', 'inexact_quotient_kept',
          'dilation_ignored_in_dgrad', 'bias_per_tap', 'bias_per_kernel_row', 'assign_not_add', 'last_range_dropped', 'image_seam_ignored')


def conv_f64(case, inp):
    """F.conv2d(groups=C) and its autograd in float64 on the CPU -> y, dx [NHWC], dw [K * K, C] (tap-major), db [C]"""
    x = inp['x'].permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    w = inp['w'].clone().requires_grad_(True)
    b = torch.zeros(case.C, dtype=F64, requires_grad=True)
    y = F.conv2d(x, w, b if inp['b'] is None else b + inp['b'], case.stride, case.pad, case.dil, groups=case.C)
    gx, gw, gb = torch.autograd.grad(y, (x, w, b), inp['dy'].permute(0, 3, 1, 2).contiguous())
    return {'y': y.detach().permute(0, 2, 3, 1), 'dx': gx.permute(0, 2, 3, 1), 'dw': gw[:, 0].permute(1, 2, 0).reshape(case.K ** 2, case.C), 'db': gb}


def _axis_taps(case, n_dst, n_src, k, dgrad, keep_inexact=False):
    """the source index of tap k for every destination index of one axis, and whether the tap exists.  Forward: i * stride - pad + k dil;
    data gradient: (i + pad - k dil) / stride where the quotient is exact (keep_inexact: C's truncated quotient, the planted fault)"""
    i = torch.arange(n_dst)
    if not dgrad:
        src = i * case.stride - case.pad + k * case.dil
        ok = torch.ones_like(src, dtype=torch.bool)
    else:
        num = i + case.pad - k * case.dil
        ok = (num >= 0) if keep_inexact else (num >= 0) & (num % case.stride == 0)
        src = torch.div(num.clamp_min(0), case.stride, rounding_mode='floor')
    ok = ok & (src >= 0) & (src < n_src)
    return src.clamp(0, n_src - 1), ok


def gather_form(case, src, w, bias, dgrad, wd=F64, keep_inexact=False, descending=False):
    """the kernels' own gather form: every destination pixel collects its taps one after the other from the bias (wd = F32: an fp32
    fused multiply-add per tap, the emulation).  src: x (forward) or dy (data gradient); descending: the taps in the mirrored order of
    dwconv_s1_kernel<FLIPW = true>"""
    K = case.K
    DH, DW_, SH, SW = (case.H, case.W, case.OH, case.OW) if dgrad else (case.OH, case.OW, case.H, case.W)
    src, w = src.to(wd), w.to(wd)
    acc = torch.zeros((case.N, DH, DW_, case.C), dtype=wd)
    if bias is not None and not dgrad:
        acc = acc + bias.to(wd)
    order = [(r, c) for r in range(K) for c in range(K)]
    for r, c in (reversed(order) if descending else order):
        ih, okh = _axis_taps(case, DH, SH, r, dgrad, keep_inexact)
        iw, okw = _axis_taps(case, DW_, SW, c, dgrad, keep_inexact)
        ok = (okh[:, None] & okw[None, :])[None, :, :, None]
        v = torch.where(ok, src[:, ih][:, :, iw], torch.zeros((), dtype=wd))
        acc = _fma32(v, w[:, 0, r, c].expand_as(v), acc) if wd == F32 else acc + v * w[:, 0, r, c]
    return acc


def direct(case, inp, fault=None, mag=False):
    """The second formulation, independent of F.conv2d: tap-shifted adds on a zero-padded copy -- the forward and the weight gradient read
    strided windows of it, the data gradient scatters dy * w into it.  mag: the same on magnitudes (the judge's bounds, no pre-fill).
    fault: one of FAULTS, planted here and nowhere else.  -> y, dx, dw [K * K, C], db"""
    N, H, W, C, K, s, p, d, OH, OW = case.N, case.H, case.W, case.C, case.K, case.stride, case.pad, case.dil, case.OH, case.OW
    x, dy, w, b = inp['x'], inp['dy'], inp['w'][:, 0], inp['b']
    if mag:
        x, dy, w, b = x.abs(), dy.abs(), w.abs(), None if b is None else b.abs()
    big = p + d * (K - 1) + s + 2
    xp = torch.zeros((N, H + 2 * big, W + 2 * big, C), dtype=F64)
    xp[:, big:big + H, big:big + W] = x
    if fault == 'row_wrap':                                 # a tap left of column 0 reads the previous row's last pixels (flat addressing)
        flat = x.reshape(N * H * W, C)
        for j in range(1, min(big, W) + 1):
            idx = torch.arange(N * H) * W - j
            v = torch.where((idx >= 0)[:, None], flat[idx.clamp_min(0)], torch.zeros((), dtype=F64))
            xp[:, big:big + H, big - j] = v.view(N, H, C)
    if fault == 'image_seam_ignored':                       # rows above / below an image are the neighbouring image's
        for j in range(1, min(big, H) + 1):
            xp[1:, big - j, big:big + W] = x[:-1, H - j]
            xp[:-1, big + H + j - 1, big:big + W] = x[1:, j - 1]
    pe = p + 1 if fault == 'pad_off_by_one' else p
    tap = (lambda r, c: w[:, c, r]) if fault == 'taps_transposed' else (lambda r, c: w[:, r, c])

    def window(t, r, c, dd=d):
        h0, w0 = big - pe + r * dd, big - pe + c * dd
        return t[:, h0:h0 + (OH - 1) * s + 1:s, w0:w0 + (OW - 1) * s + 1:s]

    y = torch.zeros((N, OH, OW, C), dtype=F64)
    for r in range(K):
        for c in range(K):
            y = y + window(xp, r, c) * tap(r, c)
    if b is not None:
        y = y + b * {'bias_per_tap': K * K, 'bias_per_kernel_row': K}.get(fault, 1)

    if fault == 'inexact_quotient_kept':
        dx = gather_form(case, dy, inp['w'], None, True, keep_inexact=True)
    else:
        dxp = torch.zeros_like(xp)
        dd = 1 if fault == 'dilation_ignored_in_dgrad' else d
        for r in range(K):
            for c in range(K):
                wt = tap(K - 1 - r, K - 1 - c) if fault == 'unmirrored_dgrad' else tap(r, c)
                window(dxp, r, c, dd).add_(dy * wt)
        dx = dxp[:, big:big + H, big:big + W].clone()

    keep = torch.ones(case.npix, dtype=F64)
    if fault == 'last_range_dropped':
        g = case.wgrad
        if g['ranges'] > 1:
            keep[(g['ranges'] - 1) * g['ppb']:] = 0.0
    dyk = dy * keep.view(N, OH, OW, 1)
    dw = torch.stack([(dyk * window(xp, r, c)).sum((0, 1, 2)) for r in range(K) for c in range(K)])
    if fault == 'taps_transposed':
        dw = dw.view(K, K, C).transpose(0, 1).reshape(K * K, C)
    return {'y': y, 'dx': dx, 'dw': dw, 'db': dyk.sum((0, 1, 2))}


def dw_prefill(case):
    """the known integers the accumulation targets hold before the launch -> (dwt [K * K, C], dbias [C])"""
    return col_prefill(case.K ** 2 * case.C, 0).view(case.K ** 2, case.C), col_prefill(case.C, 1)


def _entry(ref, dt, exact, bound, q):
    """one spec entry for an output stored in the dtype dt"""
    if exact:
        return ('equal', rdt(ref, dt))
    return ('bound', ref, bound, q, bf16_half_ulp(ref) if dt == 'bf16' else None)


def reference(case, inp, fault=None):
    """-> spec for judge(): y and dx of a forward / data-gradient case, dw (and db) of a weight-gradient case.  The values are
    F.conv2d's and its autograd's; under a planted fault the direct formulation's.  The bounds are the direct formulation on magnitudes."""
    vals = conv_f64(case, inp) if fault is None else direct(case, inp, fault)
    mags = direct(case, inp, mag=True)
    if case.table != 'wgrad':
        y, dx = vals['y'].clone(), vals['dx'].clone()
        if fault == 'last_tile_dropped':                    # the last width tile of each destination is never written
            for t, width, route in ((y, case.OW, case.fwd_route), (dx, case.W, case.dgrad_route)):
                tw = tile_width(route)
                t[:, :, (-(-width // tw) - 1) * tw:] = math.nan
        q = f'chain_k{case.K}'
        return {'y': _entry(y, case.dt, case.exact, mags['y'], q), 'dx': _entry(dx, case.dt, case.exact, mags['dx'], q)}
    pw, pb = dw_prefill(case)
    keep = 0.0 if fault == 'assign_not_add' else 1.0
    spec = {'dw': ('equal', vals['dw'] + keep * pw) if case.exact else ('bound', vals['dw'] + keep * pw, mags['dw'] + pw, 'dw', None)}
    if case.bias:
        spec['db'] = ('equal', vals['db'] + keep * pb) if case.exact else ('bound', vals['db'] + keep * pb, mags['db'] + pb, 'db', None)
    return spec


# ================================================================================================ the judge
def allowed_ratio(q):
    return FIXED[q] if q in FIXED else MARGIN * CONSTANTS[q]


def judge(got, spec, worst=None):
    """spec: {name: ('equal', ref) | ('bound', ref, bound, quantity, extra)} -> list of complaints.  'equal' is torch.equal with NaN equal
    to NaN; for 'bound' the error beyond the absolute allowance `extra` (None: none) is held to allowed * u * bound, an element whose bound
    is 0 must be exact and a NaN never passes.  worst: receives the worst ratios."""
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


def values(spec):
    """the reference values of a spec as a `got` dict (a planted fault's candidate)"""
    return {n: s[1] for n, s in spec.items()}


# ================================================================================================ fp32 emulations of the kernels' order
def emulate_conv(case, inp, wd=F32, store=None):
    """forward and data gradient tap by tap in the working precision wd (fp32: fused multiply-adds in the kernels' order), the result
    stored in the case's dtype (store: another one)"""
    dt = case.dt if store is None else store
    if wd == F32:
        y = gather_form(case, inp['x'], inp['w'], inp['b'], False, F32)
        dx = gather_form(case, inp['dy'], inp['w'], None, True, F32, descending=case.dgrad_route == 'walk')
    else:                                                   # a plain evaluation in wd (the exact regime's check): products and sums rounded to wd
        lo = {k: (None if v is None else v.to(wd)) for k, v in inp.items()}
        y = gather_form(case, lo['x'], lo['w'], lo['b'], False, wd)
        dx = gather_form(case, lo['dy'], lo['w'], None, True, wd)
    return {'y': rdt(y.to(F64), dt), 'dx': rdt(dx.to(F64), dt)}


def wgrad_partials(case, inp):
    """fp32 partial sums of dwconv_wgrad_kernel, one row per pixel range -> (dw [ranges, K * K, C], db [ranges, C]) as float32 numpy.
    A thread adds the pixels of its sub-range one after the other (fma(dy, x, acc) per tap, dy alone for the bias), then the ps == 0
    thread adds the other sub-ranges' sums in order"""
    N, H, W, C, K, s, p, d, OH, OW = case.N, case.H, case.W, case.C, case.K, case.stride, case.pad, case.dil, case.OH, case.OW
    g = case.wgrad
    ranges, nps, sub, ppb, npix = g['ranges'], g['nps'], g['sub'], g['ppb'], case.npix
    big = p + d * (K - 1) + s
    xp = torch.zeros((N, H + 2 * big, W + 2 * big, C), dtype=F32)
    xp[:, big:big + H, big:big + W] = inp['x'].to(F32)
    wins = [xp[:, big - p + r * d:big - p + r * d + (OH - 1) * s + 1:s, big - p + c * d:big - p + c * d + (OW - 1) * s + 1:s].reshape(npix, C)
            for r in range(K) for c in range(K)]
    v = torch.cat([torch.stack(wins), torch.zeros((K * K, 1, C), dtype=F32)], 1)                      # [K * K, npix + 1, C], the last row zeros
    gy = torch.cat([inp['dy'].to(F32).reshape(npix, C), torch.zeros((1, C), dtype=F32)], 0)
    b0 = torch.arange(ranges)[:, None, None] * ppb
    idx = b0 + torch.arange(nps)[None, :, None] * sub + torch.arange(sub)[None, None, :]
    idx = torch.where(idx < (b0 + ppb).clamp_max(npix), idx, torch.full_like(idx, npix))               # outside the block: the zero row
    acc = torch.zeros((K * K, ranges, nps, C), dtype=F32)
    bacc = torch.zeros((ranges, nps, C), dtype=F32)
    for k in range(sub):
        gi = gy[idx[:, :, k]]
        acc = _fma32(gi[None].expand_as(acc), v[:, idx[:, :, k]], acc)
        bacc = bacc + gi
    tot, btot = acc[:, :, 0], bacc[:, 0]
    for o in range(1, nps):
        tot, btot = tot + acc[:, :, o], btot + bacc[:, o]
    return tot.permute(1, 0, 2).contiguous().numpy(), btot.numpy()


def _fold(parts, pre, seed):
    """parts [ranges, n] float32, pre [n] -> [n] float64: fold_partials per element (one range: the one addition, vectorised)"""
    if parts.shape[0] == 1:
        return torch.from_numpy((pre.numpy().astype(np.float32) + parts[0]).astype(np.float64))
    pre = pre.numpy()
    return torch.tensor([fold_partials(parts[:, i], pre[i], seed) for i in range(parts.shape[1])], dtype=F64)


def emulate_wgrad(case, inp, seed=None, parts=None):
    """-> (got, parts): the pixel ranges folded in the order `seed` (None: the deterministic fold; else a seeded arrival order of the
    atomic form).  parts: the partials of an earlier call, to fold them again."""
    if parts is None:
        parts = wgrad_partials(case, inp)
    pw, pb = dw_prefill(case)
    got = {'dw': _fold(parts[0].reshape(parts[0].shape[0], -1), pw.reshape(-1), seed).view(case.K ** 2, case.C)}
    if case.bias:
        got['db'] = _fold(parts[1], pb, seed)
    return got, parts


def emulate(case, inp):
    """every candidate the emulation yields for a case: one for forward / data gradient, one per ORDER_SEEDS for the weight gradient"""
    if case.table != 'wgrad':
        return [emulate_conv(case, inp)]
    out, parts = [], None
    for seed in (ORDER_SEEDS if case.wgrad['ranges'] > 1 else ORDER_SEEDS[:1]):
        got, parts = emulate_wgrad(case, inp, seed, parts)
        out.append(got)
    return out


# ================================================================================================ the launchers (need a GPU)
def tap_major(w, dt, device):
    """PyTorch's [C, 1, K, K] -> the kernels' [K * K][C] in the compute dtype"""
    K = w.shape[-1]
    return _dev(w[:, 0].permute(1, 2, 0).reshape(K * K, w.shape[0]), dt, device)


def _args(case):
    return (case.N, case.H, case.W, case.C, case.OH, case.OW, case.K, case.stride, case.pad, case.dil)


def run_conv(case, inp, device='cuda'):
    """saicv_dwconv2d_fwd and saicv_dwconv2d_dgrad -> (got for judge(), complaints of the guards)"""
    _lib, L = _L()
    dt = case.dt
    code, st, P = _lib.dtype_code(TD[dt]), _lib.stream(), _lib.ptr
    x, dy, wt, b = _dev(inp['x'], dt, device), _dev(inp['dy'], dt, device), tap_major(inp['w'], dt, device), _dev(inp['b'], 'f32', device)
    y, dx = _guard((case.N, case.OH, case.OW, case.C), dt, device), _guard((case.N, case.H, case.W, case.C), dt, device)
    _lib.check(L.saicv_dwconv2d_fwd(code, P(x), P(wt), P(b), P(y.view), *_args(case), st), 'dwconv2d_fwd')
    _lib.check(L.saicv_dwconv2d_dgrad(code, P(dy), P(wt), P(dx.view), *_args(case), st), 'dwconv2d_dgrad')
    return _finish([('y', y), ('dx', dx)])


def run_wgrad(case, inp, device='cuda'):
    """saicv_dwconv2d_wgrad in the engine's current accumulation mode (atomic, or ordered under the `deterministic` fixture), into
    pre-filled targets"""
    _lib, L = _L()
    dt = case.dt
    code, st, P = _lib.dtype_code(TD[dt]), _lib.stream(), _lib.ptr
    x, dy = _dev(inp['x'], dt, device), _dev(inp['dy'], dt, device)
    pw, pb = dw_prefill(case)
    dw = GuardedFill((case.K ** 2, case.C), F32, device, pw, written=False)
    outs = [('dw', dw)]
    db = None
    if case.bias:
        db = GuardedFill((case.C,), F32, device, pb, written=False)
        outs.append(('db', db))
    _lib.check(L.saicv_dwconv2d_wgrad(code, P(dy), P(x), P(dw.view), P(db.view) if db else None, *_args(case), st), 'dwconv2d_wgrad')
    return _finish(outs)
