"""What tests/test_detloss_judge_host.py (no GPU) and tests/test_gpu_detloss_f64.py (MI355X) share for csrc/detloss.hip: the case
tables of saicv_retina_assign, saicv_fcos_assign, saicv_focal_loss_level, saicv_smoothl1_level, saicv_det_best_class and
saicv_detr_box_loss_fwd / _bwd, the input builders, the float64 references with hand-written gradients and planted faults, the
working-precision emulations that set the constants, the judge, and the launchers (C-ABI, outputs in guarded allocations).

Two regimes.
  exact     inputs on which fp32 holds every intermediate exactly (integer corners and areas below 2^24; FCOS points at
            stride * (i + 1/2) against integer boxes with corners <= 256; SmoothL1 operands in eighths with beta = 1/2; DETR boxes in
            64ths).  The reference is float64; where the kernel makes ONE correctly rounded fp32 operation on exact operands (the IoU
            quotient, the FCOS distance) the reference rounds its float64 result once to fp32 -- the IEEE result, 53 >= 2 * 24 + 2.
            Decisions, copied values, counts and dyadic sums are compared with torch.equal, nothing left out.
  accuracy  random fp32 inputs; an element passes when |got - ref| <= MARGIN * c * u * bound, u = 2^-24, bound the magnitude sum of
            the element's own expression in float64, c = CONSTANTS[quantity]: the worst ratio of a CPU fp32 emulation over the whole
            case table (the host test measures and holds it); for the loss sums over the index order of the deterministic fold AND
            eight seeded random workgroup orders, since the atomic form adds the workgroups' partials as they arrive and the error of
            a sequential fp32 sum of 4 096 partials is a random walk of which one order is one draw.  Decisions on random real coordinates are compared with the unrounded
            float64 ones; an anchor / point is left out only when a decision of its own lies within k * u (relative) of its
            threshold or its two best candidates within k * u of each other, k = 4 x the worst fp32-vs-float64 error of that quantity
            on that case, and at most LEFT_OUT_CAP of a case may be left out.

Bounds.   sums of non-negative terms: the sum (plus the pre-fill).  focal gradient: w (gamma max(1, (1-q)^(gamma-1)) |log q| + 1/q),
every factor in [0, 1] replaced by 1 (1 - q carries an absolute error of u in fp32).  RetinaNet tx, ty: (|gcx| + |cx|) / w; tw, th:
1 + |log(gw / w)|.  FCOS centre-ness and the decoder's sqrt(p * centre-ness): four correctly rounded operations, 3 u ref, derived not
measured.  DETR: magnitude sums of the L1 / GIoU expressions and of the reverse-mode products (giou_backward(mag=True)).

One listed fault has no observable value: SmoothL1 with `>` instead of `>=` at |d| == beta.  Both branches give the term beta / 2 and
the gradient +-1 there (the function is C1 at beta), so the planted |d| == beta elements pin the VALUE at the boundary and the fault
`gt_at_beta` is kept in NEUTRAL_FAULTS: the host test asserts that it changes nothing, which is why no case can miss it.
"""
import math
from dataclasses import dataclass

import numpy as np
import torch

from attn_common import GUARD, MARGIN, SENTINEL, U, Guarded

F32, F64 = torch.float32, torch.float64
UF = U[F32]
DL_THREADS, DL_MAX_GT, DL_GRID_CAP = 256, 1024, 4096
LO = float(np.float32(1e-4))                               # the clamp of the focal loss as the kernel holds it
HI = float(np.float32(1.0) - np.float32(1e-4))             # `1.f - 1e-4f`, evaluated in fp32
T04, T05 = float(np.float32(0.4)), 0.5
POS_PREFILL, SUM_PREFILL = 5.0, 3.0
LEFT_OUT_CAP = 0.005

# Worst ratio of the fp32 emulations to the float64 references over every case of the tables, in units of u * bound.
# Measured by tests/test_detloss_judge_host.py::test_constants_table_is_what_the_emulations_measure (which fails if a row drifts by
# more than a quarter, on one thread); the judge allows MARGIN times these.  Never raised by hand.
CONSTANTS = {
    'retina_txy': 0.971, 'retina_twh': 0.999, 'focal_sum': 29.4, 'focal_grad_g2': 2.71, 'focal_grad_g1.5': 2.64, 'focal_grad_g1': 2.47,
    'focal_grad_g0.5': 20.8, 'smoothl1_sum': 29.8, 'smoothl1_grad': 1.76, 'detr_l1': 0.780, 'detr_iou': 2.06, 'detr_grad': 1.80,
}
CONSTANTS_MEASURED_WITH = 'torch 2.10.0+rocm7.0 (CPU, one thread), 2026-10-19'
FIXED = {'chain4': 3.0}                                     # derived: |got - ref| <= 3 u ref for four correctly rounded operations


def dl_grid(items):
    """dl_grid() of csrc/detloss.hip restated"""
    return int(min(max((items + DL_THREADS - 1) // DL_THREADS, 1), DL_GRID_CAP))


def r32(x):
    """one rounding to fp32 (of a float64 tensor), kept as float64"""
    return x.to(F32).to(F64)


def _gen(name):
    return torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31))


def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi, shape, generator=g).to(F64)


# ------------------------------------------------------------------------------------------------ the judge
def judge(got, spec, worst=None):
    """spec: {name: ('equal', ref[, keep]) | ('bound', ref, bound, quantity) | ('fixed', ref, bound, key)} -> list of complaints.
    'equal' is torch.equal (over the kept elements when a keep mask is given); for 'bound' / 'fixed' an element whose bound is 0 must
    be exact and a NaN never passes.  worst: dict that receives the worst ratio per quantity."""
    bad = []
    for name, (kind, ref, *rest) in spec.items():
        g = got[name].detach().to(F64).cpu().reshape(ref.shape)
        if kind == 'equal':
            if rest and rest[0] is not None:
                g, ref = g[rest[0]], ref[rest[0]]
            same = torch.equal(g, ref) or (g.shape == ref.shape and bool(((g == ref) | (torch.isnan(g) & torch.isnan(ref))).all()))
            if not same:
                n = int(((g != ref) & ~(torch.isnan(g) & torch.isnan(ref))).sum())
                bad.append(f'{name}: {n} of {ref.numel()} elements differ (exact comparison)')
            continue
        bnd, q = rest
        b = bnd.abs() * UF
        err = (g - ref).abs()
        ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
        ratio = torch.where(torch.isnan(g) | torch.isnan(err), torch.full_like(ratio, math.inf), ratio)
        r = float(ratio.max()) if ratio.numel() else 0.0
        if worst is not None:
            worst[q] = max(worst.get(q, 0.0), r)
        allowed = FIXED[q] if kind == 'fixed' else MARGIN * CONSTANTS[q]
        if not r <= allowed:
            bad.append(f'{name}: worst ratio {r:.4g} u*bound > {allowed:.4g} ({q}), {int((ratio > allowed).sum())} elements')
    return bad


def values(spec):
    """the reference values of a spec as a `got` dict (a planted fault's candidate)"""
    return {n: s[1] for n, s in spec.items()}


# ================================================================================================ retina_assign
RETINA_FAULTS = ('iou_tie_last', 'le_at_04', 'gt_at_05', 'padding_kept', 'assign_not_add', 'last_block_dropped')


@dataclass(frozen=True)
class RetinaCase:
    id: str
    A: int
    B: int
    G: int
    smoothl1: int
    exact: bool = True


def _retina_table():
    c, i = [], 0
    for A in (1, 255, 256, 257, 3001):
        for G in (0, 1, 37, 1024):
            for s in (0, 1):
                B = (1, 3)[(i // 2 + i) % 2]
                c.append(RetinaCase(f'exact-a{A}-b{B}-g{G}-s{s}', A, B, G, s))
                i += 1
    c += [RetinaCase(f'random-a{A}-b{B}-g{G}-s{s}', A, B, G, s, exact=False)
          for (A, B, G, s) in ((257, 3, 37, 0), (3001, 1, 37, 1), (3001, 3, 37, 0), (255, 1, 1024, 1))]
    return tuple(c)


RETINA_CASES = _retina_table()

# valid ground-truth rows planted in image 0 (x1, y1, x2, y2, class) and the anchors that meet them
_RG = ((0, 0, 10, 10, 3), (0, 0, 10, 10, 5), (50, 50, 50, 60, 1), (100, 100, 120, 110, 2), (140, 100, 150, 110, 6), (150, 100, 160, 110, 0))
RETINA_PLANTED = {                       # name: (anchor, expected class target, expected copied box target)
    'iou_half': ((0, 0, 10, 20), 4, (0, 0, 10, 10)),
    'iou_one_tied_classes': ((0, 0, 10, 10), 4, (0, 0, 10, 10)),
    'iou_two_fifths': ((0, 0, 10, 25), -1, (0, 0, 10, 10)),
    'iou_zero_everywhere': ((200, 200, 210, 210), 0, (0, 0, 10, 10)),
    'iou_third_tied_boxes': ((145, 100, 155, 110), 0, (140, 100, 150, 110)),
    'iou_one': ((100, 100, 120, 110), 3, (100, 100, 120, 110)),
    'beside_zero_area_box': ((50, 50, 52, 60), 0, (0, 0, 10, 10)),
}


def _far_boxes(g, n, real):
    xy = _randint(g, 256, 900, (n, 2))
    wh = _randint(g, 8, 200, (n, 2))
    if real:
        xy, wh = xy + torch.rand(n, 2, generator=g, dtype=F64), wh + torch.rand(n, 2, generator=g, dtype=F64)
    cls = _randint(g, 0, 80, (n, 1))
    return r32(torch.cat([xy, xy + wh, cls], 1))


def retina_inputs(case):
    """-> {'anchors': [A, 4], 'annots': [B, G, 5] or None (G = 0: the null pointer)} float64 tensors of fp32 values"""
    g = _gen(case.id)
    A, B, G = case.A, case.B, case.G
    annots = None
    if G:
        annots = torch.full((B, G, 5), -1.0, dtype=F64)
        planted = torch.tensor(_RG, dtype=F64)
        for b in range(B):
            if G == 1:
                if b != 1:
                    annots[b, 0] = planted[0] if case.exact else _far_boxes(g, 1, True)[0]
                continue                               # image 1: one padding row
            if G < DL_MAX_GT and b == 1:
                continue                               # an image of only padding rows
            rows = _far_boxes(g, G, not case.exact)
            if case.exact:
                head = planted if b == 0 else planted[[1, 0, 2, 3, 5, 4]]
                if G == DL_MAX_GT:                     # every row valid: LDS filled completely
                    rows[:6] = head
                else:                                  # padding first, in the middle and last
                    rows[0:2] = -1.0
                    rows[2:4] = head[0:2]
                    rows[4] = -1.0
                    rows[5:9] = head[2:6]
                    rows[12] = -1.0
                    rows[G - 2:] = -1.0
            elif G < DL_MAX_GT:
                rows[[0, 7, G - 1]] = -1.0
            annots[b] = rows
    pl = torch.tensor([v[0] for v in RETINA_PLANTED.values()], dtype=F64)
    if not case.exact:
        pl = pl[:0]
    if A == 1 and case.exact:
        anchors = pl[:1].clone()
    else:
        n = A - min(A, pl.shape[0])
        xy = _randint(g, 250, 900, (n, 2))
        wh = _randint(g, 4, 160, (n, 2))
        if not case.exact:
            xy, wh = xy + torch.rand(n, 2, generator=g, dtype=F64), wh + torch.rand(n, 2, generator=g, dtype=F64)
        rnd = torch.cat([xy, xy + wh], 1)
        if annots is not None and n:                   # every other random anchor sits near a ground-truth box: positives exist
            src = annots[0][annots[0][:, 4] >= 0][:, :4]
            pick = src[torch.randint(0, src.shape[0], (n,), generator=g)]
            jit = _randint(g, -6, 7, (n, 4)) + (0 if case.exact else torch.rand(n, 4, generator=g, dtype=F64))
            near = pick + jit
            near[:, 2:] = torch.maximum(near[:, 2:], near[:, :2] + 1)
            rnd[::2] = near[::2]
        anchors = torch.cat([pl[:min(A, pl.shape[0])], rnd], 0)
    return {'anchors': r32(anchors), 'annots': annots}


def _iou_matrix(an, gt, wd=F64):
    """[A, n] IoU as retina_assign_kernel writes it, in the precision wd"""
    an, gt = an.to(wd), gt.to(wd)
    zero = torch.zeros((), dtype=wd)
    ax1, ay1, ax2, ay2 = (an[:, j, None] for j in range(4))
    gx1, gy1, gx2, gy2 = (gt[None, :, j] for j in range(4))
    a_area = torch.maximum(ax2 - ax1, zero) * torch.maximum(ay2 - ay1, zero)
    ow = torch.maximum(torch.minimum(ax2, gx2) - torch.maximum(ax1, gx1), zero)
    oh = torch.maximum(torch.minimum(ay2, gy2) - torch.maximum(ay1, gy1), zero)
    overlap = ow * oh
    g_area = torch.maximum(gx2 - gx1, zero) * torch.maximum(gy2 - gy1, zero)
    uni = torch.maximum(a_area + g_area - overlap, torch.tensor(LO, dtype=wd))
    return overlap / uni


def _box_targets(an, gb, wd=F64, bounds=False):
    """snap_annotations_to_txtytwth in the precision wd -> [A, 4] (and the bounds of the docstring)"""
    an, gb = an.to(wd), gb.to(wd)
    wh = an[:, 2:] - an[:, :2]
    ctr = an[:, :2] + 0.5 * wh
    gwh = torch.clamp(gb[:, 2:] - gb[:, :2], min=LO)
    gctr = gb[:, :2] + 0.5 * gwh
    t = torch.cat([(gctr - ctr) / wh, torch.log(gwh / wh)], 1)
    if not bounds:
        return t
    return t, torch.cat([(gctr.abs() + ctr.abs()) / wh, 1 + torch.log(gwh / wh).abs()], 1)


def retina_reference(case, inp, fault=None, emulate=False):
    """-> (spec for judge(), aux).  aux: 'best' / 'second' [B, A] float64 IoUs, 'iou_err' the worst relative fp32 error of an IoU in u,
    'left_out' [B, A] (accuracy regime only).  emulate: box targets in fp32 (the constants' candidate)."""
    A, B = case.A, case.B
    an = inp['anchors']
    cls = torch.full((B, A), -1.0, dtype=F64)
    box = torch.full((B, A, 4), -1.0, dtype=F64)
    bnd = torch.zeros((B, A, 4), dtype=F64)
    best_all, second_all = torch.full((B, A), -1.0, dtype=F64), torch.full((B, A), -1.0, dtype=F64)
    iou_err = 0.0
    for b in range(B):
        if inp['annots'] is None:
            continue
        rows = inp['annots'][b]
        gt = rows if fault == 'padding_kept' else rows[rows[:, 4] >= 0]
        if gt.shape[0] == 0:
            continue
        iou = _iou_matrix(an, gt)
        if case.exact:
            iou = r32(iou)
        else:
            i32 = _iou_matrix(an, gt, F32).to(F64)
            iou_err = max(iou_err, float(((i32 - iou).abs() / iou.clamp_min(1e-300))[iou > 0].max() / UF) if bool((iou > 0).any()) else 0.0)
        if fault == 'iou_tie_last':
            best, bi = iou.flip(1).max(1)
            bi = gt.shape[0] - 1 - bi
        else:
            best, bi = iou.max(1)                       # first maximum
        if gt.shape[0] > 1:
            second_all[b] = iou.scatter(1, bi[:, None], -1.0).max(1)[0]
        best_all[b] = best
        c = torch.full((A,), -1.0, dtype=F64)
        c[(best <= T04) if fault == 'le_at_04' else (best < T04)] = 0.0
        pos = (best > T05) if fault == 'gt_at_05' else (best >= T05)
        c[pos] = gt[bi, 4][pos] + 1.0
        cls[b] = c
        if case.smoothl1:
            if emulate:
                box[b] = _box_targets(an, gt[bi, :4], F32).to(F64)
            else:
                box[b], bnd[b] = _box_targets(an, gt[bi, :4], bounds=True)
        else:
            box[b] = gt[bi, :4]
    pos_count = float((cls > 0).sum()) + (0.0 if fault == 'assign_not_add' else POS_PREFILL)
    if fault == 'last_block_dropped' and A % DL_THREADS:
        tail = slice((A // DL_THREADS) * DL_THREADS, A)
        pos_count -= float((cls[:, tail] > 0).sum())
        cls[:, tail] = math.nan
        box[:, tail] = math.nan
    keep = None
    aux = {'best': best_all, 'second': second_all, 'iou_err': iou_err}
    if not case.exact:
        k = 4.0 * max(iou_err, 1.0) * UF
        near = ((best_all - T04).abs() <= k * T04) | ((best_all - T05).abs() <= k * T05)
        near |= (best_all > 0) & ((best_all - second_all) <= k * best_all)
        aux['left_out'] = near
        keep = ~near
    spec = {'cls': ('equal', cls, keep)}
    if case.smoothl1:
        k4 = None if keep is None else keep[:, :, None].expand(B, A, 4)
        ref, bd = (box, bnd) if k4 is None else (torch.where(k4, box, torch.zeros_like(box)), torch.where(k4, bnd, torch.full_like(bnd, math.inf)))
        spec['box_xy'] = ('bound', ref[..., :2], bd[..., :2], 'retina_txy')
        spec['box_wh'] = ('bound', ref[..., 2:], bd[..., 2:], 'retina_twh')
    else:
        spec['box'] = ('equal', box, None if keep is None else keep[:, :, None].expand(B, A, 4))
    if keep is None or bool(keep.all()):
        spec['pos'] = ('equal', torch.tensor([pos_count], dtype=F64))
    return spec, aux


def retina_split(targets, pos, case):
    """the kernel's [B, A, 5] targets and pos_count as the names of the spec"""
    t = targets.detach().to(F64).cpu()
    got = {'cls': t[..., 4], 'pos': pos.detach().to(F64).cpu().reshape(1)}
    if case.smoothl1:
        got['box_xy'], got['box_wh'] = t[..., 0:2], t[..., 2:4]
    else:
        got['box'] = t[..., :4]
    return got


# ================================================================================================ fcos_assign
FCOS_FAULTS = ('inside_nonstrict', 'range_closed', 'radius_nonstrict', 'largest_area', 'equal_area_last', 'padding_kept', 'assign_not_add',
               'last_block_dropped')
FCOS_STRIDES = (8, 16, 32, 64, 128)
FCOS_RANGES = {'default': ((-1, 64), (64, 128), (128, 256), (256, 512), (512, 100000000)),
               'second': ((-1, 24), (24, 48), (48, 96), (96, 160), (160, 100000000))}
FCOS_RADIUS = 1.5


@dataclass(frozen=True)
class FcosCase:
    id: str
    P: int
    B: int
    G: int
    center_sample: int
    ranges: str = 'default'
    exact: bool = True


def _fcos_table():
    c, i = [], 0
    for P in (1, 255, 256, 257, 3001):
        for G in (0, 1, 37, 1024):
            for cs in (0, 1):
                B = (1, 3)[(i // 2 + i) % 2]
                rg = 'second' if (i % 4 == 3 and P > 1) else 'default'
                c.append(FcosCase(f'exact-p{P}-b{B}-g{G}-cs{cs}-{rg}', P, B, G, cs, rg))
                i += 1
    c += [FcosCase('exact-p3001-b3-g37-cs1-second', 3001, 3, 37, 1, 'second'), FcosCase('exact-p257-b1-g37-cs0-second', 257, 1, 37, 0, 'second')]
    c += [FcosCase(f'random-p{P}-b{B}-g{G}-cs{cs}-{rg}', P, B, G, cs, rg, exact=False)
          for (P, B, G, cs, rg) in ((257, 3, 37, 1, 'default'), (3001, 1, 37, 0, 'second'), (3001, 3, 37, 1, 'second'), (255, 1, 1024, 1, 'default'))]
    return tuple(c)


FCOS_CASES = _fcos_table()

# boxes planted in image 0 (default ranges; stride-8 points sit at 4 mod 8, stride-16 points at 8 mod 16)
_FG = ((12, 2, 22, 22, 1),            # 0  point (12, 12): l == 0
       (30, 2, 44, 22, 2),            # 1  point (44, 12): r == 0
       (68, 64, 108, 88, 3),          # 2  centre (88, 76): point (100, 76) is exactly 12 = 8 * 1.5 away
       (4, 135, 118, 145, 4),         # 3  point (68, 140): l == 64 == m1 of stride 8
       (8, 194, 130, 206, 5),         # 4  point (72, 200) of stride 16: l == 64 == m0
       (130, 2, 190, 62, 6),          # 5  outer, then
       (150, 22, 170, 42, 7),         # 6  inner: point (156, 28)
       (214, 22, 234, 42, 8),         # 7  inner, then
       (194, 2, 254, 62, 9),          # 8  outer: point (220, 28)
       (130, 70, 150, 90, 10),        # 9  equal areas (400): point (140, 76), the first wins
       (132, 72, 152, 92, 11),        # 10
       (130, 100, 250, 250, 12))      # 11 point (188, 172) of stride 8: inside, near the centre, largest side 78 > 64
FCOS_PLANTED = {                      # name: (x, y, stride index, expected class target under the default ranges)
    'l_zero': (12, 12, 0, 0), 'r_zero': (44, 12, 0, 0), 'dist_at_radius': (100, 76, 0, 0), 'side_at_m1': (68, 140, 0, 0),
    'side_at_m0': (72, 200, 1, 0), 'nested_outer_first': (156, 28, 0, 8), 'nested_inner_first': (220, 28, 0, 9),
    'equal_area': (140, 76, 0, 11), 'all_fail_range': (188, 172, 0, 0), 'inside_padding_box': (76, 116, 0, 0),
}
FCOS_PADDING_BOX = (60, 100, 90, 130, -1)       # the padding row in the middle holds a real box: class < 0 alone makes a row padding
# what each planted point becomes under the fault that it guards against (centre sampling on or off, default ranges)
FCOS_PLANTED_FAULT = {'l_zero': ('inside_nonstrict', 2), 'r_zero': ('inside_nonstrict', 3), 'dist_at_radius': ('radius_nonstrict', 4),
                      'side_at_m1': ('range_closed', 5), 'side_at_m0': ('range_closed', 6), 'nested_outer_first': ('largest_area', 7),
                      'nested_inner_first': ('largest_area', 10), 'equal_area': ('equal_area_last', 12)}


def fcos_points(case):
    """[P, 5] = (x, y, stride, m0, m1): the planted points first, then the pyramid of a 256 x 256 image level after level, repeated"""
    rg = FCOS_RANGES[case.ranges]
    rows = [(x, y, FCOS_STRIDES[s], rg[s][0], rg[s][1]) for (x, y, s, _) in FCOS_PLANTED.values()] if case.exact else []
    pyr = []
    for s, (m0, m1) in zip(FCOS_STRIDES, rg):
        n = 256 // s
        pyr += [((i + 0.5) * s, (j + 0.5) * s, s, m0, m1) for j in range(n) for i in range(n)]
    while len(rows) < case.P:
        rows += pyr
    pts = torch.tensor(rows[:case.P], dtype=F64)
    if not case.exact:
        g = _gen(case.id + 'points')
        pts[:, :2] = r32(pts[:, :2] + torch.rand(case.P, 2, generator=g, dtype=F64) * 3 - 1.5)
    return pts


def fcos_inputs(case):
    """-> {'points': [P, 5], 'annots': [B, G, 5] or None}"""
    g = _gen(case.id)
    B, G = case.B, case.G
    annots = None
    if G:
        annots = torch.full((B, G, 5), -1.0, dtype=F64)
        planted = torch.tensor(_FG, dtype=F64)
        for b in range(B):
            if G == 1:
                if b != 1:
                    annots[b, 0] = planted[6] if case.exact else torch.tensor([100.3, 90.7, 171.9, 160.2, 4.0], dtype=F64)
                continue
            if G < DL_MAX_GT and b == 1:
                continue
            # fillers: boxes that hold no point of any level (every point coordinate is a multiple of 4), and real candidates
            k = _randint(g, 0, 31, (G, 2)) * 8
            rows = torch.cat([k + 5, k + 7, _randint(g, 0, 80, (G, 1))], 1)
            real = torch.rand(G, generator=g) < 0.3
            xy = torch.cat([_randint(g, 0, 88, (G, 1)), _randint(g, 208, 240, (G, 1))], 1)      # a corner no planted point lies in
            wh = _randint(g, 6, 40, (G, 2))
            cand = torch.cat([xy, torch.minimum(xy + wh, torch.tensor(256.0, dtype=F64)), rows[:, 4:]], 1)
            rows = torch.where(real[:, None], cand, rows)
            if not case.exact:
                xy = torch.rand(G, 2, generator=g, dtype=F64) * 200
                wh = torch.rand(G, 2, generator=g, dtype=F64) * 120 + 4
                rows = torch.cat([xy, xy + wh, rows[:, 4:]], 1)
                if G < DL_MAX_GT:
                    rows[[0, 7, G - 1]] = -1.0
            else:
                head = planted if b == 0 else planted[[1, 0, 2, 3, 4, 6, 5, 8, 7, 10, 9, 11]]
                if G == DL_MAX_GT:
                    rows[:12] = head
                else:
                    rows[0:2] = -1.0
                    rows[2:8] = head[0:6]
                    rows[8] = torch.tensor(FCOS_PADDING_BOX, dtype=F64)
                    rows[9:15] = head[6:12]
                    rows[G - 2:] = -1.0
            annots[b] = r32(rows)
    return {'points': fcos_points(case), 'annots': annots}


def fcos_exactness(inp):
    """the exactness premises of the exact regime, in float64: every intermediate of the membership tests equals its fp32 rounding"""
    p, ok = inp['points'], True
    if inp['annots'] is None:
        return True
    for rows in inp['annots']:
        gt = rows[rows[:, 4] >= 0]
        x, y = p[:, 0, None], p[:, 1, None]
        cx, cy = (gt[None, :, 2] + gt[None, :, 0]) / 2, (gt[None, :, 3] + gt[None, :, 1]) / 2
        dx, dy = x - cx, y - cy
        for t in (x - gt[None, :, 0], gt[None, :, 2] - x, y - gt[None, :, 1], gt[None, :, 3] - y, cx, cy, dx, dy, dx * dx, dy * dy,
                  dx * dx + dy * dy, (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1]), p[:, 2] * FCOS_RADIUS):
            ok = ok and torch.equal(r32(t), t)
    return ok


def fcos_reference(case, inp, fault=None, wd=F64):
    """-> (spec, aux).  wd = F32: every operation in fp32 (the decisions' emulation, for the measured decision errors)."""
    P, B = case.P, case.B
    pts = inp['points'].to(wd)
    ltrb = torch.zeros((B, P, 4), dtype=F64)
    cls = torch.zeros((B, P), dtype=F64)
    ctr = torch.zeros((B, P), dtype=F64)
    near_all = torch.zeros((B, P), dtype=torch.bool)
    err = {'dist': 0.0, 'area': 0.0}
    x, y, stride, m0, m1 = (pts[:, j, None] for j in range(5))
    exact = case.exact and wd == F64
    rnd = r32 if exact else (lambda t: t)
    judge_d = rnd(stride * torch.tensor(np.float32(FCOS_RADIUS), dtype=wd))
    for b in range(B):
        if inp['annots'] is None:
            continue
        rows = inp['annots'][b].to(wd)
        gt = rows if fault == 'padding_kept' else rows[rows[:, 4] >= 0]
        n = gt.shape[0]
        if n == 0:
            continue
        x1, y1, x2, y2 = (gt[None, :, j] for j in range(4))
        l, t, r, bt = x - x1, y - y1, x2 - x, y2 - y
        mn = torch.minimum(torch.minimum(l, t), torch.minimum(r, bt))
        ok = (mn >= 0) if fault == 'inside_nonstrict' else (mn > 0)
        near = torch.zeros_like(ok)
        k = 0.0
        if not case.exact and wd == F64:               # the measured fp32 error of the quantities that decide
            f, d = fcos_quantities(inp['points'], gt, F32), fcos_quantities(inp['points'], gt, F64)
            for q in ('dist', 'area'):         # the distance against the threshold it may cross, the area against itself
                scale = judge_d.to(F64).expand_as(d[q]) if q == 'dist' else d[q].abs().clamp_min(1e-300)
                e = (f[q].to(F64) - d[q]).abs() / scale
                if q == 'dist':
                    e = e[d[q] <= 2 * scale]
                e = float(e.max() / UF) if e.numel() else 0.0
                err[q] = max(err[q], e)
            k = 4.0 * max(err['dist'], err['area'], 1.0) * UF
        if case.center_sample:
            cx, cy = (x2 + x1) / 2, (y2 + y1) / 2
            dx, dy = x - cx, y - cy
            dist = rnd(torch.sqrt(dx * dx + dy * dy))
            ok &= (dist <= judge_d) if fault == 'radius_nonstrict' else (dist < judge_d)
            near |= (dist - judge_d).abs() <= k * judge_d
        mx = torch.maximum(torch.maximum(l, t), torch.maximum(r, bt))
        ok &= ((mx >= m0) & (mx <= m1)) if fault == 'range_closed' else ((mx > m0) & (mx < m1))
        near |= ((mx - m0).abs() <= k * m0.abs()) | ((mx - m1).abs() <= k * m1.abs())
        area = ((x2 - x1) * (y2 - y1)).expand(P, n)
        inf = torch.full_like(area, math.inf)
        if fault == 'largest_area':
            gi = torch.where(ok, area, -inf).max(1)[1]
        elif fault == 'equal_area_last':
            gi = n - 1 - torch.where(ok, area, inf).flip(1).min(1)[1]
        else:
            masked = torch.where(ok, area, inf)
            gi = masked.min(1)[1]                       # first minimum
            if k:
                two = masked.topk(min(2, n), dim=1, largest=False)[0]
                if n > 1:
                    near_pt = near.any(1) | (torch.isfinite(two[:, 1]) & ((two[:, 1] - two[:, 0]) <= k * two[:, 0].abs()))
                else:
                    near_pt = near.any(1)
                near_all[b] = near_pt
        found = ok.any(1)
        idx = torch.arange(P)
        sel = torch.stack([l[idx, gi], t[idx, gi], r[idx, gi], bt[idx, gi]], 1).to(F64)
        sel = torch.where(found[:, None], r32(sel), torch.zeros_like(sel))
        ltrb[b] = sel
        cls[b] = torch.where(found, gt[gi, 4].to(F64) + 1.0, torch.zeros((), dtype=F64))
        ll, tt, rr, bb = sel.unbind(1)
        c = torch.sqrt(torch.minimum(ll, rr) / torch.maximum(ll, rr) * torch.minimum(tt, bb) / torch.maximum(tt, bb))
        ctr[b] = torch.where(found, c, torch.zeros_like(c))
    pos_count = float((cls > 0).sum()) + (0.0 if fault == 'assign_not_add' else POS_PREFILL)
    if fault == 'last_block_dropped' and P % DL_THREADS:
        tail = slice((P // DL_THREADS) * DL_THREADS, P)
        pos_count -= float((cls[:, tail] > 0).sum())
        cls[:, tail], ltrb[:, tail], ctr[:, tail] = math.nan, math.nan, math.nan
    keep = None
    aux = {'err': err}
    if not case.exact:
        aux['left_out'] = near_all
        keep = ~near_all
    spec = {'cls': ('equal', cls, keep), 'ltrb': ('equal', ltrb, None if keep is None else keep[:, :, None].expand(B, P, 4))}
    if keep is None:
        spec['ctr'] = ('fixed', ctr, ctr, 'chain4')
    else:
        spec['ctr'] = ('fixed', torch.where(keep, ctr, torch.zeros_like(ctr)), torch.where(keep, ctr, torch.full_like(ctr, math.inf)), 'chain4')
    if keep is None or bool(keep.all()):
        spec['pos'] = ('equal', torch.tensor([pos_count], dtype=F64))
    return spec, aux


def fcos_quantities(points, gt, wd):
    """the distance to the centre and the area of every (point, box) pair in the precision wd"""
    p, gt = points.to(wd), gt.to(wd)
    x, y = p[:, 0, None], p[:, 1, None]
    cx, cy = (gt[None, :, 2] + gt[None, :, 0]) / 2, (gt[None, :, 3] + gt[None, :, 1]) / 2
    dx, dy = x - cx, y - cy
    return {'dist': torch.sqrt(dx * dx + dy * dy), 'area': ((gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1]))[None, :].expand(p.shape[0], -1)}


def fcos_split(targets, centerness, pos):
    t = targets.detach().to(F64).cpu()
    return {'cls': t[..., 4], 'ltrb': t[..., :4], 'ctr': centerness.detach().to(F64).cpu(), 'pos': pos.detach().to(F64).cpu().reshape(1)}


# ================================================================================================ the partition of the level sums
ORDER_SEEDS = (None, 1, 2, 3, 4, 5, 6, 7, 8)       # workgroup orders the constants of the sums are measured over (None: index order)


def workgroup_partials(terms, per_item=1):
    """fp32 partial sums of `terms` (float32 numpy, [items * per_item]), one per workgroup, in the partition of focal_level_kernel /
    smoothl1_level_kernel: per-thread grid-strided partials (an item's per_item terms one after the other), 64 lanes by xor butterfly,
    the 4 waves in order."""
    t = np.asarray(terms, dtype=np.float32).reshape(-1, per_item)
    items = t.shape[0]
    grid = dl_grid(items)
    span = grid * DL_THREADS
    K = (items + span - 1) // span
    pad = np.zeros((K * span, per_item), dtype=np.float32)
    pad[:items] = t
    pad = pad.reshape(K, grid, DL_THREADS, per_item)
    acc = np.zeros((grid, DL_THREADS), dtype=np.float32)
    for k in range(K):
        for j in range(per_item):
            acc = acc + pad[k, :, :, j]
    v = acc.reshape(grid, DL_THREADS // 64, 64)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lanes ^ o]
    tot = np.zeros(grid, dtype=np.float32)
    for w in range(DL_THREADS // 64):
        tot = tot + v[:, w, 0]
    return tot


def fold_partials(parts, prefill, seed=None):
    """the workgroups' partials added one after the other in fp32.  seed None: in index order onto 0, the total then added to the
    pre-fill (the deterministic fold, det.h).  A seed: in a seeded random order straight onto the pre-fill -- one of the orders in
    which the atomic form's workgroups may arrive.  A workgroup whose total is 0 adds nothing."""
    parts = parts[parts != 0]
    if seed is None:
        s = np.float32(0.0)
        for part in parts:
            s = np.float32(s + part)
        return float(np.float32(np.float32(prefill) + s))
    s = np.float32(prefill)
    for part in parts[np.random.RandomState(seed).permutation(parts.size)]:
        s = np.float32(s + part)
    return float(s)


def kernel_order_sum(terms, prefill, per_item=1, seed=None):
    return fold_partials(workgroup_partials(terms, per_item), prefill, seed)


def _drop(flat_len, fault, per_block_items=DL_THREADS):
    """bool [items]: the items a 'last_block_dropped' / 'remainder_dropped' fault loses"""
    lost = torch.zeros(flat_len, dtype=torch.bool)
    if fault == 'last_block_dropped' and flat_len % DL_THREADS:
        lost[(flat_len // DL_THREADS) * DL_THREADS:] = True
    if fault == 'remainder_dropped':
        lost[dl_grid(flat_len) * DL_THREADS:] = True
    return lost


# ================================================================================================ focal_loss_level
FOCAL_FAULTS = ('open_clamp_mask', 'ignored_counted', 'offset_dropped', 'last_block_dropped', 'remainder_dropped', 'assign_not_add')
GAMMAS = (2.0, 1.5, 1.0, 0.5)


@dataclass(frozen=True)
class FocalCase:
    id: str
    B: int
    Al: int
    At: int
    off: int
    C: int
    gamma: float
    alpha: float = 0.25
    grad: bool = True

    @property
    def total(self):
        return self.B * self.Al * self.C

    @property
    def gq(self):
        return f'focal_grad_g{self.gamma:g}'


def _focal_table():
    c = []
    shapes = ((1, 1, 1, 0), (2, 37, 50, 5), (3, 100, 260, 160), (1, 211, 300, 89))
    for i, C in enumerate((1, 7, 80, 91)):
        for j, gamma in enumerate(GAMMAS):
            B, Al, At, off = shapes[(i + j) % 4]
            c.append(FocalCase(f'c{C}-g{gamma:g}-b{B}-al{Al}-at{At}-off{off}', B, Al, At, off, C, gamma, alpha=(0.25, 0.3)[j % 2],
                               grad=(i * 4 + j) % 5 != 4))
    c += [FocalCase(f'edge-total{n}', 1, n, n + 3, 2, 1, 2.0) for n in (255, 256, 257)]
    c += [FocalCase('edge-c7-total259', 1, 37, 37, 0, 7, 1.5)]
    c += [FocalCase('cap-c80-g2', 1, 13109, 13200, 91, 80, 2.0), FocalCase('cap-c80-g1.5', 1, 13109, 13109, 0, 80, 1.5),
          FocalCase('cap-c7-g0.5-nograd', 2, 74899, 74900, 1, 7, 0.5, grad=False), FocalCase('cap-c91-g1', 3, 3841, 4000, 100, 91, 1.0)]
    return tuple(c)


FOCAL_CASES = _focal_table()
_NEXT = lambda v, d: float(np.nextafter(np.float32(v), np.float32(d)))      # noqa: E731
# (probability, hot?) planted on rows 0 .. 8 of image 0 when the level has at least 12 rows; rows 9 .. 11 get classes -1, C and 1
FOCAL_PLANTED = ((LO, True), (HI, True), (_NEXT(LO, 0), True), (_NEXT(HI, 1), False), (0.0, True), (1.0, False),
                 (float(np.float32(2e-5)), True), (LO, False), (HI, False))


def focal_inputs(case):
    """-> {'probs': [B, Al, C], 'targets': [B, At, 5]} (the other levels' rows carry classes of their own)"""
    g = _gen(case.id)
    B, Al, At, C = case.B, case.Al, case.At, case.C
    probs = r32(torch.rand(B, Al, C, generator=g, dtype=F64) * 0.998 + 0.001)
    targets = r32(torch.rand(B, At, 5, generator=g, dtype=F64))
    targets[:, :, 4] = _randint(g, -1, C + 1, (B, At))
    if Al >= 12:
        for j, (p, hot) in enumerate(FOCAL_PLANTED):
            col = j % C
            probs[0, j, col] = p
            targets[0, case.off + j, 4] = col + 1 if hot else 0
        targets[0, case.off + 9, 4], targets[0, case.off + 10, 4], targets[0, case.off + 11, 4] = -1, C, 1
    return {'probs': probs, 'targets': targets}


def focal_math(case, inp, wd=F64, fault=None):
    """per-element loss terms and gradient in the precision wd -> (terms [B, Al, C], grad, gradient bound)"""
    B, Al, C, off = case.B, case.Al, case.C, (0 if fault == 'offset_dropped' else case.off)
    p0 = inp['probs'].to(wd)
    cls = inp['targets'][:, off:off + Al, 4]
    alpha = torch.tensor(np.float32(case.alpha), dtype=wd)
    gamma = torch.tensor(np.float32(case.gamma), dtype=wd)
    one = torch.ones((), dtype=wd)
    lo, hi = torch.tensor(LO, dtype=wd), torch.tensor(HI, dtype=wd)
    p = torch.clamp(p0, lo, hi)
    live = ((p0 > lo) & (p0 < hi)) if fault == 'open_clamp_mask' else ((p0 >= lo) & (p0 <= hi))
    hot = (cls[:, :, None] > 0) & ((cls[:, :, None] - 1) == torch.arange(C)[None, None, :])
    counted = (cls >= 0)[:, :, None].expand(B, Al, C)
    if fault == 'ignored_counted':
        counted = torch.ones_like(counted)
    q = torch.where(hot, p, one - p)
    w = torch.where(hot, alpha, one - alpha)
    lq = torch.log(q)
    omq = one - q
    if case.gamma == 2.0:
        mod, dmod = omq * omq, -2.0 * omq
    else:
        mod = torch.pow(omq, gamma)
        dmod = torch.where(omq > 0, -gamma * torch.pow(omq, gamma - one), torch.zeros_like(omq))
    terms = torch.where(counted, -w * mod * lq, torch.zeros_like(q))
    dq = -w * (dmod * lq + mod / q)
    grad = torch.where(counted & live, torch.where(hot, dq, -dq), torch.zeros_like(q))
    amp = torch.clamp(torch.pow(omq.clamp_min(1e-300), gamma - one), min=1.0)
    bound = torch.where(counted & live, w * (gamma * amp * lq.abs() + one / q), torch.zeros_like(q))
    return terms, grad, bound


def focal_reference(case, inp, fault=None):
    terms, grad, bound = focal_math(case, inp, fault=fault)
    lost = _drop(case.total, fault).view(terms.shape)
    s = float(terms[~lost].sum())
    total = s + (0.0 if fault == 'assign_not_add' else SUM_PREFILL)
    spec = {'sum': ('bound', torch.tensor([total], dtype=F64), torch.tensor([float(focal_math(case, inp)[0].sum()) + SUM_PREFILL], dtype=F64),
                    'focal_sum')}
    if case.grad:
        spec['grad'] = ('bound', torch.where(lost, torch.full_like(grad, math.nan), grad), bound, case.gq)
    return spec


def focal_emulate(case, inp, seed=None, parts=None):
    """seed: the workgroup order of the sum (fold_partials); parts: workgroup_partials of an earlier call, to fold them again"""
    if parts is not None:
        return {'sum': torch.tensor([fold_partials(parts, SUM_PREFILL, seed)], dtype=F64)}
    terms, grad, _ = focal_math(case, inp, wd=F32)
    got = {'sum': torch.tensor([kernel_order_sum(terms.numpy().reshape(-1), SUM_PREFILL, 1, seed)], dtype=F64)}
    if case.grad:
        got['grad'] = grad.to(F64)
    return got


# ================================================================================================ smoothl1_level
SMOOTHL1_FAULTS = ('offset_dropped', 'last_block_dropped', 'remainder_dropped', 'assign_not_add')
NEUTRAL_FAULTS = ('gt_at_beta',)


@dataclass(frozen=True)
class SmoothCase:
    id: str
    B: int
    Al: int
    At: int
    off: int
    beta: float
    grad: bool = True

    @property
    def rows(self):
        return self.B * self.Al

    @property
    def dyadic(self):
        return self.beta == 0.5


def _smooth_table():
    c = []
    for i, rows in enumerate((1, 255, 257, 3001)):
        for j, beta in enumerate((0.5, 1.0 / 9.0)):
            off = (0, 77)[(i + j) % 2]
            c.append(SmoothCase(f'rows{rows}-beta{beta:.3g}-off{off}', 1, rows, rows + off + (5 if off else 0), off, beta, grad=(i + j) % 3 != 2))
    c += [SmoothCase('b3-al100-off150-beta0.5', 3, 100, 300, 150, 0.5), SmoothCase('b3-al100-off150-beta0.111', 3, 100, 300, 150, 1.0 / 9.0),
          SmoothCase('cap-beta0.5', 2, 524300, 524300, 0, 0.5), SmoothCase('cap-beta0.111', 2, 524300, 524310, 10, 1.0 / 9.0),
          SmoothCase('cap-beta0.5-nograd', 2, 524300, 524301, 1, 0.5, grad=False)]
    return tuple(c)


SMOOTH_CASES = _smooth_table()
SMOOTH_PLANTED_D = (0.5, -0.5, 0.0, 0.25)               # row 0 of the dyadic cases: |d| == beta both ways, d == 0, the quadratic branch


def smooth_inputs(case):
    """-> {'reg': [B, Al, 4], 'targets': [B, At, 5]}.  dyadic: eighths in [-1/2, 1/2], one row in 16 positive (the whole sum stays
    below 2^18, a multiple of 1/64: exact in fp32 in any order)"""
    g = _gen(case.id)
    B, Al, At = case.B, case.Al, case.At
    if case.dyadic:
        reg = _randint(g, -4, 5, (B, Al, 4)) / 8
        targets = _randint(g, -4, 5, (B, At, 5)) / 8
        cls = _randint(g, -1, 3, (B, At))
        cls = torch.where(_randint(g, 0, 16, (B, At)) == 0, _randint(g, 1, 81, (B, At)), torch.minimum(cls, torch.zeros((), dtype=F64)))
    else:
        reg = r32(torch.rand(B, Al, 4, generator=g, dtype=F64) * 0.6 - 0.3)
        targets = r32(torch.rand(B, At, 5, generator=g, dtype=F64) * 0.6 - 0.3)
        cls = _randint(g, -1, 4, (B, At))
    targets[:, :, 4] = cls
    targets[0, case.off, 4] = 2.0
    if case.dyadic:
        reg[0, 0] = targets[0, case.off, :4] + torch.tensor(SMOOTH_PLANTED_D, dtype=F64)
    if Al >= 3:
        targets[0, case.off + 1, 4], targets[0, case.off + 2, 4] = -1.0, 0.0
    return {'reg': reg, 'targets': targets}


def smooth_math(case, inp, wd=F64, fault=None):
    off = 0 if fault == 'offset_dropped' else case.off
    reg = inp['reg'].to(wd)
    t = inp['targets'][:, off:off + case.Al].to(wd)
    beta = torch.tensor(np.float32(case.beta), dtype=wd)
    pos = (t[:, :, 4] > 0)[:, :, None]
    d = reg - t[:, :, :4]
    x = d.abs()
    lin = (x > beta) if fault == 'gt_at_beta' else (x >= beta)
    terms = torch.where(lin, x - 0.5 * beta, 0.5 * x * x / beta)
    g = torch.where(lin, torch.sign(d), d / beta)
    zero = torch.zeros_like(d)
    bound = torch.where(lin, zero, (reg.abs() + t[:, :, :4].abs()) / beta)
    return torch.where(pos, terms, zero), torch.where(pos, g, zero), torch.where(pos, bound, zero)


def smooth_reference(case, inp, fault=None):
    terms, grad, bound = smooth_math(case, inp, fault=fault)
    lost = _drop(case.rows, fault).view(case.B, case.Al, 1).expand_as(terms)
    total = float(terms[~lost].sum()) + (0.0 if fault == 'assign_not_add' else SUM_PREFILL)
    ref = torch.tensor([total], dtype=F64)
    grad = torch.where(lost, torch.full_like(grad, math.nan), grad)
    if case.dyadic:
        spec = {'sum': ('equal', ref)}
        if case.grad:
            spec['grad'] = ('equal', grad)
        return spec
    spec = {'sum': ('bound', ref, torch.tensor([float(smooth_math(case, inp)[0].sum()) + SUM_PREFILL], dtype=F64), 'smoothl1_sum')}
    if case.grad:
        # the +-1 of the linear branch may become d / beta = +-(1 - O(u)) when fl(r - t) falls on the other side of beta: one unit
        spec['grad'] = ('bound', grad, torch.maximum(bound, (grad.abs() == 1).to(F64)), 'smoothl1_grad')
    return spec


def smooth_emulate(case, inp, seed=None, parts=None):
    if parts is not None:
        return {'sum': torch.tensor([fold_partials(parts, SUM_PREFILL, seed)], dtype=F64)}
    terms, grad, _ = smooth_math(case, inp, wd=F32)
    got = {'sum': torch.tensor([kernel_order_sum(terms.numpy().reshape(-1), SUM_PREFILL, 4, seed)], dtype=F64)}
    if case.grad:
        got['grad'] = grad.to(F64)
    return got


# ================================================================================================ det_best_class
BEST_FAULTS = ('last_maximum', 'offset_dropped', 'last_block_dropped', 'remainder_dropped')


@dataclass(frozen=True)
class BestCase:
    id: str
    B: int
    Al: int
    At: int
    off: int
    C: int
    ctr: bool

    @property
    def rows(self):
        return self.B * self.Al


def _best_table():
    c = []
    for i, C in enumerate((1, 2, 80, 91)):
        for j, rows in enumerate((1, 255, 256, 257)):
            c.append(BestCase(f'c{C}-rows{rows}-ctr{(i + j) % 2}', 1, rows, rows, 0, C, bool((i + j) % 2)))
    c += [BestCase('off150-c80', 3, 100, 300, 150, 80, False), BestCase('off150-c91-ctr', 3, 100, 300, 150, 91, True),
          BestCase('off7-c2-ctr', 2, 301, 400, 7, 2, True),
          BestCase('cap-c2', 2, 524300, 524300, 0, 2, False), BestCase('cap-c2-ctr-off', 2, 524300, 524303, 3, 2, True)]
    return tuple(c)


BEST_CASES = _best_table()


def best_inputs(case):
    """-> {'probs': [B, Al, C], 'ctr': [B, Al] or None}.  Every other row is quantised to 16ths: ties are common, not only planted.
    Rows 0 / 1 / 2 of image 0: two equal maxima, all values equal, the maximum at C - 1."""
    g = _gen(case.id)
    B, Al, C = case.B, case.Al, case.C
    probs = r32(torch.rand(B, Al, C, generator=g, dtype=F64))
    probs[:, ::2] = torch.floor(probs[:, ::2] * 16) / 16
    if Al >= 3:
        probs[0, 0] = 0.25
        probs[0, 0, C // 3], probs[0, 0, C - 1] = 0.875, 0.875
        probs[0, 1] = 0.375
        probs[0, 2] = r32(torch.arange(C, dtype=F64) / (2 * C))
    ctr = r32(torch.rand(B, Al, generator=g, dtype=F64)) if case.ctr else None
    return {'probs': probs, 'ctr': ctr}


def best_reference(case, inp, fault=None):
    """spec over the [B, Al] slots of this level (the launcher returns that view; the other levels' slots are guard elements)"""
    p = inp['probs']
    if fault == 'last_maximum':
        best, bc = p.flip(2).max(2)
        bc = case.C - 1 - bc
    else:
        best, bc = p.max(2)
    score = best if inp['ctr'] is None else torch.sqrt(best * inp['ctr'])
    bc = bc.to(F64)
    if fault == 'offset_dropped' and case.off:           # the level's results land in the slots of level 0: this level's stay unwritten
        score, bc = torch.full_like(score, math.nan), torch.full_like(bc, -1.0)
    lost = _drop(case.rows, fault).view(case.B, case.Al)
    score = torch.where(lost, torch.full_like(score, math.nan), score)
    bc = torch.where(lost, torch.full_like(bc, -1.0), bc)
    return {'classes': ('equal', bc), 'scores': ('equal', score) if inp['ctr'] is None else ('fixed', score, score, 'chain4')}


# ================================================================================================ detr_box_loss
DETR_FAULTS = ('tie_all_to_first', 'clamp_mask_open', 'touching_blocks_gradient')


@dataclass(frozen=True)
class DetrCase:
    id: str
    L: int
    B: int
    T: int
    lo: float
    hi: float
    d_l1: bool = True
    d_iou: bool = True

    @property
    def Q(self):
        return self.T + 2


def _detr_table():
    c = []
    for i, (B, T) in enumerate(((1, 1), (3, 85), (2, 128), (1, 257), (3, 171))):
        for L in (1, 6):
            lo, hi = ((1 / 64, 63 / 64), (0.0, 1.0))[(i + L) % 2]
            c.append(DetrCase(f'l{L}-b{B}-t{T}-lo{lo:g}', L, B, T, lo, hi, d_l1=not (i == 1 and L == 6), d_iou=not (i == 2 and L == 1)))
    return tuple(c)


DETR_CASES = _detr_table()
DETR_PLANTED = ('equal', 'disjoint', 'touching', 'at_lo', 'at_hi', 'below_lo', 'above_hi', 'zero_size')


def detr_inputs(case):
    """-> reg [L, B, Q, 4], gt [B, T, 5] (cx cy w h class, -1 rows padding), src / tgt int64 [B, T], w [B, T], d_l1 / d_iou [L]: every
    box component a multiple of 1/64.  Image 1 (when there is one) has no boxes.  The first 8 pairs of image 0 (T >= 8), layer 0,
    are DETR_PLANTED; with T == 1 the only pair is 'equal'."""
    g = _gen(case.id)
    L, B, T, Q, lo, hi = case.L, case.B, case.T, case.Q, case.lo, case.hi
    reg = _randint(g, 2, 63, (L, B, Q, 4)) / 64
    reg[:, :, 5::7, 2] = 1.25                            # outside the clamp range
    reg[:, :, 3::9, 1] = -0.25
    gt = torch.full((B, T, 5), -1.0, dtype=F64)
    src = torch.zeros(B, T, dtype=torch.int64)
    tgt = torch.zeros(B, T, dtype=torch.int64)
    w = torch.zeros(B, T, dtype=F64)
    for b in range(B):
        n = 0 if b == 1 else (T if b == 0 else max(1, T // 2))
        gt[b, :n, 0:2] = _randint(g, 16, 49, (n, 2)) / 64
        gt[b, :n, 2:4] = _randint(g, 2, 21, (n, 2)) / 64
        gt[b, :n, 4] = _randint(g, 0, 80, (n,))
        src[b, :n] = torch.randperm(Q, generator=g)[:n]
        tgt[b, :n] = torch.randperm(n, generator=g) if b else torch.arange(n)
        w[b, :n] = torch.where(torch.arange(n) % 5 == 4, 0.5, 1.0).to(F64)
    t0 = torch.tensor([24, 32, 8, 12], dtype=F64) / 64
    below, above = float(np.nextafter(np.float32(lo), np.float32(-1))), float(np.nextafter(np.float32(hi), np.float32(2)))
    if lo == 0.0:
        below = -1 / 64
    if T >= 8:
        gt[0, :8, :4] = t0
        rows = {'equal': t0, 'disjoint': [50 / 64, 50 / 64, 6 / 64, 6 / 64], 'touching': [(24 + 4 + 3) / 64, 32 / 64, 6 / 64, 12 / 64],
                'at_lo': [24 / 64, 32 / 64, lo, 12 / 64], 'at_hi': [hi, 32 / 64, 8 / 64, 12 / 64],
                'below_lo': [24 / 64, 32 / 64, below, 12 / 64], 'above_hi': [above, 32 / 64, 8 / 64, 12 / 64],
                'zero_size': [24 / 64, 32 / 64, 0.0, 0.0]}
        for k, name in enumerate(DETR_PLANTED):
            reg[0, 0, src[0, k]] = torch.as_tensor(rows[name], dtype=F64)
    else:
        gt[0, 0, :4] = t0
        reg[0, 0, src[0, 0]] = t0
    d_l1 = r32(torch.randn(L, generator=g, dtype=F64)) if case.d_l1 else None
    d_iou = r32(torch.randn(L, generator=g, dtype=F64)) if case.d_iou else None
    return {'reg': r32(reg), 'gt': gt, 'src': src, 'tgt': tgt, 'w': w, 'd_l1': d_l1, 'd_iou': d_iou}


def giou_tape(p, t, wd=F64):
    """giou_fwd of csrc/detloss.hip on [..., 4] cx cy w h boxes -> dict of its intermediates"""
    p, t = p.to(wd), t.to(wd)
    z = torch.zeros((), dtype=wd)
    e = torch.tensor(LO, dtype=wd)
    g = {'x1': p[..., 0] - 0.5 * p[..., 2], 'y1': p[..., 1] - 0.5 * p[..., 3], 'x2': p[..., 0] + 0.5 * p[..., 2], 'y2': p[..., 1] + 0.5 * p[..., 3],
         'tx1': t[..., 0] - 0.5 * t[..., 2], 'ty1': t[..., 1] - 0.5 * t[..., 3], 'tx2': t[..., 0] + 0.5 * t[..., 2], 'ty2': t[..., 1] + 0.5 * t[..., 3]}
    g['a10'] = (g['x2'] - g['x1']) * (g['y2'] - g['y1'])
    a1 = torch.maximum(g['a10'], z)
    a2 = torch.maximum((g['tx2'] - g['tx1']) * (g['ty2'] - g['ty1']), z)
    g['iw'] = torch.minimum(g['x2'], g['tx2']) - torch.maximum(g['x1'], g['tx1'])
    g['ih'] = torch.minimum(g['y2'], g['ty2']) - torch.maximum(g['y1'], g['ty1'])
    g['cw'], g['ch'] = torch.maximum(g['iw'], z), torch.maximum(g['ih'], z)
    g['i0'] = g['cw'] * g['ch']
    g['inter'] = torch.maximum(g['i0'], z)
    g['u0'] = a1 + a2 - g['inter']
    g['uni'] = torch.maximum(g['u0'], e)
    g['ew0'] = torch.maximum(g['x2'], g['tx2']) - torch.minimum(g['x1'], g['tx1'])
    g['eh0'] = torch.maximum(g['y2'], g['ty2']) - torch.minimum(g['y1'], g['ty1'])
    g['ew'], g['eh'] = torch.maximum(g['ew0'], z), torch.maximum(g['eh0'], z)
    g['e0'] = g['ew'] * g['eh']
    g['enc'] = torch.maximum(g['e0'], e)
    g['iou'], g['pen'] = g['inter'] / g['uni'], (g['enc'] - g['uni']) / g['enc']
    g['giou'] = g['iou'] - g['pen']
    return g


def giou_backward(g, mag=False, fault=None):
    """giou_bwd of csrc/detloss.hip on a tape -> d giou / d (cx, cy, w, h) [..., 4]; mag: every product by magnitude, every sum a sum of
    magnitudes (the bound of the gradient)."""
    s = 1.0 if mag else -1.0
    ab = torch.abs if mag else (lambda v: v)
    zero = torch.zeros_like(g['uni'])
    e = LO
    d_inter = 1.0 / g['uni']
    d_uni = s * g['inter'] / (g['uni'] * g['uni']) + 1.0 / g['enc']
    d_enc = s / g['enc'] + ab(g['enc'] - g['uni']) / (g['enc'] * g['enc'])
    d_u0 = torch.where(g['u0'] >= e, d_uni, zero)
    d_a1 = d_u0
    d_inter = d_inter + s * d_u0
    d_i0 = torch.where(g['i0'] >= 0, d_inter, zero)
    pass_iw = (g['iw'] > 0) if fault == 'touching_blocks_gradient' else (g['iw'] >= 0)
    d_iw = torch.where(pass_iw, d_i0 * g['ch'], zero)
    d_ih = torch.where(g['ih'] >= 0, d_i0 * g['cw'], zero)
    d_e0 = torch.where(g['e0'] >= e, d_enc, zero)
    d_ew0 = torch.where(g['ew0'] >= 0, d_e0 * g['eh'], zero)
    d_eh0 = torch.where(g['eh0'] >= 0, d_e0 * g['ew'], zero)
    d_a10 = torch.where(g['a10'] >= 0, d_a1, zero)
    half = 1.0 if fault == 'tie_all_to_first' else 0.5

    def sel_min(a, b):
        return torch.where(a < b, 1.0, torch.where(a == b, half, 0.0)).to(a.dtype)

    def sel_max(a, b):
        return torch.where(a > b, 1.0, torch.where(a == b, half, 0.0)).to(a.dtype)
    hgt, wid = ab(g['y2'] - g['y1']), ab(g['x2'] - g['x1'])
    dx2 = d_iw * sel_min(g['x2'], g['tx2']) + d_ew0 * sel_max(g['x2'], g['tx2']) + d_a10 * hgt
    dx1 = s * d_iw * sel_max(g['x1'], g['tx1']) + s * d_ew0 * sel_min(g['x1'], g['tx1']) + s * d_a10 * hgt
    dy2 = d_ih * sel_min(g['y2'], g['ty2']) + d_eh0 * sel_max(g['y2'], g['ty2']) + d_a10 * wid
    dy1 = s * d_ih * sel_max(g['y1'], g['ty1']) + s * d_eh0 * sel_min(g['y1'], g['ty1']) + s * d_a10 * wid
    return torch.stack([dx1 + dx2, dy1 + dy2, 0.5 * (dx2 + s * dx1), 0.5 * (dy2 + s * dy1)], -1)


def detr_math(case, inp, wd=F64, fault=None, bounds=False):
    """the kernels' arithmetic in the precision wd -> {'l1' [L], 'iou' [L], 'n' [1], 'dreg' [L, B, Q, 4]} (and the bounds)"""
    L, B, T, Q = case.L, case.B, case.T, case.Q
    lo, hi = torch.tensor(np.float32(case.lo), dtype=wd), torch.tensor(np.float32(case.hi), dtype=wd)
    raw = inp['reg'].to(wd)
    gt, w = inp['gt'].to(wd), inp['w'].to(wd)
    bidx = torch.arange(B)[:, None].expand(B, T)
    on = w > 0
    pr = raw[:, bidx, inp['src']]                        # [L, B, T, 4]
    p = torch.clamp(pr, lo, hi)
    t = gt[bidx, inp['tgt'], 0:4][None].expand(L, B, T, 4)
    n = (gt[:, :, 4] >= 0).sum().to(wd)
    tape = giou_tape(p, t, wd)
    wl = torch.where(on, w, torch.zeros_like(w))[None]
    l1 = ((p - t).abs().sum(-1) * wl).sum((1, 2)) / n
    iou = ((1.0 - tape['giou']) * wl).sum((1, 2)) / n
    res = {'l1': l1, 'iou': iou, 'n': n.reshape(1)}
    g_l1 = (inp['d_l1'].to(wd) if inp['d_l1'] is not None else torch.zeros(L, dtype=wd)) / n
    g_iou = (inp['d_iou'].to(wd) if inp['d_iou'] is not None else torch.zeros(L, dtype=wd)) / n
    live = ((pr > lo) & (pr < hi)) if fault == 'clamp_mask_open' else ((pr >= lo) & (pr <= hi))
    dg = giou_backward(tape, fault=fault)
    dp = wl[..., None] * (g_l1[:, None, None, None] * torch.sign(p - t) - g_iou[:, None, None, None] * dg)
    dp = torch.where(live & on[None, :, :, None], dp, torch.zeros_like(dp))
    dreg = torch.zeros(L, B, Q, 4, dtype=wd)
    sidx = torch.where(on, inp['src'], torch.full_like(inp['src'], Q))          # pairs that are off scatter into a spare row
    dreg = torch.cat([dreg, torch.zeros(L, B, 1, 4, dtype=wd)], 2)
    dreg[:, bidx, sidx] = dp
    res['dreg'] = dreg[:, :, :Q]
    if not bounds:
        return res
    bnd = {'l1': l1, 'iou': ((1.0 + tape['iou'].abs() + tape['pen'].abs()) * wl).sum((1, 2)) / n}
    mg = giou_backward(tape, mag=True)
    bp = wl[..., None] * (g_l1.abs()[:, None, None, None] * torch.sign(p - t).abs() + g_iou.abs()[:, None, None, None] * mg)
    bp = torch.where(live & on[None, :, :, None], bp, torch.zeros_like(bp))
    bd = torch.zeros(L, B, Q + 1, 4, dtype=wd)
    bd[:, bidx, sidx] = bp
    bnd['dreg'] = bd[:, :, :Q]
    return res, bnd


def detr_autograd(case, inp):
    """float64 torch autograd over losses._giou: the reference of the values and of the gradient"""
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.detection import losses as LS
    L, B, T = case.L, case.B, case.T
    r = inp['reg'].clone().requires_grad_(True)
    p = torch.clamp(r, min=float(np.float32(case.lo)), max=float(np.float32(case.hi)))
    bidx = torch.arange(B)[:, None].expand(B, T)
    on = inp['w'] > 0
    dummy = torch.tensor([0.5, 0.5, 0.25, 0.25], dtype=F64)
    pm = torch.where(on[None, :, :, None], p[:, bidx, inp['src']], dummy)
    tb = torch.where(on[:, :, None], inp['gt'][bidx, inp['tgt'], 0:4], dummy)
    n = (inp['gt'][:, :, 4] >= 0).sum().to(F64)
    l1 = ((pm - tb).abs().sum(-1) * inp['w']).sum((1, 2)) / n
    iou = ((1 - LS._giou(LS._cxcywh_to_xyxy(pm), LS._cxcywh_to_xyxy(tb))) * inp['w']).sum((1, 2)) / n
    seed = torch.zeros((), dtype=F64)
    if inp['d_l1'] is not None:
        seed = seed + (l1 * inp['d_l1']).sum()
    if inp['d_iou'] is not None:
        seed = seed + (iou * inp['d_iou']).sum()
    grad = torch.autograd.grad(seed, r)[0] if seed.requires_grad else torch.zeros_like(r)
    return {'l1': l1.detach(), 'iou': iou.detach(), 'n': n.reshape(1), 'dreg': grad}


def detr_reference(case, inp, fault=None):
    ref = detr_autograd(case, inp) if fault is None else detr_math(case, inp, fault=fault)
    _, bnd = detr_math(case, inp, bounds=True)
    return {'l1': ('bound', ref['l1'], bnd['l1'], 'detr_l1'), 'iou': ('bound', ref['iou'], bnd['iou'], 'detr_iou'),
            'n': ('equal', ref['n']), 'dreg': ('bound', ref['dreg'], bnd['dreg'], 'detr_grad')}


def detr_emulate(case, inp):
    return {k: v.to(F64) for k, v in detr_math(case, inp, wd=F32).items()}


# ================================================================================================ the forms the tables reach
def looped_items():
    """{kernel: [items of every case]} of the kernels that loop beyond dl_grid()'s cap"""
    return {'focal_level_kernel': [c.total for c in FOCAL_CASES], 'smoothl1_level_kernel': [c.rows for c in SMOOTH_CASES],
            'best_class_kernel': [c.rows for c in BEST_CASES]}


# ================================================================================================ device side (needs a GPU)
class GuardedInt:
    """Guarded for an int32 output: the view pre-filled with -1 (never a class), SENTINEL around and between its rows"""

    def __init__(self, shape, strides, device):
        span = 1 + sum((n - 1) * s for n, s in zip(shape, strides))
        self.flat = torch.full((2 * GUARD + span,), int(SENTINEL), dtype=torch.int32, device=device)
        self.view = self.flat.as_strided(tuple(shape), tuple(strides), GUARD)
        self.view.fill_(-1)
        self.inside = self.flat == -1

    def check(self, name):
        bad = []
        if bool((self.flat[self.inside] == -1).any()):
            bad.append(f'{name}: {int((self.flat[self.inside] == -1).sum())} elements were never written')
        outside = self.flat[~self.inside]
        if not bool((outside == int(SENTINEL)).all()):
            bad.append(f'{name}: {int((outside != int(SENTINEL)).sum())} sentinel elements outside the view were overwritten')
        return bad


def _dev(t, device, dtype=F32):
    return None if t is None else t.to(dtype).contiguous().to(device)


def _L():
    from simpleaicv_pytorch_training_examples_amd import _lib
    return _lib, _lib.lib()


def _scalar(device, value):
    g = Guarded((1,), (1,), F32, device)
    g.view.fill_(value)
    return g


def _complaints(guards):
    return [m for name, g in guards for m in g.check(name)]


def run_retina_assign(case, inp, device='cuda'):
    """-> (got for judge(), complaints of the guards)"""
    _lib, L = _L()
    an, ann = _dev(inp['anchors'], device), _dev(inp['annots'], device)
    g_t = Guarded((case.B, case.A, 5), (case.A * 5, 5, 1), F32, device)
    g_p = _scalar(device, POS_PREFILL)
    _lib.check(L.saicv_retina_assign(_lib.ptr(an), _lib.ptr(ann), _lib.ptr(g_t.view), _lib.ptr(g_p.view), case.B, case.A, case.G,
                                     case.smoothl1, _lib.stream()), 'retina_assign')
    torch.cuda.synchronize()
    return retina_split(g_t.view, g_p.view, case), _complaints([('targets', g_t), ('pos_count', g_p)])


def run_fcos_assign(case, inp, device='cuda'):
    _lib, L = _L()
    pts, ann = _dev(inp['points'], device), _dev(inp['annots'], device)
    g_t = Guarded((case.B, case.P, 5), (case.P * 5, 5, 1), F32, device)
    g_c = Guarded((case.B, case.P), (case.P, 1), F32, device)
    g_p = _scalar(device, POS_PREFILL)
    _lib.check(L.saicv_fcos_assign(_lib.ptr(pts), _lib.ptr(ann), _lib.ptr(g_t.view), _lib.ptr(g_c.view), _lib.ptr(g_p.view), case.B, case.P,
                                   case.G, FCOS_RADIUS, case.center_sample, _lib.stream()), 'fcos_assign')
    torch.cuda.synchronize()
    return fcos_split(g_t.view, g_c.view, g_p.view), _complaints([('targets', g_t), ('centerness', g_c), ('pos_count', g_p)])


def run_focal(case, inp, device='cuda'):
    _lib, L = _L()
    probs, targets = _dev(inp['probs'], device), _dev(inp['targets'], device)
    g_s = _scalar(device, SUM_PREFILL)
    guards = [('loss_sum', g_s)]
    g_d = None
    if case.grad:
        g_d = Guarded((case.B, case.Al, case.C), (case.Al * case.C, case.C, 1), F32, device)
        guards.append(('dprobs', g_d))
    _lib.check(L.saicv_focal_loss_level(_lib.ptr(probs), _lib.ptr(targets), _lib.ptr(g_d.view) if g_d else None, _lib.ptr(g_s.view), case.B,
                                        case.Al, case.At, case.off, case.C, float(case.alpha), float(case.gamma), _lib.stream()), 'focal_loss_level')
    torch.cuda.synchronize()
    got = {'sum': g_s.view.to(F64).cpu()}
    if g_d:
        got['grad'] = g_d.view.to(F64).cpu()
    return got, _complaints(guards)


def run_smoothl1(case, inp, device='cuda'):
    _lib, L = _L()
    reg, targets = _dev(inp['reg'], device), _dev(inp['targets'], device)
    g_s = _scalar(device, SUM_PREFILL)
    guards = [('loss_sum', g_s)]
    g_d = None
    if case.grad:
        g_d = Guarded((case.B, case.Al, 4), (case.Al * 4, 4, 1), F32, device)      # GUARD * 4 bytes in front: still 16-byte aligned
        guards.append(('dreg', g_d))
    _lib.check(L.saicv_smoothl1_level(_lib.ptr(reg), _lib.ptr(targets), _lib.ptr(g_d.view) if g_d else None, _lib.ptr(g_s.view), case.B,
                                      case.Al, case.At, case.off, float(case.beta), _lib.stream()), 'smoothl1_level')
    torch.cuda.synchronize()
    got = {'sum': g_s.view.to(F64).cpu()}
    if g_d:
        got['grad'] = g_d.view.to(F64).cpu()
    return got, _complaints(guards)


def run_best_class(case, inp, device='cuda'):
    """scores / classes are [B, At] buffers of which this level owns [off, off + Al) of every image: the guarded view is exactly those
    slots, every other level's slots are sentinel elements, and the kernel gets the address of slot [0, 0] of the whole buffer"""
    _lib, L = _L()
    assert case.off <= GUARD
    probs, ctr = _dev(inp['probs'], device), _dev(inp['ctr'], device)
    g_s = Guarded((case.B, case.Al), (case.At, 1), F32, device)
    g_c = GuardedInt((case.B, case.Al), (case.At, 1), device)
    _lib.check(L.saicv_det_best_class(_lib.ptr(probs), _lib.ptr(ctr), _lib.ptr(g_s.view) - 4 * case.off, _lib.ptr(g_c.view) - 4 * case.off,
                                      case.B, case.Al, case.At, case.off, case.C, _lib.stream()), 'det_best_class')
    torch.cuda.synchronize()
    return {'scores': g_s.view.to(F64).cpu(), 'classes': g_c.view.to(F64).cpu()}, _complaints([('scores', g_s), ('classes', g_c)])


def run_detr(case, inp, device='cuda'):
    _lib, L = _L()
    reg, gt, w = _dev(inp['reg'], device), _dev(inp['gt'], device), _dev(inp['w'], device)
    src, tgt = inp['src'].to(device), inp['tgt'].to(device)
    d_l1, d_iou = _dev(inp['d_l1'], device), _dev(inp['d_iou'], device)
    Lr, B, Q, T = case.L, case.B, case.Q, case.T
    g_o = Guarded((2 * Lr + 1,), (1,), F32, device)
    g_d = Guarded((Lr, B, Q, 4), (B * Q * 4, Q * 4, 4, 1), F32, device)
    _lib.check(L.saicv_detr_box_loss_fwd(_lib.ptr(reg), _lib.ptr(gt), _lib.ptr(src), _lib.ptr(tgt), _lib.ptr(w), Lr, B, Q, T, float(case.lo),
                                         float(case.hi), _lib.ptr(g_o.view), _lib.stream()), 'detr_box_loss_fwd')
    _lib.check(L.saicv_detr_box_loss_bwd(_lib.ptr(reg), _lib.ptr(gt), _lib.ptr(src), _lib.ptr(tgt), _lib.ptr(w), _lib.ptr(d_l1), _lib.ptr(d_iou),
                                         _lib.ptr(g_o.view), Lr, B, Q, T, float(case.lo), float(case.hi), _lib.ptr(g_d.view), _lib.stream()),
               'detr_box_loss_bwd')
    torch.cuda.synchronize()
    out = g_o.view.to(F64).cpu()
    return {'l1': out[:Lr], 'iou': out[Lr:2 * Lr], 'n': out[2 * Lr:], 'dreg': g_d.view.to(F64).cpu()}, _complaints([('out', g_o), ('dreg', g_d)])


# ================================================================================================ the edge fixture
EDGE_CLASSES, EDGE_BETA = 80, 1.0 / 9.0


def _pick(table, **kw):
    return next(c for c in table if all(getattr(c, k) == v for k, v in kw.items()))


def edge_cases():
    """the exact-regime cases oracle/make_golden_detloss_edges.py runs the reference project's own code on (tests/golden/detloss_edges.pt)"""
    return {'retina': (_pick(RETINA_CASES, A=257, G=37, smoothl1=0), _pick(RETINA_CASES, A=257, G=37, smoothl1=1),
                       _pick(RETINA_CASES, A=256, G=1024, smoothl1=0)),
            'fcos': (_pick(FCOS_CASES, P=257, G=37, center_sample=0, ranges='default'), _pick(FCOS_CASES, P=257, G=37, center_sample=1, ranges='default'),
                     _pick(FCOS_CASES, P=257, G=37, center_sample=0, ranges='second'), _pick(FCOS_CASES, P=256, G=1024, center_sample=1)),
            'best': (_pick(BEST_CASES, C=80, Al=257), _pick(BEST_CASES, C=2, Al=255), _pick(BEST_CASES, C=91, Al=256))}


def edge_heads(case_id, B, N):
    """head outputs for the loss scalars of the edge fixture: probabilities [B, N, 80] (with the planted clamp edges) and box offsets"""
    probs = focal_inputs(FocalCase('edge-' + case_id, B, N, N, 0, EDGE_CLASSES, 2.0))['probs']
    reg = smooth_inputs(SmoothCase('edge-' + case_id, B, N, N, 0, EDGE_BETA))['reg']
    return probs, reg


def edge_focal_scalar(case_id, cls):
    """float64 focal loss / positives (0 without positives) of edge_heads() against class targets [B, N] -> (value, bound)"""
    B, N = cls.shape
    fc = FocalCase('edge-' + case_id, B, N, N, 0, EDGE_CLASSES, 2.0)
    targets = torch.zeros(B, N, 5, dtype=F64)
    targets[:, :, 4] = cls
    terms = focal_math(fc, {'probs': edge_heads(case_id, B, N)[0], 'targets': targets})[0]
    pos = float((cls > 0).sum())
    return (float(terms.sum()) / pos if pos else 0.0), (float(terms.sum()) / max(pos, 1.0))


def edge_smooth_scalar(case_id, cls, box):
    B, N = cls.shape
    sc = SmoothCase('edge-' + case_id, B, N, N, 0, EDGE_BETA)
    targets = torch.cat([box, cls[:, :, None]], 2)
    terms = smooth_math(sc, {'reg': edge_heads(case_id, B, N)[1], 'targets': targets})[0]
    pos = float((cls > 0).sum())
    return (float(terms.sum()) / pos if pos else 0.0), (float(terms.sum()) / max(pos, 1.0))
