"""What tests/test_sam_judge_host.py (no GPU) and tests/test_gpu_sam_kernels.py (MI355X) share: the case tables of SAM's own kernels
(csrc/sam.hip, csrc/samtail.hip, csrc/maskloss.hip), their input builders, float64 references with hand-written gradients, the
working-precision emulations that set the constants, the restated relpos dispatch, and the launchers that call the C-ABI with outputs
inside sentinel guards.

Two kinds of check.

Structure, bit for bit: operands that every precision holds exactly ({-1, 0, 1}, small integers, multiples of 1/8), so that the
result must equal the float64 computation in every bit -- a lost tile, a skewed index, a transposed fragment or a missing accumulate
cannot hide inside a tolerance.  exact_limits() states, and the tests assert in float64 first, that every intermediate is an integer
(or a dyadic number) the working precision holds.

Accuracy, element by element: random inputs rounded to the working dtype, the float64 reference over the values the device holds,
and an element passes when |got - ref| <= MARGIN * c * u * bound (attn_common's judge): u = 2^-24 (fp32) or 2^-9 (bf16), bound the
magnitude sum of the element's own expression in float64, c the worst ratio over the whole case table of a CPU emulation in the working
precision (CONSTANTS, measured and held by test_sam_judge_host.py).  Where bound is 0 the result must be 0.  Nothing is sampled.

    relpos       rel_h[b n, q, kh] = <q[b, q, n, :], Th[qh - kh + Sh - 1]>    bound sum_c |q_c| |T_c|          (rel_w alike)
                 dq = dq0 + sum_kh g_h Th[..] + sum_kw g_w Tw[..]             bound |dq0| + sum |g| |T|
                 dtab_h[j] = dtab0[j] + sum over qh - kh + Sh - 1 = j of g_h q  bound |dtab0| + sum |g| |q|     (dtab_w alike)
    hyper        out = hyper x^T, dx = dout^T hyper, dhyper = dout x            bounds: the same products of magnitudes
    mask loss    the four real sums (focal, p t, p, t): every term is >= 0, so the bound is the sum itself; these are fp32 results of
                 fp32 arithmetic in either dtype and are judged with u = 2^-24 in both.
                 gradient g = c0 dfocal + (c1 t + c2) p (1 - p), bound |c0| af (gamma bce + 1) + |c1| t + |c2|: the magnitude with
                 every factor that lies in [0, 1] replaced by 1.  `1 - p` in fp32 carries an ABSOLUTE error of u, so a confident
                 pixel's gradient (orders of magnitude below the bound) is judged absolutely, not relative to itself.  In bf16 the
                 stored gradient is that fp32 value rounded once: the fp32 allowance plus half a bf16 unit in the last place of the
                 reference value (between 2^-9 and 2^-8 of it -- a flat 2^-9 is below the rounding itself for most values, which
                 test_sam_judge_host.py shows on the float64 reference rounded once).
    _up4 route   x = U low (U: the x4 half-pixel bilinear operator as two dense float64 matrices), then the loss; the gradient is
                 U^T g and its bound U^T bound (U >= 0).

The emulations round where the kernels round: tables rounded to bf16 in the bf16 forward; tables and d_rel rounded to bf16 in the
MFMA backward forms (64 x 64, and Sh, Sw <= 16); one bf16 rounding of every stored bf16 output, `prior dq + increment` included.  Two
long fp32 sums are emulated in the kernels' own partition: the relpos table gradients as one fp32 partial per (batch entry, query row)
workgroup added in workgroup order (what the deterministic fold does), and dhyper as one partial per 256 pixels.  The mask-loss sums are
NOT: their emulation is torch's flat fp32 `sum` over the plane (on the up4 route after F.interpolate), not one partial per 8192- /
16384-element slab or per (column block, low-resolution row).
"""
import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from attn_common import DT_NAME, GUARD, MARGIN, SENTINEL, U, Guarded  # noqa: F401  (re-exported to the two test files)

D = 64                              # head dim of the relpos kernels (RP_D)
ALPHA = 0.25
F32, BF16 = torch.float32, torch.bfloat16

RELPOS_Q = ('rel_h', 'rel_w', 'dq', 'dtab_h', 'dtab_w')
HYPER_Q = ('hp_out', 'hp_dx', 'hp_dhyper')
SUMS = ('focal', 'inter', 'psum', 'tsum')
MASK_Q = tuple('ml_' + s for s in SUMS) + ('ml_grad',)
UP4_Q = tuple('up_' + s for s in SUMS) + ('up_grad',)
QUANTITIES = RELPOS_Q + HYPER_Q + MASK_Q + UP4_Q
FP32_UNIT = set(MASK_Q + UP4_Q)     # fp32 results of fp32 arithmetic in either dtype (the bf16 gradients: plus one bf16 rounding)

# Worst ratio of the emulations to the float64 reference over every case of the tables, in units of u * bound.
# Measured by tests/test_sam_judge_host.py::test_constants_table_is_what_the_emulations_measure (CPU, one thread), which fails if a row
# drifts by more than a quarter; the judge allows MARGIN times these.
CONSTANTS = {
    F32: {'rel_h': 5.84, 'rel_w': 6.08, 'dq': 5.93, 'dtab_h': 3.17, 'dtab_w': 1.70, 'hp_out': 3.86, 'hp_dx': 3.43, 'hp_dhyper': 2.81,
          'ml_focal': 3.07, 'ml_inter': 2.43, 'ml_psum': 2.72, 'ml_tsum': 0.0, 'ml_grad': 1.30,
          'up_focal': 3.58, 'up_inter': 6.16, 'up_psum': 2.63, 'up_tsum': 0.0, 'up_grad': 1.62},
    # (hp_dhyper: fp32 sums of products that are exact in fp32, measured in the bf16 unit.  No gradient rows: the bf16 gradient is held to
    # the fp32 allowance plus its one rounding -- constant() -- and its emulation, measured the same way, sits at 0.727 / 0.148 of the unit)
    BF16: {'rel_h': 0.853, 'rel_w': 0.822, 'dq': 2.82, 'dtab_h': 1.09, 'dtab_w': 0.917, 'hp_out': 1.51, 'hp_dx': 1.99, 'hp_dhyper': 5.14e-05,
           'ml_focal': 4.16, 'ml_inter': 2.41, 'ml_psum': 2.75, 'ml_tsum': 0.0,
           'up_focal': 3.45, 'up_inter': 2.46, 'up_psum': 2.75, 'up_tsum': 0.0},
}
CONSTANTS_MEASURED_WITH = 'torch 2.10.0+rocm7.0, 2026-10-18'


def unit(quantity, dtype):
    return U[F32] if quantity in FP32_UNIT else U[dtype]


def constant(quantity, dtype):
    """the bf16 gradients take the fp32 row: their allowance is the fp32 one plus the rounding of the store"""
    return CONSTANTS[F32 if quantity.endswith('_grad') else dtype][quantity]


def _seed(text):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(text)) % (2 ** 31)


def _bf16(x):
    return x.to(BF16).to(x.dtype)


def half_ulp_bf16(x):
    """half a unit in the last place of bf16 at |x| (float64 in, float64 out): 2^(floor(log2 |x|) - 8), the subnormal spacing below 2^-126"""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -140))          # |x| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(x), (e - 1).clamp_min(-126) - 8)


# ================================================================================================ relpos
RP_GRIDS = ((1, 1), (1, 16), (16, 1), (3, 7), (7, 16), (14, 14), (16, 16), (16, 17), (17, 16), (17, 17), (20, 37), (32, 32), (33, 31),
            (5, 64), (64, 5), (63, 64), (64, 63), (64, 64), (65, 64), (100, 24), (128, 64), (128, 1))


@dataclass(frozen=True)
class RelPos:
    Sh: int
    Sw: int
    heads: int = 3
    B: int = 2
    contiguous: bool = False        # q as a contiguous [B, N, C] instead of the strided slice of a packed [B, N, 3C]

    @property
    def id(self):
        return f'{self.Sh}x{self.Sw}-h{self.heads}-b{self.B}' + ('-contig' if self.contiguous else '')

    @property
    def N(self):
        return self.Sh * self.Sw

    @property
    def C(self):
        return self.heads * D


def _relpos_cases():
    c = [RelPos(sh, sw) for sh, sw in RP_GRIDS]
    # 5 heads: 70 items at Sw = 14 (a full 64-item tile of the FMA table kernel, then a partial one), 160 at 32, 320 at 64 (a second
    # pass of the 256-thread item loop); 12 heads x 64: SAM-B's 768 items
    c += [RelPos(s, s, heads=5) for s in (14, 32, 64)]
    c += [RelPos(64, 64, heads=12, B=1)]
    c += [RelPos(14, 14, contiguous=True), RelPos(64, 64, contiguous=True)]
    return tuple(c)


RELPOS_CASES = _relpos_cases()
RELPOS_ACCURACY_CASES = tuple(c for c in RELPOS_CASES if not c.contiguous)


def relpos_forms(dt, Sh, Sw):
    """The kernels relpos_fwd / relpos_bwd launch for (dtype, Sh, Sw), restated from csrc/sam.hip (namespace saicv: relpos_fwd picks on
    the dtype alone; relpos_bwd on the dtype, on (Sh, Sw) == (64, 64) and on Sh, Sw <= 16; the RP_TAB macro on NHc / NWc).
    -> (forward, dq, table gradient)"""
    nh, nw = (Sh + 15) // 16, (2 * Sw - 1 + 15) // 16
    NH, NW = (1 if nh <= 1 else 4 if nh <= 4 else 8), (2 if nw <= 2 else 8)
    tile = (NH, NW) if (NH, NW) in ((1, 2), (4, 8)) else (8, 8)
    if dt == 'bf16':
        if (Sh, Sw) == (64, 64):
            return 'relpos_fwd_mfma_kernel', 'relpos_bwd_dq_mfma_kernel<2,4>', 'relpos_bwd_tab_mfma_kernel<2,4,8>'
        if Sh <= 16 and Sw <= 16:
            return 'relpos_fwd_mfma_kernel', 'relpos_bwd_dq_mfma_kernel<1,1>', 'relpos_bwd_tab_mfma_kernel<1,1,2>'
        return 'relpos_fwd_mfma_kernel', 'relpos_bwd_dq_kernel<bf16>', f'relpos_bwd_tab_kernel<bf16,{tile[0]},{tile[1]}>'
    return 'relpos_fwd_kernel<f32>', 'relpos_bwd_dq_kernel<f32>', f'relpos_bwd_tab_kernel<f32,{tile[0]},{tile[1]}>'


RELPOS_MAX_SH, RELPOS_MAX_SW = 128, 64          # what relpos_fill admits
# every instantiation in csrc/sam.hip
RELPOS_INSTANTIATED = {'relpos_fwd_mfma_kernel', 'relpos_fwd_kernel<f32>', 'relpos_bwd_dq_mfma_kernel<2,4>', 'relpos_bwd_dq_mfma_kernel<1,1>',
                       'relpos_bwd_dq_kernel<bf16>', 'relpos_bwd_dq_kernel<f32>', 'relpos_bwd_tab_mfma_kernel<2,4,8>',
                       'relpos_bwd_tab_mfma_kernel<1,1,2>'} | {f'relpos_bwd_tab_kernel<{t},{a},{b}>' for t in ('f32', 'bf16')
                                                                for a, b in ((1, 2), (4, 8), (8, 8))}
# instantiated by the RP_TAB macro, never launched: NHc == 1 and NWc == 2 means Sh, Sw <= 16, which in bf16 takes the MFMA form
RELPOS_UNREACHABLE = {'relpos_bwd_tab_kernel<bf16,1,2>'}


def relpos_mfma_backward(dtype, Sh, Sw):
    return dtype == BF16 and ((Sh, Sw) == (64, 64) or (Sh <= 16 and Sw <= 16))


def relpos_inputs(case, dtype, exact):
    """-> float64 CPU tensors holding the values the device will hold: q / dq0 [B, N, C] (the prior dq the kernel adds to), tab_h
    [2 Sh - 1, 64], tab_w [2 Sw - 1, 64], g_h [B heads, N, Sh], g_w [B heads, N, Sw] (the gradients of the logits), dtab_h0 / dtab_w0
    (the prior table gradients).  exact: entries in {-1, 0, 1}, prior table gradients integers in [-3, 3]."""
    g = torch.Generator().manual_seed(_seed(case.id + ('x' if exact else DT_NAME[dtype])))
    B, H, Sh, Sw, N, C = case.B, case.heads, case.Sh, case.Sw, case.N, case.C
    shapes = {'q': (B, N, C), 'dq0': (B, N, C), 'tab_h': (2 * Sh - 1, D), 'tab_w': (2 * Sw - 1, D), 'g_h': (B * H, N, Sh),
              'g_w': (B * H, N, Sw), 'dtab_h0': (2 * Sh - 1, D), 'dtab_w0': (2 * Sw - 1, D)}
    x = {}
    for n, s in shapes.items():
        if exact:
            lo, hi = (-3, 4) if n.startswith('dtab') else (-1, 2)
            x[n] = torch.randint(lo, hi, s, generator=g).double()
        else:
            v = torch.randn(s, generator=g, dtype=torch.float64) * (0.5 if n.startswith('tab') else 1.0)
            x[n] = v.to(dtype if n in ('q', 'dq0') else F32).double()
    return x


def _rel_index(S):
    return torch.arange(S)[:, None] - torch.arange(S)[None, :] + S - 1          # [q, k] -> table row


RELPOS_FAULTS = ('skip_last_kw_of_one_row', 'rel_w_unskewed_in_one_tile', 'dq_prior_overwritten', 'dtab_w_row0_dropped',
                 'one_copy_left_out_of_the_fold')


def relpos_math(case, x, wd=torch.float64, dtype=None, fault=None, bounds=False):
    """The formulas of the module docstring in the precision `wd`.  dtype: emulate that working dtype (round where its kernels round,
    sum the table gradients per workgroup); None: plain.  fault: one of RELPOS_FAULTS, planted.  -> (results, bounds or None)"""
    B, H, Sh, Sw, N, C = case.B, case.heads, case.Sh, case.Sw, case.N, case.C
    emu_bf16 = dtype == BF16
    mfma = dtype is not None and relpos_mfma_backward(dtype, Sh, Sw)
    q = x['q'].to(wd).view(B, Sh, Sw, H, D)
    th, tw = x['tab_h'].to(wd), x['tab_w'].to(wd)
    ih, iw = _rel_index(Sh), _rel_index(Sw)
    tf_h, tf_w = (_bf16(th), _bf16(tw)) if emu_bf16 else (th, tw)              # the bf16 forward stages its tables as bf16
    res = {'rel_h': torch.einsum('bhwnc,hkc->bnhwk', q, tf_h[ih]).reshape(B * H, N, Sh),
           'rel_w': torch.einsum('bhwnc,wkc->bnhwk', q, tf_w[iw]).reshape(B * H, N, Sw)}
    if fault == 'skip_last_kw_of_one_row':
        res['rel_w'][B * H - 1, N - 1, Sw - 1] = 0.0
    if fault == 'rel_w_unskewed_in_one_tile':       # P[q][j] = <q, Tw[2 Sw - 2 - j]> stored at kw = j for the first 16 queries of a row
        qw = torch.arange(min(16, Sw))
        rows = tw[(2 * Sw - 2 - torch.arange(Sw))]
        res['rel_w'].view(B, H, Sh, Sw, Sw)[0, 0, 0, qw] = torch.einsum('wc,kc->wk', q[0, 0, qw, 0], rows)
    g_h = x['g_h'].to(wd).view(B, H, Sh, Sw, Sh)
    g_w = x['g_w'].to(wd).view(B, H, Sh, Sw, Sw)
    gm_h, gm_w, tb_h, tb_w = (_bf16(g_h), _bf16(g_w), _bf16(th), _bf16(tw)) if mfma else (g_h, g_w, th, tw)
    inc = torch.einsum('bnhwk,hkc->bhwnc', gm_h, tb_h[ih]) + torch.einsum('bnhwk,wkc->bhwnc', gm_w, tb_w[iw])
    dq = inc.reshape(B, N, C) + (0.0 if fault == 'dq_prior_overwritten' else x['dq0'].to(wd))
    res['dq'] = _bf16(dq) if emu_bf16 else dq
    if fault == 'one_copy_left_out_of_the_fold':    # workgroup (b, qh) adds into copy (b Sh + qh) % 32 (RP_COPIES)
        keep = ((torch.arange(B)[:, None] * Sh + torch.arange(Sh)[None, :]) % 32 != 31).to(wd)
        assert not bool(keep.all())
        gm_h, gm_w = gm_h * keep[:, None, :, None, None], gm_w * keep[:, None, :, None, None]
    if dtype is None:
        ah = torch.zeros(2 * Sh - 1, D, dtype=wd).index_add_(0, ih.flatten(), torch.einsum('bnhwk,bhwnc->hkc', gm_h, q).reshape(-1, D))
        aw = torch.zeros(2 * Sw - 1, D, dtype=wd).index_add_(0, iw.flatten(), torch.einsum('bnhwk,bhwnc->wkc', gm_w, q).reshape(-1, D))
    else:                                           # one partial per workgroup (b, qh), added in workgroup order
        ah, aw = torch.zeros(2 * Sh - 1, D, dtype=wd), torch.zeros(2 * Sw - 1, D, dtype=wd)
        ph = torch.einsum('bnhwk,bhwnc->bhkc', gm_h, q)
        for b in range(B):
            for qh in range(Sh):
                ah[ih[qh]] += ph[b, qh]
                pw = torch.einsum('nwk,wnc->wkc', gm_w[b, :, qh], q[b, qh]).reshape(-1, D)
                aw += torch.zeros(2 * Sw - 1, D, dtype=wd).index_add_(0, iw.flatten(), pw)
    res['dtab_h'], res['dtab_w'] = x['dtab_h0'].to(wd) + ah, x['dtab_w0'].to(wd) + aw
    if fault == 'dtab_w_row0_dropped':
        res['dtab_w'][0] = x['dtab_w0'][0].to(wd)
    bnd = None
    if bounds:
        qa, gha, gwa = q.abs(), g_h.abs(), g_w.abs()
        bnd = {'rel_h': torch.einsum('bhwnc,hkc->bnhwk', qa, th.abs()[ih]).reshape(B * H, N, Sh),
               'rel_w': torch.einsum('bhwnc,wkc->bnhwk', qa, tw.abs()[iw]).reshape(B * H, N, Sw),
               'dq': x['dq0'].abs() + (torch.einsum('bnhwk,hkc->bhwnc', gha, th.abs()[ih]) +
                                       torch.einsum('bnhwk,wkc->bhwnc', gwa, tw.abs()[iw])).reshape(B, N, C),
               'dtab_h': x['dtab_h0'].abs() + torch.zeros(2 * Sh - 1, D, dtype=wd).index_add_(
                   0, ih.flatten(), torch.einsum('bnhwk,bhwnc->hkc', gha, qa).reshape(-1, D)),
               'dtab_w': x['dtab_w0'].abs() + torch.zeros(2 * Sw - 1, D, dtype=wd).index_add_(
                   0, iw.flatten(), torch.einsum('bnhwk,bhwnc->wkc', gwa, qa).reshape(-1, D))}
    return res, bnd


def relpos_exact_limits(case):
    """largest magnitude an exact-operand result may have: every one is an integer below 2^24, and dq (stored in bf16) at most 256"""
    return {'rel_h': D, 'rel_w': D, 'dq': case.Sh + case.Sw + 1, 'dtab_h': 2 ** 24, 'dtab_w': 2 ** 24}


# ================================================================================================ hyper-network product
@dataclass(frozen=True)
class Hyper:
    B: int
    T: int
    P: int

    @property
    def id(self):
        return f'b{self.B}-t{self.T}-p{self.P}'


HYPER_CASES = tuple(Hyper(B, T, P) for T in (1, 4, 8) for P in (1, 255, 256, 257, 1000) for B in (1, 3))
HC = 32


def hyper_inputs(case, dtype, exact):
    g = torch.Generator().manual_seed(_seed(case.id + ('x' if exact else DT_NAME[dtype])))
    shapes = {'x': (case.B, case.P, HC), 'hyper': (case.B, case.T, HC), 'dout': (case.B, case.T, case.P)}
    if not exact:
        return {n: torch.randn(s, generator=g, dtype=torch.float64).to(dtype).double() for n, s in shapes.items()}
    x = {n: torch.randint(-1, 2, s, generator=g).double() for n, s in shapes.items()}
    if dtype == BF16:           # at most 250 nonzero gradients per token: |dhyper| <= 256, another set of pixels for each token
        step = (case.P + 249) // 250
        p, t = torch.arange(case.P)[None, :], torch.arange(case.T)[:, None]
        x['dout'] = x['dout'] * ((p + t) % step == 0).double()
    return x


def hyper_math(case, x, wd=torch.float64, dtype=None, fault=None, bounds=False):
    xx, hy, do = (x[n].to(wd) for n in ('x', 'hyper', 'dout'))
    if fault == 'eighth_token_dropped':
        hy, do = hy.clone(), do.clone()
        hy[:, 7], do[:, 7] = 0.0, 0.0
    rnd = _bf16 if dtype == BF16 else (lambda t: t)
    res = {'hp_out': rnd(hy @ xx.transpose(1, 2)), 'hp_dx': rnd(do.transpose(1, 2) @ hy)}
    if dtype is None:
        res['hp_dhyper'] = do @ xx
    else:                       # one partial per block of 256 pixels, added in block order
        acc = torch.zeros(case.B, case.T, HC, dtype=wd)
        for p0 in range(0, case.P, 256):
            acc += do[:, :, p0:p0 + 256] @ xx[:, p0:p0 + 256]
        res['hp_dhyper'] = acc
    bnd = None
    if bounds:
        xa, ha, da = x['x'].abs(), x['hyper'].abs(), x['dout'].abs()
        bnd = {'hp_out': ha @ xa.transpose(1, 2), 'hp_dx': da.transpose(1, 2) @ ha, 'hp_dhyper': da @ xa}
    return res, bnd


# ================================================================================================ x4 bilinear
UP4_HW = ((1, 1), (1, 5), (2, 3), (15, 17), (16, 16), (17, 33), (24, 40), (3, 300), (33, 16))
UP4_PLANES = (1, 6)


def up4_matrix(n, clamp=True):
    """The x4 half-pixel bilinear operator along one axis as a dense float64 [4 n, n] matrix (ATen upsample_bilinear2d,
    align_corners = False): src = max(0.25 (d + 0.5) - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, n - 1), weights 1 - l1 and l1.
    Every weight is a multiple of 1/8.  clamp = False: the fault `i1 = i0 + 1` -- the tap past the last row reads nothing (zero)."""
    d = torch.arange(4 * n, dtype=torch.float64)
    src = (0.25 * (d + 0.5) - 0.5).clamp_min(0.0)
    i0 = src.floor().long()
    l1 = src - i0.double()
    W = torch.zeros(4 * n, n + 1, dtype=torch.float64)
    W[torch.arange(4 * n), i0] += 1.0 - l1
    i1 = (i0 + 1).clamp_max(n - 1) if clamp else i0 + 1
    W[torch.arange(4 * n), i1] += l1
    return W[:, :n].contiguous()


def up4(low, clamp=True):
    """[..., h, w] -> [..., 4 h, 4 w]"""
    return up4_matrix(low.shape[-2], clamp).to(low.dtype) @ low @ up4_matrix(low.shape[-1]).to(low.dtype).t()


def up4_adjoint(ghi):
    """[..., 4 h, 4 w] -> [..., h, w]: the gradient of up4 (and, the weights being >= 0, its magnitude sum when fed magnitudes)"""
    return up4_matrix(ghi.shape[-2] // 4).to(ghi.dtype).t() @ ghi @ up4_matrix(ghi.shape[-1] // 4).to(ghi.dtype)


def up4_exact_inputs(planes, h, w):
    """low = k / 8 with |k| <= 255 and d_hi = k / 8 with |k| <= 64: exact in bf16; every x4 weight product is a multiple of 1/64, so
    every output (<= 15 significant bits) and every gathered gradient (64 terms) is exact in fp32"""
    g = torch.Generator().manual_seed(_seed(f'up4-{planes}-{h}-{w}'))
    low = torch.randint(-255, 256, (planes, h, w), generator=g).double() / 8
    dhi = torch.randint(-64, 65, (planes, 4 * h, 4 * w), generator=g).double() / 8
    return low, dhi


# ================================================================================================ mask loss
GAMMAS = (2.0, 1.5, 3.0)
SCALES = (3.0, 12.0, 40.0)
BM = ((1, 1), (3, 4), (1, 4), (3, 1))
PLAIN_HW = ((2, 4), (64, 128), (65, 128), (130, 200))       # fp32 slabs of 8192 elements: 1, exactly 1, 2, 4 (the last partial); bf16 slabs of 16384: 1, 1, 1, 2
SLAB = {F32: 8192, BF16: 16384}                             # ML_THREADS * ML_CHUNKS * elements per 16-byte chunk


@dataclass(frozen=True)
class Mask:
    route: str                      # 'plain': logits [B, M, H, W] at full resolution; 'up4': low-resolution logits [B, M, h, w]
    h: int
    w: int
    B: int
    M: int
    gamma: float
    scale: float
    signs: tuple

    @property
    def id(self):
        return f'{self.route}-{self.h}x{self.w}-b{self.B}-m{self.M}-g{self.gamma}-s{self.scale:g}'


def _mask_cases(route, sizes):
    """every (gamma, scale) pair at every size; (B, M) and the signs of (c0, c1, c2) walk their lists so that each meets each size
    and each gamma"""
    out, i = [], 0
    for si, (h, w) in enumerate(sizes):
        for gi, gamma in enumerate(GAMMAS):
            for ci, scale in enumerate(SCALES):
                B, M = BM[(gi + ci + si) % 4]
                k = i % 8
                out.append(Mask(route, h, w, B, M, gamma, scale, (1 - 2 * (k & 1), 1 - (k & 2), 1 - ((k & 4) >> 1))))
                i += 1
    return tuple(out)


MASK_PLAIN_CASES = _mask_cases('plain', PLAIN_HW)
MASK_UP4_CASES = _mask_cases('up4', UP4_HW)


def mask_inputs(case, dtype):
    """-> logits [B, M, h, w] (rounded to dtype; low resolution on the up4 route), targets [B, 1, H, W] in {0, 1} (shared over M),
    coef [B, M, 3] with the case's signs (alternating over the masks), all float64"""
    g = torch.Generator().manual_seed(_seed(case.id + DT_NAME[dtype]))
    k = 4 if case.route == 'up4' else 1
    x = (torch.randn(case.B, case.M, case.h, case.w, generator=g, dtype=torch.float64) * case.scale).to(dtype).double()
    t = (torch.rand(case.B, 1, k * case.h, k * case.w, generator=g) > 0.6).double()
    mag = (torch.rand(case.B, case.M, 3, generator=g, dtype=torch.float64) + 0.5) * torch.tensor([20.0, 1.0, 1.0], dtype=torch.float64)
    flip = (1 - 2 * (torch.arange(case.B * case.M) % 2)).double().view(case.B, case.M, 1)
    coef = (mag * torch.tensor(case.signs, dtype=torch.float64) * flip).float().double()
    return x, t, coef


MASK_FAULTS = ('c1_c2_exchanged', 'gamma_minus_1_in_w_g', 'second_slab_left_out', 'no_clamp_at_last_row')


def mask_math(x, t, coef, gamma, thr, alpha=ALPHA, fault=None):
    """float64 reference of maskloss.hip's terms at the logits x [B, M, ...] (full resolution), targets t [B, 1, ...]: written so that
    no `1 - p` cancels (sigmoid(-x) is 1 - p).  -> per-element (focal, p t, p, t, x > thr and t > thr, x > thr or t > thr), the
    gradient with respect to x, and the gradient's bound"""
    p, pn = torch.sigmoid(x), torch.sigmoid(-x)
    bce = x.clamp_min(0.0) - x * t + torch.log1p(torch.exp(-x.abs()))
    om = p * (1 - t) + pn * t                                   # 1 - pt
    af = alpha * t + (1 - alpha) * (1 - t)
    w_g = om ** ((gamma - 1.0) if fault == 'gamma_minus_1_in_w_g' else gamma)
    sp = p * pn
    dfocal = af * (gamma * om ** (gamma - 1.0) * (-(sp * (2 * t - 1))) * bce + w_g * (p * (1 - t) - pn * t))
    c0, c1, c2 = (coef[:, :, i].reshape(coef.shape[0], coef.shape[1], *([1] * (x.dim() - 2))) for i in range(3))
    if fault == 'c1_c2_exchanged':
        c1, c2 = c2, c1
    grad = c0 * dfocal + (c1 * t + c2) * sp
    bound = c0.abs() * af * (gamma * bce + 1.0) + c1.abs() * t + c2.abs()
    pi, ti = x > thr, (t > thr).expand_as(x)
    terms = (af * w_g * bce, p * t, p, t.expand_as(x), (pi & ti).double(), (pi | ti).double())
    return terms, grad, bound


def mask_math_fp32(x, t, coef, gamma, alpha=ALPHA):
    """the kernels' own formulas (mask_term / pow_gamma / loss_grad) in fp32 torch -> per-element (focal, p t, p, t), gradient"""
    x, t, coef = x.float(), t.float(), coef.float()
    al, gm = torch.tensor(alpha, dtype=F32), torch.tensor(gamma, dtype=F32)
    e = torch.exp(-x.abs())
    p = torch.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    bce = x.clamp_min(0.0) - x * t + torch.log1p(e)
    om = 1.0 - (p * t + (1.0 - p) * (1.0 - t))
    af = al * t + (1.0 - al) * (1.0 - t)
    w_g = om * om if gamma == 2.0 else om.clamp_min(0.0) ** gm
    w_gm1 = om if gamma == 2.0 else om.clamp_min(0.0) ** (gm - 1.0)
    sp = p * (1.0 - p)
    dfocal = af * (gm * w_gm1 * (-(sp * (2.0 * t - 1.0))) * bce + w_g * (p - t))
    c0, c1, c2 = (coef[:, :, i].reshape(coef.shape[0], coef.shape[1], *([1] * (x.dim() - 2))) for i in range(3))
    return (af * w_g * bce, p * t, p, t.expand_as(x)), c0 * dfocal + (c1 * t + c2) * sp


def _sums(terms, skip=None):
    """[B, M, ...] terms -> [B, M] sums; skip: a (first, last) range of flat pixel indices left out (a fault's handle)"""
    out = []
    for v in terms:
        v = v.flatten(2)
        if skip is not None:
            v = v.clone()
            v[:, :, skip[0]:skip[1]] = 0
        out.append(v.sum(-1))
    return out


def mask_reference(case, x, t, coef, thr=0.0, fault=None, slab=None):
    """float64 results and bounds of one case -> (res, bnd); res also carries the two IoU counts (exact integers, no bound).
    On the up4 route x is the low-resolution tensor: the loss is taken at U x and the gradient brought back by U^T."""
    pre = 'up_' if case.route == 'up4' else 'ml_'
    xf = up4(x, clamp=fault != 'no_clamp_at_last_row') if case.route == 'up4' else x
    terms, grad, gb = mask_math(xf, t, coef, case.gamma, thr, fault=fault)
    sums = _sums(terms, (slab, 2 * slab) if fault == 'second_slab_left_out' else None)
    res = {pre + n: s for n, s in zip(SUMS, sums[:4])}
    res['count_and'], res['count_or'] = sums[4], sums[5]
    bnd = {pre + n: s.clone() for n, s in zip(SUMS, _sums(terms[:4]))}         # every term is >= 0
    res[pre + 'grad'] = up4_adjoint(grad) if case.route == 'up4' else grad
    bnd[pre + 'grad'] = up4_adjoint(gb) if case.route == 'up4' else gb
    return res, bnd


def mask_emulate(case, x, t, coef, dtype):
    """fp32 torch: F.interpolate and its backward on the up4 route, the kernels' formulas, fp32 sums; the bf16 gradient rounded once"""
    pre = 'up_' if case.route == 'up4' else 'ml_'
    if case.route == 'up4':
        low = x.float().requires_grad_(True)
        xf = F.interpolate(low, scale_factor=4, mode='bilinear', align_corners=False)
        terms, grad = mask_math_fp32(xf.detach(), t, coef, case.gamma)
        grad, = torch.autograd.grad(xf, low, grad)
    else:
        terms, grad = mask_math_fp32(x, t, coef, case.gamma)
    res = {pre + n: v.flatten(2).sum(-1) for n, v in zip(SUMS, terms)}
    res[pre + 'grad'] = _bf16(grad) if dtype == BF16 else grad
    return res


def count_inputs(route, h, w, thr, dtype, B=2, M=3):
    """Dyadic logits k / 8 (exact in bf16, and every x4 interpolation of them exact in fp32), half of them drawn from {0, 0.5}, the
    first plane wholly equal to thr -- so logits exactly AT the threshold occur, directly and as interpolated values -- and targets
    in {0, 1}"""
    g = torch.Generator().manual_seed(_seed(f'count-{route}-{h}-{w}-{thr}'))
    k = 4 if route == 'up4' else 1
    x = torch.randint(-255, 256, (B, M, h, w), generator=g).double() / 8
    ties = torch.randint(0, 2, (B, M, h, w), generator=g).double() / 2
    x = torch.where(torch.rand(B, M, h, w, generator=g) < 0.5, ties, x)
    x[0, 0] = thr
    t = (torch.rand(B, 1, k * h, k * w, generator=g) > 0.6).double()
    return x.to(dtype).double(), t


# ================================================================================================ windows
# (B, H, W, C, ws, dtypes).  Both kernels walk 16-byte chunks (C / 4 per token in fp32, C / 8 in bf16) with a grid capped at
# WINDOW_GRID_CAP threads: window_partition over the padded grid, window_unpartition over B H W.
WINDOW_GRID_CAP = 4096 * 256                                # sgrid() in csrc/sam.hip: at most 4096 blocks of 256 threads
WINDOW_CASES = ((2, 5, 9, 8, 14, ('f32', 'bf16')),          # H and W below the window
                (1, 14, 14, 8, 14, ('f32', 'bf16')),
                (2, 15, 29, 32, 14, ('f32', 'bf16')),
                (1, 7, 7, 8, 1, ('f32', 'bf16')),
                (2, 70, 70, 384, 14, ('f32',)),             # 940,800 chunk items (70 = 5 x 14: no padding): 3675 blocks, just below the cap
                (3, 70, 70, 384, 14, ('f32',)),             # 1,411,200: the grid-stride loop takes a second pass in fp32
                (3, 70, 70, 768, 14, ('bf16',)))            # SAM-B at 1024 with batch 3, 1,411,200: a second pass in bf16
WINDOW_SECOND_PASS = {'f32': (3, 70, 70, 384, 14), 'bf16': (3, 70, 70, 768, 14)}


def window_items(B, H, W, C, ws, dt):
    """-> (chunk items of window_partition, of window_unpartition)"""
    per = C // (8 if dt == 'bf16' else 4)
    nwh, nww = (H + ws - 1) // ws, (W + ws - 1) // ws
    return B * nwh * nww * ws * ws * per, B * H * W * per


def window_reference(x, ws):
    B, H, W, C = x.shape
    ph, pw = (ws - H % ws) % ws, (ws - W % ws) % ws
    xp = F.pad(x, (0, 0, 0, pw, 0, ph))
    hp, wp = H + ph, W + pw
    return xp.view(B, hp // ws, ws, wp // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C).contiguous()


# ================================================================================================ the judge
def ratio(got, ref, bound, u, extra=None):
    """worst |got - ref| / (u * bound) over every element (after taking off `extra`, an absolute allowance per element); inf for a NaN,
    or for a nonzero error where the bound is 0"""
    g = got.double().reshape(ref.shape)
    err = (g - ref).abs()
    if extra is not None:
        err = (err - extra).clamp_min(0.0)
    b = bound * u
    r = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    r = torch.where(torch.isnan(g), torch.full_like(r, math.inf), r)
    return float(r.max()) if r.numel() else 0.0


def ratios(got, ref, bnd, dtype):
    """-> {quantity: worst ratio} for every quantity of bnd that got carries"""
    out = {}
    for n, b in bnd.items():
        if n in got:
            extra = half_ulp_bf16(ref[n]) if (dtype == BF16 and n.endswith('_grad')) else None
            out[n] = ratio(got[n], ref[n], b, unit(n, dtype), extra)
    return out


def misses(rat, dtype):
    return {n: (r, MARGIN * constant(n, dtype)) for n, r in rat.items() if not r <= MARGIN * constant(n, dtype)}


# ================================================================================================ device side (needs a GPU)
def _api():
    from simpleaicv_pytorch_training_examples_amd._lib import dtype_code, lib, ptr, stream
    return lib(), dtype_code, ptr, stream


def last_error():
    lib = _api()[0]
    msg = lib.saicv_last_error_string()
    return msg.decode() if msg else ''


def _ok(rc, what):
    assert rc == 0, f'{what} returned {rc}: {last_error()}'


def _filled(shape, dtype, values, device='cuda'):
    """a Guarded buffer of `shape` (contiguous) holding `values`"""
    st, n = [], 1
    for s in reversed(shape):
        st.insert(0, n)
        n *= s
    gd = Guarded(tuple(shape), tuple(st), dtype, device)
    if values is not None:
        gd.view.copy_(values.to(dtype).to(device))
    return gd


KV_MARK = 5.0                       # what the k / v slices of the packed gradient buffer hold before the launch


def run_relpos(case, x, dtype, tables=True, device='cuda'):
    """saicv_relpos_fwd and saicv_relpos_bwd on one case -> (results as float64 CPU tensors, complaints).  rel_h / rel_w are
    pre-filled with NaN; dq is the q slice of a packed [B, N, 3C] gradient buffer that holds the prior dq (k / v slices: KV_MARK);
    the table gradients hold their priors; the workspace is NaN (the atomic path has to clear it itself)."""
    lib, dtype_code, ptr, stream = _api()
    B, H, Sh, Sw, N, C = case.B, case.heads, case.Sh, case.Sw, case.N, case.C
    W = C if case.contiguous else 3 * C
    qbuf = torch.randn(B, N, W, device=device).to(dtype)
    qbuf[:, :, :C] = x['q'].to(dtype).to(device)
    q = qbuf[:, :, :C]
    th, tw, gh, gw = (x[n].float().contiguous().to(device) for n in ('tab_h', 'tab_w', 'g_h', 'g_w'))
    g_rh, g_rw = _filled((B * H, N, Sh), F32, None, device), _filled((B * H, N, Sw), F32, None, device)
    _ok(lib.saicv_relpos_fwd(dtype_code(dtype), ptr(q), q.stride(1), q.stride(0), ptr(th), ptr(tw), ptr(g_rh.view), ptr(g_rw.view),
                             B, H, Sh, Sw, stream()), 'relpos_fwd')
    prior = torch.full((B, N, W), KV_MARK, dtype=torch.float64)
    prior[:, :, :C] = x['dq0']
    g_dq = _filled((B, N, W), dtype, prior, device)
    dq = g_dq.view[:, :, :C]
    guards = [('rel_h', g_rh), ('rel_w', g_rw), ('dq', g_dq)]
    g_th = g_tw = ws = None
    if tables:
        g_th, g_tw = _filled((2 * Sh - 1, D), F32, x['dtab_h0'], device), _filled((2 * Sw - 1, D), F32, x['dtab_w0'], device)
        ws = torch.full((lib.saicv_relpos_bwd_ws_floats(Sh, Sw),), math.nan, dtype=F32, device=device)
        guards += [('dtab_h', g_th), ('dtab_w', g_tw)]
    _ok(lib.saicv_relpos_bwd(dtype_code(dtype), ptr(q), ptr(dq), q.stride(1), q.stride(0), ptr(th), ptr(tw), ptr(gh), ptr(gw),
                             ptr(g_th.view if tables else None), ptr(g_tw.view if tables else None), ptr(ws), B, H, Sh, Sw, stream()),
        'relpos_bwd')
    torch.cuda.synchronize()
    got = {'rel_h': g_rh.view.double().cpu(), 'rel_w': g_rw.view.double().cpu(), 'dq': dq.double().cpu()}
    if tables:
        got['dtab_h'], got['dtab_w'] = g_th.view.double().cpu(), g_tw.view.double().cpu()
    bad = [msg for name, g in guards for msg in g.check(name)]
    if W > C and not bool((g_dq.view[:, :, C:] == KV_MARK).all()):
        bad.append('dq: the k / v slices of the packed gradient buffer were written')
    return got, bad


def run_hyper(case, x, dtype, device='cuda'):
    lib, dtype_code, ptr, stream = _api()
    B, T, P = case.B, case.T, case.P
    xd, hd, dd = (x[n].to(dtype).contiguous().to(device) for n in ('x', 'hyper', 'dout'))
    g_out, g_dx, g_dh = _filled((B, T, P), dtype, None, device), _filled((B, P, HC), dtype, None, device), _filled((B, T, HC), F32, None, device)
    _ok(lib.saicv_hyper_product_fwd(dtype_code(dtype), ptr(xd), ptr(hd), ptr(g_out.view), B, T, P, HC, stream()), 'hyper_product_fwd')
    _ok(lib.saicv_hyper_product_bwd(dtype_code(dtype), ptr(xd), ptr(hd), ptr(dd), ptr(g_dx.view), ptr(g_dh.view), B, T, P, HC, stream()),
        'hyper_product_bwd')
    torch.cuda.synchronize()
    got = {'hp_out': g_out.view.double().cpu(), 'hp_dx': g_dx.view.double().cpu(), 'hp_dhyper': g_dh.view.double().cpu()}
    return got, [m for n, g in (('out', g_out), ('dx', g_dx), ('dhyper', g_dh)) for m in g.check(n)]


def run_up4(low, dhi, dtype, device='cuda'):
    lib, dtype_code, ptr, stream = _api()
    planes, h, w = low.shape
    ld, gd = low.to(dtype).contiguous().to(device), dhi.to(dtype).contiguous().to(device)
    g_out, g_dl = _filled((planes, 4 * h, 4 * w), dtype, None, device), _filled((planes, h, w), dtype, None, device)
    _ok(lib.saicv_upsample4_fwd(dtype_code(dtype), ptr(ld), ptr(g_out.view), planes, h, w, stream()), 'upsample4_fwd')
    _ok(lib.saicv_upsample4_bwd(dtype_code(dtype), ptr(gd), ptr(g_dl.view), planes, h, w, stream()), 'upsample4_bwd')
    torch.cuda.synchronize()
    return {'out': g_out.view.double().cpu(), 'dlow': g_dl.view.double().cpu()}, g_out.check('out') + g_dl.check('dlow')


def run_mask(route, x, t, coef, gamma, thr, dtype, alpha=ALPHA, device='cuda', raw=False):
    """the stats and the gradient kernel of one route -> (results, complaints).  stats [B, M, 6] come back as the four sums and the
    two counts; raw: also the gradient tensor as the device holds it (for bit comparisons)"""
    lib, dtype_code, ptr, stream = _api()
    B, M, h, w = x.shape
    pre = 'up_' if route == 'up4' else 'ml_'
    xd, td, cd = x.to(dtype).contiguous().to(device), t.float().contiguous().to(device), coef.float().contiguous().to(device)
    g_st, g_gr = _filled((B, M, 6), F32, None, device), _filled((B, M, h, w), dtype, None, device)
    if route == 'up4':
        _ok(lib.saicv_mask_loss_stats_up4(dtype_code(dtype), ptr(xd), ptr(td), ptr(g_st.view), B, M, h, w, alpha, gamma, thr, stream()),
            'mask_loss_stats_up4')
        _ok(lib.saicv_mask_loss_grad_up4(dtype_code(dtype), ptr(xd), ptr(td), ptr(cd), ptr(g_gr.view), B, M, h, w, alpha, gamma, stream()),
            'mask_loss_grad_up4')
    else:
        _ok(lib.saicv_mask_loss_stats(dtype_code(dtype), ptr(xd), ptr(td), ptr(g_st.view), B, M, h * w, alpha, gamma, thr, stream()),
            'mask_loss_stats')
        _ok(lib.saicv_mask_loss_grad(dtype_code(dtype), ptr(xd), ptr(td), ptr(cd), ptr(g_gr.view), B, M, h * w, alpha, gamma, stream()),
            'mask_loss_grad')
    torch.cuda.synchronize()
    st = g_st.view.double().cpu()
    got = {pre + n: st[:, :, i] for i, n in enumerate(SUMS)}
    got['count_and'], got['count_or'] = st[:, :, 4], st[:, :, 5]
    got[pre + 'grad'] = g_gr.view.double().cpu()
    if raw:
        got['raw_grad'], got['raw_stats'] = g_gr.view.cpu().clone(), g_st.view.cpu().clone()
    return got, g_st.check('stats') + g_gr.check('grad')


def run_window(x, add, ws, device='cuda'):
    """-> (windows, un-partitioned, un-partitioned + addend) as CPU tensors of x's dtype, complaints"""
    lib, dtype_code, ptr, stream = _api()
    B, H, W, C = x.shape
    nwh, nww = (H + ws - 1) // ws, (W + ws - 1) // ws
    xd, ad = x.contiguous().to(device), add.contiguous().to(device)
    g_win = _filled((B * nwh * nww, ws * ws, C), x.dtype, None, device)
    g_back, g_fused = _filled((B, H, W, C), x.dtype, None, device), _filled((B, H, W, C), x.dtype, None, device)
    dc = dtype_code(x.dtype)
    _ok(lib.saicv_window_partition(dc, ptr(xd), ptr(g_win.view), B, H, W, C, ws, stream()), 'window_partition')
    _ok(lib.saicv_window_unpartition(dc, ptr(g_win.view), 0, ptr(g_back.view), B, H, W, C, ws, stream()), 'window_unpartition')
    _ok(lib.saicv_window_unpartition(dc, ptr(g_win.view), ptr(ad), ptr(g_fused.view), B, H, W, C, ws, stream()), 'window_unpartition')
    torch.cuda.synchronize()
    bad = g_win.check('windows') + g_back.check('unpartition') + g_fused.check('unpartition + addend')
    return g_win.view.cpu(), g_back.view.cpu(), g_fused.view.cpu(), bad
