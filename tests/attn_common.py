"""What tests/test_attn_judge_host.py (no GPU), tests/test_gpu_attn_f64.py and tests/attn_fwd2_worker.py (MI355X) share: the case
table of every attention kernel form, the input builder, the float64 reference with hand-written gradients, the restated
dropout mask, the working-precision emulations that set the constants, and the componentwise judge.

Reference (float64, over the values the device holds: inputs are rounded to the compute dtype first):
    logits = scale * q.k + key_bias[b, k] + rel_h[bh, q, k // Sw] + rel_w[bh, q, k % Sw]
    P = softmax(logits)        lse = logsumexp(logits)  (undropped)        Pd = P o M / (1 - p)        out = Pd v
    dP = dout v^T    dsum = rowsum(dout o out)    dS = P o (M o dP / (1 - p) - dsum)
    dq = scale dS k    dk = scale dS^T q    dv = Pd^T dout    d_rel_h = sum_kw dS    d_rel_w = sum_kh dS

Judge: an element passes when |got - ref| <= 4 * c * u * bound.  u = 2^-24 (fp32) or 2^-9 (bf16); bound is the magnitude sum of
the element's own expression in float64:
    out  Pd |v|          dv  Pd^T |dout|          mS = P o (|M o dP / (1 - p)| + sum_k Pd |dP|)
    dq   scale mS |k|    dk  scale mS^T |q|       d_rel_*  the matching sums of mS        lse  1 + |lse|  (absolute)
A large-logit case (Case.large) multiplies each query row of Pd and mS, and the lse unit, by 1 + max_k sum_d |q_d k_d| scale:
an error in a logit scales the error in P by the logit's size.  An element whose bound is 0 (every key of the row dropped) must
be exactly 0.  Nothing is sampled or left out.

The constants c are the worst ratio |cand - ref| / (u * bound) over the WHOLE case table of a CPU implementation in the working
precision (emulate()): plain fp32 torch for fp32; for bf16 an fp32 emulation that rounds to bf16 where csrc/attn_stream.hip does --
P / Pd before P.V and Pd^T.dout, dS before dS.K and dS^T.Q (and before the REL 1 table gradients, which ride on the same MFMA
operand), the REL 1 tables R = rel / scale (SARel: "bf16 mode rounds R to bf16"), and every stored output (dsum is taken from the
stored out).  The margin of 4 stands for what a kernel may do differently from that emulation: another summation order, the
online-softmax rescaling, v_exp_f32 in the log2 domain, LDS atomics in the generic table form.  test_attn_judge_host.py measures
the constants and holds CONSTANTS to them; they are never raised by hand.
"""
import math
from dataclasses import dataclass

import numpy as np
import torch

U = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -9}
DT_NAME = {torch.float32: 'f32', torch.bfloat16: 'bf16'}
MARGIN = 4.0
QUANTITIES = ('out', 'lse', 'dq', 'dk', 'dv', 'd_rel_h', 'd_rel_w', 'dq@mag', 'dk@mag', 'd_rel_h@mag', 'd_rel_w@mag')

# Worst ratio of emulate() to the float64 reference over every case of the table, in units of u * bound.
# Measured 2026-10-17 with torch 2.10.0+rocm7.0 (CPU, one thread) by tests/test_attn_judge_host.py::test_constants_table_is_what_the_emulations_measure
# (which fails if a row drifts by more than a quarter); the judge allows MARGIN times these.
CONSTANTS = {
    #                 stated bounds                                                    magnitude-sum bounds (see attention_math)
    torch.float32: {'out': 14.1, 'lse': 5.05, 'dq': 669.0, 'dk': 31.1, 'dv': 21.7, 'd_rel_h': 14.3, 'd_rel_w': 20.3,
                    'dq@mag': 4.52, 'dk@mag': 5.26, 'd_rel_h@mag': 2.71, 'd_rel_w@mag': 5.60},
    torch.bfloat16: {'out': 3.50, 'lse': 0.507, 'dq': 182.0, 'dk': 5.50, 'dv': 3.80, 'd_rel_h': 3.58, 'd_rel_w': 4.44,
                     'dq@mag': 1.58, 'dk@mag': 1.36, 'd_rel_h@mag': 1.02, 'd_rel_w@mag': 0.700},
}
CONSTANTS_MEASURED_WITH = 'torch 2.10.0+rocm7.0, 2026-10-17'


# ------------------------------------------------------------------------------------------------ the case table
@dataclass(frozen=True)
class Case:
    id: str
    B: int
    H: int
    D: int
    Nq: int
    Nk: int
    bias: float = None          # key-bias value on the padded keys (None: no key bias)
    p: float = 0.0              # dropout probability
    rel: tuple = None           # (Sh, Sw)
    layout: str = 'sep'         # sep | packed | qk_v | wide | seqfirst | packed_qk_fn
    pattern: str = None         # ramp | spike | flat: the large-logit inputs of test_gpu_sam's deferred-rescale test
    qscale: float = 1.0
    seed: int = 0               # host dropout seed handed to the kernels
    dtypes: tuple = ('f32', 'bf16')

    @property
    def large(self):
        return self.pattern is not None or self.qscale != 1.0

    @property
    def shared_inputs(self):
        """a big case builds inputs that are exact in bf16, so that one float64 reference serves both compute dtypes"""
        return self.B * self.H * self.Nq * self.Nk > (1 << 21)

    @property
    def scale(self):
        return self.D ** -0.5

    @property
    def rel_mode(self):
        """the REL template argument sa_dispatch selects (csrc/attn_stream.hip)"""
        if self.rel is None:
            return 0
        sh, sw = self.rel
        if sw == 64:
            return 2
        return 1 if (sh + sw <= 32 and self.Nk <= 256) else 3


NQ_SWEEP = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129)
NK_SWEEP = (1, 5, 63, 64, 65, 127, 128, 129, 191, 192, 193)
BIAS_VALUES = (1.0, -1e4)       # DETR's float key-padding mask, and a mask that removes the key
DROP_VALUES = (0.1, 0.5)


def _sweeps():
    """Every Nq of NQ_SWEEP and every Nk of NK_SWEEP for the plain, key-bias, dropout and dropout + key-bias forms at both head
    dims: the partner length walks the other list so that the 16 / 32 / 64 / 128 boundaries meet each other in many pairs."""
    cases, n = [], 0
    for D in (32, 64):
        for form in ('plain', 'kb', 'drop', 'dropkb'):
            pairs = [(nq, NK_SWEEP[(3 * i + n) % len(NK_SWEEP)]) for i, nq in enumerate(NQ_SWEEP)]
            pairs += [(NQ_SWEEP[(3 * j + n + 1) % len(NQ_SWEEP)], nk) for j, nk in enumerate(NK_SWEEP)]
            for i, (nq, nk) in enumerate(dict.fromkeys(pairs)):
                bias = BIAS_VALUES[i % 2] if 'kb' in form else None
                p = DROP_VALUES[(i // 2) % 2] if 'drop' in form else 0.0
                b, h = ((2, 2), (1, 3), (2, 1))[i % 3]
                cases.append(Case(f'{form}-d{D}-q{nq}-k{nk}', b, h, D, nq, nk, bias=bias, p=p, seed=1000 + 7 * n + i))
            n += 1
    return cases


def _table():
    c = _sweeps()
    # relative-position forms (head dim 64 only)
    c += [Case('rel1-14x14', 1, 3, 64, 196, 196, rel=(14, 14)),
          Case('rel1-16x16', 2, 1, 64, 256, 256, rel=(16, 16)),
          Case('rel1-4x20', 1, 2, 64, 80, 80, rel=(4, 20)),
          Case('rel2-1x64', 1, 3, 64, 70, 64, rel=(1, 64)),
          Case('rel2-3x64', 2, 2, 64, 192, 192, rel=(3, 64)),
          Case('rel2-5x64', 1, 2, 64, 129, 320, rel=(5, 64)),
          Case('rel2-64x64-sam-global', 1, 1, 64, 4096, 4096, rel=(64, 64)),
          Case('rel2kb-3x64-plus1', 2, 2, 64, 100, 192, rel=(3, 64), bias=1.0),
          Case('rel2kb-5x64-minus1e4', 2, 1, 64, 33, 320, rel=(5, 64), bias=-1e4),
          Case('rel3-20x20', 1, 2, 64, 400, 400, rel=(20, 20)),
          # Sh + Sw = 94 is the widest the fp32 dQ kernel's LDS tables allow, 126 the widest of the bf16 one (attention_stream)
          Case('rel3-47x47', 1, 2, 64, 40, 2209, rel=(47, 47)),
          Case('rel3-62x63-bf16', 1, 1, 64, 33, 3906, rel=(62, 63), dtypes=('bf16',))]
    # model shapes
    c += [Case('vit-197-12heads', 1, 12, 64, 197, 197, layout='packed'),
          Case('vit-196-12heads', 1, 12, 64, 196, 196, layout='packed'),
          Case('detr-cross-100x1764', 2, 2, 32, 100, 1764, bias=1.0, p=0.1, seed=77),
          Case('detr-self-1764x1764', 2, 2, 32, 1764, 1764, bias=1.0, p=0.1, seed=78, layout='qk_v')]
    # layouts
    c += [Case('layout-packed-d32-drop', 2, 2, 32, 70, 70, p=0.1, layout='packed', seed=5),
          Case('layout-qk_v-d32-kb', 2, 2, 32, 130, 130, bias=1.0, layout='qk_v'),
          Case('layout-wide-d64', 2, 2, 64, 65, 129, layout='wide'),
          Case('layout-wide-d32-dropkb', 2, 2, 32, 33, 70, bias=1.0, p=0.5, layout='wide', seed=6),
          Case('layout-seqfirst-d32-kb', 3, 2, 32, 100, 130, bias=1.0, layout='seqfirst'),
          Case('layout-seqfirst-d64', 2, 2, 64, 129, 65, layout='seqfirst'),
          Case('layout-packed_qk_fn-d32-dropkb', 2, 2, 32, 130, 130, bias=1.0, p=0.1, layout='packed_qk_fn')]
    # large logits (the patterns of test_gpu_sam.test_stream_attention_forward_deferred_rescale_branch), gradients included
    for pat in ('ramp', 'spike', 'flat'):
        c += [Case(f'large-{pat}', 1, 2, 64, 512, 512, pattern=pat),
              Case(f'large-{pat}-rel2', 1, 2, 64, 512, 512, pattern=pat, rel=(8, 64))]
    c += [Case('large-q4-d32-kb', 2, 2, 32, 129, 193, bias=1.0, qscale=4.0),
          Case('large-q4-d64-drop', 1, 2, 64, 65, 130, p=0.1, qscale=4.0, seed=9)]
    ids = [x.id for x in c]
    assert len(set(ids)) == len(ids)
    return tuple(c)


STREAM_CASES = _table()
WHOLE_N = (1, 17, 31, 32, 33, 63, 64, 65, 196, 197, 255, 256)
WHOLE_CASES = tuple(Case(f'whole-n{n}', 2, 2, 64, n, n, layout='packed') for n in WHOLE_N)


# ------------------------------------------------------------------------------------------------ kernel forms
def stream_form(dt, D, rel, drop, kb, which, fwd2_env=1):
    """Name of the template instantiation sa_dispatch / sa_launch (csrc/attn_stream.hip) select.  which: 0 forward, 1 dQ, 2 dK/dV;
    fwd2_env: the value of SAICV_SA_FWD2 (default 1)."""
    tail = f'{dt},D{D},REL{rel},DROP{int(drop)},KB{int(kb)}'
    if which == 1:
        return f'sa_bwd_dq<{tail}>'
    if which == 2:
        return f'sa_bwd_dkv<{tail}>'
    if dt == 'bf16' and not drop and rel <= 2:
        fwd2 = fwd2_env == 2 or (fwd2_env == 1 and rel != 1)
        if fwd2 and (rel == 0 or not kb):
            return f'sa_fwd2<{dt},D{D},REL{rel},KB{int(kb)}>'
    return f'sa_fwd<{tail}>'


def stream_combos():
    """(D, REL, DROP, KB) of every sa_launch instantiation in sa_dispatch"""
    combos = [(D, 0, drop, kb) for D in (32, 64) for drop in (False, True) for kb in (False, True)]
    return combos + [(64, 1, False, False), (64, 2, False, False), (64, 2, False, True), (64, 3, False, False)]


def all_stream_forms():
    return {stream_form(dt, D, rel, drop, kb, which, env) for dt in ('f32', 'bf16') for (D, rel, drop, kb) in stream_combos()
            for which in (0, 1, 2) for env in (0, 1, 2)}


def case_forms(case, dt, whiches=(0, 1, 2), fwd2_env=1):
    return {stream_form(dt, case.D, case.rel_mode, case.p > 0, case.bias is not None, w, fwd2_env) for w in whiches}


def fwd2_eligible(case):
    """bf16 forward launches whose kernel depends on SAICV_SA_FWD2"""
    return 'bf16' in case.dtypes and case.p == 0 and case.rel_mode <= 2 and case.layout != 'packed_qk_fn'


WHOLE_FORMS = ('attention_fwd<f32>', 'attention_fwd<bf16>', 'attention_bwd<f32>', 'attention_bwd<bf16>',
               'attention_bwd2<2>', 'attention_bwd2<1>')


def whole_bwd_form(dt, mode):
    """saicv_attention_bwd's dispatch on SAICV_ATTN_BWD2 (csrc/tfm.hip); mode None: unset"""
    if dt == 'bf16' and mode in ('1', '2'):
        return 'attention_bwd2<2>' if mode == '1' else 'attention_bwd2<1>'      # =1: two tiles per wavefront, =2: one
    return f'attention_bwd<{dt}>'


# ------------------------------------------------------------------------------------------------ inputs
def _seed_of(case):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(case.id)) % (2 ** 31)


def build_inputs(case):
    """-> dict of float64 CPU tensors before rounding: q [B, Nq, C], k / v [B, Nk, C], dout [B, Nq, C], key_bias [B, Nk] or None,
    rel_h [B*H, Nq, Sh] / rel_w [B*H, Nq, Sw] or None (fp32 values: the kernels take them in fp32 for either compute dtype)."""
    g = torch.Generator().manual_seed(_seed_of(case))
    B, H, D, Nq, Nk = case.B, case.H, case.D, case.Nq, case.Nk
    C = H * D
    q = torch.randn(B, Nq, C, dtype=torch.float64, generator=g) * case.qscale
    k = torch.randn(B, Nk, C, dtype=torch.float64, generator=g)
    v = torch.randn(B, Nk, C, dtype=torch.float64, generator=g)
    dout = torch.randn(B, Nq, C, dtype=torch.float64, generator=g)
    if case.pattern == 'ramp':
        k = k * (1.0 + 0.9 * (torch.arange(Nk) // 64).double())[None, :, None]
        q = q * 2.0
    elif case.pattern == 'spike':
        k[0, 5 * 64 + 7, :D] = q[0, 33, :D] * 6.0
    elif case.pattern == 'flat':
        q = torch.zeros_like(q)
    if case.shared_inputs:
        q, k, v, dout = (t.to(torch.bfloat16).double() for t in (q, k, v, dout))
    key_bias = None
    if case.bias is not None:
        # padded keys: the tail of each batch element's key row, of another length per element; key 0 is never padded
        key_bias = torch.zeros(B, Nk, dtype=torch.float64)
        for b in range(B):
            first = max(1, int(math.ceil(Nk * (0.55 + 0.2 * b / max(1, B)))))
            key_bias[b, first:] = case.bias
        key_bias = key_bias.float().double()
    rel_h = rel_w = None
    if case.rel is not None:
        rel_h = torch.randn(B * H, Nq, case.rel[0], dtype=torch.float64, generator=g).float().double()
        rel_w = torch.randn(B * H, Nq, case.rel[1], dtype=torch.float64, generator=g).float().double()
    return {'q': q, 'k': k, 'v': v, 'dout': dout, 'key_bias': key_bias, 'rel_h': rel_h, 'rel_w': rel_w}


def rounded(inp, dtype):
    """the same inputs as the device holds them: q / k / v / dout rounded to the compute dtype (still float64 tensors)"""
    out = dict(inp)
    for n in ('q', 'k', 'v', 'dout'):
        out[n] = inp[n].to(dtype).double()
    return out


# ------------------------------------------------------------------------------------------------ dropout mask
def drop_threshold(p):
    """sa_thresh: (unsigned) fminf(p * 2^32, 4294967040.f) in fp32"""
    return int(min(np.float32(p) * np.float32(4294967296.0), np.float32(4294967040.0)))


def keep_prob(p):
    """1 - p as the kernels see p: the descriptor carries a float"""
    return 1.0 - float(np.float32(p))


def keep_mask(seed, BH, Nq, Nk, p, bh_term=None):
    """sa_keep restated on uint32 with wrapping arithmetic -> bool [BH, Nq, Nk] (True: the probability survives).
    bh_term: the batch*head index that enters the hash, per head (a fault's handle; default the head's own)."""
    M32 = np.uint64(0xffffffff)
    q = np.arange(Nq, dtype=np.uint64)[None, :, None]
    key = np.arange(Nk, dtype=np.uint64)[None, None, :]
    bh = np.asarray(range(BH) if bh_term is None else bh_term, dtype=np.uint64)[:, None, None]
    h = (q * np.uint64(Nk) + key) & M32
    h = h ^ np.uint64(int(seed) & 0xffffffff)
    h = (h + bh * np.uint64(0x9E3779B9)) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85ebca6b)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xc2b2ae35)) & M32
    h ^= h >> np.uint64(16)
    return torch.from_numpy(h >= np.uint64(drop_threshold(p)))


def effective_seed(seed, step_word):
    """the kernels add the device-side step word (ops_tfm.dropout_step_word) to the host seed, uint32"""
    return (int(seed) + int(step_word)) & 0xffffffff


# ------------------------------------------------------------------------------------------------ the arithmetic
FAULTS = ('skip_last_key_in_one_row', 'bias_ignored_in_partial_chunk', 'mask_without_bh_for_one_head', 'mask_seed_plus_1_in_dkv',
          'lse_from_dropped', 'dsum_from_undropped_out', 'dk_without_keep_scale', 'dk_without_scale', 'stale_row_of_a_tile',
          'rel_w_indexed_by_kh')


def _heads(x, H):
    B, N, C = x.shape
    return x.view(B, N, H, C // H).permute(0, 2, 1, 3).reshape(B * H, N, C // H)


def _unheads(x, B):
    BH, N, D = x.shape
    return x.view(B, BH // B, N, D).permute(0, 2, 1, 3).reshape(B, N, (BH // B) * D)


def _bf16(x):
    return x.to(torch.bfloat16).to(x.dtype)


def attention_math(case, inp, seed, wd=torch.float64, bf16_points=False, fault=None, grads=True, bounds=False):
    """The formulas of the module docstring in the precision `wd`.  seed: the effective dropout seed.  bf16_points: round where the
    bf16 kernels do.  fault: one of FAULTS, planted into the computation.  bounds: also return the magnitude sums (float64 only).
    -> (results, bounds) with q-like tensors as [B, N, C], lse [B*H, Nq], d_rel_* [B*H, Nq, S]."""
    B, H, Nq, Nk, scale = case.B, case.H, case.Nq, case.Nk, case.scale
    BH = B * H
    rnd = _bf16 if bf16_points else (lambda t: t)
    q, k, v, do = (_heads(inp[n].to(wd), H) for n in ('q', 'k', 'v', 'dout'))
    s = (q @ k.transpose(1, 2)) * scale
    if inp['key_bias'] is not None:
        kb = inp['key_bias'].to(wd).repeat_interleave(H, 0)[:, None, :]
        if fault == 'bias_ignored_in_partial_chunk':
            kb = kb.clone()
            kb[:, :, (Nk // 64) * 64:] = 0
        s = s + kb
    if case.rel is not None:
        sh, sw = case.rel
        rh, rw = inp['rel_h'].to(wd), inp['rel_w'].to(wd)
        if bf16_points and case.rel_mode == 1:
            rh, rw = rnd(rh / scale) * scale, rnd(rw / scale) * scale
        if fault == 'rel_w_indexed_by_kh':
            kh = torch.arange(Nk) // sw
            s = s + (rh[:, :, :, None].expand(BH, Nq, sh, sw).reshape(BH, Nq, Nk) + rw[:, :, kh.clamp(max=sw - 1)])
        else:
            s = (s.view(BH, Nq, sh, sw) + rh[:, :, :, None] + rw[:, :, None, :]).view(BH, Nq, Nk)
    if fault == 'skip_last_key_in_one_row':
        s = s.clone()
        s[BH - 1, Nq - 1, Nk - 1] = -math.inf
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[:, :, None])
    del s
    keep = keep_prob(case.p)
    if case.p > 0:
        bh_term = None
        if fault == 'mask_without_bh_for_one_head':
            bh_term = list(range(BH))
            bh_term[BH - 1] = 0
        M = keep_mask(seed, BH, Nq, Nk, case.p, bh_term).to(wd)
        Pd = P * M / keep
    else:
        M, Pd = None, P
    if fault == 'lse_from_dropped':
        lse = lse + torch.log(Pd.sum(-1))
    res = {'lse': lse}
    Pr = rnd(Pd)
    out = rnd(Pr @ v)
    if fault == 'stale_row_of_a_tile':
        out = out.clone()
        out[0, min(Nq - 1, 16 + 3)] = 0.0
    res['out'] = _unheads(out, B)
    bnd = None
    if bounds:
        f = 1.0 + (q.abs() @ k.abs().transpose(1, 2)).amax(-1) * scale if case.large else torch.ones(BH, Nq, dtype=wd)
        bnd = {'out': _unheads((Pd @ v.abs()) * f[:, :, None], B), 'lse': (1.0 + lse.abs()) * f}
    if not grads:
        return res, bnd
    dP = do @ v.transpose(1, 2)
    dsum = (do * (P @ v if fault == 'dsum_from_undropped_out' else out)).sum(-1)
    dPm = dP if M is None else dP * M / keep
    dS = P * (dPm - dsum[:, :, None])
    dSr = rnd(dS)
    res['dq'] = _unheads(rnd((dSr @ k) * scale), B)
    dS_k, Pd_v = dSr, Pr
    if fault == 'mask_seed_plus_1_in_dkv':
        M2 = keep_mask((seed + 1) & 0xffffffff, BH, Nq, Nk, case.p).to(wd)
        dS_k, Pd_v = P * (dP * M2 / keep - dsum[:, :, None]), P * M2 / keep
    if fault == 'dk_without_keep_scale':
        dS_k = P * (dP * M - dsum[:, :, None])
    res['dk'] = _unheads(rnd((dS_k.transpose(1, 2) @ q) * (1.0 if fault == 'dk_without_scale' else scale)), B)
    res['dv'] = _unheads(rnd(Pd_v.transpose(1, 2) @ do), B)
    if case.rel is not None:
        g = (dSr if case.rel_mode == 1 else dS).view(BH, Nq, sh, sw)
        res['d_rel_h'], res['d_rel_w'] = g.sum(-1), g.sum(-2)
    if bounds:
        bnd['dv'] = _unheads((Pd * f[:, :, None]).transpose(1, 2) @ do.abs(), B)
        aP = do.abs() @ v.abs().transpose(1, 2)             # the magnitude sum of dP's own expression
        for tag, mag in (('', dP.abs()), ('@mag', aP)):
            mS = P * ((mag if M is None else mag * M / keep) + (Pd * mag).sum(-1, keepdim=True)) * f[:, :, None]
            bnd['dq' + tag] = _unheads((mS @ k.abs()) * scale, B)
            bnd['dk' + tag] = _unheads((mS.transpose(1, 2) @ q.abs()) * scale, B)
            if case.rel is not None:
                g = mS.view(BH, Nq, sh, sw)
                bnd['d_rel_h' + tag], bnd['d_rel_w' + tag] = g.sum(-1), g.sum(-2)
    return res, bnd


def reference(case, inp_rounded, seed=0, grads=True, fault=None):
    """float64 results and bounds (fault: a planted one -- the host test's candidates)"""
    return attention_math(case, inp_rounded, seed, torch.float64, False, fault, grads, bounds=True)


def emulate(case, inp_rounded, dtype, seed=0, grads=True):
    """the working-precision implementation the constants are measured with"""
    res, _ = attention_math(case, inp_rounded, seed, torch.float32, dtype == torch.bfloat16, None, grads)
    return res


# ------------------------------------------------------------------------------------------------ the judge
def ratios(got, ref, bnd, dtype):
    """-> {quantity: worst |got - ref| / (u * bound)} over every element; inf for a NaN, or for a nonzero where the bound is 0"""
    u, out = U[dtype], {}
    for name, b in bnd.items():
        base = name.split('@')[0]
        if base not in got or base not in ref:
            continue
        r = ref[base]
        g = got[base].double().cpu().reshape(r.shape)
        b = b * u
        err = (g - r).abs()
        ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
        ratio = torch.where(torch.isnan(g), torch.full_like(ratio, math.inf), ratio)
        out[name] = float(ratio.max())
    return out


def misses(rat, dtype):
    """the quantities whose worst ratio exceeds MARGIN * CONSTANTS"""
    return {n: (r, MARGIN * CONSTANTS[dtype][n]) for n, r in rat.items() if not r <= MARGIN * CONSTANTS[dtype][n]}


# ------------------------------------------------------------------------------------------------ device side (needs a GPU)
SENTINEL = -12288.0             # exact in bf16; never a result of these inputs
GUARD = 1024                    # elements in front of and behind every output buffer


class Guarded:
    """An output view of `shape` / `strides` pre-filled with NaN inside an allocation filled with SENTINEL: GUARD elements before
    and after, and whatever lies between the view's rows.  check() -> list of complaints after the launch."""

    def __init__(self, shape, strides, dtype, device):
        span = 1 + sum((n - 1) * s for n, s in zip(shape, strides))
        self.flat = torch.full((2 * GUARD + span,), SENTINEL, dtype=dtype, device=device)
        self.view = self.flat.as_strided(tuple(shape), tuple(strides), GUARD)
        self.view.fill_(math.nan)
        self.inside = torch.isnan(self.flat)

    def check(self, name):
        bad = []
        if bool(torch.isnan(self.flat[self.inside]).any()):
            bad.append(f'{name}: {int(torch.isnan(self.flat[self.inside]).sum())} elements were never written (still NaN)')
        outside = self.flat[~self.inside]
        if not bool((outside == SENTINEL).all()):
            bad.append(f'{name}: {int((outside != SENTINEL).sum())} sentinel elements outside the view were overwritten')
        return bad


def _group_layout(layout):
    return {'packed': (('q', 'k', 'v'),), 'qk_v': (('q', 'k'), ('v',)), 'packed_qk_fn': (('q', 'k'), ('v',))}.get(layout, (('q',), ('k',), ('v',)))


def _strides(layout, B, N, W):
    if layout == 'wide':
        return ((N * (W + 16), W + 16, 1))
    if layout == 'seqfirst':            # a [N, B, W] tensor viewed as [B, N, W]: the batch stride is smaller than the row stride
        return (W, B * W, 1)
    return (N * W, W, 1)


def device_operands(case, inp, dtype, device='cuda'):
    """-> (inputs {q, k, v} as device views in the case's layout, gradient outputs {dq, dk, dv} as views of Guarded buffers with
    the same strides, [Guarded buffers with names])"""
    B, C = case.B, case.H * case.D
    ins, outs, guards = {}, {}, []
    for group in _group_layout(case.layout):
        N = case.Nq if group[0] == 'q' else case.Nk
        assert all((case.Nq if n == 'q' else case.Nk) == N for n in group), 'a packed layout needs Nq == Nk'
        W = C * len(group)
        st = _strides(case.layout, B, N, W)
        span = 1 + (B - 1) * st[0] + (N - 1) * st[1] + (W - 1)
        base = torch.zeros(span, dtype=dtype, device=device).as_strided((B, N, W), st)
        gd = Guarded((B, N, W), st, dtype, device)
        guards.append(('d' + '|'.join(group), gd))
        for i, n in enumerate(group):
            base[:, :, i * C:(i + 1) * C] = inp[n].to(dtype).to(device)
            ins[n] = base[:, :, i * C:(i + 1) * C]
            outs['d' + n] = gd.view[:, :, i * C:(i + 1) * C]
    return ins, outs, guards


def _dev_f32(t, device):
    return None if t is None else t.float().contiguous().to(device)


def run_stream(case, inp, dtype, grads=True, device='cuda'):
    """Launch the streaming forward (and backward) of `case` through the C-ABI with guarded, NaN-pre-filled outputs.
    -> (results as CPU tensors, complaints about guards, the effective dropout seed of the launch)"""
    from simpleaicv_pytorch_training_examples_amd import ops_tfm
    from simpleaicv_pytorch_training_examples_amd._lib import check, dtype_code, lib, ptr, stream
    B, H, Nq, C = case.B, case.H, case.Nq, case.H * case.D
    ins, gouts, guards = device_operands(case, inp, dtype, device)
    kb, rh, rw = (_dev_f32(inp[n], device) for n in ('key_bias', 'rel_h', 'rel_w'))
    ost = _strides('wide' if case.layout == 'wide' else 'sep', B, Nq, C)
    g_out = Guarded((B, Nq, C), ost, dtype, device)
    g_lse = Guarded((B * H, Nq), (Nq, 1), torch.float32, device)
    guards += [('out', g_out), ('lse', g_lse)]
    # the step word is process-global and other tests advance it: read at the time of the launch
    seed = effective_seed(case.seed, int(ops_tfm.dropout_step_word(ins['q'].device).item())) if case.p > 0 else 0
    d, hd = ops_tfm._attn_desc(ins['q'], ins['k'], ins['v'], H, case.scale, kb, rh, rw, case.p, case.seed)
    d.out, d.o_bs, d.o_rs, d.lse = ptr(g_out.view), ost[0], ost[1], ptr(g_lse.view)
    check(lib().saicv_attention_stream_fwd(dtype_code(dtype), hd, d, stream()), 'attention_stream_fwd')
    torch.cuda.synchronize()
    got = {'out': g_out.view.double().cpu(), 'lse': g_lse.view.double().cpu()}
    if grads:
        span = 1 + (B - 1) * ost[0] + (Nq - 1) * ost[1] + (C - 1)
        dout = torch.zeros(span, dtype=dtype, device=device).as_strided((B, Nq, C), ost)
        dout.copy_(inp['dout'].to(dtype).to(device))
        dsum = torch.empty((B * H, Nq), dtype=torch.float32, device=device)
        d.dout, d.dq, d.dk, d.dv, d.dsum = ptr(dout), ptr(gouts['dq']), ptr(gouts['dk']), ptr(gouts['dv']), ptr(dsum)
        if rh is not None:
            g_rh = Guarded(tuple(rh.shape), (rh.shape[1] * rh.shape[2], rh.shape[2], 1), torch.float32, device)
            g_rw = Guarded(tuple(rw.shape), (rw.shape[1] * rw.shape[2], rw.shape[2], 1), torch.float32, device)
            guards += [('d_rel_h', g_rh), ('d_rel_w', g_rw)]
            d.d_rel_h, d.d_rel_w = ptr(g_rh.view), ptr(g_rw.view)
            got_rel = (g_rh, g_rw)
        check(lib().saicv_attention_stream_bwd(dtype_code(dtype), hd, d, stream()), 'attention_stream_bwd')
        torch.cuda.synchronize()
        for n in ('dq', 'dk', 'dv'):
            got[n] = gouts[n].double().cpu()
        if rh is not None:
            got['d_rel_h'], got['d_rel_w'] = got_rel[0].view.double().cpu(), got_rel[1].view.double().cpu()
    else:
        guards = [g for g in guards if g[0] in ('out', 'lse')]
    bad = [msg for name, g in guards for msg in g.check(name)]
    return got, bad, seed


def run_whole_head(case, inp, dtype, grads=True, device='cuda'):
    """saicv_attention_fwd / saicv_attention_bwd called directly on a packed qkv [B*N, 3C] -> (results, complaints)"""
    from simpleaicv_pytorch_training_examples_amd._lib import check, dtype_code, lib, ptr, stream
    B, H, N, D = case.B, case.H, case.Nq, case.D
    C = H * D
    qkv = torch.cat([inp['q'], inp['k'], inp['v']], -1).to(dtype).to(device).reshape(B * N, 3 * C).contiguous()
    g_out = Guarded((B * N, C), (C, 1), dtype, device)
    g_lse = Guarded((B * H, N), (N, 1), torch.float32, device)
    check(lib().saicv_attention_fwd(dtype_code(dtype), ptr(qkv), ptr(g_out.view), ptr(g_lse.view), B, N, H, D, float(case.scale), stream()),
          'attention_fwd')
    torch.cuda.synchronize()
    got = {'out': g_out.view.double().cpu().view(B, N, C), 'lse': g_lse.view.double().cpu()}
    guards = [('out', g_out), ('lse', g_lse)]
    if grads:
        dout = inp['dout'].to(dtype).to(device).reshape(B * N, C).contiguous()
        g_d = Guarded((B * N, 3 * C), (3 * C, 1), dtype, device)
        guards.append(('dqkv', g_d))
        check(lib().saicv_attention_bwd(dtype_code(dtype), ptr(qkv), ptr(g_out.view), ptr(dout), ptr(g_lse.view), ptr(g_d.view), B, N, H, D,
                                        float(case.scale), stream()), 'attention_bwd')
        torch.cuda.synchronize()
        dqkv = g_d.view.double().cpu().view(B, N, 3 * C)
        got['dq'], got['dk'], got['dv'] = dqkv[:, :, :C], dqkv[:, :, C:2 * C], dqkv[:, :, 2 * C:]
    bad = [msg for name, g in guards for msg in g.check(name)]
    return got, bad
