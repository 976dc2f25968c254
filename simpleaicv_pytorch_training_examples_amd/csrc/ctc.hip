// Text recognition (reference 09.ocr_text_recognition_training): the CTC loss of SimpleAICV/text_recognition/losses.py (CTCLoss :21-46
// = preds.float(), F.log_softmax(dim=2), torch.nn.CTCLoss(reduction='none', zero_infinity=True), optional focal weight, / target
// length / batch, sum) and the greedy decode of its validation loop, straight from the [T, B, C] logits in their own dtype.
//
// logits: T x B rows of C classes (bf16 or fp32), unit stride over the classes, ANY stride over t and b (the model emits [B, T, C];
// the permuted view is used as it is).  targets int32 [B, S], input / target lengths int32 [B], all in device memory: no host sync.
//
//   row pass     one wavefront per (t, b) row with t < input_length[b]: ONE read of the row -> its maximum M, the arg-max, and
//                Sm1 = the sum of exp(x - M) over all OTHER elements (running per lane, then across the lanes), so that the
//                log-sum-exp is M + log1p(Sm1) with both parts kept apart; and the log-probabilities (x - M) - log1p(Sm1) of the
//                blank and of the sample's labels into the compact lp [T, B, 1 + S] (slot 0 the blank, slot 1 + i label i).
//   alpha-beta   one workgroup per sample, threads over the 2 L + 1 extended states, time sequential, log space, fp32; the emission
//                is in alpha AND in beta (torch's formulation).  alpha goes to a global table [B, T, 2 S + 1] (T is not bounded), the
//                running rows live in LDS.  -> nll[b]; the occupancy occ[t, b, slot] = log sum_{s: l'_s = class of slot}
//                alpha_t(s) beta_t(s) for every DISTINCT class of the sample: slot 0 sums the L + 1 blank states, the slot of a
//                label's FIRST occurrence sums its repeats in index order (maximum, then the sum in that order), later
//                occurrences have slot class -1.  term[b] = w_b nll_b / L_b / B with w_b = (1 - exp(-nll_b))^gamma (focal) or 1.
//   fold         loss = sum_b term[b], the ordered sum of ordered_sum.h.
//   gradient     one wavefront per row re-reads the logits and writes  g_b (softmax_c P - post_c)  for all C classes in the
//                logits' dtype, EVERY element exactly once: post_c = exp(occ_c + nll_b - lp_c), P = sum_c post_c (= 1 up to
//                rounding: what log_softmax's backward multiplies in); a per-wave LDS bitmap says which classes the sample
//                holds, and only a hit looks its slot up.  At the row's arg-max the difference is formed from 1 - softmax and
//                P - post (see `hit`).  g_b = dL/dloss (read on the device) / L_b / B * ((1 - p)^gamma + gamma nll p
//                (1 - p)^(gamma - 1)).  Rows with t >= input_length[b] and all rows of a dropped sample are zeros.
//
// zero_infinity: a sample is dropped (nll 0, term 0, zero gradient) when L + repeats > input_length, when input_length is 0, when
// its nll is not finite, or when a label is outside [0, C) or equals the blank (torch rejects those).  Entries of targets at or
// beyond target_length are never read.  L = 0 divides by max(L, 1).  Focal gamma is at least 1.
// Non-finite logits: a NaN anywhere in a frame the sample uses makes that row's sum, hence the sample's nll, NaN, and the sample
// is dropped (torch's loss would be NaN there: zero_infinity only clears +inf); the same for a frame that is all -inf.  A -inf
// logit is an impossible class: it adds nothing to the sum, gets gradient 0, and a path through it has probability 0.  The greedy
// decode takes the arg-max over the entries that are not NaN and gives probability NaN for a row with a NaN or with nothing
// above -inf (index -1 for the latter).
//
// Bits: a row's element c belongs to chunk c / EPC, chunk k to lane k % 64, and a lane adds its chunks in index order, wherever the
// row starts (16-byte accesses at element alignment).  So a result depends on the values alone, not on where the row lies or on
// the batch around it.
#include "common.h"
#include "ordered_sum.h"
#include "saicv_internal.h"
#include "../../include/saicv_hip.h"

namespace {

constexpr int CTC_MAX_S = 1819;             // (3 (2 S + 1) + 3 S + 4) * 4 bytes of LDS in the alpha-beta kernel: within 64 KB
constexpr int CTC_MAX_C = 1 << 20;          // 4 bitmaps of C bits + 4 slot lists in LDS in the gradient kernel (checked against 64 KB)
constexpr float NEG_INF = -INFINITY;

extern __shared__ __attribute__((aligned(16))) unsigned char ctc_smem[];

DEVINL int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// 16 bytes at an address aligned to sizeof(T) only: rows of 12 113 classes start anywhere.  (One global_load / store_dwordx4 each:
// gfx950 takes unaligned vector accesses to global memory.)
template <typename T>
DEVINL u32x4 ctc_ld(const T* p) {
    u32x4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}
template <typename T>
DEVINL void ctc_st(T* p, u32x4 v) { __builtin_memcpy(p, &v, 16); }

// One more value for a lane: its running maximum m, the index am of the FIRST element that holds it, and s = the sum of
// exp(x - m) over every OTHER element the lane has seen.  The maximum's own term (exactly 1) is left out so that a confident row
// (sum = 1 + 1e-4) keeps the 1e-4 at full precision: log1p(s) for the log-sum-exp, s / (1 + s) for 1 - softmax at the maximum.
DEVINL void ctc_acc(float& m, float& s, int& am, float x, int idx) {
    if (x != x) {                           // NaN: s stays NaN whatever follows, and so does the row's sum
        s = x;
        return;
    }
    if (x == NEG_INF) return;               // -inf adds nothing
    const float e = expf(-fabsf(x - m));    // m = -inf (nothing seen yet): 0
    if (x > m) {                            // the old maximum becomes an ordinary element; indices only grow: ">" keeps the first
        s = (s + 1.f) * e;
        m = x;
        am = idx;
    } else {
        s += e;
    }
}

// one wavefront over one row -> the same in every lane: the maximum M, the index of its first occurrence, and
// Sm1 = sum over all other elements of exp(x_c - M)  (softmax_c = exp(x_c - M) / (1 + Sm1))
template <typename T>
DEVINL void ctc_row_stats(const T* row, int C, int lane, float& M, float& Sm1, int& arg) {
    constexpr int EPC = ElemTraits<T>::EPC;
    const int nfull = C / EPC;
    float m = NEG_INF, s = 0.f;
    int am = 0x7fffffff;
    for (int k0 = 0; k0 < nfull; k0 += 256) {
        u32x4 ch[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + 64 * u + lane;
            if (k < nfull) ch[u] = ctc_ld<T>(row + (size_t)k * EPC);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + 64 * u + lane;
            if (k < nfull) {
                float f[EPC];
                Chunk<T>::unpack(ch[u], f);
#pragma unroll
                for (int i = 0; i < EPC; ++i) ctc_acc(m, s, am, f[i], k * EPC + i);
            }
        }
    }
    const int c = nfull * EPC + lane;       // the tail: fewer than EPC <= 8 elements, one per lane
    if (c < C) ctc_acc(m, s, am, to_f32(row[c]), c);
    M = wave_max(m);
    int cand = m == M ? am : 0x7fffffff;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
    arg = cand == 0x7fffffff ? -1 : cand;   // -1: no element above -inf
    // the lane that holds the row's first maximum keeps it left out; every other lane's own maximum is an ordinary element now
    // (a lane that saw nothing above -inf adds 0, unless it saw a NaN: then s is NaN and stays so)
    const bool owner = m == M && am == cand;
    Sm1 = wave_sum((m == NEG_INF && s == s) ? 0.f : (owner ? s : (s + 1.f) * expf(m - M)));
}

// ------------------------------------------------------------------------------------------------ row pass
// lse [T B 4]: M, ls = log(1 + Sm1), Sm1, the arg-max index (as bits)
template <typename T>
__global__ __launch_bounds__(256) void ctc_row_kernel(const T* __restrict__ logits, long long st, long long sb,
                                                      const int* __restrict__ targets, const int* __restrict__ in_len,
                                                      const int* __restrict__ tg_len, int Tn, int B, int S, int C, int blank,
                                                      float* __restrict__ lse, float* __restrict__ lp) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (long long)Tn * B) return;     // wave-uniform; no barrier below
    const int t = (int)(r / B), b = (int)(r % B);
    if (t >= clampi(in_len[b], 0, Tn)) return;
    const T* row = logits + t * st + b * sb;
    float M, Sm1;
    int arg;
    ctc_row_stats<T>(row, C, lane, M, Sm1, arg);
    const float ls = log1pf(Sm1);           // kept apart from M: lp = (x - M) - ls rounds at the size of x - M, not of the logits
    if (lane == 0) {
        lse[4 * r] = M;
        lse[4 * r + 1] = ls;
        lse[4 * r + 2] = Sm1;
        lse[4 * r + 3] = __int_as_float(arg);
    }
    const int L = clampi(tg_len[b], 0, S);
    float* out = lp + (size_t)r * (1 + S);
    for (int j = lane; j <= L; j += 64) {
        const int c = j == 0 ? blank : targets[(size_t)b * S + j - 1];
        out[j] = (c >= 0 && c < C) ? (to_f32(row[c]) - M) - ls : NEG_INF;
    }
}

// ------------------------------------------------------------------------------------------------ alpha-beta
DEVINL float ctc_lse3(float a, float b, float c) {
    float m = fmaxf(fmaxf(a, b), c);
    if (m == NEG_INF) m = 0.f;
    return logf(expf(a - m) + expf(b - m) + expf(c - m)) + m;
}

__global__ __launch_bounds__(256) void ctc_ab_kernel(const float* __restrict__ lp, const int* __restrict__ targets,
                                                     const int* __restrict__ in_len, const int* __restrict__ tg_len, int Tn, int B,
                                                     int S, int C, int blank, int focal, float gamma, float* __restrict__ alpha,
                                                     float* __restrict__ occ, int* __restrict__ slotcls, float* __restrict__ nll,
                                                     float* __restrict__ feas, float* __restrict__ term) {
    const int NSM = 2 * S + 1, W = 1 + S;
    float* row0 = reinterpret_cast<float*>(ctc_smem);
    float* row1 = row0 + NSM;
    float* ab = row1 + NSM;
    int* cls = reinterpret_cast<int*>(ab + NSM);
    int* nxt = cls + S;
    int* fst = nxt + S;
    int* flag = fst + S;                    // [0] bad label, [1] repeats; [2] the nll's bits
    const int tid = threadIdx.x, b = blockIdx.x;
    const int Tin = clampi(in_len[b], 0, Tn), L = clampi(tg_len[b], 0, S);
    const int NS = 2 * L + 1;
    if (tid < 3) flag[tid] = 0;
    __syncthreads();
    for (int i = tid; i < L; i += 256) {
        const int c = targets[(size_t)b * S + i];
        cls[i] = c;
        if (c < 0 || c >= C || c == blank) atomicOr(&flag[0], 1);
    }
    __syncthreads();
    for (int i = tid; i < L; i += 256) {
        const int c = cls[i];
        if (i > 0 && cls[i - 1] == c) atomicAdd(&flag[1], 1);
        int n = -1, f = 1;
        for (int j = i + 1; j < L; ++j)
            if (cls[j] == c) { n = j; break; }
        for (int j = 0; j < i; ++j)
            if (cls[j] == c) { f = 0; break; }
        nxt[i] = n;
        fst[i] = f;
    }
    __syncthreads();
    // what the gradient pass looks classes up in: slot 0 the blank, slot 1 + i label i at its first occurrence
    for (int j = tid; j < W; j += 256) slotcls[(size_t)b * W + j] = j == 0 ? blank : ((j - 1 < L && fst[j - 1]) ? cls[j - 1] : -1);
    const bool ok = flag[0] == 0 && Tin > 0 && L + flag[1] <= Tin;          // block-uniform
    if (!ok) {
        if (tid == 0) { nll[b] = 0.f; feas[b] = 0.f; term[b] = 0.f; }
        return;
    }
    const float* lpb = lp + (size_t)b * W;                                  // row t at lpb + t * B * W
    const size_t lpt = (size_t)B * W;
    float* al = alpha + (size_t)b * Tn * NSM;
    // alpha
    for (int s = tid; s < NS; s += 256) {
        const float v = s < 2 ? lpb[s] : NEG_INF;                           // state 1 is label 0 = slot 1
        row0[s] = v;
        al[s] = v;
    }
    __syncthreads();
    for (int t = 1; t < Tin; ++t) {
        const float* prev = (t & 1) ? row0 : row1;
        float* cur = (t & 1) ? row1 : row0;
        const float* e = lpb + t * lpt;
        for (int s = tid; s < NS; s += 256) {
            const int i = s >> 1;
            const float a1 = prev[s], a2 = s > 0 ? prev[s - 1] : NEG_INF;
            const float a3 = (s > 1 && (s & 1) && cls[i] != cls[i - 1]) ? prev[s - 2] : NEG_INF;
            const float v = ctc_lse3(a1, a2, a3) + e[(s & 1) ? 1 + i : 0];
            cur[s] = v;
            al[(size_t)t * NSM + s] = v;
        }
        __syncthreads();
    }
    if (tid == 0) {
        const float* last = ((Tin - 1) & 1) ? row1 : row0;
        const float v = -ctc_lse3(last[NS - 1], NS > 1 ? last[NS - 2] : NEG_INF, NEG_INF);
        flag[2] = __float_as_int(v);
    }
    __syncthreads();
    const float nl = __int_as_float(flag[2]);
    if (!(fabsf(nl) < INFINITY)) {                                          // inf or nan: zero_infinity
        if (tid == 0) { nll[b] = 0.f; feas[b] = 0.f; term[b] = 0.f; }
        return;
    }
    if (tid == 0) {
        float w = 1.f;
        if (focal) w = powf(1.f - expf(-nl), gamma);
        nll[b] = nl;
        feas[b] = 1.f;
        term[b] = ((w * nl) / (float)(L > 0 ? L : 1)) / (float)B;
    }
    // beta (the alpha rows are in global memory now; row0 / row1 hold beta), newest frame first
    for (int t = Tin - 1; t >= 0; --t) {
        const float* prev = (t & 1) ? row0 : row1;
        float* cur = (t & 1) ? row1 : row0;
        const float* e = lpb + t * lpt;
        for (int s = tid; s < NS; s += 256) {
            const int i = s >> 1;
            float v;
            if (t == Tin - 1) {
                v = s >= NS - 2 ? e[(s & 1) ? 1 + i : 0] : NEG_INF;
            } else {
                const float b1 = prev[s], b2 = s + 1 < NS ? prev[s + 1] : NEG_INF;
                const float b3 = (s + 2 < NS && (s & 1) && cls[i] != cls[i + 1]) ? prev[s + 2] : NEG_INF;
                v = ctc_lse3(b1, b2, b3) + e[(s & 1) ? 1 + i : 0];
            }
            cur[s] = v;
            ab[s] = al[(size_t)t * NSM + s] + v;
        }
        __syncthreads();
        float* o = occ + ((size_t)t * B + b) * W;
        for (int i = tid; i < L; i += 256) {
            if (!fst[i]) continue;
            float m = ab[2 * i + 1];
            if (nxt[i] >= 0) {                                              // a repeated character: its occurrences in index order
                for (int j = nxt[i]; j >= 0; j = nxt[j]) m = fmaxf(m, ab[2 * j + 1]);
                if (m > NEG_INF) {
                    float sum = 0.f;
                    for (int j = i; j >= 0; j = nxt[j]) sum += expf(ab[2 * j + 1] - m);
                    m += logf(sum);
                }
            }
            o[1 + i] = m;
        }
        if (tid >= 192) {                                                   // the last wavefront: the L + 1 blank states
            const int lane = tid - 192;
            float m = NEG_INF;
            for (int k = lane; k <= L; k += 64) m = fmaxf(m, ab[2 * k]);
            m = wave_max(m);
            float sum = 0.f;
            if (m > NEG_INF)
                for (int k = lane; k <= L; k += 64) sum += expf(ab[2 * k] - m);
            sum = wave_sum(sum);
            if (lane == 0) o[0] = m > NEG_INF ? m + logf(sum) : NEG_INF;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void ctc_fold_kernel(const float* __restrict__ term, int B, float* __restrict__ loss) {
    const float total = fold_rows<1>(term, B, 1);
    if (threadIdx.x == 0) loss[0] = total;
}

// ------------------------------------------------------------------------------------------------ gradient
template <typename T>
__global__ __launch_bounds__(256) void ctc_grad_kernel(const T* __restrict__ logits, long long st, long long sb, T* __restrict__ dlog,
                                                       long long dst, long long dsb, const float* __restrict__ lse,
                                                       const float* __restrict__ lp, const float* __restrict__ occ,
                                                       const int* __restrict__ slotcls, const float* __restrict__ nll,
                                                       const float* __restrict__ feas, const int* __restrict__ in_len,
                                                       const int* __restrict__ tg_len, const float* __restrict__ gout, int Tn, int B,
                                                       int S, int C, int focal, float gamma) {
    constexpr int EPC = ElemTraits<T>::EPC;
    const int W = 1 + S, BW = (C + 31) >> 5;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t* bm = reinterpret_cast<uint32_t*>(ctc_smem) + (size_t)wave * (BW + 2 * W);
    int* wcls = reinterpret_cast<int*>(bm + BW);
    float* wd = reinterpret_cast<float*>(wcls + W);
    const long long r = (long long)blockIdx.x * 4 + wave;
    const bool active = r < (long long)Tn * B;
    const int t = active ? (int)(r / B) : 0, b = active ? (int)(r % B) : 0;
    const int L = clampi(tg_len[b], 0, S);
    const bool live = active && t < clampi(in_len[b], 0, Tn) && feas[b] != 0.f;           // wave-uniform
    if (live)
        for (int k = lane; k < BW; k += 64) bm[k] = 0u;
    __syncthreads();
    float g = 0.f, M = 0.f, ls = 0.f, Sm1 = 0.f, P = 1.f;
    int arg = -1;
    if (live) {
        const float nl = nll[b];
        g = gout[0] / (float)(L > 0 ? L : 1) / (float)B;
        if (focal) {
            const float p = expf(-nl), q = 1.f - p;
            g *= powf(q, gamma) + gamma * nl * p * powf(q, gamma - 1.f);
        }
        M = lse[4 * r];
        ls = lse[4 * r + 1];
        Sm1 = lse[4 * r + 2];
        arg = __float_as_int(lse[4 * r + 3]);
        float psum = 0.f;
        for (int j = lane; j <= L; j += 64) {
            const int c = slotcls[(size_t)b * W + j];
            wcls[j] = c;
            if (c >= 0) {
                const float lpv = lp[(size_t)r * W + j];                     // -inf logit at a class of the sample: no state holds it
                const float d = lpv > NEG_INF ? expf(occ[(size_t)r * W + j] + nl - lpv) : 0.f;
                wd[j] = d;
                psum += d;
                atomicOr(&bm[c >> 5], 1u << (c & 31));
            }
        }
        // the row's posteriors sum to 1 up to the rounding of occ + nll - lp, values as large as nll whose error is common to the
        // whole row.  softmax_c * P - post_c is what log_softmax's backward makes of torch's CTC gradient (g_lp - softmax * sum g_lp
        // with sum softmax = 1): the common error then scales the gradient instead of adding post_c times it.
        P = wave_sum(psum);
    }
    __syncthreads();
    if (!active) return;
    const T* row = logits + t * st + b * sb;
    T* drow = dlog + t * dst + b * dsb;
    const int nfull = C / EPC;
    // class c is one of the sample's: f = softmax_c P -> softmax_c P - post_c.  At the row's arg-max both may be 1 - 1e-4 and
    // their difference all rounding; there softmax = 1 - u with u = Sm1 / (1 + Sm1) and post_c = P - (the other slots' sum), so
    // the difference is (the other slots' sum) - u P, two small numbers known to full precision.
    auto hit = [&](int c, float f) -> float {
        for (int j = 0; j <= L; ++j) {
            if (wcls[j] != c) continue;
            if (c != arg) return f - wd[j];
            float rest = 0.f;
            for (int q = 0; q <= L; ++q)
                if (q != j && wcls[q] >= 0) rest += wd[q];
            return rest - (Sm1 / (1.f + Sm1)) * P;
        }
        return f;
    };
    if (!live) {
        for (int k = lane; k < nfull; k += 64) ctc_st<T>(drow + (size_t)k * EPC, zero_chunk());
        const int c = nfull * EPC + lane;
        if (c < C) drow[c] = from_f32<T>(0.f);
        return;
    }
    for (int k0 = 0; k0 < nfull; k0 += 256) {
        u32x4 ch[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + 64 * u + lane;
            if (k < nfull) ch[u] = ctc_ld<T>(row + (size_t)k * EPC);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + 64 * u + lane;
            if (k < nfull) {
                float f[EPC];
                Chunk<T>::unpack(ch[u], f);
                const int c0 = k * EPC;                                      // EPC divides 32: a chunk lies inside one bitmap word
                const uint32_t bits = (bm[c0 >> 5] >> (c0 & 31)) & ((1u << EPC) - 1u);
#pragma unroll
                for (int i = 0; i < EPC; ++i) f[i] = expf((f[i] - M) - ls) * P;
                if (bits) {
#pragma unroll
                    for (int i = 0; i < EPC; ++i) {
                        if ((bits >> i) & 1u) f[i] = hit(c0 + i, f[i]);
                    }
                }
#pragma unroll
                for (int i = 0; i < EPC; ++i) f[i] *= g;
                ctc_st<T>(drow + (size_t)k * EPC, Chunk<T>::pack(f));
            }
        }
    }
    const int c = nfull * EPC + lane;
    if (c < C) {
        float f = expf((to_f32(row[c]) - M) - ls) * P;
        if ((bm[c >> 5] >> (c & 31)) & 1u) f = hit(c, f);
        drow[c] = from_f32<T>(f * g);
    }
}

// ------------------------------------------------------------------------------------------------ greedy decode
template <typename T>
__global__ __launch_bounds__(256) void ctc_greedy_kernel(const T* __restrict__ logits, long long st, long long sb,
                                                         const int* __restrict__ in_len, int Tn, int B, int C, int* __restrict__ index,
                                                         float* __restrict__ prob) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (long long)Tn * B) return;
    const int t = (int)(r / B), b = (int)(r % B);
    if (in_len != nullptr && t >= clampi(in_len[b], 0, Tn)) {
        if (lane == 0) { index[r] = -1; prob[r] = 0.f; }
        return;
    }
    float M, Sm1;
    int arg;
    ctc_row_stats<T>(logits + t * st + b * sb, C, lane, M, Sm1, arg);
    if (lane == 0) {
        index[r] = arg;
        prob[r] = arg >= 0 ? 1.f / (1.f + Sm1) : NAN;                         // (a row of -inf has no softmax)
    }
}

int ctc_check(const char* what, const void* logits, int Tn, int B, int C, long long st, long long sb) {
    SAICV_REQUIRE(logits != nullptr, "%s: null logits", what);
    SAICV_REQUIRE(Tn > 0 && B > 0 && C >= 2 && C <= CTC_MAX_C, "%s: T %d, B %d, C %d; need T, B >= 1 and 2 <= C <= %d", what, Tn, B, C,
                  CTC_MAX_C);
    SAICV_REQUIRE((long long)Tn * B <= 0x7fffffffLL / 4, "%s: %lld rows; at most 2^29 - 1", what, (long long)Tn * B);
    SAICV_REQUIRE(st >= 0 && sb >= 0, "%s: negative strides", what);
    return 0;
}

size_t ctc_grad_smem(int S, int C) { return (size_t)4 * (((C + 31) >> 5) + 2 * (1 + S)) * 4; }
size_t ctc_ab_smem(int S) { return (size_t)(3 * (2 * S + 1) + 3 * S + 4) * 4; }

}  // namespace

namespace saicv {

// floats of workspace for ctc_loss_fwd; the pieces, in order: lse [T B 4] (row maximum, log of the rescaled sum, that sum less 1, arg-max), lp [T B W], occ [T B W], alpha [B T (2 S + 1)],
// slotcls [B W] (int32), feas [B], term [B]   (W = 1 + S)
extern "C" size_t saicv_ctc_ws_floats(int Tn, int B, int S) {
    const size_t rows = (size_t)Tn * B, W = 1 + (size_t)S;
    return 4 * rows + 2 * rows * W + rows * (2 * (size_t)S + 1) + (size_t)B * W + 2 * (size_t)B;
}

namespace {
struct CtcWs {
    float *lse, *lp, *occ, *alpha, *feas, *term;
    int* slotcls;
};
CtcWs ctc_carve(float* ws, int Tn, int B, int S) {
    const size_t rows = (size_t)Tn * B, W = 1 + (size_t)S;
    CtcWs w;
    w.lse = ws;
    w.lp = w.lse + 4 * rows;
    w.occ = w.lp + rows * W;
    w.alpha = w.occ + rows * W;
    w.slotcls = reinterpret_cast<int*>(w.alpha + rows * (2 * (size_t)S + 1));
    w.feas = reinterpret_cast<float*>(w.slotcls) + (size_t)B * W;
    w.term = w.feas + B;
    return w;
}
}  // namespace

extern "C" int saicv_ctc_loss_fwd(int dtype, const void* logits, long long st, long long sb, const int* targets, const int* in_len, const int* tg_len,
                                  int Tn, int B, int S, int C, int blank, int focal, float gamma, float* ws, float* nll, float* loss, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (ctc_check("ctc_loss_fwd", logits, Tn, B, C, st, sb)) return -1;
    SAICV_REQUIRE(targets && in_len && tg_len && ws && nll && loss, "ctc_loss_fwd: null targets, lengths, workspace or output");
    SAICV_REQUIRE(S >= 1 && S <= CTC_MAX_S, "ctc_loss_fwd: targets are [B, %d]; 1 .. %d columns", S, CTC_MAX_S);
    SAICV_REQUIRE(blank >= 0 && blank < C, "ctc_loss_fwd: blank %d outside [0, %d)", blank, C);
    SAICV_REQUIRE(ctc_ab_smem(S) <= 64 * 1024, "ctc_loss_fwd: %d target columns need %zu bytes of LDS; at most 65536 (%d columns)", S,
                  ctc_ab_smem(S), CTC_MAX_S);
    SAICV_REQUIRE(!focal || gamma >= 1.f, "ctc_loss_fwd: focal gamma %g; at least 1 (the derivative holds (1 - p)^(gamma - 1))",
                  (double)gamma);
    const CtcWs w = ctc_carve(ws, Tn, B, S);
    const int blocks = (int)(((long long)Tn * B + 3) / 4);
    const bool bf = dtype == SAICV_DTYPE_BF16;
#define CTC_ROW(T)                                                                                                          \
    hipLaunchKernelGGL(ctc_row_kernel<T>, dim3(blocks), dim3(256), 0, s, (const T*)logits, st, sb, targets, in_len, tg_len, Tn, B, \
                       S, C, blank, w.lse, w.lp)
    if (bf) CTC_ROW(bf16_t);
    else CTC_ROW(float);
#undef CTC_ROW
    hipLaunchKernelGGL(ctc_ab_kernel, dim3(B), dim3(256), ctc_ab_smem(S), s, w.lp, targets, in_len, tg_len, Tn, B, S, C, blank, focal,
                       gamma, w.alpha, w.occ, w.slotcls, nll, w.feas, w.term);
    hipLaunchKernelGGL(ctc_fold_kernel, dim3(1), dim3(256), 0, s, w.term, B, loss);
    return check_launch("ctc_loss_fwd");
}

extern "C" int saicv_ctc_loss_bwd(int dtype, const void* logits, long long st, long long sb, void* dlogits, long long dst, long long dsb,
                                  const int* in_len, const int* tg_len, const float* ws, const float* nll, const float* gout, int Tn, int B, int S, int C,
                                  int focal, float gamma, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (ctc_check("ctc_loss_bwd", logits, Tn, B, C, st, sb)) return -1;
    SAICV_REQUIRE(dlogits && in_len && tg_len && ws && nll && gout, "ctc_loss_bwd: null gradient, lengths, workspace or dL/dloss");
    SAICV_REQUIRE(S >= 1 && S <= CTC_MAX_S, "ctc_loss_bwd: targets are [B, %d]; 1 .. %d columns", S, CTC_MAX_S);
    SAICV_REQUIRE(dst >= 0 && dsb >= 0, "ctc_loss_bwd: negative strides");
    const size_t smem = ctc_grad_smem(S, C);
    SAICV_REQUIRE(smem <= 64 * 1024, "ctc_loss_bwd: %d classes and %d target columns need %zu bytes of LDS; at most 65536", C, S, smem);
    const CtcWs w = ctc_carve(const_cast<float*>(ws), Tn, B, S);
    const int blocks = (int)(((long long)Tn * B + 3) / 4);
    const bool bf = dtype == SAICV_DTYPE_BF16;
#define CTC_GRAD(T)                                                                                                         \
    hipLaunchKernelGGL(ctc_grad_kernel<T>, dim3(blocks), dim3(256), smem, s, (const T*)logits, st, sb, (T*)dlogits, dst, dsb, w.lse, \
                       w.lp, w.occ, w.slotcls, nll, w.feas, in_len, tg_len, gout, Tn, B, S, C, focal, gamma)
    if (bf) CTC_GRAD(bf16_t);
    else CTC_GRAD(float);
#undef CTC_GRAD
    return check_launch("ctc_loss_bwd");
}

extern "C" int saicv_ctc_greedy(int dtype, const void* logits, long long st, long long sb, const int* in_len, int Tn, int B, int C, int* index,
                                float* prob, void* stream) {
    hipStream_t s = S(stream);
    if (ctc_check("ctc_greedy", logits, Tn, B, C, st, sb)) return -1;
    SAICV_REQUIRE(index && prob, "ctc_greedy: null output");
    const int blocks = (int)(((long long)Tn * B + 3) / 4);
    const bool bf = dtype == SAICV_DTYPE_BF16;
#define CTC_GREEDY(T)                                                                                                        \
    hipLaunchKernelGGL(ctc_greedy_kernel<T>, dim3(blocks), dim3(256), 0, s, (const T*)logits, st, sb, in_len, Tn, B, C, index, prob)
    if (bf) CTC_GREEDY(bf16_t);
    else CTC_GREEDY(float);
#undef CTC_GREEDY
    return check_launch("ctc_greedy");
}

}  // namespace saicv
