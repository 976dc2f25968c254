// The pixel sums of the universal-segmentation (EoMT / Mask2Former) set loss: SimpleAICV/universal_segmentation/segmentation_losses.py.
//
// (a) pair sums for the Hungarian matcher, the whole batch in one launch pair.  Per image i, query q, target t, over the P = H*W pixels:
//       P[q,t] = sum softplus(-x_qp) y_tp      N[q,t] = sum softplus(x_qp) (1 - y_tp)      S[q,t] = sum sigmoid(x_qp) y_tp
//     and sum_p sigmoid(x_qp) per query, sum_p y_tp per target.  The three products are fp32-operand MFMAs (v_mfma_f32_16x16x4_f32:
//     exact fp32 operands, fp32 accumulate): a lane of the operand layout holds row (l & 15), k-group (l >> 4), and the k order is
//     one permutation shared by both operands, so every lane loads eight CONSECUTIVE pixels of its row straight from global memory
//     and no LDS staging is needed.  N is formed against (1 - y) itself: softplus(x) summed minus the product with y cancels
//     when a prediction is confident and right.  The transcendentals of a query tile are computed once per pixel for up to 64
//     targets.  A workgroup takes one chunk of US_CHUNK pixels, 64 queries (a wavefront per 16) and 64 targets; the chunk partials
//     are then added in chunk order by ordered_sum.h's fold_rows.  No atomics: the bits depend on (Q, T_i, P) of the image alone.
// (c) matched-pair statistics [M][4] = (sum bce(x, y), sum sigmoid(x) y, sum sigmoid(x), sum y) through row index tables (no
//     gather copy), and their backward over ALL B*Q rows: a matched row gets g0 (s - y) + s (1 - s)(g1 y + g2), every other row
//     exact zeros in the same launch.
#include "common.h"
#include "saicv_internal.h"
#include "../../include/saicv_hip.h"
#include "ordered_sum.h"

namespace {

constexpr int US_THREADS = 256;      // four wavefronts (ordered_sum.h)
constexpr int US_CHUNK = 4096;       // pixels per workgroup; a multiple of US_STEP and of 8 * US_THREADS
constexpr int US_STEP = 32;          // pixels per wavefront step: 4 k-groups x 8 consecutive pixels
constexpr int US_TT = 4;             // 16-target tiles per workgroup
constexpr int US_FOLD = 16;          // totals per stage-2 workgroup

// the stable pieces of maskterm.h's mask_term for both signs of the target at once
struct SoftTerms {
    float sp_neg, sp_pos, sig;       // softplus(-x), softplus(x), sigmoid(x)
};
DEVINL SoftTerms soft_terms(float x) {
    SoftTerms r;
    const float e = expf(-fabsf(x));
    const float l = log1pf(e);
    r.sig = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
    r.sp_pos = fmaxf(x, 0.f) + l;
    r.sp_neg = fmaxf(-x, 0.f) + l;
    return r;
}

// eight consecutive values row[p .. p + 8), those at or past `end` read as 0.  vec: every row start and p are 16-byte aligned.
template <typename T>
DEVINL void load8(const T* __restrict__ row, size_t p, size_t end, bool vec, float (&v)[8]) {
    if (vec && p + 8 <= end) {
        if constexpr (sizeof(T) == 2) {
            Chunk<bf16_t>::unpack(ld_chunk(row + p), v);
        } else {
            Chunk<float>::unpack(ld_chunk(row + p), v);
            Chunk<float>::unpack(ld_chunk(row + p + 4), v + 4);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = p + k < end ? to_f32(row[p + k]) : 0.f;
    }
}

// partial [nchunks][ld]; a row holds, in this order: 3 planes [Q][TT] (P, N, S; TT = sum T_i, column off_i + t), qsum [B][Q], tsum [TT]
template <typename T>
__global__ __launch_bounds__(US_THREADS) void pair_sums_kernel(const T* __restrict__ preds, const float* __restrict__ targets,
                                                               const int* __restrict__ offsets, float* __restrict__ partial, int B,
                                                               int Q, int TT, size_t P, size_t ld, int qblocks, bool vec) {
    const int b = blockIdx.z;
    const int qb = blockIdx.y % qblocks, tg = blockIdx.y / qblocks;
    const int off = offsets[b], Ti = offsets[b + 1] - off;
    const int tbase = tg * (US_TT * 16);
    float* prow = partial + (size_t)blockIdx.x * ld;
    const size_t ncols = (size_t)3 * Q * TT + (size_t)B * Q + TT;
    if (b == 0 && blockIdx.y == 0 && ncols + threadIdx.x < ld) prow[ncols + threadIdx.x] = 0.f;      // the padding the fold reads
    if (tg > 0 && tbase >= Ti) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q0 = (qb * 4 + wave) * 16;
    if (q0 >= Q) return;
    const int r = lane & 15, g = lane >> 4;
    const int ntt = Ti > tbase ? min(US_TT, (Ti - tbase + 15) / 16) : 0;
    const T* xrow = preds + ((size_t)b * Q + min(q0 + r, Q - 1)) * P;
    const size_t p0 = (size_t)blockIdx.x * US_CHUNK;
    const size_t end = min(P, p0 + US_CHUNK);

    f32x4 accP[US_TT], accN[US_TT], accS[US_TT];
    float ysum[US_TT];
#pragma unroll
    for (int tt = 0; tt < US_TT; ++tt) {
        accP[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
        accN[tt] = accP[tt];
        accS[tt] = accP[tt];
        ysum[tt] = 0.f;
    }
    float ssig = 0.f;
    for (size_t ps = p0; ps < end; ps += US_STEP) {
        const size_t p = ps + (size_t)g * 8;
        float x[8], a0[8], a1[8], a2[8];
        load8<T>(xrow, p, end, vec, x);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const SoftTerms s = soft_terms(x[k]);
            const bool in = p + k < end;
            a0[k] = in ? s.sp_neg : 0.f;
            a1[k] = in ? s.sp_pos : 0.f;
            a2[k] = in ? s.sig : 0.f;
            ssig += a2[k];
        }
#pragma unroll
        for (int tt = 0; tt < US_TT; ++tt) {
            if (tt < ntt) {
                const int t = tbase + tt * 16 + r;
                float y[8];
                if (t < Ti) {
                    load8<float>(targets + (size_t)(off + t) * P, p, end, vec, y);
                } else {
#pragma unroll
                    for (int k = 0; k < 8; ++k) y[k] = 0.f;
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float yn = (t < Ti && p + k < end) ? 1.f - y[k] : 0.f;
                    accP[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[k], y[k], accP[tt], 0, 0, 0);
                    accN[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[k], yn, accN[tt], 0, 0, 0);
                    accS[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[k], y[k], accS[tt], 0, 0, 0);
                    ysum[tt] += y[k];
                }
            }
        }
    }
    // C layout: column (target) = lane & 15, row (query) = (lane >> 4) * 4 + register
    const size_t plane = (size_t)Q * TT;
#pragma unroll
    for (int tt = 0; tt < US_TT; ++tt) {
        if (tt < ntt) {
            const int t = tbase + tt * 16 + r;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int q = q0 + g * 4 + i;
                if (q < Q && t < Ti) {
                    const size_t c = (size_t)q * TT + off + t;
                    prow[c] = accP[tt][i];
                    prow[plane + c] = accN[tt][i];
                    prow[2 * plane + c] = accS[tt][i];
                }
            }
        }
    }
    // the four k-groups of a row, in a fixed order
    ssig += __shfl_xor(ssig, 16, 64);
    ssig += __shfl_xor(ssig, 32, 64);
    if (tg == 0 && g == 0 && q0 + r < Q) prow[3 * plane + (size_t)b * Q + q0 + r] = ssig;
    if (qb == 0 && wave == 0) {
#pragma unroll
        for (int tt = 0; tt < US_TT; ++tt) {
            float v = ysum[tt];
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            const int t = tbase + tt * 16 + r;
            if (tt < ntt && g == 0 && t < Ti) prow[3 * plane + (size_t)B * Q + off + t] = v;
        }
    }
}

// stage 2 over partial [n][ld] -> out [ncols], US_FOLD totals per workgroup (ld is a multiple of US_FOLD)
__global__ __launch_bounds__(US_THREADS) void pair_fold_kernel(const float* __restrict__ partial, int n, size_t ld, size_t ncols,
                                                               float* __restrict__ out) {
    const size_t c0 = (size_t)blockIdx.x * US_FOLD;
    float s[US_FOLD];
#pragma unroll
    for (int j = 0; j < US_FOLD; ++j) s[j] = 0.f;
    for (int i = threadIdx.x; i < n; i += US_THREADS) {
#pragma unroll
        for (int j = 0; j < US_FOLD; ++j) s[j] += partial[(size_t)i * ld + c0 + j];
    }
#pragma unroll
    for (int j = 0; j < US_FOLD; ++j) s[j] = wave_sum(s[j]);
    const float v = block_tree<US_FOLD>(s);
    if (threadIdx.x < US_FOLD && c0 + threadIdx.x < ncols) out[c0 + threadIdx.x] = v;
}

// ---------------------------------------------------------------- matched pairs
template <typename T>
__global__ __launch_bounds__(US_THREADS) void matched_stats_kernel(const T* __restrict__ preds, const float* __restrict__ targets,
                                                                   const int* __restrict__ rowx, const int* __restrict__ rowy,
                                                                   size_t P, int nchunks, bool vec, float* __restrict__ partial) {
    const int m = blockIdx.y;
    const T* xr = preds + (size_t)rowx[m] * P;
    const float* yr = targets + (size_t)rowy[m] * P;
    const size_t p0 = (size_t)blockIdx.x * US_CHUNK;
    const size_t end = min(P, p0 + US_CHUNK);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (size_t p = p0 + (size_t)threadIdx.x * 8; p < end; p += (size_t)US_THREADS * 8) {
        float x[8], y[8];
        load8<T>(xr, p, end, vec, x);
        load8<float>(yr, p, end, vec, y);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (p + k < end) {
                const SoftTerms s = soft_terms(x[k]);
                // BCEWithLogits as its two non-negative terms: softplus(x) - x y cancels where x is large and right
                acc[0] += y[k] * s.sp_neg + (1.f - y[k]) * s.sp_pos;
                acc[1] += s.sig * y[k];
                acc[2] += s.sig;
                acc[3] += y[k];
            }
        }
    }
    block_sums<4>(acc, partial + ((size_t)m * nchunks + blockIdx.x) * 4);
}

__global__ __launch_bounds__(US_THREADS) void matched_fold_kernel(const float* __restrict__ partial, int nchunks,
                                                                  float* __restrict__ stats) {
    const float v = fold_rows<4>(partial + (size_t)blockIdx.x * nchunks * 4, nchunks, 4);
    if (threadIdx.x < 4) stats[(size_t)blockIdx.x * 4 + threadIdx.x] = v;
}

// rowmap [R]: the pair of row (b, q), or -1
template <typename T>
__global__ __launch_bounds__(US_THREADS) void matched_grad_kernel(const T* __restrict__ preds, const float* __restrict__ targets,
                                                                  const int* __restrict__ rowmap, const int* __restrict__ rowy,
                                                                  const float* __restrict__ gstats, size_t P, bool vec,
                                                                  T* __restrict__ dpreds) {
    const size_t row = blockIdx.y;
    const int m = rowmap[row];
    T* dr = dpreds + row * P;
    const size_t p0 = (size_t)blockIdx.x * US_CHUNK;
    const size_t end = min(P, p0 + US_CHUNK);
    const T* xr = preds + row * P;
    const float* yr = m >= 0 ? targets + (size_t)rowy[m] * P : nullptr;
    const float g0 = m >= 0 ? gstats[(size_t)m * 4] : 0.f, g1 = m >= 0 ? gstats[(size_t)m * 4 + 1] : 0.f,
                g2 = m >= 0 ? gstats[(size_t)m * 4 + 2] : 0.f;
    for (size_t p = p0 + (size_t)threadIdx.x * 8; p < end; p += (size_t)US_THREADS * 8) {
        float d[8];
        if (m >= 0) {
            float x[8], y[8];
            load8<T>(xr, p, end, vec, x);
            load8<float>(yr, p, end, vec, y);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float e = expf(-fabsf(x[k]));
                const float s = x[k] >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
                d[k] = g0 * (s - y[k]) + s * (1.f - s) * (g1 * y[k] + g2);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = 0.f;
        }
        if (vec && p + 8 <= end) {
            if constexpr (sizeof(T) == 2) {
                st_chunk(dr + p, Chunk<bf16_t>::pack(d));
            } else {
                st_chunk(dr + p, Chunk<float>::pack(d));
                st_chunk(dr + p + 4, Chunk<float>::pack(d + 4));
            }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (p + k < end) dr[p + k] = from_f32<T>(d[k]);
        }
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
size_t pair_cols(int B, int Q, int TT) { return (size_t)3 * Q * TT + (size_t)B * Q + TT; }
size_t pair_ld(int B, int Q, int TT) { return (pair_cols(B, Q, TT) + US_FOLD - 1) / US_FOLD * US_FOLD; }
int chunks_of(size_t P) { return (int)((P + US_CHUNK - 1) / US_CHUNK); }

}  // namespace

namespace saicv {

extern "C" int saicv_univseg_chunk() { return US_CHUNK; }

extern "C" size_t saicv_univseg_pair_ws_floats(int B, int Q, int TT, size_t P) { return (size_t)chunks_of(P) * pair_ld(B, Q, TT); }

extern "C" int saicv_univseg_pair_sums(int dtype, const void* preds, const float* targets, const int* offsets, int B, int Q, int TT, int Tmax, size_t P,
                                       float* partial, float* sums, void* stream) {
    hipStream_t st = S(stream);
    SAICV_REQUIRE(B > 0 && Q > 0 && P > 0 && TT >= 0 && Tmax >= 0 && Tmax <= TT, "univseg_pair_sums: B=%d Q=%d P=%zu T=%d Tmax=%d", B,
                  Q, P, TT, Tmax);
    SAICV_REQUIRE(dtype == SAICV_DTYPE_BF16 || dtype == SAICV_DTYPE_F32, "univseg_pair_sums: dtype %d", dtype);
    SAICV_REQUIRE(B <= 65535, "univseg_pair_sums: B=%d exceeds the grid's z extent", B);
    const int nchunks = chunks_of(P);
    const int qblocks = (Q + 63) / 64, tgroups = Tmax > 0 ? (Tmax + US_TT * 16 - 1) / (US_TT * 16) : 1;
    SAICV_REQUIRE((size_t)qblocks * tgroups <= 65535, "univseg_pair_sums: Q=%d x Tmax=%d exceeds the grid's y extent", Q, Tmax);
    const bool vec = P % 8 == 0 && aligned16(preds) && aligned16(targets);
    const size_t ld = pair_ld(B, Q, TT), ncols = pair_cols(B, Q, TT);
    dim3 grid(nchunks, qblocks * tgroups, B);
    if (dtype == SAICV_DTYPE_BF16)
        hipLaunchKernelGGL(pair_sums_kernel<bf16_t>, grid, dim3(US_THREADS), 0, st, (const bf16_t*)preds, targets, offsets, partial, B,
                           Q, TT, P, ld, qblocks, vec);
    else
        hipLaunchKernelGGL(pair_sums_kernel<float>, grid, dim3(US_THREADS), 0, st, (const float*)preds, targets, offsets, partial, B, Q,
                           TT, P, ld, qblocks, vec);
    if (check_launch("univseg_pair_sums")) return -2;
    hipLaunchKernelGGL(pair_fold_kernel, dim3((unsigned)(ld / US_FOLD)), dim3(US_THREADS), 0, st, partial, nchunks, ld, ncols, sums);
    return check_launch("univseg_pair_fold");
}

extern "C" size_t saicv_univseg_matched_ws_floats(int M, size_t P) { return (size_t)M * chunks_of(P) * 4; }

extern "C" int saicv_univseg_matched_fwd(int dtype, const void* preds, const float* targets, const int* rowx, const int* rowy, int M, size_t P,
                                         float* partial, float* stats, void* stream) {
    hipStream_t st = S(stream);
    SAICV_REQUIRE(M >= 0 && P > 0 && M <= 65535, "univseg_matched_fwd: M=%d P=%zu", M, P);
    SAICV_REQUIRE(dtype == SAICV_DTYPE_BF16 || dtype == SAICV_DTYPE_F32, "univseg_matched_fwd: dtype %d", dtype);
    if (M == 0) return 0;
    const int nchunks = chunks_of(P);
    const bool vec = P % 8 == 0 && aligned16(preds) && aligned16(targets);
    dim3 grid(nchunks, M);
    if (dtype == SAICV_DTYPE_BF16)
        hipLaunchKernelGGL(matched_stats_kernel<bf16_t>, grid, dim3(US_THREADS), 0, st, (const bf16_t*)preds, targets, rowx, rowy, P,
                           nchunks, vec, partial);
    else
        hipLaunchKernelGGL(matched_stats_kernel<float>, grid, dim3(US_THREADS), 0, st, (const float*)preds, targets, rowx, rowy, P,
                           nchunks, vec, partial);
    if (check_launch("univseg_matched_fwd")) return -2;
    hipLaunchKernelGGL(matched_fold_kernel, dim3(M), dim3(US_THREADS), 0, st, partial, nchunks, stats);
    return check_launch("univseg_matched_fold");
}

extern "C" int saicv_univseg_matched_bwd(int dtype, const void* preds, const float* targets, const int* rowmap, const int* rowy, const float* gstats,
                                         int R, size_t P, void* dpreds, void* stream) {
    hipStream_t st = S(stream);
    SAICV_REQUIRE(R > 0 && P > 0 && R <= 65535, "univseg_matched_bwd: rows=%d P=%zu", R, P);
    SAICV_REQUIRE(dtype == SAICV_DTYPE_BF16 || dtype == SAICV_DTYPE_F32, "univseg_matched_bwd: dtype %d", dtype);
    const bool vec = P % 8 == 0 && aligned16(preds) && aligned16(targets) && aligned16(dpreds);
    dim3 grid(chunks_of(P), R);
    if (dtype == SAICV_DTYPE_BF16)
        hipLaunchKernelGGL(matched_grad_kernel<bf16_t>, grid, dim3(US_THREADS), 0, st, (const bf16_t*)preds, targets, rowmap, rowy,
                           gstats, P, vec, (bf16_t*)dpreds);
    else
        hipLaunchKernelGGL(matched_grad_kernel<float>, grid, dim3(US_THREADS), 0, st, (const float*)preds, targets, rowmap, rowy,
                           gstats, P, vec, (float*)dpreds);
    return check_launch("univseg_matched_bwd");
}

}  // namespace saicv
