// Face and human parsing (reference 11.face_parsing_training / 12.human_parsing_training): everything the four losses of
// SimpleAICV/human_parsing/losses.py (CELoss :13-43, MultiClassBCELoss :46-76, IoULoss :79-113, DiceLoss :116-149) read of the
// full-resolution prediction, in ONE pass over the logits each way.
//
// logits [rows][C] (the NHWC view of the prediction, bf16 or fp32, 2 <= C <= 256), label fp32 [rows] holding class ids.  Per row,
// with lo = 1e-4, hi = 1 - 1e-4, target t, one-hot y:
//   a = softmax(z) or sigmoid(z),  q_c = clamp(a_c, lo, hi),  m_c = [lo <= a_c <= hi] (per ELEMENT),
//   I = q_t,  S = sum_c q_c,  U = max(S + 1 - I, 1e-4),  D = S + 1 + 1e-4
//   terms[0] = mean_rows -log q_t                                     (softmax)
//            = mean_{rows C} -(y_c log q_c + (1 - y_c) log(1 - q_c))  (sigmoid)
//   terms[1] = mean_rows 1 - I / U,   terms[2] = mean_rows 1 - (2 I + 1e-4) / D
// A label outside [0, C) adds nothing to any term, no gradient, and still counts in the denominators.
// Backward from g[3] = dL/dterms (device memory):  h_c = m_c * sum_k g_k dterm_k/dq_c,  then  dz_j = a_j (h_j - sum_c h_c a_c)
// (softmax) or dz_j = h_j a_j (1 - a_j) (sigmoid).  h takes two values per row under softmax (the target's and everybody else's),
// so sum_c h_c a_c is two masked sums of a.
//
// Accuracy at the upper bound: under softmax only a class with a_c > 1/2 can exceed hi, and it does iff the SUM of the other
// classes' probabilities is below lo (never 1 - a_c); under sigmoid 1 - a is sigmoid(-z), both from exp(-|z|).
//
// Two row mappings:
//   lane form (C <= 32): a workgroup owns 256 consecutive rows = one contiguous span of 256 * C elements (<= 32 KB; whole 16-byte
//     chunks, so it starts on a 16-byte boundary), copied into LDS with 16-byte loads; lane l then takes row l into registers.
//     No cross-lane traffic per row; at 19 or 20 classes every lane works.
//   wave form (C <= 256): pixel_ce's mapping -- 32 rows per workgroup, one wavefront per row, lane l holding classes l + 64 j.
// Both run the same row routine (pct_*<N, WAVE>): only the slot -> class map and the reductions differ.  The backward recomputes
// the row statistics from the logits (nothing per row is kept: 4 bytes per row each way would be a tenth of the traffic at 20 bf16
// classes); the gradient leaves through the same LDS span with 16-byte stores.  All means are ordered sums (ordered_sum.h): no atomics.
#include "common.h"
#include "ordered_sum.h"
#include "rowspan.h"
#include "saicv_internal.h"
#include "../../include/saicv_hip.h"

namespace {

constexpr int PCT_LANE_ROWS = 256;    // lane form: one row per lane
constexpr int PCT_LANE_MAX_C = 32;    // ... while the row fits 32 registers
constexpr int PCT_WAVE_ROWS = 32;     // wave form: rows per workgroup (a multiple of 8: whole 16-byte chunks)
constexpr int PCT_MAX_C = 256;
constexpr float PCT_LO = 1e-4f, PCT_HI = 1.f - 1e-4f, PCT_EPS = 1e-4f;

extern __shared__ __attribute__((aligned(16))) unsigned char pct_smem[];

// slot j of a lane's registers holds class j (lane form, N = 32) or class lane + 64 j (wave form, N = 4)
template <bool WAVE> DEVINL int pct_class(int j, int lane) { return WAVE ? lane + 64 * j : j; }
template <bool WAVE> DEVINL float pct_sum(float x) { return WAVE ? wave_sum(x) : x; }
template <bool WAVE> DEVINL float pct_max(float x) { return WAVE ? wave_max(x) : x; }

template <int N, bool WAVE, typename T>
DEVINL void pct_load_row(const T* row, int C, int lane, float (&v)[N]) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int c = pct_class<WAVE>(j, lane);
        v[j] = c < C ? to_f32(row[c]) : -INFINITY;
    }
}
template <int N, bool WAVE, typename T>
DEVINL void pct_store_row(T* row, int C, int lane, const float (&v)[N]) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int c = pct_class<WAVE>(j, lane);
        if (c < C) row[c] = from_f32<T>(v[j]);
    }
}

// what a row's terms and gradient coefficients are made of
struct PctRow {
    float S;         // sum_c q_c
    float at;        // a_t (softmax) -- unused under sigmoid
    float qt;        // q_t
    float term0;     // -log q_t (softmax) or the row's BCE sum (sigmoid)
    bool up;         // softmax: the class with a > 1/2 (if any) is above hi
};

// softmax: v <- a = softmax(v) in place; the row's lse; whether the one class above 1/2 lies above hi; x_t
template <int N, bool WAVE>
DEVINL void pct_softmax(float (&v)[N], int C, int t, int lane, float& lse, float& xt, bool& up) {
    float mx = -INFINITY, x = 0.f;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int c = pct_class<WAVE>(j, lane);
        if (c < C) {
            mx = fmaxf(mx, v[j]);
            if (c == t) x = v[j];
        }
    }
    mx = pct_max<WAVE>(mx);
    xt = pct_sum<WAVE>(x);
    float se = 0.f;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        if (pct_class<WAVE>(j, lane) < C) {
            v[j] = expf(v[j] - mx);
            se += v[j];
        }
    }
    se = pct_sum<WAVE>(se);
    const float inv = 1.f / se;
    float rest = 0.f;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        if (pct_class<WAVE>(j, lane) < C) {
            v[j] *= inv;
            rest += v[j] <= 0.5f ? v[j] : 0.f;
        }
    }
    up = pct_sum<WAVE>(rest) < PCT_LO;
    lse = mx + logf(se);
}

DEVINL bool pct_sm_live(float a, bool up) { return !(a < PCT_LO) && !(a > 0.5f && up); }
DEVINL float pct_sm_clamp(float a, bool up) { return a < PCT_LO ? PCT_LO : ((a > 0.5f && up) ? PCT_HI : a); }

// sigmoid of one logit: a, 1 - a (= sigmoid(-z)), their clamped values and the element mask, all from exp(-|z|)
struct PctSig { float a, na, q, nq; bool m; };
DEVINL PctSig pct_sigmoid(float z) {
    const float e = expf(-fabsf(z)), r = 1.f / (1.f + e), s = e * r;
    PctSig o;
    o.a = z >= 0.f ? r : s;
    o.na = z >= 0.f ? s : r;
    const bool low = o.a < PCT_LO, high = o.na < PCT_LO;
    o.q = low ? PCT_LO : (high ? PCT_HI : o.a);
    o.nq = low ? PCT_HI : (high ? PCT_LO : o.na);
    o.m = !low && !high;
    return o;
}

// softmax row after pct_softmax: S, a_t, q_t, -log q_t
template <int N, bool WAVE>
DEVINL PctRow pct_softmax_stats(const float (&a)[N], int C, int t, int lane, float lse, float xt, bool up) {
    float S = 0.f, at = 0.f;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int c = pct_class<WAVE>(j, lane);
        if (c < C) {
            S += pct_sm_clamp(a[j], up);
            if (c == t) at = a[j];
        }
    }
    PctRow r;
    r.S = pct_sum<WAVE>(S);
    r.at = pct_sum<WAVE>(at);
    r.qt = pct_sm_clamp(r.at, up);
    r.up = up;
    r.term0 = r.at < PCT_LO ? -logf(PCT_LO) : ((r.at > 0.5f && up) ? -logf(PCT_HI) : lse - xt);
    return r;
}

// sigmoid row straight from the logits: S, q_t, the BCE sum over the classes
template <int N, bool WAVE>
DEVINL PctRow pct_sigmoid_stats(const float (&v)[N], int C, int t, int lane) {
    float S = 0.f, qt = 0.f, bce = 0.f;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int c = pct_class<WAVE>(j, lane);
        if (c < C) {
            const PctSig s = pct_sigmoid(v[j]);
            S += s.q;
            if (c == t) qt = s.q;
            bce -= logf(c == t ? s.q : s.nq);
        }
    }
    PctRow r;
    r.S = pct_sum<WAVE>(S);
    r.qt = pct_sum<WAVE>(qt);
    r.term0 = pct_sum<WAVE>(bce);
    r.at = 0.f;
    r.up = false;
    return r;
}

// one valid row (t >= 0): v holds the logits on entry.  -> the row's three terms (the same value in every lane of a wave-form row)
template <int N, bool WAVE, bool SIG>
DEVINL void pct_row_fwd(float (&v)[N], int C, int t, int lane, float (&out)[3]) {
    PctRow r;
    if constexpr (SIG) {
        r = pct_sigmoid_stats<N, WAVE>(v, C, t, lane);
    } else {
        float lse, xt;
        bool up;
        pct_softmax<N, WAVE>(v, C, t, lane, lse, xt, up);
        r = pct_softmax_stats<N, WAVE>(v, C, t, lane, lse, xt, up);
    }
    const float U = fmaxf(r.S + 1.f - r.qt, PCT_EPS), D = r.S + 1.f + PCT_EPS;
    out[0] = r.term0;
    out[1] = 1.f - r.qt / U;
    out[2] = 1.f - (2.f * r.qt + PCT_EPS) / D;
}

// one valid row: v holds the logits on entry and the gradient dz on return.  g = dL/dterms, inv_rows = 1 / rows
template <int N, bool WAVE, bool SIG>
DEVINL void pct_row_bwd(float (&v)[N], int C, int t, int lane, const float (&g)[3], float inv_rows) {
    PctRow r;
    float lse, xt;
    bool up = false;
    if constexpr (SIG) {
        r = pct_sigmoid_stats<N, WAVE>(v, C, t, lane);
    } else {
        pct_softmax<N, WAVE>(v, C, t, lane, lse, xt, up);
        r = pct_softmax_stats<N, WAVE>(v, C, t, lane, lse, xt, up);
    }
    const float U = fmaxf(r.S + 1.f - r.qt, PCT_EPS), D = r.S + 1.f + PCT_EPS, two_i = 2.f * r.qt + PCT_EPS;
    const float g0 = SIG ? g[0] / (float)C : g[0];
    // dterm/dq at the target and at every other class (the BCE part of the others depends on the class: added per element)
    const float ht = -g0 / r.qt - g[1] / U - g[2] * (2.f * D - two_i) / (D * D);
    const float ho = g[1] * r.qt / (U * U) + g[2] * two_i / (D * D);
    if constexpr (SIG) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int c = pct_class<WAVE>(j, lane);
            if (c < C) {
                const PctSig s = pct_sigmoid(v[j]);
                const float h = c == t ? ht : ho + g0 / s.nq;
                v[j] = s.m ? (h * (s.a * s.na)) * inv_rows : 0.f;
            }
        }
    } else {
        float am = 0.f;                                           // sum over the live classes other than t of a
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int c = pct_class<WAVE>(j, lane);
            if (c < C && c != t && pct_sm_live(v[j], up)) am += v[j];
        }
        am = pct_sum<WAVE>(am);
        const bool tlive = pct_sm_live(r.at, up);
        const float dot = ho * am + (tlive ? ht * r.at : 0.f);    // sum_c h_c a_c
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int c = pct_class<WAVE>(j, lane);
            if (c < C) {
                const float h = pct_sm_live(v[j], up) ? (c == t ? ht : ho) : 0.f;
                v[j] = (v[j] * (h - dot)) * inv_rows;
            }
        }
    }
}

// -------------------------------------------------------------------------------------------------- lane form
// partial [blocks][3]
template <typename T, bool SIG>
__global__ __launch_bounds__(256) void pct_lane_fwd_kernel(const T* __restrict__ logits, const float* __restrict__ label, int rows,
                                                           int C, float* __restrict__ partial) {
    T* lds = reinterpret_cast<T*>(pct_smem);
    const int r0 = blockIdx.x * PCT_LANE_ROWS;
    const int nrow = min(PCT_LANE_ROWS, rows - r0);
    stage_in(logits, lds, (size_t)r0 * C, nrow * C);
    __syncthreads();
    const int tid = threadIdx.x, lane = tid & 63;
    float out[3] = {0.f, 0.f, 0.f};
    if (tid < nrow) {
        const int t = class_label(label[r0 + tid], C);
        if (t >= 0) {
            float v[PCT_LANE_MAX_C];
            pct_load_row<PCT_LANE_MAX_C, false>(lds + (size_t)tid * C, C, lane, v);
            pct_row_fwd<PCT_LANE_MAX_C, false, SIG>(v, C, t, lane, out);
        }
    }
    block_sums<3>(out, partial + (size_t)blockIdx.x * 3);
}

template <typename T, bool SIG>
__global__ __launch_bounds__(256) void pct_lane_bwd_kernel(const T* __restrict__ logits, const float* __restrict__ label,
                                                           const float* __restrict__ gterms, int rows, int C,
                                                           T* __restrict__ dlogits) {
    T* lds = reinterpret_cast<T*>(pct_smem);
    const int r0 = blockIdx.x * PCT_LANE_ROWS;
    const int nrow = min(PCT_LANE_ROWS, rows - r0);
    stage_in(logits, lds, (size_t)r0 * C, nrow * C);
    __syncthreads();
    const int tid = threadIdx.x, lane = tid & 63;
    const float g[3] = {gterms[0], gterms[1], gterms[2]};
    if (tid < nrow) {
        // (a lane reads and writes only its own row of the span: no barrier between the two)
        T* row = lds + (size_t)tid * C;
        const int t = class_label(label[r0 + tid], C);
        float v[PCT_LANE_MAX_C];
        if (t >= 0) {
            pct_load_row<PCT_LANE_MAX_C, false>(row, C, lane, v);
            pct_row_bwd<PCT_LANE_MAX_C, false, SIG>(v, C, t, lane, g, 1.f / (float)rows);
        } else {
#pragma unroll
            for (int j = 0; j < PCT_LANE_MAX_C; ++j) v[j] = 0.f;
        }
        pct_store_row<PCT_LANE_MAX_C, false>(row, C, lane, v);
    }
    __syncthreads();
    stage_out(dlogits, lds, (size_t)r0 * C, nrow * C);
}

// -------------------------------------------------------------------------------------------------- wave form
template <typename T, bool SIG>
__global__ __launch_bounds__(256) void pct_wave_fwd_kernel(const T* __restrict__ logits, const float* __restrict__ label, int rows,
                                                           int C, float* __restrict__ partial) {
    T* lds = reinterpret_cast<T*>(pct_smem);
    const int r0 = blockIdx.x * PCT_WAVE_ROWS;
    const int nrow = min(PCT_WAVE_ROWS, rows - r0);
    stage_in(logits, lds, (size_t)r0 * C, nrow * C);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int i = 0; i < PCT_WAVE_ROWS / 4; ++i) {
        const int lr = wave * (PCT_WAVE_ROWS / 4) + i;
        if (lr >= nrow) break;                                   // wave-uniform
        const int t = class_label(label[r0 + lr], C);
        if (t < 0) continue;                                     // wave-uniform
        float v[4], out[3];
        pct_load_row<4, true>(lds + (size_t)lr * C, C, lane, v);
        pct_row_fwd<4, true, SIG>(v, C, t, lane, out);
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] += out[k];
    }
    block_fold<3>(acc, partial + (size_t)blockIdx.x * 3);           // wave-uniform already: block_fold, not block_sums
}

template <typename T, bool SIG>
__global__ __launch_bounds__(256) void pct_wave_bwd_kernel(const T* __restrict__ logits, const float* __restrict__ label,
                                                           const float* __restrict__ gterms, int rows, int C,
                                                           T* __restrict__ dlogits) {
    T* lds = reinterpret_cast<T*>(pct_smem);
    const int r0 = blockIdx.x * PCT_WAVE_ROWS;
    const int nrow = min(PCT_WAVE_ROWS, rows - r0);
    stage_in(logits, lds, (size_t)r0 * C, nrow * C);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float g[3] = {gterms[0], gterms[1], gterms[2]};
    const float inv_rows = 1.f / (float)rows;
    for (int i = 0; i < PCT_WAVE_ROWS / 4; ++i) {
        const int lr = wave * (PCT_WAVE_ROWS / 4) + i;
        if (lr >= nrow) break;
        T* row = lds + (size_t)lr * C;
        const int t = class_label(label[r0 + lr], C);
        float v[4];
        if (t >= 0) {
            pct_load_row<4, true>(row, C, lane, v);
            pct_row_bwd<4, true, SIG>(v, C, t, lane, g, inv_rows);
        } else {
            v[0] = v[1] = v[2] = v[3] = 0.f;
        }
        pct_store_row<4, true>(row, C, lane, v);                 // (a wavefront reads and writes only its own rows of the span)
    }
    __syncthreads();
    stage_out(dlogits, lds, (size_t)r0 * C, nrow * C);
}

// terms[k] = (sum of the workgroup partials of term k, in a fixed order) / denominator
__global__ __launch_bounds__(256) void pct_mean_kernel(const float* __restrict__ partial, int n, float inv0, float inv12,
                                                       float* __restrict__ terms) {
    const float total = fold_rows<3>(partial, n, 3);
    if (threadIdx.x < 3) terms[threadIdx.x] = total * (threadIdx.x == 0 ? inv0 : inv12);
}

int pct_check(const char* what, const void* logits, const float* label, size_t rows, int C, int form) {
    SAICV_REQUIRE(logits != nullptr && label != nullptr, "%s: null logits or labels", what);
    SAICV_REQUIRE(rows > 0 && rows <= 0x7fffffffu, "%s: empty problem or more than 2^31 - 1 rows", what);
    SAICV_REQUIRE(C <= PCT_MAX_C, "%s: %d classes; the row-in-registers kernel holds at most %d", what, C, PCT_MAX_C);
    SAICV_REQUIRE(C >= 2, "%s: %d classes; at least 2", what, C);
    SAICV_REQUIRE(((uintptr_t)logits & 15) == 0, "%s: the logits must start on a 16-byte boundary", what);
    SAICV_REQUIRE(form >= 0 && form <= 2, "%s: form is 0 (by class count), 1 (lane per row) or 2 (wavefront per row)", what);
    SAICV_REQUIRE(form != 1 || C <= PCT_LANE_MAX_C, "%s: the lane-per-row form holds at most %d classes, got %d", what,
                  PCT_LANE_MAX_C, C);
    return 0;
}

bool pct_lane_form(int C, int form) { return form == 1 || (form == 0 && C <= PCT_LANE_MAX_C); }

template <typename T>
void pct_launch_fwd(const T* logits, const float* label, int rows, int C, bool sig, bool lane, float* partial, hipStream_t st) {
    const int tile = lane ? PCT_LANE_ROWS : PCT_WAVE_ROWS;
    const int blocks = (rows + tile - 1) / tile;
    const size_t smem = span_bytes(tile, C, sizeof(T));
    auto k = lane ? (sig ? pct_lane_fwd_kernel<T, true> : pct_lane_fwd_kernel<T, false>)
                  : (sig ? pct_wave_fwd_kernel<T, true> : pct_wave_fwd_kernel<T, false>);
    hipLaunchKernelGGL(k, dim3(blocks), dim3(256), smem, st, logits, label, rows, C, partial);
}

template <typename T>
void pct_launch_bwd(const T* logits, const float* label, const float* g, int rows, int C, bool sig, bool lane, T* dlogits,
                    hipStream_t st) {
    const int tile = lane ? PCT_LANE_ROWS : PCT_WAVE_ROWS;
    const int blocks = (rows + tile - 1) / tile;
    const size_t smem = span_bytes(tile, C, sizeof(T));
    auto k = lane ? (sig ? pct_lane_bwd_kernel<T, true> : pct_lane_bwd_kernel<T, false>)
                  : (sig ? pct_wave_bwd_kernel<T, true> : pct_wave_bwd_kernel<T, false>);
    hipLaunchKernelGGL(k, dim3(blocks), dim3(256), smem, st, logits, label, g, rows, C, dlogits);
}

}  // namespace

namespace saicv {

// enough for either form: three partials per workgroup of the smaller tile
extern "C" size_t saicv_pixel_class_terms_ws_floats(size_t rows) { return 3 * ((rows + PCT_WAVE_ROWS - 1) / PCT_WAVE_ROWS); }

extern "C" int saicv_pixel_class_terms_lane_max_classes() { return PCT_LANE_MAX_C; }

extern "C" int saicv_pixel_class_terms_fwd(int dtype, const void* logits, const float* label, size_t rows, int C, int sigmoid, int form,
                                           float* partial, float* terms, void* stream) {
    hipStream_t st = S(stream);
    if (pct_check("pixel_class_terms_fwd", logits, label, rows, C, form)) return -1;
    SAICV_REQUIRE(partial != nullptr && terms != nullptr, "pixel_class_terms_fwd: null workspace or output");
    const bool lane = pct_lane_form(C, form);
    if (dtype == SAICV_DTYPE_BF16)
        pct_launch_fwd((const bf16_t*)logits, label, (int)rows, C, sigmoid != 0, lane, partial, st);
    else
        pct_launch_fwd((const float*)logits, label, (int)rows, C, sigmoid != 0, lane, partial, st);
    const int tile = lane ? PCT_LANE_ROWS : PCT_WAVE_ROWS;
    const int blocks = (int)((rows + tile - 1) / tile);
    const float inv = (float)(1.0 / (double)rows);
    hipLaunchKernelGGL(pct_mean_kernel, dim3(1), dim3(256), 0, st, partial, blocks,
                       sigmoid ? (float)(1.0 / ((double)rows * C)) : inv, inv, terms);
    return check_launch("pixel_class_terms_fwd");
}

extern "C" int saicv_pixel_class_terms_bwd(int dtype, const void* logits, const float* label, const float* gterms, size_t rows, int C, int sigmoid,
                                           int form, void* dlogits, void* stream) {
    hipStream_t st = S(stream);
    if (pct_check("pixel_class_terms_bwd", logits, label, rows, C, form)) return -1;
    SAICV_REQUIRE(gterms != nullptr, "pixel_class_terms_bwd: null dL/dterms");
    SAICV_REQUIRE(dlogits != nullptr && ((uintptr_t)dlogits & 15) == 0,
                  "pixel_class_terms_bwd: the gradient must start on a 16-byte boundary");
    const bool lane = pct_lane_form(C, form);
    if (dtype == SAICV_DTYPE_BF16)
        pct_launch_bwd((const bf16_t*)logits, label, gterms, (int)rows, C, sigmoid != 0, lane, (bf16_t*)dlogits, st);
    else
        pct_launch_bwd((const float*)logits, label, gterms, (int)rows, C, sigmoid != 0, lane, (float*)dlogits, st);
    return check_launch("pixel_class_terms_bwd");
}

}  // namespace saicv
