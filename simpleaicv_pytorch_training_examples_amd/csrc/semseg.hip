// Semantic segmentation (reference 04.semantic_segmentation_training): the per-pixel clamped softmax cross-entropy of
// SimpleAICV/semantic_segmentation/losses.py:13-43 (CELoss) and the tap gather that turns ONE GEMM into the four convolutions of a
// CPFE block (models/pfan_semantic_segmentation.py:68-122: a 1x1 and three dilated 3x3, all Cin -> P with P << Cin).
//
// Loss.  logits [rows][C] (the NHWC view of the prediction convolution's output, bf16 or fp32, C <= 256), label fp32 [rows].
// A workgroup owns 32 consecutive rows = ONE contiguous span of 32 * C elements: it is copied into LDS with 16-byte loads (the span
// starts on a 16-byte boundary because 32 * C elements are a whole number of chunks), then every wavefront takes 8 of the rows, one
// at a time, lane l holding classes l, l + 64, l + 128, l + 192 in registers.  Forward: logits are read once; backward: read once,
// the gradient goes back through the same LDS span and leaves with 16-byte stores.  Everything else is per-row scalars.
//   p_t = exp(x_t - lse),  q = sum_{c != t} exp(x_c - lse)  (= 1 - p_t, but with RELATIVE accuracy when p_t is close to 1)
//   row loss = -log(clamp(p_t, 1e-4, 1 - 1e-4));  the row's gradient is (p - onehot) / rows inside the clamp and exactly 0
//   outside it (torch.clamp's backward), decided by p_t < 1e-4 and q < 1e-4.  (The forward takes p_t and q from its one pass of
//   exp(x - max) / sum, the backward from exp(x - lse): they can disagree only within rounding of a bound, where the loss is
//   continuous -- the gradient's regime is the backward's decision alone.)
// The mean is the ordered two-stage sum of ordered_sum.h: no atomics, bit-reproducible in every mode.
//
// Gather.  Z [N*H*W][ldz] fp32 = x . W_all^T with W_all rows (1x1 weight | per dilated branch its nine taps, tap-major);
//   out[n,h,w, 0:P] = Z[n,h,w, 0:P],  out[n,h,w, P(1+j)+k] = sum_t Z[n, h+(ty-1)d_j, w+(tx-1)d_j, P + 9P j + P t + k]
// (fp32 sum in tap order, one rounding at the store; taps outside the image count as zero), and the transposed gather backward.
// Every Z element is read by exactly one output element, every dZ element written by exactly one thread.
#include "common.h"
#include "ordered_sum.h"
#include "rowspan.h"
#include "saicv_internal.h"
#include "../../include/saicv_hip.h"

namespace {

constexpr int PCE_ROWS = 32;          // rows per workgroup (a multiple of 8: the span is whole 16-byte chunks for bf16 and fp32)
constexpr int PCE_MAX_C = 256;        // four values per lane
constexpr float PCE_LO = 1e-4f;

extern __shared__ __attribute__((aligned(16))) unsigned char pce_smem[];

// one row in registers: v[j] = x[lane + 64 j] (-inf beyond C)
template <typename T>
DEVINL void pce_load_row(const T* row, int C, int lane, float (&v)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = lane + 64 * j;
        v[j] = c < C ? to_f32(row[c]) : -INFINITY;
    }
}

// p[j] = exp(v[j] - lse);  -> q = sum over the classes other than t (all classes when t < 0), the same value in every lane
DEVINL float pce_probs(const float (&v)[4], float lse, int t, int lane, float (&p)[4]) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        p[j] = expf(v[j] - lse);                 // exp(-inf) = 0 beyond C
        if (lane + 64 * j != t) s += p[j];
    }
    return wave_sum(s);
}

template <typename T>
__global__ __launch_bounds__(256) void pixel_ce_fwd_kernel(const T* __restrict__ logits, const float* __restrict__ label, int rows,
                                                           int C, float* __restrict__ lse_out, float* __restrict__ partial) {
    T* lds = reinterpret_cast<T*>(pce_smem);
    const int r0 = blockIdx.x * PCE_ROWS;
    const int nrow = min(PCE_ROWS, rows - r0);
    stage_in(logits, lds, (size_t)r0 * C, nrow * C);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float loss_lo = -logf(PCE_LO), loss_hi = -logf(1.f - PCE_LO);
    float acc = 0.f;
    for (int i = 0; i < PCE_ROWS / 4; ++i) {
        const int lr = wave * (PCE_ROWS / 4) + i;
        if (lr >= nrow) break;                                   // wave-uniform
        const T* row = lds + (size_t)lr * C;
        float v[4];
        pce_load_row(row, C, lane, v);
        const int t = class_label(label[r0 + lr], C);
        const float mx = wave_max(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
        // one exponential pass: the denominator and the mass of the classes other than t, reduced side by side
        float se = 0.f, so = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float e = expf(v[j] - mx);                     // exp(-inf) = 0 beyond C
            se += e;
            if (lane + 64 * j != t) so += e;
        }
        se = wave_sum(se);
        so = wave_sum(so);
        const float lse = mx + logf(se);
        float loss = 0.f;
        if (t >= 0) {
            const float xt = to_f32(row[t]);
            const float pt = expf(xt - mx) / se, q = so / se;
            loss = pt < PCE_LO ? loss_lo : (q < PCE_LO ? loss_hi : lse - xt);
        }
        acc += loss;
        if (lane == 0) lse_out[r0 + lr] = lse;
    }
    const float w[1] = {acc};                                        // wave-uniform already: block_fold, not block_sums
    block_fold<1>(w, partial + blockIdx.x);
}

// loss = (sum of the workgroup partials, in a fixed order) / rows
__global__ __launch_bounds__(256) void pixel_ce_mean_kernel(const float* __restrict__ partial, int n, int rows,
                                                            float* __restrict__ loss) {
    const float total = fold_rows<1>(partial, n, 1);
    if (threadIdx.x == 0) loss[0] = total / (float)rows;
}

template <typename T>
__global__ __launch_bounds__(256) void pixel_ce_bwd_kernel(const T* __restrict__ logits, const float* __restrict__ label,
                                                           const float* __restrict__ lse_in, const float* __restrict__ upstream,
                                                           int rows, int C, T* __restrict__ dlogits) {
    T* lds = reinterpret_cast<T*>(pce_smem);
    const int r0 = blockIdx.x * PCE_ROWS;
    const int nrow = min(PCE_ROWS, rows - r0);
    stage_in(logits, lds, (size_t)r0 * C, nrow * C);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float inv_rows = 1.f / (float)rows, up = upstream[0];
    for (int i = 0; i < PCE_ROWS / 4; ++i) {
        const int lr = wave * (PCE_ROWS / 4) + i;
        if (lr >= nrow) break;
        T* row = lds + (size_t)lr * C;
        float v[4], p[4];
        pce_load_row(row, C, lane, v);
        const float lse = lse_in[r0 + lr];
        const int t = class_label(label[r0 + lr], C);
        const float q = pce_probs(v, lse, t, lane, p);
        bool live = false;
        if (t >= 0) {
            const float pt = expf(to_f32(row[t]) - lse);
            live = !(pt < PCE_LO) && !(q < PCE_LO);
        }
        // (the row is in registers and x_t has been read by every lane of this wavefront: its LDS span now takes the gradient)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = lane + 64 * j;
            if (c < C) {
                const float d = (c == t) ? -q : p[j];            // p_t - 1 = -q
                row[c] = from_f32<T>(live ? (d * inv_rows) * up : 0.f);
            }
        }
    }
    __syncthreads();
    stage_out(dlogits, lds, (size_t)r0 * C, nrow * C);
}

// ------------------------------------------------------------------------------------------------ CPFE tap gather
template <typename T> struct Quad;            // four consecutive elements as one access
template <> struct Quad<bf16_t> { typedef bf16x4 type; };
template <> struct Quad<float> { typedef f32x4 type; };

struct CpfeGeom {
    int N, H, W, P, nb;
    int dil[3];
    long ldz;
};

// one thread: four consecutive channels of one output pixel
template <typename T>
__global__ __launch_bounds__(256) void cpfe_gather_fwd_kernel(const float* __restrict__ z, T* __restrict__ out, CpfeGeom g,
                                                              size_t total) {
    const int P = g.P, groups = (1 + g.nb) * P / 4, Co = (1 + g.nb) * P;
    const size_t gstride = (size_t)gridDim.x * blockDim.x;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gstride) {
        const size_t pix = idx / groups;
        const int c0 = (int)(idx - pix * groups) * 4;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (c0 < P) {
            acc = *reinterpret_cast<const f32x4*>(z + pix * (size_t)g.ldz + c0);
        } else {
            const int j = c0 / P - 1, k = c0 - (j + 1) * P, d = g.dil[j];
            const int w = (int)(pix % g.W), h = (int)((pix / g.W) % g.H);
            const float* zb = z + P + (size_t)9 * P * j + k;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int hh = h + (t / 3 - 1) * d, ww = w + (t % 3 - 1) * d;
                if (hh >= 0 && hh < g.H && ww >= 0 && ww < g.W) {
                    const size_t src = pix + (ptrdiff_t)(hh - h) * g.W + (ww - w);
                    acc += *reinterpret_cast<const f32x4*>(zb + src * (size_t)g.ldz + (size_t)P * t);
                }
            }
        }
        typename Quad<T>::type o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = from_f32<T>(acc[e]);
        *reinterpret_cast<typename Quad<T>::type*>(out + pix * Co + c0) = o;
    }
}

// one thread: four consecutive columns of one dZ row (dZ in the compute dtype, dense [M][(1 + 9 nb) P])
template <typename T>
__global__ __launch_bounds__(256) void cpfe_gather_bwd_kernel(const T* __restrict__ dout, T* __restrict__ dz, CpfeGeom g,
                                                              size_t total) {
    const int P = g.P, Cz = (1 + 9 * g.nb) * P, groups = Cz / 4, Co = (1 + g.nb) * P;
    const size_t gstride = (size_t)gridDim.x * blockDim.x;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gstride) {
        const size_t pix = idx / groups;
        const int c0 = (int)(idx - pix * groups) * 4;
        typedef typename Quad<T>::type Q;
        Q val;
#pragma unroll
        for (int e = 0; e < 4; ++e) val[e] = from_f32<T>(0.f);
        const T* src = nullptr;
        if (c0 < P) {
            src = dout + pix * Co + c0;
        } else {
            const int r = c0 - P, j = r / (9 * P), t = (r - j * 9 * P) / P, k = r - j * 9 * P - t * P, d = g.dil[j];
            const int w = (int)(pix % g.W), h = (int)((pix / g.W) % g.H);
            const int hh = h - (t / 3 - 1) * d, ww = w - (t % 3 - 1) * d;
            if (hh >= 0 && hh < g.H && ww >= 0 && ww < g.W)
                src = dout + (pix + (ptrdiff_t)(hh - h) * g.W + (ww - w)) * Co + (size_t)P * (1 + j) + k;
        }
        if (src) val = *reinterpret_cast<const Q*>(src);
        *reinterpret_cast<Q*>(dz + pix * Cz + c0) = val;
    }
}

int cpfe_geom(CpfeGeom& g, int N, int H, int W, int P, int nb, const int* dil, long ldz, const char* what) {
    SAICV_REQUIRE(N > 0 && H > 0 && W > 0 && P > 0, "%s: empty problem", what);
    SAICV_REQUIRE(P % 4 == 0, "%s: planes per branch (%d) must be a multiple of 4", what, P);
    SAICV_REQUIRE(nb >= 1 && nb <= 3, "%s: 1 to 3 dilated branches, got %d", what, nb);
    SAICV_REQUIRE(dil != nullptr, "%s: null dilation list", what);
    g.N = N; g.H = H; g.W = W; g.P = P; g.nb = nb; g.ldz = ldz;
    for (int j = 0; j < 3; ++j) {
        g.dil[j] = j < nb ? dil[j] : 1;
        SAICV_REQUIRE(g.dil[j] >= 1, "%s: dilation %d must be positive", what, g.dil[j]);
    }
    return 0;
}

int grid_for(size_t total) {
    size_t b = (total + 255) / 256;
    if (b > 16384) b = 16384;
    return b < 1 ? 1 : (int)b;
}

}  // namespace

namespace saicv {

extern "C" size_t saicv_pixel_softmax_ce_ws_floats(size_t rows) { return (rows + PCE_ROWS - 1) / PCE_ROWS; }

static int pce_check(const char* what, const void* logits, size_t rows, int C) {
    SAICV_REQUIRE(logits != nullptr, "%s: null logits", what);
    SAICV_REQUIRE(rows > 0 && rows <= 0x7fffffffu && C >= 1, "%s: empty problem or more than 2^31 - 1 rows", what);
    SAICV_REQUIRE(C <= PCE_MAX_C, "%s: %d classes; the row-in-registers kernel holds at most %d", what, C, PCE_MAX_C);
    SAICV_REQUIRE(((uintptr_t)logits & 15) == 0, "%s: the logits must start on a 16-byte boundary", what);
    return 0;
}

extern "C" int saicv_pixel_softmax_ce_fwd(int dtype, const void* logits, const float* label, size_t rows, int C, float* lse, float* partial,
                                          float* loss, void* stream) {
    hipStream_t st = S(stream);
    if (pce_check("pixel_softmax_ce_fwd", logits, rows, C)) return -1;
    const int blocks = (int)saicv_pixel_softmax_ce_ws_floats(rows);
    if (dtype == SAICV_DTYPE_BF16) {
        const size_t smem = span_bytes(PCE_ROWS, C, sizeof(bf16_t));
        hipLaunchKernelGGL(pixel_ce_fwd_kernel<bf16_t>, dim3(blocks), dim3(256), smem, st, (const bf16_t*)logits, label, (int)rows, C,
                           lse, partial);
    } else {
        const size_t smem = span_bytes(PCE_ROWS, C, sizeof(float));
        hipLaunchKernelGGL(pixel_ce_fwd_kernel<float>, dim3(blocks), dim3(256), smem, st, (const float*)logits, label, (int)rows, C,
                           lse, partial);
    }
    hipLaunchKernelGGL(pixel_ce_mean_kernel, dim3(1), dim3(256), 0, st, partial, blocks, (int)rows, loss);
    return check_launch("pixel_softmax_ce_fwd");
}

extern "C" int saicv_pixel_softmax_ce_bwd(int dtype, const void* logits, const float* label, const float* lse, const float* upstream, size_t rows,
                                          int C, void* dlogits, void* stream) {
    hipStream_t st = S(stream);
    if (pce_check("pixel_softmax_ce_bwd", logits, rows, C)) return -1;
    SAICV_REQUIRE(((uintptr_t)dlogits & 15) == 0 && dlogits != nullptr, "pixel_softmax_ce_bwd: the gradient must start on a 16-byte boundary");
    const int blocks = (int)saicv_pixel_softmax_ce_ws_floats(rows);
    if (dtype == SAICV_DTYPE_BF16)
        hipLaunchKernelGGL(pixel_ce_bwd_kernel<bf16_t>, dim3(blocks), dim3(256), span_bytes(PCE_ROWS, C, sizeof(bf16_t)), st,
                           (const bf16_t*)logits, label, lse, upstream, (int)rows, C, (bf16_t*)dlogits);
    else
        hipLaunchKernelGGL(pixel_ce_bwd_kernel<float>, dim3(blocks), dim3(256), span_bytes(PCE_ROWS, C, sizeof(float)), st,
                           (const float*)logits, label, lse, upstream, (int)rows, C, (float*)dlogits);
    return check_launch("pixel_softmax_ce_bwd");
}

extern "C" int saicv_cpfe_gather_fwd(int dtype, const float* z, long ldz, void* out, int N, int H, int W, int P, int nb, int d0, int d1,
                                     int d2, void* stream) {
    const int dil[3] = {d0, d1, d2};
    hipStream_t st = S(stream);
    CpfeGeom g;
    if (cpfe_geom(g, N, H, W, P, nb, dil, ldz, "cpfe_gather_fwd")) return -1;
    SAICV_REQUIRE(ldz >= (long)(1 + 9 * nb) * P && ldz % 4 == 0 && ((uintptr_t)z & 15) == 0,
                  "cpfe_gather_fwd: Z rows must hold (1 + 9 * branches) * P floats on 16-byte boundaries");
    const size_t total = (size_t)N * H * W * ((1 + nb) * P / 4);
    if (dtype == SAICV_DTYPE_BF16)
        hipLaunchKernelGGL(cpfe_gather_fwd_kernel<bf16_t>, dim3(grid_for(total)), dim3(256), 0, st, z, (bf16_t*)out, g, total);
    else
        hipLaunchKernelGGL(cpfe_gather_fwd_kernel<float>, dim3(grid_for(total)), dim3(256), 0, st, z, (float*)out, g, total);
    return check_launch("cpfe_gather_fwd");
}

extern "C" int saicv_cpfe_gather_bwd(int dtype, const void* dout, void* dz, int N, int H, int W, int P, int nb, int d0, int d1, int d2,
                                     void* stream) {
    const int dil[3] = {d0, d1, d2};
    hipStream_t st = S(stream);
    CpfeGeom g;
    if (cpfe_geom(g, N, H, W, P, nb, dil, 0, "cpfe_gather_bwd")) return -1;
    const size_t total = (size_t)N * H * W * ((1 + 9 * nb) * P / 4);
    if (dtype == SAICV_DTYPE_BF16)
        hipLaunchKernelGGL(cpfe_gather_bwd_kernel<bf16_t>, dim3(grid_for(total)), dim3(256), 0, st, (const bf16_t*)dout, (bf16_t*)dz, g, total);
    else
        hipLaunchKernelGGL(cpfe_gather_bwd_kernel<float>, dim3(grid_for(total)), dim3(256), 0, st, (const float*)dout, (float*)dz, g, total);
    return check_launch("cpfe_gather_bwd");
}

}  // namespace saicv
