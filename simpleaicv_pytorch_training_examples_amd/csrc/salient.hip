// Salient object detection (reference 06.salient_object_detection_training): the one-channel 3x3 prediction head of
// SimpleAICV/salient_object_detection/models/pfan_segmentation.py:254-300 (pred_conv, pred.float(), sigmoid) and the four per-sample
// sums that BCELoss / BCEIouloss / BCEDiceLoss of SimpleAICV/salient_object_detection/losses.py:16-134 are made of.
//
// Head.  x NHWC [N][H][W][C] (bf16 or fp32, C % 8 == 0, 8 <= C <= 64), weight fp32 [1][C][3][3] read in place through two strides
// (element (c, tap) at w[c * wsc + tap * wsk]: contiguous and channels-last parameters alike), fp32 bias, fp32 output [N][H][W].
// Both directions stream x once in 16-byte chunks, consecutive lanes on consecutive chunks; nothing is an MFMA tile (one output
// channel would leave the tile empty).
//   forward:  a workgroup owns a 16 x 32 output tile.  For every pixel of the 18 x 34 input tile it forms the nine tap products
//             t[k] = sum_c x[c] * w[c][k] (1, 2 or 4 lanes share a pixel's chunks and add their parts with lane exchanges), parks
//             them in LDS, and an output pixel is the sum of nine parked values of its neighbours + bias (+ sigmoid).
//   backward: a workgroup owns an 8 x 256 pixel tile and holds dz (= dout * p * (1 - p), or dout) with a one-pixel halo in LDS.  A
//             lane owns ONE chunk position (its channels never change) and walks over pixels: the nine dz neighbours give its
//             chunk of dx (stored once) and, times x, its 9 x 8 (9 x 4 for fp32) weight-gradient accumulators, which stay in
//             registers for the whole tile.  They are folded through LDS in thread order into one partial row per workgroup;
//             a second launch adds the rows in index order.  No atomics: dw and db are bit-reproducible in every mode.
//
// Mask statistics.  prob, label fp32 [B][P] -> stats [B][4] = (sum bce, sum ph, sum l, sum ph * l) with ph = clamp(p, 1e-4f,
// 1 - 1e-4f) and bce = -(l log ph + (1 - l) log(1 - ph)); one read of both arrays each way, the ordered sums of ordered_sum.h.
#include "common.h"
#include "ordered_sum.h"
#include "saicv_internal.h"
#include "../../include/saicv_hip.h"

namespace {

constexpr int C1_MAX_C = 64;
constexpr int C1_TH = 16, C1_TW = 32;                                   // forward: output tile
constexpr int C1_IH = C1_TH + 2, C1_IW = C1_TW + 2, C1_NPIX = C1_IH * C1_IW;
constexpr int C1_BH = 8, C1_BW = 256;                                   // backward: pixel tile
constexpr int C1_ZW = C1_BW + 2, C1_ZH = C1_BH + 2;
constexpr int C1_PASS = 18;                                             // accumulators folded per LDS pass
constexpr int C1_RED_LD = 257;

struct C1Geom {
    int N, H, W, C, tiles_h, tiles_w, sigmoid;
    long wsc, wsk;
};

DEVINL void c1_stage_weight(const float* __restrict__ w, float* wl, const C1Geom& g) {
    for (int i = threadIdx.x; i < 9 * g.C; i += 256) {
        const int c = i / 9, k = i - 9 * c;
        wl[i] = w[c * g.wsc + k * g.wsk];
    }
}

// NG > 0: a lane owns NG chunk positions of a pixel and keeps their 9 * EPC * NG weights in registers (at most 72: C = 32 in bf16
// and in fp32, the reference's head) -- the weight reads leave the LDS port, which they otherwise hold as long as the FMAs hold the
// VALU.  NG == 0: any C, weights read from LDS by every item.
template <typename T, int NG>
__global__ __launch_bounds__(256) void conv3x3_c1_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ bias, float* __restrict__ out, C1Geom g) {
    constexpr int EPC = ElemTraits<T>::EPC;
    __shared__ __attribute__((aligned(16))) float wl[C1_MAX_C * 9];
    __shared__ float part[C1_NPIX * 9];                                 // (stride 9: consecutive pixels fall on distinct banks)
    const int C = g.C, G = C / EPC;
    const int gs_log = (G % 4 == 0) ? 2 : (G % 2 == 0) ? 1 : 0, GS = 1 << gs_log;      // lanes per input pixel
    int b = blockIdx.x;
    const int tw = b % g.tiles_w;
    b /= g.tiles_w;
    const int th = b % g.tiles_h, n = b / g.tiles_h;
    const int h0 = th * C1_TH - 1, w0 = tw * C1_TW - 1;                 // origin of the input tile
    c1_stage_weight(w, wl, g);
    __syncthreads();
    float wr[NG > 0 ? NG * EPC * 9 : 1];
    if (NG > 0) {
        const int sub0 = threadIdx.x & (GS - 1);                        // (256 % GS == 0: a lane's chunk positions never change)
#pragma unroll
        for (int q = 0; q < NG; ++q)
#pragma unroll
            for (int i = 0; i < EPC * 9; ++i) wr[q * EPC * 9 + i] = wl[(sub0 + q * GS) * EPC * 9 + i];
    }
    const int items = C1_NPIX << gs_log;
    // the activation address of item `it` (null: outside the tile's items or the image)
    auto item_px = [&](int it) -> const T* {
        const int pix = it >> gs_log;
        const int ly = pix / C1_IW, lx = pix - ly * C1_IW;
        const int h = h0 + ly, ww = w0 + lx;
        return (it < items && h >= 0 && h < g.H && ww >= 0 && ww < g.W) ? x + (((size_t)n * g.H + h) * g.W + ww) * C : nullptr;
    };
    u32x4 nxt[NG > 0 ? NG : 1];
    const T* px_next = item_px(threadIdx.x);
    if (NG > 0 && px_next != nullptr) {
#pragma unroll
        for (int q = 0; q < NG; ++q) nxt[q] = ld_chunk(px_next + ((threadIdx.x & (GS - 1)) + q * GS) * EPC);
    }
    for (int base = 0; base < items; base += 256) {                     // (uniform trip count: the lane exchanges see whole waves)
        const int it = base + threadIdx.x;
        const int pix = it >> gs_log, sub = it & (GS - 1);
        const T* px = px_next;
        float acc[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[k] = 0.f;
        if (NG > 0) {
            u32x4 raw[NG > 0 ? NG : 1];
#pragma unroll
            for (int q = 0; q < NG; ++q) raw[q] = nxt[q];
            px_next = item_px(it + 256);                                // the next item's load is in flight during this item's FMAs
            if (px_next != nullptr) {
#pragma unroll
                for (int q = 0; q < NG; ++q) nxt[q] = ld_chunk(px_next + (sub + q * GS) * EPC);
            }
            if (px != nullptr) {
#pragma unroll
                for (int q = 0; q < NG; ++q) {
                    float xv[EPC];
                    Chunk<T>::unpack(raw[q], xv);
#pragma unroll
                    for (int j = 0; j < EPC; ++j)
#pragma unroll
                        for (int k = 0; k < 9; ++k) acc[k] = fmaf(xv[j], wr[(q * EPC + j) * 9 + k], acc[k]);
                }
            }
        } else {
            px_next = item_px(it + 256);
            if (px != nullptr) {
                for (int gi = sub; gi < G; gi += GS) {
                    float xv[EPC];
                    Chunk<T>::unpack(ld_chunk(px + gi * EPC), xv);
                    const float* wg = wl + gi * EPC * 9;
#pragma unroll
                    for (int j = 0; j < EPC; ++j)
#pragma unroll
                        for (int k = 0; k < 9; ++k) acc[k] = fmaf(xv[j], wg[j * 9 + k], acc[k]);
                }
            }
        }
        if (gs_log >= 1) {
#pragma unroll
            for (int k = 0; k < 9; ++k) acc[k] += __shfl_xor(acc[k], 1, 64);
        }
        if (gs_log >= 2) {
#pragma unroll
            for (int k = 0; k < 9; ++k) acc[k] += __shfl_xor(acc[k], 2, 64);
        }
        if (sub == 0 && it < items) {
#pragma unroll
            for (int k = 0; k < 9; ++k) part[pix * 9 + k] = acc[k];
        }
    }
    __syncthreads();
    const float bv = bias[0];
    for (int o = threadIdx.x; o < C1_TH * C1_TW; o += 256) {
        const int ty = o / C1_TW, tx = o - ty * C1_TW;
        const int h = th * C1_TH + ty, ww = tw * C1_TW + tx;
        if (h < g.H && ww < g.W) {
            float z = 0.f;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int s = 0; s < 3; ++s) z += part[((ty + r) * C1_IW + tx + s) * 9 + r * 3 + s];
            z += bv;
            out[((size_t)n * g.H + h) * g.W + ww] = g.sigmoid ? 1.f / (1.f + expf(-z)) : z;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256, 4) void conv3x3_c1_bwd_kernel(const T* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ p, const float* __restrict__ dout,
                                                             T* __restrict__ dx, float* __restrict__ ws, C1Geom g) {
    constexpr int EPC = ElemTraits<T>::EPC, NACC = EPC * 9;
    __shared__ __attribute__((aligned(16))) float wl[C1_MAX_C * 9];
    __shared__ float dzt[C1_ZH * C1_ZW];
    __shared__ float red[C1_PASS * C1_RED_LD];
    const int C = g.C, G = C / EPC;
    const int per = 256 / G, A = per * G;                               // active threads: whole pixels, a lane's chunk never changes
    int b = blockIdx.x;
    const int tw = b % g.tiles_w;
    b /= g.tiles_w;
    const int th = b % g.tiles_h, n = b / g.tiles_h;
    const int hb = th * C1_BH, wb = tw * C1_BW;
    const int twe = min(C1_BW, g.W - wb), the = min(C1_BH, g.H - hb);   // the tile's pixels inside the image
    c1_stage_weight(w, wl, g);
    for (int i = threadIdx.x; i < C1_ZH * (twe + 2); i += 256) {
        const int ly = i / (twe + 2), lx = i - ly * (twe + 2);
        const int h = hb - 1 + ly, ww = wb - 1 + lx;
        float v = 0.f;
        if (h >= 0 && h < g.H && ww >= 0 && ww < g.W) {
            const size_t at = ((size_t)n * g.H + h) * g.W + ww;
            v = dout[at];
            if (g.sigmoid) {
                const float pv = p[at];
                v = v * (pv * (1.f - pv));
            }
        }
        dzt[ly * C1_ZW + lx] = v;
    }
    __syncthreads();
    float acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = 0.f;
    float accb = 0.f;
    const int tid = threadIdx.x;
    if (tid < A) {
        const int gi = tid % G;
        const float* wg = wl + gi * NACC;
        const int npix = the * twe;
        for (int pix = tid / G; pix < npix; pix += per) {
            const int ty = pix / twe, tx = pix - ty * twe;
            float dzn[9];                                               // dzn[r * 3 + s] = dz[h + 1 - r][w + 1 - s]
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int s = 0; s < 3; ++s) dzn[r * 3 + s] = dzt[(ty + 2 - r) * C1_ZW + tx + 2 - s];
            const size_t at = ((((size_t)n * g.H + hb + ty) * g.W + wb + tx) * C) + gi * EPC;
            float xv[EPC];
            Chunk<T>::unpack(ld_chunk_nt(x + at), xv);
            if (gi == 0) accb += dzn[4];
#pragma unroll
            for (int j = 0; j < EPC; ++j)
#pragma unroll
                for (int k = 0; k < 9; ++k) acc[j * 9 + k] = fmaf(xv[j], dzn[k], acc[j * 9 + k]);
            if (dx != nullptr) {
                float dv[EPC];
#pragma unroll
                for (int j = 0; j < EPC; ++j) {
                    float s = 0.f;
#pragma unroll
                    for (int k = 0; k < 9; ++k) s = fmaf(dzn[k], wg[j * 9 + k], s);
                    dv[j] = s;
                }
                st_chunk(dx + at, Chunk<T>::pack(dv));
            }
        }
    }
    // fold the accumulators of the threads that own the same chunk, in thread order: C1_PASS values per pass through LDS
    const size_t row = (size_t)blockIdx.x * (9 * C + 1);
#pragma unroll
    for (int ps = 0; ps < NACC / C1_PASS; ++ps) {
        __syncthreads();
#pragma unroll
        for (int v = 0; v < C1_PASS; ++v) red[v * C1_RED_LD + tid] = acc[ps * C1_PASS + v];
        __syncthreads();
        for (int o = tid; o < G * C1_PASS; o += 256) {
            const int gg = o / C1_PASS, v = o - gg * C1_PASS;
            float s = 0.f;
            for (int t = gg; t < A; t += G) s += red[v * C1_RED_LD + t];
            ws[row + gg * NACC + ps * C1_PASS + v] = s;
        }
    }
    float sb[1] = {accb};
    block_sums<1>(sb, ws + row + 9 * C);
}

// second stage: out[o] (+)= sum over the workgroup rows in index order; 16 columns x 16 row groups per workgroup
__global__ __launch_bounds__(256) void conv3x3_c1_fold_kernel(const float* __restrict__ ws, int rows, int C, float* __restrict__ dw,
                                                              float* __restrict__ db, long wsc, long wsk, int accumulate) {
    __shared__ float part[16][17];
    const int ld = 9 * C + 1;
    const int ol = threadIdx.x & 15, ig = threadIdx.x >> 4;
    const int o = blockIdx.x * 16 + ol;
    float s = 0.f;
    if (o < ld)
        for (int i = ig; i < rows; i += 16) s += ws[(size_t)i * ld + o];
    part[ig][ol] = s;
    __syncthreads();
    if (ig == 0 && o < ld) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) t += part[i][ol];
        float* dst = nullptr;
        if (o < 9 * C) {
            const int c = o / 9, k = o - 9 * c;
            if (dw != nullptr) dst = dw + c * wsc + k * wsk;
        } else {
            dst = db;
        }
        if (dst != nullptr) *dst = accumulate ? *dst + t : t;
    }
}

int c1_geom(C1Geom& g, const char* what, int dtype, const void* x, int N, int H, int W, int C, long wsc, long wsk, int sigmoid,
            int th, int tw) {
    SAICV_REQUIRE(dtype == SAICV_DTYPE_BF16 || dtype == SAICV_DTYPE_F32, "%s: dtype %d is neither bf16 nor fp32", what, dtype);
    SAICV_REQUIRE(N > 0 && H > 0 && W > 0, "%s: empty problem", what);
    SAICV_REQUIRE(C >= 8 && C <= C1_MAX_C && C % 8 == 0, "%s: %d input channels; the kernel takes a multiple of 8 from 8 to %d", what,
                  C, C1_MAX_C);
    SAICV_REQUIRE(x != nullptr && ((uintptr_t)x & 15) == 0, "%s: the activation must start on a 16-byte boundary", what);
    g.N = N; g.H = H; g.W = W; g.C = C; g.sigmoid = sigmoid ? 1 : 0; g.wsc = wsc; g.wsk = wsk;
    g.tiles_h = (H + th - 1) / th;
    g.tiles_w = (W + tw - 1) / tw;
    SAICV_REQUIRE((size_t)N * g.tiles_h * g.tiles_w <= 0x7fffffffu, "%s: more than 2^31 - 1 tiles", what);
    return 0;
}

// ------------------------------------------------------------------------------------------------ mask statistics
constexpr int BSS_SPAN = 4096;                                          // elements of one sample per workgroup: 256 lanes x 4 x 4
constexpr float BSS_LO = 1e-4f, BSS_HI = 1.f - 1e-4f;                   // float32(1e-4), float32(1 - 1e-4): torch.clamp's bounds in fp32

DEVINL float bss_clamp(float p) { return p < BSS_LO ? BSS_LO : (p > BSS_HI ? BSS_HI : p); }    // (a NaN stays a NaN, as in torch.clamp)

DEVINL void bss_add(float p, float l, float (&s)[4]) {
    const float ph = bss_clamp(p);
    s[0] -= l * logf(ph) + (1.f - l) * logf(1.f - ph);
    s[1] += ph;
    s[2] += l;
    s[3] += ph * l;
}

// grid (blocks per sample, B): partial[b][blk][4]
__global__ __launch_bounds__(256) void bss_fwd_kernel(const float* __restrict__ prob, const float* __restrict__ label, size_t P,
                                                      int vec, float* __restrict__ partial) {
    const size_t off = (size_t)blockIdx.y * P, e0 = (size_t)blockIdx.x * BSS_SPAN;
    const size_t e1 = e0 + BSS_SPAN < P ? e0 + BSS_SPAN : P;
    const float* pp = prob + off;
    const float* ll = label + off;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec) {                                                          // P % 4 == 0 and aligned bases: whole 16-byte chunks
        for (size_t i = e0 + (size_t)threadIdx.x * 4; i < e1; i += 1024) {
            const f32x4 pv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(pp + i));
            const f32x4 lv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(ll + i));
#pragma unroll
            for (int j = 0; j < 4; ++j) bss_add(pv[j], lv[j], s);
        }
    } else {
        for (size_t i = e0 + threadIdx.x; i < e1; i += 256) bss_add(pp[i], ll[i], s);
    }
    block_sums<4>(s, partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4);
}

// one workgroup per sample: stats[b][j] = sum of partial[b][0 .. nblk)[j]
__global__ __launch_bounds__(256) void bss_fold_kernel(const float* __restrict__ partial, int nblk, float* __restrict__ stats) {
    const float total = fold_rows<4>(partial + (size_t)blockIdx.x * nblk * 4, nblk, 4);
    if (threadIdx.x < 4) stats[(size_t)blockIdx.x * 4 + threadIdx.x] = total;
}

DEVINL float bss_grad(float p, float l, float g0, float g1, float g3) {
    if (!(p >= BSS_LO && p <= BSS_HI)) return 0.f;                      // torch.clamp's backward, decided on the fp32 input
    return g0 * ((1.f - l) / (1.f - p) - l / p) + g1 + g3 * l;
}

__global__ __launch_bounds__(256) void bss_bwd_kernel(const float* __restrict__ prob, const float* __restrict__ label,
                                                      const float* __restrict__ gstats, size_t P, int vec, float* __restrict__ dprob) {
    const size_t off = (size_t)blockIdx.y * P, e0 = (size_t)blockIdx.x * BSS_SPAN;
    const size_t e1 = e0 + BSS_SPAN < P ? e0 + BSS_SPAN : P;
    const float g0 = gstats[blockIdx.y * 4 + 0], g1 = gstats[blockIdx.y * 4 + 1], g3 = gstats[blockIdx.y * 4 + 3];
    const float* pp = prob + off;
    const float* ll = label + off;
    float* dp = dprob + off;
    if (vec) {
        for (size_t i = e0 + (size_t)threadIdx.x * 4; i < e1; i += 1024) {
            const f32x4 pv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(pp + i));
            const f32x4 lv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(ll + i));
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = bss_grad(pv[j], lv[j], g0, g1, g3);
            *reinterpret_cast<f32x4*>(dp + i) = o;
        }
    } else {
        for (size_t i = e0 + threadIdx.x; i < e1; i += 256) dp[i] = bss_grad(pp[i], ll[i], g0, g1, g3);
    }
}

int bss_check(const char* what, const float* prob, const float* label, int B, size_t P) {
    SAICV_REQUIRE(prob != nullptr && label != nullptr, "%s: null input", what);
    SAICV_REQUIRE(B > 0 && B <= 65535 && P > 0, "%s: 1 to 65535 samples of at least one element", what);
    SAICV_REQUIRE((P + BSS_SPAN - 1) / BSS_SPAN <= 0x7fffffffu, "%s: too many elements per sample", what);
    return 0;
}

int bss_vec(const void* a, const void* b, const void* c, size_t P) {
    return P % 4 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

}  // namespace

namespace saicv {

extern "C" size_t saicv_conv3x3_c1_ws_floats(int N, int H, int W, int C) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
    return (size_t)N * ((H + C1_BH - 1) / C1_BH) * ((W + C1_BW - 1) / C1_BW) * (size_t)(9 * C + 1);
}

extern "C" int saicv_conv3x3_c1_fwd(int dtype, const void* x, const float* weight, long wsc, long wsk, const float* bias, float* out, int N, int H,
                                    int W, int C, int sigmoid, void* stream) {
    hipStream_t st = S(stream);
    C1Geom g;
    if (c1_geom(g, "conv3x3_c1_fwd", dtype, x, N, H, W, C, wsc, wsk, sigmoid, C1_TH, C1_TW)) return -1;
    SAICV_REQUIRE(weight != nullptr && bias != nullptr && out != nullptr, "conv3x3_c1_fwd: null weight, bias or output");
    const dim3 grid((unsigned)(N * g.tiles_h * g.tiles_w));
    // chunk positions per lane: G / lanes per pixel; 1 for bf16 at C = 8, 16, 32 and 2 for fp32 at C = 32 fit the register form
    if (dtype == SAICV_DTYPE_BF16) {
        if (C == 8 || C == 16 || C == 32)
            hipLaunchKernelGGL((conv3x3_c1_fwd_kernel<bf16_t, 1>), grid, dim3(256), 0, st, (const bf16_t*)x, weight, bias, out, g);
        else
            hipLaunchKernelGGL((conv3x3_c1_fwd_kernel<bf16_t, 0>), grid, dim3(256), 0, st, (const bf16_t*)x, weight, bias, out, g);
    } else {
        if (C == 8 || C == 16)
            hipLaunchKernelGGL((conv3x3_c1_fwd_kernel<float, 1>), grid, dim3(256), 0, st, (const float*)x, weight, bias, out, g);
        else if (C == 32)
            hipLaunchKernelGGL((conv3x3_c1_fwd_kernel<float, 2>), grid, dim3(256), 0, st, (const float*)x, weight, bias, out, g);
        else
            hipLaunchKernelGGL((conv3x3_c1_fwd_kernel<float, 0>), grid, dim3(256), 0, st, (const float*)x, weight, bias, out, g);
    }
    return check_launch("conv3x3_c1_fwd");
}

extern "C" int saicv_conv3x3_c1_bwd(int dtype, const void* x, const float* weight, long wsc, long wsk, const float* p, const float* dout, void* dx,
                                    float* dw, float* db, float* ws, int N, int H, int W, int C, int sigmoid, int accumulate, void* stream) {
    hipStream_t st = S(stream);
    C1Geom g;
    if (c1_geom(g, "conv3x3_c1_bwd", dtype, x, N, H, W, C, wsc, wsk, sigmoid, C1_BH, C1_BW)) return -1;
    SAICV_REQUIRE(weight != nullptr && dout != nullptr && ws != nullptr, "conv3x3_c1_bwd: null weight, gradient or workspace");
    SAICV_REQUIRE(!sigmoid || p != nullptr, "conv3x3_c1_bwd: the sigmoid form needs the saved output");
    SAICV_REQUIRE(((uintptr_t)dx & 15) == 0, "conv3x3_c1_bwd: the input gradient must start on a 16-byte boundary");
    const int rows = N * g.tiles_h * g.tiles_w;
    if (dtype == SAICV_DTYPE_BF16)
        hipLaunchKernelGGL(conv3x3_c1_bwd_kernel<bf16_t>, dim3(rows), dim3(256), 0, st, (const bf16_t*)x, weight, p, dout, (bf16_t*)dx,
                           ws, g);
    else
        hipLaunchKernelGGL(conv3x3_c1_bwd_kernel<float>, dim3(rows), dim3(256), 0, st, (const float*)x, weight, p, dout, (float*)dx, ws,
                           g);
    if (dw != nullptr || db != nullptr)
        hipLaunchKernelGGL(conv3x3_c1_fold_kernel, dim3((9 * C + 1 + 15) / 16), dim3(256), 0, st, ws, rows, C, dw, db, wsc, wsk,
                           accumulate ? 1 : 0);
    return check_launch("conv3x3_c1_bwd");
}

extern "C" size_t saicv_binary_seg_stats_ws_floats(int B, size_t P) {
    if (B <= 0 || P == 0) return 0;
    return (size_t)B * ((P + BSS_SPAN - 1) / BSS_SPAN) * 4;
}

extern "C" int saicv_binary_seg_stats_fwd(const float* prob, const float* label, int B, size_t P, float* partial, float* stats, void* stream) {
    hipStream_t st = S(stream);
    if (bss_check("binary_seg_stats_fwd", prob, label, B, P)) return -1;
    SAICV_REQUIRE(partial != nullptr && stats != nullptr, "binary_seg_stats_fwd: null workspace or output");
    const int nblk = (int)((P + BSS_SPAN - 1) / BSS_SPAN);
    hipLaunchKernelGGL(bss_fwd_kernel, dim3(nblk, B), dim3(256), 0, st, prob, label, P, bss_vec(prob, label, nullptr, P), partial);
    hipLaunchKernelGGL(bss_fold_kernel, dim3(B), dim3(256), 0, st, partial, nblk, stats);
    return check_launch("binary_seg_stats_fwd");
}

extern "C" int saicv_binary_seg_stats_bwd(const float* prob, const float* label, const float* gstats, int B, size_t P, float* dprob, void* stream) {
    hipStream_t st = S(stream);
    if (bss_check("binary_seg_stats_bwd", prob, label, B, P)) return -1;
    SAICV_REQUIRE(gstats != nullptr && dprob != nullptr, "binary_seg_stats_bwd: null gradient");
    const int nblk = (int)((P + BSS_SPAN - 1) / BSS_SPAN);
    hipLaunchKernelGGL(bss_bwd_kernel, dim3(nblk, B), dim3(256), 0, st, prob, label, gstats, P, bss_vec(prob, label, dprob, P), dprob);
    return check_launch("binary_seg_stats_bwd");
}

}  // namespace saicv
