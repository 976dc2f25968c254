// Backward of the ResNet stem behind BatchNorm + ReLU + MaxPool2d(3, 2, 1): BatchNorm-backward apply + weight gradient as ONE stream.
//
// Reference SimpleAICV/classification/backbones/resnet.py:172-184, 226-229: conv1 = ConvBnActBlock(3, 64, 7, stride 2, padding 3), then
// maxpool1.  The stem has no data gradient, so the gradient dy of its convolution output (411 MB at batch 256) has exactly one
// consumer, the weight gradient: bn_relu_maxpool_bwd_apply_k3s2_kernel (pool.hip) wrote it, igemm_tn_dma_kernel (igemm.hip) read it
// back.  Here a workgroup forms 32 pixels of dy in registers, parks them in LDS next to the 32 x 256 tap operand of the space-to-depth
// image and multiplies; dy never reaches memory.
//
// THE RESULTS ARE THOSE OF THE TWO KERNELS, BIT FOR BIT (deterministic mode), as csrc/c3bwd.hip keeps them for its layer:
//   * dy is k3s2_dy (poolbwd.h) -- the statement the apply kernel itself uses, rounded to bf16 by the same pack;
//   * the reduction rows are the output pixels in linear (n, oh, ow) order, consumed in 32-row steps of the 16 x 16 x 32 bf16 MFMA, one
//     accumulator chain per output element, dy as the first operand, both operands read transposed from LDS images swizzled as
//     igemm_tn_dma_kernel's; workgroup s takes the CONSECUTIVE rows of split s of igemm_tn's plan for the same product (tn_plan through
//     igemm_plan) and hands its [64][256] partial to saicv::DetParts as part s: the same chains, the same fold;
//   * rows past the split's end are zero in both operands, as that kernel's out-of-range loads are.
// A thread owns one 16-byte chunk of dy per step (pixel tid / 8, channels 8 (tid % 8) ..) and the 64 contiguous bytes of the tap
// operand next to it (tap row (tid % 8) / 2, two of its four columns): 32 consecutive pixels share their taps, so the image is read
// from HBM once and the rest are cache hits.  Two steps of loads are in flight in registers; the LDS images are double-buffered, one
// barrier per step.
#include <stdlib.h>

#include <type_traits>

#include "common.h"
#include "det.h"
#include "poolbwd.h"
#include "saicv_internal.h"
#include "../../include/saicv_hip.h"

namespace {

constexpr int kCO = 64, kKd = 256, kCQ = 16, kTaps = 4, kStep = 32;

struct StemParams {
    const bf16_t* dout;         // [N][PH][PW][64] gradient of the pooled output
    const uint8_t* idx;         // [N][PH][PW][64] window position of the recorded maximum
    const bf16_t* y;            // [N][H][W][64] convolution output
    const bf16_t* x;            // [N][H + 3][W + 3][16] space-to-depth image
    const float* gamma;
    const float* mean;
    const float* invstd;
    const float* scale;
    const float* shift;
    const float* sums;          // [2][64]: sum g, sum g * xhat
    float* dw;                  // [64][4][4][16], accumulated into
    float* dgamma;
    float* dbeta;
    int accumulate;
    saicv::DetSink det;
    uint32_t y_bytes, dout_bytes, x_bytes;
    int M, m_per_split, Nimg, H, W, PH, PW;
};

template <int B, int E, typename F> DEVINL void static_for(F&& f) {
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        static_for<B + 1, E>(f);
    }
}
// swizzle of the transposed-read images (igemm.hip, igemm_tn_dma_kernel): the 32-byte pair p of row r lives at pair slot p ^ g(r)
DEVINL int st_key(int r) { return (r & 3) | (((r >> 3) & 1) << 2); }
template <int CPR> DEVINL int st_g(int r) { return CPR >= 16 ? st_key(r) : (st_key(r) >> 1); }

__global__ __launch_bounds__(256) void stem_bwd_stream_kernel(const StemParams p) {
    constexpr int DEPTH = 2;                      // steps in flight in registers
    constexpr int N = 8;
    constexpr int A_BYTES = kStep * kCO * 2, B_BYTES = kStep * kKd * 2, STAGE = A_BYTES + B_BYTES;
    constexpr int PA = kCO * 2, PB = kKd * 2;     // row pitches of the two images
    constexpr uint32_t OOB = 0xfffffff0u;
    typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    const int row = tid >> 3, cb = tid & 7;       // this thread's pixel of a step and its channel chunk / tap slice
    const int tr = cb >> 1, ts = (cb & 1) * 2;    // tap row, first of its two tap columns

    const int m_begin = (int)blockIdx.x * p.m_per_split;
    const int m_end = min(p.M, m_begin + p.m_per_split);
    const int nt = m_begin < m_end ? (m_end - m_begin + kStep - 1) / kStep : 0;

    // ---- per-channel coefficients of dy, as the apply kernel forms them
    const float inv_m = 1.f / ((float)p.Nimg * (float)p.H * (float)p.W);
    float sc[N], sh[N], mu[N], is[N], k0[N], mg[N], mx[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int c = cb * N + j;
        sc[j] = p.scale[c]; sh[j] = p.shift[c]; mu[j] = p.mean[c]; is[j] = p.invstd[c];
        k0[j] = p.gamma[c] * is[j];
        mg[j] = p.sums[c] * inv_m;
        mx[j] = p.sums[kCO + c] * inv_m;
    }
    if (blockIdx.x == 0 && tid < kCO) {
        if (p.accumulate) { p.dbeta[tid] += p.sums[tid]; p.dgamma[tid] += p.sums[kCO + tid]; }
        else { p.dbeta[tid] = p.sums[tid]; p.dgamma[tid] = p.sums[kCO + tid]; }
    }

    const __amdgpu_buffer_rsrc_t y_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(p.y), 0, p.y_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t d_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(p.dout), 0, p.dout_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t i_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.idx), 0, p.dout_bytes / 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t x_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(p.x), 0, p.x_bytes, 0x00020000);

    // one step's operands in registers.  A row past the split's end reads zeros (buffer bounds) and its dy is zeroed as well
    struct Slot { u32x4 y, d[4], x[4]; u32x2 ix[4]; int meta; };
    Slot slot[DEPTH];
    const int hw = p.H * p.W, HQ = p.H + kTaps - 1, WQ = p.W + kTaps - 1;
    auto load_step = [&](Slot& s, int i) __attribute__((always_inline)) {
        const int m = m_begin + i * kStep + row;
        const bool ok = i < nt && m < m_end;
        const int mm = ok ? m : 0;
        const int n = mm / hw, rem = mm - n * hw;
        const int h = rem / p.W, w = rem - h * p.W;
        const int a = h >> 1, b = w >> 1;
        s.meta = (h & 1) | ((w & 1) << 1) | ((a + 1 < p.PH) ? 4 : 0) | ((b + 1 < p.PW) ? 8 : 0) | (ok ? 16 : 0);
        s.y = __builtin_amdgcn_raw_buffer_load_b128(y_rs, (int)(ok ? ((uint32_t)mm * kCO + cb * N) * 2u : OOB), 0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {             // the four windows (a + dy, b + dx); one that does not exist is fetched clamped and ignored
            const int ph = min(a + (q >> 1), p.PH - 1), pw = min(b + (q & 1), p.PW - 1);
            const uint32_t o = (uint32_t)((n * p.PH + ph) * p.PW + pw) * kCO + cb * N;
            s.d[q] = __builtin_amdgcn_raw_buffer_load_b128(d_rs, (int)(ok ? o * 2u : OOB), 0, 0);
            s.ix[q] = __builtin_amdgcn_raw_buffer_load_b64(i_rs, (int)(ok ? o : OOB), 0, 0);
        }
        const uint32_t xo = (uint32_t)((n * HQ + h + tr) * WQ + w + ts) * (kCQ * 2u);
#pragma unroll
        for (int k = 0; k < 4; ++k) s.x[k] = __builtin_amdgcn_raw_buffer_load_b128(x_rs, (int)(ok ? xo + k * 16 : OOB), 0, 0);
    };
#pragma unroll
    for (int dd = 0; dd < DEPTH; ++dd) load_step(slot[dd], dd);

    // wavefront w multiplies all 64 dy channels with the reduction columns 64 w .. 64 w + 63
    f32x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    // transposed fragment reads: lane (column l15, k-group lg) gets rows lg * 8 .. + 7 of its column (two reads of four rows)
    const int row0 = lg * 8 + (l15 >> 2);
    int fa_off[4], fb_off[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) fa_off[a] = row0 * PA + ((a ^ st_g<8>(row0)) << 5) + (l15 & 3) * 8;
#pragma unroll
    for (int b = 0; b < 4; ++b) fb_off[b] = A_BYTES + row0 * PB + (((wave * 4 + b) ^ st_g<32>(row0)) << 5) + (l15 & 3) * 8;
    const int wa_off = row * PA + ((cb ^ (st_g<8>(row) << 1)) << 4);
    int wb_off[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) wb_off[k] = A_BYTES + row * PB + (((cb * 4 + k) ^ (st_g<32>(row) << 1)) << 4);

    // One step of slot D (a compile-time index: the slots are registers)
    auto step = [&](auto D, int i) __attribute__((always_inline)) {
        constexpr int d = decltype(D)::value;
        Slot& s = slot[d];
        char* const st = smem + (i & 1) * STAGE;
        {
            float yv[N], dv[4][N];
            uint8_t ib[4][N];
            bool use[4];
            int want[4];
            Chunk<bf16_t>::unpack(s.y, yv);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                Chunk<bf16_t>::unpack(s.d[q], dv[q]);
                __builtin_memcpy(ib[q], &s.ix[q], 8);
                const bool wok = (q < 2 || (s.meta & 4)) && (!(q & 1) || (s.meta & 8));
                use[q] = k3s2_window(s.meta & 1, (s.meta >> 1) & 1, q, wok, want[q]);
            }
            u32x4 dy = k3s2_dy<bf16_t>(yv, dv, ib, use, want, sc, sh, k0, mg, mu, is, mx);
            if (!(s.meta & 16)) dy = u32x4{0u, 0u, 0u, 0u};
            *reinterpret_cast<u32x4*>(st + wa_off) = dy;
#pragma unroll
            for (int k = 0; k < 4; ++k) *reinterpret_cast<u32x4*>(st + wb_off[k]) = s.x[k];
        }
        load_step(s, i + DEPTH);                      // the slot is free again: DEPTH steps ahead
        __syncthreads();                              // both images of this step are written (the other stage is the previous step's)
        u32x4 af[4], bf[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const bf16x4 l4 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(st + fa_off[a]));
            const bf16x4 h4 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(st + fa_off[a] + 4 * PA));
            const u32x2 l2 = __builtin_bit_cast(u32x2, l4), h2 = __builtin_bit_cast(u32x2, h4);
            af[a] = u32x4{l2[0], l2[1], h2[0], h2[1]};
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const bf16x4 l4 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(st + fb_off[b]));
            const bf16x4 h4 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(st + fb_off[b] + 4 * PB));
            const u32x2 l2 = __builtin_bit_cast(u32x2, l4), h2 = __builtin_bit_cast(u32x2, h4);
            bf[b] = u32x4{l2[0], l2[1], h2[0], h2[1]};
        }
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int a = 0; a < 4; ++a) Mma<bf16_t>::run(acc[a][b], af[a], bf[b]);
    };
    int i0 = 0;
    for (; i0 + DEPTH <= nt; i0 += DEPTH) static_for<0, DEPTH>([&](auto D) { step(D, i0 + decltype(D)::value); });
    static_for<0, DEPTH - 1>([&](auto D) {
        if (i0 + decltype(D)::value < nt) step(D, i0 + decltype(D)::value);      // uniform over the workgroup
    });

    // ---- this split's partial: D row -> dy channel, D column -> reduction column (every element, zeros included)
    if (nt == 0) return;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const size_t e = (size_t)(a * 16 + lg * 4 + r) * kKd + (wave * 4 + b) * 16 + l15;
                saicv::det_add(p.det, p.dw + e, e, (int)blockIdx.x, acc[a][b][r]);
            }
}

// Buffer-addressed operands stay below 4 GiB (the clamped rows of the last step included)
bool stem_fits(int N, int H, int W) {
    const size_t m = (size_t)N * H * W;
    return (m + kStep) * kCO * 2 < 0xfffffff0ull && (size_t)N * (H + kTaps - 1) * (W + kTaps - 1) * kCQ * 2 < 0xfffffff0ull;
}

// splits (= workgroups = parts of the weight gradient) and rows per split: igemm_tn's plan for the same product
int stem_plan(int N, int H, int W, int* splits, int* m_per_split) {
    saicv_plan_query q = {};
    q.op = SAICV_PLAN_CONV_WGRAD;
    q.conv.N = N; q.conv.H = H + kTaps - 1; q.conv.W = W + kTaps - 1; q.conv.C = kCQ; q.conv.K = kCO; q.conv.R = kTaps; q.conv.S = kTaps;
    q.conv.stride = 1; q.conv.pad = 0; q.conv.OH = H; q.conv.OW = W; q.conv.dtype = SAICV_BF16;
    saicv_plan pl;
    if (saicv::igemm_plan(&q, &pl) != 0) return -1;
    SAICV_REQUIRE(pl.splits >= 1 && (pl.rt_per * pl.rows_per_step) % kStep == 0, "stem_bwd_stream: weight-gradient plan with %d splits of %d x %d rows",
                  pl.splits, pl.rt_per, pl.rows_per_step);
    *splits = pl.splits;
    *m_per_split = pl.rt_per * pl.rows_per_step;
    return 0;
}

}  // namespace

namespace saicv {

// Has the launch a form for this block (no switches)?  bf16, 64 output channels, a K x K stride-2 stem as taps x taps over the
// cq-channel space-to-depth image, MaxPool2d(3, 2, 1) behind it, operands below 4 GiB.
bool stem_bwd_stream_supported(int dtype, int N, int H, int W, int CO, int cq, int taps_r, int taps_s, int pk, int ps, int pp) {
    if (dtype != SAICV_DTYPE_BF16 || N < 1 || H < 1 || W < 1) return false;
    if (CO != kCO || cq != kCQ || taps_r != kTaps || taps_s != kTaps || pk != 3 || ps != 2 || pp != 1) return false;
    return stem_fits(N, H, W);
}

// Which parts of the streamed backward the block takes: 0 none; bit 0: the forward keeps the maxima and the two sums come from them
// (pool.hip); bit 1: stem_bwd_stream_kernel replaces the apply pass and the weight gradient.  A pure function of its arguments and of
// SAICV_STEM_BWD_STREAM / SAICV_STEM_BWD_MIN_ROWS (default 65536), read per call.
// routed: bit 0.  The stream kernel is built and tested but stays unrouted by default (SAICV_STEM_BWD_STREAM=2 takes it): one
// wavefront per SIMD forms dy AND multiplies, and forming a pixel chunk costs ~300 vector instructions -- 566 us per launch against
// the 370 us of the two kernels it replaces (profiles/stem_bwd_stream.md).
extern "C" int saicv_stem_bwd_stream_ok(int dtype, int N, int H, int W, int CO, int cq, int taps_r, int taps_s, int pk, int ps, int pp) {
    const char* es = getenv("SAICV_STEM_BWD_STREAM");
    const char* er = getenv("SAICV_STEM_BWD_MIN_ROWS");
    const int mode = es ? atoi(es) : 1;
    const int min_rows = er ? atoi(er) : 65536;
    if (mode <= 0 || !stem_bwd_stream_supported(dtype, N, H, W, CO, cq, taps_r, taps_s, pk, ps, pp)) return 0;
    const size_t m = (size_t)N * H * W;
    if (m < (size_t)(min_rows > 1 ? min_rows : 1)) return 0;
    return mode >= 2 ? 3 : 1;
}

// Workspace floats of the launch: in the fast mode the weight-gradient parts (parked and folded in BOTH modes, as c3_bwd_stream's are)
extern "C" size_t saicv_stem_bwd_stream_ws_floats(int N, int H, int W) {
    int splits = 0, mps = 0;
    if (!g_deterministic && N >= 1 && H >= 1 && W >= 1 && stem_fits(N, H, W) && stem_plan(N, H, W, &splits, &mps) == 0 && splits > 1)
        return (size_t)splits * kCO * kKd;
    return 1;
}

int stem_bwd_stream(const void* dout, const uint8_t* idx, const void* y, const float* gamma, const float* mean, const float* invstd,
                    const float* scale, const float* shift, const float* sums, const void* x, float* dw, float* dgamma, float* dbeta,
                    int accumulate, float* part_ws, int N, int H, int W, hipStream_t st) {
    SAICV_REQUIRE(dout && idx && y && gamma && mean && invstd && scale && shift && sums && x && dw && dgamma && dbeta,
                  "stem_bwd_stream: operand missing");
    StemParams p = {};
    p.dout = (const bf16_t*)dout; p.idx = idx; p.y = (const bf16_t*)y; p.x = (const bf16_t*)x;
    p.gamma = gamma; p.mean = mean; p.invstd = invstd; p.scale = scale; p.shift = shift; p.sums = sums;
    p.dw = dw; p.dgamma = dgamma; p.dbeta = dbeta; p.accumulate = accumulate;
    p.Nimg = N; p.H = H; p.W = W; p.PH = (H + 1) / 2; p.PW = (W + 1) / 2;
    p.M = N * H * W;
    p.y_bytes = (uint32_t)((size_t)p.M * kCO * 2);
    p.dout_bytes = (uint32_t)((size_t)N * p.PH * p.PW * kCO * 2);
    p.x_bytes = (uint32_t)((size_t)N * (H + kTaps - 1) * (W + kTaps - 1) * kCQ * 2);
    int splits = 0;
    if (stem_plan(N, H, W, &splits, &p.m_per_split) != 0) return -1;
    DetParts parts;
    if (parts.begin(st, splits, (size_t)kCO * kKd, "stem_bwd_stream", false) != 0) return -1;      // every split writes its whole part
    if (!parts.on() && splits > 1) {                  // fast mode: the parts go to the caller's workspace, the same fold
        SAICV_REQUIRE(part_ws != nullptr, "stem_bwd_stream: workspace for the weight-gradient parts missing");
        parts.s.part = part_ws;
    }
    p.det = parts.sink();
    hipLaunchKernelGGL(stem_bwd_stream_kernel, dim3(splits), dim3(256), 0, st, p);
    if (check_launch("stem_bwd_stream") != 0) return -1;
    if (parts.fold(dw, 0, (size_t)kCO * kKd, true) != 0) return -1;
    return 0;
}

}  // namespace saicv
