// One bidirectional LSTM layer's recurrence, forward and backward (nn.LSTM: one layer, batch_first, zero initial state, gate
// order i, f, g, o).  The input projection x W_ih^T + b_ih + b_hh and every parameter / input gradient are GEMMs on igemm.hip;
// these two kernels do only what cannot be a GEMM: the walk over T.
//
// A workgroup owns one direction and 16 batch rows (one MFMA M tile) and walks all T steps alone: no workgroup waits on another,
// every loop is bounded by T, there are no atomics.  Each of the 8 waves owns hidden-column slices of 16 (slice = wave + 8 n); for
// a slice it computes the i, f, g and o tiles, which share the accumulator lane layout, so the gate math is in-lane fp32 and the
// cell state (forward) / dh and dc (backward) never leave their registers.  W_hh is streamed from L2 once per step: a lane's B
// fragment is 16 contiguous bytes of one row ([4H][H] forward, the transposed [H][4H] backward), straight to registers, the next
// group of chunks issued before the MFMAs of the current one; the caller hands the weights over in fragment order (stream_dot), a
// copy it makes once per call.  The A operand (h_{t-1}, 16 x H; dgates_t, 16 x 4H) sits in LDS.
#include "common.h"
#include "saicv_internal.h"
#include "../../include/saicv_hip.h"

namespace saicv {
namespace {

constexpr int LSTM_ROWS = 16;        // batch rows of a workgroup
constexpr int LSTM_WAVES = 8;
constexpr int LSTM_THREADS = LSTM_WAVES * 64;
constexpr int LSTM_PAD = 16;         // bytes behind every LDS row: the 16 rows of a fragment read start on distinct banks
constexpr int LSTM_LDS_MAX = 160 * 1024;

DEVINL float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

// acc[g] += A[16 x K] * W_g^T for the G gates of one 16-column slice.  a: this lane's A row + its k-group's 16 bytes.  w: the
// slice's weights in FRAGMENT ORDER, [k chunk][gate][lane][16 bytes] (+ this lane's 16 bytes): what one load instruction of the wave
// reads is one contiguous KiB.  (Read from the row-major matrix, a fragment is 16 rows x 64 bytes at a row stride of H or 4H
// elements -- a power-of-two stride at the workload's H, which parks all 16 rows on a few L2 channels.)  nk chunks of 64 bytes of K
// per row (32 bf16 / 16 fp32).
template <typename T, int G, int KU>
DEVINL void stream_dot(f32x4 (&acc)[G], const char* a, const char* w, int nk) {
    const int groups = nk / KU;
    u32x4 wn[G][KU];
    if (groups > 0) {
#pragma unroll
        for (int u = 0; u < KU; ++u)
#pragma unroll
            for (int g = 0; g < G; ++g) wn[g][u] = ld_chunk(w + (size_t)(u * G + g) * 1024);
    }
    for (int i = 0; i < groups; ++i) {
        u32x4 wc[G][KU], av[KU];
#pragma unroll
        for (int u = 0; u < KU; ++u)
#pragma unroll
            for (int g = 0; g < G; ++g) wc[g][u] = wn[g][u];
        if (i + 1 < groups) {
#pragma unroll
            for (int u = 0; u < KU; ++u)
#pragma unroll
                for (int g = 0; g < G; ++g) wn[g][u] = ld_chunk(w + (size_t)(((i + 1) * KU + u) * G + g) * 1024);
        }
#pragma unroll
        for (int u = 0; u < KU; ++u) av[u] = ld_chunk(a + (size_t)(i * KU + u) * 64);
#pragma unroll
        for (int u = 0; u < KU; ++u)
#pragma unroll
            for (int g = 0; g < G; ++g) Mma<T>::run(acc[g], av[u], wc[g][u]);
    }
    for (int kc = groups * KU; kc < nk; ++kc) {
        u32x4 wc[G];
#pragma unroll
        for (int g = 0; g < G; ++g) wc[g] = ld_chunk(w + (size_t)(kc * G + g) * 1024);
        const u32x4 av = ld_chunk(a + (size_t)kc * 64);
#pragma unroll
        for (int g = 0; g < G; ++g) Mma<T>::run(acc[g], av, wc[g]);
    }
}

// gates [B * T][8H] fp32: on entry the pre-activations x W_ih^T + b of both directions (direction-major columns, i f g o inside), on
// exit the activated gates, written in place by the lane that read them.  y [B][T][2H] = h_t in T; cs [B][T][2H] = c_t fp32.
// whh [2][H / 16][nk][4 gates][64 lanes][16 bytes]: lane l of slice s, chunk k, gate g holds W_hh[g H + 16 s + (l & 15)][k-th 64
// bytes of the row, 16-byte piece l >> 4].
template <typename T, int NSL>
__global__ __launch_bounds__(LSTM_THREADS) void lstm_fwd_kernel(float* __restrict__ gates, const T* __restrict__ whh, T* __restrict__ y,
                                                                float* __restrict__ cs, int B, int Tn, int H) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // workgroups go round-robin over the 8 XCDs by blockIdx.x % 8: the direction from that residue, so one L2 holds one direction's weights
    const int dir = blockIdx.x & 1, tile = blockIdx.x >> 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int nct = H >> 4;
    const int rowbytes = H * (int)sizeof(T) + LSTM_PAD;
    const int bufbytes = LSTM_ROWS * rowbytes;
    const int nk = H * (int)sizeof(T) / 64;
    const size_t H8 = (size_t)8 * H, H2 = (size_t)2 * H;
    const char* w = reinterpret_cast<const char*>(whh + (size_t)dir * 4 * H * H);

    for (int i = threadIdx.x * 16; i < bufbytes; i += LSTM_THREADS * 16) st_chunk(smem + i, zero_chunk());      // h_{-1} = 0
    __syncthreads();

    size_t brow[4];
    bool bok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int b = tile * LSTM_ROWS + fq * 4 + j;
        bok[j] = b < B;
        brow[j] = (size_t)(b < B ? b : B - 1) * Tn;
    }
    f32x4 c[NSL];
#pragma unroll
    for (int sl = 0; sl < NSL; ++sl) c[sl] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int s = 0; s < Tn; ++s) {
        const int t = dir ? Tn - 1 - s : s;
        const char* hin = smem + (s & 1) * bufbytes;
        char* hout = smem + ((s + 1) & 1) * bufbytes;
#pragma unroll
        for (int sl = 0; sl < NSL; ++sl) {
            const int ct = wave + sl * LSTM_WAVES;
            if (ct < nct) {
                int col = ct * 16 + fr;
                asm volatile("" : "+v"(col));             // addresses are rebuilt per step, not kept live per slice across the walk
                float gx[4][4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int g = 0; g < 4; ++g) gx[g][j] = __builtin_nontemporal_load(gates + (brow[j] + t) * H8 + (size_t)(dir * 4 + g) * H + col);
                f32x4 acc[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
                // (eight slices per wave leave registers for two chunks per gate in flight, fewer slices for four)
                stream_dot<T, 4, (NSL <= 4 ? 4 : 2)>(acc, hin + fr * rowbytes + fq * 16,
                                                     w + (size_t)(col >> 4) * nk * 4096 + lane * 16, nk);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float gi = sigmoid_f(acc[0][j] + gx[0][j]);
                    const float gf = sigmoid_f(acc[1][j] + gx[1][j]);
                    const float gg = tanhf(acc[2][j] + gx[2][j]);
                    const float go = sigmoid_f(acc[3][j] + gx[3][j]);
                    const float cn = gf * c[sl][j] + gi * gg;
                    c[sl][j] = cn;
                    const T hv = from_f32<T>(go * tanhf(cn));
                    // the value fed back is the value stored: y[t] is h_t bit for bit
                    *reinterpret_cast<T*>(hout + (fq * 4 + j) * rowbytes + col * (int)sizeof(T)) = hv;
                    if (bok[j]) {
                        float* gp = gates + (brow[j] + t) * H8 + (size_t)(dir * 4) * H + col;
                        // gates, c and y pass through once: nontemporal, so that W_hh keeps its place in L2
                        __builtin_nontemporal_store(gi, gp);
                        __builtin_nontemporal_store(gf, gp + (size_t)H);
                        __builtin_nontemporal_store(gg, gp + (size_t)2 * H);
                        __builtin_nontemporal_store(go, gp + (size_t)3 * H);
                        __builtin_nontemporal_store(cn, cs + (brow[j] + t) * H2 + (size_t)dir * H + col);
                        y[(brow[j] + t) * H2 + (size_t)dir * H + col] = hv;
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);          // one slice at a time: loads of the next do not pile onto this one's registers
        }
        __syncthreads();
    }
}

// Walks T against the direction's order with dh and dc in registers.  dgates [B * T][8H] in T: the pre-activation gradients, written
// per step and fed, as stored, to dh_{t-1} = dgates_t W_hh.  whhT is W_hh transposed ([H][4H], so a B fragment is again 16
// contiguous bytes of one row) in fragment order: [2][H / 16][nk][64 lanes][16 bytes].  A_LDS: dgates_t also goes to LDS (nbuf tiles of 16 x 4H) and is read from there; else (fp32,
// H >= 640: the tile does not fit) it is read back from the global rows this workgroup wrote before the barrier.
template <typename T, int NSL, bool A_LDS>
__global__ __launch_bounds__(LSTM_THREADS) void lstm_bwd_kernel(const T* __restrict__ dy, const float* __restrict__ acts,
                                                                const float* __restrict__ cs, const T* __restrict__ whhT, T* dgates,
                                                                int B, int Tn, int H, int nbuf) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int dir = blockIdx.x & 1, tile = blockIdx.x >> 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int nct = H >> 4;
    const int rowbytes = 4 * H * (int)sizeof(T) + LSTM_PAD;
    const int bufbytes = LSTM_ROWS * rowbytes;
    const int nk = 4 * H * (int)sizeof(T) / 64;
    const size_t H8 = (size_t)8 * H, H2 = (size_t)2 * H;
    const char* w = reinterpret_cast<const char*>(whhT + (size_t)dir * 4 * H * H);

    size_t brow[4];
    bool bok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int b = tile * LSTM_ROWS + fq * 4 + j;
        bok[j] = b < B;
        brow[j] = (size_t)(b < B ? b : B - 1) * Tn;
    }
    const int ba = tile * LSTM_ROWS + fr;                                   // the batch row of this lane's A fragment
    const size_t arow = (size_t)(ba < B ? ba : B - 1) * Tn;
    f32x4 dhc[NSL], dcc[NSL];
#pragma unroll
    for (int sl = 0; sl < NSL; ++sl) dhc[sl] = dcc[sl] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int s = 0; s < Tn; ++s) {
        const int t = dir ? s : Tn - 1 - s;
        const int tp = dir ? t + 1 : t - 1;                                 // the step before t in the direction's order
        const bool first = s == Tn - 1;                                     // t is the direction's first step: c_{t-1} = 0, no carry out
        char* buf = smem + (nbuf == 2 ? (s & 1) * bufbytes : 0);
#pragma unroll
        for (int sl = 0; sl < NSL; ++sl) {
            const int ct = wave + sl * LSTM_WAVES;
            if (ct < nct) {
                int col = ct * 16 + fr;
                asm volatile("" : "+v"(col));             // addresses are rebuilt per step, not kept live per slice across the walk
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const size_t r = brow[j] + t;
                    const float* ap = acts + r * H8 + (size_t)(dir * 4) * H + col;
                    const float gi = __builtin_nontemporal_load(ap), gf = __builtin_nontemporal_load(ap + (size_t)H),
                                gg = __builtin_nontemporal_load(ap + (size_t)2 * H), go = __builtin_nontemporal_load(ap + (size_t)3 * H);
                    const float cn = cs[r * H2 + (size_t)dir * H + col];
                    const float cp = first ? 0.f : cs[(brow[j] + tp) * H2 + (size_t)dir * H + col];
                    const float dh = to_f32(dy[r * H2 + (size_t)dir * H + col]) + dhc[sl][j];
                    const float tc = tanhf(cn);
                    const float dc = dcc[sl][j] + dh * go * (1.f - tc * tc);
                    dcc[sl][j] = dc * gf;
                    const T vi = from_f32<T>(dc * gg * gi * (1.f - gi));
                    const T vf = from_f32<T>(dc * cp * gf * (1.f - gf));
                    const T vg = from_f32<T>(dc * gi * (1.f - gg * gg));
                    const T vo = from_f32<T>(dh * tc * go * (1.f - go));
                    if (A_LDS) {
                        T* lp = reinterpret_cast<T*>(buf + (fq * 4 + j) * rowbytes) + col;
                        lp[0] = vi;
                        lp[H] = vf;
                        lp[2 * H] = vg;
                        lp[3 * H] = vo;
                    }
                    if (bok[j]) {
                        T* gp = dgates + r * H8 + (size_t)(dir * 4) * H + col;
                        gp[0] = vi;
                        gp[(size_t)H] = vf;
                        gp[(size_t)2 * H] = vg;
                        gp[(size_t)3 * H] = vo;
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();                                                    // dgates_t is complete: in LDS, or in the rows of this workgroup
        if (!first) {
            const char* a = A_LDS ? buf + fr * rowbytes + fq * 16
                                  : reinterpret_cast<const char*>(dgates + (arow + t) * H8 + (size_t)(dir * 4) * H) + fq * 16;
#pragma unroll
            for (int sl = 0; sl < NSL; ++sl) {
                const int ct = wave + sl * LSTM_WAVES;
                if (ct < nct) {
                    int col = ct * 16 + fr;
                    asm volatile("" : "+v"(col));
                    f32x4 acc[1];
                    acc[0] = f32x4{0.f, 0.f, 0.f, 0.f};
                    stream_dot<T, 1, 8>(acc, a, w + (size_t)(col >> 4) * nk * 1024 + lane * 16, nk);
                    dhc[sl] = acc[0];
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (A_LDS && nbuf == 1) __syncthreads();                            // one tile only: every wave has read it before the next step writes
    }
}

int lstm_check(const char* who, int dtype, int B, int Tn, int H) {
    SAICV_REQUIRE(dtype == SAICV_DTYPE_BF16 || dtype == SAICV_DTYPE_F32, "%s: dtype %d", who, dtype);
    SAICV_REQUIRE(B >= 1 && Tn >= 1, "%s: batch %d, %d steps", who, B, Tn);
    SAICV_REQUIRE(H >= 32 && H <= 1024 && H % 32 == 0, "%s: hidden size %d; a multiple of 32 in 32 .. 1024", who, H);
    SAICV_REQUIRE((long long)((B + LSTM_ROWS - 1) / LSTM_ROWS) * 2 <= 0x7fffffffLL, "%s: batch %d", who, B);
    return 0;
}

int lstm_slices(int H) {                 // hidden-column slices of a wave, rounded up to a built form
    const int need = ((H >> 4) + LSTM_WAVES - 1) / LSTM_WAVES;
    return need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : 8;
}

template <typename K>
void lstm_allow_lds(K k) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, LSTM_LDS_MAX);
}
}  // namespace

extern "C" int saicv_lstm_fwd(int dtype, float* gates, const void* whh, void* y, float* c, int B, int Tn, int H, void* stream) {
    hipStream_t s = S(stream);
    if (lstm_check("lstm_fwd", dtype, B, Tn, H)) return -1;
    SAICV_REQUIRE(gates && whh && y && c, "lstm_fwd: null gates, weights, output or cell state");
    const size_t esz = dtype == SAICV_DTYPE_BF16 ? 2 : 4;
    const size_t smem = 2 * LSTM_ROWS * ((size_t)H * esz + LSTM_PAD);
    SAICV_REQUIRE(smem <= (size_t)LSTM_LDS_MAX, "lstm_fwd: hidden size %d needs %zu bytes of LDS", H, smem);
    const dim3 grid(2 * ((B + LSTM_ROWS - 1) / LSTM_ROWS));
#define LSTM_FWD(T, N)                                                                                                     \
    do {                                                                                                                   \
        static bool once = (lstm_allow_lds(lstm_fwd_kernel<T, N>), true);                                                  \
        (void)once;                                                                                                        \
        hipLaunchKernelGGL((lstm_fwd_kernel<T, N>), grid, dim3(LSTM_THREADS), smem, s, gates, (const T*)whh, (T*)y, c, B, Tn, H); \
    } while (0)
#define LSTM_FWD_N(T)                        \
    switch (lstm_slices(H)) {                \
        case 1: LSTM_FWD(T, 1); break;       \
        case 2: LSTM_FWD(T, 2); break;       \
        case 4: LSTM_FWD(T, 4); break;       \
        default: LSTM_FWD(T, 8); break;      \
    }
    if (dtype == SAICV_DTYPE_BF16) LSTM_FWD_N(bf16_t)
    else LSTM_FWD_N(float)
#undef LSTM_FWD_N
#undef LSTM_FWD
    return check_launch("lstm_fwd");
}

extern "C" int saicv_lstm_bwd(int dtype, const void* dy, const float* acts, const float* c, const void* whhT, void* dgates, int B, int Tn, int H,
                              void* stream) {
    hipStream_t s = S(stream);
    if (lstm_check("lstm_bwd", dtype, B, Tn, H)) return -1;
    SAICV_REQUIRE(dy && acts && c && whhT && dgates, "lstm_bwd: null gradient, saved state, weights or output");
    const size_t esz = dtype == SAICV_DTYPE_BF16 ? 2 : 4;
    const size_t tilebytes = LSTM_ROWS * ((size_t)4 * H * esz + LSTM_PAD);
    const bool lds = tilebytes <= (size_t)LSTM_LDS_MAX;
    const int nbuf = 2 * tilebytes <= (size_t)LSTM_LDS_MAX ? 2 : 1;
    const size_t smem = lds ? nbuf * tilebytes : 0;
    const dim3 grid(2 * ((B + LSTM_ROWS - 1) / LSTM_ROWS));
#define LSTM_BWD(T, N, L)                                                                                                  \
    do {                                                                                                                   \
        static bool once = (lstm_allow_lds(lstm_bwd_kernel<T, N, L>), true);                                               \
        (void)once;                                                                                                        \
        hipLaunchKernelGGL((lstm_bwd_kernel<T, N, L>), grid, dim3(LSTM_THREADS), smem, s, (const T*)dy, acts, c, (const T*)whhT, \
                           (T*)dgates, B, Tn, H, nbuf);                                                                    \
    } while (0)
    const int n = lstm_slices(H);
    if (dtype == SAICV_DTYPE_BF16) {                                        // 16 x 4H bf16 fits at every H
        SAICV_REQUIRE(lds, "lstm_bwd: hidden size %d needs %zu bytes of LDS", H, tilebytes);
        switch (n) {
            case 1: LSTM_BWD(bf16_t, 1, true); break;
            case 2: LSTM_BWD(bf16_t, 2, true); break;
            case 4: LSTM_BWD(bf16_t, 4, true); break;
            default: LSTM_BWD(bf16_t, 8, true); break;
        }
    } else if (lds) {                                                       // fp32, H <= 608
        switch (n) {
            case 1: LSTM_BWD(float, 1, true); break;
            case 2: LSTM_BWD(float, 2, true); break;
            case 4: LSTM_BWD(float, 4, true); break;
            default: LSTM_BWD(float, 8, true); break;
        }
    } else {                                                                // fp32, H >= 640: more than four slices per wave
        LSTM_BWD(float, 8, false);
    }
#undef LSTM_BWD
    return check_launch("lstm_bwd");
}

}  // namespace saicv
