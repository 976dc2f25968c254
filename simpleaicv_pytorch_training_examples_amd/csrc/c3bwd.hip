// Backward of the third (1 x 1) convolution of a bottleneck block behind its BatchNorm + residual + ReLU join, as ONE stream.
//
// Reference SimpleAICV/classification/backbones/resnet.py:100-155: conv3 = ConvBnActBlock(planes, planes * 4, 1, has_act=False),
// then `x = x + inputs; x = relu(x)`.  Its backward moved the gradient dy of the convolution output through HBM three times: the
// BatchNorm-backward apply pass (bn.hip, bn_bwd_apply_kernel) wrote it, the data gradient (pwstream.hip / igemm.hip) and the weight
// gradient (igemm.hip, igemm_tn_dma_kernel) each read it, and nothing else ever does.  At 56 x 56 x 256 channels (batch 256: 411 MB
// per tensor) these kernels all run at the HBM rate, so only removed bytes buy time: here dy lives in registers and in LDS.
//
// THE RESULTS ARE THOSE OF THE THREE KERNELS, BIT FOR BIT (deterministic mode, the shapes the streaming data gradient takes): a
// training step is chaotic enough that another association of a sum changes every parameter after a few steps, so the fused kernel
// keeps every association of the kernels it replaces:
//   * dy = fmaf(ca, g, fmaf(cb, y, cc)), g = mask ? dz : 0, rounded to bf16 -- expression and rounding of bn_bwd_apply_kernel;
//   * data gradient: one accumulator per output element over the WHOLE reduction, k-steps of 32 dy channels in ascending order,
//     the weights as the first MFMA operand -- pw_stream_kernel's chain.  A workgroup has CO / 64 wavefronts; wavefront w FORMS the
//     64 dy channels 64 w .. 64 w + 63 of a 32-pixel tile (their 48 coefficients in registers) and parks them in LDS; after a
//     barrier wavefront w MULTIPLIES 16 pixels x 32 input channels over all dy channels (its weight rows in registers);
//   * weight gradient: dW[64 w ..][CI] += dy^T x, one 32-pixel k-step per tile, both operands read TRANSPOSED from LDS
//     (ds_read_b64_tr_b16; images swizzled as igemm_tn_dma_kernel's), accumulators in registers for the whole stream.  Workgroup s
//     takes the CONSECUTIVE rows of split s of igemm_tn's plan for the same product (tn_plan through igemm_plan) and hands its
//     [CO][CI] partial to saicv::DetParts as part s: the same chains, the same fold;
//   * the BatchNorm-backward sums of the NEXT node (bs_*) over the stored dx are pw_stream_kernel's: its lanes walk the tensor in a
//     strided order that no workgroup of consecutive rows can follow, so a second, small kernel (c3_bs_sums_kernel: 0.5 tensor
//     passes at a quarter of the channels) re-reads dx and repeats that kernel's additions lane for lane, row for row.
// Two tiles of loads are in flight in registers per wavefront (dz and y as the MFMA operand needs them: lane (pixel = lane & 15,
// k-group = lane >> 4) = 16 contiguous bytes of that pixel's row; the mask byte of the same chunk; the x tile one chunk per thread).
#include <stdlib.h>

#include <type_traits>

#include "common.h"
#include "det.h"
#include "saicv_internal.h"
#include "../../include/saicv_hip.h"

namespace {

struct C3Params {
    const bf16_t* dz;           // [M][CO] gradient of the join's output
    const bf16_t* y;            // [M][CO] c3 output before BatchNorm
    const uint8_t* mask;        // [M][CO / 8] ReLU mask of the join
    const float* ca;            // [CO] each: dy = ca * g + cb * y + cc (bn_finalize_bwd_kernel)
    const float* cb;
    const float* cc;
    const bf16_t* x;            // [M][CI] input of the convolution
    const bf16_t* wd;           // [CI][CO] data-gradient weights
    bf16_t* dx;                 // [M][CI]
    float* dw;                  // [CO][CI], accumulated into
    const bf16_t* bs_y;         // BatchNorm-backward sums of the stored dx (PWParams of pwstream.hip): g = dx * [mask],
    const uint8_t* bs_mask;     //   bs_g = sum g, bs_gx = sum g * (y - mean) * invstd
    const float* bs_mean;
    const float* bs_invstd;
    float* bs_g;
    float* bs_gx;
    int bs_atomic_rows;         // > 0: the sums are ADDED into this many zeroed rows; 0: row = workgroup
    saicv::DetSink det;
    uint32_t dz_bytes, mask_bytes, x_bytes;
    int M, ntiles, tiles_per_wg;
};

// (as pwstream.hip: a store the compiler does not see leaves it counting the prefetched loads only, in order)
DEVINL void st_plain(void* q, u32x4 v) {
    asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" ::"v"(q), "v"(v) : "memory");
}
template <int B, int E, typename F> DEVINL void static_for(F&& f) {
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        static_for<B + 1, E>(f);
    }
}
// swizzle of the transposed-read images (igemm.hip, igemm_tn_dma_kernel): the 32-byte pair p of row r lives at pair slot p ^ g(r)
DEVINL int c3_key(int r) { return (r & 3) | (((r >> 3) & 1) << 2); }
template <int CPR> DEVINL int c3_g(int r) { return CPR >= 16 ? c3_key(r) : (c3_key(r) >> 1); }

constexpr int kTilePx = 32;
constexpr size_t c3_lds_bytes(int co, int ci) {
    return (size_t)kTilePx * (ci * 2 + 16) + (size_t)kTilePx * ci * 2 + (size_t)(co / 64) * kTilePx * 128;
}

template <int CO, int CI>
__global__ __launch_bounds__(CO) void c3_bwd_stream_kernel(const C3Params p) {
    constexpr int DEPTH = 2;                      // tiles in flight in registers
    constexpr int NW = CO / 64;                   // wavefronts = 64-channel slices of dy
    constexpr int TP = kTilePx;
    constexpr int XT = CI / 16;                   // MFMA tiles over the input channels
    constexpr int CPX = CI / 8;                   // 16-byte chunks per row of x / dx
    constexpr int KSA = CO / 32;                  // k-steps of the data gradient's whole reduction
    constexpr int NT2 = 2 * XT / NW;              // input-channel tiles a wavefront multiplies (for one 16-pixel half of the tile)
    constexpr int OP = CI * 2 + 16;               // bytes per row of the staged dx tile
    constexpr int OUT_BYTES = TP * OP;
    constexpr int XS_BYTES = TP * CI * 2;
    constexpr uint32_t OOB = 0xfffffff0u;
    static_assert(CO % 64 == 0 && CI % 16 == 0 && TP * CPX == CO && NT2 == 2, "one x / dx chunk per thread and tile");
    typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const outt = smem;
    char* const xs = smem + OUT_BYTES;
    char* const strips = smem + OUT_BYTES + XS_BYTES;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    const int nc0 = wave * 64;
    char* const strip = strips + wave * (TP * 128);
    const int opx = tid / CPX, och = tid % CPX;   // this thread's chunk of the x tile and of the dx tile
    const int mpt = wave & 1, mnt0 = (wave >> 1) * NT2;      // the data-gradient block this wavefront multiplies

    // ---- resident operands: coefficients of this lane's 2 x 8 dy channels; weight fragments (row = input channel, k = dy channel)
    float ka[2][8], kb[2][8], kc[2][8];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = nc0 + ks * 32 + lg * 8 + j;
            ka[ks][j] = p.ca[c]; kb[ks][j] = p.cb[c]; kc[ks][j] = p.cc[c];
        }
    u32x4 wf[NT2][KSA];
#pragma unroll
    for (int n2 = 0; n2 < NT2; ++n2)
#pragma unroll
        for (int ks = 0; ks < KSA; ++ks) wf[n2][ks] = ld_chunk(p.wd + (size_t)((mnt0 + n2) * 16 + l15) * CO + ks * 32 + lg * 8);

    const __amdgpu_buffer_rsrc_t dz_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(p.dz), 0, p.dz_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t y_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(p.y), 0, p.dz_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t mk_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.mask), 0, p.mask_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t x_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(p.x), 0, p.x_bytes, 0x00020000);

    // one tile's operands in registers.  Rows past M read zeros (buffer bounds): x = 0 keeps them out of dW, dx is not stored there
    struct Slot { u32x4 g[2][2], y[2][2]; uint32_t m[2][2]; u32x4 x; };
    Slot slot[DEPTH];
    const int first = (int)blockIdx.x * p.tiles_per_wg;       // consecutive tiles: the rows of split blockIdx.x of igemm_tn's plan
    const int count = max(0, min(p.tiles_per_wg, p.ntiles - first));
    auto tile_of = [&](int i) { return i < count ? first + i : -1; };
    const uint32_t frag_off = ((uint32_t)l15 * CO + nc0 + lg * 8) * 2u;
    const uint32_t xo_off = ((uint32_t)opx * CI + och * 8) * 2u;
    auto load_tile = [&](Slot& s, int tile) __attribute__((always_inline)) {
        const bool ok = tile >= 0;
        const uint32_t fb = (uint32_t)tile * (TP * CO * 2) + frag_off;
#pragma unroll
        for (int pt = 0; pt < 2; ++pt)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const uint32_t o = fb + pt * (16 * CO * 2) + ks * 64;
                s.g[pt][ks] = __builtin_amdgcn_raw_buffer_load_b128(dz_rs, (int)(ok ? o : OOB), 0, 0);
                s.y[pt][ks] = __builtin_amdgcn_raw_buffer_load_b128(y_rs, (int)(ok ? o : OOB), 0, 0);
                s.m[pt][ks] = __builtin_amdgcn_raw_buffer_load_b8(mk_rs, (int)(ok ? (o >> 4) : OOB), 0, 0);
            }
        const uint32_t xo = (uint32_t)tile * (TP * CI * 2) + xo_off;
        s.x = __builtin_amdgcn_raw_buffer_load_b128(x_rs, (int)(ok ? xo : OOB), 0, 0);
    };
#pragma unroll
    for (int dd = 0; dd < DEPTH; ++dd) load_tile(slot[dd], tile_of(dd));

    f32x4 accw[4][XT];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < XT; ++b) accw[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    // transposed fragment reads: lane (column l15, k-group lg) gets rows lg * 8 .. + 7 of its column (two reads of four rows)
    const int row0 = lg * 8 + (l15 >> 2);
    int fa_off[4], fb_off[XT];
#pragma unroll
    for (int a = 0; a < 4; ++a) fa_off[a] = row0 * 128 + ((a ^ c3_g<8>(row0)) << 5) + (l15 & 3) * 8;
#pragma unroll
    for (int b = 0; b < XT; ++b) fb_off[b] = row0 * (CI * 2) + ((b ^ c3_g<CPX>(row0)) << 5) + (l15 & 3) * 8;
    const int xs_off = opx * (CI * 2) + ((och ^ (c3_g<CPX>(opx) << 1)) << 4);
    // the data gradient's second operand: pixel mpt * 16 + l15, 16-byte chunk (k-step & 1) * 4 + lg of the strip of wavefront k-step / 2
    const int mrow = mpt * 16 + l15;
    int mb_off[2];
#pragma unroll
    for (int k1 = 0; k1 < 2; ++k1) mb_off[k1] = mrow * 128 + (((k1 * 4 + lg) ^ (c3_g<8>(mrow) << 1)) << 4);

    // One tile of slot D (a compile-time index: the slots are registers; no path skips a slot, see pwstream.hip)
    auto step = [&](auto D, int i) __attribute__((always_inline)) {
        constexpr int d = decltype(D)::value;
        Slot& s = slot[d];
        const int tile = tile_of(i);
        // ---- dy of this wavefront's 64 channels, 32 pixels -> its strip (the image both products read)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int pt = 0; pt < 2; ++pt) {
                float g[8], yy[8], o[8];
                Chunk<bf16_t>::unpack(s.g[pt][ks], g);
                Chunk<bf16_t>::unpack(s.y[pt][ks], yy);
                const uint32_t bits = s.m[pt][ks];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float gj = ((bits >> j) & 1u) ? g[j] : 0.f;
                    o[j] = fmaf(ka[ks][j], gj, fmaf(kb[ks][j], yy[j], kc[ks][j]));
                }
                const int row = pt * 16 + l15, ch = ks * 4 + lg;
                *reinterpret_cast<u32x4*>(strip + row * 128 + ((ch ^ (c3_g<8>(row) << 1)) << 4)) = Chunk<bf16_t>::pack(o);
            }
        *reinterpret_cast<u32x4*>(xs + xs_off) = s.x;
        load_tile(s, tile_of(i + DEPTH));             // the slot is free again: DEPTH tiles ahead
        __syncthreads();                              // every strip and the x image are written
        // ---- data gradient: 16 pixels x NT2 * 16 input channels over ALL dy channels, one chain per element (pw_stream_kernel's)
        f32x4 acc[NT2];
#pragma unroll
        for (int n2 = 0; n2 < NT2; ++n2) acc[n2] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KSA; ++ks) {
            const u32x4 bfr = ld_chunk(strips + (ks >> 1) * (TP * 128) + mb_off[ks & 1]);
#pragma unroll
            for (int n2 = 0; n2 < NT2; ++n2) Mma<bf16_t>::run(acc[n2], wf[n2][ks], bfr);
        }
        // D row lg * 4 + r = input channel, D column = pixel l15
#pragma unroll
        for (int n2 = 0; n2 < NT2; ++n2) {
            bf16x4 pk;
#pragma unroll
            for (int r = 0; r < 4; ++r) pk[r] = (bf16_t)acc[n2][r];
            *reinterpret_cast<bf16x4*>(outt + mrow * OP + ((mnt0 + n2) * 16 + lg * 4) * 2) = pk;
        }
        // ---- weight gradient: dW[nc0 + a * 16 + ..][b * 16 + ..] += dy^T x over the tile's 32 pixels
        {
            u32x4 af[4], bf[XT];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const bf16x4 l4 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(strip + fa_off[a]));
                const bf16x4 h4 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(strip + fa_off[a] + 4 * 128));
                const u32x2 l2 = __builtin_bit_cast(u32x2, l4), h2 = __builtin_bit_cast(u32x2, h4);
                af[a] = u32x4{l2[0], l2[1], h2[0], h2[1]};
            }
#pragma unroll
            for (int b = 0; b < XT; ++b) {
                const bf16x4 l4 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(xs + fb_off[b]));
                const bf16x4 h4 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(xs + fb_off[b] + 4 * CI * 2));
                const u32x2 l2 = __builtin_bit_cast(u32x2, l4), h2 = __builtin_bit_cast(u32x2, h4);
                bf[b] = u32x4{l2[0], l2[1], h2[0], h2[1]};
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < XT; ++b) Mma<bf16_t>::run(accw[a][b], af[a], bf[b]);
        }
        __syncthreads();                              // the dx tile is staged
        {
            const u32x4 v = ld_chunk(outt + opx * OP + och * 16);
            const int row = tile * TP + opx;
            if (row < p.M) st_plain(p.dx + (size_t)row * CI + och * 8, v);
        }
        __syncthreads();                              // strips, x image and dx tile are free for the next tile
    };
    int i0 = 0;
    for (; i0 + DEPTH <= count; i0 += DEPTH) static_for<0, DEPTH>([&](auto D) { step(D, i0 + decltype(D)::value); });
    static_for<0, DEPTH - 1>([&](auto D) {
        if (i0 + decltype(D)::value < count) step(D, i0 + decltype(D)::value);      // uniform over the workgroup
    });

    // ---- weight-gradient partial of this workgroup: D row -> dy channel, D column -> input channel (every element, zeros included)
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < XT; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const size_t idx = (size_t)(nc0 + a * 16 + lg * 4 + r) * CI + b * 16 + l15;
                saicv::det_add(p.det, p.dw + idx, idx, (int)blockIdx.x, accw[a][b][r]);
            }
}

// BatchNorm-backward sums of the stored dx, as the data-gradient epilogue of pw_stream_kernel takes them (pwstream.hip, EXTRAS): the
// same streams (unit u walks the 16-row groups u, u + U, ...; lane (row lane / 8 and + 8, chunk lane % 8)), the same additions in
// the same order, the same combination at the end -- the partial rows are that kernel's bit for bit.
constexpr int bs_nwaves(int nd) { return nd / 64 > 4 ? nd / 64 : 4; }
template <int ND>
__global__ __launch_bounds__(64 * bs_nwaves(ND)) void c3_bs_sums_kernel(const C3Params p, int mtiles, int units) {
    constexpr int NSPLIT = ND / 64, NWAVES = bs_nwaves(ND), GPB = NWAVES / NSPLIT;
    constexpr int CPR = 8, RPP = 8;
    __shared__ float red[NWAVES * 2 * 64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int slice = wave % NSPLIT, nc0 = slice * 64;
    const int unit = blockIdx.x * GPB + wave / NSPLIT;
    const int U = units;
    const int crow = lane / CPR, cchunk = lane % CPR;
    const bool maskp = p.bs_mask != nullptr;
    const int count = unit < mtiles ? (mtiles - unit + U - 1) / U : 0;
    struct Ops { u32x4 v[2], y[2]; unsigned m[2]; };
    auto load = [&](Ops& o, int i) __attribute__((always_inline)) {
        const int tile = unit + i * U;
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            const int row = tile * 16 + ps * RPP + crow;
            const bool rok = i < count && row < p.M;
            const size_t ooff = (size_t)row * ND + nc0 + cchunk * 8;
            o.v[ps] = u32x4{0u, 0u, 0u, 0u};
            o.y[ps] = u32x4{0u, 0u, 0u, 0u};
            o.m[ps] = 0xffu;
            if (rok) {
                o.v[ps] = ld_chunk(p.dx + ooff);
                o.y[ps] = ld_chunk(p.bs_y + ooff);
                if (maskp) o.m[ps] = p.bs_mask[ooff >> 3];
            }
        }
    };
    float ssum[8], ssq[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { ssum[e] = 0.f; ssq[e] = 0.f; }
    auto add = [&](const Ops& o) __attribute__((always_inline)) {
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            float f[8], yy[8];
            Chunk<bf16_t>::unpack(o.v[ps], f);
            Chunk<bf16_t>::unpack(o.y[ps], yy);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float ge = ((o.m[ps] >> e) & 1u) ? f[e] : 0.f;
                ssum[e] += ge;
                ssq[e] = fmaf(ge, yy[e], ssq[e]);
            }
        }
    };
    Ops oa, ob;
    load(oa, 0);
    for (int i = 0; i < count; i += 2) {              // two row groups in flight; the additions stay in stream order
        load(ob, i + 1);
        add(oa);
        load(oa, i + 2);
        if (i + 1 < count) add(ob);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = nc0 + cchunk * 8 + e;
        ssq[e] = p.bs_invstd[c] * fmaf(-p.bs_mean[c], ssum[e], ssq[e]);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        ssum[e] += __shfl_xor(ssum[e], 8, 64);  ssq[e] += __shfl_xor(ssq[e], 8, 64);
        ssum[e] += __shfl_xor(ssum[e], 16, 64); ssq[e] += __shfl_xor(ssq[e], 16, 64);
        ssum[e] += __shfl_xor(ssum[e], 32, 64); ssq[e] += __shfl_xor(ssq[e], 32, 64);
    }
    if (lane < CPR) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            red[(wave * 2 + 0) * 64 + lane * 8 + e] = ssum[e];
            red[(wave * 2 + 1) * 64 + lane * 8 + e] = ssq[e];
        }
    }
    __syncthreads();
    const size_t row = p.bs_atomic_rows ? (size_t)(blockIdx.x % p.bs_atomic_rows) : (size_t)blockIdx.x;
    for (int c = threadIdx.x; c < 2 * ND; c += 64 * NWAVES) {
        const int which = c / ND, col = c - which * ND;
        const int sl = col / 64, cc = col - sl * 64;
        float a = 0.f;
#pragma unroll
        for (int g = 0; g < GPB; ++g) a += red[((g * NSPLIT + sl) * 2 + which) * 64 + cc];       // fixed order over the streams
        float* dst = (which ? p.bs_gx : p.bs_g) + row * ND + col;
        if (p.bs_atomic_rows) unsafeAtomicAdd(dst, a); else *dst = a;
    }
}

// rows of partial sums = workgroups of c3_bs_sums_kernel = those of the streaming data gradient for [M][CI] (pw_stream_blocks)
int c3_sum_rows(int M, int ci) {
    const int nsplit = ci / 64, nwaves = nsplit > 4 ? nsplit : 4, gpb = nwaves / nsplit;
    const int mtiles = (M + 15) / 16, want = (mtiles + gpb - 1) / gpb, cap = 256 * 2 * 4 / nwaves;
    return want < cap ? want : cap;
}

// routed: ConvBnActFn.backward takes the fused launch for this class (profiles/c3_bwd_stream.md).  (512, 128) is built and tested but
// stays on the three kernels: its weight rows (128 registers) and weight-gradient accumulators (128) leave a wavefront of the
// 512-thread workgroup none of its 256 registers for the operands in flight -- the compiler spills, and it is several times slower.
struct C3Shape { int co, ci; bool routed; };
constexpr C3Shape kC3Shapes[] = {{256, 64, true}, {512, 128, false}};

template <int CO, int CI>
int launch_c3(const C3Params& p, int blocks, hipStream_t st) {
    auto k = c3_bwd_stream_kernel<CO, CI>;
    constexpr size_t smem = c3_lds_bytes(CO, CI);
    static bool once = (hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem), true);
    (void)once;
    hipLaunchKernelGGL(k, dim3(blocks), dim3(CO), smem, st, p);
    return saicv::check_launch("c3_bwd_stream");
}

}  // namespace

namespace saicv {

// Rows of partial BatchNorm-backward sums of the launch for a shape it has a form for (no switches), else 0.  Buffer-addressed operands stay below 4 GiB,
// the last tile's rows past M included.
extern "C" int saicv_c3_bwd_stream_rows(int M, int CO, int CI) {
    if (M < 1 || ((size_t)M + kTilePx) * CO * 2 >= 0xfffffff0ull) return 0;
    for (const C3Shape& s : kC3Shapes)
        if (s.co == CO && s.ci == CI) return c3_sum_rows(M, CI);
    return 0;
}

// splits (= workgroups = parts of the weight gradient) and 32-row tiles per split: igemm_tn's plan for the same product
static int c3_plan(int M, int CO, int CI, int* splits, int* tiles_per_wg) {
    saicv_plan_query q = {};
    q.op = SAICV_PLAN_CONV_WGRAD;
    q.conv.N = 1; q.conv.H = M; q.conv.W = 1; q.conv.C = CI; q.conv.K = CO; q.conv.R = 1; q.conv.S = 1; q.conv.stride = 1; q.conv.pad = 0;
    q.conv.OH = M; q.conv.OW = 1; q.conv.dtype = SAICV_BF16;
    saicv_plan pl;
    if (igemm_plan(&q, &pl) != 0) return -1;
    SAICV_REQUIRE(pl.splits >= 1 && (pl.rt_per * pl.rows_per_step) % kTilePx == 0, "c3_bwd_stream: weight-gradient plan with %d x %d rows per split",
                  pl.rt_per, pl.rows_per_step);
    *splits = pl.splits;
    *tiles_per_wg = pl.rt_per * pl.rows_per_step / kTilePx;
    return 0;
}

// Workspace floats of the launch: 64 * CO for the finalize step's second stage, 3 * CO coefficients and, in the fast mode, the
// weight-gradient parts.  (The fast mode of the kernels this launch replaces adds the splits' tiles with fp32 atomics in completion
// order; here the parts are parked and folded in BOTH modes -- the fold is 5 us at 56 x 56, and the sum of 245 ... 256 atomics in
// an order that changes from run to run strayed up to 2.4 times as far from float64 as the three kernels' did.)
extern "C" size_t saicv_c3_bwd_stream_ws_floats(int M, int CO, int CI) {
    size_t n = (size_t)67 * CO;
    int splits = 0, tpw = 0;
    if (!g_deterministic && saicv_c3_bwd_stream_rows(M, CO, CI) > 0 && c3_plan(M, CO, CI, &splits, &tpw) == 0 && splits > 1)
        n += (size_t)splits * CO * CI;
    return n;
}

// Rows of partial BatchNorm-backward sums of the fused launch, 0 if the three-kernel route keeps this layer.  A pure
// function of its arguments and of SAICV_C3_BWD_STREAM (default 1) / SAICV_C3_BWD_MIN_ROWS (default 65536), read per call.
extern "C" int saicv_c3_bwd_stream_ok(int dtype, int M, int CO, int CI) {
    const char* es = getenv("SAICV_C3_BWD_STREAM");
    const char* er = getenv("SAICV_C3_BWD_MIN_ROWS");
    const int on = es ? atoi(es) : 1;
    const int min_rows = er ? atoi(er) : 65536;
    if (!on || dtype != SAICV_DTYPE_BF16 || M < min_rows) return 0;
    for (const C3Shape& s : kC3Shapes)
        if (s.co == CO && s.ci == CI && s.routed) return saicv_c3_bwd_stream_rows(M, CO, CI);
    return 0;
}

// The launch (no switches: any M).  coef = [3][CO] as bn_finalize_bwd_kernel wrote them; ex: the bs_* operands of EpiExtra or nullptr;
// bs_rows > 0: the sums are added into that many pooled rows, else saicv_c3_bwd_stream_rows() rows are written.
int c3_bwd_stream(int M, int CO, int CI, const void* dz, const void* y, const void* mask, const float* coef, const void* x,
                  const void* wd, void* dx, float* dw, const EpiExtra* ex, int bs_rows, float* part_ws, hipStream_t st) {
    SAICV_REQUIRE(saicv_c3_bwd_stream_rows(M, CO, CI) > 0, "c3_bwd_stream: no form for M = %d, Cout = %d, Cin = %d (bf16, (256, 64) or (512, 128), "
                  "operands below 4 GiB)", M, CO, CI);
    SAICV_REQUIRE(dz && y && mask && coef && x && wd && dx && dw, "c3_bwd_stream: operand missing");
    C3Params p = {};
    p.dz = (const bf16_t*)dz; p.y = (const bf16_t*)y; p.mask = (const uint8_t*)mask;
    p.ca = coef; p.cb = coef + CO; p.cc = coef + 2 * CO;
    p.x = (const bf16_t*)x; p.wd = (const bf16_t*)wd; p.dx = (bf16_t*)dx; p.dw = dw;
    if (ex && ex->bs_y) {
        SAICV_REQUIRE(ex->bs_mean && ex->bs_invstd && ex->bs_g && ex->bs_gx, "c3_bwd_stream: BatchNorm-backward sums need mean / invstd / outputs");
        p.bs_y = (const bf16_t*)ex->bs_y; p.bs_mask = ex->bs_mask; p.bs_mean = ex->bs_mean; p.bs_invstd = ex->bs_invstd;
        p.bs_g = ex->bs_g; p.bs_gx = ex->bs_gx;
        p.bs_atomic_rows = bs_rows;
    }
    p.dz_bytes = (uint32_t)((size_t)M * CO * 2);
    p.mask_bytes = (uint32_t)((size_t)M * CO / 8);
    p.x_bytes = (uint32_t)((size_t)M * CI * 2);
    p.M = M;
    p.ntiles = (M + kTilePx - 1) / kTilePx;
    // the splits of the weight gradient this launch replaces: workgroup = split
    int blocks = 0;
    if (c3_plan(M, CO, CI, &blocks, &p.tiles_per_wg) != 0) return -1;
    DetParts parts;
    if (parts.begin(st, blocks, (size_t)CO * CI, "c3_bwd_stream", false) != 0) return -1;      // every workgroup writes its whole part
    if (!parts.on() && blocks > 1) {                  // fast mode: the parts go to the caller's workspace, the same fold
        SAICV_REQUIRE(part_ws != nullptr, "c3_bwd_stream: workspace for the weight-gradient parts missing");
        parts.s.part = part_ws;
    }
    p.det = parts.sink();
    int rc = CO == 256 ? launch_c3<256, 64>(p, blocks, st) : launch_c3<512, 128>(p, blocks, st);
    if (rc != 0) return rc;
    if (parts.fold(dw, 0, (size_t)CO * CI, true) != 0) return -1;
    if (p.bs_y) {
        const int rows = c3_sum_rows(M, CI), mtiles = (M + 15) / 16;
        if (CI == 64) hipLaunchKernelGGL(c3_bs_sums_kernel<64>, dim3(rows), dim3(64 * bs_nwaves(64)), 0, st, p, mtiles, rows * (bs_nwaves(64) / 1));
        else hipLaunchKernelGGL(c3_bs_sums_kernel<128>, dim3(rows), dim3(64 * bs_nwaves(128)), 0, st, p, mtiles, rows * (bs_nwaves(128) / 2));
        return check_launch("c3_bs_sums");
    }
    return 0;
}

}  // namespace saicv
