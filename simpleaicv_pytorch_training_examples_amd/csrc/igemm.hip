// Implicit-GEMM convolution / linear kernels for gfx950 (MI355X), NHWC.
//
//   igemm_nt : OUT[m][n] = sum_k GATHER(src)[m][k] * WGT[n][k]
//              conv forward (rows = output pixels, k = (r,s,c)), conv data-gradient
//              (rows = input pixels, k = (r,s,cout)) and nn.Linear forward / input-grad.
//   igemm_tn : DW[n][kk] += sum_m DY[m][n] * GATHER(src)[m][kk]
//              conv / linear weight-gradient; both operands are reduction-major in HBM,
//              so bf16 fragments are built with the LDS transpose read
//              (ds_read_b64_tr_b16) and the reduction over pixels is split across
//              workgroups with fp32 hardware atomics into a pre-zeroed fp32 gradient.
//
// Replaces the ATen `convolution` / `convolution_backward` / `addmm` / `mm` dispatches of
// reference SimpleAICV/classification/backbones/resnet.py:33-43 (ConvBnActBlock) and
// resnet.py:204 (fc).  NT: four tile geometries (256x256 / 8 wavefronts, 256x128 / 8, 128x128 / 4, 128x64 / 4), 64-byte
// K slices streamed global -> LDS by DMA (buffer_load ... lds) into a 3- or 4-stage ring, counted vmcnt and one raw
// barrier per K step, MFMA 16x16x32 bf16 (perf mode) or 16x16x4 f32 (parity mode), an XOR swizzle that makes the
// ds_read_b128 fragment reads conflict free, LDS-staged epilogue with the fused modes listed at NTParams.
// TN: 64x64 .. 256x256 tiles, register-staged loads, ds_read_b64_tr_b16 fragments, one resident round of workgroups.
#include <type_traits>

#include <stdlib.h>
#include "common.h"
#include "saicv_internal.h"
#include "det.h"
#include "../../include/saicv_hip.h"

namespace {

struct FastDiv {           // exact unsigned division by a runtime constant (Granlund-Montgomery)
    uint32_t mul, s1, s2;
};
DEVINL uint32_t fdiv(uint32_t n, FastDiv d) {
    const uint32_t t = __umulhi(d.mul, n);
    return (t + ((n - t) >> d.s1)) >> d.s2;
}

// LDS-DMA ring depth per geometry: 4 stages, except 256 x 128 where 3 stages (72 KiB) let TWO workgroups share
// a CU so that one's epilogue overlaps the other's main loop
constexpr int nt_stages(int bm, int bn) { return (bm == 256 && bn == 128) ? 3 : 4; }
constexpr int nt_stages_kc8(int bm, int bn) { return (bm + bn) * 128 * 3 <= 150 * 1024 ? 3 : 2; }      // 128-byte K slices

struct NTParams {
    const void* src;
    const void* wgt;
    void* out;
    const float* bias;
    float* stat_sum;
    float* stat_sq;
    const void* addend;         // epilogue: out = addend + row_scale * (acc + bias)   (act_mode 2: the GELU pre-activation)
    void* out2;                 // act_mode 1: second output, gelu(out)
    int lean_gelu;              // 1: act modes 1 / 3 without addend / row scale take the lean epilogue row loop (SAICV_GELU_EPI=0: the general one)
    int act_mode;               // 0 none | 1 out2 = gelu(out) | 2 out = (acc + bias) * gelu'(addend) | 3 out = gelu'(pre), out2 = gelu(pre) | 4 out = (acc + bias) * addend
    const float* row_scale;
    int rows_per_scale;
    // data-gradient epilogue extras of a residual network (all tensors share out's [M][ldo] coordinates):
    const uint8_t* addend_gate; // addend counts only where its bit is set (the shortcut gradient behind a ReLU: one bit per
                                // element, one byte per 16-byte chunk -- the mask bn_act_fwd wrote)
    const void* bs_y;           // BatchNorm-backward partial sums of THIS output, for the BatchNorm whose dz it is:
    const uint8_t* bs_mask;     //   g = out * [mask bit];  bs_g[row][c] = sum g,  bs_gx[row][c] = sum g * (y - mean) * invstd
    const float* bs_mean;       //   over the rows of one tile; row = parity class * bs_rows + tile_m
    const float* bs_invstd;
    float* bs_g;
    float* bs_gx;
    int bs_rows;
    // > 0: the statistics (forward sum / sum of squares, backward bs_g / bs_gx) are ADDED with fp32 atomics into this many
    // rows (row = tile row mod count) of a zeroed buffer instead of written one row per tile row: few enough rows that the
    // consuming BatchNorm kernel finalises them itself (no partial-reduce / finalize launches)
    int stat_atomic_rows;
    uint32_t src_bytes, wgt_bytes;
    int H, W, C;        // gather-source spatial dims / channels
    int OH, OW;         // pixel grid that indexes the GEMM rows
    int R, S, stride, pad;
    int M, Nn, Kd;
    int ldo;
    int tiles_n;
    int nblk;
    int kc8;            // host: launch the 128-byte-K-slice instantiation (pointwise bf16, 256-row tiles)
    int stream_out;     // host: the output is written with streaming stores (see NT_OUT_ST)
    FastDiv fd_ohw, fd_ow;   // for OH*OW and OW (unit-stride row decomposition)
#ifdef SAICV_NT_TIMELINE
    unsigned long long* timeline;       // debug build only (scripts/nt_timeline.py): 8 shader-clock stamps per workgroup
#endif
};
#ifdef SAICV_NT_TIMELINE
// Debug build: per-workgroup phase stamps of igemm_nt1_kernel.  Stamps live in scalar registers and are written once, by one lane,
// behind the last store of the workgroup -- nothing is added to the vector-memory queue the K loop counts.
#define NT_STAMP(i) do { if (tl_on) tl_t[i] = __builtin_readcyclecounter(); } while (0)
static unsigned long long* g_nt_timeline = nullptr;
#else
#define NT_STAMP(i) do { } while (0)
#endif
// r05 -- output stores of igemm_nt1_kernel's epilogue are STREAMING stores ("nt": the line is not kept in L2 / MALL).  A training step's
// outputs are read by a LATER kernel and are 25-411 MB each against 32 MB of L2 and 256 MB of MALL; written with the default policy
// they evict what the neighbouring kernels re-read (the operand panels other tiles of this launch share, the dy a weight-gradient
// kernel reads right after the data-gradient kernel did).  Same box, library A/B (profiles/r05_nt_experiments.md): ResNet-50 21.85 ->
// 21.27 ms per step (igemm_nt 10.82 -> 10.60, igemm_tn 4.51 -> 4.30, bn_act_fwd 2.63 -> 2.55), ViT-B 40.04 -> 39.34 ms (igemm_nt 21.39 -> 20.43).
// (A run-time choice between the two store forms does not survive the compiler: `if (flag) nontemporal_store else store` is merged
// into one plain store.)
// Which launches stream: outputs of at least SAICV_NT_STREAM_MIN_MB MiB (p.stream_out).  The streaming form is an assembly statement --
// a run-time choice between __builtin_nontemporal_store and a plain store does not survive the compiler (both arms are merged into ONE
// plain store; the first build of this switch measured exactly like plain stores).  `s_nop 1`: the statement's data registers may be
// rewritten right behind it (guide section 5.7).
DEVINL void st_chunk_stream(void* q, u32x4 v) {
    asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 1" ::"v"(q), "v"(v) : "memory");
}
#define NT_OUT_ST(ptr, v) do { if (stream_out) st_chunk_stream(ptr, v); else st_chunk(ptr, v); } while (0)
// the data gradient's fused epilogue operands (shortcut gradient, pre-BatchNorm output, two mask bytes per chunk) are read exactly
// once; streaming loads of them measured neutral, so they keep the default policy
#define NT_EPI_LD ld_chunk

// NT kernel LDS image: one K tile = 64-byte rows = 4 chunks; chunk c of row r lives at slot
// c ^ f((r>>2)&3), f = {0,2,3,1}.  ds_read_b128 is served in 16-lane groups that mix rows 0-3 /
// 12-15 of chunk c with rows 4-11 of chunk c^1 (MI355X_MICROARCH.md, LDS table): with this f
// the 16 lanes of every group hit 16 distinct 16-byte bank groups.
DEVINL int lds_swz(int q) { return ((q & 1) << 1) ^ ((q >> 1) * 3); }
DEVINL int lds_off(int row, int chunk) { return row * 64 + ((chunk ^ lds_swz((row >> 2) & 3)) << 4); }
// 128-byte rows (KC = 8): chunk c of row r at slot c ^ ((r >> 1) & 7).  Two rows share a 256-byte bank window, and the 16-lane
// groups of ds_read_b128 mix rows {0-3, 12-15} of chunk c with rows {4-11} of chunk c + 1: per row parity that is eight (row,
// chunk) pairs whose slots c ^ {0, 1, 6, 7} and (c + 1) ^ {2, 3, 4, 5} are all different.
DEVINL int lds_off128(int row, int chunk) { return row * 128 + (((chunk ^ (row >> 1)) & 7) << 4); }

DEVINL u32x4 buf_ld(__amdgpu_buffer_rsrc_t rsrc, uint32_t byte_off) {
    return __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)byte_off, 0, 0);
}

// compile-time loop: f(std::integral_constant<int, I>) for I in [I0, N) -- immediates of assembly statements must be constants
template <int I, int N, typename F> DEVINL void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}
// r05 -- fragment reads of the bf16 K loops as ASSEMBLY statements.  With the reads as plain loads hipcc's scheduler, aiming at the
// launch bound's register budget, sinks the loads of W fragments 1.. BETWEEN the MFMA groups and reuses one register quad for
// all of them: `ds_read_b128; s_waitcnt lgkmcnt(0); 4 (8) MFMAs` four times per K step, i.e. four exposed LDS round trips per
// step and wavefront (a lone 256 x 128 workgroup ran 1 150 cycles per step for 544 cycles of MFMA work -- profiles/r05_nt_timeline.md).
// Here every read of a step is issued up front in a fixed order (W fragment 0, all A fragments, the other W fragments) and each MFMA
// group is released by a COUNTED lgkmcnt wait that names the registers it releases (LDS returns in order), as igemm_tn_dma_kernel does.
DEVINL uint32_t lds_addr32(const void* q) {
    typedef __attribute__((address_space(3))) const char lds_cchar;
    return (uint32_t)reinterpret_cast<uintptr_t>((lds_cchar*)q);
}
template <int IMM> DEVINL void lds_rd128(u32x4& d, uint32_t addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(IMM) : "memory");
}
template <int N> DEVINL void lgkm_release(u32x4& a) { asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(a) : "n"(N) : "memory"); }
template <int N> DEVINL void lgkm_release(u32x4& a, u32x4& b) { asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N) : "memory"); }

// r05 -- MFMA shape of igemm_nt1_kernel: the kernel is written over a fragment geometry (FR rows per fragment, NV accumulator values
// per lane, KSUB MFMAs per 64-byte LDS row), so that v_mfma_f32_32x32x16_bf16 could be tried against 16x16x32.  Why it was tried:
// the GEMM kernels run AT the 1 400 W socket limit on random operands (scripts/power_probe.py: 1 397 W at 2.22 GHz), and an isolated
// 64 x 64 wavefront tile fed from LDS sustains 1 622 TFLOP/s at that limit on the 32 x 32 shape against 1 418 on 16x16x32
// (scripts/probes/mfma_power_probe.hip).  What the models said, same box, library A/B (profiles/r05_nt_experiments.md): ViT-B 40.37 ->
// 41.19 ms, ResNet-50 22.0 -> 22.2 ms with the 32 x 32 shape -- it moves twice the accumulator registers per flop (16 read + 16
// written per K = 16) and the real loop, unlike the probe's, was never issue-bound.  16x16x32 stays (the 32 x 32 form: DESIGN.md).
// fp32 (parity mode): 16x16x4, four per 16-byte chunk.
template <typename T> struct NtMma;
template <> struct NtMma<bf16_t> {
    static constexpr int FR = 16, NV = 4, KSUB = 1;
    typedef f32x4 Acc;
    static DEVINL void run(Acc& acc, const u32x4& a, const u32x4& b) { Mma<bf16_t>::run(acc, a, b); }
};
template <> struct NtMma<float> {
    static constexpr int FR = 16, NV = 4, KSUB = 1;
    typedef f32x4 Acc;
    static DEVINL void run(Acc& acc, const u32x4& a, const u32x4& b) { Mma<float>::run(acc, a, b); }
};

// ------------------------------------------------------------------------------------ NT, one tile per workgroup
// The tiled kernel of every igemm_nt launch the streaming kernels of pwstream.hip do not take.  One tile per workgroup; its
// workgroup-wide epilogue (whole tile staged in LDS, statistics over all rows of the tile, eight independent row chunks per
// thread in flight) writes ONE partial-statistics row per tile row.
// Main loop = LDS-DMA ring: `buffer_load ... lds` writes global chunks straight into a 4-stage
// LDS ring (no staging registers, no ds_write), three K tiles are in flight across the single
// raw s_barrier of each tile, and the wait is a COUNTED s_waitcnt vmcnt(N) that only retires the
// tile about to be consumed (guide section 5, T3/T4).  The DMA destination is wave-linear
// (base + lane*16), so the XOR swizzle is applied to the SOURCE: lane l fetches the chunk that
// belongs in the slot it will fill.
// The loop is bound by MFMA issue only if the integer work per K tile is tiny, so:
//  * all gathers are raw buffer loads: an out-of-range lane (padding halo, M/N/K tails) gets
//    an offset beyond the buffer and the hardware writes zeros -- no branches, no exec masking;
//  * the (r, s, c) position of a thread's K chunk advances incrementally (no divisions);
//  * per-row constants fold image base and top-left corner, so a gather address is one add;
//  * LDS fragment addresses (with the XOR swizzle) are computed once.
// PLAIN: 1x1 taps without padding (pointwise conv, nn.Linear and their data-gradients): the K
// index IS the channel offset, no tap walker and no halo tests in the loop.
// Tile geometry (BM_T x BN_T output tile, WM_ x WN_ wavefronts, each owning a
// (BM_T/WM_) x (BN_T/WN_) sub-tile): 256x256 / 2x4, 256x128 / 4x2, 128x128 / 2x2, 128x64 / 2x2.
// Wider tiles raise flop per LDS-fill byte and the MFMAs issued per barrier and per DMA.
// KC = 16-byte chunks per LDS row = width of the K slice a step loads: 4 (64 bytes, 32 bf16) or 8 (128 bytes).  With 64-byte
// slices every DMA request is half a cache line; scripts/probes/fill_probe.hip measures what that costs on the fill path
// alone (profiles/r03_lds_fill_probe.jsonl: 8.7-10 TB/s against 11.5-12.3 TB/s for whole lines when four workgroups share
// a stream) and the 64-byte kernels sit exactly at that figure.  KC = 8 rows take twice the LDS per step: 3 slots of
// 48 KiB for the 256 x 128 tile, one workgroup per CU.
template <typename T, int BM_T, int BN_T, int WM_, int WN_, int MODE, bool OUT_F32, bool PLAIN, int KC = 4>
__global__ __launch_bounds__(64 * WM_ * WN_, (BM_T == 256 && BN_T == 128 && !OUT_F32 && KC == 4) ? 4 : 1) void igemm_nt1_kernel(const NTParams p) {
    constexpr int EPC = ElemTraits<T>::EPC;
    constexpr int BK = KC * EPC;                 // one 64- or 128-byte row per K tile
    constexpr int ROWB = KC * 16;                // bytes of an LDS row
    constexpr int RPI = 1024 / ROWB;             // tile rows filled by one DMA wave-instruction
    constexpr int NWAVES = WM_ * WN_;
    constexpr int NTHREADS = 64 * NWAVES;
    constexpr int WMR = BM_T / WM_;              // rows of the output tile owned by one wavefront
    constexpr int WN = BN_T / WN_;
    typedef NtMma<T> MM;
    constexpr int FR = MM::FR;                   // rows of a fragment (both operands): 16 (bf16 16x16x32, fp32 16x16x4)
    constexpr int NG = MM::NV / 4;               // groups of four consecutive output columns per lane and accumulator tile
    constexpr int KSUB = MM::KSUB;
    constexpr int NT_ = WN / FR;
    constexpr int MT_ = WMR / FR;
    static_assert(WN % FR == 0 && WMR % FR == 0, "wavefront sub-tile in whole MFMA tiles");
    constexpr int AROWS = BM_T / RPI / NWAVES;   // A-tile DMA instructions per thread
    constexpr int WROWS = BN_T / RPI / NWAVES;   // weight-tile DMA instructions per thread
    constexpr int LPT = AROWS + WROWS;           // loads per thread per K tile
    constexpr int NSTAGE = KC == 8 ? nt_stages_kc8(BM_T, BN_T) : nt_stages(BM_T, BN_T);
    constexpr int A_BYTES = BM_T * ROWB;
    constexpr int W_BYTES = BN_T * ROWB;
    static_assert(KC == 4 || (KC == 8 && NWAVES % 2 == 0 && sizeof(T) == 2), "128-byte K slices: bf16, even wavefront count");
    constexpr int STAGE = A_BYTES + W_BYTES;
    constexpr uint32_t OOB = 0xfffffff0u;   // 16-byte aligned, beyond any operand (host checks sizes)

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // provably wave-uniform (LDS-DMA base)
    const int wm = wave % WM_;
    const int wn = wave / WM_;
#ifdef SAICV_NT_TIMELINE
    const bool tl_on = p.timeline != nullptr;
    unsigned long long tl_t[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};       // 8..10: inside the set-up (tile known | rows decomposed | walker ready)
    const unsigned long long tl_rt0 = tl_on ? __builtin_amdgcn_s_memrealtime() : 0ull;      // 100 MHz, the same on every XCD
    NT_STAMP(0);
#endif

    // ---- data-gradient with stride s > 1: the input pixels split into s*s parity classes
    // (h % s, w % s); a class only ever meets the taps r == (h + pad) mod s, so each class is a
    // dense GEMM over its own tap subset (no multiply-by-zero work).  blockIdx.y = class.
    // In class-local terms the source pixel of (row, tap) is (A0 - tr, B0 - ts).
    int cs = 1, ph = 0, pw = 0, r0 = 0, s0 = 0, q0h = p.pad, q0w = p.pad;
    int Sc = p.S, Hc = p.OH, Wc = p.OW, Mc = p.M, Kc = p.Kd;
    int nblk = p.nblk;
    if (MODE == 1 && p.stride > 1) {
        cs = p.stride;
        ph = blockIdx.y / cs;
        pw = blockIdx.y - ph * cs;
        Hc = (p.OH - ph + cs - 1) / cs;
        Wc = (p.OW - pw + cs - 1) / cs;
        Mc = (p.M / (p.OH * p.OW)) * Hc * Wc;
        r0 = (ph + p.pad) % cs;
        s0 = (pw + p.pad) % cs;
        q0h = (ph + p.pad - r0) / cs;
        q0w = (pw + p.pad - s0) / cs;
        const int Rc = r0 < p.R ? (p.R - r0 + cs - 1) / cs : 0;
        Sc = s0 < p.S ? (p.S - s0 + cs - 1) / cs : 0;
        Kc = Rc * Sc * p.C;
        nblk = ((Mc + BM_T - 1) / BM_T) * p.tiles_n;
    }
    // ---- tile loop: the host launches one workgroup per tile (the hardware dispatcher balances the load), so the body runs once.
    // Spreading the workgroups' start times over a tile period -- so that epilogue write bursts and MFMA loops of
    // different CUs interleave -- was measured and bought nothing: the ramp costs what the steady state gains.
    for (int tix = blockIdx.x; tix < nblk; tix += gridDim.x) {
    if (tix != (int)blockIdx.x) {                  // the previous tile's LDS reads are done (its stores may still drain)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
    const int bid = xcd_remap(tix, nblk);
    const int tile_n = bid % p.tiles_n;
    const int tile_m = bid / p.tiles_n;
#ifdef SAICV_NT_TIMELINE
    if (tl_on) { int t_ = tile_m; asm volatile("" : "+s"(t_)); NT_STAMP(8); }
#endif

    const __amdgpu_buffer_rsrc_t src_rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.src), 0, p.src_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wgt_rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.wgt), 0, p.wgt_bytes, 0x00020000);

    typename MM::Acc acc[NT_][MT_];
#pragma unroll
    for (int ni = 0; ni < NT_; ++ni)
#pragma unroll
        for (int mi = 0; mi < MT_; ++mi)
#pragma unroll
            for (int r = 0; r < MM::NV; ++r) acc[ni][mi][r] = 0.f;

    const int ohw = Hc * Wc;
    const int lr = lane & (FR - 1);              // fragment row (first operand) / column (second operand) this lane addresses
    const int lk = lane / FR;                    // its 16-byte K chunk: 0..3 of the 64-byte row (fp32), 0..1 of each 32-byte half (bf16)
    // accumulator value r of tile (ni, mi): row m_base + mi*FR + lr, column n_base + ni*FR + fcol(r / 4) + r % 4
    auto fcol = [&](int g) { return FR == 32 ? 8 * g + 4 * lk : 4 * lk; };
    // r05 -- the bias starts the accumulators (see the prologue of the K loop): requested here, columns past N read zeros (buffer
    // bounds); N % 4 != 0 keeps the epilogue path
    const bool bias_early = p.bias != nullptr && (p.Nn & 3) == 0;      // uniform
    u32x4 bias_v[NT_][NG];
#pragma unroll
    for (int ni = 0; ni < NT_; ++ni)
#pragma unroll
        for (int g = 0; g < NG; ++g) bias_v[ni][g] = u32x4{0u, 0u, 0u, 0u};
    if (bias_early) {
        const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.bias), 0, p.Nn * 4, 0x00020000);
#pragma unroll
        for (int ni = 0; ni < NT_; ++ni)
#pragma unroll
            for (int g = 0; g < NG; ++g)
                bias_v[ni][g] = buf_ld(brs, (uint32_t)(tile_n * BN_T + wn * WN + ni * FR + fcol(g)) * 4u);
    }
    {
    // ---- per-thread DMA state.  Wave w, instruction i, lane l fills LDS bytes
    // [(i*NWAVES + w)*1024 + l*16, +16) of the A region: row (i*NWAVES+w)*16 + (l>>2), slot l&3, i.e. the
    // logical chunk (l&3) ^ f((row>>2)&3) = (l&3) ^ f((l>>4)&3) -- one K-chunk column per thread.
    // KC = 8: row (i*NWAVES + wave)*8 + (lane>>3), slot lane&7, logical chunk slot ^ ((row >> 1) & 7); (row >> 1) & 7 =
    // ((lane >> 4) + 4 * (wave & 1)) & 7 because NWAVES is even -- still one K-chunk column per thread
    const int cc = KC == 4 ? ((lane & 3) ^ lds_swz((lane >> 4) & 3)) : ((lane & 7) ^ (((lane >> 4) + 4 * (wave & 1)) & 7));
    int rowc[AROWS], a0[AROWS], b0[AROWS];   // rowc = (image base + A0*W + B0) * C  [elements]
#pragma unroll
    for (int i = 0; i < AROWS; ++i) {
        const int m = tile_m * BM_T + (i * NWAVES + wave) * RPI + lane / KC;
        if (m < Mc) {
            int img, oh, ow;
            if (cs == 1) {
                img = (int)fdiv((uint32_t)m, p.fd_ohw);
                const int rem = m - img * ohw;
                oh = (int)fdiv((uint32_t)rem, p.fd_ow);
                ow = rem - oh * Wc;
            } else {
                img = m / ohw;
                const int rem = m - img * ohw;
                oh = rem / Wc;
                ow = rem - oh * Wc;
            }
            if (MODE == 0) {
                a0[i] = oh * p.stride - p.pad;
                b0[i] = ow * p.stride - p.pad;
            } else {
                a0[i] = oh + q0h;
                b0[i] = ow + q0w;
            }
            rowc[i] = ((img * p.H + a0[i]) * p.W + b0[i]) * p.C;
        } else {
            rowc[i] = 0;
            a0[i] = -(1 << 24);
            b0[i] = -(1 << 24);
        }
    }
#ifdef SAICV_NT_TIMELINE
    if (tl_on) { int t_ = rowc[0]; asm volatile("" : "+v"(t_)); NT_STAMP(9); }
#endif
    int wrow[WROWS];                    // weight row base [elements], or -1
#pragma unroll
    for (int j = 0; j < WROWS; ++j) {
        const int n = tile_n * BN_T + (j * NWAVES + wave) * RPI + lane / KC;
        wrow[j] = n < p.Nn ? n * p.Kd : -1;
    }

    // K-chunk walker: k = kt*BK + cc*EPC  ->  (tr, ts, c0), advanced by BK per tile
    int kpos = cc * EPC;
    int tc0, ttr, tts;
    {
        const int tap = kpos / p.C;
        tc0 = kpos - tap * p.C;
        ttr = Sc > 0 ? tap / Sc : 0;
        tts = tap - ttr * Sc;
    }

    typedef __attribute__((address_space(3))) void lds_void;
    // issue the DMA of the next K tile (walker position) into ring slot `stage`
    auto issue_tile = [&](int stage) {
        char* base = smem + stage * STAGE + wave * 1024;
        const bool kvalid = kpos < Kc;
        int tapoff, kw;
        if (PLAIN) {
            tapoff = kpos;
            kw = kpos;
        } else if (MODE == 0) {
            tapoff = (ttr * p.W + tts) * p.C + tc0;
            kw = kpos;
        } else {
            tapoff = tc0 - (ttr * p.W + tts) * p.C;
            kw = ((r0 + ttr * cs) * p.S + (s0 + tts * cs)) * p.C + tc0;
        }
#pragma unroll
        for (int i = 0; i < AROWS; ++i) {
            const int ih = PLAIN ? a0[i] : (MODE == 0) ? a0[i] + ttr : a0[i] - ttr;
            const int iw = PLAIN ? b0[i] : (MODE == 0) ? b0[i] + tts : b0[i] - tts;
            // bitwise (not short-circuit) logic keeps this branch-free
            const bool ok = PLAIN ? (kvalid & (a0[i] >= 0))
                                  : (kvalid & ((unsigned)ih < (unsigned)p.H) & ((unsigned)iw < (unsigned)p.W));
            const uint32_t off = ok ? (uint32_t)(rowc[i] + tapoff) * (uint32_t)sizeof(T) : OOB;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(src_rs, (lds_void*)(base + i * NWAVES * 1024), 16, (int)off, 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < WROWS; ++j) {
            const bool ok = kvalid & (wrow[j] >= 0);
            const uint32_t off = ok ? (uint32_t)(wrow[j] + kw) * (uint32_t)sizeof(T) : OOB;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wgt_rs, (lds_void*)(base + A_BYTES + j * NWAVES * 1024), 16, (int)off, 0, 0, 0);
        }
        // advance to the next K tile
        kpos += BK;
        if (PLAIN) return;
        tc0 += BK;
        if (p.C >= BK) {                 // at most one tap boundary per tile (uniform branch)
            const bool wrap = tc0 >= p.C;
            tc0 -= wrap ? p.C : 0;
            tts += wrap ? 1 : 0;
            const bool wrap2 = tts == Sc;
            tts = wrap2 ? 0 : tts;
            ttr += wrap2 ? 1 : 0;
        } else {
            while (tc0 >= p.C) {
                tc0 -= p.C;
                if (++tts == Sc) { tts = 0; ++ttr; }
            }
        }
    };

    // LDS fragment offsets within a stage (K sub-step 0 of the first 64-byte half).  Fragment mi / ni sits mi (ni) * FR rows below
    // fragment 0 at the same swizzle (FR rows change neither (row >> 2) & 3 nor (row >> 1) & 7): one register per operand + immediates.
    // bf16 sub-step s reads chunk 2 s + lk: an XOR of the offset with 32 s; the second 64-byte half of a 128-byte row (KC = 8): XOR 64.
    const int fa0 = KC == 4 ? lds_off(wm * WMR + lr, lk) : lds_off128(wm * WMR + lr, lk);
    const int fw0 = A_BYTES + (KC == 4 ? lds_off(wn * WN + lr, lk) : lds_off128(wn * WN + lr, lk));

    // bf16: fragment reads as assembly statements in a fixed order, MFMA groups released by counted waits (see lds_rd128 above).  Per
    // 64-byte half: sub-steps s = 0, 1 (K = 16 each), per sub-step W fragment 0, every A fragment, the other W fragments -- all
    // KSUB * (MT_ + NT_) reads of the half in flight before the first MFMA.  fp32 (parity mode) keeps the compiler's schedule: its
    // 16x16x4 MFMAs take 32 cycles each, an LDS round trip hides behind any group of them.
    constexpr bool ASM_FRAGS = sizeof(T) == 2;
    constexpr int RPH = KSUB * (MT_ + NT_);      // reads per 64-byte half
    // (16 reads: the counter holds 15, the sixteenth issues once the first -- they return in order -- has landed, which is what lgkmcnt(15) then asks for)
    static_assert(RPH <= 16, "lgkmcnt counts 15 operations");
    const uint32_t lds0 = lds_addr32(smem);
    auto frag_reads = [&](int stage, auto KS, u32x4 (&af)[KSUB][MT_], u32x4 (&wf)[KSUB][NT_]) __attribute__((always_inline)) {
        constexpr int ks = decltype(KS)::value;
        static_for<0, KSUB>([&](auto S) {
            constexpr int sb = decltype(S)::value;
            const uint32_t a_addr = lds0 + (uint32_t)(stage * STAGE) + (uint32_t)(fa0 ^ (ks * 64 + sb * 32));
            const uint32_t w_addr = lds0 + (uint32_t)(stage * STAGE) + (uint32_t)(fw0 ^ (ks * 64 + sb * 32));
            lds_rd128<0>(wf[sb][0], w_addr);
            static_for<0, MT_>([&](auto MI) { lds_rd128<decltype(MI)::value * FR * ROWB>(af[sb][decltype(MI)::value], a_addr); });
            static_for<1, NT_>([&](auto NI) { lds_rd128<decltype(NI)::value * FR * ROWB>(wf[sb][decltype(NI)::value], w_addr); });
        });
    };
    auto frag_mma = [&](u32x4 (&af)[KSUB][MT_], u32x4 (&wf)[KSUB][NT_]) __attribute__((always_inline)) {
        // read number P (issue order) has landed once lgkmcnt <= RPH - 1 - P.  The scheduling barriers keep each MFMA group above
        // the next wait: left alone, the MFMAs -- which touch no memory -- sink below the later assembly statements and the whole
        // step waits for its last read.
        static_for<0, KSUB>([&](auto S) {
            constexpr int sb = decltype(S)::value;
            constexpr int P0 = sb * (MT_ + NT_);
            static_for<0, MT_>([&](auto MI) {
                constexpr int mi = decltype(MI)::value;
                lgkm_release<RPH - 1 - (P0 + 1 + mi)>(wf[sb][0], af[sb][mi]);
                MM::run(acc[0][mi], wf[sb][0], af[sb][mi]);
                __builtin_amdgcn_sched_barrier(0);
            });
            static_for<1, NT_>([&](auto NI) {
                constexpr int ni = decltype(NI)::value;
                lgkm_release<RPH - 1 - (P0 + MT_ + ni)>(wf[sb][ni]);
#pragma unroll
                for (int mi = 0; mi < MT_; ++mi) MM::run(acc[ni][mi], wf[sb][ni], af[sb][mi]);
                __builtin_amdgcn_sched_barrier(0);
            });
        });
    };
    auto compute = [&](int stage) {
        const char* base = smem + stage * STAGE;
#pragma unroll
        for (int ks = 0; ks < KC / 4; ++ks) {        // the swizzle is an XOR, so the second 64-byte half is offset ^ 64
#pragma unroll
            for (int sb = 0; sb < KSUB; ++sb) {
                u32x4 af[MT_], wf[NT_];
#pragma unroll
                for (int mi = 0; mi < MT_; ++mi) af[mi] = ld_chunk(base + (fa0 ^ (ks * 64 + sb * 32)) + mi * FR * ROWB);
#pragma unroll
                for (int ni = 0; ni < NT_; ++ni) wf[ni] = ld_chunk(base + (fw0 ^ (ks * 64 + sb * 32)) + ni * FR * ROWB);
#pragma unroll
                for (int ni = 0; ni < NT_; ++ni)
#pragma unroll
                    for (int mi = 0; mi < MT_; ++mi) MM::run(acc[ni][mi], wf[ni], af[mi]);
            }
        }
    };

#ifdef SAICV_NT_TIMELINE
    if (tl_on) { int t_ = kpos + fa0; asm volatile("" : "+v"(t_)); NT_STAMP(10); }
#endif
    const int nkt = (Kc + BK - 1) / BK;        // 0 for a class without taps: the output is zero
    // r05 -- the bias starts the accumulators: out = bias + sum, and the epilogue's 16 masked loads + adds per thread behind the K loop
    // (1.5 us of a 27 us ViT-B tile, profiles/r05_nt_timeline.md) are gone.  The four values per 16-column fragment were requested
    // at the top of the tile (bias_v, a compiler-visible load: an assembly load would be spilled before it has landed) and are consumed
    // HERE, before the first DMA is issued, so that the wait the compiler places does not drain the DMA ring.
    if (bias_early) {
#pragma unroll
        for (int ni = 0; ni < NT_; ++ni)
#pragma unroll
            for (int mi = 0; mi < MT_; ++mi)
#pragma unroll
                for (int r = 0; r < MM::NV; ++r) acc[ni][mi][r] = __uint_as_float(bias_v[ni][r / 4][r % 4]);
    }
    // prologue: NSTAGE-1 tiles in flight
    int issued = 0;
    for (; issued < NSTAGE - 1 && issued < nkt; ++issued) issue_tile(issued);
    NT_STAMP(1);
    int st_c = 0;                              // ring slot of the tile being consumed
    int st_i = issued % NSTAGE;                // ring slot the next DMA fills
    for (int kt = 0; kt < nkt; ++kt) {
        // retire tile kt only: the tiles issued after it stay in flight across the barrier
        const int ahead = issued - kt - 1;     // wave-uniform
        if (ahead >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LPT) : "memory");
        else if (ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPT) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();          // everyone's part of tile kt landed; tile kt-1 fully consumed
#ifdef SAICV_NT_TIMELINE
        if (kt == 0) NT_STAMP(2);
#endif
        if constexpr (ASM_FRAGS) {
            u32x4 af[KSUB][MT_], wf[KSUB][NT_];
            frag_reads(st_c, std::integral_constant<int, 0>{}, af, wf);      // the first fragments travel while the DMA below is issued
            if (issued < nkt) {                // refill the slot tile kt-1 just vacated
                issue_tile(st_i);
                ++issued;
                st_i = (st_i + 1 == NSTAGE) ? 0 : st_i + 1;
            }
            frag_mma(af, wf);
            if constexpr (KC == 8) {
                frag_reads(st_c, std::integral_constant<int, 1>{}, af, wf);
                frag_mma(af, wf);
            }
        } else {
            if (issued < nkt) {                // refill the slot tile kt-1 just vacated
                issue_tile(st_i);
                ++issued;
                st_i = (st_i + 1 == NSTAGE) ? 0 : st_i + 1;
            }
            compute(st_c);
        }
        st_c = (st_c + 1 == NSTAGE) ? 0 : st_c + 1;
    }
    }
    __syncthreads();                           // LDS is reused by the epilogue
    NT_STAMP(3);

    // ---- epilogue.  acc[ni][mi][r]: n = n_base + ni*FR + fcol(r / 4) + r % 4 ; m = m_base + mi*FR + lr
    // BN statistics come straight from the accumulators; the output tile is staged through LDS
    // so that HBM sees whole rows written 16 bytes per lane (a lane's fragment is only 4 values
    // of one row: storing it directly gives 32- or 64-byte row segments and half the write bandwidth -- measured).
    // CODE SIZE is what this section is tuned for: with one workgroup per CU nothing overlaps the epilogue, and a
    // fully unrolled epilogue that carries every fused mode in every unrolled copy (6 k instructions, 48 KiB)
    // spent most of its 6 us per tile waiting for instruction fetch.  So: the unrolled part (accumulator -> LDS)
    // carries no alternatives, the common copy-out is 16 loads + 16 stores, and everything with a fused operand,
    // a row remap, an N tail or an unaligned leading dimension runs in ROLLED loops (one copy of the mode code).
    // the thread coordinates of the epilogue are re-derived from an opaque copy of the thread index: nothing of the epilogue's
    // address arithmetic can be hoisted above the K loop and held in registers (or spilled) across it
    int tid_e = threadIdx.x;
    asm volatile("" : "+v"(tid_e));
    {
    const int tid = tid_e;
    const int lane = tid & 63;
    const int l15 = lane & 15;
    const int lg = lane >> 4;
    const int lr = lane & (FR - 1);
    const int lk = lane / FR;
    auto fcol = [&](int g) { return FR == 32 ? 8 * g + 4 * lk : 4 * lk; };
    typedef typename std::conditional<OUT_F32, float, T>::type TO;
    constexpr int OPITCH = BN_T * (int)sizeof(TO) + 16;         // bytes; +16 staggers banks
    constexpr int OCPR = BN_T * (int)sizeof(TO) / 16;           // 16-byte chunks per tile row
    constexpr int OEPC = 16 / (int)sizeof(TO);
    const int m_base = tile_m * BM_T + wm * WMR;
    const int n_base = tile_n * BN_T + wn * WN;
    const bool do_stats = p.stat_sum != nullptr;
    // bf16 outputs: the BN statistics are taken from the STAGED tile by the matrix cores (below), not here
    constexpr bool MSTAT = !OUT_F32 && sizeof(T) == 2;
    const bool valu_stats = do_stats && !MSTAT;
#pragma unroll
    for (int ni = 0; ni < NT_; ++ni) {
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const int n0 = n_base + ni * FR + fcol(g);
            float bs[4] = {0.f, 0.f, 0.f, 0.f};
            if (p.bias != nullptr && !bias_early) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (n0 + r < p.Nn) bs[r] = p.bias[n0 + r];
            }
            float ssum[4] = {0.f, 0.f, 0.f, 0.f}, ssq[4] = {0.f, 0.f, 0.f, 0.f};
            char* q0 = smem + (wm * WMR + lr) * OPITCH + (wn * WN + ni * FR + fcol(g)) * (int)sizeof(TO);
#pragma unroll
            for (int mi = 0; mi < MT_; ++mi) {
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = acc[ni][mi][4 * g + r] + bs[r];
                if (valu_stats) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float vr = OUT_F32 ? v[r] : round_through<T>(v[r]);
                        ssum[r] += vr;
                        ssq[r] += vr * vr;
                    }
                }
                char* q = q0 + mi * FR * OPITCH;
                if (sizeof(TO) == 2) {
                    bf16x4 pk;
#pragma unroll
                    for (int r = 0; r < 4; ++r) pk[r] = (bf16_t)v[r];
                    *reinterpret_cast<bf16x4*>(q) = pk;
                } else {
                    *reinterpret_cast<f32x4*>(q) = f32x4{v[0], v[1], v[2], v[3]};
                }
            }
            if (valu_stats) {
                // rows m >= M were gathered as zeros (no bias when stats are requested) -> add 0.
#pragma unroll
                for (int r = 0; r < 4; ++r) {        // over the FR pixel lanes that share these columns
                    ssum[r] = row16_sum(ssum[r]);
                    ssq[r] = row16_sum(ssq[r]);
                    if (FR == 32) {
                        ssum[r] += __shfl_xor(ssum[r], 16, 64);
                        ssq[r] += __shfl_xor(ssq[r], 16, 64);
                    }
                }
                if (lr == 0) {                       // per-wavefront column sums -> LDS [2][WM_][BN_T] behind the staged tile
                    float* ws = reinterpret_cast<float*>(smem + BM_T * OPITCH) + wm * BN_T + wn * WN + ni * FR + fcol(g);
                    *reinterpret_cast<f32x4*>(ws) = f32x4{ssum[0], ssum[1], ssum[2], ssum[3]};
                    *reinterpret_cast<f32x4*>(ws + WM_ * BN_T) = f32x4{ssq[0], ssq[1], ssq[2], ssq[3]};
                }
            }
        }
    }
    __syncthreads();
    NT_STAMP(4);
    if constexpr (MSTAT) {
        if (do_stats) {
            // Column sums of the staged bf16 tile on the matrix cores: with Y the [32 rows][16 cols] block read
            // TRANSPOSED from LDS (ds_read_b64_tr_b16: lane (col, k-group) gets 8 consecutive rows of its column),
            //   sum_m y      = (1 . Y)[any row][col]          -- A = ones
            //   sum_m y * y  = (Y^T . Y)[col][col]            -- A = B = the same fragment, the diagonal
            // exact products, fp32 accumulation, and exactly the values the next kernel reads (bf16-rounded).
            // One wavefront owns 16 columns over ALL rows of the tile: no cross-wave combine, and the 14 VALU
            // operations per output element + 128 DPP adds of the accumulator version are gone from the epilogue.
            typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
            const u32x4 ones = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};
            for (int cg = wave; cg < BN_T / 16; cg += NWAVES) {
                f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
                const char* q = smem + (lg * 8 + (l15 >> 2)) * OPITCH + (cg * 16 + (l15 & 3) * 4) * 2;
#pragma unroll 4
                for (int rb = 0; rb < BM_T / 32; ++rb, q += 32 * OPITCH) {
                    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(q));
                    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(q + 4 * OPITCH));
                    const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
                    const u32x4 y = {l2[0], l2[1], h2[0], h2[1]};
                    Mma<T>::run(s1, ones, y);
                    Mma<T>::run(s2, y, y);
                }
                const int n = tile_n * BN_T + cg * 16 + l15;          // D: row lg*4 + r, column l15
                if (n < p.Nn) {
                    const size_t srow = p.stat_atomic_rows ? (size_t)(tile_m % p.stat_atomic_rows) : (size_t)tile_m;
                    if (lg == 0) {
                        if (p.stat_atomic_rows) unsafeAtomicAdd(&p.stat_sum[srow * (size_t)p.Nn + n], s1[0]);
                        else p.stat_sum[srow * (size_t)p.Nn + n] = s1[0];
                    }
                    if (lg == (l15 >> 2)) {
                        const int r = l15 & 3;
                        const float qv = r == 0 ? s2[0] : r == 1 ? s2[1] : r == 2 ? s2[2] : s2[3];
                        if (p.stat_atomic_rows) unsafeAtomicAdd(&p.stat_sq[srow * (size_t)p.Nn + n], qv);
                        else p.stat_sq[srow * (size_t)p.Nn + n] = qv;
                    }
                }
            }
        }
    } else
    if (do_stats) {
        // one row of partial statistics per WORKGROUP (fixed summation order over its wavefront rows): four times
        // fewer partial rows for the finalize kernels to read than one row per wavefront row
        for (int c = tid; c < 2 * BN_T; c += NTHREADS) {
            const int which = c / BN_T, col = c - which * BN_T;
            const float* ws = reinterpret_cast<const float*>(smem + BM_T * OPITCH) + which * WM_ * BN_T + col;
            float a = 0.f;
#pragma unroll
            for (int w = 0; w < WM_; ++w) a += ws[w * BN_T];
            const int n = tile_n * BN_T + col;
            if (n < p.Nn) {
                float* dst = (which ? p.stat_sq : p.stat_sum) +
                             (size_t)(p.stat_atomic_rows ? tile_m % p.stat_atomic_rows : tile_m) * (size_t)p.Nn + n;
                if (p.stat_atomic_rows) unsafeAtomicAdd(dst, a); else *dst = a;
            }
        }
    }
    NT_STAMP(5);
    const bool stream_out = p.stream_out != 0;      // uniform
    const int oc = tid % OCPR;               // chunk within the tile row
    const int orow0 = tid / OCPR;
    constexpr int RPP = NTHREADS / OCPR;     // tile rows per pass
    constexpr int NIT = BM_T / RPP;
    const int ncol = tile_n * BN_T + oc * OEPC;
    TO* const outp = reinterpret_cast<TO*>(p.out);
    const bool aligned = ((p.ldo * (int)sizeof(TO)) & 15) == 0;
    const bool remap = MODE == 1 && cs > 1;
    constexpr bool DGRAD_EXTRAS = MODE == 1 && sizeof(TO) == sizeof(T);       // gated shortcut / BatchNorm-backward sums: data gradient only
    const bool bstats = DGRAD_EXTRAS && p.bs_y != nullptr;                                                        // uniform
    const bool plain = aligned && !remap && p.act_mode == 0 && p.addend == nullptr && p.row_scale == nullptr && !bstats;   // uniform
    float bag[OEPC], bax[OEPC];                                // this thread's sum g, sum g * y over its rows of the tile
#pragma unroll
    for (int j = 0; j < OEPC; ++j) { bag[j] = 0.f; bax[j] = 0.f; }
    if (plain && ncol + OEPC <= p.Nn) {
        // the common case: a branch-free copy, the LDS reads of eight rows in flight before the first store
        constexpr int GRP = NIT < 8 ? NIT : 8;
        const int mrow0 = tile_m * BM_T + orow0;
        const char* ls = smem + orow0 * OPITCH + oc * 16;
        TO* o = outp + (size_t)mrow0 * p.ldo + ncol;
        const size_t ostep = (size_t)RPP * p.ldo;
        const bool full = (tile_m + 1) * BM_T <= Mc;                                         // uniform
#pragma unroll
        for (int g = 0; g < NIT; g += GRP) {
            u32x4 v[GRP];
#pragma unroll
            for (int j = 0; j < GRP; ++j) v[j] = ld_chunk(ls + (g + j) * RPP * OPITCH);
            if (full) {
#pragma unroll
                for (int j = 0; j < GRP; ++j) NT_OUT_ST(o + (g + j) * ostep, v[j]);
            } else {
#pragma unroll
                for (int j = 0; j < GRP; ++j)
                    if (mrow0 + (g + j) * RPP < Mc) NT_OUT_ST(o + (g + j) * ostep, v[j]);
            }
        }
    } else if (aligned && !remap && (p.act_mode == 0 || p.act_mode == 4) && (p.Nn % OEPC) == 0) {   // uniform
        // residual add / drop-path scale (forward and data gradient) and the data gradient's gated shortcut and
        // BatchNorm-backward sums, on dense rows of whole chunks: four rows at a time, every global load of the group
        // (addend, y, the two mask bytes) in flight before the first use
        if (ncol < p.Nn) {
            constexpr int GRP = NIT < 4 ? NIT : 4;
            const int mrow0 = tile_m * BM_T + orow0;
            const char* ls = smem + orow0 * OPITCH + oc * 16;
            const bool addp = p.addend != nullptr, scalep = p.row_scale != nullptr;
            const bool mulp = p.act_mode == 4;          // out = (acc + bias) * addend: the stored gelu'() of an MLP (grouped loads instead of the rolled loop)
            const bool gatep = DGRAD_EXTRAS && p.addend_gate != nullptr, maskp = DGRAD_EXTRAS && p.bs_mask != nullptr;
            const TO* const addend = reinterpret_cast<const TO*>(p.addend);
            const TO* const ybn = reinterpret_cast<const TO*>(p.bs_y);
#pragma unroll 1
            for (int g = 0; g < NIT; g += GRP) {
                u32x4 v[GRP], av[GRP], yv[GRP];
                unsigned gb[GRP], mb[GRP];
                float sc[GRP];
#pragma unroll
                for (int j = 0; j < GRP; ++j) {
                    const int mrow = mrow0 + (g + j) * RPP;
                    const bool ok = mrow < Mc;
                    const size_t off = (size_t)mrow * p.ldo + ncol;
                    v[j] = ld_chunk(ls + (g + j) * RPP * OPITCH);
                    av[j] = u32x4{0u, 0u, 0u, 0u};
                    yv[j] = u32x4{0u, 0u, 0u, 0u};
                    gb[j] = 0xffu;
                    mb[j] = 0xffu;
                    sc[j] = 1.f;
                    if (ok) {
                        if (scalep) sc[j] = p.row_scale[mrow / p.rows_per_scale];
                        if (addp) av[j] = NT_EPI_LD(addend + off);
                        if (bstats) yv[j] = NT_EPI_LD(ybn + off);
                        if (gatep) gb[j] = p.addend_gate[off / OEPC];
                        if (bstats && maskp) mb[j] = p.bs_mask[off / OEPC];
                    }
                }
#pragma unroll
                for (int j = 0; j < GRP; ++j) {
                    const int mrow = mrow0 + (g + j) * RPP;
                    if (mrow < Mc) {
                        float f[OEPC];
                        Chunk<TO>::unpack(v[j], f);
                        if (addp || scalep) {
                            float a[OEPC];
                            Chunk<TO>::unpack(av[j], a);
                            if (mulp) {
#pragma unroll
                                for (int e = 0; e < OEPC; ++e) f[e] *= a[e];
                            } else {
#pragma unroll
                                for (int e = 0; e < OEPC; ++e) f[e] = fmaf(sc[j], f[e], ((gb[j] >> e) & 1u) ? a[e] : 0.f);
                            }
                            v[j] = Chunk<TO>::pack(f);
                            if (bstats) Chunk<TO>::unpack(v[j], f);      // the sums are over what is stored
                        }
                        if (bstats) {
                            float yy[OEPC];
                            Chunk<TO>::unpack(yv[j], yy);
#pragma unroll
                            for (int e = 0; e < OEPC; ++e) {
                                const float ge = ((mb[j] >> e) & 1u) ? f[e] : 0.f;
                                bag[e] += ge;
                                bax[e] = fmaf(ge, yy[e], bax[e]);
                            }
                        }
                        NT_OUT_ST(outp + (size_t)mrow * p.ldo + ncol, v[j]);
                    }
                }
            }
        }
    } else if (p.lean_gelu && aligned && !remap && (p.act_mode == 1 || p.act_mode == 3) && p.addend == nullptr && p.row_scale == nullptr && !bstats &&
               (p.Nn % OEPC) == 0) {   // uniform
        // fc1 of an MLP (r04): out = the pre-activation (1) or gelu'(pre) (3), out2 = gelu(pre).  Nothing but the staged tile is read,
        // so the row loop is just unpack -> packed-fp32 GELU pieces -> two packs -> two 16-byte stores: 322 -> ~150 vector
        // instructions per row of eight against the general rolled loop below (an epilogue instruction competes with the other
        // workgroup's MFMAs for the issue port)
        if (ncol < p.Nn) {
            const int mrow0 = tile_m * BM_T + orow0;
            const char* ls = smem + orow0 * OPITCH + oc * 16;
            TO* const o2 = reinterpret_cast<TO*>(p.out2);
            const bool emit_grad = p.act_mode == 3;
#pragma unroll 2
            for (int g = 0; g < NIT; ++g) {
                const int mrow = mrow0 + g * RPP;
                if (mrow < Mc) {
                    const u32x4 v = ld_chunk(ls + g * RPP * OPITCH);
                    float f[OEPC], gl[OEPC], gr[OEPC];
                    Chunk<TO>::unpack(v, f);
                    gelu_and_grad8(f, gl, gr);
                    const size_t off = (size_t)mrow * p.ldo + ncol;
                    NT_OUT_ST(o2 + off, Chunk<TO>::pack(gl));
                    NT_OUT_ST(outp + off, emit_grad ? Chunk<TO>::pack(gr) : v);
                }
            }
        }
    } else if (ncol < p.Nn) {
        // one copy of the fused-mode code in a ROLLED loop; the staged chunk and the addend chunk of the NEXT row are
        // fetched before the current row is processed, so a row's global-load latency hides under its predecessor
        const bool whole = aligned && ncol + OEPC <= p.Nn;
        const bool pre_add = whole && p.addend != nullptr;
        const bool gated = DGRAD_EXTRAS && pre_add && p.addend_gate != nullptr;   // host: the gate needs whole, aligned chunks
        const bool bst = bstats && whole;
        // per row: gate byte of the addend (bits 0-7) | ReLU-mask byte of the statistics (bits 8-15)
        auto side_bits = [&](int mrow) -> unsigned {
            const size_t ch = ((size_t)mrow * p.ldo + ncol) / OEPC;
            unsigned b = 0xffffu;
            if (gated) b = (b & 0xff00u) | p.addend_gate[ch];
            if (bst && p.bs_mask != nullptr) b = (b & 0x00ffu) | ((unsigned)p.bs_mask[ch] << 8);
            return b;
        };
        auto out_row = [&](int rr) -> int {                // output row of tile row rr, -1 past the end
            const int mrow = tile_m * BM_T + rr;
            if (rr >= BM_T || mrow >= Mc) return -1;
            if (!remap) return mrow;
            const int img = mrow / ohw;
            const int rem = mrow - img * ohw;
            const int hc = rem / Wc;
            return (img * p.OH + hc * cs + ph) * p.OW + (rem - hc * Wc) * cs + pw;
        };
        int rr = orow0;
        int m = out_row(rr);
        u32x4 v = {0u, 0u, 0u, 0u}, av = {0u, 0u, 0u, 0u}, yv = {0u, 0u, 0u, 0u};
        unsigned sb = 0xffffu;
        if (m >= 0) {
            v = ld_chunk(smem + rr * OPITCH + oc * 16);
            if (pre_add) av = ld_chunk(reinterpret_cast<const TO*>(p.addend) + (size_t)m * p.ldo + ncol);
            if (bst) yv = ld_chunk(reinterpret_cast<const TO*>(p.bs_y) + (size_t)m * p.ldo + ncol);
            if (gated || bst) sb = side_bits(m);
        }
#pragma unroll 1
        while (m >= 0) {
            const int rn = rr + RPP;
            const int mn = out_row(rn);
            u32x4 vn = {0u, 0u, 0u, 0u}, an = {0u, 0u, 0u, 0u}, yn = {0u, 0u, 0u, 0u};
            unsigned sbn = 0xffffu;
            if (mn >= 0) {
                vn = ld_chunk(smem + rn * OPITCH + oc * 16);
                if (pre_add) an = ld_chunk(reinterpret_cast<const TO*>(p.addend) + (size_t)mn * p.ldo + ncol);
                if (bst) yn = ld_chunk(reinterpret_cast<const TO*>(p.bs_y) + (size_t)mn * p.ldo + ncol);
                if (gated || bst) sbn = side_bits(mn);
            }
            TO* o = outp + (size_t)m * p.ldo + ncol;
            if (p.act_mode == 1 || p.act_mode == 3) {   // fc1 of an MLP: emit gelu() beside the pre-activation (1) or beside gelu'() (3)
                float f[OEPC], gl[OEPC], gr[OEPC];
                Chunk<TO>::unpack(v, f);
                gelu_and_grad8(f, gl, gr);
                NT_OUT_ST(reinterpret_cast<TO*>(p.out2) + (size_t)m * p.ldo + ncol, Chunk<TO>::pack(gl));
                if (p.act_mode == 3) v = Chunk<TO>::pack(gr);
            } else if (p.act_mode == 2 || p.act_mode == 4) {     // dgrad of fc2: d pre-activation = d act * gelu'(pre) (2) or * the stored derivative (4)
                float f[OEPC], a[OEPC];
                Chunk<TO>::unpack(v, f);
                Chunk<TO>::unpack(av, a);
                if (p.act_mode == 2) {
#pragma unroll
                    for (int j = 0; j < OEPC; ++j) f[j] *= gelu_grad_f(a[j]);
                } else {
#pragma unroll
                    for (int j = 0; j < OEPC; ++j) f[j] *= a[j];
                }
                v = Chunk<TO>::pack(f);
            } else if (p.addend != nullptr || p.row_scale != nullptr) {
                float f[OEPC], a[OEPC];
                Chunk<TO>::unpack(v, f);
                const float sc = p.row_scale ? p.row_scale[m / p.rows_per_scale] : 1.f;
                if (pre_add) {
                    Chunk<TO>::unpack(av, a);
                    if (gated) {
#pragma unroll
                        for (int j = 0; j < OEPC; ++j) a[j] = ((sb >> j) & 1u) ? a[j] : 0.f;
                    }
                } else {
                    for (int j = 0; j < OEPC; ++j)
                        a[j] = (p.addend != nullptr && ncol + j < p.Nn)
                                   ? to_f32(reinterpret_cast<const TO*>(p.addend)[(size_t)m * p.ldo + ncol + j]) : 0.f;
                }
#pragma unroll
                for (int j = 0; j < OEPC; ++j) f[j] = fmaf(sc, f[j], a[j]);
                v = Chunk<TO>::pack(f);
            }
            if (bst) {                        // BatchNorm-backward sums of what is stored (rounded to TO), behind its ReLU gate
                float f[OEPC], yy[OEPC];
                Chunk<TO>::unpack(v, f);
                Chunk<TO>::unpack(yv, yy);
#pragma unroll
                for (int j = 0; j < OEPC; ++j) {
                    const float gj = ((sb >> (8 + j)) & 1u) ? f[j] : 0.f;
                    bag[j] += gj;
                    bax[j] = fmaf(gj, yy[j], bax[j]);
                }
            }
            if (whole) {
                NT_OUT_ST(o, v);
            } else {                          // N tail, or a leading dimension without 16-byte alignment
                const TO* e = reinterpret_cast<const TO*>(&v);
                for (int j = 0; j < OEPC; ++j)
                    if (ncol + j < p.Nn) o[j] = e[j];
            }
            rr = rn; m = mn; v = vn; av = an; yv = yn; sb = sbn;
        }
    }
    if (bstats) {       // uniform: combine the row lanes of every column through the (now consumed) staging area
        __syncthreads();
        float* red = reinterpret_cast<float*>(smem);                      // [RPP][2][BN_T]
        const bool have = ncol + OEPC <= p.Nn;
#pragma unroll
        for (int j = 0; j < OEPC; ++j) {
            // sum g * (y - mean) * invstd = invstd * (sum g y - mean * sum g): the mean leaves after this thread's few
            // rows (BM_T / RPP of them), while the sums are still small -- not after the whole column
            const float mu = have ? p.bs_mean[ncol + j] : 0.f, is = have ? p.bs_invstd[ncol + j] : 0.f;
            red[(orow0 * 2 + 0) * BN_T + oc * OEPC + j] = bag[j];
            red[(orow0 * 2 + 1) * BN_T + oc * OEPC + j] = is * fmaf(-mu, bag[j], bax[j]);
        }
        __syncthreads();
        const size_t prow = (size_t)((MODE == 1 && cs > 1) ? blockIdx.y : 0) * p.bs_rows + tile_m;
        for (int c = tid; c < 2 * BN_T; c += NTHREADS) {
            const int which = c / BN_T, col = c - which * BN_T;
            float a = 0.f;
            for (int r = 0; r < RPP; ++r) a += red[(r * 2 + which) * BN_T + col];
            const int n = tile_n * BN_T + col;
            if (n < p.Nn) {
                float* dst = (which ? p.bs_gx : p.bs_g) + (p.stat_atomic_rows ? prow % p.stat_atomic_rows : prow) * (size_t)p.Nn + n;
                if (p.stat_atomic_rows) unsafeAtomicAdd(dst, a); else *dst = a;
            }
        }
    }
    }   // epilogue scope
#ifdef SAICV_NT_TIMELINE
    if (tl_on && tix == (int)blockIdx.x) {
        NT_STAMP(6);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the workgroup's stores are acknowledged
        NT_STAMP(7);
        if (tid == 0) {
            unsigned long long* rec = p.timeline + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 16;
            unsigned int hw, xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
#pragma unroll
            for (int i = 0; i < 8; ++i) rec[i] = tl_t[i];
            rec[8] = ((unsigned long long)xcc << 32) | hw;
            rec[9] = __builtin_amdgcn_s_memrealtime();
            rec[10] = tl_rt0;
            rec[11] = tl_t[8]; rec[12] = tl_t[9]; rec[13] = tl_t[10];
        }
    }
#endif
    }   // tile loop
}


// ------------------------------------------------------------------------------------ TN
struct TNParams {
    const void* dy;     // [M][Cout]
    const void* src;    // [Nimg,H,W,C] gather source (layer input)
    float* dw;          // [Cout][Kd] fp32, accumulated with atomics
    float* dbias;       // optional [Cout] fp32: column sums of dy (bias gradient), accumulated
    uint32_t dy_bytes, src_bytes;
    int H, W, C;
    int OH, OW;
    int R, S, stride, pad;
    int M, Cout, Kd;
    int tiles_a, tiles_b;       // tiles over Cout / over Kd
    int m_per_split;            // multiple of BR
    int d_img, d_oh, d_ow;      // mixed-radix digits of BR in (img, oh, ow)
    FastDiv fd_ohw, fd_ow;
    saicv::DetSink det;         // deterministic mode: split s parks its tile in part[s][n * Kd + kk], its bias sums in part[s][Cout * Kd + n]
};

template <typename T, int BA, int BB, int NWA, int NWB>
__global__ __launch_bounds__(64 * NWA * NWB) void igemm_tn_kernel(const TNParams p) {
    constexpr int THREADS = 64 * NWA * NWB;
    constexpr int EPC = ElemTraits<T>::EPC;
    constexpr int BR = 8 * EPC;                  // reduction rows per tile (64 bf16 / 32 f32)
    constexpr int PITCH_A = (BA + 16) * (int)sizeof(T);
    constexpr int PITCH_B = (BB + 16) * (int)sizeof(T);
    constexpr int A_BYTES = BR * PITCH_A;
    constexpr int B_BYTES = BR * PITCH_B;
    constexpr int STAGE = A_BYTES + B_BYTES;
    constexpr int CPR_A = BA / EPC, CPR_B = BB / EPC;     // chunks per row
    constexpr int RPP_A = THREADS / CPR_A, RPP_B = THREADS / CPR_B;
    constexpr int NA = BR / RPP_A, NB = BR / RPP_B;       // chunks per thread
    constexpr int WA = BA / NWA, WB = BB / NWB;
    constexpr int AT = WA / 16, BT = WB / 16;
    constexpr uint32_t OOB = 0xfffffff0u;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wa = wave % NWA, wb = wave / NWA;
    const int l15 = lane & 15, lg = lane >> 4;

    // XCD-aware mapping: workgroups are dealt to the 8 XCDs round-robin in launch order (x fastest).  All output
    // tiles of one reduction split read the SAME rows of dY and of the gather source, so each XCD gets a contiguous
    // range of (split, tile) pairs in split-major order: those rows are fetched into one L2 instead of eight
    // (PMC: the weight-gradient kernels read 25 GB per ResNet-50 step against 11 GB of operands).
    const int ntile = gridDim.x;
    const int lid = xcd_remap(blockIdx.y * ntile + blockIdx.x, ntile * gridDim.y);
    const int split = lid / ntile;
    const int tile = lid - split * ntile;
    const int tile_a = tile % p.tiles_a;
    const int tile_b = tile / p.tiles_a;
    const int m_begin = split * p.m_per_split;
    const int m_end = min(p.M, m_begin + p.m_per_split);
    if (m_begin >= m_end) return;

    const __amdgpu_buffer_rsrc_t dy_rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.dy), 0, p.dy_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t src_rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.src), 0, p.src_bytes, 0x00020000);

    // dY loader state: byte offset of this thread's chunk in row (m_begin + rba), advanced per tile
    const int ca = tid % CPR_A, rba = tid / CPR_A;
    const int n_ld = tile_a * BA + ca * EPC;
    const bool n_ok = n_ld < p.Cout;
    uint32_t dy_off = (uint32_t)((m_begin + rba) * p.Cout + n_ld) * (uint32_t)sizeof(T);
    const uint32_t dy_row_step = (uint32_t)(RPP_A * p.Cout) * (uint32_t)sizeof(T);
    const uint32_t dy_tile_step = (uint32_t)(BR * p.Cout) * (uint32_t)sizeof(T);
    int m_a = m_begin + rba;
    // gather loader state
    const int cb = tid % CPR_B, rbb = tid / CPR_B;
    const int kk_ld = tile_b * BB + cb * EPC;
    const bool kk_ok = kk_ld < p.Kd;
    const int tap = kk_ld / p.C;
    const int c0 = kk_ld - tap * p.C;
    const int fr = tap / p.S - p.pad;            // tap offsets with the padding folded in
    const int fs = tap - (tap / p.S) * p.S - p.pad;
    int g_img[NB], g_oh[NB], g_ow[NB];
    const int ohw = p.OH * p.OW;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int m = m_begin + rbb + RPP_B * i;
        const int img = (int)fdiv((uint32_t)m, p.fd_ohw);
        const int rem = m - img * ohw;
        g_img[i] = img;
        g_oh[i] = (int)fdiv((uint32_t)rem, p.fd_ow);
        g_ow[i] = rem - g_oh[i] * p.OW;
    }
    int m_b = m_begin + rbb;

    u32x4 ra[NA], rbv[NB];
    // bias gradient for free: the workgroups of the first kk tile also sum the dY chunks they stream
    const bool do_bias = (p.dbias != nullptr) && (tile_b == 0);
    float bsum[EPC];
#pragma unroll
    for (int k = 0; k < EPC; ++k) bsum[k] = 0.f;
    auto load_tile = [&]() {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const bool ok = n_ok & (m_a + RPP_A * i < m_end);
            ra[i] = buf_ld(dy_rs, ok ? dy_off + (uint32_t)i * dy_row_step : OOB);
        }
        dy_off += dy_tile_step;
        m_a += BR;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int ih = g_oh[i] * p.stride + fr;
            const int iw = g_ow[i] * p.stride + fs;
            const bool ok = kk_ok & (m_b + RPP_B * i < m_end) & ((unsigned)ih < (unsigned)p.H) &
                            ((unsigned)iw < (unsigned)p.W);
            const uint32_t off = (uint32_t)(((g_img[i] * p.H + ih) * p.W + iw) * p.C + c0) * (uint32_t)sizeof(T);
            rbv[i] = buf_ld(src_rs, ok ? off : OOB);
            // advance this row by BR pixels (mixed radix add with carries)
            int ow = g_ow[i] + p.d_ow;
            int cy = ow >= p.OW;
            ow -= cy ? p.OW : 0;
            int oh = g_oh[i] + p.d_oh + cy;
            cy = oh >= p.OH;
            oh -= cy ? p.OH : 0;
            g_ow[i] = ow;
            g_oh[i] = oh;
            g_img[i] += p.d_img + cy;
        }
        m_b += BR;
    };
    int st_a[NA], st_b[NB];
#pragma unroll
    for (int i = 0; i < NA; ++i) st_a[i] = (rba + RPP_A * i) * PITCH_A + ca * 16;
#pragma unroll
    for (int i = 0; i < NB; ++i) st_b[i] = A_BYTES + (rbb + RPP_B * i) * PITCH_B + cb * 16;
    auto store_tile = [&](int stage) {
        char* base = smem + stage * STAGE;
        if (do_bias) {
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                float f[EPC];
                Chunk<T>::unpack(ra[i], f);
#pragma unroll
                for (int k = 0; k < EPC; ++k) bsum[k] += f[k];
            }
        }
#pragma unroll
        for (int i = 0; i < NA; ++i) st_chunk(base + st_a[i], ra[i]);
#pragma unroll
        for (int i = 0; i < NB; ++i) st_chunk(base + st_b[i], rbv[i]);
    };

    f32x4 acc[AT][BT];
#pragma unroll
    for (int ai = 0; ai < AT; ++ai)
#pragma unroll
        for (int bi = 0; bi < BT; ++bi) acc[ai][bi] = f32x4{0.f, 0.f, 0.f, 0.f};

    // LDS fragment offsets (stage 0), hoisted out of the reduction loop
    int fa_off[AT], fb_off[BT];
    if constexpr (sizeof(T) == 2) {
        // ds_read_b64_tr_b16: a 16-lane group reads a [4 rows][16 cols] block; lane t supplies the
        // 8-byte address of row (t>>2), cols (t&3)*4.. and receives column t of the four rows.
        const int row0 = lg * 8 + (l15 >> 2);
#pragma unroll
        for (int ai = 0; ai < AT; ++ai) fa_off[ai] = row0 * PITCH_A + (wa * WA + ai * 16 + (l15 & 3) * 4) * 2;
#pragma unroll
        for (int bi = 0; bi < BT; ++bi) fb_off[bi] = A_BYTES + row0 * PITCH_B + (wb * WB + bi * 16 + (l15 & 3) * 4) * 2;
    } else {
#pragma unroll
        for (int ai = 0; ai < AT; ++ai) fa_off[ai] = lg * PITCH_A + (wa * WA + ai * 16 + l15) * 4;
#pragma unroll
        for (int bi = 0; bi < BT; ++bi) fb_off[bi] = A_BYTES + lg * PITCH_B + (wb * WB + bi * 16 + l15) * 4;
    }

    auto compute = [&](int stage) {
        const char* base = smem + stage * STAGE;
        if constexpr (sizeof(T) == 2) {
            // BR = 64 rows -> two 32-deep k-steps
            typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                u32x4 af[AT], bf[BT];
#pragma unroll
                for (int ai = 0; ai < AT; ++ai) {
                    const char* q = base + fa_off[ai] + ks * 32 * PITCH_A;
                    bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(q));
                    bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(q + 4 * PITCH_A));
                    u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
                    af[ai] = u32x4{l2[0], l2[1], h2[0], h2[1]};
                }
#pragma unroll
                for (int bi = 0; bi < BT; ++bi) {
                    const char* q = base + fb_off[bi] + ks * 32 * PITCH_B;
                    bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(q));
                    bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(q + 4 * PITCH_B));
                    u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
                    bf[bi] = u32x4{l2[0], l2[1], h2[0], h2[1]};
                }
#pragma unroll
                for (int ai = 0; ai < AT; ++ai)
#pragma unroll
                    for (int bi = 0; bi < BT; ++bi)
                        acc[ai][bi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            __builtin_bit_cast(bf16x8, af[ai]), __builtin_bit_cast(bf16x8, bf[bi]),
                            acc[ai][bi], 0, 0, 0);
            }
        } else {
            // f32: BR = 32 rows -> eight 4-deep k-steps of mfma 16x16x4 (lane: row/col l15, k = lg)
#pragma unroll
            for (int ks = 0; ks < BR / 4; ++ks) {
                float af[AT], bf[BT];
#pragma unroll
                for (int ai = 0; ai < AT; ++ai)
                    af[ai] = *reinterpret_cast<const float*>(base + fa_off[ai] + ks * 4 * PITCH_A);
#pragma unroll
                for (int bi = 0; bi < BT; ++bi)
                    bf[bi] = *reinterpret_cast<const float*>(base + fb_off[bi] + ks * 4 * PITCH_B);
#pragma unroll
                for (int ai = 0; ai < AT; ++ai)
#pragma unroll
                    for (int bi = 0; bi < BT; ++bi)
                        acc[ai][bi] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[ai], bf[bi],
                                                                          acc[ai][bi], 0, 0, 0);
            }
        }
    };

    const int nt = (m_end - m_begin + BR - 1) / BR;
    load_tile();
    store_tile(0);
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
        const int cur = t & 1;
        const bool more = (t + 1) < nt;
        if (more) load_tile();
        compute(cur);
        if (more) store_tile(cur ^ 1);
        __syncthreads();
    }

    if (do_bias) {          // combine the RPP_A row lanes of each chunk column through LDS (now free)
        float* red = reinterpret_cast<float*>(smem);
#pragma unroll
        for (int k = 0; k < EPC; ++k) red[tid * EPC + k] = bsum[k];
        __syncthreads();
        if (rba == 0 && n_ok) {
#pragma unroll
            for (int k = 0; k < EPC; ++k) {
                float sgm = 0.f;
                for (int t = 0; t < RPP_A; ++t) sgm += red[(t * CPR_A + ca) * EPC + k];
                saicv::det_add(p.det, p.dbias + n_ld + k, (size_t)p.Cout * p.Kd + n_ld + k, split, sgm);
            }
        }
    }
    // epilogue: D row -> n = .. + lg*4 + r ; D col -> kk = .. + l15
#pragma unroll
    for (int ai = 0; ai < AT; ++ai) {
        const int n0 = tile_a * BA + wa * WA + ai * 16 + lg * 4;
#pragma unroll
        for (int bi = 0; bi < BT; ++bi) {
            const int kk = tile_b * BB + wb * WB + bi * 16 + l15;
            if (kk < p.Kd) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (n0 + r < p.Cout)
                        saicv::det_add(p.det, p.dw + (size_t)(n0 + r) * (size_t)p.Kd + kk, (size_t)(n0 + r) * (size_t)p.Kd + kk, split, acc[ai][bi][r]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------ TN, LDS-DMA ring (bf16)
// The weight-gradient product with the operand stream of the forward kernel: `buffer_load ... lds` writes the dY and
// gather-source rows of a 32-row reduction step straight into a 4-slot LDS ring (no staging registers, no ds_write),
// three steps stay in flight across the single raw s_barrier of a step and the wait is a counted s_waitcnt vmcnt(N).
// The register-staged kernel above keeps ONE step (64 rows) in flight: at one resident 256 x 256 workgroup per CU its
// 0.85 us of MFMA work per step is shorter than a loaded L2/HBM round trip, so its loop runs at the latency, not at the
// matrix cores (620-700 TFLOP/s on the ViT shapes where the forward kernel reaches 800-900).
// LDS image of a step: [32 rows][BA] then [32 rows][BB], rows unpadded (the DMA destination is wave-linear, 1 KiB per
// instruction).  ds_read_b64_tr_b16 is served in 32-lane groups that read rows {R..R+3, R+8..R+11}, 32 bytes each, at
// one column offset: the 32-byte PAIR p of row r lives at pair slot p ^ g(r), g = (r & 3) | ((r >> 3) & 1) << 2 (halved
// for 128-byte rows, where two rows share a 256-byte bank window), so the eight rows hit eight distinct bank groups.
// As everywhere, the swizzle is applied on the SOURCE side: lane l fetches the chunk that belongs in the slot it fills.
// Bias gradient: the workgroups of the first kk tile multiply their dY fragments with a ones operand (AT / NWB extra
// MFMAs per wavefront and step) instead of summing staged registers.
DEVINL int tn_key(int r) { return (r & 3) | (((r >> 3) & 1) << 2); }
template <int CPR> DEVINL int tn_g(int r) { return CPR >= 16 ? tn_key(r) : (tn_key(r) >> 1); }

// Convolution form (PLAIN = false): the gathered operand's byte offset and its (oh, ow) are CARRIED from step to step with adds and selects
// (r05; the r03 form rebuilt the offset from (img, oh, ow) with three 32-bit multiplies per DMA instruction -- 58 full-rate + 10
// quarter-rate vector instructions per 16 MFMAs in the K loop, more issue slots than the MFMAs themselves, profiles/r04_nt_experiments.md
// section 6): ResNet-50 22.01 -> 21.93 ms per step on one box (profiles/r05_nt_experiments.md), host emulation of the recurrence in
// tests/test_r04_host.py, GPU parity in tests/test_gpu_kernels.py.
template <int BA, int BB, int NWA, int NWB, bool PLAIN>
__global__ __launch_bounds__(64 * NWA * NWB) void igemm_tn_dma_kernel(const TNParams p) {
    typedef bf16_t T;
    constexpr int NWAVES = NWA * NWB;
    constexpr int BR = 32;                                 // reduction rows per step: one MFMA k-step
    constexpr int CPR_A = BA / 8, CPR_B = BB / 8;           // 16-byte chunks per row
    constexpr int RPI_A = 64 / CPR_A, RPI_B = 64 / CPR_B;   // rows filled by one DMA wave-instruction
    constexpr int NIA = (BR / RPI_A) / NWAVES, NIB = (BR / RPI_B) / NWAVES;
    static_assert(NIA >= 1 && NIB >= 1 && NIA * NWAVES * RPI_A == BR && NIB * NWAVES * RPI_B == BR, "tile / wavefront split");
    constexpr int LPT = NIA + NIB;                          // loads per thread per step
    constexpr int PITCH_A = BA * 2, PITCH_B = BB * 2;
    constexpr int A_BYTES = BR * PITCH_A, B_BYTES = BR * PITCH_B;
    constexpr int STAGE = A_BYTES + B_BYTES;
    constexpr int NSTAGE = 4;
    constexpr int WA = BA / NWA, WB = BB / NWB;
    constexpr int AT = WA / 16, BT = WB / 16;
    static_assert(AT % NWB == 0, "bias-gradient tiles per wavefront");
    constexpr int ABT = AT / NWB;
    constexpr uint32_t OOB = 0xfffffff0u;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wa = wave % NWA, wb = wave / NWA;
    const int l15 = lane & 15, lg = lane >> 4;

    const int ntile = gridDim.x;
    const int lid = xcd_remap(blockIdx.y * ntile + blockIdx.x, ntile * gridDim.y);
    const int split = lid / ntile;
    const int tile = lid - split * ntile;
    const int tile_a = tile % p.tiles_a;
    const int tile_b = tile / p.tiles_a;
    const int m_begin = split * p.m_per_split;
    const int m_end = min(p.M, m_begin + p.m_per_split);
    if (m_begin >= m_end) return;

    const __amdgpu_buffer_rsrc_t dy_rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.dy), 0, p.dy_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t src_rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.src), 0, p.src_bytes, 0x00020000);

    // ---- per-thread DMA state.  Instruction i of wavefront w fills bytes [(i*NWAVES + w)*1024 + lane*16, +16) of a
    // region: row (i*NWAVES + w)*RPI + lane/CPR, slot lane%CPR, i.e. the logical chunk slot ^ (g(row) << 1)
    uint32_t a_off[NIA];
    int a_m[NIA];
    bool a_ok[NIA];
#pragma unroll
    for (int i = 0; i < NIA; ++i) {
        const int row = (i * NWAVES + wave) * RPI_A + lane / CPR_A;
        const int chunk = (lane % CPR_A) ^ (tn_g<CPR_A>(row) << 1);
        const int n = tile_a * BA + chunk * 8;
        a_ok[i] = n < p.Cout;
        a_m[i] = m_begin + row;
        a_off[i] = (uint32_t)((m_begin + row) * p.Cout + n) * 2u;
    }
    const uint32_t a_step = (uint32_t)(BR * p.Cout) * 2u;
    uint32_t b_off[NIB];                 // byte offset, advanced per step
    int b_m[NIB], g_oh[NIB], g_ow[NIB], b_fr[NIB], b_fs[NIB];
    bool b_ok[NIB];
    const int ohw = p.OH * p.OW;
    // a step moves every DMA row by BR output pixels = (d_img, d_oh, d_ow) in mixed radix; a carry out of the column digit
    // takes OW columns back and adds a row, a carry out of the row digit takes OH rows back and adds an image (wave-uniform scalars)
    const int st_dow = p.stride * p.d_ow, st_ow = p.stride * p.OW, st_doh = p.stride * p.d_oh, st_oh = p.stride * p.OH;     // in input pixels
    const uint32_t inc_base = (uint32_t)(((p.d_img * p.H + st_doh) * p.W + st_dow) * p.C) * 2u;
    const uint32_t inc_cy1 = (uint32_t)((p.stride * p.W - st_ow) * p.C) * 2u;
    const uint32_t inc_cy2 = (uint32_t)(((p.H - st_oh) * p.W) * p.C) * 2u;
#pragma unroll
    for (int j = 0; j < NIB; ++j) {
        const int row = (j * NWAVES + wave) * RPI_B + lane / CPR_B;
        const int chunk = (lane % CPR_B) ^ (tn_g<CPR_B>(row) << 1);
        const int kk = tile_b * BB + chunk * 8;
        b_ok[j] = kk < p.Kd;
        const int m = m_begin + row;
        b_m[j] = m;
        if (PLAIN) {
            b_off[j] = (uint32_t)(m * p.C + kk) * 2u;
            g_oh[j] = g_ow[j] = b_fr[j] = b_fs[j] = 0;
        } else {
            const int tap = kk / p.C;
            const int c0 = kk - tap * p.C;
            b_fr[j] = tap / p.S - p.pad;
            b_fs[j] = tap - (tap / p.S) * p.S - p.pad;
            const int img = (int)fdiv((uint32_t)m, p.fd_ohw);
            const int rem = m - img * ohw;
            g_oh[j] = (int)fdiv((uint32_t)rem, p.fd_ow);
            g_ow[j] = rem - g_oh[j] * p.OW;
            const int ih0 = g_oh[j] * p.stride + b_fr[j], iw0 = g_ow[j] * p.stride + b_fs[j];
            // (wraps when ih / iw are negative: such an offset is never used, `ok` is false there)
            b_off[j] = (uint32_t)(((img * p.H + ih0) * p.W + iw0) * p.C + c0) * 2u;
        }
    }
    const uint32_t b_step = (uint32_t)(BR * p.C) * 2u;

    typedef __attribute__((address_space(3))) void lds_void;
    auto issue_step = [&](int stage) __attribute__((always_inline)) {
        char* base = smem + stage * STAGE + wave * 1024;
#pragma unroll
        for (int i = 0; i < NIA; ++i) {
            const bool ok = a_ok[i] & (a_m[i] < m_end);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(dy_rs, (lds_void*)(base + i * NWAVES * 1024), 16, (int)(ok ? a_off[i] : OOB), 0, 0, 0);
            a_off[i] += a_step;
            a_m[i] += BR;
        }
#pragma unroll
        for (int j = 0; j < NIB; ++j) {
            if (PLAIN) {
                const bool ok = b_ok[j] & (b_m[j] < m_end);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(src_rs, (lds_void*)(base + A_BYTES + j * NWAVES * 1024), 16, (int)(ok ? b_off[j] : OOB), 0, 0, 0);
                b_off[j] += b_step;
            } else {
                // (ih, iw) for the bounds test only: one 24-bit multiply-add each (full rate; oh, ow and the stride are far below 2^24)
                const int ih = __mul24(g_oh[j], p.stride) + b_fr[j];
                const int iw = __mul24(g_ow[j], p.stride) + b_fs[j];
                const bool ok = b_ok[j] & (b_m[j] < m_end) & ((unsigned)ih < (unsigned)p.H) & ((unsigned)iw < (unsigned)p.W);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(src_rs, (lds_void*)(base + A_BYTES + j * NWAVES * 1024), 16, (int)(ok ? b_off[j] : OOB), 0, 0, 0);
                int ow = g_ow[j] + p.d_ow;
                const bool c1 = ow >= p.OW;
                ow -= c1 ? p.OW : 0;
                int oh = g_oh[j] + p.d_oh + (c1 ? 1 : 0);
                const bool c2 = oh >= p.OH;
                oh -= c2 ? p.OH : 0;
                g_ow[j] = ow;
                g_oh[j] = oh;
                b_off[j] += inc_base + (c1 ? inc_cy1 : 0u) + (c2 ? inc_cy2 : 0u);
            }
            b_m[j] += BR;
        }
    };

    f32x4 acc[AT][BT];
#pragma unroll
    for (int ai = 0; ai < AT; ++ai)
#pragma unroll
        for (int bi = 0; bi < BT; ++bi) acc[ai][bi] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool do_bias = (p.dbias != nullptr) && (tile_b == 0);
    f32x4 bacc[ABT];
#pragma unroll
    for (int t = 0; t < ABT; ++t) bacc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    // fragment offsets within a step: rows row0 .. row0+3 (and +4), 16 columns = one 32-byte pair
    const int row0 = lg * 8 + (l15 >> 2);
    int fa_off[AT], fb_off[BT];
#pragma unroll
    for (int ai = 0; ai < AT; ++ai)
        fa_off[ai] = row0 * PITCH_A + (((wa * AT + ai) ^ tn_g<CPR_A>(row0)) << 5) + (l15 & 3) * 8;
#pragma unroll
    for (int bi = 0; bi < BT; ++bi)
        fb_off[bi] = A_BYTES + row0 * PITCH_B + (((wb * BT + bi) ^ tn_g<CPR_B>(row0)) << 5) + (l15 & 3) * 8;

    const u32x4 ones = {0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u};
    // The transposed fragment reads are spelled as asm: behind the BUILTIN the compiler waits vmcnt(0) (an LDS access it can
    // see while LDS-DMA writes are pending), which would drain the whole ring every step.  All reads of a step are issued at
    // once; a counted lgkmcnt wait tied to the B fragment of column bi releases that column's MFMAs (LDS returns in order,
    // and the A fragments were issued first).
    auto compute = [&](int stage) __attribute__((always_inline)) {
        const uint32_t base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)(smem + stage * STAGE);
        u32x2 alo[AT], ahi[AT], blo[BT], bhi[BT];
#pragma unroll
        for (int ai = 0; ai < AT; ++ai) {
            const uint32_t q = base + (uint32_t)fa_off[ai];
            asm volatile("ds_read_b64_tr_b16 %0, %2\n\tds_read_b64_tr_b16 %1, %2 offset:%3"
                         : "=&v"(alo[ai]), "=&v"(ahi[ai]) : "v"(q), "n"(4 * PITCH_A) : "memory");
        }
#pragma unroll
        for (int bi = 0; bi < BT; ++bi) {
            const uint32_t q = base + (uint32_t)fb_off[bi];
            asm volatile("ds_read_b64_tr_b16 %0, %2\n\tds_read_b64_tr_b16 %1, %2 offset:%3"
                         : "=&v"(blo[bi]), "=&v"(bhi[bi]) : "v"(q), "n"(4 * PITCH_B) : "memory");
        }
        u32x4 af[AT];
#pragma unroll
        for (int bi = 0; bi < BT; ++bi) {
            asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(blo[bi]), "+v"(bhi[bi]) : "n"(2 * (BT - 1 - bi)) : "memory");
            if (bi == 0) {
#pragma unroll
                for (int ai = 0; ai < AT; ++ai) af[ai] = u32x4{alo[ai][0], alo[ai][1], ahi[ai][0], ahi[ai][1]};
            }
            const u32x4 bf = {blo[bi][0], blo[bi][1], bhi[bi][0], bhi[bi][1]};
#pragma unroll
            for (int ai = 0; ai < AT; ++ai)
                acc[ai][bi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[ai]),
                                                                      __builtin_bit_cast(bf16x8, bf), acc[ai][bi], 0, 0, 0);
        }
        if (do_bias) {
#pragma unroll
            for (int t = 0; t < ABT; ++t)
                bacc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[wb * ABT + t]),
                                                                  __builtin_bit_cast(bf16x8, ones), bacc[t], 0, 0, 0);
        }
    };

    const int nt = (m_end - m_begin + BR - 1) / BR;
    int issued = 0;
    for (; issued < NSTAGE - 1 && issued < nt; ++issued) issue_step(issued);
    int st_c = 0;
    int st_i = issued % NSTAGE;
    for (int t = 0; t < nt; ++t) {
        const int ahead = issued - t - 1;          // wave-uniform
        if (ahead >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LPT) : "memory");
        else if (ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPT) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();              // everyone's part of step t landed; step t-1 is fully consumed
        if (issued < nt) {
            issue_step(st_i);
            ++issued;
            st_i = (st_i + 1 == NSTAGE) ? 0 : st_i + 1;
        }
        compute(st_c);
        st_c = (st_c + 1 == NSTAGE) ? 0 : st_c + 1;
    }

    if (do_bias && l15 == 0) {      // every column of bacc holds the row sums: D row -> n = .. + lg*4 + r
#pragma unroll
        for (int t = 0; t < ABT; ++t) {
            const int n0 = tile_a * BA + wa * WA + (wb * ABT + t) * 16 + lg * 4;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (n0 + r < p.Cout) saicv::det_add(p.det, p.dbias + n0 + r, (size_t)p.Cout * p.Kd + n0 + r, split, bacc[t][r]);
        }
    }
    // epilogue: D row -> n = .. + lg*4 + r ; D col -> kk = .. + l15
#pragma unroll
    for (int ai = 0; ai < AT; ++ai) {
        const int n0 = tile_a * BA + wa * WA + ai * 16 + lg * 4;
#pragma unroll
        for (int bi = 0; bi < BT; ++bi) {
            const int kk = tile_b * BB + wb * WB + bi * 16 + l15;
            if (kk < p.Kd) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (n0 + r < p.Cout)
                        saicv::det_add(p.det, p.dw + (size_t)(n0 + r) * (size_t)p.Kd + kk, (size_t)(n0 + r) * (size_t)p.Kd + kk, split, acc[ai][bi][r]);
            }
        }
    }
}

FastDiv make_fastdiv(uint32_t d) {
    FastDiv f;
    uint32_t l = 0;
    while ((1ull << l) < d) ++l;                       // l = ceil(log2 d)
    f.mul = (uint32_t)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
    f.s1 = l < 1 ? l : 1;
    f.s2 = l > 0 ? l - 1 : 0;
    return f;
}

template <typename K>
void allow_lds(K k, size_t smem) {
    // one-time opt-in for > 64 KiB dynamic LDS (idempotent; cheap enough to repeat)
    hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
}

// ---- launches: one workgroup per tile.  The instantiated forms: fp32 data writes fp32 only; the 256 x 256 tile writes bf16 only
// (an fp32 output tile would need ~264 KiB of epilogue LDS; pick_tile() never gives it one); bf16 data writes fp32 in the forward
// mode only; 128-byte K slices for pointwise bf16 products on the 256-row tiles.
template <typename T, int BM_T, int BN_T, int WM_, int WN_, int MODE, bool OUT_F32, bool PLAIN, int KC = 4>
int launch_nt1_inst(const NTParams& p, size_t smem, hipStream_t st) {
    auto k = igemm_nt1_kernel<T, BM_T, BN_T, WM_, WN_, MODE, OUT_F32, PLAIN, KC>;
    static bool once = (allow_lds(k, 160 * 1024), true);
    (void)once;
    dim3 grid(p.nblk, (MODE == 1 && p.stride > 1) ? p.stride * p.stride : 1), block(64 * WM_ * WN_);
    hipLaunchKernelGGL(k, grid, block, smem, st, p);
    return saicv::check_launch("igemm_nt");
}

template <typename T, int BM_T, int BN_T, int WM_, int WN_, int MODE>
int launch_nt1(const NTParams& p, bool out_f32, bool plain, hipStream_t st) {
    // fp32 output of bf16 data: forward only (logits, fp32 residual streams) -- no public entry point asks a data gradient for it
    constexpr bool F32_OUT = !(BM_T == 256 && BN_T == 256) && (sizeof(T) == 4 || MODE == 0);
    constexpr bool BF16_OUT = sizeof(T) == 2;
    constexpr size_t smem_full = nt_stages(BM_T, BN_T) * (size_t)(BM_T * 64 + BN_T * 64);      // DMA ring
    const size_t epi = BM_T * (size_t)(BN_T * ((out_f32 || sizeof(T) == 4) ? 4 : 2) + 16) +
                       2 * WM_ * BN_T * sizeof(float);      // staged output tile + per-wavefront BN column sums
    size_t smem = smem_full;
    if (smem < epi) smem = epi;
#ifdef SAICV_NT_TIMELINE
    if (getenv("SAICV_NT_SOLO") && smem < 84 * 1024) smem = 84 * 1024;      // debug build: one workgroup per CU (what a lone K loop sustains)
#endif
    if constexpr (BF16_OUT && BM_T == 256) {
        if (p.kc8 && plain && !out_f32) {
            constexpr size_t ring = nt_stages_kc8(BM_T, BN_T) * (size_t)(BM_T + BN_T) * 128;
            return launch_nt1_inst<T, BM_T, BN_T, WM_, WN_, MODE, false, true, 8>(p, ring < epi ? epi : ring, st);
        }
    }
    if constexpr (F32_OUT) {
        if (out_f32) {
            if (plain) return launch_nt1_inst<T, BM_T, BN_T, WM_, WN_, MODE, true, true>(p, smem, st);
            return launch_nt1_inst<T, BM_T, BN_T, WM_, WN_, MODE, true, false>(p, smem, st);
        }
    }
    if constexpr (BF16_OUT) {
        if (!out_f32) {
            if (plain) return launch_nt1_inst<T, BM_T, BN_T, WM_, WN_, MODE, false, true>(p, smem, st);
            return launch_nt1_inst<T, BM_T, BN_T, WM_, WN_, MODE, false, false>(p, smem, st);
        }
    }
    saicv::set_error("igemm_nt: the %d x %d tile has no %s-output form for %s data", BM_T, BN_T, out_f32 ? "fp32" : "bf16",
                     sizeof(T) == 2 ? "bf16" : "fp32");
    return -1;
}

// Tile choice of nt_plan(): relative per-flop speed of each geometry x
// wave-quantisation efficiency on 256 CUs x useful fraction of the tile.  The speeds are fitted to a sweep of
// every geometry over the 23 ResNet-50 shapes and the ViT / SAM linear shapes (scripts/gpu_tiles.sh, r01e): two
// co-resident 256 x 128 workgroups hide each other's epilogue (launch, prologue latency, store drain: ~11 us per
// 64 K outputs per CU whatever the geometry), which beats one 256 x 256 workgroup until the K loop is long enough
// (~100 K tiles) for its lower LDS traffic per flop to matter.
struct NTTile { int bm, bn, blocks_per_cu; float speed; };
const NTTile kTiles[4] = {{256, 256, 1, 0.80f}, {256, 128, 2, 1.00f}, {128, 128, 2, 0.60f}, {128, 64, 3, 0.50f}};

int pick_tile(int M, int Nn, int nkt, bool f32_out_big) {
    if (const char* force = getenv("SAICV_NT_TILE")) {      // tuning aid: force a geometry
        const int t = atoi(force);
        if (t >= 0 && t < 4 && !(f32_out_big && kTiles[t].bm * kTiles[t].bn * 4 > 150 * 1024)) return t;
    }
    int best = 2;
    float best_score = -1.f;
    for (int t = 0; t < 4; ++t) {
        if (f32_out_big && kTiles[t].bm * kTiles[t].bn * 4 > 150 * 1024) continue;   // fp32 epilogue tile must fit LDS
        const NTTile& g = kTiles[t];
        const long tm = (M + g.bm - 1) / g.bm, tn = (Nn + g.bn - 1) / g.bn;
        const float blocks = (float)(tm * tn);
        const float slots = 256.f * g.blocks_per_cu;
        const float rounds = blocks / slots;
        const float quant = rounds / (float)(long)(rounds + 0.999999f);
        const float useful = ((float)M / (tm * g.bm)) * ((float)Nn / (tn * g.bn));
        float speed = g.speed;
        if (t == 0) speed = nkt >= 100 ? 1.10f : nkt >= 48 ? 0.90f : 0.80f;
        const float score = speed * quant * useful;
        if (score > best_score) { best_score = score; best = t; }
    }
    return best;
}

// Everything that decides how igemm_nt runs a product.
struct NTProblem {
    int dtype, mode;
    int H, W, C, OH, OW, R, S, stride, pad;      // gather source, row pixel grid, taps (igemm_nt's arguments)
    int M, Nn, Kd, ldo;
    bool out_f32;                                // fp32 output of bf16 data
    bool bias, stats, addend, row_scale, out2, bn_sums;      // which epilogue operands are present (bn_sums: EpiExtra::bs_*)
    int act_mode;
};
enum NTRoute { NT_TILED, NT_PW_STREAM, NT_PW3_STREAM };
struct NTPlan {
    NTRoute route;
    int tile;           // NT_TILED: kTiles index
    bool kc8;           // NT_TILED: the 128-byte-K-slice instantiation
    bool plain;         // NT_TILED: pointwise taps without padding (the source pixel of a row never leaves the image): no tap walker
    bool f32o;          // NT_TILED: the output is fp32 (fp32 data, or bf16 data with out_f32)
    int blocks;         // workgroups (NT_TILED: one per tile, all parity classes of a stride > 1 data gradient)
    int stat_rows;      // rows of partial statistics (forward sums or BatchNorm-backward sums) the launch writes
};

// How igemm_nt runs a product, as a pure function of the problem and of the tuning switches SAICV_PW_STREAM, SAICV_PW_STREAM3,
// SAICV_PW_MIN_ROWS, SAICV_NT_KC8 and SAICV_NT_TILE (read per call: tests and sweeps flip them in-process).  The launch and
// the partial-statistics row queries (conv_stat_rows, conv_bwd_stat_rows) both ask it, so a buffer sized by a query always
// matches the launch.
NTPlan nt_plan(const NTProblem& q) {
    NTPlan pl = {NT_TILED, 0, false, false, false, 0, 0};
    // the weight-resident streaming kernels of pwstream.hip: bf16 in and out, dense rows, a plain epilogue (statistics, or a
    // data gradient's shortcut addend / BatchNorm-backward sums, never both) -- no tiles, no workgroup barriers, one partial
    // row per workgroup
    const bool streamable = q.dtype == SAICV_DTYPE_BF16 && !q.out_f32 && q.stride == 1 && q.ldo == q.Nn && !q.bias && !q.act_mode &&
                            !q.row_scale && !q.out2 && !(q.stats && (q.addend || q.bn_sums));
    // small-K x small-N pointwise products over many rows (ResNet stage 1-2 1 x 1 convolutions and their data gradients)
    if (streamable && q.R == 1 && q.S == 1 && q.pad == 0) {
        pl.blocks = saicv::pw_stream_blocks(q.dtype, q.M, q.Nn, q.Kd, (q.addend || q.bn_sums) && !q.stats);
        if (pl.blocks > 0) {
            pl.route = NT_PW_STREAM;
            pl.stat_rows = pl.blocks;
            return pl;
        }
    }
    // ... and the 3 x 3 / stride 1 / padding 1 convolution 64 -> 64 of the same stage and its data gradient, as the same stream over nine taps
    if (streamable && q.R == 3 && q.S == 3 && q.pad == 1 && q.C == 64 && q.H == q.OH && q.W == q.OW && q.H >= 1 && q.W >= 1 &&
        q.M % (q.H * q.W) == 0) {
        pl.blocks = saicv::pw3_stream_blocks(q.dtype, q.M, q.Nn, q.Kd);
        if (pl.blocks > 0) {
            pl.route = NT_PW3_STREAM;
            pl.stat_rows = pl.blocks;
            return pl;
        }
    }
    const bool f32o = q.out_f32 || q.dtype == SAICV_DTYPE_F32;
    int M_tile = q.M;
    if (q.mode == 1 && q.stride > 1)       // largest parity class
        M_tile = (q.M / (q.OH * q.OW)) * ((q.OH + q.stride - 1) / q.stride) * ((q.OW + q.stride - 1) / q.stride);
    const int bk = q.dtype == SAICV_DTYPE_BF16 ? 32 : 16;
    pl.tile = pick_tile(M_tile, q.Nn, (q.Kd + bk - 1) / bk, f32o);      // K tiles (stride > 1 data-gradient classes run fewer)
    // 128-byte K slices (igemm_nt1_kernel, KC = 8) on the 256 x 256 tile: one workgroup per CU, so only where the main loop is
    // long against the exposed prologue / epilogue and the launch fills the CUs several times.  SAICV_NT_KC8: 0 never,
    // 1 every eligible launch of a 256-row tile, 2 (default) wide pointwise GEMMs without a fused activation, 3 the same with
    // them -- measured on the ViT-B shapes (profiles/r03_lds_fill_and_kc8.md): +10...13 % for N >= 2048, K = 768; -8 % for
    // N = K = 768; the GELU-fused launches (two output tensors / one more input in the epilogue) lose 10 % with one workgroup
    // per CU: ViT-B step 42.57 ms off, 42.95 with them, 42.31 without.
    const char* ke = getenv("SAICV_NT_KC8");
    const int kc8_mode = ke ? atoi(ke) : 2;
    const bool pointwise = q.R == 1 && q.S == 1 && q.pad == 0 && (q.mode == 0 || q.stride == 1);
    pl.plain = pointwise;
    pl.f32o = f32o;
    const bool ok = q.dtype == SAICV_DTYPE_BF16 && !f32o && pointwise && kTiles[pl.tile].bm == 256 && q.Kd >= 256;
    if (ok && kc8_mode == 1) pl.kc8 = true;
    const bool rule_ok = (kc8_mode == 2 && q.act_mode == 0) || kc8_mode == 3;
    if (ok && rule_ok && q.Nn >= 2048 && q.Nn % 256 == 0 && q.Kd >= 512 && (long)((M_tile + 255) / 256) * (q.Nn / 256) >= 4 * 256) {
        pl.kc8 = true;
        pl.tile = 0;
    }
    // one row per tile row, per parity class of a stride > 1 data gradient
    const int classes = q.mode == 1 && q.stride > 1 ? q.stride * q.stride : 1;
    pl.stat_rows = ((M_tile + kTiles[pl.tile].bm - 1) / kTiles[pl.tile].bm) * classes;
    pl.blocks = pl.stat_rows * ((q.Nn + kTiles[pl.tile].bn - 1) / kTiles[pl.tile].bn);
    return pl;
}

// operands the tiled kernel addresses through 32-bit buffer offsets
bool nt_operands_fit(const NTProblem& q) {
    const size_t esz = q.dtype == SAICV_DTYPE_BF16 ? 2 : 4;
    const size_t src_bytes = (size_t)(q.M / (q.OH * q.OW)) * q.H * q.W * q.C * esz;
    const size_t wgt_bytes = (size_t)q.Nn * q.Kd * esz;
    return src_bytes < 0xfffffff0ull && wgt_bytes < 0xfffffff0ull;
}

// Everything that decides how igemm_tn runs a weight gradient.
struct TNProblem {
    int dtype;
    int H, W, C, OH, OW, R, S, stride, pad;
    int M, Cout, Kd;
};
struct TNPlan {
    bool big;           // the 256 x 256 tile
    int ba, bb;         // tile: ba output channels x bb reduction columns (r, s, c)
    int tiles_a, tiles_b;
    int BR;             // rows of a reduction step the splits are counted in
    int total_rt;       // reduction steps of the whole product
    int rt_per;         // ... of one split
    int splits;
    bool dma;           // igemm_tn_dma_kernel (bf16) / the register-staged igemm_tn_kernel
    bool plain;         // igemm_tn_dma_kernel: 1 x 1 / stride 1 / no padding (row m of the source is row m of the GEMM)
};

// How igemm_tn runs a product, as a pure function of the problem, of the switches SAICV_TN_SLOTS_PCT and SAICV_TN_DMA (read per call)
// and of whether the process holds a multi-rank communicator.  The launch and the plan query both ask it.
TNPlan tn_plan(const TNProblem& q) {
    TNPlan pl;
    const int epc = q.dtype == SAICV_DTYPE_BF16 ? 8 : 4;
    const int M = q.M, Cout = q.Cout, Kd = q.Kd;
    const int BR = 8 * epc;
    pl.BR = BR;
    // 256 x 256 tiles (8 wavefronts of 128 x 64) halve both the HBM/L2 traffic and the LDS fragment reads per
    // MFMA of the 128 x 128 geometry; used when both output dimensions fill them
    // ... when both output dimensions fill them and every workgroup keeps >= 48 reduction steps (below that the
    // 256 KiB of fp32 atomics per workgroup outweigh the gain: the small-M ResNet stages stay on 128 x 128)
    const int big_tiles = ((Cout + 255) / 256) * ((Kd + 255) / 256);
    const int big_steps = ((M + BR - 1) / BR) / (256 / big_tiles > 0 ? 256 / big_tiles : 1);
    const bool big = Cout % 256 == 0 && Kd >= 256 && (Kd % 256 == 0 || Kd >= 1024) && big_steps >= 48;
    pl.big = big;
    const int ba = big ? 256 : Cout <= 64 ? 64 : 128;
    const int bb = big ? 256 : Kd <= 64 ? 64 : 128;
    pl.ba = ba; pl.bb = bb;
    pl.tiles_a = (Cout + ba - 1) / ba;
    pl.tiles_b = (Kd + bb - 1) / bb;
    const int tiles = pl.tiles_a * pl.tiles_b;
    // split the pixel reduction so that ~4 workgroups per CU are in flight
    const int total_rt = (M + BR - 1) / BR;
    // 128-wide tiles: 2 workgroups per CU are resident (73 KiB LDS each); 256-wide: one (139 KiB)
    // rounded DOWN: one full round of resident workgroups beats a second, nearly empty one
    // The split count is sized for ALL resident slots when this GPU runs nothing else, and for 85 % of them once the process has
    // created an RCCL communicator over more than one rank (g_saicv_comm_world, comm.hip): the one-round design has no slack -- under
    // data-parallel training RCCL's all-reduce kernels hold CU slots (and LDS) during backward, and every workgroup that cannot
    // start with the others costs this kernel a whole second round.  Measured on one GPU (r05, same box, twice each): 100 against
    // 85 is ViT-B 40.02 -> 39.52 ms (weight gradients 10.0 -> 9.4 ms), ResNet-50 21.00 -> 20.95 ms; 70 is ResNet-50 21.60 ms.
    // SAICV_TN_SLOTS_PCT overrides (read per call; e.g. 85 for a torch.distributed process group without the native communicator).
    const char* slots_env = getenv("SAICV_TN_SLOTS_PCT");
    const int slots_pct = slots_env ? atoi(slots_env) : (g_saicv_comm_world > 1 ? 85 : 100);
    int splits = ((big ? 256 : 512) * slots_pct / 100) / tiles;
    if (splits > total_rt) splits = total_rt;
    if (splits < 1) splits = 1;
    int rt_per = (total_rt + splits - 1) / splits;
    splits = (total_rt + rt_per - 1) / rt_per;
    pl.total_rt = total_rt; pl.rt_per = rt_per; pl.splits = splits;
    // bf16: the LDS-DMA ring kernel (32-row steps; SAICV_TN_DMA=0 selects the register-staged kernel for A/B runs)
    const char* de = getenv("SAICV_TN_DMA");             // read per call
    const int use_dma = de ? atoi(de) : 1;
    pl.dma = use_dma && q.dtype == SAICV_DTYPE_BF16;
    pl.plain = q.R == 1 && q.S == 1 && q.stride == 1 && q.pad == 0 && q.H == q.OH && q.W == q.OW;
    return pl;
}

bool tn_operands_fit(const TNProblem& q) {
    const size_t esz = q.dtype == SAICV_DTYPE_BF16 ? 2 : 4;
    const size_t dy_bytes = (size_t)q.M * q.Cout * esz;
    const size_t src_bytes = (size_t)(q.M / (q.OH * q.OW)) * q.H * q.W * q.C * esz;
    return dy_bytes < 0xfffffff0ull && src_bytes < 0xfffffff0ull;
}

template <typename T, int BA, int BB, int NWA = 2, int NWB = 2>
int launch_tn(const TNParams& p, int splits, hipStream_t st) {
    constexpr int EPC = ElemTraits<T>::EPC;
    constexpr int BR = 8 * EPC;
    constexpr size_t smem = 2 * (size_t)BR * ((BA + 16) + (BB + 16)) * sizeof(T);
    dim3 grid(p.tiles_a * p.tiles_b, splits), block(64 * NWA * NWB);
    auto k = igemm_tn_kernel<T, BA, BB, NWA, NWB>;
    static bool once = (allow_lds(k, smem), true);
    (void)once;
    hipLaunchKernelGGL(k, grid, block, smem, st, p);
    return saicv::check_launch("igemm_tn");
}

template <int BA, int BB, int NWA = 2, int NWB = 2>
int launch_tn_dma(const TNParams& p, int splits, bool plain, hipStream_t st) {
    constexpr size_t smem = 4 * (size_t)32 * (BA + BB) * 2;
    dim3 grid(p.tiles_a * p.tiles_b, splits), block(64 * NWA * NWB);
    if (plain) {
        auto k = igemm_tn_dma_kernel<BA, BB, NWA, NWB, true>;
        static bool once = (allow_lds(k, smem), true);
        (void)once;
        hipLaunchKernelGGL(k, grid, block, smem, st, p);
    } else {
        auto k = igemm_tn_dma_kernel<BA, BB, NWA, NWB, false>;
        static bool once = (allow_lds(k, smem), true);
        (void)once;
        hipLaunchKernelGGL(k, grid, block, smem, st, p);
    }
    return saicv::check_launch("igemm_tn");
}

}  // namespace

namespace saicv {

// rows of BatchNorm partial statistics saicv_conv2d_fwd writes with stat_sum (the output in the data type, no bias)
int conv_stat_rows(const saicv_conv_desc* d) {
    const NTProblem q = {d->dtype, 0, d->H, d->W, d->C, d->OH, d->OW, d->R, d->S, d->stride, d->pad,
                         d->N * d->OH * d->OW, d->K, d->R * d->S * d->C, d->K,
                         /*out_f32=*/false, /*bias=*/false, /*stats=*/true, false, false, false, false, 0};
    return nt_plan(q).stat_rows;
}

// rows of BatchNorm-backward partial sums saicv_conv2d_dgrad_fused writes with bn_y (with or without the shortcut addend)
int conv_bwd_stat_rows(const saicv_conv_desc* d) {
    const NTProblem q = {d->dtype, 1, d->OH, d->OW, d->K, d->H, d->W, d->R, d->S, d->stride, d->pad,
                         d->N * d->H * d->W, d->C, d->R * d->S * d->K, d->C,
                         /*out_f32=*/false, false, false, false, false, false, /*bn_sums=*/true, 0};
    return nt_plan(q).stat_rows;
}

// r05, measured and NOT kept: cutting a badly quantised linear GEMM (ViT-B's 768-wide outputs: 1 182 tiles of 256 x 128 on 512 slots
// = 2.31 rounds of work in 3 rounds of time) into whole rounds of 256 x 128 tiles + one round of 128 x 128 tiles.  Correct (torch fp32
// parity on the row-addressed fused operands), but the ViT-B step went 39.44 -> 40.11 ms on the same box: the second launch pays its
// own ramp, and at the socket power limit the idle CUs of the third round are not lost time (profiles/r05_nt_experiments.md).
int igemm_nt(int dtype, int mode, const void* src, const void* wgt, void* out, const float* bias,
             float* stat_sum, float* stat_sq, int H, int W, int C, int OH, int OW, int R, int S,
             int stride, int pad, int M, int Nn, int Kd, int ldo, int out_f32, hipStream_t st,
             const EpiExtra* ex) {
    const int epc = dtype == SAICV_DTYPE_BF16 ? 8 : 4;
    SAICV_REQUIRE(C % epc == 0, "igemm_nt: C=%d must be a multiple of %d", C, epc);
    SAICV_REQUIRE(Kd % epc == 0, "igemm_nt: Kd=%d must be a multiple of %d", Kd, epc);
    SAICV_REQUIRE(M > 0 && Nn > 0 && Kd > 0, "igemm_nt: empty problem");
    SAICV_REQUIRE(!(bias && stat_sum), "igemm_nt: bias and BN statistics are exclusive");
    NTParams p;
    p.src = src; p.wgt = wgt; p.out = out; p.bias = bias; p.stat_sum = stat_sum; p.stat_sq = stat_sq;
    p.addend = ex ? ex->addend : nullptr;
    p.row_scale = ex ? ex->row_scale : nullptr;
    p.rows_per_scale = ex ? ex->rows_per_scale : 1;
    p.out2 = ex ? ex->out2 : nullptr;
    p.act_mode = ex ? ex->act_mode : 0;
    static const int lean_gelu_env = getenv("SAICV_GELU_EPI") ? atoi(getenv("SAICV_GELU_EPI")) : 1;
    p.lean_gelu = lean_gelu_env;
    p.addend_gate = ex ? ex->addend_gate : nullptr;
    p.bs_y = ex ? ex->bs_y : nullptr;
    p.bs_mask = ex ? ex->bs_mask : nullptr;
    p.bs_mean = ex ? ex->bs_mean : nullptr;
    p.bs_invstd = ex ? ex->bs_invstd : nullptr;
    p.bs_g = ex ? ex->bs_g : nullptr;
    p.bs_gx = ex ? ex->bs_gx : nullptr;
    p.bs_rows = 0;
    p.stat_atomic_rows = ex ? ex->stat_atomic_rows : 0;
#ifdef SAICV_NT_TIMELINE
    p.timeline = g_nt_timeline;
#endif
    SAICV_REQUIRE(p.stat_atomic_rows >= 0 && p.stat_atomic_rows <= 64, "igemm_nt: stat_atomic_rows=%d outside [0, 64]", p.stat_atomic_rows);
    if (p.addend_gate || p.bs_y) {
        const int osz1 = (out_f32 || dtype == SAICV_DTYPE_F32) ? 4 : 2;
        SAICV_REQUIRE(mode == 1 && p.act_mode == 0 && (!out_f32 || dtype == SAICV_DTYPE_F32), "igemm_nt: gated shortcut / BatchNorm-backward sums belong to the data gradient");
        SAICV_REQUIRE((ldo * osz1) % 16 == 0 && Nn % (16 / osz1) == 0 && ldo == Nn,
                      "igemm_nt: gated shortcut / BatchNorm-backward sums need dense rows of whole 16-byte chunks (N=%d)", Nn);
        SAICV_REQUIRE(!p.addend_gate || p.addend, "igemm_nt: a gate without an addend");
        SAICV_REQUIRE(!p.bs_y || (p.bs_mean && p.bs_invstd && p.bs_g && p.bs_gx),
                      "igemm_nt: BatchNorm-backward sums need mean, invstd and both partial buffers");
    }
    if (p.act_mode) {
        const int osz0 = (out_f32 || dtype == SAICV_DTYPE_F32) ? 4 : 2;
        SAICV_REQUIRE((ldo * osz0) % 16 == 0 && Nn % (16 / osz0) == 0,
                      "igemm_nt: the fused GELU epilogues need 16-byte aligned rows (N=%d)", Nn);
        SAICV_REQUIRE(p.act_mode >= 1 && p.act_mode <= 4, "igemm_nt: act_mode %d", p.act_mode);
        SAICV_REQUIRE((p.act_mode & 1) ? p.out2 != nullptr : p.addend != nullptr, "igemm_nt: fused GELU operand missing");
        SAICV_REQUIRE(stat_sum == nullptr && p.row_scale == nullptr, "igemm_nt: fused GELU excludes BN statistics / row scale");
    }
    if (p.addend || p.row_scale) {
        const int osz = (out_f32 || dtype == SAICV_DTYPE_F32) ? 4 : 2;
        SAICV_REQUIRE((ldo * osz) % 16 == 0, "igemm_nt: fused residual needs a 16-byte aligned leading dimension");
        SAICV_REQUIRE(p.rows_per_scale >= 1, "igemm_nt: rows_per_scale must be >= 1");
    }
    const NTProblem q = {dtype, mode, H, W, C, OH, OW, R, S, stride, pad, M, Nn, Kd, ldo, out_f32 != 0,
                         bias != nullptr, stat_sum != nullptr, p.addend != nullptr, p.row_scale != nullptr, p.out2 != nullptr,
                         p.bs_y != nullptr, p.act_mode};
    const NTPlan pl = nt_plan(q);
    const bool f32o = out_f32 != 0 || dtype == SAICV_DTYPE_F32;
    // streaming output stores from SAICV_NT_STREAM_MIN_MB MiB of output on (0: always; a huge value: never)
    static const long min_mb = getenv("SAICV_NT_STREAM_MIN_MB") ? atol(getenv("SAICV_NT_STREAM_MIN_MB")) : 0;
    const int stream_out = (size_t)M * Nn * (f32o ? 4 : 2) >= (size_t)min_mb * 1024 * 1024 ? 1 : 0;
    if (pl.route == NT_PW_STREAM)
        return pw_stream(M, Nn, Kd, src, wgt, out, stat_sum, stat_sq, p.stat_atomic_rows, ex, stream_out, pl.blocks, st);
    if (pl.route == NT_PW3_STREAM)
        return pw3_stream(mode, M, H, W, src, wgt, out, stat_sum, stat_sq, p.stat_atomic_rows, ex, stream_out, pl.blocks, st);
    p.H = H; p.W = W; p.C = C; p.OH = OH; p.OW = OW; p.R = R; p.S = S; p.stride = stride; p.pad = pad;
    p.M = M; p.Nn = Nn; p.Kd = Kd; p.ldo = ldo;
    const size_t esz = dtype == SAICV_DTYPE_BF16 ? 2 : 4;
    SAICV_REQUIRE(nt_operands_fit(q), "igemm_nt: operand larger than 4 GiB (buffer addressing)");
    p.src_bytes = (uint32_t)((size_t)(M / (OH * OW)) * H * W * C * esz);
    p.wgt_bytes = (uint32_t)((size_t)Nn * Kd * esz);
    p.fd_ohw = make_fastdiv((uint32_t)(OH * OW));
    p.fd_ow = make_fastdiv((uint32_t)OW);
    p.stream_out = stream_out;
    p.kc8 = pl.kc8 ? 1 : 0;
    // (r03's staged-range main loop for 3 x 3 / stride 1 convolutions -- one contiguous input range per channel slice instead of nine
    // gathered taps, LDS-fill traffic / 2.3 -- measured level with the gather on every ResNet-50 layer (profiles/r03_lds_fill_and_kc8.md
    // section 7) and was removed in r05.)
    const NTTile& g = kTiles[pl.tile];
    const int classes = mode == 1 && stride > 1 ? stride * stride : 1;
    p.bs_rows = pl.stat_rows / classes;
    p.tiles_n = (Nn + g.bn - 1) / g.bn;
    p.nblk = p.tiles_n * p.bs_rows;
#define NT_DISPATCH(TT, MODE_)                                                              \
    switch (pl.tile) {                                                                      \
        case 0: return launch_nt1<TT, 256, 256, 2, 4, MODE_>(p, f32o, pl.plain, st);                  \
        case 1: return launch_nt1<TT, 256, 128, 4, 2, MODE_>(p, f32o, pl.plain, st);                  \
        case 2: return launch_nt1<TT, 128, 128, 2, 2, MODE_>(p, f32o, pl.plain, st);                  \
        default: return launch_nt1<TT, 128, 64, 2, 2, MODE_>(p, f32o, pl.plain, st);                  \
    }
    if (dtype == SAICV_DTYPE_BF16) {
        if (mode == 0) { NT_DISPATCH(bf16_t, 0) } else { NT_DISPATCH(bf16_t, 1) }
    } else {
        if (mode == 0) { NT_DISPATCH(float, 0) } else { NT_DISPATCH(float, 1) }
    }
#undef NT_DISPATCH
}

static int igemm_tn_launch(int dtype, TNParams& p, const TNPlan& pl, hipStream_t st);

int igemm_tn(int dtype, const void* dy, const void* src, float* dw, int H, int W, int C, int OH,
             int OW, int R, int S, int stride, int pad, int M, int Cout, int Kd, hipStream_t st, float* dbias) {
    const int epc = dtype == SAICV_DTYPE_BF16 ? 8 : 4;
    SAICV_REQUIRE(C % epc == 0 && Cout % epc == 0, "igemm_tn: C=%d, Cout=%d must be multiples of %d", C, Cout, epc);
    SAICV_REQUIRE(M > 0 && Cout > 0 && Kd > 0, "igemm_tn: empty problem");
    TNParams p;
    p.dy = dy; p.src = src; p.dw = dw; p.dbias = dbias; p.H = H; p.W = W; p.C = C; p.OH = OH; p.OW = OW;
    p.R = R; p.S = S; p.stride = stride; p.pad = pad; p.M = M; p.Cout = Cout; p.Kd = Kd;
    const TNProblem q = {dtype, H, W, C, OH, OW, R, S, stride, pad, M, Cout, Kd};
    const size_t esz = dtype == SAICV_DTYPE_BF16 ? 2 : 4;
    SAICV_REQUIRE(tn_operands_fit(q), "igemm_tn: operand larger than 4 GiB (buffer addressing)");
    p.dy_bytes = (uint32_t)((size_t)M * Cout * esz);
    p.src_bytes = (uint32_t)((size_t)(M / (OH * OW)) * H * W * C * esz);
    p.fd_ohw = make_fastdiv((uint32_t)(OH * OW));
    p.fd_ow = make_fastdiv((uint32_t)OW);
    const TNPlan pl = tn_plan(q);
    p.tiles_a = pl.tiles_a;
    p.tiles_b = pl.tiles_b;
    p.m_per_split = pl.rt_per * pl.BR;
    // deterministic mode (det.h): the splits park their tiles (and bias sums) side by side, one launch folds them in split order
    // (not zeroed: every split owns at least one row tile -- (splits - 1) * rt_per < total_rt in tn_plan() -- and writes its whole tile and bias sums)
    DetParts det;
    if (det.begin(st, pl.splits, (size_t)Cout * Kd + (dbias ? Cout : 0), "igemm_tn", /*zero=*/false)) return -1;
    p.det = det.sink();
    const int rc = igemm_tn_launch(dtype, p, pl, st);
    if (rc) return rc;
    if (det.fold(dw, 0, (size_t)Cout * Kd, /*wide=*/true)) return -1;
    if (dbias && det.fold(dbias, (size_t)Cout * Kd, (size_t)Cout)) return -1;
    return 0;
}

static int igemm_tn_launch(int dtype, TNParams& p, const TNPlan& pl, hipStream_t st) {
    const int OW = p.OW;
    const int ohw = p.OH * OW;
    const int splits = pl.splits, ba = pl.ba, bb = pl.bb;
    const bool big = pl.big;
    p.d_img = pl.BR / ohw;
    const int rem = pl.BR - p.d_img * ohw;
    p.d_oh = rem / OW;
    p.d_ow = rem - p.d_oh * OW;
    if (pl.dma) {
        const int br = 32;
        p.d_img = br / ohw;
        const int rem32 = br - p.d_img * ohw;
        p.d_oh = rem32 / OW;
        p.d_ow = rem32 - p.d_oh * OW;
        const bool plain = pl.plain;
        if (big) return launch_tn_dma<256, 256, 2, 4>(p, splits, plain, st);
        if (ba == 64 && bb == 64) return launch_tn_dma<64, 64>(p, splits, plain, st);
        if (ba == 64) return launch_tn_dma<64, 128>(p, splits, plain, st);
        if (bb == 64) return launch_tn_dma<128, 64>(p, splits, plain, st);
        return launch_tn_dma<128, 128>(p, splits, plain, st);
    }
    if (big) {
        if (dtype == SAICV_DTYPE_BF16) return launch_tn<bf16_t, 256, 256, 2, 4>(p, splits, st);
        return launch_tn<float, 256, 256, 2, 4>(p, splits, st);
    }
    if (dtype == SAICV_DTYPE_BF16) {
        if (ba == 64 && bb == 64) return launch_tn<bf16_t, 64, 64>(p, splits, st);
        if (ba == 64) return launch_tn<bf16_t, 64, 128>(p, splits, st);
        if (bb == 64) return launch_tn<bf16_t, 128, 64>(p, splits, st);
        return launch_tn<bf16_t, 128, 128>(p, splits, st);
    } else {
        if (ba == 64 && bb == 64) return launch_tn<float, 64, 64>(p, splits, st);
        if (ba == 64) return launch_tn<float, 64, 128>(p, splits, st);
        if (bb == 64) return launch_tn<float, 128, 64>(p, splits, st);
        return launch_tn<float, 128, 128>(p, splits, st);
    }
}

// ---- the launch plan of a public entry point's product, for saicv_igemm_plan (no tensors, nothing launched)
static NTProblem nt_problem_of(const saicv_plan_query* q) {
    const saicv_conv_desc* d = &q->conv;
    const bool out2 = q->act_mode == 1 || q->act_mode == 3;
    switch (q->op) {
        case SAICV_PLAN_CONV_FWD:        // saicv_conv2d_fwd / _fwd_stats
            return {d->dtype, 0, d->H, d->W, d->C, d->OH, d->OW, d->R, d->S, d->stride, d->pad, d->N * d->OH * d->OW, d->K,
                    d->R * d->S * d->C, d->K, q->out_f32 != 0, q->bias != 0, q->stats != 0, q->addend != 0, q->row_scale != 0, out2,
                    q->bn_sums != 0, q->act_mode};
        case SAICV_PLAN_CONV_DGRAD:      // saicv_conv2d_dgrad / _dgrad_add / _dgrad_fused
            return {d->dtype, 1, d->OH, d->OW, d->K, d->H, d->W, d->R, d->S, d->stride, d->pad, d->N * d->H * d->W, d->C,
                    d->R * d->S * d->K, d->C, false, false, false, q->addend != 0, false, false, q->bn_sums != 0, 0};
        case SAICV_PLAN_LINEAR_FWD:      // saicv_linear_fwd / _gelu_fwd / _gelu_fwd_aux
            return {q->dtype, 0, 1, 1, q->K, 1, 1, 1, 1, 1, 0, q->M, q->N, q->K, q->N, q->out_f32 != 0, q->bias != 0, false,
                    q->addend != 0, q->row_scale != 0, out2, false, q->act_mode};
        default:                         // SAICV_PLAN_LINEAR_DGRAD: saicv_linear_dgrad / _dgrad_gelu / _dgrad_mul
            return {q->dtype, 1, 1, 1, q->N, 1, 1, 1, 1, 1, 0, q->M, q->K, q->N, q->K, false, false, false,
                    q->addend != 0 || q->act_mode == 2 || q->act_mode == 4, false, false, false, q->act_mode};
    }
}

int igemm_plan(const saicv_plan_query* q, saicv_plan* out) {
    *out = saicv_plan{};
    if (q->op == SAICV_PLAN_CONV_WGRAD || q->op == SAICV_PLAN_LINEAR_WGRAD) {
        const saicv_conv_desc* d = &q->conv;
        const TNProblem t = q->op == SAICV_PLAN_CONV_WGRAD
            ? TNProblem{d->dtype, d->H, d->W, d->C, d->OH, d->OW, d->R, d->S, d->stride, d->pad, d->N * d->OH * d->OW, d->K, d->R * d->S * d->C}
            : TNProblem{q->dtype, 1, 1, q->K, 1, 1, 1, 1, 1, 0, q->M, q->N, q->K};
        const int epc = t.dtype == SAICV_DTYPE_BF16 ? 8 : 4;
        SAICV_REQUIRE(t.C % epc == 0 && t.Cout % epc == 0, "igemm_tn: C=%d, Cout=%d must be multiples of %d", t.C, t.Cout, epc);
        SAICV_REQUIRE(t.M > 0 && t.Cout > 0 && t.Kd > 0, "igemm_tn: empty problem");
        SAICV_REQUIRE(tn_operands_fit(t), "igemm_tn: operand larger than 4 GiB (buffer addressing)");
        const TNPlan pl = tn_plan(t);
        out->route = SAICV_ROUTE_TN;
        out->tile = pl.big ? 4 : (pl.ba == 128 ? 2 : 0) + (pl.bb == 128 ? 1 : 0);
        out->bm = pl.ba; out->bn = pl.bb;
        out->plain = pl.plain; out->out_f32 = 1; out->dma = pl.dma;
        out->blocks = pl.tiles_a * pl.tiles_b * pl.splits;
        out->splits = pl.splits; out->rt_per = pl.rt_per; out->total_rt = pl.total_rt; out->rows_per_step = pl.BR;
        return 0;
    }
    const NTProblem n = nt_problem_of(q);
    const int epc = n.dtype == SAICV_DTYPE_BF16 ? 8 : 4;
    SAICV_REQUIRE(n.C % epc == 0, "igemm_nt: C=%d must be a multiple of %d", n.C, epc);
    SAICV_REQUIRE(n.Kd % epc == 0, "igemm_nt: Kd=%d must be a multiple of %d", n.Kd, epc);
    SAICV_REQUIRE(n.M > 0 && n.Nn > 0 && n.Kd > 0, "igemm_nt: empty problem");
    SAICV_REQUIRE(!(n.bias && n.stats), "igemm_nt: bias and BN statistics are exclusive");
    SAICV_REQUIRE(!(n.stats && n.out_f32), "saicv_conv2d_fwd: BN statistics need out_f32 = 0");
    const NTPlan pl = nt_plan(n);
    out->route = pl.route == NT_TILED ? SAICV_ROUTE_TILED : pl.route == NT_PW_STREAM ? SAICV_ROUTE_PW_STREAM : SAICV_ROUTE_PW3_STREAM;
    out->blocks = pl.blocks;
    out->stat_rows = pl.stat_rows;
    if (pl.route != NT_TILED) return 0;
    SAICV_REQUIRE(nt_operands_fit(n), "igemm_nt: operand larger than 4 GiB (buffer addressing)");
    out->tile = pl.tile;
    out->bm = kTiles[pl.tile].bm; out->bn = kTiles[pl.tile].bn;
    out->kc8 = pl.kc8;
    out->plain = pl.plain;
    out->out_f32 = pl.f32o;
    return 0;
}

}  // namespace saicv

#ifdef SAICV_NT_TIMELINE
// debug build only (scripts/nt_timeline.py): 16 u64 per workgroup of the NEXT igemm_nt launches (one tile per workgroup kernels)
extern "C" void saicv_debug_nt_timeline(unsigned long long* buf) { g_nt_timeline = buf; }
#endif
