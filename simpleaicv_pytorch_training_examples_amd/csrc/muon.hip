// Muon on the flat fp32 arenas, gfx950: momentum + operand packing, grouped Newton-Schulz GEMMs on MFMA, update.
// Semantics follow the reference tools/muon_optimizer.py (momentum -> nesterov -> Newton-Schulz -> decoupled decay ->
// p -= lr * 0.2 sqrt(max(shape[:2])) * u, and its own AdamW for everything that is no matrix); the kernels are new.
//
// Every Muon parameter is ONE problem of a device table (kTab ints per problem, filled by ops.MuonPlan).  In storage order a
// parameter is a row-major [size(0)][numel / size(0)] matrix (contiguous and channels-last tensors alike: dim 0 is outermost;
// Newton-Schulz commutes with a permutation of the columns, so a channels-last conv weight is orthogonalised as stored).  Its
// bf16 operand X lives in a packed workspace in the WIDE orientation (m <= n, transposed on the way in and out if needed), padded
// with zero rows and columns to multiples of 64: zero rows of X give zero rows / columns of A and B and zero rows of X', zero
// columns add nothing to X X^T, so no loop below has an edge predicate and any m, n >= 1 is served.
//
// One launch per stage covers every problem (prefix sums of tile counts in the table):
//   stage 1  A  = X X^T             NT, only tiles with tile-row <= tile-column, mirror stored
//   stage 2  B  = b A + c A A       NT (A is symmetric: A A = A A^T), same tile set, b A added in the epilogue
//   stage 3  X' = a X + B X         NN: the X tile is staged as stored ([k][column]) and read with ds_read_b64_tr_b16
// fp32 accumulation, fp32 epilogue, ONE rounding to bf16 per stored matrix; X ping-pongs between two buffers.
//
// The diagonals of A and B carry most of their weight (the rows of a normalised operand are nearly orthogonal), and the update
// a X + B X cancels: at convergence B_ii is about -2.7 against a result of 0.7, so the bf16 rounding of the DIAGONAL of B alone
// costs 4 x 2^-9 per row and iteration.  The fp32 residuals of the two diagonals (what rounding to bf16 took away: dA, dB, one
// float per row) are therefore kept and put back in the fp32 epilogues, to first order:
//   B_ij = (b + c (dA_i + dA_j)) A_ij + c (A A)_ij + [i = j] b dA_i,      X'_ij = (a + dB_i) X_ij + (B X)_ij.
// That halves the distance to float64 arithmetic at no cost; with integer operands the residuals are 0.
#include "common.h"
#include "saicv_internal.h"
#include "../../include/saicv_hip.h"

namespace {

constexpr int kTab = 13;            // ints per problem
enum { T_XOFF = 0, T_AOFF, T_MP, T_NP, T_SYM0, T_FULL0, T_BLK0, T_COLS, T_TR, T_RATIO, T_M, T_N, T_DOFF };
// hyper table (floats): lr, wd, momentum, nesterov, beta1, beta2, eps, 1-beta1, 1-beta2
constexpr int TILE = 64;
constexpr int PITCH = TILE * 2 + 16;      // bytes per LDS row: 16-byte chunks stay aligned, rows start 4 banks apart
constexpr int kSlices = 32;               // partial sums of squares per problem

// ------------------------------------------------------------------------------------------------ prepare
// block_prob[block]: problem index of a Muon block, -1 for an AdamW-backup block, -2 for a block nobody steps.
__global__ __launch_bounds__(256) void muon_prepare_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ s1, float* __restrict__ s2,
                                                           const int32_t* __restrict__ block_prob,
                                                           const int32_t* __restrict__ tab, const float* __restrict__ hyper,
                                                           const float* __restrict__ inv_scale,
                                                           const float* __restrict__ found_inf,
                                                           const uint8_t* __restrict__ has_grad,
                                                           float* __restrict__ step_blk, bf16_t* __restrict__ xws) {
    if (found_inf && found_inf[0] != 0.f) return;
    const int prob = block_prob[blockIdx.x];
    if (prob < -1) return;
    if (has_grad && !has_grad[blockIdx.x]) return;
    const float is = inv_scale ? inv_scale[0] : 1.f;
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
    if (prob < 0) {
        // the reference's own AdamW: m = lerp(m, g, 1-b1); s = lerp(s, g^2, 1-b2); p *= 1 - lr wd;
        // p -= lr / scale * m / (eps + sqrt(s)), scale = (1 - b1^t) / sqrt(1 - b2^t): eps joins the UNCORRECTED root
        const float lr = hyper[0], wd = hyper[1], eps = hyper[6], omb1 = hyper[7], omb2 = hyper[8];
        const float t = step_blk[blockIdx.x] + 1.f;
        __syncthreads();                                     // every wavefront has read the old count
        if (threadIdx.x == 0) step_blk[blockIdx.x] = t;
        const float bc1 = -expm1f(t * log1pf(-omb1)), bc2 = -expm1f(t * log1pf(-omb2));
        const float step = lr * sqrtf(bc2) / bc1;
        f32x4 pv = *reinterpret_cast<f32x4*>(p + i);
        f32x4 mv = *reinterpret_cast<f32x4*>(s1 + i);
        f32x4 vv = *reinterpret_cast<f32x4*>(s2 + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float d = gv[k] * is;
            mv[k] = fmaf(omb1, d - mv[k], mv[k]);
            vv[k] = fmaf(omb2, d * d - vv[k], vv[k]);
            pv[k] *= (1.f - lr * wd);
            pv[k] = fmaf(-step, mv[k] / (eps + sqrtf(vv[k])), pv[k]);
        }
        *reinterpret_cast<f32x4*>(p + i) = pv;
        *reinterpret_cast<f32x4*>(s1 + i) = mv;
        *reinterpret_cast<f32x4*>(s2 + i) = vv;
        return;
    }
    const int32_t* T = tab + prob * kTab;
    const float mu = hyper[2];
    const bool nesterov = hyper[3] != 0.f;
    f32x4 mv = *reinterpret_cast<f32x4*>(s1 + i);
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float d = gv[k] * is;
        mv[k] = fmaf(mu, mv[k], d);
        v[k] = nesterov ? fmaf(mu, mv[k], d) : mv[k];
    }
    *reinterpret_cast<f32x4*>(s1 + i) = mv;
    const int cols = T[T_COLS], np = T[T_NP], numel = T[T_M] * T[T_N];
    const bool tr = T[T_TR] != 0;
    bf16_t* x = xws + (size_t)T[T_XOFF];
    const int e0 = ((int)blockIdx.x - T[T_BLK0]) * 1024 + (int)threadIdx.x * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int e = e0 + k;
        if (e < numel) {                                     // the arena pads a parameter to a multiple of 1024
            const int r = e / cols, c = e - r * cols;
            x[tr ? (size_t)c * np + r : (size_t)r * np + c] = (bf16_t)v[k];
        }
    }
}

// ------------------------------------------------------------------------------------------------ normalisation
// ||X||^2 per problem in two ORDERED steps (always, not only in deterministic mode): kSlices block partials, each a fixed
// chunk range summed in a fixed order; the scale kernel folds the kSlices partials in index order.
__global__ __launch_bounds__(256) void muon_sumsq_kernel(const bf16_t* __restrict__ xws, const int32_t* __restrict__ tab,
                                                         float* __restrict__ partials) {
    __shared__ float wsum[4];
    const int32_t* T = tab + blockIdx.y * kTab;
    const int chunks = T[T_MP] * (T[T_NP] / 8);
    const int per = (chunks + kSlices - 1) / kSlices;
    const int c0 = blockIdx.x * per, c1 = min(chunks, c0 + per);
    const u32x4* x = reinterpret_cast<const u32x4*>(xws + (size_t)T[T_XOFF]);
    float ss = 0.f;
    for (int c = c0 + threadIdx.x; c < c1; c += 256) {
        float f[8];
        Chunk<bf16_t>::unpack(x[c], f);
#pragma unroll
        for (int k = 0; k < 8; ++k) ss = fmaf(f[k], f[k], ss);
    }
    ss = wave_sum(ss);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = ss;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.y * kSlices + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// X = bf16(X / (||X|| + 1e-7)); an all-zero X stays zero
__global__ __launch_bounds__(256) void muon_scale_kernel(bf16_t* __restrict__ xws, const int32_t* __restrict__ tab,
                                                         const float* __restrict__ partials) {
    const int32_t* T = tab + blockIdx.y * kTab;
    float ss = 0.f;
    for (int k = 0; k < kSlices; ++k) ss += partials[blockIdx.y * kSlices + k];
    const float inv = 1.f / (sqrtf(ss) + 1e-7f);
    const int chunks = T[T_MP] * (T[T_NP] / 8);
    u32x4* x = reinterpret_cast<u32x4*>(xws + (size_t)T[T_XOFF]);
    for (int c = blockIdx.x * 256 + threadIdx.x; c < chunks; c += gridDim.x * 256) {
        float f[8];
        Chunk<bf16_t>::unpack(x[c], f);
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] *= inv;
        x[c] = Chunk<bf16_t>::pack(f);
    }
}

// ------------------------------------------------------------------------------------------------ grouped GEMMs
// 64 x 64 tile per workgroup, four wavefronts of 32 x 32 (2 x 2 MFMA 16x16x32 bf16), K in steps of 64 through LDS with the
// next step's global loads in flight during the MFMAs.
template <int STAGE>
__global__ __launch_bounds__(256) void muon_ns_gemm_kernel(const bf16_t* __restrict__ xin, bf16_t* __restrict__ xout,
                                                           bf16_t* __restrict__ amat, bf16_t* __restrict__ bmat,
                                                           float* __restrict__ da, float* __restrict__ db,
                                                           const int32_t* __restrict__ tab, int nprob, float coef0,
                                                           float coef1) {
    __shared__ __attribute__((aligned(16))) char smem[2 * TILE * PITCH];
    constexpr int field = STAGE == 3 ? T_FULL0 : T_SYM0;
    int lo = 0, hi = nprob - 1;
    while (lo < hi) {                                       // last problem whose first tile is <= this block (uniform)
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid * kTab + field] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const int32_t* T = tab + lo * kTab;
    const int mp = T[T_MP], np = T[T_NP];
    int t = (int)blockIdx.x - T[field], ti = 0, tj;
    if constexpr (STAGE == 3) {
        const int tn = np / TILE;
        ti = t / tn;
        tj = t - ti * tn;
    } else {
        const int tm = mp / TILE;                           // row ti of the upper triangle holds tm - ti tiles
        while (t >= tm - ti) { t -= tm - ti; ++ti; }
        tj = ti + t;
    }
    const size_t xoff = (size_t)T[T_XOFF], aoff = (size_t)T[T_AOFF];
    const int doff = T[T_DOFF];
    const bf16_t *P, *Q;
    int ldp, ldq, K;
    if constexpr (STAGE == 1) {
        P = xin + xoff + (size_t)ti * TILE * np; Q = xin + xoff + (size_t)tj * TILE * np; ldp = ldq = np; K = np;
    } else if constexpr (STAGE == 2) {
        P = amat + aoff + (size_t)ti * TILE * mp; Q = amat + aoff + (size_t)tj * TILE * mp; ldp = ldq = mp; K = mp;
    } else {
        P = bmat + aoff + (size_t)ti * TILE * mp; Q = xin + xoff + (size_t)tj * TILE; ldp = mp; ldq = np; K = mp;
    }

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wr = w >> 1, wc = w & 1;
    const int l15 = lane & 15, lg = lane >> 4;
    char* sP = smem;
    char* sQ = smem + TILE * PITCH;

    u32x4 rp[2], rq[2];
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int q = tid + 256 * i, row = q >> 3, ch = q & 7;
            rp[i] = ld_chunk(P + (size_t)row * ldp + k0 + ch * 8);
            if constexpr (STAGE == 3) rq[i] = ld_chunk(Q + (size_t)(k0 + row) * ldq + ch * 8);      // rows are k
            else rq[i] = ld_chunk(Q + (size_t)row * ldq + k0 + ch * 8);
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int q = tid + 256 * i, row = q >> 3, ch = q & 7;
            st_chunk(sP + row * PITCH + ch * 16, rp[i]);
            st_chunk(sQ + row * PITCH + ch * 16, rq[i]);
        }
    };

    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
    load(0);
    for (int k0 = 0; k0 < K; k0 += TILE) {
        __syncthreads();                                    // the previous step's fragments are read
        stage();
        __syncthreads();
        if (k0 + TILE < K) load(k0 + TILE);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            u32x4 af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
                af[i] = ld_chunk(sP + (wr * 32 + i * 16 + l15) * PITCH + (ks * 32 + lg * 8) * 2);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if constexpr (STAGE == 3) {
                    // ds_read_b64_tr_b16: a 16-lane group reads a [4 rows][16 columns] block; lane t supplies the 8-byte
                    // address of row t >> 2, columns 4 (t & 3) ..., and receives column t of the four rows.  Every lane is
                    // active here (no divergence above), every address is 8-byte aligned (PITCH and the column offset are).
                    const char* q = sQ + (ks * 32 + lg * 8 + (l15 >> 2)) * PITCH + (wc * 32 + j * 16 + (l15 & 3) * 4) * 2;
                    const bf16x4 l4 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(q));
                    const bf16x4 h4 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(q + 4 * PITCH));
                    const u32x2 l2 = __builtin_bit_cast(u32x2, l4), h2 = __builtin_bit_cast(u32x2, h4);
                    bf[j] = u32x4{l2[0], l2[1], h2[0], h2[1]};
                } else {
                    bf[j] = ld_chunk(sQ + (wc * 32 + j * 16 + l15) * PITCH + (ks * 32 + lg * 8) * 2);
                }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) Mma<bf16_t>::run(acc[i][j], af[i], bf[j]);
        }
    }

    // epilogue: accumulator (i, j) holds rows r0 .. r0 + 3 of column c (guide section 3: col = lane & 15, row = 4 (lane >> 4) + reg)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int r0 = ti * TILE + wr * 32 + i * 16 + lg * 4, c = tj * TILE + wc * 32 + j * 16 + l15;
            bf16x4 out;
            if constexpr (STAGE == 3) {
                const bf16_t* xo = xin + xoff;
                bf16_t* xn = xout + xoff;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    out[r] = (bf16_t)fmaf(coef0 + db[doff + r0 + r], (float)xo[(size_t)(r0 + r) * np + c], acc[i][j][r]);
                    xn[(size_t)(r0 + r) * np + c] = out[r];
                }
            } else {
                bf16_t* dst = (STAGE == 1 ? amat : bmat) + aoff;
                float* dres = (STAGE == 1 ? da : db) + doff;             // this stage's diagonal residuals
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = acc[i][j][r];
                    if constexpr (STAGE == 2) {
                        const float dr = da[doff + r0 + r], dc = da[doff + c];
                        v = fmaf(fmaf(coef1, dr + dc, coef0), (float)amat[aoff + (size_t)(r0 + r) * mp + c], coef1 * v);
                        if (r0 + r == c) v = fmaf(coef0, dr, v);
                    }
                    out[r] = (bf16_t)v;
                    dst[(size_t)(r0 + r) * mp + c] = out[r];
                    if (r0 + r == c) dres[c] = v - (float)out[r];        // (every diagonal element belongs to exactly one lane)
                }
                if (ti != tj) *reinterpret_cast<bf16x4*>(dst + (size_t)c * mp + r0) = out;       // the mirror tile
            }
        }
}

// ------------------------------------------------------------------------------------------------ apply
// p = p (1 - lr wd) - lr ratio u, u read back through the orientation and the padding of the workspace
__global__ __launch_bounds__(256) void muon_apply_kernel(float* __restrict__ p, const bf16_t* __restrict__ uws,
                                                         const int32_t* __restrict__ block_prob,
                                                         const int32_t* __restrict__ tab, const float* __restrict__ hyper,
                                                         const float* __restrict__ found_inf,
                                                         const uint8_t* __restrict__ has_grad) {
    if (found_inf && found_inf[0] != 0.f) return;
    const int prob = block_prob[blockIdx.x];
    if (prob < 0) return;
    if (has_grad && !has_grad[blockIdx.x]) return;
    const int32_t* T = tab + prob * kTab;
    const float lr = hyper[0], wd = hyper[1];
    const float step = lr * __int_as_float(T[T_RATIO]);
    const int cols = T[T_COLS], np = T[T_NP], numel = T[T_M] * T[T_N];
    const bool tr = T[T_TR] != 0;
    const bf16_t* u = uws + (size_t)T[T_XOFF];
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    const int e0 = ((int)blockIdx.x - T[T_BLK0]) * 1024 + (int)threadIdx.x * 4;
    f32x4 pv = *reinterpret_cast<f32x4*>(p + i);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int e = e0 + k;
        if (e < numel) {
            const int r = e / cols, c = e - r * cols;
            const float uv = (float)u[tr ? (size_t)c * np + r : (size_t)r * np + c];
            pv[k] = fmaf(-step, uv, pv[k] * (1.f - lr * wd));
        }
    }
    *reinterpret_cast<f32x4*>(p + i) = pv;
}

}  // namespace

namespace saicv {

extern "C" int saicv_muon_prepare(float* p, const float* g, float* s1, float* s2, const int32_t* block_prob, const int32_t* tab,
                                  const float* hyper, const float* inv_scale, const float* found_inf, const uint8_t* has_grad,
                                  float* step_blk, void* xws, size_t n, void* stream) {
    hipStream_t st = S(stream);
    SAICV_REQUIRE(n % 1024 == 0 && n > 0, "muon_prepare: arena length %zu must be a positive multiple of 1024", n);
    SAICV_REQUIRE(step_blk != nullptr && block_prob != nullptr, "muon_prepare: the per-block tables are required");
    hipLaunchKernelGGL(muon_prepare_kernel, dim3((unsigned)(n / 1024)), dim3(256), 0, st, p, g, s1, s2, block_prob, tab, hyper,
                       inv_scale, found_inf, has_grad, step_blk, (bf16_t*)xws);
    return check_launch("muon_prepare");
}

// X (in x0) -> NS(X): after `steps` iterations the result is in x0 for an even count, in x1 for an odd one.
extern "C" int saicv_muon_newton_schulz(void* x0, void* x1, void* amat, void* bmat, float* da, float* db, const int32_t* tab, int nprob, int tiles_sym,
                                        int tiles_full, int steps, double a, double b, double c, int normalize, float* partials,
                                        void* stream) {
    hipStream_t st = S(stream);
    SAICV_REQUIRE(nprob >= 0 && steps >= 0, "muon_newton_schulz: %d problems, %d steps", nprob, steps);
    if (nprob == 0) return 0;
    SAICV_REQUIRE(x0 && x1 && amat && bmat && da && db && tab && tiles_sym > 0 && tiles_full > 0,
                  "muon_newton_schulz: null workspace or empty tile counts");
    if (normalize) {
        SAICV_REQUIRE(partials != nullptr, "muon_newton_schulz: normalize needs the partials scratch (32 floats per problem)");
        hipLaunchKernelGGL(muon_sumsq_kernel, dim3(kSlices, nprob), dim3(256), 0, st, (const bf16_t*)x0, tab, partials);
        hipLaunchKernelGGL(muon_scale_kernel, dim3(64, nprob), dim3(256), 0, st, (bf16_t*)x0, tab, partials);
    }
    bf16_t* xs[2] = {(bf16_t*)x0, (bf16_t*)x1};
    for (int s = 0; s < steps; ++s) {
        const bf16_t* xin = xs[s & 1];
        bf16_t* xout = xs[(s + 1) & 1];
        hipLaunchKernelGGL(muon_ns_gemm_kernel<1>, dim3(tiles_sym), dim3(256), 0, st, xin, xout, (bf16_t*)amat, (bf16_t*)bmat, da, db, tab,
                           nprob, 0.f, 0.f);
        hipLaunchKernelGGL(muon_ns_gemm_kernel<2>, dim3(tiles_sym), dim3(256), 0, st, xin, xout, (bf16_t*)amat, (bf16_t*)bmat, da, db, tab,
                           nprob, (float)b, (float)c);
        hipLaunchKernelGGL(muon_ns_gemm_kernel<3>, dim3(tiles_full), dim3(256), 0, st, xin, xout, (bf16_t*)amat, (bf16_t*)bmat, da, db, tab,
                           nprob, (float)a, 0.f);
    }
    return check_launch("muon_newton_schulz");
}

extern "C" int saicv_muon_apply(float* p, const void* uws, const int32_t* block_prob, const int32_t* tab, const float* hyper,
                                const float* found_inf, const uint8_t* has_grad, size_t n, void* stream) {
    hipStream_t st = S(stream);
    SAICV_REQUIRE(n % 1024 == 0 && n > 0, "muon_apply: arena length %zu must be a positive multiple of 1024", n);
    hipLaunchKernelGGL(muon_apply_kernel, dim3((unsigned)(n / 1024)), dim3(256), 0, st, p, (const bf16_t*)uws, block_prob, tab, hyper,
                       found_inf, has_grad);
    return check_launch("muon_apply");
}

}  // namespace saicv
