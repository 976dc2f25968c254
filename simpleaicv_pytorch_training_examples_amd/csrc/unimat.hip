// The streaming passes of universal matting (SimpleAICV/universal_segmentation/matting_losses.py, models/dinov3_universal_matting.py).
//
// (a) pair sums for the Hungarian matcher, the whole batch in one launch pair.  With g, l, f clamped to [1e-4, 1 - 1e-4], k the
//     trimap class of target t at pixel p (255 -> 2, else anything > 2 -> 1, else the integer part) and w = [trimap == 128], per image,
//     query q and target t over the P pixels:
//       Cpos = sum -log g[q,k]    Cneg = sum_p sum_{c != k} -log(1 - g[q,c])    I = sum g[q,k]    L = sum w |l - a|    F = sum |f - a|
//     and G[q] = sum_p sum_c g, W[t] = sum_p w.  The predictions are read in place through strides, pixel-fastest ([B, Q, 3, H, W]
//     contiguous) or channel-fastest ([B, H, W, 3Q] memory) alike: a workgroup stages a tile of UM_QT queries x UM_PT pixels in LDS,
//     and the six logarithms of a (query, pixel) are taken there, once for the workgroup's up to UM_TG targets (one workgroup serves
//     all targets of an image that has no more than that).  The targets' trimap and alpha values of the tile sit in LDS next to them
//     and serve every query.  A thread then owns one query and one of UM_SLICES pixel slices and adds SELECTED terms (never
//     total - part) in pixel order; the slices are added in slice order, the chunks of UM_CHUNK pixels in chunk order by the
//     ordered_sum.h tree.  No atomics: the bits of an image's sums depend on (Q, T_i, P) alone.
// (b) the head: sigmoid of the global (3Q channels) and local (Q channels) logits in channels-last memory, bf16 or fp32, and
//     fused = local [argmax == 1] + [argmax == 2] over the first maximum of the three fp32 PROBABILITIES, one read and one write per
//     element; its backward writes both logit gradients in one pass.
#include "common.h"
#include "saicv_internal.h"
#include "../../include/saicv_hip.h"
#include "ordered_sum.h"

namespace {

constexpr int UM_THREADS = 256;                  // four wavefronts (ordered_sum.h)
constexpr int UM_CHUNK = 4096;                   // pixels per workgroup, a multiple of UM_PT
constexpr int UM_QT = 32;                        // queries per workgroup
constexpr int UM_PT = 32;                        // pixels per staged tile
constexpr int UM_SLICES = UM_THREADS / UM_QT;    // pixel slices of a tile, one per (thread / UM_QT)
constexpr int UM_SPIX = UM_PT / UM_SLICES;       // consecutive pixels of a slice
constexpr int UM_TG = 8;                         // targets per workgroup at most
constexpr int UM_VALS = 11;                      // staged per (query, pixel): -log g [3], -log(1 - g) [3], g [3], l, f
constexpr int UM_VSTR = UM_QT + 1;               // odd strides keep the staging stores off one LDS bank
constexpr int UM_PSTR = UM_VALS * UM_VSTR;
constexpr int UM_UNITS = UM_QT * 5 * UM_PT / 4;  // 16-byte units of a tile: (3 + 1 + 1) maps
constexpr int UM_NACC = 6;                       // Cpos, Cneg, I, L, F, W
constexpr int UM_FOLD = 16;                      // totals per stage-2 workgroup
constexpr float UM_LO = 1e-4f, UM_HI = 1.f - 1e-4f;

static_assert(UM_CHUNK % UM_PT == 0 && UM_PT % 4 == 0 && UM_QT % 4 == 0 && UM_UNITS % UM_THREADS == 0, "tile shapes");
static_assert(UM_SLICES * UM_NACC * UM_QT <= UM_PT * UM_PSTR, "the slice reduction reuses the staging buffer");

struct PredView {                                // element strides over image, query, channel, pixel
    const float *g, *l, *f;
    long gsb, gsq, gsc, gsp, lsb, lsq, lsp, fsb, fsq, fsp;
};

struct Elem {
    int q, v, p;                                 // query and pixel inside the tile; v: 0..2 global channel, 3 local, 4 fused
};

// element e of 16-byte unit u.  Pixel-fastest: a unit is four pixels of one (query, map) row.  Channel-fastest: a pixel owns 40
// units, 24 over its 96 global channels (channel 3 q + c), 8 over the local and 8 over the fused values.
template <bool CL>
DEVINL Elem unit_elem(int u, int e) {
    Elem r;
    if constexpr (!CL) {
        const int row = u / (UM_PT / 4);
        r.q = row / 5;
        r.v = row - 5 * r.q;
        r.p = (u - row * (UM_PT / 4)) * 4 + e;
    } else {
        constexpr int per = 5 * UM_QT / 4, gl = 3 * UM_QT / 4, lo = UM_QT / 4;
        r.p = u / per;
        const int piece = u - r.p * per;
        if (piece < gl) {
            const int ch = 4 * piece + e;
            r.q = ch / 3;
            r.v = ch - 3 * r.q;
        } else if (piece < gl + lo) {
            r.q = 4 * (piece - gl) + e;
            r.v = 3;
        } else {
            r.q = 4 * (piece - gl - lo) + e;
            r.v = 4;
        }
    }
    return r;
}

DEVINL const float* elem_addr(const PredView& v, int b, int q, int c, size_t pix) {
    if (c < 3) return v.g + (size_t)b * v.gsb + (size_t)q * v.gsq + (size_t)c * v.gsc + pix * v.gsp;
    if (c == 3) return v.l + (size_t)b * v.lsb + (size_t)q * v.lsq + pix * v.lsp;
    return v.f + (size_t)b * v.fsb + (size_t)q * v.fsq + pix * v.fsp;
}

DEVINL float um_clamp(float x) { return fminf(fmaxf(x, UM_LO), UM_HI); }
DEVINL float pick3(int k, float a0, float a1, float a2) { return k == 0 ? a0 : (k == 1 ? a1 : a2); }
// Kahan: s += x with the rounding of the previous additions carried in c
DEVINL void comp_add(float& s, float& c, float x) {
    const float y = x - c;
    const float t = s + y;
    c = (t - s) - y;
    s = t;
}
DEVINL int um_class(float t) { return t == 255.f ? 2 : (t > 2.f ? 1 : (int)t); }

// partial [nchunks][ld]; a row holds five planes [Q][TT] (Cpos, Cneg, I, L, F; column off_i + t), then G [B][Q], then W [TT]
template <int NT, bool CL>
__global__ __launch_bounds__(UM_THREADS) void um_pair_kernel(PredView v, const float* __restrict__ trimap,
                                                             const float* __restrict__ alpha, const int* __restrict__ offsets,
                                                             float* __restrict__ partial, int B, int Q, int TT, size_t P, size_t ld,
                                                             int qblocks, bool vec) {
    __shared__ float stage[UM_PT * UM_PSTR];
    __shared__ float tgt[2][NT][UM_PT];
    const int tid = threadIdx.x;
    const int b = blockIdx.z;
    const int qb = blockIdx.y % qblocks, tg = blockIdx.y / qblocks;
    const int off = offsets[b], Ti = offsets[b + 1] - off;
    const int tbase = tg * NT;
    float* prow = partial + (size_t)blockIdx.x * ld;
    const size_t plane = (size_t)Q * TT;
    const size_t ncols = 5 * plane + (size_t)B * Q + TT;
    if (b == 0 && blockIdx.y == 0 && ncols + tid < ld) prow[ncols + tid] = 0.f;        // the padding the fold reads
    if (tg > 0 && tbase >= Ti) return;
    const int nt = Ti > tbase ? min(NT, Ti - tbase) : 0;
    const int q0 = qb * UM_QT;
    const int ql = tid % UM_QT, slice = tid / UM_QT;
    const bool qok = q0 + ql < Q;
    const size_t p0 = (size_t)blockIdx.x * UM_CHUNK;
    const size_t end = min(P, p0 + UM_CHUNK);

    float acc[NT][UM_NACC], comp[NT][UM_NACC];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int j = 0; j < UM_NACC; ++j) acc[t][j] = comp[t][j] = 0.f;
    float gsum = 0.f, gcomp = 0.f;

    for (size_t pt = p0; pt < end; pt += UM_PT) {
        // stage: clamp, and take every logarithm of the tile once
        for (int u = tid; u < UM_UNITS; u += UM_THREADS) {
            const Elem e0 = unit_elem<CL>(u, 0), e3 = unit_elem<CL>(u, 3);
            float x[4];
            if (vec && q0 + e3.q < Q && pt + e3.p < end) {
                Chunk<float>::unpack(ld_chunk(elem_addr(v, b, q0 + e0.q, e0.v, pt + e0.p)), x);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const Elem el = unit_elem<CL>(u, e);
                    x[e] = (q0 + el.q < Q && pt + el.p < end) ? *elem_addr(v, b, q0 + el.q, el.v, pt + el.p) : 0.5f;
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const Elem el = unit_elem<CL>(u, e);
                float* s = stage + el.p * UM_PSTR + el.q;
                const float c = um_clamp(x[e]);
                if (el.v < 3) {
                    s[el.v * UM_VSTR] = -logf(c);
                    s[(el.v + 3) * UM_VSTR] = -log1pf(-c);                  // 1 - c itself would round c away where c is small
                    s[(el.v + 6) * UM_VSTR] = c;
                } else {
                    s[(el.v + 6) * UM_VSTR] = c;
                }
            }
        }
        for (int i = tid; i < nt * 2 * UM_PT; i += UM_THREADS) {
            const int t = i / (2 * UM_PT), m = (i / UM_PT) & 1, p = i % UM_PT;
            const float* src = m ? alpha : trimap;
            tgt[m][t][p] = pt + p < end ? src[(size_t)(off + tbase + t) * P + pt + p] : 0.f;
        }
        __syncthreads();
        if (qok) {
            // the slice's pixels of this tile are added first; the tile's sum then joins the chunk's by a compensated addition (a
            // plain sequential sum of a chunk lay 5.7e-7 of its magnitude from float64, past what the reference's own fp32 run allows)
            float ta[NT][UM_NACC];
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int j = 0; j < UM_NACC; ++j) ta[t][j] = 0.f;
            float tgs = 0.f;
#pragma unroll
            for (int j = 0; j < UM_SPIX; ++j) {
                const int p = slice * UM_SPIX + j;
                if (pt + p < end) {
                    const float* s = stage + p * UM_PSTR + ql;
                    const float nl0 = s[0], nl1 = s[UM_VSTR], nl2 = s[2 * UM_VSTR];
                    const float nm0 = s[3 * UM_VSTR], nm1 = s[4 * UM_VSTR], nm2 = s[5 * UM_VSTR];
                    const float g0 = s[6 * UM_VSTR], g1 = s[7 * UM_VSTR], g2 = s[8 * UM_VSTR];
                    const float l = s[9 * UM_VSTR], f = s[10 * UM_VSTR];
                    const float o0 = nm1 + nm2, o1 = nm0 + nm2, o2 = nm0 + nm1;        // the two other channels of each class
                    tgs += (g0 + g1) + g2;
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        if (t < nt) {
                            const float tv = tgt[0][t][p], a = tgt[1][t][p];
                            const int k = um_class(tv);
                            const bool w = tv == 128.f;
                            ta[t][0] += pick3(k, nl0, nl1, nl2);
                            ta[t][1] += pick3(k, o0, o1, o2);
                            ta[t][2] += pick3(k, g0, g1, g2);
                            ta[t][3] += w ? fabsf(l - a) : 0.f;
                            ta[t][4] += fabsf(f - a);
                            ta[t][5] += w ? 1.f : 0.f;
                        }
                    }
                }
            }
            comp_add(gsum, gcomp, tgs);
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int j = 0; j < UM_NACC; ++j) comp_add(acc[t][j], comp[t][j], ta[t][j]);
        }
        __syncthreads();
    }

    // the slices of a query, in slice order
    float* red = stage;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t < nt) {
#pragma unroll
            for (int j = 0; j < UM_NACC; ++j) red[(slice * UM_NACC + j) * UM_QT + ql] = acc[t][j];
            __syncthreads();
            if (tid < UM_NACC * UM_QT) {
                const int j = tid / UM_QT, q = tid % UM_QT;
                float sum = red[j * UM_QT + q];
                for (int s = 1; s < UM_SLICES; ++s) sum += red[(s * UM_NACC + j) * UM_QT + q];
                if (q0 + q < Q) {
                    const size_t col = (size_t)off + tbase + t;
                    if (j < 5)
                        prow[j * plane + (size_t)(q0 + q) * TT + col] = sum;
                    else if (qb == 0 && q == 0)
                        prow[5 * plane + (size_t)B * Q + col] = sum;
                }
            }
            __syncthreads();
        }
    }
    if (tg == 0) {
        red[slice * UM_QT + ql] = gsum;
        __syncthreads();
        if (tid < UM_QT && q0 + tid < Q) {
            float sum = red[tid];
            for (int s = 1; s < UM_SLICES; ++s) sum += red[s * UM_QT + tid];
            prow[5 * plane + (size_t)b * Q + q0 + tid] = sum;
        }
    }
}

// stage 2 over partial [n][ld] -> out [ncols], UM_FOLD totals per workgroup (ld is a multiple of UM_FOLD)
__global__ __launch_bounds__(UM_THREADS) void um_fold_kernel(const float* __restrict__ partial, int n, size_t ld, size_t ncols,
                                                             float* __restrict__ out) {
    const size_t c0 = (size_t)blockIdx.x * UM_FOLD;
    float s[UM_FOLD];
#pragma unroll
    for (int j = 0; j < UM_FOLD; ++j) s[j] = 0.f;
    for (int i = threadIdx.x; i < n; i += UM_THREADS) {
#pragma unroll
        for (int j = 0; j < UM_FOLD; ++j) s[j] += partial[(size_t)i * ld + c0 + j];
    }
#pragma unroll
    for (int j = 0; j < UM_FOLD; ++j) s[j] = wave_sum(s[j]);
    const float v = block_tree<UM_FOLD>(s);
    if (threadIdx.x < UM_FOLD && c0 + threadIdx.x < ncols) out[c0 + threadIdx.x] = v;
}

// ---------------------------------------------------------------- head
DEVINL float um_sigmoid(float x) {
    const float e = expf(-fabsf(x));
    return x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}
DEVINL int first_max3(float a0, float a1, float a2) {                    // torch.max: the first maximum
    int k = 0;
    float m = a0;
    if (a1 > m) { m = a1; k = 1; }
    if (a2 > m) k = 2;
    return k;
}

// n values from p; vec: n == 4 and p is aligned to four elements
template <typename T>
DEVINL void load4(const T* p, int n, bool vec, float (&x)[4]) {
    if (vec) {
        if constexpr (sizeof(T) == 2) {
            const u32x2 c = *reinterpret_cast<const u32x2*>(p);
            x[0] = __uint_as_float(c[0] << 16);
            x[1] = __uint_as_float(c[0] & 0xffff0000u);
            x[2] = __uint_as_float(c[1] << 16);
            x[3] = __uint_as_float(c[1] & 0xffff0000u);
        } else {
            Chunk<float>::unpack(ld_chunk(p), x);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = k < n ? to_f32(p[k]) : 0.f;
    }
}
template <typename T>
DEVINL void store4(T* p, int n, bool vec, const float (&x)[4]) {
    if (vec) {
        if constexpr (sizeof(T) == 2) {
            u32x2 c;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                bf16x2 h;
                h[0] = (bf16_t)x[2 * i];
                h[1] = (bf16_t)x[2 * i + 1];
                c[i] = __builtin_bit_cast(uint32_t, h);
            }
            *reinterpret_cast<u32x2*>(p) = c;
        } else {
            st_chunk(p, Chunk<float>::pack(x));
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) p[k] = from_f32<T>(x[k]);
    }
}

// a thread takes four queries of one pixel: 12 global channels and 4 local ones
template <typename T>
__global__ __launch_bounds__(UM_THREADS) void um_head_fwd_kernel(const T* __restrict__ gl, const T* __restrict__ ll,
                                                                 float* __restrict__ g, float* __restrict__ l, float* __restrict__ f,
                                                                 size_t rows, int Q, bool vec) {
    const int groups = (Q + 3) / 4;
    const size_t i = (size_t)blockIdx.x * UM_THREADS + threadIdx.x;
    if (i >= rows * groups) return;
    const size_t row = i / groups;
    const int q = (int)(i - row * groups) * 4;
    const int n = min(4, Q - q);
    const size_t go = row * 3 * Q + 3 * q, lo = row * Q + q;
    float x[3][4], y[4], pg[3][4], pl[4], pf[4];
#pragma unroll
    for (int j = 0; j < 3; ++j) load4<T>(gl + go + 4 * j, 3 * n - 4 * j, vec, x[j]);
    load4<T>(ll + lo, n, vec, y);
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) pg[j][k] = um_sigmoid(x[j][k]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = 3 * k;
        const int a = first_max3(pg[c / 4][c % 4], pg[(c + 1) / 4][(c + 1) % 4], pg[(c + 2) / 4][(c + 2) % 4]);
        pl[k] = um_sigmoid(y[k]);
        pf[k] = a == 1 ? pl[k] : (a == 2 ? 1.f : 0.f);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) store4<float>(g + go + 4 * j, 3 * n - 4 * j, vec, pg[j]);
    store4<float>(l + lo, n, vec, pl);
    store4<float>(f + lo, n, vec, pf);
}

template <typename T>
__global__ __launch_bounds__(UM_THREADS) void um_head_bwd_kernel(const float* __restrict__ g, const float* __restrict__ l,
                                                                 const float* __restrict__ dg, const float* __restrict__ dl,
                                                                 const float* __restrict__ df, T* __restrict__ dgl, T* __restrict__ dll,
                                                                 size_t rows, int Q, bool vec) {
    const int groups = (Q + 3) / 4;
    const size_t i = (size_t)blockIdx.x * UM_THREADS + threadIdx.x;
    if (i >= rows * groups) return;
    const size_t row = i / groups;
    const int q = (int)(i - row * groups) * 4;
    const int n = min(4, Q - q);
    const size_t go = row * 3 * Q + 3 * q, lo = row * Q + q;
    float pg[3][4], gg[3][4], pl[4], gl4[4], gf[4], out[4];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        load4<float>(g + go + 4 * j, 3 * n - 4 * j, vec, pg[j]);
        load4<float>(dg + go + 4 * j, 3 * n - 4 * j, vec, gg[j]);
    }
    load4<float>(l + lo, n, vec, pl);
    load4<float>(dl + lo, n, vec, gl4);
    load4<float>(df + lo, n, vec, gf);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = 3 * k;
        const int a = first_max3(pg[c / 4][c % 4], pg[(c + 1) / 4][(c + 1) % 4], pg[(c + 2) / 4][(c + 2) % 4]);
        out[k] = (gl4[k] + (a == 1 ? gf[k] : 0.f)) * (pl[k] * (1.f - pl[k]));
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
        for (int k = 0; k < 4; ++k) gg[j][k] = gg[j][k] * (pg[j][k] * (1.f - pg[j][k]));
        store4<T>(dgl + go + 4 * j, 3 * n - 4 * j, vec, gg[j]);
    }
    store4<T>(dll + lo, n, vec, out);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool mult4(long s) { return s % 4 == 0; }
size_t pair_cols(int B, int Q, int TT) { return (size_t)5 * Q * TT + (size_t)B * Q + TT; }
size_t pair_ld(int B, int Q, int TT) { return (pair_cols(B, Q, TT) + UM_FOLD - 1) / UM_FOLD * UM_FOLD; }
int chunks_of(size_t P) { return (int)((P + UM_CHUNK - 1) / UM_CHUNK); }

template <int NT>
void launch_pair(bool cl, dim3 grid, hipStream_t st, const PredView& v, const float* trimap, const float* alpha, const int* offsets,
                 float* partial, int B, int Q, int TT, size_t P, size_t ld, int qblocks, bool vec) {
    if (cl)
        hipLaunchKernelGGL((um_pair_kernel<NT, true>), grid, dim3(UM_THREADS), 0, st, v, trimap, alpha, offsets, partial, B, Q, TT, P,
                           ld, qblocks, vec);
    else
        hipLaunchKernelGGL((um_pair_kernel<NT, false>), grid, dim3(UM_THREADS), 0, st, v, trimap, alpha, offsets, partial, B, Q, TT, P,
                           ld, qblocks, vec);
}

}  // namespace

namespace saicv {

extern "C" int saicv_unimat_chunk() { return UM_CHUNK; }

extern "C" size_t saicv_unimat_pair_ws_floats(int B, int Q, int TT, size_t P) { return (size_t)chunks_of(P) * pair_ld(B, Q, TT); }

extern "C" int saicv_unimat_pair_sums(const float* global_preds, long gsb, long gsq, long gsc, long gsp, const float* local_preds, long lsb,
                                      long lsq, long lsp, const float* fused_preds, long fsb, long fsq, long fsp, const float* trimaps,
                                      const float* alphas, const int* offsets, int B, int Q, int TT, int Tmax, size_t P, float* partial,
                                      float* sums, void* stream) {
    hipStream_t st = S(stream);
    SAICV_REQUIRE(B > 0 && Q > 0 && P > 0 && TT >= 0 && Tmax >= 0 && Tmax <= TT, "unimat_pair_sums: B=%d Q=%d P=%zu T=%d Tmax=%d", B, Q,
                  P, TT, Tmax);
    SAICV_REQUIRE(B <= 65535, "unimat_pair_sums: B=%d exceeds the grid's z extent", B);
    SAICV_REQUIRE(gsb >= 0 && gsq >= 0 && gsc >= 0 && gsp >= 0 && lsb >= 0 && lsq >= 0 && lsp >= 0 && fsb >= 0 && fsq >= 0 && fsp >= 0,
                  "unimat_pair_sums: a negative stride");
    const int nt = Tmax <= 1 ? 1 : (Tmax <= 4 ? 4 : UM_TG);
    const int nchunks = chunks_of(P);
    const int qblocks = (Q + UM_QT - 1) / UM_QT, tgroups = Tmax > 0 ? (Tmax + nt - 1) / nt : 1;
    SAICV_REQUIRE((size_t)qblocks * tgroups <= 65535, "unimat_pair_sums: Q=%d x Tmax=%d exceeds the grid's y extent", Q, Tmax);
    PredView v{global_preds, local_preds, fused_preds, gsb, gsq, gsc, gsp, lsb, lsq, lsp, fsb, fsq, fsp};
    const bool cl = gsc == 1 && gsq == 3;
    const bool base = aligned16(global_preds) && aligned16(local_preds) && aligned16(fused_preds) && mult4(gsb) && mult4(lsb) && mult4(fsb);
    const bool vec = cl ? base && lsq == 1 && fsq == 1 && mult4(gsp) && mult4(lsp) && mult4(fsp)
                        : base && gsp == 1 && lsp == 1 && fsp == 1 && mult4(gsq) && mult4(gsc) && mult4(lsq) && mult4(fsq);
    const size_t ld = pair_ld(B, Q, TT), ncols = pair_cols(B, Q, TT);
    dim3 grid(nchunks, qblocks * tgroups, B);
    if (nt == 1)
        launch_pair<1>(cl, grid, st, v, trimaps, alphas, offsets, partial, B, Q, TT, P, ld, qblocks, vec);
    else if (nt == 4)
        launch_pair<4>(cl, grid, st, v, trimaps, alphas, offsets, partial, B, Q, TT, P, ld, qblocks, vec);
    else
        launch_pair<UM_TG>(cl, grid, st, v, trimaps, alphas, offsets, partial, B, Q, TT, P, ld, qblocks, vec);
    if (check_launch("unimat_pair_sums")) return -2;
    hipLaunchKernelGGL(um_fold_kernel, dim3((unsigned)(ld / UM_FOLD)), dim3(UM_THREADS), 0, st, partial, nchunks, ld, ncols, sums);
    return check_launch("unimat_pair_fold");
}

extern "C" int saicv_unimat_head_fwd(int dtype, const void* global_logits, const void* local_logits, size_t rows, int Q, float* global_preds,
                                     float* local_preds, float* fused_preds, void* stream) {
    hipStream_t st = S(stream);
    SAICV_REQUIRE(rows > 0 && Q > 0, "unimat_head_fwd: rows=%zu Q=%d", rows, Q);
    SAICV_REQUIRE(dtype == SAICV_DTYPE_BF16 || dtype == SAICV_DTYPE_F32, "unimat_head_fwd: dtype %d", dtype);
    const size_t items = rows * ((Q + 3) / 4), blocks = (items + UM_THREADS - 1) / UM_THREADS;
    SAICV_REQUIRE(blocks <= 0x7fffffffu, "unimat_head_fwd: rows=%zu Q=%d exceed the grid", rows, Q);
    const bool vec = Q % 4 == 0 && aligned16(global_logits) && aligned16(local_logits) && aligned16(global_preds) &&
                     aligned16(local_preds) && aligned16(fused_preds);
    if (dtype == SAICV_DTYPE_BF16)
        hipLaunchKernelGGL(um_head_fwd_kernel<bf16_t>, dim3((unsigned)blocks), dim3(UM_THREADS), 0, st, (const bf16_t*)global_logits,
                           (const bf16_t*)local_logits, global_preds, local_preds, fused_preds, rows, Q, vec);
    else
        hipLaunchKernelGGL(um_head_fwd_kernel<float>, dim3((unsigned)blocks), dim3(UM_THREADS), 0, st, (const float*)global_logits,
                           (const float*)local_logits, global_preds, local_preds, fused_preds, rows, Q, vec);
    return check_launch("unimat_head_fwd");
}

extern "C" int saicv_unimat_head_bwd(int dtype, const float* global_preds, const float* local_preds, const float* dglobal_preds,
                                     const float* dlocal_preds, const float* dfused_preds, size_t rows, int Q, void* dglobal_logits,
                                     void* dlocal_logits, void* stream) {
    hipStream_t st = S(stream);
    SAICV_REQUIRE(rows > 0 && Q > 0, "unimat_head_bwd: rows=%zu Q=%d", rows, Q);
    SAICV_REQUIRE(dtype == SAICV_DTYPE_BF16 || dtype == SAICV_DTYPE_F32, "unimat_head_bwd: dtype %d", dtype);
    const size_t items = rows * ((Q + 3) / 4), blocks = (items + UM_THREADS - 1) / UM_THREADS;
    SAICV_REQUIRE(blocks <= 0x7fffffffu, "unimat_head_bwd: rows=%zu Q=%d exceed the grid", rows, Q);
    const bool vec = Q % 4 == 0 && aligned16(global_preds) && aligned16(local_preds) && aligned16(dglobal_preds) &&
                     aligned16(dlocal_preds) && aligned16(dfused_preds) && aligned16(dglobal_logits) && aligned16(dlocal_logits);
    if (dtype == SAICV_DTYPE_BF16)
        hipLaunchKernelGGL(um_head_bwd_kernel<bf16_t>, dim3((unsigned)blocks), dim3(UM_THREADS), 0, st, global_preds, local_preds,
                           dglobal_preds, dlocal_preds, dfused_preds, (bf16_t*)dglobal_logits, (bf16_t*)dlocal_logits, rows, Q, vec);
    else
        hipLaunchKernelGGL(um_head_bwd_kernel<float>, dim3((unsigned)blocks), dim3(UM_THREADS), 0, st, global_preds, local_preds,
                           dglobal_preds, dlocal_preds, dfused_preds, (float*)dglobal_logits, (float*)dlocal_logits, rows, Q, vec);
    return check_launch("unimat_head_bwd");
}

}  // namespace saicv
