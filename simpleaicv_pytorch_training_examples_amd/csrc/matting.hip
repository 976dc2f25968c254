// Human matting (reference 07.human_matting_training): what the seven losses of SimpleAICV/human_matting/losses.py read of the
// full-resolution fp32 maps, and collaborative_matting of SimpleAICV/human_matting/models/pfan_matting.py:434-454.
//
// Pixel kernels.  A workgroup owns 4096 consecutive pixels of one sample (256 lanes x 4 pixels x 4 rounds), reads every map once in
// 16-byte chunks and leaves one partial row; a second launch folds the rows of a sample (ordered_sum.h).  No atomics: every sum is
// bit-reproducible in every mode.  ph = clamp(p, float32(1e-4), float32(1 - 1e-4)); every backward takes dL/dsums from device
// memory and gives exactly 0 where p lies outside the clamp (bounds inclusive), as torch.clamp's backward does.
//   trimap_stats     global_pred [B][3][P] through three strides (NCHW-contiguous and channels-last alike), trimap [B][P] ->
//                    (sum of the 3-channel bce against the one-hot class, sum of 1 - (ph_k + s) / (sum ph + 1 - ph_k + s)).
//                    class: 255 -> 2, else anything > 2 -> 1, else (long)t  (losses.py:36-40 in the order it rewrites)
//   alpha_l1         (sum sqrt(((ph - alpha) w)^2 + 1e-12), sum w), w = [trimap == 128] or 1 (no trimap)
//   composition_l1   sum over 3 channels of sqrt((ph fg + (1 - ph) bg - image)^2 + 1e-12)
//   matting_fuse     fused = local [argmax == 1] + [argmax == 2], argmax = the first maximum of the three global probabilities
//
// Laplacian pyramid level.  cur [B][h][w] -> sum |cur - G * cur| and next = avg_pool2(G * cur) (an odd last row / column is
// dropped), G the 5x5 table passed by value, replicate padding 2.  At level 0 cur is formed while loading:
// (clamp(pred) - alpha) * w.  A workgroup owns a 32 x 32 tile: the 36 x 36 clamped neighbourhood sits in LDS, a lane forms four
// neighbouring outputs from five rows of eight values held in registers.  Backward is the exact adjoint,
// g_cur = gs sign(e) + G^T (P^T g_next - gs sign(e)): the tile's 40 x 40 neighbourhood gives e and its sign again on the 36 x 36
// ring (the same operations in the same order as forward, so the sign is the forward's), P^T spreads a quarter of g_next to the
// four pixels it averaged, and G^T is the adjoint of replicate padding -- a border pixel collects the taps that were clamped onto it.
#include "common.h"
#include "ordered_sum.h"
#include "saicv_internal.h"
#include "../../include/saicv_hip.h"

namespace {

constexpr int MT_SPAN = 4096;
constexpr float MT_LO = 1e-4f, MT_HI = 1.f - 1e-4f, MT_EPS = 1e-12f;

DEVINL float mt_clamp(float p) { return p < MT_LO ? MT_LO : (p > MT_HI ? MT_HI : p); }
DEVINL bool mt_inside(float p) { return p >= MT_LO && p <= MT_HI; }
DEVINL int mt_class(float t) { return t == 255.f ? 2 : (t > 2.f ? 1 : (int)t); }
DEVINL float mt_sign(float e) { return (e > 0.f ? 1.f : 0.f) - (e < 0.f ? 1.f : 0.f); }
DEVINL f32x4 mt_ld4(const float* p) { return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p)); }
DEVINL void mt_st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// one workgroup per sample: out[b * sb + j * sj] = sum of partial[b][0 .. nblk)[j] for j < NOUT of the NS columns of a partial row
template <int NS, int NOUT>
__global__ __launch_bounds__(256) void mt_fold_kernel(const float* __restrict__ partial, int nblk, float* __restrict__ out, long sb,
                                                      long sj) {
    const float total = fold_rows<NOUT>(partial + (size_t)blockIdx.x * nblk * NS, nblk, NS);
    if (threadIdx.x < NOUT) out[(size_t)blockIdx.x * sb + (int)threadIdx.x * sj] = total;
}

// ------------------------------------------------------------------------------------------------ three-channel maps
// mode 0: any strides, one pixel per lane; 1: planes (pixel stride 1), 2: interleaved (channel stride 1, pixel stride 3); in
// modes 1 and 2 four pixels are whole 16-byte chunks
struct Tri {
    size_t P;
    long sb, sc, sp;
    int mode;
    float smooth;
};

DEVINL void tri_load4(const float* g, const Tri& t, size_t i, float (&p)[4][3]) {
    if (t.mode == 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const f32x4 v = mt_ld4(g + c * t.sc + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) p[j][c] = v[j];
        }
    } else {
        float flat[12];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const f32x4 v = mt_ld4(g + i * 3 + q * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) flat[q * 4 + j] = v[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) p[j][c] = flat[j * 3 + c];
    }
}

DEVINL void tri_store4(float* g, const Tri& t, size_t i, const float (&p)[4][3]) {
    if (t.mode == 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = p[j][c];
            mt_st4(g + c * t.sc + i, v);
        }
    } else {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = p[(q * 4 + j) / 3][(q * 4 + j) % 3];
            mt_st4(g + i * 3 + q * 4, v);
        }
    }
}

DEVINL void tri_add(const float (&p)[3], float tv, float smooth, float (&s)[2]) {
    const int k = mt_class(tv);
    float ph[3], sum = 0.f, pk = 0.f, lab = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ph[c] = mt_clamp(p[c]);
        sum += ph[c];
        if (c == k) {
            pk = ph[c];
            lab = 1.f;
        }
        s[0] -= c == k ? logf(ph[c]) : logf(1.f - ph[c]);
    }
    s[1] += 1.f - (pk + smooth) / (((sum + lab) - pk) + smooth);
}

DEVINL void tri_grad(const float (&p)[3], float tv, float smooth, float g0, float g1, float (&d)[3]) {
    const int k = mt_class(tv);
    float ph[3], sum = 0.f, pk = 0.f, lab = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ph[c] = mt_clamp(p[c]);
        sum += ph[c];
        if (c == k) {
            pk = ph[c];
            lab = 1.f;
        }
    }
    const float den = ((sum + lab) - pk) + smooth, num = pk + smooth;
    const float dk = -1.f / den, dother = num / (den * den);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float bce = c == k ? -1.f / ph[c] : 1.f / (1.f - ph[c]);
        d[c] = mt_inside(p[c]) ? g0 * bce + g1 * (c == k ? dk : dother) : 0.f;
    }
}

__global__ __launch_bounds__(256) void trimap_stats_fwd_kernel(const float* __restrict__ gp, const float* __restrict__ trimap, Tri t,
                                                               float* __restrict__ partial) {
    const size_t e0 = (size_t)blockIdx.x * MT_SPAN, e1 = e0 + MT_SPAN < t.P ? e0 + MT_SPAN : t.P;
    const float* g = gp + (size_t)blockIdx.y * t.sb;
    const float* tm = trimap + (size_t)blockIdx.y * t.P;
    float s[2] = {0.f, 0.f};
    if (t.mode) {
        for (size_t i = e0 + (size_t)threadIdx.x * 4; i < e1; i += 1024) {
            float p[4][3];
            tri_load4(g, t, i, p);
            const f32x4 tv = mt_ld4(tm + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) tri_add(p[j], tv[j], t.smooth, s);
        }
    } else {
        for (size_t i = e0 + threadIdx.x; i < e1; i += 256) {
            const float p[3] = {g[i * t.sp], g[t.sc + i * t.sp], g[2 * t.sc + i * t.sp]};
            tri_add(p, tm[i], t.smooth, s);
        }
    }
    block_sums<2>(s, partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2);
}

__global__ __launch_bounds__(256) void trimap_stats_bwd_kernel(const float* __restrict__ gp, const float* __restrict__ trimap,
                                                               const float* __restrict__ gstats, Tri t, float* __restrict__ dgp) {
    const size_t e0 = (size_t)blockIdx.x * MT_SPAN, e1 = e0 + MT_SPAN < t.P ? e0 + MT_SPAN : t.P;
    const float* g = gp + (size_t)blockIdx.y * t.sb;
    float* dg = dgp + (size_t)blockIdx.y * t.sb;
    const float* tm = trimap + (size_t)blockIdx.y * t.P;
    const float g0 = gstats[blockIdx.y * 2], g1 = gstats[blockIdx.y * 2 + 1];
    if (t.mode) {
        for (size_t i = e0 + (size_t)threadIdx.x * 4; i < e1; i += 1024) {
            float p[4][3], d[4][3];
            tri_load4(g, t, i, p);
            const f32x4 tv = mt_ld4(tm + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) tri_grad(p[j], tv[j], t.smooth, g0, g1, d[j]);
            tri_store4(dg, t, i, d);
        }
    } else {
        for (size_t i = e0 + threadIdx.x; i < e1; i += 256) {
            const float p[3] = {g[i * t.sp], g[t.sc + i * t.sp], g[2 * t.sc + i * t.sp]};
            float d[3];
            tri_grad(p, tm[i], t.smooth, g0, g1, d);
#pragma unroll
            for (int c = 0; c < 3; ++c) dg[c * t.sc + i * t.sp] = d[c];
        }
    }
}

DEVINL int tri_argmax(const float (&p)[3]) {                            // torch.max: the first maximum
    int k = 0;
    float m = p[0];
    if (p[1] > m) {
        k = 1;
        m = p[1];
    }
    if (p[2] > m) k = 2;
    return k;
}

// bwd == 0: out = local [k == 1] + [k == 2]; bwd == 1: out = in [k == 1] (in = dL/dfused)
__global__ __launch_bounds__(256) void matting_fuse_kernel(const float* __restrict__ gp, const float* __restrict__ in, Tri t, int bwd,
                                                           float* __restrict__ out) {
    const size_t e0 = (size_t)blockIdx.x * MT_SPAN, e1 = e0 + MT_SPAN < t.P ? e0 + MT_SPAN : t.P;
    const float* g = gp + (size_t)blockIdx.y * t.sb;
    const float* src = in + (size_t)blockIdx.y * t.P;
    float* dst = out + (size_t)blockIdx.y * t.P;
    const float two = bwd ? 0.f : 1.f;
    if (t.mode) {
        for (size_t i = e0 + (size_t)threadIdx.x * 4; i < e1; i += 1024) {
            float p[4][3];
            tri_load4(g, t, i, p);
            const f32x4 v = mt_ld4(src + i);
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = tri_argmax(p[j]);
                o[j] = k == 1 ? v[j] : (k == 2 ? two : 0.f);
            }
            mt_st4(dst + i, o);
        }
    } else {
        for (size_t i = e0 + threadIdx.x; i < e1; i += 256) {
            const float p[3] = {g[i * t.sp], g[t.sc + i * t.sp], g[2 * t.sc + i * t.sp]};
            const int k = tri_argmax(p);
            dst[i] = k == 1 ? src[i] : (k == 2 ? two : 0.f);
        }
    }
}

// ------------------------------------------------------------------------------------------------ alpha and composition
DEVINL float mt_weight(const float* tm, size_t i) { return tm == nullptr ? 1.f : (tm[i] == 128.f ? 1.f : 0.f); }

DEVINL void alpha_add(float p, float a, float w, float (&s)[2]) {
    const float d = (mt_clamp(p) - a) * w;
    s[0] += sqrtf(d * d + MT_EPS);
    s[1] += w;
}

DEVINL float alpha_grad(float p, float a, float w, float g0) {
    if (!mt_inside(p)) return 0.f;
    const float d = (p - a) * w;
    return g0 * (d * w) / sqrtf(d * d + MT_EPS);
}

__global__ __launch_bounds__(256) void alpha_l1_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ alpha,
                                                           const float* __restrict__ trimap, size_t P, int vec,
                                                           float* __restrict__ partial) {
    const size_t off = (size_t)blockIdx.y * P, e0 = (size_t)blockIdx.x * MT_SPAN, e1 = e0 + MT_SPAN < P ? e0 + MT_SPAN : P;
    const float* pp = pred + off;
    const float* aa = alpha + off;
    const float* tm = trimap ? trimap + off : nullptr;
    float s[2] = {0.f, 0.f};
    if (vec) {
        for (size_t i = e0 + (size_t)threadIdx.x * 4; i < e1; i += 1024) {
            const f32x4 pv = mt_ld4(pp + i), av = mt_ld4(aa + i);
            f32x4 wv = {1.f, 1.f, 1.f, 1.f};
            if (tm) {
                const f32x4 tv = mt_ld4(tm + i);
#pragma unroll
                for (int j = 0; j < 4; ++j) wv[j] = tv[j] == 128.f ? 1.f : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) alpha_add(pv[j], av[j], wv[j], s);
        }
    } else {
        for (size_t i = e0 + threadIdx.x; i < e1; i += 256) alpha_add(pp[i], aa[i], mt_weight(tm, i), s);
    }
    block_sums<2>(s, partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2);
}

__global__ __launch_bounds__(256) void alpha_l1_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ alpha,
                                                           const float* __restrict__ trimap, const float* __restrict__ gsums, size_t P,
                                                           int vec, float* __restrict__ dpred) {
    const size_t off = (size_t)blockIdx.y * P, e0 = (size_t)blockIdx.x * MT_SPAN, e1 = e0 + MT_SPAN < P ? e0 + MT_SPAN : P;
    const float* pp = pred + off;
    const float* aa = alpha + off;
    const float* tm = trimap ? trimap + off : nullptr;
    float* dp = dpred + off;
    const float g0 = gsums[blockIdx.y * 2];
    if (vec) {
        for (size_t i = e0 + (size_t)threadIdx.x * 4; i < e1; i += 1024) {
            const f32x4 pv = mt_ld4(pp + i), av = mt_ld4(aa + i);
            f32x4 wv = {1.f, 1.f, 1.f, 1.f}, o;
            if (tm) {
                const f32x4 tv = mt_ld4(tm + i);
#pragma unroll
                for (int j = 0; j < 4; ++j) wv[j] = tv[j] == 128.f ? 1.f : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = alpha_grad(pv[j], av[j], wv[j], g0);
            mt_st4(dp + i, o);
        }
    } else {
        for (size_t i = e0 + threadIdx.x; i < e1; i += 256) dp[i] = alpha_grad(pp[i], aa[i], mt_weight(tm, i), g0);
    }
}

// fg, bg, image [B][3][P] planes; BWD: the gradient towards pred instead of the sum
template <int BWD>
DEVINL float comp_px(float p, const float (&f)[3], const float (&b)[3], const float (&im)[3], float g0) {
    const float ph = mt_clamp(p);
    float r = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float e = (ph * f[c] + (1.f - ph) * b[c]) - im[c];
        const float q = sqrtf(e * e + MT_EPS);
        r += BWD ? (e / q) * (f[c] - b[c]) : q;
    }
    if (BWD) return mt_inside(p) ? g0 * r : 0.f;
    return r;
}

template <int BWD>
__global__ __launch_bounds__(256) void composition_l1_kernel(const float* __restrict__ pred, const float* __restrict__ fg,
                                                             const float* __restrict__ bg, const float* __restrict__ image,
                                                             const float* __restrict__ gsums, size_t P, int vec,
                                                             float* __restrict__ out) {
    const size_t off = (size_t)blockIdx.y * P, e0 = (size_t)blockIdx.x * MT_SPAN, e1 = e0 + MT_SPAN < P ? e0 + MT_SPAN : P;
    const float* pp = pred + off;
    const float* ff = fg + 3 * off;
    const float* bb = bg + 3 * off;
    const float* ii = image + 3 * off;
    const float g0 = BWD ? gsums[blockIdx.y] : 0.f;
    float s[1] = {0.f};
    if (vec) {
        for (size_t i = e0 + (size_t)threadIdx.x * 4; i < e1; i += 1024) {
            const f32x4 pv = mt_ld4(pp + i);
            f32x4 fv[3], bv[3], iv[3], o;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                fv[c] = mt_ld4(ff + c * P + i);
                bv[c] = mt_ld4(bb + c * P + i);
                iv[c] = mt_ld4(ii + c * P + i);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float f[3] = {fv[0][j], fv[1][j], fv[2][j]}, b[3] = {bv[0][j], bv[1][j], bv[2][j]};
                const float im[3] = {iv[0][j], iv[1][j], iv[2][j]};
                o[j] = comp_px<BWD>(pv[j], f, b, im, g0);
                s[0] += o[j];
            }
            if (BWD) mt_st4(out + off + i, o);
        }
    } else {
        for (size_t i = e0 + threadIdx.x; i < e1; i += 256) {
            const float f[3] = {ff[i], ff[P + i], ff[2 * P + i]}, b[3] = {bb[i], bb[P + i], bb[2 * P + i]};
            const float im[3] = {ii[i], ii[P + i], ii[2 * P + i]};
            const float v = comp_px<BWD>(pp[i], f, b, im, g0);
            s[0] += v;
            if (BWD) out[off + i] = v;
        }
    }
    if (!BWD) block_sums<1>(s, out + (size_t)blockIdx.y * gridDim.x + blockIdx.x);
}

// ------------------------------------------------------------------------------------------------ grouped statistics
// SAM matting (interactive_segmentation/losses_matting.py): M predictions per sample are judged against ONE set of targets.
// Prediction rows are (b, m), contiguous planes [B][M][3][P] / [B][M][P] in T (fp32 or bf16); targets are rows b.  A workgroup owns
// 4096 pixels of a sample: the 11 target values of a pixel are loaded once and serve up to GM_M masks (blockIdx.z takes the next
// GM_M when M is larger).  Column j of a (b, m) row:
//   0 bce sum, 1 IoU-term sum, 2 local alpha sum, 3 sum w, 4 fused alpha sum, 5 composition sum,
//   6 count [clamp(fused) > thr & alpha > thr], 7 count of their union (whole numbers, exact in fp32 below 2^24 pixels)
constexpr int GM_M = 4, GM_K = 8;

struct GmTargets {
    const float *alpha, *trimap, *image, *fg, *bg;      // rows b: [P], [P], [3][P] each
};

template <typename T> DEVINL f32x4 gm_ld4(const T* p);
template <> DEVINL f32x4 gm_ld4<float>(const float* p) { return mt_ld4(p); }
template <> DEVINL f32x4 gm_ld4<bf16_t>(const bf16_t* p) {
    const bf16x4 v = __builtin_nontemporal_load(reinterpret_cast<const bf16x4*>(p));
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (float)v[j];
    return o;
}
template <typename T> DEVINL void gm_st4(T* p, f32x4 v);
template <> DEVINL void gm_st4<float>(float* p, f32x4 v) { mt_st4(p, v); }
template <> DEVINL void gm_st4<bf16_t>(bf16_t* p, f32x4 v) {
    bf16x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (bf16_t)v[j];
    *reinterpret_cast<bf16x4*>(p) = o;
}

// one pixel of one mask: the same expressions, in the same order, as tri_add / alpha_add / comp_px
DEVINL void gm_add(const float (&gp)[3], float lp, float fp, float a, float tv, const float (&f)[3], const float (&b)[3],
                   const float (&im)[3], float thr, float* s) {
    float two[2] = {0.f, 0.f};
    tri_add(gp, tv, 1e-4f, two);
    s[0] += two[0];
    s[1] += two[1];
    const float w = tv == 128.f ? 1.f : 0.f;
    const float dl = (mt_clamp(lp) - a) * w;
    s[2] += sqrtf(dl * dl + MT_EPS);
    s[3] += w;
    const float df = mt_clamp(fp) - a;
    s[4] += sqrtf(df * df + MT_EPS);
    s[5] += comp_px<0>(fp, f, b, im, 0.f);
    const bool pb = mt_clamp(fp) > thr, ab = a > thr;
    s[6] += pb && ab ? 1.f : 0.f;
    s[7] += pb || ab ? 1.f : 0.f;
}

// grid (blocks of a sample, B, groups of GM_M masks): partial[(b * groups + z)][block][GM_M * GM_K]
template <typename T>
__global__ __launch_bounds__(256) void group_stats_fwd_kernel(const T* __restrict__ gpred, const T* __restrict__ lpred,
                                                              const T* __restrict__ fpred, GmTargets t, size_t P, int M, int vec,
                                                              float thr, float* __restrict__ partial) {
    const size_t e0 = (size_t)blockIdx.x * MT_SPAN, e1 = e0 + MT_SPAN < P ? e0 + MT_SPAN : P;
    const int b = blockIdx.y, m0 = blockIdx.z * GM_M;
    const float* aa = t.alpha + (size_t)b * P;
    const float* tm = t.trimap + (size_t)b * P;
    const float* ii = t.image + (size_t)b * 3 * P;
    const float* ff = t.fg + (size_t)b * 3 * P;
    const float* bb = t.bg + (size_t)b * 3 * P;
    float s[GM_M * GM_K];
#pragma unroll
    for (int j = 0; j < GM_M * GM_K; ++j) s[j] = 0.f;
    if (vec) {
        for (size_t i = e0 + (size_t)threadIdx.x * 4; i < e1; i += 1024) {
            const f32x4 av = mt_ld4(aa + i), tv = mt_ld4(tm + i);
            f32x4 fv[3], bv[3], iv[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                fv[c] = mt_ld4(ff + c * P + i);
                bv[c] = mt_ld4(bb + c * P + i);
                iv[c] = mt_ld4(ii + c * P + i);
            }
#pragma unroll
            for (int mm = 0; mm < GM_M; ++mm) {
                if (m0 + mm >= M) break;
                const size_t row = (size_t)b * M + m0 + mm;
                f32x4 gv[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) gv[c] = gm_ld4<T>(gpred + (row * 3 + c) * P + i);
                const f32x4 lv = gm_ld4<T>(lpred + row * P + i), pv = gm_ld4<T>(fpred + row * P + i);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float gp[3] = {gv[0][j], gv[1][j], gv[2][j]};
                    const float f[3] = {fv[0][j], fv[1][j], fv[2][j]}, bg[3] = {bv[0][j], bv[1][j], bv[2][j]};
                    const float im[3] = {iv[0][j], iv[1][j], iv[2][j]};
                    gm_add(gp, lv[j], pv[j], av[j], tv[j], f, bg, im, thr, s + mm * GM_K);
                }
            }
        }
    } else {
        for (size_t i = e0 + threadIdx.x; i < e1; i += 256) {
            const float a = aa[i], tv = tm[i];
            const float f[3] = {ff[i], ff[P + i], ff[2 * P + i]}, bg[3] = {bb[i], bb[P + i], bb[2 * P + i]};
            const float im[3] = {ii[i], ii[P + i], ii[2 * P + i]};
#pragma unroll
            for (int mm = 0; mm < GM_M; ++mm) {
                if (m0 + mm >= M) break;
                const size_t row = (size_t)b * M + m0 + mm;
                const float gp[3] = {to_f32(gpred[row * 3 * P + i]), to_f32(gpred[(row * 3 + 1) * P + i]),
                                     to_f32(gpred[(row * 3 + 2) * P + i])};
                gm_add(gp, to_f32(lpred[row * P + i]), to_f32(fpred[row * P + i]), a, tv, f, bg, im, thr, s + mm * GM_K);
            }
        }
    }
    block_sums<GM_M * GM_K>(s, partial + (((size_t)b * gridDim.z + blockIdx.z) * gridDim.x + blockIdx.x) * (GM_M * GM_K));
}

// one workgroup per (sample, group): stats[b][m][k]
__global__ __launch_bounds__(256) void group_stats_fold_kernel(const float* __restrict__ partial, int nblk, int M, int groups,
                                                               float* __restrict__ stats) {
    const float total = fold_rows<GM_M * GM_K>(partial + (size_t)blockIdx.x * nblk * (GM_M * GM_K), nblk, GM_M * GM_K);
    const int b = blockIdx.x / groups, m = (blockIdx.x % groups) * GM_M + (int)threadIdx.x / GM_K;
    if (threadIdx.x < GM_M * GM_K && m < M) stats[((size_t)b * M + m) * GM_K + threadIdx.x % GM_K] = total;
}

// gstats [B][M][GM_K] = dL/dstats (columns 3, 6 and 7 carry no gradient).  Every element of the three gradients is written once; a
// row whose five live coefficients are all zero gets zeros and its predictions are not read.
template <typename T>
__global__ __launch_bounds__(256) void group_stats_bwd_kernel(const T* __restrict__ gpred, const T* __restrict__ lpred,
                                                              const T* __restrict__ fpred, GmTargets t,
                                                              const float* __restrict__ gstats, size_t P, int M, int vec,
                                                              T* __restrict__ dgpred, T* __restrict__ dlpred, T* __restrict__ dfpred) {
    const size_t e0 = (size_t)blockIdx.x * MT_SPAN, e1 = e0 + MT_SPAN < P ? e0 + MT_SPAN : P;
    const int b = blockIdx.y, m0 = blockIdx.z * GM_M;
    const float* aa = t.alpha + (size_t)b * P;
    const float* tm = t.trimap + (size_t)b * P;
    const float* ii = t.image + (size_t)b * 3 * P;
    const float* ff = t.fg + (size_t)b * 3 * P;
    const float* bb = t.bg + (size_t)b * 3 * P;
    float c[GM_M][5];
    bool live[GM_M], any = false;
#pragma unroll
    for (int mm = 0; mm < GM_M; ++mm) {
        live[mm] = false;
        if (m0 + mm < M) {
            const float* g = gstats + ((size_t)b * M + m0 + mm) * GM_K;
            c[mm][0] = g[0]; c[mm][1] = g[1]; c[mm][2] = g[2]; c[mm][3] = g[4]; c[mm][4] = g[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) live[mm] = live[mm] || c[mm][j] != 0.f;
        }
        any = any || live[mm];
    }
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
        for (size_t i = e0 + (size_t)threadIdx.x * 4; i < e1; i += 1024) {
            f32x4 av = zero4, tv = zero4, fv[3], bv[3], iv[3];
            if (any) {
                av = mt_ld4(aa + i);
                tv = mt_ld4(tm + i);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    fv[ch] = mt_ld4(ff + ch * P + i);
                    bv[ch] = mt_ld4(bb + ch * P + i);
                    iv[ch] = mt_ld4(ii + ch * P + i);
                }
            }
#pragma unroll
            for (int mm = 0; mm < GM_M; ++mm) {
                if (m0 + mm >= M) break;
                const size_t row = (size_t)b * M + m0 + mm;
                f32x4 dg[3] = {zero4, zero4, zero4}, dl = zero4, df = zero4;
                if (live[mm]) {
                    f32x4 gv[3];
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) gv[ch] = gm_ld4<T>(gpred + (row * 3 + ch) * P + i);
                    const f32x4 lv = gm_ld4<T>(lpred + row * P + i), pv = gm_ld4<T>(fpred + row * P + i);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float gp[3] = {gv[0][j], gv[1][j], gv[2][j]};
                        const float f[3] = {fv[0][j], fv[1][j], fv[2][j]}, bg[3] = {bv[0][j], bv[1][j], bv[2][j]};
                        const float im[3] = {iv[0][j], iv[1][j], iv[2][j]};
                        float d[3];
                        tri_grad(gp, tv[j], 1e-4f, c[mm][0], c[mm][1], d);
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) dg[ch][j] = d[ch];
                        dl[j] = alpha_grad(lv[j], av[j], tv[j] == 128.f ? 1.f : 0.f, c[mm][2]);
                        df[j] = alpha_grad(pv[j], av[j], 1.f, c[mm][3]) + comp_px<1>(pv[j], f, bg, im, c[mm][4]);
                    }
                }
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) gm_st4<T>(dgpred + (row * 3 + ch) * P + i, dg[ch]);
                gm_st4<T>(dlpred + row * P + i, dl);
                gm_st4<T>(dfpred + row * P + i, df);
            }
        }
    } else {
        for (size_t i = e0 + threadIdx.x; i < e1; i += 256) {
            float a = 0.f, tv = 0.f, f[3] = {0.f, 0.f, 0.f}, bg[3] = {0.f, 0.f, 0.f}, im[3] = {0.f, 0.f, 0.f};
            if (any) {
                a = aa[i];
                tv = tm[i];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    f[ch] = ff[ch * P + i];
                    bg[ch] = bb[ch * P + i];
                    im[ch] = ii[ch * P + i];
                }
            }
#pragma unroll
            for (int mm = 0; mm < GM_M; ++mm) {
                if (m0 + mm >= M) break;
                const size_t row = (size_t)b * M + m0 + mm;
                float d[3] = {0.f, 0.f, 0.f}, dl = 0.f, df = 0.f;
                if (live[mm]) {
                    const float gp[3] = {to_f32(gpred[row * 3 * P + i]), to_f32(gpred[(row * 3 + 1) * P + i]),
                                         to_f32(gpred[(row * 3 + 2) * P + i])};
                    const float lp = to_f32(lpred[row * P + i]), fp = to_f32(fpred[row * P + i]);
                    tri_grad(gp, tv, 1e-4f, c[mm][0], c[mm][1], d);
                    dl = alpha_grad(lp, a, tv == 128.f ? 1.f : 0.f, c[mm][2]);
                    df = alpha_grad(fp, a, 1.f, c[mm][3]) + comp_px<1>(fp, f, bg, im, c[mm][4]);
                }
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) dgpred[(row * 3 + ch) * P + i] = from_f32<T>(d[ch]);
                dlpred[row * P + i] = from_f32<T>(dl);
                dfpred[row * P + i] = from_f32<T>(df);
            }
        }
    }
}

int mt_check(const char* what, int B, size_t P) {
    SAICV_REQUIRE(B > 0 && B <= 65535 && P > 0, "%s: 1 to 65535 samples of at least one pixel", what);
    SAICV_REQUIRE((P + MT_SPAN - 1) / MT_SPAN <= 0x7fffffffu, "%s: too many pixels per sample", what);
    return 0;
}

int mt_nblk(size_t P) { return (int)((P + MT_SPAN - 1) / MT_SPAN); }

bool mt_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int tri_make(Tri& t, const char* what, const float* gp, long sb, long sc, long sp, int B, size_t P, float smooth) {
    if (mt_check(what, B, P)) return -1;
    SAICV_REQUIRE(gp != nullptr, "%s: null global prediction", what);
    SAICV_REQUIRE(sb >= 0 && sc > 0 && sp > 0, "%s: strides must be positive", what);
    t.P = P; t.sb = sb; t.sc = sc; t.sp = sp; t.smooth = smooth;
    t.mode = 0;
    if (P % 4 == 0 && sb % 4 == 0 && mt_al16(gp)) {
        if (sp == 1 && sc % 4 == 0 && (size_t)sc >= P) t.mode = 1;
        else if (sc == 1 && sp == 3) t.mode = 2;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ Laplacian pyramid level
constexpr int LP_T = 32, LP_IN = LP_T + 4, LP_BC = LP_T + 8;

struct LapTable {
    float k[25];
};

// group: level 0 only -- row r of src reads alpha / trimap of sample r / group (1: a target row per source row)
struct LapGeom {
    int h, w, h2, w2, tiles_x, level0, group;
};

DEVINL int lp_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the level's map at pixel `at` of the flat [B][h][w] array: level 0 forms (clamp(pred) - alpha) * w with the targets at `tat`
DEVINL float lap_src(const float* __restrict__ src, const float* __restrict__ alpha, const float* __restrict__ trimap, size_t at,
                     size_t tat, int level0) {
    const float v = src[at];
    if (!level0) return v;
    const float d = mt_clamp(v) - alpha[tat];
    return trimap ? (trimap[tat] == 128.f ? d : 0.f * d) : d;
}

// G * cur for four neighbouring pixels from the five rows of eight values above and below them; the taps of one output are added
// in row-major order starting from zero (forward and backward share this so that both see the same e)
template <int LD>
DEVINL void lap_conv4(const float (*tile)[LD], int r, int c0, const LapTable& K, float (&acc)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = 0.f;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy) {
        float row[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) row[q] = tile[r + dy][c0 + q];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int dx = 0; dx < 5; ++dx) acc[j] = fmaf(K.k[dy * 5 + dx], row[j + dx], acc[j]);
    }
}

// grid (tiles, B): partial[b][tile][2] = (sum |e|, sum |next|) of the tile
__global__ __launch_bounds__(256) void lap_fwd_kernel(const float* __restrict__ src, const float* __restrict__ alpha,
                                                      const float* __restrict__ trimap, float* __restrict__ next,
                                                      float* __restrict__ partial, LapTable K, LapGeom g) {
    __shared__ float C[LP_IN][LP_IN + 1];
    __shared__ float F[LP_T][LP_T + 1];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int ty0 = (tile / g.tiles_x) * LP_T, tx0 = (tile % g.tiles_x) * LP_T;
    const size_t off = (size_t)b * g.h * g.w, toff = (size_t)(b / g.group) * g.h * g.w;
    for (int i = threadIdx.x; i < LP_IN * LP_IN; i += 256) {
        const int ly = i / LP_IN, lx = i - ly * LP_IN;
        const int y = lp_clampi(ty0 - 2 + ly, g.h - 1), x = lp_clampi(tx0 - 2 + lx, g.w - 1);
        C[ly][lx] = lap_src(src, alpha, trimap, off + (size_t)y * g.w + x, toff + (size_t)y * g.w + x, g.level0);
    }
    __syncthreads();
    const int r = threadIdx.x >> 3, c0 = (threadIdx.x & 7) * 4;
    float acc[4], s[2] = {0.f, 0.f};
    lap_conv4<LP_IN + 1>(C, r, c0, K, acc);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        F[r][c0 + j] = acc[j];
        if (ty0 + r < g.h && tx0 + c0 + j < g.w) s[0] += fabsf(C[r + 2][c0 + j + 2] - acc[j]);
    }
    __syncthreads();
    const int py = threadIdx.x >> 4, px = threadIdx.x & 15;
    const int oy = (ty0 >> 1) + py, ox = (tx0 >> 1) + px;
    if (oy < g.h2 && ox < g.w2) {
        const float v = ((F[2 * py][2 * px] + F[2 * py][2 * px + 1]) + (F[2 * py + 1][2 * px] + F[2 * py + 1][2 * px + 1])) * 0.25f;
        next[((size_t)b * g.h2 + oy) * g.w2 + ox] = v;
        s[1] += fabsf(v);
    }
    block_sums<2>(s, partial + ((size_t)b * gridDim.x + tile) * 2);
}

// g_cur (level 0: dL/dpred) of the tile.  gnext: dL/dnext [B][h2][w2], or with topcur != null gtop[b] * sign(topcur) (the last
// level: the sixth pyramid entry is next itself).  gs[b] = dL/d(sum |e|) of this level.
// gall (or null) [nsum][B]: every dL/dsums of the pyramid.  A row b whose nsum entries are all zero takes no pass: level 0 writes
// zeros without reading src, a coarser level writes nothing (the finer level of that row does not read it).
__global__ __launch_bounds__(256) void lap_bwd_kernel(const float* __restrict__ src, const float* __restrict__ alpha,
                                                      const float* __restrict__ trimap, const float* __restrict__ gnext,
                                                      const float* __restrict__ topcur, const float* __restrict__ gs,
                                                      const float* __restrict__ gtop, const float* __restrict__ gall, int nsum,
                                                      float* __restrict__ gcur, LapTable K, LapGeom g) {
    __shared__ float C[LP_BC][LP_BC + 1];
    __shared__ float GF[LP_IN][LP_IN + 1];
    __shared__ float SS[LP_IN][LP_IN + 1];
    __shared__ float Ks[25];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int ty0 = (tile / g.tiles_x) * LP_T, tx0 = (tile % g.tiles_x) * LP_T;
    const size_t off = (size_t)b * g.h * g.w, toff = (size_t)(b / g.group) * g.h * g.w;
    if (gall != nullptr) {
        bool any = false;
        for (int j = 0; j < nsum; ++j) any = any || gall[(size_t)j * gridDim.y + b] != 0.f;
        if (!any) {                                                     // uniform over the workgroup: no barrier is skipped by a part
            if (g.level0) {
                for (int i = threadIdx.x; i < LP_T * LP_T; i += 256) {
                    const int y = ty0 + i / LP_T, x = tx0 + i % LP_T;
                    if (y < g.h && x < g.w) gcur[off + (size_t)y * g.w + x] = 0.f;
                }
            }
            return;
        }
    }
    const float gsv = gs[b];
    if (threadIdx.x < 25) Ks[threadIdx.x] = K.k[threadIdx.x];
    for (int i = threadIdx.x; i < LP_BC * LP_BC; i += 256) {
        const int ly = i / LP_BC, lx = i - ly * LP_BC;
        const int y = lp_clampi(ty0 - 4 + ly, g.h - 1), x = lp_clampi(tx0 - 4 + lx, g.w - 1);
        C[ly][lx] = lap_src(src, alpha, trimap, off + (size_t)y * g.w + x, toff + (size_t)y * g.w + x, g.level0);
    }
    __syncthreads();
    // gF = P^T g_next - gs sign(e) on the 36 x 36 ring, zero outside the image: 9 rows x 36 columns in groups of four
    for (int i = threadIdx.x; i < LP_IN * (LP_IN / 4); i += 256) {
        const int ly = i / (LP_IN / 4), lx0 = (i - ly * (LP_IN / 4)) * 4;
        const int vy = ty0 - 2 + ly;
        float acc[4];
        lap_conv4<LP_BC + 1>(C, ly, lx0, K, acc);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int vx = tx0 - 2 + lx0 + j;
            float gf = 0.f, ss = 0.f;
            if (vy >= 0 && vy < g.h && vx >= 0 && vx < g.w) {
                ss = gsv * mt_sign(C[ly + 2][lx0 + j + 2] - acc[j]);
                float pt = 0.f;
                if ((vy >> 1) < g.h2 && (vx >> 1) < g.w2) {
                    const size_t at = ((size_t)b * g.h2 + (vy >> 1)) * g.w2 + (vx >> 1);
                    pt = 0.25f * (topcur ? gtop[b] * mt_sign(topcur[at]) : gnext[at]);
                }
                gf = pt - ss;
            }
            GF[ly][lx0 + j] = gf;
            SS[ly][lx0 + j] = ss;
        }
    }
    __syncthreads();
    const int r = threadIdx.x >> 3, c0 = (threadIdx.x & 7) * 4;
    const int y = ty0 + r, x0 = tx0 + c0;
    if (y >= g.h || x0 >= g.w) return;
    float out[4] = {0.f, 0.f, 0.f, 0.f};
    if (y >= 2 && y < g.h - 2 && x0 >= 2 && x0 + 3 < g.w - 2) {
        // interior: nothing was clamped onto these pixels; G^T is the flipped table
#pragma unroll
        for (int ty = 0; ty < 5; ++ty) {
            float row[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) row[q] = GF[r + 4 - ty][c0 + q];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int tx = 0; tx < 5; ++tx) out[j] = fmaf(K.k[ty * 5 + tx], row[j + 4 - tx], out[j]);
        }
    } else {
        for (int j = 0; j < 4; ++j) {
            const int x = x0 + j;
            if (x >= g.w) break;
            const int uylo = y == 0 ? -2 : y, uyhi = y == g.h - 1 ? g.h + 1 : y;
            const int uxlo = x == 0 ? -2 : x, uxhi = x == g.w - 1 ? g.w + 1 : x;
            float a = 0.f;
            for (int uy = uylo; uy <= uyhi; ++uy)
                for (int ux = uxlo; ux <= uxhi; ++ux)
                    for (int ty = 0; ty < 5; ++ty) {
                        const int vy = uy - ty + 2;
                        if (vy < 0 || vy >= g.h) continue;
                        for (int tx = 0; tx < 5; ++tx) {
                            const int vx = ux - tx + 2;
                            if (vx < 0 || vx >= g.w) continue;
                            a = fmaf(Ks[ty * 5 + tx], GF[vy - ty0 + 2][vx - tx0 + 2], a);
                        }
                    }
            out[j] = a;
        }
    }
    for (int j = 0; j < 4; ++j) {
        const int x = x0 + j;
        if (x >= g.w) break;
        const size_t at = off + (size_t)y * g.w + x;
        float v = SS[r + 2][c0 + j + 2] + out[j];
        if (g.level0) {
            const bool on = mt_inside(src[at]) && (trimap == nullptr || trimap[toff + (size_t)y * g.w + x] == 128.f);
            v = on ? v : 0.f;
        }
        gcur[at] = v;
    }
}

int lap_geom(LapGeom& g, const char* what, int B, int h, int w, int level0, int group = 1) {
    SAICV_REQUIRE(B > 0 && B <= 65535 && h > 0 && w > 0, "%s: 1 to 65535 samples of at least one pixel", what);
    SAICV_REQUIRE(group >= 1 && B % group == 0, "%s: %d rows are no whole groups of %d", what, B, group);
    g.h = h; g.w = w; g.h2 = h / 2; g.w2 = w / 2; g.level0 = level0 ? 1 : 0; g.group = group;
    g.tiles_x = (w + LP_T - 1) / LP_T;
    SAICV_REQUIRE((size_t)g.tiles_x * ((h + LP_T - 1) / LP_T) <= 0x7fffffffu, "%s: more than 2^31 - 1 tiles", what);
    return 0;
}

int lap_tiles(const LapGeom& g) { return g.tiles_x * ((g.h + LP_T - 1) / LP_T); }

}  // namespace

namespace saicv {

extern "C" size_t saicv_matting_ws_floats(int B, size_t P) {
    if (B <= 0 || P == 0) return 0;
    return (size_t)B * ((P + MT_SPAN - 1) / MT_SPAN) * 2;
}

extern "C" int saicv_trimap_stats_fwd(const float* gp, long sb, long sc, long sp, const float* trimap, int B, size_t P, float smooth, float* partial,
                                      float* stats, void* stream) {
    hipStream_t st = S(stream);
    Tri t;
    if (tri_make(t, "trimap_stats_fwd", gp, sb, sc, sp, B, P, smooth)) return -1;
    SAICV_REQUIRE(trimap != nullptr && partial != nullptr && stats != nullptr, "trimap_stats_fwd: null trimap, workspace or output");
    if (!mt_al16(trimap)) t.mode = 0;
    const int nblk = mt_nblk(P);
    hipLaunchKernelGGL(trimap_stats_fwd_kernel, dim3(nblk, B), dim3(256), 0, st, gp, trimap, t, partial);
    hipLaunchKernelGGL((mt_fold_kernel<2, 2>), dim3(B), dim3(256), 0, st, partial, nblk, stats, 2L, 1L);
    return check_launch("trimap_stats_fwd");
}

extern "C" int saicv_trimap_stats_bwd(const float* gp, long sb, long sc, long sp, const float* trimap, const float* gstats, int B, size_t P,
                                      float smooth, float* dgp, void* stream) {
    hipStream_t st = S(stream);
    Tri t;
    if (tri_make(t, "trimap_stats_bwd", gp, sb, sc, sp, B, P, smooth)) return -1;
    SAICV_REQUIRE(trimap != nullptr && gstats != nullptr && dgp != nullptr, "trimap_stats_bwd: null trimap or gradient");
    if (!mt_al16(trimap) || !mt_al16(dgp)) t.mode = 0;
    hipLaunchKernelGGL(trimap_stats_bwd_kernel, dim3(mt_nblk(P), B), dim3(256), 0, st, gp, trimap, gstats, t, dgp);
    return check_launch("trimap_stats_bwd");
}

extern "C" int saicv_alpha_l1_fwd(const float* pred, const float* alpha, const float* trimap, int B, size_t P, float* partial, float* sums,
                                  void* stream) {
    hipStream_t st = S(stream);
    if (mt_check("alpha_l1_fwd", B, P)) return -1;
    SAICV_REQUIRE(pred != nullptr && alpha != nullptr && partial != nullptr && sums != nullptr, "alpha_l1_fwd: null argument");
    const int vec = P % 4 == 0 && mt_al16(pred) && mt_al16(alpha) && mt_al16(trimap);
    const int nblk = mt_nblk(P);
    hipLaunchKernelGGL(alpha_l1_fwd_kernel, dim3(nblk, B), dim3(256), 0, st, pred, alpha, trimap, P, vec, partial);
    hipLaunchKernelGGL((mt_fold_kernel<2, 2>), dim3(B), dim3(256), 0, st, partial, nblk, sums, 2L, 1L);
    return check_launch("alpha_l1_fwd");
}

extern "C" int saicv_alpha_l1_bwd(const float* pred, const float* alpha, const float* trimap, const float* gsums, int B, size_t P, float* dpred,
                                  void* stream) {
    hipStream_t st = S(stream);
    if (mt_check("alpha_l1_bwd", B, P)) return -1;
    SAICV_REQUIRE(pred != nullptr && alpha != nullptr && gsums != nullptr && dpred != nullptr, "alpha_l1_bwd: null argument");
    const int vec = P % 4 == 0 && mt_al16(pred) && mt_al16(alpha) && mt_al16(trimap) && mt_al16(dpred);
    hipLaunchKernelGGL(alpha_l1_bwd_kernel, dim3(mt_nblk(P), B), dim3(256), 0, st, pred, alpha, trimap, gsums, P, vec, dpred);
    return check_launch("alpha_l1_bwd");
}

extern "C" int saicv_composition_l1_fwd(const float* pred, const float* fg, const float* bg, const float* image, int B, size_t P, float* partial,
                                        float* sums, void* stream) {
    hipStream_t st = S(stream);
    if (mt_check("composition_l1_fwd", B, P)) return -1;
    SAICV_REQUIRE(pred && fg && bg && image && partial && sums, "composition_l1_fwd: null argument");
    const int vec = P % 4 == 0 && mt_al16(pred) && mt_al16(fg) && mt_al16(bg) && mt_al16(image);
    const int nblk = mt_nblk(P);
    hipLaunchKernelGGL(composition_l1_kernel<0>, dim3(nblk, B), dim3(256), 0, st, pred, fg, bg, image, (const float*)nullptr, P, vec,
                       partial);
    hipLaunchKernelGGL((mt_fold_kernel<1, 1>), dim3(B), dim3(256), 0, st, partial, nblk, sums, 1L, 0L);
    return check_launch("composition_l1_fwd");
}

extern "C" int saicv_composition_l1_bwd(const float* pred, const float* fg, const float* bg, const float* image, const float* gsums, int B, size_t P,
                                        float* dpred, void* stream) {
    hipStream_t st = S(stream);
    if (mt_check("composition_l1_bwd", B, P)) return -1;
    SAICV_REQUIRE(pred && fg && bg && image && gsums && dpred, "composition_l1_bwd: null argument");
    const int vec = P % 4 == 0 && mt_al16(pred) && mt_al16(fg) && mt_al16(bg) && mt_al16(image) && mt_al16(dpred);
    hipLaunchKernelGGL(composition_l1_kernel<1>, dim3(mt_nblk(P), B), dim3(256), 0, st, pred, fg, bg, image, gsums, P, vec, dpred);
    return check_launch("composition_l1_bwd");
}

extern "C" int saicv_matting_fuse_fwd(const float* gp, long sb, long sc, long sp, const float* local, int B, size_t P, float* fused, void* stream) {
    hipStream_t st = S(stream);
    Tri t;
    if (tri_make(t, "matting_fuse_fwd", gp, sb, sc, sp, B, P, 0.f)) return -1;
    SAICV_REQUIRE(local != nullptr && fused != nullptr, "matting_fuse_fwd: null local prediction or output");
    if (!mt_al16(local) || !mt_al16(fused)) t.mode = 0;
    hipLaunchKernelGGL(matting_fuse_kernel, dim3(mt_nblk(P), B), dim3(256), 0, st, gp, local, t, 0, fused);
    return check_launch("matting_fuse_fwd");
}

extern "C" int saicv_matting_fuse_bwd(const float* gp, long sb, long sc, long sp, const float* dfused, int B, size_t P, float* dlocal, void* stream) {
    hipStream_t st = S(stream);
    Tri t;
    if (tri_make(t, "matting_fuse_bwd", gp, sb, sc, sp, B, P, 0.f)) return -1;
    SAICV_REQUIRE(dfused != nullptr && dlocal != nullptr, "matting_fuse_bwd: null gradient");
    if (!mt_al16(dfused) || !mt_al16(dlocal)) t.mode = 0;
    hipLaunchKernelGGL(matting_fuse_kernel, dim3(mt_nblk(P), B), dim3(256), 0, st, gp, dfused, t, 1, dlocal);
    return check_launch("matting_fuse_bwd");
}

extern "C" size_t saicv_group_matting_ws_floats(int B, int M, size_t P) {
    if (B <= 0 || M <= 0 || P == 0) return 0;
    return (size_t)B * ((M + GM_M - 1) / GM_M) * ((P + MT_SPAN - 1) / MT_SPAN) * (GM_M * GM_K);
}

namespace {
int gm_check(const char* what, int dtype, const void* gp, const void* lp, const void* fp, const float* alpha, const float* trimap,
             const float* image, const float* fg, const float* bg, int B, int M, size_t P) {
    if (mt_check(what, B, P)) return -1;
    SAICV_REQUIRE(dtype == SAICV_DTYPE_BF16 || dtype == SAICV_DTYPE_F32, "%s: predictions are bf16 or fp32", what);
    SAICV_REQUIRE(M > 0 && (M + GM_M - 1) / GM_M <= 65535, "%s: 1 to %d masks per sample", what, 65535 * GM_M);
    SAICV_REQUIRE(gp && lp && fp && alpha && trimap && image && fg && bg, "%s: null argument", what);
    return 0;
}
}  // namespace

extern "C" int saicv_group_matting_stats_fwd(int dtype, const void* gp, const void* lp, const void* fp, const float* alpha, const float* trimap,
                                             const float* image, const float* fg, const float* bg, int B, int M, size_t P, float thr, float* partial,
                                             float* stats, void* stream) {
    hipStream_t st = S(stream);
    if (gm_check("group_matting_stats_fwd", dtype, gp, lp, fp, alpha, trimap, image, fg, bg, B, M, P)) return -1;
    SAICV_REQUIRE(partial != nullptr && stats != nullptr, "group_matting_stats_fwd: null workspace or output");
    const GmTargets t = {alpha, trimap, image, fg, bg};
    const int vec = P % 4 == 0 && mt_al16(gp) && mt_al16(lp) && mt_al16(fp) && mt_al16(alpha) && mt_al16(trimap) && mt_al16(image) &&
                    mt_al16(fg) && mt_al16(bg);
    const int nblk = mt_nblk(P), groups = (M + GM_M - 1) / GM_M;
    const dim3 grid(nblk, B, groups);
    if (dtype == SAICV_DTYPE_BF16)
        hipLaunchKernelGGL(group_stats_fwd_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)gp, (const bf16_t*)lp,
                           (const bf16_t*)fp, t, P, M, vec, thr, partial);
    else
        hipLaunchKernelGGL(group_stats_fwd_kernel<float>, grid, dim3(256), 0, st, (const float*)gp, (const float*)lp,
                           (const float*)fp, t, P, M, vec, thr, partial);
    hipLaunchKernelGGL(group_stats_fold_kernel, dim3(B * groups), dim3(256), 0, st, partial, nblk, M, groups, stats);
    return check_launch("group_matting_stats_fwd");
}

extern "C" int saicv_group_matting_stats_bwd(int dtype, const void* gp, const void* lp, const void* fp, const float* alpha, const float* trimap,
                                             const float* image, const float* fg, const float* bg, const float* gstats, int B, int M, size_t P,
                                             void* dgp, void* dlp, void* dfp, void* stream) {
    hipStream_t st = S(stream);
    if (gm_check("group_matting_stats_bwd", dtype, gp, lp, fp, alpha, trimap, image, fg, bg, B, M, P)) return -1;
    SAICV_REQUIRE(gstats && dgp && dlp && dfp, "group_matting_stats_bwd: null gradient");
    const GmTargets t = {alpha, trimap, image, fg, bg};
    const int vec = P % 4 == 0 && mt_al16(gp) && mt_al16(lp) && mt_al16(fp) && mt_al16(alpha) && mt_al16(trimap) && mt_al16(image) &&
                    mt_al16(fg) && mt_al16(bg) && mt_al16(dgp) && mt_al16(dlp) && mt_al16(dfp);
    const dim3 grid(mt_nblk(P), B, (M + GM_M - 1) / GM_M);
    if (dtype == SAICV_DTYPE_BF16)
        hipLaunchKernelGGL(group_stats_bwd_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)gp, (const bf16_t*)lp,
                           (const bf16_t*)fp, t, gstats, P, M, vec, (bf16_t*)dgp, (bf16_t*)dlp, (bf16_t*)dfp);
    else
        hipLaunchKernelGGL(group_stats_bwd_kernel<float>, grid, dim3(256), 0, st, (const float*)gp, (const float*)lp,
                           (const float*)fp, t, gstats, P, M, vec, (float*)dgp, (float*)dlp, (float*)dfp);
    return check_launch("group_matting_stats_bwd");
}

extern "C" size_t saicv_lap_level_ws_floats(int B, int h, int w) {
    if (B <= 0 || h <= 0 || w <= 0) return 0;
    return (size_t)B * ((h + LP_T - 1) / LP_T) * ((w + LP_T - 1) / LP_T) * 2;
}

extern "C" int saicv_lap_level_fwd(const float* src, const float* alpha, const float* trimap, int level0, int B, int h, int w,
                                   const float* table, float* next, float* partial, float* sum_e, float* sum_next, void* stream) {
    SAICV_REQUIRE(table != nullptr, "lap_level_fwd: null weight table");
    hipStream_t st = S(stream);
    LapGeom g;
    if (lap_geom(g, "lap_level_fwd", B, h, w, level0)) return -1;
    SAICV_REQUIRE(src != nullptr && table != nullptr && partial != nullptr && sum_e != nullptr, "lap_level_fwd: null argument");
    SAICV_REQUIRE(!level0 || alpha != nullptr, "lap_level_fwd: level 0 needs alpha");
    SAICV_REQUIRE(next != nullptr || g.h2 == 0 || g.w2 == 0, "lap_level_fwd: null output map");
    LapTable K;
    for (int i = 0; i < 25; ++i) K.k[i] = table[i];
    const int tiles = lap_tiles(g);
    hipLaunchKernelGGL(lap_fwd_kernel, dim3(tiles, B), dim3(256), 0, st, src, level0 ? alpha : nullptr, level0 ? trimap : nullptr, next,
                       partial, K, g);
    hipLaunchKernelGGL((mt_fold_kernel<2, 1>), dim3(B), dim3(256), 0, st, partial, tiles, sum_e, 1L, 0L);
    if (sum_next != nullptr)
        hipLaunchKernelGGL((mt_fold_kernel<2, 1>), dim3(B), dim3(256), 0, st, partial + 1, tiles, sum_next, 1L, 0L);
    return check_launch("lap_level_fwd");
}

extern "C" int saicv_lap_level_bwd(const float* src, const float* alpha, const float* trimap, int level0, int B, int h, int w,
                                   const float* table, const float* gnext, const float* topcur, const float* gs, const float* gtop,
                                   float* gcur, void* stream) {
    SAICV_REQUIRE(table != nullptr, "lap_level_bwd: null weight table");
    hipStream_t st = S(stream);
    LapGeom g;
    if (lap_geom(g, "lap_level_bwd", B, h, w, level0)) return -1;
    SAICV_REQUIRE(src != nullptr && table != nullptr && gs != nullptr && gcur != nullptr, "lap_level_bwd: null argument");
    SAICV_REQUIRE(!level0 || alpha != nullptr, "lap_level_bwd: level 0 needs alpha");
    SAICV_REQUIRE(g.h2 == 0 || g.w2 == 0 || gnext != nullptr || (topcur != nullptr && gtop != nullptr),
                  "lap_level_bwd: neither the next level's gradient nor the top map");
    LapTable K;
    for (int i = 0; i < 25; ++i) K.k[i] = table[i];
    hipLaunchKernelGGL(lap_bwd_kernel, dim3(lap_tiles(g), B), dim3(256), 0, st, src, level0 ? alpha : nullptr,
                       level0 ? trimap : nullptr, gnext, topcur, gs, gtop, (const float*)nullptr, 0, gcur, K, g);
    return check_launch("lap_level_bwd");
}

extern "C" int saicv_lap_level0_group_fwd(const float* src, const float* alpha, const float* trimap, int group, int R, int h, int w,
                                          const float* table, float* next, float* partial, float* sum_e, void* stream) {
    SAICV_REQUIRE(table != nullptr, "lap_level0_group_fwd: null weight table");
    hipStream_t st = S(stream);
    LapGeom g;
    if (lap_geom(g, "lap_level0_group_fwd", R, h, w, 1, group)) return -1;
    SAICV_REQUIRE(src && alpha && table && partial && sum_e, "lap_level0_group_fwd: null argument");
    SAICV_REQUIRE(next != nullptr || g.h2 == 0 || g.w2 == 0, "lap_level0_group_fwd: null output map");
    LapTable K;
    for (int i = 0; i < 25; ++i) K.k[i] = table[i];
    const int tiles = lap_tiles(g);
    hipLaunchKernelGGL(lap_fwd_kernel, dim3(tiles, R), dim3(256), 0, st, src, alpha, trimap, next, partial, K, g);
    hipLaunchKernelGGL((mt_fold_kernel<2, 1>), dim3(R), dim3(256), 0, st, partial, tiles, sum_e, 1L, 0L);
    return check_launch("lap_level0_group_fwd");
}

extern "C" int saicv_lap_level_group_bwd(const float* src, const float* alpha, const float* trimap, int level0, int group, int R, int h,
                                         int w, const float* table, const float* gnext, const float* topcur, const float* gs,
                                         const float* gtop, const float* gall, int nsum, float* gcur, void* stream) {
    SAICV_REQUIRE(table != nullptr, "lap_level_group_bwd: null weight table");
    hipStream_t st = S(stream);
    LapGeom g;
    if (lap_geom(g, "lap_level_group_bwd", R, h, w, level0, level0 ? group : 1)) return -1;
    SAICV_REQUIRE(src && table && gs && gall && gcur && nsum > 0, "lap_level_group_bwd: null argument");
    SAICV_REQUIRE(!level0 || alpha != nullptr, "lap_level_group_bwd: level 0 needs alpha");
    SAICV_REQUIRE(g.h2 == 0 || g.w2 == 0 || gnext != nullptr || (topcur != nullptr && gtop != nullptr),
                  "lap_level_group_bwd: neither the next level's gradient nor the top map");
    LapTable K;
    for (int i = 0; i < 25; ++i) K.k[i] = table[i];
    hipLaunchKernelGGL(lap_bwd_kernel, dim3(lap_tiles(g), R), dim3(256), 0, st, src, level0 ? alpha : nullptr,
                       level0 ? trimap : nullptr, gnext, topcur, gs, gtop, gall, nsum, gcur, K, g);
    return check_launch("lap_level_group_bwd");
}

}  // namespace saicv
