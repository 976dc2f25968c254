// extern "C" surface of libsaicv_hip.so (declared in include/saicv_hip.h).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "common.h"
#include "saicv_internal.h"
#include "../../include/saicv_hip.h"

namespace saicv {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return -2;
    }
    return 0;
}

// declared in the other translation units
int pack_weight_batched(int, const saicv_pack_desc*, int, int, hipStream_t);
int pack_input_s2d(int, const float*, long, long, long, long, void*, int, int, int, int, int, int, hipStream_t);
int pack_weight_s2d(int, const float*, long, long, long, long, int, int, int, int, int, void*, hipStream_t);
int unpack_wgrad_s2d(const float*, int, int, int, int, int, float*, long, long, long, long, int, hipStream_t);
size_t bn_ws_floats(int C);
int bn_finalize_fwd(const float*, const float*, int, int, double, const float*, const float*, float*,
                    float*, double, double, float*, float*, float*, float*, float*, long long*, hipStream_t);
int bn_eval_coeffs(int, const float*, const float*, const float*, const float*, double, float*, float*,
                   hipStream_t);
int bn_act_fwd(int, const void*, const void*, void*, const float*, const float*, size_t, int, int, void*,
               hipStream_t);
size_t bn_bwd_ws_floats(size_t, int, int);
int bn_bwd(int, const void*, const void*, const void*, const void*, const float*, const float*, const float*, void*,
           void*, float*, float*, size_t, int, int, int, float*, hipStream_t);
int bn_act_fwd_stats(int, const void*, const void*, void*, const float*, const float*, int, double, const float*, const float*,
                     float*, float*, double, double, long long*, float*, float*, size_t, int, int, void*, hipStream_t);
int bn_act_fwd_join(int, const void*, const void*, const float*, const float*, void*, const float*, const float*, const float*,
                    const float*, int, double, const float*, const float*, float*, float*, double, double, long long*, float*,
                    float*, size_t, int, int, void*, hipStream_t);
int bn_bwd_inline(int, const void*, const void*, const void*, const float*, const float*, const float*, const float*,
                  const float*, int, void*, void*, float*, float*, size_t, int, int, int, hipStream_t);
int bn_bwd_from_partials(int, const void*, const void*, const void*, const float*, const float*, const float*, const float*,
                         const float*, int, void*, void*, float*, float*, size_t, int, int, int, float*, hipStream_t);
int maxpool_fwd(int, const void*, void*, uint8_t*, int, int, int, int, int, int, int, int, int, hipStream_t);
int maxpool_bwd(int, const void*, const uint8_t*, void*, int, int, int, int, int, int, int, int, int, hipStream_t);
int bn_relu_maxpool_fwd(int, const void*, const float*, const float*, void*, uint8_t*, int, int, int, int, int, int, int, int, int, hipStream_t);
int bn_relu_maxpool_bwd(int, const void*, const uint8_t*, const void*, const float*, const float*, const float*, const float*, const float*,
                        void*, float*, float*, int, float*, int, int, int, int, int, int, int, int, int, hipStream_t);
int avgpool_fwd(int, const void*, void*, int, int, int, hipStream_t);
int avgpool_bwd(int, const void*, void*, int, int, int, hipStream_t);
int softmax_ce_fwd(const float*, const void*, int, int, int, float*, float*, float*, hipStream_t);
int scale_by_scalar(int, const float*, const float*, void*, size_t, hipStream_t);
int pack_input(int, const float*, long, long, long, long, void*, int, int, int, int, int, hipStream_t);
int pack_weight(int, const float*, long, long, long, long, int, int, int, int, int, int, void*, void*, hipStream_t);
int unpack_wgrad(const float*, int, int, int, int, int, float*, long, long, long, long, int, hipStream_t);
int colsum(int, const void*, int, int, float*, hipStream_t);
int row_scale(int, const void*, const float*, void*, size_t, int, int, hipStream_t);
int sgd_flat(float*, const float*, float*, const int32_t*, const float*, const float*, const float*, const uint8_t*, size_t, hipStream_t);
int adamw_flat(float*, const float*, float*, float*, const int32_t*, const float*, const float*, const float*, const uint8_t*, float*, size_t, hipStream_t);
int muon_prepare(float*, const float*, float*, float*, const int32_t*, const int32_t*, const float*, const float*, const float*, const uint8_t*, float*, void*, size_t, hipStream_t);
int muon_newton_schulz(void*, void*, void*, void*, float*, float*, const int32_t*, int, int, int, int, double, double, double, int, float*, hipStream_t);
int muon_apply(float*, const void*, const int32_t*, const int32_t*, const float*, const float*, const uint8_t*, size_t, hipStream_t);
int grad_stats(const float*, size_t, float*, float*, hipStream_t);
int grad_clip_scale(float*, size_t, const float*, const float*, double, hipStream_t);
int grad_clip_value(float*, size_t, const float*, double, hipStream_t);
int scaler_update(float*, const float*, double, double, int, hipStream_t);
int layernorm_fwd(int, const void*, const float*, const float*, void*, float*, float*, int, int, double, hipStream_t);
size_t layernorm_bwd_ws_floats(int, int);
int dropout_add_layernorm_fwd(int, const void*, const void*, double, unsigned, const unsigned*, const float*, const float*, void*, void*,
                              float*, float*, int, int, double, hipStream_t);
int dropout_add_layernorm_bwd(int, const void*, const void*, const float*, const float*, const float*, double, unsigned, const unsigned*,
                              void*, void*, float*, float*, float*, int, int, int, hipStream_t);
int layernorm_bwd(int, const void*, const void*, const float*, const float*, const float*, const void*, void*,
                  float*, float*, float*, int, int, int, hipStream_t, const float* = nullptr, int = 1, void* = nullptr);
int gelu_fwd(int, const void*, void*, size_t, hipStream_t);
int gelu_bwd(int, const void*, const void*, void*, size_t, hipStream_t);
int relu_dropout_fwd(int, const void*, void*, size_t, double, unsigned, const unsigned*, hipStream_t);
int relu_dropout_bwd(int, const void*, const void*, void*, size_t, double, hipStream_t);
int attention_fwd(int, const void*, void*, float*, int, int, int, int, double, hipStream_t);
int attention_bwd(int, const void*, const void*, const void*, const float*, void*, int, int, int, int, double,
                  hipStream_t);

}  // namespace saicv

using namespace saicv;

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

static int check_desc(const saicv_conv_desc* d, const char* who) {
    SAICV_REQUIRE(d != nullptr, "%s: null descriptor", who);
    SAICV_REQUIRE(d->dtype == SAICV_BF16 || d->dtype == SAICV_F32, "%s: bad dtype %d", who, d->dtype);
    SAICV_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->K > 0 && d->R > 0 && d->S > 0,
                  "%s: non-positive dimension", who);
    SAICV_REQUIRE(d->stride >= 1 && d->pad >= 0, "%s: bad stride/pad", who);
    const int oh = (d->H + 2 * d->pad - d->R) / d->stride + 1;
    const int ow = (d->W + 2 * d->pad - d->S) / d->stride + 1;
    SAICV_REQUIRE(oh == d->OH && ow == d->OW, "%s: OH/OW (%d,%d) inconsistent with geometry (%d,%d)",
                  who, d->OH, d->OW, oh, ow);
    SAICV_REQUIRE((long long)d->N * d->H * d->W * (long long)d->C < (1ll << 31) &&
                      (long long)d->N * d->OH * d->OW * (long long)d->K < (1ll << 31),
                  "%s: tensor exceeds 2^31 elements", who);
    return 0;
}

extern "C" {

int saicv_version(void) { return 100; }
const char* saicv_last_error_string(void) { return g_err; }

int saicv_pack_input(int dtype, const float* src, long sN, long sC, long sH, long sW, void* dst,
                     int N, int C, int H, int W, int Cp, void* stream) {
    return pack_input(dtype, src, sN, sC, sH, sW, dst, N, C, H, W, Cp, S(stream));
}
int saicv_pack_weight(int dtype, const float* w, long sO, long sI, long sR, long sS, int O, int I,
                      int R, int Sx, int Ip, int Op, void* wf, void* wd, void* stream) {
    return pack_weight(dtype, w, sO, sI, sR, sS, O, I, R, Sx, Ip, Op, wf, wd, S(stream));
}
int saicv_unpack_wgrad(const float* dw, int O, int I, int R, int Sx, int Ip, float* grad, long sO,
                       long sI, long sR, long sS, int accumulate, void* stream) {
    return unpack_wgrad(dw, O, I, R, Sx, Ip, grad, sO, sI, sR, sS, accumulate, S(stream));
}

int saicv_pack_weight_batched(int dtype, const saicv_pack_desc* descs, int n, int total_tiles, void* stream) {
    return pack_weight_batched(dtype, descs, n, total_tiles, S(stream));
}
int saicv_pack_input_s2d(int dtype, const float* src, long sN, long sC, long sH, long sW, void* dst, int N, int C, int H,
                         int W, int pad, int Cq, void* stream) {
    return pack_input_s2d(dtype, src, sN, sC, sH, sW, dst, N, C, H, W, pad, Cq, S(stream));
}
int saicv_pack_weight_s2d(int dtype, const float* w, long sO, long sI, long sR, long sS, int O, int I, int R, int Sx,
                          int Cq, void* wf, void* stream) {
    return pack_weight_s2d(dtype, w, sO, sI, sR, sS, O, I, R, Sx, Cq, wf, S(stream));
}
int saicv_unpack_wgrad_s2d(const float* dw, int O, int I, int R, int Sx, int Cq, float* grad, long sO, long sI, long sR,
                           long sS, int accumulate, void* stream) {
    return unpack_wgrad_s2d(dw, O, I, R, Sx, Cq, grad, sO, sI, sR, sS, accumulate, S(stream));
}

int saicv_conv2d_stat_rows(const saicv_conv_desc* d) {
    if (!d) return -1;
    return conv_stat_rows(d);
}

int saicv_conv2d_fwd(const saicv_conv_desc* d, const void* x, const void* wf, const float* bias,
                     void* y, int out_f32, float* stat_sum, float* stat_sq, void* stream) {
    if (check_desc(d, "saicv_conv2d_fwd")) return -1;
    // saicv_conv2d_stat_rows describes the statistics launch with an output in the data type only
    SAICV_REQUIRE(!(stat_sum && out_f32), "saicv_conv2d_fwd: BN statistics need out_f32 = 0");
    const int M = d->N * d->OH * d->OW;
    return igemm_nt(d->dtype, 0, x, wf, y, bias, stat_sum, stat_sq, d->H, d->W, d->C, d->OH, d->OW,
                    d->R, d->S, d->stride, d->pad, M, d->K, d->R * d->S * d->C, d->K, out_f32, S(stream));
}

int saicv_conv2d_dgrad(const saicv_conv_desc* d, const void* dy, const void* wd, void* dx,
                       void* stream) {
    if (check_desc(d, "saicv_conv2d_dgrad")) return -1;
    // rows = input pixels; gather source = dy [N,OH,OW,K]; k = (r,s,kout)
    const int M = d->N * d->H * d->W;
    return igemm_nt(d->dtype, 1, dy, wd, dx, nullptr, nullptr, nullptr, d->OH, d->OW, d->K, d->H, d->W,
                    d->R, d->S, d->stride, d->pad, M, d->C, d->R * d->S * d->K, d->C, 0, S(stream));
}

int saicv_conv2d_wgrad(const saicv_conv_desc* d, const void* dy, const void* x, float* dw,
                       void* stream) {
    if (check_desc(d, "saicv_conv2d_wgrad")) return -1;
    const int M = d->N * d->OH * d->OW;
    return igemm_tn(d->dtype, dy, x, dw, d->H, d->W, d->C, d->OH, d->OW, d->R, d->S, d->stride, d->pad,
                    M, d->K, d->R * d->S * d->C, S(stream));
}

int saicv_conv2d_wgrad_bias(const saicv_conv_desc* d, const void* dy, const void* x, float* dw, float* dbias,
                            void* stream) {
    if (check_desc(d, "saicv_conv2d_wgrad_bias")) return -1;
    const int M = d->N * d->OH * d->OW;
    return igemm_tn(d->dtype, dy, x, dw, d->H, d->W, d->C, d->OH, d->OW, d->R, d->S, d->stride, d->pad,
                    M, d->K, d->R * d->S * d->C, S(stream), dbias);
}

int saicv_linear_fwd(int dtype, const void* x, const void* wf, const float* bias, void* y, int M, int K, int N,
                     int out_f32, const void* addend, const float* row_scale, int rows_per_scale, void* stream) {
    EpiExtra ex;
    ex.addend = addend; ex.row_scale = row_scale; ex.rows_per_scale = rows_per_scale > 0 ? rows_per_scale : 1;
    return igemm_nt(dtype, 0, x, wf, y, bias, nullptr, nullptr, 1, 1, K, 1, 1, 1, 1, 1, 0, M, N, K, N, out_f32,
                    S(stream), (addend || row_scale) ? &ex : nullptr);
}
int saicv_linear_dgrad(int dtype, const void* dy, const void* wd, void* dx, int M, int K, int N, const void* addend,
                       void* stream) {
    EpiExtra ex;
    ex.addend = addend;
    return igemm_nt(dtype, 1, dy, wd, dx, nullptr, nullptr, nullptr, 1, 1, N, 1, 1, 1, 1, 1, 0, M, K, N, K, 0,
                    S(stream), addend ? &ex : nullptr);
}
int saicv_linear_gelu_fwd(int dtype, const void* x, const void* wf, const float* bias, void* y_pre, void* y_act, int M,
                          int K, int N, void* stream) {
    EpiExtra ex;
    ex.act_mode = 1; ex.out2 = y_act;
    return igemm_nt(dtype, 0, x, wf, y_pre, bias, nullptr, nullptr, 1, 1, K, 1, 1, 1, 1, 1, 0, M, N, K, N, 0, S(stream), &ex);
}
int saicv_linear_dgrad_gelu(int dtype, const void* dy, const void* wd, const void* pre, void* dx, int M, int K, int N,
                            void* stream) {
    EpiExtra ex;
    ex.act_mode = 2; ex.addend = pre;
    return igemm_nt(dtype, 1, dy, wd, dx, nullptr, nullptr, nullptr, 1, 1, N, 1, 1, 1, 1, 1, 0, M, K, N, K, 0, S(stream), &ex);
}
int saicv_linear_gelu_fwd_aux(int dtype, const void* x, const void* wf, const float* bias, void* y_dact, void* y_act, int M,
                              int K, int N, void* stream) {
    EpiExtra ex;
    ex.act_mode = 3; ex.out2 = y_act;
    return igemm_nt(dtype, 0, x, wf, y_dact, bias, nullptr, nullptr, 1, 1, K, 1, 1, 1, 1, 1, 0, M, N, K, N, 0, S(stream), &ex);
}
int saicv_linear_dgrad_mul(int dtype, const void* dy, const void* wd, const void* factor, void* dx, int M, int K, int N,
                           void* stream) {
    EpiExtra ex;
    ex.act_mode = 4; ex.addend = factor;
    return igemm_nt(dtype, 1, dy, wd, dx, nullptr, nullptr, nullptr, 1, 1, N, 1, 1, 1, 1, 1, 0, M, K, N, K, 0, S(stream), &ex);
}
int saicv_linear_wgrad(int dtype, const void* dy, const void* x, float* dw, float* dbias, int M, int K, int N,
                       void* stream) {
    return igemm_tn(dtype, dy, x, dw, 1, 1, K, 1, 1, 1, 1, 1, 0, M, N, K, S(stream), dbias);
}
int saicv_conv2d_dgrad_add(const saicv_conv_desc* d, const void* dy, const void* wd, const void* addend, void* dx,
                           void* stream) {
    if (check_desc(d, "saicv_conv2d_dgrad_add")) return -1;
    const int M = d->N * d->H * d->W;
    EpiExtra ex;
    ex.addend = addend;
    return igemm_nt(d->dtype, 1, dy, wd, dx, nullptr, nullptr, nullptr, d->OH, d->OW, d->K, d->H, d->W,
                    d->R, d->S, d->stride, d->pad, M, d->C, d->R * d->S * d->K, d->C, 0, S(stream),
                    addend ? &ex : nullptr);
}
int saicv_conv2d_dgrad_stat_rows(const saicv_conv_desc* d) {
    if (!d) return -1;
    return conv_bwd_stat_rows(d);
}
int saicv_conv2d_dgrad_fused(const saicv_conv_desc* d, const void* dy, const void* wd, const saicv_dgrad_fuse* f, void* dx,
                             void* stream) {
    if (check_desc(d, "saicv_conv2d_dgrad_fused")) return -1;
    if (!f) { set_error("saicv_conv2d_dgrad_fused: null fusion descriptor"); return -1; }
    const int M = d->N * d->H * d->W;
    EpiExtra ex;
    ex.addend = f->addend;
    ex.addend_gate = static_cast<const uint8_t*>(f->addend_gate);
    ex.bs_y = f->bn_y;
    ex.bs_mask = static_cast<const uint8_t*>(f->bn_mask);
    ex.bs_mean = f->bn_mean;
    ex.bs_invstd = f->bn_invstd;
    ex.bs_g = f->part_g;
    ex.bs_gx = f->part_gx;
    ex.stat_atomic_rows = f->part_rows;        // > 0: the caller zeroed part_rows rows and wants the sums added into them
    if (f->bn_y && d->stride > 1 && f->part_rows == 0) {
        // parity classes smaller than the largest one leave their last partial rows unwritten
        const size_t bytes = (size_t)saicv_conv2d_dgrad_stat_rows(d) * d->C * sizeof(float);
        if (f->part_g) hipMemsetAsync(f->part_g, 0, bytes, S(stream));
        if (f->part_gx) hipMemsetAsync(f->part_gx, 0, bytes, S(stream));
    }
    return igemm_nt(d->dtype, 1, dy, wd, dx, nullptr, nullptr, nullptr, d->OH, d->OW, d->K, d->H, d->W,
                    d->R, d->S, d->stride, d->pad, M, d->C, d->R * d->S * d->K, d->C, 0, S(stream),
                    (f->addend || f->bn_y) ? &ex : nullptr);
}
// BatchNorm-backward apply + data gradient + weight gradient of a bottleneck's third 1 x 1 convolution as one stream (c3bwd.hip)
int saicv_c3_bwd_stream_ok(int dtype, int M, int CO, int CI) { return c3_bwd_stream_blocks(dtype, M, CO, CI); }
int saicv_c3_bwd_stream_rows(int M, int CO, int CI) { return c3_bwd_stream_rows(M, CO, CI); }
size_t saicv_c3_bwd_stream_ws_floats(int M, int CO, int CI) { return c3_bwd_stream_ws_floats(M, CO, CI); }
int saicv_c3_bwd_stream(int dtype, const void* dz, const void* relu_mask, const void* y, const float* gamma, const float* mean,
                        const float* invstd, const float* part_g, const float* part_gx, int rows, float* dgamma, float* dbeta,
                        int accumulate, float* ws, const void* x, const void* wd, const saicv_dgrad_fuse* f, void* dx, float* dw,
                        int M, int CO, int CI, void* stream) {
    SAICV_REQUIRE(dtype == SAICV_BF16, "saicv_c3_bwd_stream: bf16 only (dtype %d)", dtype);
    SAICV_REQUIRE(c3_bwd_stream_rows(M, CO, CI) > 0, "saicv_c3_bwd_stream: no form for M = %d, Cout = %d, Cin = %d", M, CO, CI);
    SAICV_REQUIRE(mean && invstd && ws, "saicv_c3_bwd_stream: statistics / workspace missing");
    SAICV_REQUIRE(!f || (!f->addend && !f->addend_gate), "saicv_c3_bwd_stream: no addend form");
    if (bn_bwd_coeffs(part_g, part_gx, rows, CO, (size_t)M, gamma, mean, invstd, dgamma, dbeta, accumulate, ws, S(stream)) != 0) return -1;
    EpiExtra ex;
    if (f && f->bn_y) {
        ex.bs_y = f->bn_y;
        ex.bs_mask = static_cast<const uint8_t*>(f->bn_mask);
        ex.bs_mean = f->bn_mean;
        ex.bs_invstd = f->bn_invstd;
        ex.bs_g = f->part_g;
        ex.bs_gx = f->part_gx;
    }
    return c3_bwd_stream(M, CO, CI, dz, y, relu_mask, ws + (size_t)64 * CO, x, wd, dx, dw, (f && f->bn_y) ? &ex : nullptr,
                         f ? f->part_rows : 0, ws + (size_t)67 * CO, S(stream));
}
int saicv_igemm_plan(const saicv_plan_query* q, saicv_plan* plan) {
    if (!q || !plan) { set_error("saicv_igemm_plan: null argument"); return -1; }
    SAICV_REQUIRE(q->op >= SAICV_PLAN_CONV_FWD && q->op <= SAICV_PLAN_LINEAR_WGRAD, "saicv_igemm_plan: bad op %d", q->op);
    if (q->op <= SAICV_PLAN_CONV_WGRAD) {
        if (check_desc(&q->conv, "saicv_igemm_plan")) return -1;
    } else {
        SAICV_REQUIRE(q->dtype == SAICV_BF16 || q->dtype == SAICV_F32, "saicv_igemm_plan: bad dtype %d", q->dtype);
    }
    return igemm_plan(q, plan);
}
int saicv_row_scale(int dtype, const void* x, const float* scale, void* out, size_t rows, int row_len,
                    int rows_per_scale, void* stream) {
    return row_scale(dtype, x, scale, out, rows, row_len, rows_per_scale, S(stream));
}

int saicv_colsum(int dtype, const void* dy, int M, int N, float* dbias, void* stream) {
    return colsum(dtype, dy, M, N, dbias, S(stream));
}

size_t saicv_bn_ws_floats(int C) { return bn_ws_floats(C); }

int saicv_bn_finalize_fwd(const float* sum, const float* sq, int rows, int C, double count,
                          const float* gamma, const float* beta, float* running_mean,
                          float* running_var, double momentum, double eps, float* mean,
                          float* invstd, float* scale, float* shift, float* ws, long long* num_batches_tracked,
                          void* stream) {
    return bn_finalize_fwd(sum, sq, rows, C, count, gamma, beta, running_mean, running_var, momentum,
                           eps, mean, invstd, scale, shift, ws, num_batches_tracked, S(stream));
}
int saicv_bn_eval_coeffs(int C, const float* gamma, const float* beta, const float* running_mean,
                         const float* running_var, double eps, float* scale, float* shift,
                         void* stream) {
    return bn_eval_coeffs(C, gamma, beta, running_mean, running_var, eps, scale, shift, S(stream));
}
int saicv_bn_act_fwd(int dtype, const void* y, const void* res, void* z, const float* scale,
                     const float* shift, size_t M, int C, int relu, void* relu_mask, void* stream) {
    return bn_act_fwd(dtype, y, res, z, scale, shift, M, C, relu, relu_mask, S(stream));
}
size_t saicv_bn_bwd_ws_floats(size_t M, int C, int dtype) { return bn_bwd_ws_floats(M, C, dtype); }
int saicv_bn_act_bwd(int dtype, const void* dz, const void* z, const void* relu_mask, const void* y, const float* gamma,
                     const float* mean, const float* invstd, void* dy, void* dres, float* dgamma,
                     float* dbeta, size_t M, int C, int relu, int accumulate, float* ws, void* stream) {
    return bn_bwd(dtype, dz, z, relu_mask, y, gamma, mean, invstd, dy, dres, dgamma, dbeta, M, C, relu, accumulate, ws,
                  S(stream));
}

int saicv_conv2d_fwd_stats(const saicv_conv_desc* d, const void* x, const void* wf, void* y, float* stat_sum, float* stat_sq,
                           int stat_rows, void* stream) {
    if (check_desc(d, "saicv_conv2d_fwd_stats")) return -1;
    if (!stat_sum || !stat_sq || stat_rows < 1) { set_error("saicv_conv2d_fwd_stats: statistics rows missing"); return -1; }
    const int M = d->N * d->OH * d->OW;
    EpiExtra ex;
    ex.stat_atomic_rows = stat_rows;
    return igemm_nt(d->dtype, 0, x, wf, y, nullptr, stat_sum, stat_sq, d->H, d->W, d->C, d->OH, d->OW,
                    d->R, d->S, d->stride, d->pad, M, d->K, d->R * d->S * d->C, d->K, 0, S(stream), &ex);
}
int saicv_bn_act_fwd_stats(int dtype, const void* y, const void* res, void* z, const float* stat_sum, const float* stat_sq,
                           int stat_rows, double count, const float* gamma, const float* beta, float* running_mean,
                           float* running_var, double momentum, double eps, long long* num_batches_tracked, float* mean,
                           float* invstd, size_t M, int C, int relu, void* relu_mask, void* stream) {
    return bn_act_fwd_stats(dtype, y, res, z, stat_sum, stat_sq, stat_rows, count, gamma, beta, running_mean, running_var,
                            momentum, eps, num_batches_tracked, mean, invstd, M, C, relu, relu_mask, S(stream));
}
int saicv_bn_act_fwd_join(int dtype, const void* y, const void* res, const float* res_scale, const float* res_shift, void* z,
                          const float* scale, const float* shift, const float* stat_sum, const float* stat_sq, int stat_rows,
                          double count, const float* gamma, const float* beta, float* running_mean, float* running_var,
                          double momentum, double eps, long long* num_batches_tracked, float* mean, float* invstd, size_t M, int C,
                          int relu, void* relu_mask, void* stream) {
    return bn_act_fwd_join(dtype, y, res, res_scale, res_shift, z, scale, shift, stat_sum, stat_sq, stat_rows, count, gamma, beta,
                           running_mean, running_var, momentum, eps, num_batches_tracked, mean, invstd, M, C, relu, relu_mask,
                           S(stream));
}
int saicv_bn_act_bwd_inline(int dtype, const void* dz, const void* relu_mask, const void* y, const float* gamma,
                            const float* mean, const float* invstd, const float* part_g, const float* part_gx, int rows,
                            void* dy, void* dres, float* dgamma, float* dbeta, size_t M, int C, int relu, int accumulate,
                            void* stream) {
    return bn_bwd_inline(dtype, dz, relu_mask, y, gamma, mean, invstd, part_g, part_gx, rows, dy, dres, dgamma, dbeta, M, C,
                         relu, accumulate, S(stream));
}

int saicv_bn_act_bwd_from_partials(int dtype, const void* dz, const void* relu_mask, const void* y, const float* gamma,
                                   const float* mean, const float* invstd, const float* part_g, const float* part_gx,
                                   int rows, void* dy, void* dres, float* dgamma, float* dbeta, size_t M, int C, int relu,
                                   int accumulate, float* ws, void* stream) {
    return bn_bwd_from_partials(dtype, dz, relu_mask, y, gamma, mean, invstd, part_g, part_gx, rows, dy, dres, dgamma, dbeta,
                                M, C, relu, accumulate, ws, S(stream));
}

int saicv_maxpool_fwd(int dtype, const void* x, void* out, uint8_t* idx, int N, int H, int W, int C,
                      int OH, int OW, int K, int stride, int pad, void* stream) {
    return maxpool_fwd(dtype, x, out, idx, N, H, W, C, OH, OW, K, stride, pad, S(stream));
}
int saicv_maxpool_bwd(int dtype, const void* dout, const uint8_t* idx, void* dx, int N, int H, int W,
                      int C, int OH, int OW, int K, int stride, int pad, void* stream) {
    return maxpool_bwd(dtype, dout, idx, dx, N, H, W, C, OH, OW, K, stride, pad, S(stream));
}
int saicv_bn_relu_maxpool_fwd(int dtype, const void* y, const float* scale, const float* shift, void* out, uint8_t* idx, int N, int H,
                              int W, int C, int OH, int OW, int K, int stride, int pad, void* stream) {
    return bn_relu_maxpool_fwd(dtype, y, scale, shift, out, idx, N, H, W, C, OH, OW, K, stride, pad, S(stream));
}
size_t saicv_bn_relu_maxpool_bwd_ws_floats(int C) { return 2 * (size_t)C; }
int saicv_bn_relu_maxpool_bwd(int dtype, const void* dout, const uint8_t* idx, const void* y, const float* gamma, const float* mean,
                              const float* invstd, const float* scale, const float* shift, void* dy, float* dgamma, float* dbeta,
                              int accumulate, float* ws, int N, int H, int W, int C, int OH, int OW, int K, int stride, int pad,
                              void* stream) {
    return bn_relu_maxpool_bwd(dtype, dout, idx, y, gamma, mean, invstd, scale, shift, dy, dgamma, dbeta, accumulate, ws, N, H, W, C,
                               OH, OW, K, stride, pad, S(stream));
}
int saicv_bn_relu_maxpool_fwd_keep(int dtype, const void* y, const float* scale, const float* shift, void* out, uint8_t* idx, void* ya,
                                   int N, int H, int W, int C, int OH, int OW, int K, int stride, int pad, void* stream) {
    return bn_relu_maxpool_fwd_keep(dtype, y, scale, shift, out, idx, ya, N, H, W, C, OH, OW, K, stride, pad, S(stream));
}
int saicv_bn_relu_maxpool_bwd_sums(int dtype, const void* dout, const void* ya, const float* mean, const float* invstd,
                                   const float* scale, const float* shift, float* sums, int N, int OH, int OW, int C, void* stream) {
    return bn_relu_maxpool_bwd_sums(dtype, dout, ya, mean, invstd, scale, shift, sums, N, OH, OW, C, S(stream));
}
int saicv_bn_relu_maxpool_bwd_apply(int dtype, const void* dout, const uint8_t* idx, const void* y, const float* gamma, const float* mean,
                                    const float* invstd, const float* scale, const float* shift, const float* sums, void* dy,
                                    float* dgamma, float* dbeta, int accumulate, int N, int H, int W, int C, int OH, int OW, int K,
                                    int stride, int pad, void* stream) {
    return bn_relu_maxpool_bwd_apply(dtype, dout, idx, y, gamma, mean, invstd, scale, shift, sums, dy, dgamma, dbeta, accumulate, N, H, W,
                                     C, OH, OW, K, stride, pad, S(stream));
}
// BatchNorm-backward apply + weight gradient of the pooled space-to-depth stem as one stream (stembwd.hip)
int saicv_stem_bwd_stream_ok(int dtype, int N, int H, int W, int CO, int CQ, int R, int S_, int pool_k, int pool_stride, int pool_pad) {
    return stem_bwd_stream_ok(dtype, N, H, W, CO, CQ, R, S_, pool_k, pool_stride, pool_pad);
}
size_t saicv_stem_bwd_stream_ws_floats(int N, int H, int W) { return stem_bwd_stream_ws_floats(N, H, W); }
int saicv_stem_bwd_stream(int dtype, const void* dout, const uint8_t* idx, const void* y, const float* gamma, const float* mean,
                          const float* invstd, const float* scale, const float* shift, const float* sums, const void* x, float* dw,
                          float* dgamma, float* dbeta, int accumulate, float* ws, int N, int H, int W, int CO, int CQ, int R, int S_,
                          int pool_k, int pool_stride, int pool_pad, void* stream) {
    SAICV_REQUIRE(stem_bwd_stream_supported(dtype, N, H, W, CO, CQ, R, S_, pool_k, pool_stride, pool_pad),
                  "saicv_stem_bwd_stream: no form for dtype %d, N = %d, %d x %d outputs, Cout = %d, %d x %d taps over %d channels, pool (%d, %d, %d) "
                  "(bf16, 64 channels, 4 x 4 taps over 16, pool (3, 2, 1), operands below 4 GiB)", dtype, N, H, W, CO, R, S_, CQ, pool_k,
                  pool_stride, pool_pad);
    return stem_bwd_stream(dout, idx, y, gamma, mean, invstd, scale, shift, sums, x, dw, dgamma, dbeta, accumulate, ws, N, H, W, S(stream));
}

int saicv_avgpool_fwd(int dtype, const void* x, void* out, int N, int HW, int C, void* stream) {
    return avgpool_fwd(dtype, x, out, N, HW, C, S(stream));
}
int saicv_avgpool_bwd(int dtype, const void* dout, void* dx, int N, int HW, int C, void* stream) {
    return avgpool_bwd(dtype, dout, dx, N, HW, C, S(stream));
}

int saicv_softmax_ce_fwd(const float* logits, const void* label, int soft, int B, int C,
                         float* row_loss, float* loss, float* dlogits, void* stream) {
    return softmax_ce_fwd(logits, label, soft, B, C, row_loss, loss, dlogits, S(stream));
}
int saicv_scale_by_scalar(int out_dtype, const float* in, const float* scale, void* out, size_t n,
                          void* stream) {
    return scale_by_scalar(out_dtype, in, scale, out, n, S(stream));
}

int saicv_sgd_flat(float* p, const float* g, float* mom, const int32_t* block_group,
                   const float* hyper, const float* inv_scale, const float* found_inf,
                   const uint8_t* has_grad, size_t n, void* stream) {
    return sgd_flat(p, g, mom, block_group, hyper, inv_scale, found_inf, has_grad, n, S(stream));
}
int saicv_adamw_flat(float* p, const float* g, float* m, float* v, const int32_t* block_group,
                     const float* hyper, const float* inv_scale, const float* found_inf,
                     const uint8_t* has_grad, float* step_blk, size_t n, void* stream) {
    return adamw_flat(p, g, m, v, block_group, hyper, inv_scale, found_inf, has_grad, step_blk, n, S(stream));
}
int saicv_muon_prepare(float* p, const float* g, float* s1, float* s2, const int32_t* block_prob, const int32_t* tab,
                       const float* hyper, const float* inv_scale, const float* found_inf, const uint8_t* has_grad,
                       float* step_blk, void* xws, size_t n, void* stream) {
    return muon_prepare(p, g, s1, s2, block_prob, tab, hyper, inv_scale, found_inf, has_grad, step_blk, xws, n, S(stream));
}
int saicv_muon_newton_schulz(void* x0, void* x1, void* amat, void* bmat, float* da, float* db, const int32_t* tab, int nprob, int tiles_sym,
                             int tiles_full, int steps, double a, double b, double c, int normalize, float* partials,
                             void* stream) {
    return muon_newton_schulz(x0, x1, amat, bmat, da, db, tab, nprob, tiles_sym, tiles_full, steps, a, b, c, normalize, partials, S(stream));
}
int saicv_muon_apply(float* p, const void* uws, const int32_t* block_prob, const int32_t* tab, const float* hyper,
                     const float* found_inf, const uint8_t* has_grad, size_t n, void* stream) {
    return muon_apply(p, uws, block_prob, tab, hyper, found_inf, has_grad, n, S(stream));
}
int saicv_grad_stats(const float* g, size_t n, float* found_inf, float* sumsq, void* stream) {
    return grad_stats(g, n, found_inf, sumsq, S(stream));
}
int saicv_grad_clip_scale(float* g, size_t n, const float* sumsq, const float* inv_scale,
                          double max_norm, void* stream) {
    return grad_clip_scale(g, n, sumsq, inv_scale, max_norm, S(stream));
}
int saicv_grad_clip_value(float* g, size_t n, const float* inv_scale, double value, void* stream) {
    return grad_clip_value(g, n, inv_scale, value, S(stream));
}
int saicv_scaler_update(float* state, const float* found_inf, double growth, double backoff,
                        int interval, void* stream) {
    return scaler_update(state, found_inf, growth, backoff, interval, S(stream));
}

int saicv_layernorm_fwd(int dtype, const void* x, const float* gamma, const float* beta, void* y, float* mean,
                        float* rstd, int M, int C, double eps, void* stream) {
    return layernorm_fwd(dtype, x, gamma, beta, y, mean, rstd, M, C, eps, S(stream));
}
size_t saicv_layernorm_bwd_ws_floats(int M, int C) { return layernorm_bwd_ws_floats(M, C); }
int saicv_layernorm_bwd(int dtype, const void* dy, const void* x, const float* gamma, const float* mean,
                        const float* rstd, const void* addend, void* dx, float* dgamma, float* dbeta, float* ws,
                        int M, int C, int accumulate, void* stream) {
    return layernorm_bwd(dtype, dy, x, gamma, mean, rstd, addend, dx, dgamma, dbeta, ws, M, C, accumulate, S(stream));
}
int saicv_dropout_add_layernorm_fwd(int dtype, const void* x, const void* branch, double p, unsigned int seed, const unsigned int* seed_device,
                                    const float* gamma, const float* beta, void* sum_out, void* y, float* mean, float* rstd, int M, int C,
                                    double eps, void* stream) {
    return dropout_add_layernorm_fwd(dtype, x, branch, p, seed, seed_device, gamma, beta, sum_out, y, mean, rstd, M, C, eps, S(stream));
}
int saicv_dropout_add_layernorm_bwd(int dtype, const void* dy, const void* sum, const float* gamma, const float* mean, const float* rstd,
                                    double p, unsigned int seed, const unsigned int* seed_device, void* dsum, void* dbranch,
                                    float* dgamma, float* dbeta, float* ws, int M, int C, int accumulate, void* stream) {
    return dropout_add_layernorm_bwd(dtype, dy, sum, gamma, mean, rstd, p, seed, seed_device, dsum, dbranch, dgamma, dbeta, ws, M, C,
                                     accumulate, S(stream));
}
int saicv_layernorm_bwd_scaled(int dtype, const void* dy, const void* x, const float* gamma, const float* mean,
                               const float* rstd, const void* addend, void* dx, float* dgamma, float* dbeta, float* ws,
                               int M, int C, int accumulate, const float* out_scale, int rows_per_scale, void* dx_scaled, void* stream) {
    return layernorm_bwd(dtype, dy, x, gamma, mean, rstd, addend, dx, dgamma, dbeta, ws, M, C, accumulate, S(stream), out_scale,
                         rows_per_scale, dx_scaled);
}
int saicv_gelu_fwd(int dtype, const void* x, void* y, size_t n, void* stream) {
    return gelu_fwd(dtype, x, y, n, S(stream));
}
int saicv_gelu_bwd(int dtype, const void* dy, const void* x, void* dx, size_t n, void* stream) {
    return gelu_bwd(dtype, dy, x, dx, n, S(stream));
}
int saicv_relu_dropout_fwd(int dtype, const void* x, void* y, size_t n, double p, unsigned int seed, const unsigned int* seed_device, void* stream) {
    return relu_dropout_fwd(dtype, x, y, n, p, seed, seed_device, S(stream));
}
int saicv_relu_dropout_bwd(int dtype, const void* dy, const void* y, void* dx, size_t n, double p, void* stream) {
    return relu_dropout_bwd(dtype, dy, y, dx, n, p, S(stream));
}
int saicv_attention_fwd(int dtype, const void* qkv, void* out, float* lse, int B, int N, int H, int D,
                        double scale, void* stream) {
    return attention_fwd(dtype, qkv, out, lse, B, N, H, D, scale, S(stream));
}
int saicv_attention_bwd(int dtype, const void* qkv, const void* out, const void* dout, const float* lse,
                        void* dqkv, int B, int N, int H, int D, double scale, void* stream) {
    return attention_bwd(dtype, qkv, out, dout, lse, dqkv, B, N, H, D, scale, S(stream));
}
int saicv_window_partition(int dtype, const void* x, void* out, int B, int H, int W, int C, int ws, void* stream) {
    return window_partition(dtype, x, out, B, H, W, C, ws, S(stream));
}
int saicv_window_unpartition(int dtype, const void* win, const void* addend, void* out, int B, int H, int W, int C, int ws,
                             void* stream) {
    return window_unpartition(dtype, win, addend, out, B, H, W, C, ws, S(stream));
}
int saicv_relpos_fwd(int dtype, const void* q, long q_rs, long q_bs, const float* tab_h, const float* tab_w, float* rel_h,
                     float* rel_w, int B, int heads, int Sh, int Sw, void* stream) {
    return relpos_fwd(dtype, q, q_rs, q_bs, tab_h, tab_w, rel_h, rel_w, B, heads, Sh, Sw, S(stream));
}
int saicv_relpos_bwd(int dtype, const void* q, void* dq, long q_rs, long q_bs, const float* tab_h, const float* tab_w,
                     const float* d_rel_h, const float* d_rel_w, float* dtab_h, float* dtab_w, float* ws, int B, int heads,
                     int Sh, int Sw, void* stream) {
    return relpos_bwd(dtype, q, dq, q_rs, q_bs, tab_h, tab_w, d_rel_h, d_rel_w, dtab_h, dtab_w, ws, B, heads, Sh, Sw, S(stream));
}
size_t saicv_relpos_bwd_ws_floats(int Sh, int Sw) { return relpos_bwd_ws_floats(Sh, Sw); }
int saicv_mask_loss_stats(int dtype, const void* logits, const float* targets, float* stats, int B, int M, size_t HW,
                          double alpha, double gamma, double thr, void* stream) {
    return mask_loss_stats(dtype, logits, targets, stats, B, M, HW, alpha, gamma, thr, S(stream));
}
int saicv_mask_loss_grad(int dtype, const void* logits, const float* targets, const float* coef, void* dlogits, int B,
                         int M, size_t HW, double alpha, double gamma, void* stream) {
    return mask_loss_grad(dtype, logits, targets, coef, dlogits, B, M, HW, alpha, gamma, S(stream));
}
int saicv_hyper_product_fwd(int dtype, const void* x, const void* hyper, void* out, int B, int T, int P, int C, void* stream) {
    return hyper_product_fwd(dtype, x, hyper, out, B, T, P, C, S(stream));
}
int saicv_hyper_product_bwd(int dtype, const void* x, const void* hyper, const void* dout, void* dx, float* dhyper, int B,
                            int T, int P, int C, void* stream) {
    return hyper_product_bwd(dtype, x, hyper, dout, dx, dhyper, B, T, P, C, S(stream));
}
int saicv_upsample4_fwd(int dtype, const void* low, void* out, int planes, int h, int w, void* stream) {
    return upsample4_fwd(dtype, low, out, planes, h, w, S(stream));
}
int saicv_upsample4_bwd(int dtype, const void* dhi, void* dlow, int planes, int h, int w, void* stream) {
    return upsample4_bwd(dtype, dhi, dlow, planes, h, w, S(stream));
}
int saicv_mask_loss_stats_up4(int dtype, const void* low, const float* targets, float* stats, int B, int M, int h, int w,
                              double alpha, double gamma, double thr, void* stream) {
    return mask_loss_stats_up4(dtype, low, targets, stats, B, M, h, w, alpha, gamma, thr, S(stream));
}
int saicv_mask_loss_grad_up4(int dtype, const void* low, const float* targets, const float* coef, void* dlow, int B, int M,
                             int h, int w, double alpha, double gamma, void* stream) {
    return mask_loss_grad_up4(dtype, low, targets, coef, dlow, B, M, h, w, alpha, gamma, S(stream));
}
size_t saicv_pixel_softmax_ce_ws_floats(size_t rows) { return pixel_softmax_ce_ws_floats(rows); }
int saicv_pixel_softmax_ce_fwd(int dtype, const void* logits, const float* label, size_t rows, int C, float* lse, float* partial,
                               float* loss, void* stream) {
    return pixel_softmax_ce_fwd(dtype, logits, label, rows, C, lse, partial, loss, S(stream));
}
int saicv_pixel_softmax_ce_bwd(int dtype, const void* logits, const float* label, const float* lse, const float* upstream,
                               size_t rows, int C, void* dlogits, void* stream) {
    return pixel_softmax_ce_bwd(dtype, logits, label, lse, upstream, rows, C, dlogits, S(stream));
}
int saicv_cpfe_gather_fwd(int dtype, const float* z, long ldz, void* out, int N, int H, int W, int P, int nb, int d0, int d1,
                          int d2, void* stream) {
    const int dil[3] = {d0, d1, d2};
    return cpfe_gather_fwd(dtype, z, ldz, out, N, H, W, P, nb, dil, S(stream));
}
int saicv_cpfe_gather_bwd(int dtype, const void* dout, void* dz, int N, int H, int W, int P, int nb, int d0, int d1, int d2,
                          void* stream) {
    const int dil[3] = {d0, d1, d2};
    return cpfe_gather_bwd(dtype, dout, dz, N, H, W, P, nb, dil, S(stream));
}
size_t saicv_conv3x3_c1_ws_floats(int N, int H, int W, int C) { return conv3x3_c1_ws_floats(N, H, W, C); }
int saicv_conv3x3_c1_fwd(int dtype, const void* x, const float* weight, long wsc, long wsk, const float* bias, float* out, int N,
                         int H, int W, int C, int sigmoid, void* stream) {
    return conv3x3_c1_fwd(dtype, x, weight, wsc, wsk, bias, out, N, H, W, C, sigmoid, S(stream));
}
int saicv_conv3x3_c1_bwd(int dtype, const void* x, const float* weight, long wsc, long wsk, const float* p, const float* dout,
                         void* dx, float* dw, float* db, float* ws, int N, int H, int W, int C, int sigmoid, int accumulate,
                         void* stream) {
    return conv3x3_c1_bwd(dtype, x, weight, wsc, wsk, p, dout, dx, dw, db, ws, N, H, W, C, sigmoid, accumulate, S(stream));
}
size_t saicv_binary_seg_stats_ws_floats(int B, size_t P) { return binary_seg_stats_ws_floats(B, P); }
int saicv_binary_seg_stats_fwd(const float* prob, const float* label, int B, size_t P, float* partial, float* stats, void* stream) {
    return binary_seg_stats_fwd(prob, label, B, P, partial, stats, S(stream));
}
int saicv_binary_seg_stats_bwd(const float* prob, const float* label, const float* gstats, int B, size_t P, float* dprob,
                               void* stream) {
    return binary_seg_stats_bwd(prob, label, gstats, B, P, dprob, S(stream));
}
size_t saicv_matting_ws_floats(int B, size_t P) { return matting_ws_floats(B, P); }
int saicv_trimap_stats_fwd(const float* global_pred, long sb, long sc, long sp, const float* trimap, int B, size_t P, float smooth,
                           float* partial, float* stats, void* stream) {
    return trimap_stats_fwd(global_pred, sb, sc, sp, trimap, B, P, smooth, partial, stats, S(stream));
}
int saicv_trimap_stats_bwd(const float* global_pred, long sb, long sc, long sp, const float* trimap, const float* gstats, int B,
                           size_t P, float smooth, float* dglobal, void* stream) {
    return trimap_stats_bwd(global_pred, sb, sc, sp, trimap, gstats, B, P, smooth, dglobal, S(stream));
}
int saicv_alpha_l1_fwd(const float* pred, const float* alpha, const float* trimap, int B, size_t P, float* partial, float* sums,
                       void* stream) {
    return alpha_l1_fwd(pred, alpha, trimap, B, P, partial, sums, S(stream));
}
int saicv_alpha_l1_bwd(const float* pred, const float* alpha, const float* trimap, const float* gsums, int B, size_t P, float* dpred,
                       void* stream) {
    return alpha_l1_bwd(pred, alpha, trimap, gsums, B, P, dpred, S(stream));
}
int saicv_composition_l1_fwd(const float* pred, const float* fg, const float* bg, const float* image, int B, size_t P,
                             float* partial, float* sums, void* stream) {
    return composition_l1_fwd(pred, fg, bg, image, B, P, partial, sums, S(stream));
}
int saicv_composition_l1_bwd(const float* pred, const float* fg, const float* bg, const float* image, const float* gsums, int B,
                             size_t P, float* dpred, void* stream) {
    return composition_l1_bwd(pred, fg, bg, image, gsums, B, P, dpred, S(stream));
}
int saicv_matting_fuse_fwd(const float* global_pred, long sb, long sc, long sp, const float* local_pred, int B, size_t P,
                           float* fused, void* stream) {
    return matting_fuse_fwd(global_pred, sb, sc, sp, local_pred, B, P, fused, S(stream));
}
int saicv_matting_fuse_bwd(const float* global_pred, long sb, long sc, long sp, const float* dfused, int B, size_t P, float* dlocal,
                           void* stream) {
    return matting_fuse_bwd(global_pred, sb, sc, sp, dfused, B, P, dlocal, S(stream));
}
size_t saicv_lap_level_ws_floats(int B, int h, int w) { return lap_level_ws_floats(B, h, w); }
int saicv_lap_level_fwd(const float* src, const float* alpha, const float* trimap, int level0, int B, int h, int w,
                        const float* table, float* next, float* partial, float* sum_e, float* sum_next, void* stream) {
    if (!table) { set_error("lap_level_fwd: null weight table"); return -1; }
    return lap_level_fwd(src, alpha, trimap, level0, B, h, w, table, next, partial, sum_e, sum_next, S(stream));
}
int saicv_lap_level_bwd(const float* src, const float* alpha, const float* trimap, int level0, int B, int h, int w,
                        const float* table, const float* gnext, const float* topcur, const float* gs, const float* gtop, float* gcur,
                        void* stream) {
    if (!table) { set_error("lap_level_bwd: null weight table"); return -1; }
    return lap_level_bwd(src, alpha, trimap, level0, B, h, w, table, gnext, topcur, gs, gtop, gcur, S(stream));
}
size_t saicv_group_matting_ws_floats(int B, int M, size_t P) { return group_matting_ws_floats(B, M, P); }
int saicv_group_matting_stats_fwd(int dtype, const void* global_preds, const void* local_preds, const void* fused_preds,
                                  const float* alpha, const float* trimap, const float* image, const float* fg, const float* bg, int B,
                                  int M, size_t P, float mask_threshold, float* partial, float* stats, void* stream) {
    return group_matting_stats_fwd(dtype, global_preds, local_preds, fused_preds, alpha, trimap, image, fg, bg, B, M, P,
                                   mask_threshold, partial, stats, S(stream));
}
int saicv_group_matting_stats_bwd(int dtype, const void* global_preds, const void* local_preds, const void* fused_preds,
                                  const float* alpha, const float* trimap, const float* image, const float* fg, const float* bg,
                                  const float* gstats, int B, int M, size_t P, void* dglobal, void* dlocal, void* dfused,
                                  void* stream) {
    return group_matting_stats_bwd(dtype, global_preds, local_preds, fused_preds, alpha, trimap, image, fg, bg, gstats, B, M, P,
                                   dglobal, dlocal, dfused, S(stream));
}
int saicv_lap_level0_group_fwd(const float* src, const float* alpha, const float* trimap, int group, int R, int h, int w,
                               const float* table, float* next, float* partial, float* sum_e, void* stream) {
    if (!table) { set_error("lap_level0_group_fwd: null weight table"); return -1; }
    return lap_level0_group_fwd(src, alpha, trimap, group, R, h, w, table, next, partial, sum_e, S(stream));
}
int saicv_lap_level_group_bwd(const float* src, const float* alpha, const float* trimap, int level0, int group, int R, int h, int w,
                              const float* table, const float* gnext, const float* topcur, const float* gs, const float* gtop,
                              const float* gall, int nsum, float* gcur, void* stream) {
    if (!table) { set_error("lap_level_group_bwd: null weight table"); return -1; }
    return lap_level_group_bwd(src, alpha, trimap, level0, group, R, h, w, table, gnext, topcur, gs, gtop, gall, nsum, gcur,
                               S(stream));
}
size_t saicv_pixel_class_terms_ws_floats(size_t rows) { return pixel_class_terms_ws_floats(rows); }
int saicv_pixel_class_terms_lane_max_classes(void) { return pixel_class_terms_lane_max_classes(); }
int saicv_pixel_class_terms_fwd(int dtype, const void* logits, const float* label, size_t rows, int C, int sigmoid, int form,
                                float* partial, float* terms, void* stream) {
    return pixel_class_terms_fwd(dtype, logits, label, rows, C, sigmoid, form, partial, terms, S(stream));
}
int saicv_pixel_class_terms_bwd(int dtype, const void* logits, const float* label, const float* gterms, size_t rows, int C,
                                int sigmoid, int form, void* dlogits, void* stream) {
    return pixel_class_terms_bwd(dtype, logits, label, gterms, rows, C, sigmoid, form, dlogits, S(stream));
}
int saicv_lstm_fwd(int dtype, float* gates, const void* whh, void* y, float* c, int B, int T, int H, void* stream) {
    return lstm_fwd(dtype, gates, whh, y, c, B, T, H, S(stream));
}
int saicv_lstm_bwd(int dtype, const void* dy, const float* gates, const float* c, const void* whh_t, void* dgates, int B, int T, int H,
                   void* stream) {
    return lstm_bwd(dtype, dy, gates, c, whh_t, dgates, B, T, H, S(stream));
}
size_t saicv_ctc_ws_floats(int T, int B, int Sx) { return ctc_ws_floats(T, B, Sx); }
int saicv_ctc_loss_fwd(int dtype, const void* logits, long long st, long long sb, const int* targets, const int* input_lengths,
                       const int* target_lengths, int T, int B, int Sx, int C, int blank, int focal, float gamma, float* ws, float* nll,
                       float* loss, void* stream) {
    return ctc_loss_fwd(dtype, logits, st, sb, targets, input_lengths, target_lengths, T, B, Sx, C, blank, focal, gamma, ws, nll, loss,
                        S(stream));
}
int saicv_ctc_loss_bwd(int dtype, const void* logits, long long st, long long sb, void* dlogits, long long dst, long long dsb,
                       const int* input_lengths, const int* target_lengths, const float* ws, const float* nll, const float* gout, int T,
                       int B, int Sx, int C, int focal, float gamma, void* stream) {
    return ctc_loss_bwd(dtype, logits, st, sb, dlogits, dst, dsb, input_lengths, target_lengths, ws, nll, gout, T, B, Sx, C, focal,
                        gamma, S(stream));
}
int saicv_ctc_greedy(int dtype, const void* logits, long long st, long long sb, const int* input_lengths, int T, int B, int C,
                     int* index, float* prob, void* stream) {
    return ctc_greedy(dtype, logits, st, sb, input_lengths, T, B, C, index, prob, S(stream));
}
int saicv_univseg_chunk(void) { return univseg_chunk(); }
size_t saicv_univseg_pair_ws_floats(int B, int Q, int total_t, size_t P) { return univseg_pair_ws_floats(B, Q, total_t, P); }
int saicv_univseg_pair_sums(int dtype, const void* mask_preds, const float* targets, const int* offsets, int B, int Q, int total_t,
                            int max_t, size_t P, float* partial, float* sums, void* stream) {
    return univseg_pair_sums(dtype, mask_preds, targets, offsets, B, Q, total_t, max_t, P, partial, sums, S(stream));
}
size_t saicv_univseg_matched_ws_floats(int M, size_t P) { return univseg_matched_ws_floats(M, P); }
int saicv_univseg_matched_fwd(int dtype, const void* mask_preds, const float* targets, const int* pred_rows, const int* target_rows,
                              int M, size_t P, float* partial, float* stats, void* stream) {
    return univseg_matched_fwd(dtype, mask_preds, targets, pred_rows, target_rows, M, P, partial, stats, S(stream));
}
int saicv_univseg_matched_bwd(int dtype, const void* mask_preds, const float* targets, const int* row_pair, const int* target_rows,
                              const float* gstats, int rows, size_t P, void* dmask_preds, void* stream) {
    return univseg_matched_bwd(dtype, mask_preds, targets, row_pair, target_rows, gstats, rows, P, dmask_preds, S(stream));
}
int saicv_attention_stream_fwd(int dtype, int D, const saicv_attn_desc* desc, void* stream) {
    if (!desc) { set_error("attention_stream: null descriptor"); return -1; }
    return attention_stream(dtype, D, 0, desc, S(stream));
}
int saicv_attention_stream_bwd(int dtype, int D, const saicv_attn_desc* desc, void* stream) {
    if (!desc) { set_error("attention_stream: null descriptor"); return -1; }
    if (!desc->dout || !desc->dq || !desc->dk || !desc->dv || !desc->dsum) {
        set_error("attention_stream_bwd: dout / dq / dk / dv / dsum are required");
        return -1;
    }
    if (desc->rel_h && (!desc->d_rel_h || !desc->d_rel_w)) {
        set_error("attention_stream_bwd: d_rel_h / d_rel_w are required with rel_h / rel_w");
        return -1;
    }
    const int rc = attention_stream(dtype, D, 1, desc, S(stream));
    return rc ? rc : attention_stream(dtype, D, 2, desc, S(stream));
}

}  // extern "C"
