// The entry points of include/saicv_hip.h that compose internal functions: the error state, the convolution / linear products on
// igemm_nt / igemm_tn, the fused streams.  Every other entry point is defined in the unit that owns its kernels.
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

}  // namespace saicv

using namespace saicv;

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
int saicv_c3_bwd_stream(int dtype, const void* dz, const void* relu_mask, const void* y, const float* gamma, const float* mean,
                        const float* invstd, const float* part_g, const float* part_gx, int rows, float* dgamma, float* dbeta,
                        int accumulate, float* ws, const void* x, const void* wd, const saicv_dgrad_fuse* f, void* dx, float* dw,
                        int M, int CO, int CI, void* stream) {
    SAICV_REQUIRE(dtype == SAICV_BF16, "saicv_c3_bwd_stream: bf16 only (dtype %d)", dtype);
    SAICV_REQUIRE(saicv_c3_bwd_stream_rows(M, CO, CI) > 0, "saicv_c3_bwd_stream: no form for M = %d, Cout = %d, Cin = %d", M, CO, CI);
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

size_t saicv_bn_relu_maxpool_bwd_ws_floats(int C) { return 2 * (size_t)C; }
// BatchNorm-backward apply + weight gradient of the pooled space-to-depth stem as one stream (stembwd.hip)
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

int saicv_layernorm_bwd(int dtype, const void* dy, const void* x, const float* gamma, const float* mean,
                        const float* rstd, const void* addend, void* dx, float* dgamma, float* dbeta, float* ws,
                        int M, int C, int accumulate, void* stream) {
    return layernorm_bwd(dtype, dy, x, gamma, mean, rstd, addend, dx, dgamma, dbeta, ws, M, C, accumulate, S(stream));
}
int saicv_layernorm_bwd_scaled(int dtype, const void* dy, const void* x, const float* gamma, const float* mean,
                               const float* rstd, const void* addend, void* dx, float* dgamma, float* dbeta, float* ws,
                               int M, int C, int accumulate, const float* out_scale, int rows_per_scale, void* dx_scaled, void* stream) {
    return layernorm_bwd(dtype, dy, x, gamma, mean, rstd, addend, dx, dgamma, dbeta, ws, M, C, accumulate, S(stream), out_scale,
                         rows_per_scale, dx_scaled);
}

}  // extern "C"
