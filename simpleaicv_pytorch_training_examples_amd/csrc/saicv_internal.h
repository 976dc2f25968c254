// Internal C++ declarations shared between the .hip translation units and capi.hip.
#pragma once
#include <hip/hip_runtime.h>

struct saicv_conv_desc;      // include/saicv_hip.h
struct saicv_plan_query;
struct saicv_plan;

namespace saicv {

void set_error(const char* fmt, ...);
int check_launch(const char* what);

// igemm.hip: rows of partial statistics saicv_conv2d_fwd writes with statistics (the launch's own plan)
int conv_stat_rows(const saicv_conv_desc* d);
// optional epilogue extras: out = addend + row_scale[m / rows_per_scale] * (acc + bias)
struct EpiExtra {
    const void* addend = nullptr;      // same dtype / layout as out
    const float* row_scale = nullptr;  // one factor per group of rows_per_scale rows (drop-path)
    int rows_per_scale = 1;
    int act_mode = 0;                  // 1: out2 = gelu(out) ; 2: out = (acc + bias) * gelu'(addend)
    void* out2 = nullptr;
    // data-gradient extras (igemm.hip NTParams): gate bits of the addend; BatchNorm-backward partial sums of the output
    const uint8_t* addend_gate = nullptr;
    const void* bs_y = nullptr;
    const uint8_t* bs_mask = nullptr;      // nullptr: no ReLU in front (every element counts)
    const float* bs_mean = nullptr;
    const float* bs_invstd = nullptr;
    float* bs_g = nullptr;
    float* bs_gx = nullptr;
    int stat_atomic_rows = 0;              // > 0: statistics added atomically into this many rows of a zeroed buffer
};
// ... and the BatchNorm-backward partial rows saicv_conv2d_dgrad_fused writes with bn_y
int conv_bwd_stat_rows(const saicv_conv_desc* d);
int igemm_nt(int dtype, int mode, const void* src, const void* wgt, void* out, const float* bias,
             float* stat_sum, float* stat_sq, int H, int W, int C, int OH, int OW, int R, int S,
             int stride, int pad, int M, int Nn, int Kd, int ldo, int out_f32, hipStream_t st,
             const EpiExtra* ex = nullptr);
int igemm_tn(int dtype, const void* dy, const void* src, float* dw, int H, int W, int C, int OH,
             int OW, int R, int S, int stride, int pad, int M, int Cout, int Kd, hipStream_t st,
             float* dbias = nullptr);

// igemm.hip: the launch plan of the product a public entry point would build (saicv_igemm_plan); q's descriptor is already checked
int igemm_plan(const saicv_plan_query* q, saicv_plan* out);

// pwstream.hip: weight-resident streaming kernel for small pointwise products; blocks = rows of partial statistics (0: not eligible).
// igemm_nt launches them with the block count of its plan.
int pw_stream_blocks(int dtype, int M, int Nn, int Kd, bool fused_dgrad);
int pw_stream(int M, int Nn, int Kd, const void* src, const void* wgt, void* out, float* stat_sum, float* stat_sq,
              int stat_atomic_rows, const EpiExtra* ex, int stream_out, int blocks, hipStream_t st);
int pw3_stream_blocks(int dtype, int M, int Nn, int Kd);
int pw3_stream(int mode, int M, int H, int W, const void* src, const void* wgt, void* out, float* stat_sum, float* stat_sq,
               int stat_atomic_rows, const EpiExtra* ex, int stream_out, int blocks, hipStream_t st);

// c3bwd.hip: BatchNorm-backward apply + data gradient + weight gradient of a bottleneck's third convolution as one stream (dy never
// stored); blocks = rows of partial BatchNorm-backward sums (0: not eligible).  coef = [3][CO] of bn_bwd_coeffs.
int c3_bwd_stream_blocks(int dtype, int M, int CO, int CI);
int c3_bwd_stream_rows(int M, int CO, int CI);
int c3_bwd_stream(int M, int CO, int CI, const void* dz, const void* y, const void* mask, const float* coef, const void* x,
                  const void* wd, void* dx, float* dw, const EpiExtra* ex, int bs_rows, float* part_ws, hipStream_t st);
size_t c3_bwd_stream_ws_floats(int M, int CO, int CI);
// pool.hip: the pooled stem's forward that also keeps the raw y at each recorded maximum (ya, pooled size), and the two per-channel
// sums of its backward taken from ya instead of from the windows of y
int bn_relu_maxpool_fwd_keep(int dtype, const void* y, const float* scale, const float* shift, void* out, uint8_t* idx, void* ya,
                             int Nimg, int H, int W, int C, int OH, int OW, int K, int stride, int pad, hipStream_t st);
int bn_relu_maxpool_bwd_sums(int dtype, const void* dout, const void* ya, const float* mean, const float* invstd, const float* scale,
                             const float* shift, float* sums, int Nimg, int OH, int OW, int C, hipStream_t st);
// ... and the second pass of its backward alone, from given sums
int bn_relu_maxpool_bwd_apply(int dtype, const void* dout, const uint8_t* idx, const void* y, const float* gamma, const float* mean,
                              const float* invstd, const float* scale, const float* shift, const float* sums, void* dy, float* dgamma,
                              float* dbeta, int accumulate, int Nimg, int H, int W, int C, int OH, int OW, int K, int stride, int pad,
                              hipStream_t st);
// stembwd.hip: BatchNorm-backward apply + weight gradient of the pooled space-to-depth stem as one stream (dy never stored).
// H, W: the convolution output; _ok: which parts of the route the block takes (switches read per call): 0 none, bit 0 the sums
// from the kept maxima, bit 1 the stream kernel
bool stem_bwd_stream_supported(int dtype, int N, int H, int W, int CO, int cq, int taps_r, int taps_s, int pk, int ps, int pp);
int stem_bwd_stream_ok(int dtype, int N, int H, int W, int CO, int cq, int taps_r, int taps_s, int pk, int ps, int pp);
size_t stem_bwd_stream_ws_floats(int N, int H, int W);
int stem_bwd_stream(const void* dout, const uint8_t* idx, const void* y, const float* gamma, const float* mean, const float* invstd,
                    const float* scale, const float* shift, const float* sums, const void* x, float* dw, float* dgamma, float* dbeta,
                    int accumulate, float* part_ws, int N, int H, int W, hipStream_t st);
// bn.hip: the finalize step of BatchNorm backward alone: `rows` rows of partial sums -> dgamma, dbeta and the coefficients
// ca, cb, cc of dy = ca * g + cb * y + cc at ws + 64 * C (ws: 67 * C floats)
int bn_bwd_coeffs(const float* part_g, const float* part_gx, int rows, int C, size_t M, const float* gamma, const float* mean,
                  const float* invstd, float* dgamma, float* dbeta, int accumulate, float* ws, hipStream_t st);

// sam.hip
int window_partition(int dtype, const void* x, void* out, int B, int H, int W, int C, int ws, hipStream_t st);
int window_unpartition(int dtype, const void* win, const void* addend, void* out, int B, int H, int W, int C, int ws,
                       hipStream_t st);
int relpos_fwd(int dtype, const void* q, long q_rs, long q_bs, const float* tab_h, const float* tab_w, float* rel_h,
               float* rel_w, int B, int heads, int Sh, int Sw, hipStream_t st);
int relpos_bwd(int dtype, const void* q, void* dq, long q_rs, long q_bs, const float* tab_h, const float* tab_w,
               const float* d_rel_h, const float* d_rel_w, float* dtab_h, float* dtab_w, float* ws, int B, int heads, int Sh,
               int Sw, hipStream_t st);
size_t relpos_bwd_ws_floats(int Sh, int Sw);
// maskloss.hip
int mask_loss_stats(int dtype, const void* logits, const float* targets, float* stats, int B, int M, size_t HW,
                    double alpha, double gamma, double thr, hipStream_t st);
int mask_loss_grad(int dtype, const void* logits, const float* targets, const float* coef, void* dlogits, int B, int M,
                   size_t HW, double alpha, double gamma, hipStream_t st);
// samtail.hip
int hyper_product_fwd(int dtype, const void* x, const void* hyper, void* out, int B, int Tm, int P, int C, hipStream_t st);
int hyper_product_bwd(int dtype, const void* x, const void* hyper, const void* dout, void* dx, float* dhyper, int B, int Tm,
                      int P, int C, hipStream_t st);
int upsample4_fwd(int dtype, const void* low, void* out, int planes, int h, int w, hipStream_t st);
int upsample4_bwd(int dtype, const void* dhi, void* dlow, int planes, int h, int w, hipStream_t st);
int mask_loss_stats_up4(int dtype, const void* low, const float* targets, float* stats, int B, int M, int h, int w,
                        double alpha, double gamma, double thr, hipStream_t st);
int mask_loss_grad_up4(int dtype, const void* low, const float* targets, const float* coef, void* dlow, int B, int M, int h,
                       int w, double alpha, double gamma, hipStream_t st);
// semseg.hip
size_t pixel_softmax_ce_ws_floats(size_t rows);
int pixel_softmax_ce_fwd(int dtype, const void* logits, const float* label, size_t rows, int C, float* lse, float* partial,
                         float* loss, hipStream_t st);
int pixel_softmax_ce_bwd(int dtype, const void* logits, const float* label, const float* lse, const float* upstream, size_t rows,
                         int C, void* dlogits, hipStream_t st);
int cpfe_gather_fwd(int dtype, const float* z, long ldz, void* out, int N, int H, int W, int P, int nb, const int* dil,
                    hipStream_t st);
int cpfe_gather_bwd(int dtype, const void* dout, void* dz, int N, int H, int W, int P, int nb, const int* dil, hipStream_t st);
// salient.hip
size_t conv3x3_c1_ws_floats(int N, int H, int W, int C);
int conv3x3_c1_fwd(int dtype, const void* x, const float* weight, long wsc, long wsk, const float* bias, float* out, int N, int H,
                   int W, int C, int sigmoid, hipStream_t st);
int conv3x3_c1_bwd(int dtype, const void* x, const float* weight, long wsc, long wsk, const float* p, const float* dout, void* dx,
                   float* dw, float* db, float* ws, int N, int H, int W, int C, int sigmoid, int accumulate, hipStream_t st);
size_t binary_seg_stats_ws_floats(int B, size_t P);
int binary_seg_stats_fwd(const float* prob, const float* label, int B, size_t P, float* partial, float* stats, hipStream_t st);
int binary_seg_stats_bwd(const float* prob, const float* label, const float* gstats, int B, size_t P, float* dprob, hipStream_t st);
// matting.hip
size_t matting_ws_floats(int B, size_t P);
int trimap_stats_fwd(const float* gp, long sb, long sc, long sp, const float* trimap, int B, size_t P, float smooth, float* partial,
                     float* stats, hipStream_t st);
int trimap_stats_bwd(const float* gp, long sb, long sc, long sp, const float* trimap, const float* gstats, int B, size_t P,
                     float smooth, float* dgp, hipStream_t st);
int alpha_l1_fwd(const float* pred, const float* alpha, const float* trimap, int B, size_t P, float* partial, float* sums,
                 hipStream_t st);
int alpha_l1_bwd(const float* pred, const float* alpha, const float* trimap, const float* gsums, int B, size_t P, float* dpred,
                 hipStream_t st);
int composition_l1_fwd(const float* pred, const float* fg, const float* bg, const float* image, int B, size_t P, float* partial,
                       float* sums, hipStream_t st);
int composition_l1_bwd(const float* pred, const float* fg, const float* bg, const float* image, const float* gsums, int B, size_t P,
                       float* dpred, hipStream_t st);
int matting_fuse_fwd(const float* gp, long sb, long sc, long sp, const float* local, int B, size_t P, float* fused, hipStream_t st);
int matting_fuse_bwd(const float* gp, long sb, long sc, long sp, const float* dfused, int B, size_t P, float* dlocal, hipStream_t st);
size_t lap_level_ws_floats(int B, int h, int w);
int lap_level_fwd(const float* src, const float* alpha, const float* trimap, int level0, int B, int h, int w, const float* table,
                  float* next, float* partial, float* sum_e, float* sum_next, hipStream_t st);
int lap_level_bwd(const float* src, const float* alpha, const float* trimap, int level0, int B, int h, int w, const float* table,
                  const float* gnext, const float* topcur, const float* gs, const float* gtop, float* gcur, hipStream_t st);
// grouped forms (SAM matting): prediction rows (b, m), targets rows b; stats / gstats [B][M][8]
size_t group_matting_ws_floats(int B, int M, size_t P);
int group_matting_stats_fwd(int dtype, const void* gp, const void* lp, const void* fp, const float* alpha, const float* trimap,
                            const float* image, const float* fg, const float* bg, int B, int M, size_t P, float thr, float* partial,
                            float* stats, hipStream_t st);
int group_matting_stats_bwd(int dtype, const void* gp, const void* lp, const void* fp, const float* alpha, const float* trimap,
                            const float* image, const float* fg, const float* bg, const float* gstats, int B, int M, size_t P,
                            void* dgp, void* dlp, void* dfp, hipStream_t st);
int lap_level0_group_fwd(const float* src, const float* alpha, const float* trimap, int group, int R, int h, int w, const float* table,
                         float* next, float* partial, float* sum_e, hipStream_t st);
int lap_level_group_bwd(const float* src, const float* alpha, const float* trimap, int level0, int group, int R, int h, int w,
                        const float* table, const float* gnext, const float* topcur, const float* gs, const float* gtop,
                        const float* gall, int nsum, float* gcur, hipStream_t st);
// parsing.hip: form = 0 (by class count), 1 (lane per row, C <= 32), 2 (wavefront per row)
size_t pixel_class_terms_ws_floats(size_t rows);
int pixel_class_terms_lane_max_classes();
int pixel_class_terms_fwd(int dtype, const void* logits, const float* label, size_t rows, int C, int sigmoid, int form,
                          float* partial, float* terms, hipStream_t st);
int pixel_class_terms_bwd(int dtype, const void* logits, const float* label, const float* gterms, size_t rows, int C, int sigmoid,
                          int form, void* dlogits, hipStream_t st);
// lstm.hip: one bidirectional LSTM layer's recurrence.  gates [B * T][8H] fp32 in place (pre-activations in, activated gates out),
// whh [2][4H][H] / whhT [2][H][4H], y and dy [B][T][2H] and dgates [B * T][8H] in the compute dtype, c [B][T][2H] fp32
int lstm_fwd(int dtype, float* gates, const void* whh, void* y, float* c, int B, int T, int H, hipStream_t s);
int lstm_bwd(int dtype, const void* dy, const float* acts, const float* c, const void* whhT, void* dgates, int B, int T, int H,
             hipStream_t s);
// ctc.hip: strides in elements; targets / lengths int32 in device memory
size_t ctc_ws_floats(int T, int B, int S);
int ctc_loss_fwd(int dtype, const void* logits, long long st, long long sb, const int* targets, const int* in_len, const int* tg_len,
                 int T, int B, int S, int C, int blank, int focal, float gamma, float* ws, float* nll, float* loss, hipStream_t s);
int ctc_loss_bwd(int dtype, const void* logits, long long st, long long sb, void* dlogits, long long dst, long long dsb,
                 const int* in_len, const int* tg_len, const float* ws, const float* nll, const float* gout, int T, int B, int S, int C,
                 int focal, float gamma, hipStream_t s);
int ctc_greedy(int dtype, const void* logits, long long st, long long sb, const int* in_len, int T, int B, int C, int* index,
               float* prob, hipStream_t s);
// univseg.hip: the set loss of universal segmentation.  preds [B][Q][P] in dtype, targets [TT][P] fp32 packed over the batch,
// offsets [B + 1] int32 (device); sums = 3 planes [Q][TT] (P, N, S; column offsets[i] + t), then qsum [B][Q], then tsum [TT]
int univseg_chunk();
size_t univseg_pair_ws_floats(int B, int Q, int TT, size_t P);
int univseg_pair_sums(int dtype, const void* preds, const float* targets, const int* offsets, int B, int Q, int TT, int Tmax, size_t P,
                      float* partial, float* sums, hipStream_t st);
size_t univseg_matched_ws_floats(int M, size_t P);
int univseg_matched_fwd(int dtype, const void* preds, const float* targets, const int* rowx, const int* rowy, int M, size_t P,
                        float* partial, float* stats, hipStream_t st);
int univseg_matched_bwd(int dtype, const void* preds, const float* targets, const int* rowmap, const int* rowy, const float* gstats,
                        int R, size_t P, void* dpreds, hipStream_t st);
// attn_stream.hip: which = 0 forward, 1 dQ pass, 2 dK/dV pass; desc = const saicv_attn_desc*
int attention_stream(int dtype, int D, int which, const void* desc, hipStream_t st);

}  // namespace saicv
