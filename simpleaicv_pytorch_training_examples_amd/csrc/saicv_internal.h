// Internal C++ functions that another translation unit calls.  An entry point of include/saicv_hip.h is declared there and defined
// once, with C linkage, in the unit that owns it: the compiler checks the definition against the header.
#pragma once
#include <hip/hip_runtime.h>

struct saicv_conv_desc;      // include/saicv_hip.h
struct saicv_plan_query;
struct saicv_plan;

namespace saicv {

void set_error(const char* fmt, ...);
int check_launch(const char* what);
// the `void* stream` of the C ABI (an entry point with a parameter called S, which hides this, writes the cast out)
inline hipStream_t S(void* stream) { return static_cast<hipStream_t>(stream); }

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
int c3_bwd_stream(int M, int CO, int CI, const void* dz, const void* y, const void* mask, const float* coef, const void* x,
                  const void* wd, void* dx, float* dw, const EpiExtra* ex, int bs_rows, float* part_ws, hipStream_t st);
// stembwd.hip: BatchNorm-backward apply + weight gradient of the pooled space-to-depth stem as one stream (dy never stored).
// H, W: the convolution output
bool stem_bwd_stream_supported(int dtype, int N, int H, int W, int CO, int cq, int taps_r, int taps_s, int pk, int ps, int pp);
int stem_bwd_stream(const void* dout, const uint8_t* idx, const void* y, const float* gamma, const float* mean, const float* invstd,
                    const float* scale, const float* shift, const float* sums, const void* x, float* dw, float* dgamma, float* dbeta,
                    int accumulate, float* part_ws, int N, int H, int W, hipStream_t st);
// bn.hip: the finalize step of BatchNorm backward alone: `rows` rows of partial sums -> dgamma, dbeta and the coefficients
// ca, cb, cc of dy = ca * g + cb * y + cc at ws + 64 * C (ws: 67 * C floats)
int bn_bwd_coeffs(const float* part_g, const float* part_gx, int rows, int C, size_t M, const float* gamma, const float* mean,
                  const float* invstd, float* dgamma, float* dbeta, int accumulate, float* ws, hipStream_t st);
// tfm.hip: LayerNorm backward; saicv_layernorm_bwd and saicv_layernorm_bwd_scaled (with the three trailing arguments) share it
int layernorm_bwd(int dtype, const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                  const void* addend, void* dx, float* dgamma, float* dbeta, float* ws, int M, int C, int accumulate, hipStream_t st,
                  const float* out_scale = nullptr, int rows_per_scale = 1, void* dx_scaled = nullptr);

}  // namespace saicv
