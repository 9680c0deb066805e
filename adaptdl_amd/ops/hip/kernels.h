// Host ABI of the adaptdl_amd HIP extension: every function that
// bindings.cpp (host compiler) calls in gns_kernels.hip, bn_kernels.hip
// and conv_kernels.hip (hipcc).  Each .hip file includes this header too,
// so a definition that drifts from its declaration fails to compile
// instead of corrupting arguments at run time (C linkage: no mangling).
//
// Host-only declarations: no device code, nothing beyond the runtime API.

#pragma once

#include <hip/hip_runtime_api.h>

extern "C" {

// Element type of a gradient-statistics bucket.  16-bit buckets are
// passed as raw storage; the kernels convert per element.
enum StatDtype { STAT_F32 = 0, STAT_BF16 = 1, STAT_FP16 = 2 };

// ---- gns_kernels.hip -------------------------------------------------

void launch_sqsum(StatDtype dtype, const void* x, long n, double* out,
                  hipStream_t s);
void launch_scale_sqsum(StatDtype dtype, void* x, long n, float scale,
                        double* out, hipStream_t s);
void launch_sqsum_diff_update(StatDtype dtype, const void* cur, void* prev,
                              long n, double* out, hipStream_t s);
void launch_sqsum_avg(StatDtype dtype, const void* cur, const void* prev,
                      long n, double* out, hipStream_t s);
void launch_precond_sqsum(const float* g, const float* v, long n,
                          float inv_corr_sqrt, float eps, double* out,
                          hipStream_t s);
void launch_precond_sqsum_dev(const float* g, const float* v, long n,
                              const float* pc, double* out, hipStream_t s);
void launch_fused_sgd(float* p, const float* g, float* m, long n, float lr,
                      float momentum, float weight_decay, float dampening,
                      int nesterov, int has_momentum, hipStream_t s);
void launch_fused_adamw(float* p, const float* g, float* m, float* v,
                        long n, float lr, float beta1, float beta2,
                        float eps, float weight_decay, float bias1,
                        float bias2, int adam_mode, hipStream_t s);

// Master-weight forms: dtype (STAT_BF16 / STAT_FP16) is the element type
// of the low-precision operands p and g; master w, optimizer state and
// the Adam second moment v are fp32.
void launch_precond_sqsum_mw(StatDtype dtype, const void* g,
                             const float* v, long n, float inv_corr_sqrt,
                             float eps, double* out, hipStream_t s);
void launch_precond_sqsum_dev_mw(StatDtype dtype, const void* g,
                                 const float* v, long n, const float* pc,
                                 double* out, hipStream_t s);
void launch_fused_sgd_mw(StatDtype dtype, void* p, const void* g,
                         float* w, float* m, long n, float lr,
                         float momentum, float weight_decay,
                         float dampening, int nesterov, int has_momentum,
                         hipStream_t s);
void launch_fused_adamw_mw(StatDtype dtype, void* p, const void* g,
                           float* w, float* m, float* v, long n, float lr,
                           float beta1, float beta2, float eps,
                           float weight_decay, float bias1, float bias2,
                           int adam_mode, hipStream_t s);

// ---- bn_kernels.hip (bf16 NHWC as raw unsigned short) ----------------

// Rows of the stage-1 partials workspace (= stage-1 grid size) for M rows
// of C channels; ws holds 2 * C * bn_num_rblocks(M, C) floats.
long bn_num_rblocks(long m, int c);
// mask: nullable M*C/8-byte ReLU bitmask (relu + residual only), byte
// [row * (C/8) + slot], bit k = channel slot*8+k kept.  The forward writes
// it; the backward, given one, reads it instead of z (z may then be null).
// num_batches_tracked: nullable int64 scalar the training forward bumps.
void launch_bn_fwd(const unsigned short* x, const unsigned short* z,
                   unsigned short* y, long m, int c, const float* gamma,
                   const float* beta, float* running_mean,
                   float* running_var, float momentum, float eps,
                   int train, int relu, float* ws, float* save_mean,
                   float* save_rstd, float* scale, float* shift,
                   unsigned char* mask, long long* num_batches_tracked,
                   hipStream_t s);
void launch_bn_bwd(const unsigned short* x, const unsigned short* z,
                   const unsigned short* dy, unsigned short* dx,
                   unsigned short* dz, long m, int c, const float* gamma,
                   const float* save_mean, const float* save_rstd,
                   const float* scale, const float* shift, int train,
                   int relu, float* ws, float* dgamma, float* dbeta,
                   float* pqr, const unsigned char* mask, hipStream_t s);

// ---- conv_kernels.hip ------------------------------------------------

int conv3x3_wrw_params(int H, int W, int* P, int* Wp);
int conv3x3_wrw_supported(int H, int W, int C, int K);
int conv3x3_wrw_nsplit(int N, int H, int W, int C, int K);
void launch_conv3x3_wrw(const unsigned short* x, const unsigned short* dy,
                        float* ws, float* dw, int N, int H, int W, int C,
                        int K, hipStream_t s);
int conv3x3_mm_supported(int H, int W, int C, int K);
void launch_conv3x3_mm(const unsigned short* x, const unsigned short* w,
                       unsigned short* y, int N, int H, int W, int C,
                       int K, hipStream_t s);
int conv3x3_s2_fwd_supported(int H, int W, int C, int K);
void launch_conv3x3_s2_fwd(const unsigned short* x,
                           const unsigned short* w, unsigned short* y,
                           int N, int H, int W, int C, int K,
                           hipStream_t s);
int conv3x3_s2_bwd_supported(int Ho, int Wo, int K, int C);
void launch_conv3x3_s2_bwd(const unsigned short* dy,
                           const unsigned short* wt, unsigned short* dx,
                           int N, int Ho, int Wo, int K, int C,
                           hipStream_t s);
int conv3x3_s2_wrw_supported(int Ho, int Wo, int C, int K);
int conv3x3_s2_wrw_nsplit(int N, int Ho, int Wo, int C, int K);
void launch_conv3x3_s2_wrw(const unsigned short* x,
                           const unsigned short* dy, float* ws, float* dw,
                           int N, int Ho, int Wo, int C, int K,
                           hipStream_t s);
int conv3x3_s2_bwd_w8b_supported(int Ho, int Wo, int K, int C);
void launch_conv3x3_s2_bwd_w8b(const unsigned short* dy,
                               const unsigned short* wt,
                               unsigned short* dx, int N, int Ho, int K,
                               int C, hipStream_t s);

}  // extern "C"
