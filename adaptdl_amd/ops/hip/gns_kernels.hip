// CDNA4 (gfx950 / MI355X) kernels for the adaptdl_amd gradient hot path.
//
// These implement the fused operations of SURVEY.md §7 N1/N3: one
// bandwidth-bound pass over each flat gradient bucket computes the scale
// (gradient averaging) together with the fp64 sum-of-squares statistics
// that drive the gradient noise scale, replacing the reference's
// per-parameter `pow(2).sum(dtype=float64)` hook kernels
// (reference: adaptdl/torch/gradient_noise_scale.py:33-39,181-182) and
// `grad.div_(accum_count)` passes (:228).
//
// Design notes (see /opt/skills/guides/cdna_hip_programming.md):
// - wavefront = 64; block = 256 threads (4 waves); grid-stride loop capped
//   at ~2048 blocks (256 CU * 8 blocks) for memory-bound ops (Guideline 11)
// - ONE traversal (stat_pass) serves every statistics kernel: scalar head
//   up to 16-byte alignment, 16-byte vector body (16 B/lane; Guideline
//   13), scalar tail.  An element trait (F32 / BF16 / FP16) supplies the
//   storage type, the vector width and the conversions; a per-op functor
//   supplies the per-element math.  The kernels are thin extern "C"
//   wrappers, so their names stay stable for the profiles/ ledger.
// - two-operand kernels cast both pointers to vector pointers, which is
//   only valid when they are co-aligned (equal modulo 16 bytes; always
//   true for bucket-flat segments).  If they are not, that launch takes
//   the scalar loop for the whole range — a grid-uniform branch, since it
//   depends on kernel arguments only.
// - fp64 accumulation per thread -> wave __shfl_down reduce -> LDS partial
//   per wave -> one global fp64 atomicAdd per block (Guideline 12)
// - elementwise writes (scale / prev-copy) fused into the same pass so
//   gradient bytes are touched exactly once more than strictly necessary
// - master-weight kernels (*_mw_bf16 / *_mw_fp16: 16-bit gradient and
//   parameter, fp32 master and optimizer state) use sibling traversals
//   with the same head / 16-byte body / tail shape, pairing one 16-bit
//   vector with two fp32 vectors per lane

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include "kernels.h"

#define WAVE 64
#define BLOCK 256
#define MAX_BLOCKS 2048

__device__ __forceinline__ double wave_reduce_add(double v) {
    #pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        v += __shfl_down(v, off, WAVE);
    }
    return v;
}

// Block-level reduction: per-wave shuffle, LDS partials, lane-0 atomic.
__device__ __forceinline__ void block_reduce_atomic(double v, double* out) {
    __shared__ double partials[BLOCK / WAVE];
    v = wave_reduce_add(v);
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x / WAVE;
    if (lane == 0) partials[wid] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        #pragma unroll
        for (int i = 0; i < BLOCK / WAVE; ++i) s += partials[i];
        atomicAdd(out, s);
    }
}

// ---- element traits: storage type, 16-byte vector, conversions -------
// (bf16/fp16 buckets: true-low-precision-parameter models; the in-place
// ops round back with RNE.)

struct F32 {
    typedef float elem;
    typedef __attribute__((ext_vector_type(4))) float vec;
    static constexpr int W = 4;
    static __device__ __forceinline__ float to_f(float x) { return x; }
    static __device__ __forceinline__ float from_f(float f) { return f; }
};

struct BF16 {
    typedef unsigned short elem;
    typedef __attribute__((ext_vector_type(8))) unsigned short vec;
    static constexpr int W = 8;
    static __device__ __forceinline__ float to_f(unsigned short h) {
        union { float f; unsigned u; } c;
        c.u = ((unsigned)h) << 16;
        return c.f;
    }
    static __device__ __forceinline__ unsigned short from_f(float f) {
        __hip_bfloat16 h = __float2bfloat16(f);  // RNE
        return *reinterpret_cast<unsigned short*>(&h);
    }
};

struct FP16 {
    typedef unsigned short elem;
    typedef __attribute__((ext_vector_type(8))) unsigned short vec;
    static constexpr int W = 8;
    static __device__ __forceinline__ float to_f(unsigned short h) {
        return __half2float(*reinterpret_cast<const __half*>(&h));
    }
    static __device__ __forceinline__ unsigned short from_f(float f) {
        __half h = __float2half_rn(f);
        return *reinterpret_cast<unsigned short*>(&h);
    }
};

// ---- per-op functors -------------------------------------------------
// apply<T>(a, b) sees one stored element of each operand (b is unused by
// one-operand ops), returns its fp64 contribution and may rewrite the
// element named by `writes` (0 = a, 1 = b, -1 = read-only pass).

struct SqSum {  // sum(x^2)
    static constexpr int operands = 1, writes = -1;
    template <class T> __device__ __forceinline__ double apply(
            typename T::elem& x, typename T::elem&) const {
        double v = (double)T::to_f(x);
        return v * v;
    }
};

struct ScaleSqSum {  // x *= scale; sum(x^2)
    static constexpr int operands = 1, writes = 0;
    float scale;
    template <class T> __device__ __forceinline__ double apply(
            typename T::elem& x, typename T::elem&) const {
        float v = T::to_f(x) * scale;
        x = T::from_f(v);
        return (double)v * v;
    }
};

// sum((cur - prev)^2); prev = cur.  (accumulation microbatch stat)
struct SqSumDiffUpdate {
    static constexpr int operands = 2, writes = 1;
    template <class T> __device__ __forceinline__ double apply(
            typename T::elem& cur, typename T::elem& prev) const {
        double d = (double)T::to_f(cur) - (double)T::to_f(prev);
        prev = cur;
        return d * d;
    }
};

// sum(((cur + prev) / 2)^2)   (differenced single-sample estimator)
struct SqSumAvg {
    static constexpr int operands = 2, writes = -1;
    template <class T> __device__ __forceinline__ double apply(
            typename T::elem& cur, typename T::elem& prev) const {
        double a = 0.5 * ((double)T::to_f(cur) + (double)T::to_f(prev));
        return a * a;
    }
};

// sum((g / pinv)^2), pinv = sqrt(v) * inv_corr_sqrt + eps (Adam
// precondition; reference AdamGradientNoiseScale._calculate_preconditioner)
struct PrecondSqSum {
    static constexpr int operands = 2, writes = -1;
    float ics, eps;
    template <class T> __device__ __forceinline__ double apply(
            typename T::elem& g, typename T::elem& v) const {
        float pinv = sqrtf(T::to_f(v)) * ics + eps;
        double q = (double)(T::to_f(g) / pinv);
        return q * q;
    }
};

// ---- the traversal ---------------------------------------------------
// Grid-stride pass of functor F over n elements of a (and b): scalar head
// until a is 16-byte aligned, T::W-wide vector body, scalar tail, then one
// fp64 atomic per block into out.  A / B are T::elem or const T::elem; an
// operand is stored through only if F::writes names it.
template <class T, class F, class A, class B>
__device__ __forceinline__ void stat_pass(
        A* __restrict__ a, B* __restrict__ b, long n, const F f,
        double* __restrict__ out) {
    typedef typename T::elem E;
    typedef typename T::vec V;
    constexpr int W = T::W;
    double acc = 0.0;
    const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
    const long stride = (long)gridDim.x * BLOCK;

    auto scalar = [&](long j) {
        E ea = a[j], eb = E();
        if constexpr (F::operands == 2) eb = b[j];
        acc += f.template apply<T>(ea, eb);
        if constexpr (F::writes == 0) a[j] = ea;
        if constexpr (F::writes == 1) b[j] = eb;
    };

    long head = (16 - ((size_t)a & 15)) / sizeof(E) & (W - 1);
    if constexpr (F::operands == 2) {
        // Mis-coaligned operands: the whole range is "head" (scalar).
        if ((((size_t)a ^ (size_t)b) & 15) != 0) head = n;
    }
    if (head > n) head = n;
    for (long j = i; j < head; j += stride) scalar(j);

    const long nv = (n - head) / W;
    for (long j = i; j < nv; j += stride) {
        V va = ((const V*)(a + head))[j], vb = V();
        if constexpr (F::operands == 2) vb = ((const V*)(b + head))[j];
        #pragma unroll
        for (int k = 0; k < W; ++k) {
            E ea = va[k], eb = vb[k];
            acc += f.template apply<T>(ea, eb);
            va[k] = ea;
            vb[k] = eb;
        }
        if constexpr (F::writes == 0) ((V*)(a + head))[j] = va;
        if constexpr (F::writes == 1) ((V*)(b + head))[j] = vb;
    }

    for (long j = head + nv * W + i; j < n; j += stride) scalar(j);
    block_reduce_atomic(acc, out);
}

template <class T, class F, class A>
__device__ __forceinline__ void stat_pass(
        A* __restrict__ a, long n, const F f, double* __restrict__ out) {
    stat_pass<T>(a, (const typename T::elem*)nullptr, n, f, out);
}

// ---- statistics kernels (names are the profiles/ ledger keys) --------

#define STAT_KERNEL extern "C" __global__ __launch_bounds__(BLOCK) void

STAT_KERNEL k_sqsum(const float* __restrict__ x, long n,
                    double* __restrict__ out) {
    stat_pass<F32>(x, n, SqSum{}, out);
}
STAT_KERNEL k_sqsum_bf16(const unsigned short* __restrict__ x, long n,
                         double* __restrict__ out) {
    stat_pass<BF16>(x, n, SqSum{}, out);
}
STAT_KERNEL k_sqsum_fp16(const unsigned short* __restrict__ x, long n,
                         double* __restrict__ out) {
    stat_pass<FP16>(x, n, SqSum{}, out);
}

STAT_KERNEL k_scale_sqsum(float* __restrict__ x, long n, float scale,
                          double* __restrict__ out) {
    stat_pass<F32>(x, n, ScaleSqSum{scale}, out);
}
STAT_KERNEL k_scale_sqsum_bf16(unsigned short* __restrict__ x, long n,
                               float scale, double* __restrict__ out) {
    stat_pass<BF16>(x, n, ScaleSqSum{scale}, out);
}
STAT_KERNEL k_scale_sqsum_fp16(unsigned short* __restrict__ x, long n,
                               float scale, double* __restrict__ out) {
    stat_pass<FP16>(x, n, ScaleSqSum{scale}, out);
}

STAT_KERNEL k_sqsum_diff_update(const float* __restrict__ cur,
                                float* __restrict__ prev, long n,
                                double* __restrict__ out) {
    stat_pass<F32>(cur, prev, n, SqSumDiffUpdate{}, out);
}
STAT_KERNEL k_sqsum_diff_update_bf16(
        const unsigned short* __restrict__ cur,
        unsigned short* __restrict__ prev, long n,
        double* __restrict__ out) {
    stat_pass<BF16>(cur, prev, n, SqSumDiffUpdate{}, out);
}
STAT_KERNEL k_sqsum_diff_update_fp16(
        const unsigned short* __restrict__ cur,
        unsigned short* __restrict__ prev, long n,
        double* __restrict__ out) {
    stat_pass<FP16>(cur, prev, n, SqSumDiffUpdate{}, out);
}

STAT_KERNEL k_sqsum_avg(const float* __restrict__ cur,
                        const float* __restrict__ prev, long n,
                        double* __restrict__ out) {
    stat_pass<F32>(cur, prev, n, SqSumAvg{}, out);
}
STAT_KERNEL k_sqsum_avg_bf16(const unsigned short* __restrict__ cur,
                             const unsigned short* __restrict__ prev,
                             long n, double* __restrict__ out) {
    stat_pass<BF16>(cur, prev, n, SqSumAvg{}, out);
}
STAT_KERNEL k_sqsum_avg_fp16(const unsigned short* __restrict__ cur,
                             const unsigned short* __restrict__ prev,
                             long n, double* __restrict__ out) {
    stat_pass<FP16>(cur, prev, n, SqSumAvg{}, out);
}

STAT_KERNEL k_precond_sqsum(const float* __restrict__ g,
                            const float* __restrict__ v, long n,
                            float inv_corr_sqrt, float eps,
                            double* __restrict__ out) {
    stat_pass<F32>(g, v, n, PrecondSqSum{inv_corr_sqrt, eps}, out);
}

// hipGraph-capturable variant: the bias-correction scalars live in
// DEVICE memory (pc = {inv_corr_sqrt, eps, use_precond, unused}) so a
// captured graph picks up each step's values instead of baking them in.
// use_precond == 0 -> identity preconditioner (warmup steps).
STAT_KERNEL k_precond_sqsum_dev(const float* __restrict__ g,
                                const float* __restrict__ v, long n,
                                const float* __restrict__ pc,
                                double* __restrict__ out) {
    if (pc[2] != 0.f)
        stat_pass<F32>(g, v, n, PrecondSqSum{pc[0], pc[1]}, out);
    else
        stat_pass<F32>(g, n, SqSum{}, out);
}

// ---- preconditioned statistic on master-weight buckets ---------------
// PrecondSqSum with g in the bucket dtype (bf16/fp16) and v in fp32 (the
// fused master-weight Adam keeps its moments in fp32).  A sibling of
// stat_pass rather than a second-operand trait on it, so the single-
// dtype instantiations above stay exactly the kernels they were.  One
// 16-byte vector of g (8 elements) pairs with two 16-byte vectors of v;
// the head aligns g, and v + head must then be 16-byte aligned as well
// (true whenever both carry the same element offset), else the launch
// takes the scalar loop — a grid-uniform branch on kernel arguments.
template <class T>
__device__ __forceinline__ void precond_pass_mw(
        const typename T::elem* __restrict__ g, const float* __restrict__ v,
        long n, const PrecondSqSum f, double* __restrict__ out) {
    typedef typename T::elem E;
    typedef typename T::vec V;
    typedef F32::vec V4;
    constexpr int W = T::W;
    static_assert(W == 2 * F32::W, "one g vector pairs with two v vectors");
    double acc = 0.0;
    const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
    const long stride = (long)gridDim.x * BLOCK;

    auto scalar = [&](long j) {
        float pinv = sqrtf(v[j]) * f.ics + f.eps;
        double q = (double)(T::to_f(g[j]) / pinv);
        acc += q * q;
    };

    long head = (16 - ((size_t)g & 15)) / sizeof(E) & (W - 1);
    if (((size_t)(v + head) & 15) != 0) head = n;
    if (head > n) head = n;
    for (long j = i; j < head; j += stride) scalar(j);

    const long nv = (n - head) / W;
    for (long j = i; j < nv; j += stride) {
        const V vg = ((const V*)(g + head))[j];
        const V4 v0 = ((const V4*)(v + head))[2 * j];
        const V4 v1 = ((const V4*)(v + head))[2 * j + 1];
        #pragma unroll
        for (int k = 0; k < W; ++k) {
            float vk = k < F32::W ? v0[k & 3] : v1[k & 3];
            float pinv = sqrtf(vk) * f.ics + f.eps;
            E eg = vg[k];
            double q = (double)(T::to_f(eg) / pinv);
            acc += q * q;
        }
    }

    for (long j = head + nv * W + i; j < n; j += stride) scalar(j);
    block_reduce_atomic(acc, out);
}

STAT_KERNEL k_precond_sqsum_mw_bf16(const unsigned short* __restrict__ g,
                                    const float* __restrict__ v, long n,
                                    float inv_corr_sqrt, float eps,
                                    double* __restrict__ out) {
    precond_pass_mw<BF16>(g, v, n, PrecondSqSum{inv_corr_sqrt, eps}, out);
}
STAT_KERNEL k_precond_sqsum_mw_fp16(const unsigned short* __restrict__ g,
                                    const float* __restrict__ v, long n,
                                    float inv_corr_sqrt, float eps,
                                    double* __restrict__ out) {
    precond_pass_mw<FP16>(g, v, n, PrecondSqSum{inv_corr_sqrt, eps}, out);
}

// Device-scalar forms (see k_precond_sqsum_dev): plain sqsum of g when
// use_precond == 0.
STAT_KERNEL k_precond_sqsum_dev_mw_bf16(
        const unsigned short* __restrict__ g, const float* __restrict__ v,
        long n, const float* __restrict__ pc, double* __restrict__ out) {
    if (pc[2] != 0.f)
        precond_pass_mw<BF16>(g, v, n, PrecondSqSum{pc[0], pc[1]}, out);
    else
        stat_pass<BF16>(g, n, SqSum{}, out);
}
STAT_KERNEL k_precond_sqsum_dev_mw_fp16(
        const unsigned short* __restrict__ g, const float* __restrict__ v,
        long n, const float* __restrict__ pc, double* __restrict__ out) {
    if (pc[2] != 0.f)
        precond_pass_mw<FP16>(g, v, n, PrecondSqSum{pc[0], pc[1]}, out);
    else
        stat_pass<FP16>(g, n, SqSum{}, out);
}

// ---- fused flat-bucket optimizers -----------------------------------

// SGD with momentum on one flat bucket (param/grad/momentum share layout).
extern "C" __global__ __launch_bounds__(BLOCK) void k_fused_sgd(
        float* __restrict__ p, const float* __restrict__ g,
        float* __restrict__ m, long n, float lr, float momentum,
        float weight_decay, float dampening, int nesterov, int has_momentum) {
    long i = (long)blockIdx.x * BLOCK + threadIdx.x;
    const long stride = (long)gridDim.x * BLOCK;
    for (long j = i; j < n; j += stride) {
        float dp = g[j];
        float pj = p[j];
        if (weight_decay != 0.f) dp = fmaf(weight_decay, pj, dp);
        if (has_momentum) {
            float mj = fmaf(momentum, m[j], (1.f - dampening) * dp);
            m[j] = mj;
            dp = nesterov ? fmaf(momentum, mj, dp) : mj;
        }
        p[j] = fmaf(-lr, dp, pj);
    }
}

// Adam / AdamW on one flat bucket.
extern "C" __global__ __launch_bounds__(BLOCK) void k_fused_adamw(
        float* __restrict__ p, const float* __restrict__ g,
        float* __restrict__ m, float* __restrict__ v, long n, float lr,
        float beta1, float beta2, float eps, float weight_decay,
        float bias1, float bias2, int adam_mode) {
    long i = (long)blockIdx.x * BLOCK + threadIdx.x;
    const long stride = (long)gridDim.x * BLOCK;
    const float step_size = lr / bias1;
    const float inv_bias2_sqrt = rsqrtf(bias2);
    for (long j = i; j < n; j += stride) {
        float gj = g[j];
        float pj = p[j];
        if (adam_mode && weight_decay != 0.f) gj = fmaf(weight_decay, pj, gj);
        else if (!adam_mode && weight_decay != 0.f)
            pj *= (1.f - lr * weight_decay);
        float mj = fmaf(beta1, m[j], (1.f - beta1) * gj);
        float vj = fmaf(beta2, v[j], (1.f - beta2) * gj * gj);
        m[j] = mj;
        v[j] = vj;
        float denom = sqrtf(vj) * inv_bias2_sqrt + eps;
        p[j] = fmaf(-step_size, mj / denom, pj);
    }
}

// ---- fused optimizers with fp32 master weights (bf16/fp16 buckets) ---
// The bucket's parameters and gradients are bf16/fp16; the weight the
// optimizer integrates is an fp32 master, and the state is fp32.  One
// pass reads g (low precision), the master and the state, does the
// update in fp32 with the math of k_fused_sgd / k_fused_adamw, and
// writes master, state and p = T::from_f(master) (RNE).  p is write-only:
// the master is the only source of the weight.
//
// update<S>(g, w, s0, s1) of a functor rewrites the master w and its S
// fp32 state elements in place.

template <bool HAS_MOMENTUM>
struct SgdUpdate {
    static constexpr int states = HAS_MOMENTUM ? 1 : 0;
    float lr, momentum, weight_decay, dampening;
    int nesterov;
    __device__ __forceinline__ void update(float dp, float& w, float& m,
                                           float&) const {
        if (weight_decay != 0.f) dp = fmaf(weight_decay, w, dp);
        if (HAS_MOMENTUM) {
            m = fmaf(momentum, m, (1.f - dampening) * dp);
            dp = nesterov ? fmaf(momentum, m, dp) : m;
        }
        w = fmaf(-lr, dp, w);
    }
};

struct AdamUpdate {
    static constexpr int states = 2;
    float lr, beta1, beta2, eps, weight_decay, step_size, inv_bias2_sqrt;
    int adam_mode;
    __device__ __forceinline__ void update(float g, float& w, float& m,
                                           float& v) const {
        if (adam_mode && weight_decay != 0.f) g = fmaf(weight_decay, w, g);
        else if (!adam_mode && weight_decay != 0.f)
            w *= (1.f - lr * weight_decay);
        m = fmaf(beta1, m, (1.f - beta1) * g);
        v = fmaf(beta2, v, (1.f - beta2) * g * g);
        float denom = sqrtf(v) * inv_bias2_sqrt + eps;
        w = fmaf(-step_size, m / denom, w);
    }
};

// The parameter is the STORED master rounded to 16 bits.  Left alone,
// the compiler folds the update's last fma and the conversion into one
// v_fma_mix{lo,hi}_f16, which rounds the exact sum once and so differs
// from RNE(fp32 master) in the double-rounding cases.  Passing the
// master through an empty asm keeps the fp32 rounding in between.
__device__ __forceinline__ float as_stored(float x) {
    asm("" : "+v"(x));
    return x;
}

// Grid-stride pass of update functor F over n elements.  The low-
// precision streams move one 16-byte vector (8 elements) per lane, each
// fp32 stream two; scalar head until p is 16-byte aligned, scalar tail.
// Every operand must be 16-byte aligned after the head (true whenever
// all carry the same element offset into 16-byte-aligned buffers);
// otherwise the whole launch takes the scalar loop — grid-uniform, as it
// depends on kernel arguments only.  s0 / s1 are dereferenced only for
// the first F::states of them.
template <class T, class F>
__device__ __forceinline__ void update_pass_mw(
        typename T::elem* __restrict__ p,
        const typename T::elem* __restrict__ g, float* __restrict__ w,
        float* __restrict__ s0, float* __restrict__ s1, long n, const F f) {
    typedef typename T::elem E;
    typedef typename T::vec V;
    typedef F32::vec V4;
    constexpr int W = T::W, S = F::states;
    static_assert(W == 2 * F32::W, "one 16-bit vector pairs with two fp32");
    const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
    const long stride = (long)gridDim.x * BLOCK;

    auto scalar = [&](long j) {
        float wj = w[j], a = 0.f, b = 0.f;
        if constexpr (S >= 1) a = s0[j];
        if constexpr (S >= 2) b = s1[j];
        f.update(T::to_f(g[j]), wj, a, b);
        wj = as_stored(wj);
        w[j] = wj;
        if constexpr (S >= 1) s0[j] = a;
        if constexpr (S >= 2) s1[j] = b;
        p[j] = T::from_f(wj);
    };

    long head = (16 - ((size_t)p & 15)) / sizeof(E) & (W - 1);
    size_t mis = (size_t)(g + head) | (size_t)(w + head);
    if constexpr (S >= 1) mis |= (size_t)(s0 + head);
    if constexpr (S >= 2) mis |= (size_t)(s1 + head);
    if ((mis & 15) != 0) head = n;
    if (head > n) head = n;
    for (long j = i; j < head; j += stride) scalar(j);

    const long nv = (n - head) / W;
    for (long j = i; j < nv; j += stride) {
        const V vg = ((const V*)(g + head))[j];
        V4 vw[2], va[2] = {V4(), V4()}, vb[2] = {V4(), V4()};
        #pragma unroll
        for (int h = 0; h < 2; ++h) {
            vw[h] = ((const V4*)(w + head))[2 * j + h];
            if constexpr (S >= 1) va[h] = ((const V4*)(s0 + head))[2 * j + h];
            if constexpr (S >= 2) vb[h] = ((const V4*)(s1 + head))[2 * j + h];
        }
        V vp;
        #pragma unroll
        for (int k = 0; k < W; ++k) {
            E eg = vg[k];
            float wk = vw[k / 4][k % 4], a = va[k / 4][k % 4],
                  b = vb[k / 4][k % 4];
            f.update(T::to_f(eg), wk, a, b);
            wk = as_stored(wk);
            vw[k / 4][k % 4] = wk;
            va[k / 4][k % 4] = a;
            vb[k / 4][k % 4] = b;
            vp[k] = T::from_f(wk);
        }
        #pragma unroll
        for (int h = 0; h < 2; ++h) {
            ((V4*)(w + head))[2 * j + h] = vw[h];
            if constexpr (S >= 1) ((V4*)(s0 + head))[2 * j + h] = va[h];
            if constexpr (S >= 2) ((V4*)(s1 + head))[2 * j + h] = vb[h];
        }
        ((V*)(p + head))[j] = vp;
    }

    for (long j = head + nv * W + i; j < n; j += stride) scalar(j);
}

#define UPDATE_KERNEL extern "C" __global__ __launch_bounds__(BLOCK) void

template <class T>
__device__ __forceinline__ void fused_sgd_mw(
        typename T::elem* p, const typename T::elem* g, float* w, float* m,
        long n, float lr, float momentum, float weight_decay,
        float dampening, int nesterov, int has_momentum) {
    if (has_momentum)
        update_pass_mw<T>(p, g, w, m, (float*)nullptr, n,
                          SgdUpdate<true>{lr, momentum, weight_decay,
                                          dampening, nesterov});
    else
        update_pass_mw<T>(p, g, w, (float*)nullptr, (float*)nullptr, n,
                          SgdUpdate<false>{lr, momentum, weight_decay,
                                           dampening, nesterov});
}

UPDATE_KERNEL k_fused_sgd_mw_bf16(
        unsigned short* __restrict__ p, const unsigned short* __restrict__ g,
        float* __restrict__ w, float* __restrict__ m, long n, float lr,
        float momentum, float weight_decay, float dampening, int nesterov,
        int has_momentum) {
    fused_sgd_mw<BF16>(p, g, w, m, n, lr, momentum, weight_decay, dampening,
                       nesterov, has_momentum);
}
UPDATE_KERNEL k_fused_sgd_mw_fp16(
        unsigned short* __restrict__ p, const unsigned short* __restrict__ g,
        float* __restrict__ w, float* __restrict__ m, long n, float lr,
        float momentum, float weight_decay, float dampening, int nesterov,
        int has_momentum) {
    fused_sgd_mw<FP16>(p, g, w, m, n, lr, momentum, weight_decay, dampening,
                       nesterov, has_momentum);
}

UPDATE_KERNEL k_fused_adamw_mw_bf16(
        unsigned short* __restrict__ p, const unsigned short* __restrict__ g,
        float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
        long n, float lr, float beta1, float beta2, float eps,
        float weight_decay, float bias1, float bias2, int adam_mode) {
    update_pass_mw<BF16>(p, g, w, m, v, n,
                         AdamUpdate{lr, beta1, beta2, eps, weight_decay,
                                    lr / bias1, rsqrtf(bias2), adam_mode});
}
UPDATE_KERNEL k_fused_adamw_mw_fp16(
        unsigned short* __restrict__ p, const unsigned short* __restrict__ g,
        float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
        long n, float lr, float beta1, float beta2, float eps,
        float weight_decay, float bias1, float bias2, int adam_mode) {
    update_pass_mw<FP16>(p, g, w, m, v, n,
                         AdamUpdate{lr, beta1, beta2, eps, weight_decay,
                                    lr / bias1, rsqrtf(bias2), adam_mode});
}

// ---- host-side launchers (called from bindings.cpp, which is compiled
// by the host compiler and cannot launch kernels itself) ---------------

static inline dim3 grid_for(long n) {
    long blocks = (n + BLOCK - 1) / BLOCK;
    if (blocks > MAX_BLOCKS) blocks = MAX_BLOCKS;
    if (blocks < 1) blocks = 1;
    return dim3((unsigned)blocks);
}

// One launch of kernel K over n elements on stream s.
template <class K, class... Args>
static inline void launch(K kernel, long n, hipStream_t s, Args... args) {
    hipLaunchKernelGGL(kernel, grid_for(n), dim3(BLOCK), 0, s, args...);
}

typedef unsigned short u16;

extern "C" void launch_sqsum(StatDtype dtype, const void* x, long n, double* out,
                  hipStream_t s) {
    switch (dtype) {
    case STAT_F32: launch(k_sqsum, n, s, (const float*)x, n, out); break;
    case STAT_BF16: launch(k_sqsum_bf16, n, s, (const u16*)x, n, out); break;
    case STAT_FP16: launch(k_sqsum_fp16, n, s, (const u16*)x, n, out); break;
    }
}

extern "C" void launch_scale_sqsum(StatDtype dtype, void* x, long n, float scale,
                        double* out, hipStream_t s) {
    switch (dtype) {
    case STAT_F32:
        launch(k_scale_sqsum, n, s, (float*)x, n, scale, out); break;
    case STAT_BF16:
        launch(k_scale_sqsum_bf16, n, s, (u16*)x, n, scale, out); break;
    case STAT_FP16:
        launch(k_scale_sqsum_fp16, n, s, (u16*)x, n, scale, out); break;
    }
}

extern "C" void launch_sqsum_diff_update(StatDtype dtype, const void* cur, void* prev,
                              long n, double* out, hipStream_t s) {
    switch (dtype) {
    case STAT_F32:
        launch(k_sqsum_diff_update, n, s, (const float*)cur, (float*)prev,
               n, out);
        break;
    case STAT_BF16:
        launch(k_sqsum_diff_update_bf16, n, s, (const u16*)cur, (u16*)prev,
               n, out);
        break;
    case STAT_FP16:
        launch(k_sqsum_diff_update_fp16, n, s, (const u16*)cur, (u16*)prev,
               n, out);
        break;
    }
}

extern "C" void launch_sqsum_avg(StatDtype dtype, const void* cur, const void* prev,
                      long n, double* out, hipStream_t s) {
    switch (dtype) {
    case STAT_F32:
        launch(k_sqsum_avg, n, s, (const float*)cur, (const float*)prev, n,
               out);
        break;
    case STAT_BF16:
        launch(k_sqsum_avg_bf16, n, s, (const u16*)cur, (const u16*)prev, n,
               out);
        break;
    case STAT_FP16:
        launch(k_sqsum_avg_fp16, n, s, (const u16*)cur, (const u16*)prev, n,
               out);
        break;
    }
}

extern "C" void launch_precond_sqsum(const float* g, const float* v, long n,
                          float inv_corr_sqrt, float eps, double* out,
                          hipStream_t s) {
    launch(k_precond_sqsum, n, s, g, v, n, inv_corr_sqrt, eps, out);
}

extern "C" void launch_precond_sqsum_dev(const float* g, const float* v, long n,
                              const float* pc, double* out, hipStream_t s) {
    launch(k_precond_sqsum_dev, n, s, g, v, n, pc, out);
}

// dtype names the 16-bit element type of g (STAT_BF16 / STAT_FP16; the
// bindings send an all-fp32 call to the launchers above instead).
extern "C" void launch_precond_sqsum_mw(StatDtype dtype, const void* g,
                             const float* v, long n, float inv_corr_sqrt,
                             float eps, double* out, hipStream_t s) {
    switch (dtype) {
    case STAT_BF16:
        launch(k_precond_sqsum_mw_bf16, n, s, (const u16*)g, v, n,
               inv_corr_sqrt, eps, out);
        break;
    case STAT_FP16:
        launch(k_precond_sqsum_mw_fp16, n, s, (const u16*)g, v, n,
               inv_corr_sqrt, eps, out);
        break;
    case STAT_F32: break;
    }
}

extern "C" void launch_precond_sqsum_dev_mw(StatDtype dtype, const void* g,
                                 const float* v, long n, const float* pc,
                                 double* out, hipStream_t s) {
    switch (dtype) {
    case STAT_BF16:
        launch(k_precond_sqsum_dev_mw_bf16, n, s, (const u16*)g, v, n, pc,
               out);
        break;
    case STAT_FP16:
        launch(k_precond_sqsum_dev_mw_fp16, n, s, (const u16*)g, v, n, pc,
               out);
        break;
    case STAT_F32: break;
    }
}

extern "C" void launch_fused_sgd_mw(StatDtype dtype, void* p, const void* g,
                         float* w, float* m, long n, float lr,
                         float momentum, float weight_decay,
                         float dampening, int nesterov, int has_momentum,
                         hipStream_t s) {
    switch (dtype) {
    case STAT_BF16:
        launch(k_fused_sgd_mw_bf16, n, s, (u16*)p, (const u16*)g, w, m, n,
               lr, momentum, weight_decay, dampening, nesterov,
               has_momentum);
        break;
    case STAT_FP16:
        launch(k_fused_sgd_mw_fp16, n, s, (u16*)p, (const u16*)g, w, m, n,
               lr, momentum, weight_decay, dampening, nesterov,
               has_momentum);
        break;
    case STAT_F32: break;
    }
}

extern "C" void launch_fused_adamw_mw(StatDtype dtype, void* p, const void* g,
                           float* w, float* m, float* v, long n, float lr,
                           float beta1, float beta2, float eps,
                           float weight_decay, float bias1, float bias2,
                           int adam_mode, hipStream_t s) {
    switch (dtype) {
    case STAT_BF16:
        launch(k_fused_adamw_mw_bf16, n, s, (u16*)p, (const u16*)g, w, m, v,
               n, lr, beta1, beta2, eps, weight_decay, bias1, bias2,
               adam_mode);
        break;
    case STAT_FP16:
        launch(k_fused_adamw_mw_fp16, n, s, (u16*)p, (const u16*)g, w, m, v,
               n, lr, beta1, beta2, eps, weight_decay, bias1, bias2,
               adam_mode);
        break;
    case STAT_F32: break;
    }
}

extern "C" void launch_fused_sgd(float* p, const float* g, float* m, long n, float lr,
                      float momentum, float weight_decay, float dampening,
                      int nesterov, int has_momentum, hipStream_t s) {
    launch(k_fused_sgd, n, s, p, g, m, n, lr, momentum, weight_decay,
           dampening, nesterov, has_momentum);
}

extern "C" void launch_fused_adamw(float* p, const float* g, float* m, float* v,
                        long n, float lr, float beta1, float beta2,
                        float eps, float weight_decay, float bias1,
                        float bias2, int adam_mode, hipStream_t s) {
    launch(k_fused_adamw, n, s, p, g, m, v, n, lr, beta1, beta2, eps,
           weight_decay, bias1, bias2, adam_mode);
}
