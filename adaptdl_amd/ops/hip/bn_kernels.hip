// CDNA4 (gfx950 / MI355X) fused NHWC BatchNorm(+ReLU) training kernels.
//
// Replaces MIOpen's spatial batchnorm for channels_last bf16 conv nets:
// rocprof on ResNet-18/CIFAR (profiles/bench_r02_channels_last_kernel_
// stats.csv) shows MIOpen's NHWC BN at 56% of total kernel time, ~10x off
// the HBM3E bandwidth bound.  These kernels are plain bandwidth-bound
// passes designed per /opt/skills/guides/cdna_hip_programming.md
// (Guidelines 11-13, App. B):
//   - bf16 loads/stores vectorized 8-wide (16 B/lane); a wave's 64 lanes
//     cover whole consecutive NHWC rows, so global access is one
//     contiguous 1 KiB span per wave instruction,
//   - every thread owns a FIXED channel octet (slot); per-channel
//     parameters are loaded into registers once, outside the row loop,
//   - reductions are two-stage: per-block partials to a workspace (NO
//     cross-block atomics — v1 used one atomicAdd per (block, channel)
//     and measured 432 us vs the 20 us bandwidth-bound apply pass, pure
//     atomic serialization), then a parallel per-channel block reduce,
//   - ReLU and its backward mask are folded in, so no separate
//     threshold/clamp kernels run.  Without a residual the mask is
//     recomputed from x (read anyway, no extra stream); with a residual
//     the forward apply stores it as one bit per element so the backward
//     does not re-read z,
//   - the per-channel tail of each direction (workspace row sums +
//     finalize math + the num_batches_tracked increment) is ONE kernel.
//
// Layout contract: x is NHWC ("channels_last") bf16 with C % 8 == 0 and
// C/8 <= 256; per-channel parameters fp32.  M = N*H*W rows.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include "kernels.h"

#define WAVE 64
#define BLOCK 256
#define MAX_RBLOCKS 1024   // stage-1 reduction grid cap (partials rows)
#define MAX_BLOCKS 2048
#define VEC 8

typedef unsigned short ushort_t;

union Vec8 {
    float4 f4;
    ushort_t u[VEC];
};

__device__ __forceinline__ float b2f(ushort_t h) {
    union { float f; unsigned u; } c;
    c.u = ((unsigned)h) << 16;
    return c.f;
}

__device__ __forceinline__ ushort_t f2b(float f) {
    __hip_bfloat16 h = __float2bfloat16(f);  // RNE
    return *reinterpret_cast<ushort_t*>(&h);
}

// Shared LDS tree over the row-group dimension for VEC per-thread values.
// tid = rg * slots + slot; reduces rg in [0, rpb) down to rg == 0.
__device__ __forceinline__ void rg_tree_reduce(
        float (&s)[VEC], float* lds, int slots, int rpb, int rg) {
    int p2 = 1;
    while (p2 * 2 <= rpb) p2 *= 2;
    #pragma unroll
    for (int k = 0; k < VEC; ++k) lds[threadIdx.x * VEC + k] = s[k];
    __syncthreads();
    if (rg < p2 && rg + p2 < rpb) {
        #pragma unroll
        for (int k = 0; k < VEC; ++k)
            s[k] += lds[(threadIdx.x + p2 * slots) * VEC + k];
    }
    for (int r = p2 / 2; r > 0; r >>= 1) {
        if (rg < p2) {
            #pragma unroll
            for (int k = 0; k < VEC; ++k) lds[threadIdx.x * VEC + k] = s[k];
        }
        __syncthreads();
        if (rg < r) {
            #pragma unroll
            for (int k = 0; k < VEC; ++k)
                s[k] += lds[(threadIdx.x + r * slots) * VEC + k];
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------
// Stage-1 forward reduction: per-block partial (sum, sumsq) per channel.
// ws layout: ws[c * nb + block] (c in [0, C) sums, [C, 2C) sum-squares)
// so the stage-2 per-channel reduce reads contiguously.
// ---------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(BLOCK) void k_bn_fwd_reduce(
        const ushort_t* __restrict__ x, long m, int c, int nb,
        float* __restrict__ ws) {
    const int slots = c / VEC;
    const int rpb = BLOCK / slots > 0 ? BLOCK / slots : 1;
    const int slot = threadIdx.x % slots;
    const int rg = threadIdx.x / slots;
    __shared__ float lds[BLOCK * VEC];

    float s[VEC], s2[VEC];
    #pragma unroll
    for (int k = 0; k < VEC; ++k) { s[k] = 0.f; s2[k] = 0.f; }

    if (rg < rpb) {
        const ushort_t* base = x + (size_t)slot * VEC;
        for (long row = (long)blockIdx.x * rpb + rg; row < m;
                row += (long)gridDim.x * rpb) {
            Vec8 v;
            v.f4 = *reinterpret_cast<const float4*>(base + (size_t)row * c);
            #pragma unroll
            for (int k = 0; k < VEC; ++k) {
                float f = b2f(v.u[k]);
                s[k] += f;
                s2[k] = fmaf(f, f, s2[k]);
            }
        }
    }
    rg_tree_reduce(s, lds, slots, rpb, rg);
    if (rg == 0) {
        #pragma unroll
        for (int k = 0; k < VEC; ++k)
            ws[(size_t)(slot * VEC + k) * nb + blockIdx.x] = s[k];
    }
    __syncthreads();
    rg_tree_reduce(s2, lds, slots, rpb, rg);
    if (rg == 0) {
        #pragma unroll
        for (int k = 0; k < VEC; ++k)
            ws[(size_t)(c + slot * VEC + k) * nb + blockIdx.x] = s2[k];
    }
}

// ---------------------------------------------------------------------
// Stage-2 row sums for the tail kernels: block `ch` sums its two
// workspace rows (ws[ch * nb ..] and ws[(c + ch) * nb ..]).  Strided
// per-thread sum, wave shuffle tree, then the block's 4 wave partials in
// index order.  Both totals are valid in thread 0 only.
//
// nb <= MAX_RBLOCKS = WS_TRIPS * BLOCK, so a thread owns at most WS_TRIPS
// elements of each row: all 2 * WS_TRIPS loads issue up front (one memory
// round trip instead of one per trip and row), then add in index order.
// ---------------------------------------------------------------------
#define WS_TRIPS (MAX_RBLOCKS / BLOCK)
static_assert(WS_TRIPS * BLOCK == MAX_RBLOCKS, "row-sum trips cover a row");

__device__ __forceinline__ void ws_row_pair_sum(
        const float* __restrict__ ws, int nb, int c, int ch, float* lds,
        float& t0, float& t1) {
    const float* row0 = ws + (size_t)ch * nb;
    const float* row1 = ws + (size_t)(c + ch) * nb;
    float a[WS_TRIPS], b[WS_TRIPS];
    #pragma unroll
    for (int j = 0; j < WS_TRIPS; ++j) {
        // clamped, so the loads are unconditional; the adds are guarded
        const int i = min((int)threadIdx.x + j * BLOCK, nb - 1);
        a[j] = row0[i];
        b[j] = row1[i];
    }
    float s0 = 0.f, s1 = 0.f;
    #pragma unroll
    for (int j = 0; j < WS_TRIPS; ++j) {
        if ((int)threadIdx.x + j * BLOCK < nb) { s0 += a[j]; s1 += b[j]; }
    }
    #pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        s0 += __shfl_down(s0, off, WAVE);
        s1 += __shfl_down(s1, off, WAVE);
    }
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x / WAVE;
    if (lane == 0) {
        lds[wid] = s0;
        lds[BLOCK / WAVE + wid] = s1;
    }
    __syncthreads();
    t0 = 0.f; t1 = 0.f;
    if (threadIdx.x == 0) {
        #pragma unroll
        for (int i = 0; i < BLOCK / WAVE; ++i) t0 += lds[i];
        #pragma unroll
        for (int i = 0; i < BLOCK / WAVE; ++i) t1 += lds[BLOCK / WAVE + i];
    }
}

// ---------------------------------------------------------------------
// Forward tail (C blocks): row sums, then one thread per channel does
// statistics + affine fold + running stats.  Block 0 also bumps
// num_batches_tracked when the module tracks it (nullable).
// ---------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(BLOCK) void k_bn_fwd_tail(
        const float* __restrict__ ws, int nb, long m, int c,
        const float* __restrict__ gamma, const float* __restrict__ beta,
        float* __restrict__ running_mean, float* __restrict__ running_var,
        float momentum, float eps,
        float* __restrict__ save_mean, float* __restrict__ save_rstd,
        float* __restrict__ scale, float* __restrict__ shift,
        long long* __restrict__ num_batches_tracked) {
    __shared__ float lds[2 * BLOCK / WAVE];
    const int i = blockIdx.x;
    // per-channel inputs first, so their latency hides under the row sums
    const float g = gamma[i], b = beta[i];
    const float rm = running_mean ? running_mean[i] : 0.f;
    const float rv = running_mean ? running_var[i] : 0.f;
    float sum, sumsq;
    ws_row_pair_sum(ws, nb, c, i, lds, sum, sumsq);
    // Rounding is pinned: no implicit contraction, and an explicit fmaf
    // exactly where the former C-thread finalize kernel fused (shift and
    // the running-statistics updates; the variance stays mul, mul, sub),
    // so the statistics do not move with the compiler's choices here.
    if (threadIdx.x == 0) {
        #pragma clang fp contract(off)
        float inv_m = 1.0f / (float)m;
        float mean = sum * inv_m;
        float var = sumsq * inv_m - mean * mean;
        var = var > 0.f ? var : 0.f;
        float rstd = rsqrtf(var + eps);
        save_mean[i] = mean;
        save_rstd[i] = rstd;
        float sc = g * rstd;
        scale[i] = sc;
        shift[i] = fmaf(-mean, sc, b);
        if (running_mean != nullptr) {
            float unbiased = m > 1 ? var * (float)m / (float)(m - 1) : var;
            running_mean[i] = fmaf(momentum, mean - rm, rm);
            running_var[i] = fmaf(momentum, unbiased - rv, rv);
        }
        if (i == 0 && num_batches_tracked != nullptr)
            *num_batches_tracked += 1;
    }
}

// Eval-mode finalize: fold running statistics into scale/shift.
extern "C" __global__ void k_bn_eval_finalize(
        int c, const float* __restrict__ gamma,
        const float* __restrict__ beta,
        const float* __restrict__ running_mean,
        const float* __restrict__ running_var, float eps,
        float* __restrict__ save_mean, float* __restrict__ save_rstd,
        float* __restrict__ scale, float* __restrict__ shift) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c) return;
    float mean = running_mean[i];
    float rstd = rsqrtf(running_var[i] + eps);
    save_mean[i] = mean;
    save_rstd[i] = rstd;
    float sc = gamma[i] * rstd;
    scale[i] = sc;
    shift[i] = beta[i] - mean * sc;
}

// ---------------------------------------------------------------------
// Forward apply: y = [relu](x * scale + shift).  Row-loop structure with
// a fixed channel octet per thread so scale/shift live in registers.
// ---------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(BLOCK) void k_bn_fwd_apply(
        const ushort_t* __restrict__ x, const ushort_t* __restrict__ z,
        ushort_t* __restrict__ y, long m, int c,
        const float* __restrict__ scale,
        const float* __restrict__ shift, int relu,
        unsigned char* __restrict__ mask) {
    const int slots = c / VEC;
    const int rpb = BLOCK / slots > 0 ? BLOCK / slots : 1;
    const int slot = threadIdx.x % slots;
    const int rg = threadIdx.x / slots;
    if (rg >= rpb) return;
    float sc[VEC], sh[VEC];
    #pragma unroll
    for (int k = 0; k < VEC; ++k) {
        sc[k] = scale[slot * VEC + k];
        sh[k] = shift[slot * VEC + k];
    }
    const ushort_t* xb = x + (size_t)slot * VEC;
    const ushort_t* zb = z ? z + (size_t)slot * VEC : nullptr;
    ushort_t* yb = y + (size_t)slot * VEC;
    for (long row = (long)blockIdx.x * rpb + rg; row < m;
            row += (long)gridDim.x * rpb) {
        Vec8 in, vz, out;
        in.f4 = *reinterpret_cast<const float4*>(xb + (size_t)row * c);
        if (zb)
            vz.f4 = *reinterpret_cast<const float4*>(zb + (size_t)row * c);
        unsigned bits = 0;
        #pragma unroll
        for (int k = 0; k < VEC; ++k) {
            float f = fmaf(b2f(in.u[k]), sc[k], sh[k]);
            if (zb) f += b2f(vz.u[k]);
            if (f > 0.f) bits |= 1u << k;
            if (relu) f = f > 0.f ? f : 0.f;
            out.u[k] = f2b(f);
        }
        *reinterpret_cast<float4*>(yb + (size_t)row * c) = out.f4;
        // rpb * slots == BLOCK whenever slots divides BLOCK, so a wave's
        // 64 mask bytes are contiguous.
        if (mask) mask[(size_t)row * slots + slot] = (unsigned char)bits;
    }
}

// ---------------------------------------------------------------------
// Stage-1 backward reduction: per-block partials of (masked dy) and
// (masked dy * xhat) per channel, into the same ws layout as forward.
// ---------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(BLOCK) void k_bn_bwd_reduce(
        const ushort_t* __restrict__ x, const ushort_t* __restrict__ z,
        const ushort_t* __restrict__ dy,
        long m, int c, int nb, const float* __restrict__ mean,
        const float* __restrict__ rstd, const float* __restrict__ scale,
        const float* __restrict__ shift, int relu,
        const unsigned char* __restrict__ mask, float* __restrict__ ws) {
    const int slots = c / VEC;
    const int rpb = BLOCK / slots > 0 ? BLOCK / slots : 1;
    const int slot = threadIdx.x % slots;
    const int rg = threadIdx.x / slots;
    __shared__ float lds[BLOCK * VEC];

    float sg[VEC], sgx[VEC];
    float mn[VEC], rs[VEC], sc[VEC], sh[VEC];
    #pragma unroll
    for (int k = 0; k < VEC; ++k) {
        sg[k] = 0.f; sgx[k] = 0.f;
        mn[k] = mean[slot * VEC + k];
        rs[k] = rstd[slot * VEC + k];
        sc[k] = scale[slot * VEC + k];
        sh[k] = shift[slot * VEC + k];
    }
    if (rg < rpb) {
        const ushort_t* xb = x + (size_t)slot * VEC;
        const ushort_t* zb = z ? z + (size_t)slot * VEC : nullptr;
        const ushort_t* db = dy + (size_t)slot * VEC;
        for (long row = (long)blockIdx.x * rpb + rg; row < m;
                row += (long)gridDim.x * rpb) {
            Vec8 vx, vz, vd;
            vx.f4 = *reinterpret_cast<const float4*>(xb + (size_t)row * c);
            if (zb)
                vz.f4 = *reinterpret_cast<const float4*>(
                    zb + (size_t)row * c);
            vd.f4 = *reinterpret_cast<const float4*>(db + (size_t)row * c);
            // saved forward ReLU mask (residual BNs): bit k = "kept"
            unsigned bits = 0;
            if (mask) bits = mask[(size_t)row * slots + slot];
            #pragma unroll
            for (int k = 0; k < VEC; ++k) {
                float fx = b2f(vx.u[k]);
                float g = b2f(vd.u[k]);
                if (mask) {
                    if (!((bits >> k) & 1u)) g = 0.f;
                } else if (relu) {
                    float pre = fmaf(fx, sc[k], sh[k]);
                    if (zb) pre += b2f(vz.u[k]);
                    if (pre <= 0.f) g = 0.f;
                }
                sg[k] += g;
                sgx[k] = fmaf(g, (fx - mn[k]) * rs[k], sgx[k]);
            }
        }
    }
    rg_tree_reduce(sg, lds, slots, rpb, rg);
    if (rg == 0) {
        #pragma unroll
        for (int k = 0; k < VEC; ++k)
            ws[(size_t)(slot * VEC + k) * nb + blockIdx.x] = sg[k];
    }
    __syncthreads();
    rg_tree_reduce(sgx, lds, slots, rpb, rg);
    if (rg == 0) {
        #pragma unroll
        for (int k = 0; k < VEC; ++k)
            ws[(size_t)(c + slot * VEC + k) * nb + blockIdx.x] = sgx[k];
    }
}

// ---------------------------------------------------------------------
// Backward tail (C blocks): row sums, then one thread per channel writes
// dgamma/dbeta + dx coefficients.
// dx = p * g - q * x + r  with g = masked dy:
//   p = gamma * rstd
//   q = p * (sum_gx / M) * rstd          (0 in eval mode)
//   r = -p * (sum_g / M) + q * mean      (0 in eval mode)
// ---------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(BLOCK) void k_bn_bwd_tail(
        const float* __restrict__ ws, int nb, long m, int c,
        const float* __restrict__ gamma, const float* __restrict__ mean,
        const float* __restrict__ rstd, int train,
        float* __restrict__ dgamma, float* __restrict__ dbeta,
        float* __restrict__ pqr) {
    __shared__ float lds[2 * BLOCK / WAVE];
    const int i = blockIdx.x;
    const float g = gamma[i], rs = rstd[i], mn = mean[i];
    float sum_g, sum_gx;
    ws_row_pair_sum(ws, nb, c, i, lds, sum_g, sum_gx);
    // as in the forward tail: every product below rounds on its own
    if (threadIdx.x == 0) {
        #pragma clang fp contract(off)
        dbeta[i] = sum_g;
        dgamma[i] = sum_gx;
        float p = g * rs;
        float q = 0.f, r = 0.f;
        if (train) {
            float inv_m = 1.0f / (float)m;
            q = p * (sum_gx * inv_m) * rs;
            r = -p * (sum_g * inv_m) + q * mn;
        }
        pqr[i] = p;
        pqr[c + i] = q;
        pqr[2 * c + i] = r;
    }
}

// ---------------------------------------------------------------------
// Backward apply: dx = p * g - q * x + r (g = masked dy), row-loop with
// register-resident per-channel coefficients.
// ---------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(BLOCK) void k_bn_bwd_apply(
        const ushort_t* __restrict__ x, const ushort_t* __restrict__ z,
        const ushort_t* __restrict__ dy,
        ushort_t* __restrict__ dx, ushort_t* __restrict__ dz, long m,
        int c, const float* __restrict__ scale,
        const float* __restrict__ shift,
        const float* __restrict__ pqr, int relu,
        const unsigned char* __restrict__ mask) {
    const int slots = c / VEC;
    const int rpb = BLOCK / slots > 0 ? BLOCK / slots : 1;
    const int slot = threadIdx.x % slots;
    const int rg = threadIdx.x / slots;
    if (rg >= rpb) return;
    float sc[VEC], sh[VEC], cp[VEC], cq[VEC], cr[VEC];
    #pragma unroll
    for (int k = 0; k < VEC; ++k) {
        sc[k] = scale[slot * VEC + k];
        sh[k] = shift[slot * VEC + k];
        cp[k] = pqr[slot * VEC + k];
        cq[k] = pqr[c + slot * VEC + k];
        cr[k] = pqr[2 * c + slot * VEC + k];
    }
    const ushort_t* xb = x + (size_t)slot * VEC;
    const ushort_t* zb = z ? z + (size_t)slot * VEC : nullptr;
    const ushort_t* db = dy + (size_t)slot * VEC;
    ushort_t* ob = dx + (size_t)slot * VEC;
    ushort_t* zo = dz ? dz + (size_t)slot * VEC : nullptr;
    for (long row = (long)blockIdx.x * rpb + rg; row < m;
            row += (long)gridDim.x * rpb) {
        Vec8 vx, vz, vd, out, outz;
        vx.f4 = *reinterpret_cast<const float4*>(xb + (size_t)row * c);
        if (zb)
            vz.f4 = *reinterpret_cast<const float4*>(zb + (size_t)row * c);
        vd.f4 = *reinterpret_cast<const float4*>(db + (size_t)row * c);
        unsigned bits = 0;
        if (mask) bits = mask[(size_t)row * slots + slot];
        #pragma unroll
        for (int k = 0; k < VEC; ++k) {
            float fx = b2f(vx.u[k]);
            float g = b2f(vd.u[k]);
            if (mask) {
                if (!((bits >> k) & 1u)) g = 0.f;
            } else if (relu) {
                float pre = fmaf(fx, sc[k], sh[k]);
                if (zb) pre += b2f(vz.u[k]);
                if (pre <= 0.f) g = 0.f;
            }
            if (zo) outz.u[k] = f2b(g);
            out.u[k] = f2b(fmaf(cp[k], g, fmaf(-cq[k], fx, cr[k])));
        }
        *reinterpret_cast<float4*>(ob + (size_t)row * c) = out.f4;
        if (zo)
            *reinterpret_cast<float4*>(zo + (size_t)row * c) = outz.f4;
    }
}

// ---- host-side launchers ---------------------------------------------

static inline unsigned bn_grid(long work_items, int per_block, long cap) {
    long blocks = (work_items + per_block - 1) / per_block;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return (unsigned)blocks;
}

// Rows a block covers per grid-stride step: each thread owns one channel
// octet, so BLOCK threads span BLOCK / (C / VEC) whole rows.
static inline int bn_rows_per_block(int c) {
    const int slots = c / VEC;
    return BLOCK / slots > 0 ? BLOCK / slots : 1;
}

// Stage-1 (reduce) grid size = rows of the partials workspace.  The ONLY
// definition: launchers, the bindings' size check and the Python-side
// allocation all call this.
extern "C" long bn_num_rblocks(long m, int c) {
    return bn_grid(m, bn_rows_per_block(c), MAX_RBLOCKS);
}

// mask (nullable): M * C / 8 bytes, written only with relu and a residual.
// num_batches_tracked (nullable): int64 scalar bumped by the forward tail.
extern "C" void launch_bn_fwd(
        const ushort_t* x, const ushort_t* z, ushort_t* y, long m, int c,
        const float* gamma, const float* beta, float* running_mean,
        float* running_var, float momentum, float eps, int train, int relu,
        float* ws, float* save_mean, float* save_rstd, float* scale,
        float* shift, unsigned char* mask, long long* num_batches_tracked,
        hipStream_t s) {
    const int rpb = bn_rows_per_block(c);
    if (train) {
        const unsigned nb = (unsigned)bn_num_rblocks(m, c);
        hipLaunchKernelGGL(k_bn_fwd_reduce, dim3(nb), dim3(BLOCK), 0, s,
                           x, m, c, (int)nb, ws);
        hipLaunchKernelGGL(k_bn_fwd_tail, dim3(c), dim3(BLOCK), 0, s,
                           ws, (int)nb, m, c, gamma, beta, running_mean,
                           running_var, momentum, eps, save_mean, save_rstd,
                           scale, shift, num_batches_tracked);
    } else {
        hipLaunchKernelGGL(k_bn_eval_finalize,
                           dim3((c + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s,
                           c, gamma, beta, running_mean, running_var, eps,
                           save_mean, save_rstd, scale, shift);
    }
    if (!(relu && z)) mask = nullptr;
    hipLaunchKernelGGL(k_bn_fwd_apply, dim3(bn_grid(m, rpb, MAX_BLOCKS)),
                       dim3(BLOCK), 0, s, x, z, y, m, c, scale, shift,
                       relu, mask);
}

// With a mask (saved by the forward for relu + residual) z may be null:
// the backward reads the mask byte instead of recomputing it from z.
extern "C" void launch_bn_bwd(
        const ushort_t* x, const ushort_t* z, const ushort_t* dy,
        ushort_t* dx, ushort_t* dz, long m, int c,
        const float* gamma, const float* save_mean, const float* save_rstd,
        const float* scale, const float* shift, int train, int relu,
        float* ws, float* dgamma, float* dbeta, float* pqr,
        const unsigned char* mask, hipStream_t s) {
    const int rpb = bn_rows_per_block(c);
    const unsigned nb = (unsigned)bn_num_rblocks(m, c);
    if (!relu) mask = nullptr;
    hipLaunchKernelGGL(k_bn_bwd_reduce, dim3(nb), dim3(BLOCK), 0, s,
                       x, z, dy, m, c, (int)nb, save_mean, save_rstd,
                       scale, shift, relu, mask, ws);
    hipLaunchKernelGGL(k_bn_bwd_tail, dim3(c), dim3(BLOCK), 0, s,
                       ws, (int)nb, m, c, gamma, save_mean, save_rstd,
                       train, dgamma, dbeta, pqr);
    hipLaunchKernelGGL(k_bn_bwd_apply, dim3(bn_grid(m, rpb, MAX_BLOCKS)),
                       dim3(BLOCK), 0, s, x, z, dy, dx, dz, m, c, scale,
                       shift, pqr, relu, mask);
}
