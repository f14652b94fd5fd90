// The optimiser plumbing every trainable handle shares: the parameter block, the bodies of the rl4rs_X_params / _adam_state /
// _set_adam_step / _copy_params accessors, the host-side Adam bias correction and the element-wise Adam kernels with the small
// reductions they need.  Included by policy.hip, exactk.hip and dynamics.hip, which link into one library: everything here has
// internal linkage.  The per-element arithmetic is written once and is not to be rearranged - the build forbids contraction, so the
// same source expression gives the same bits in every unit, and the learners' tests pin those bits.
#pragma once
#include "common.hpp"

namespace rl4rs {
namespace {

// Flat parameters, their gradient and the Adam state of one handle.  The handle allocates (its `owned` list or its arena) and only
// fills the pointers; grad stays null where the gradient is the caller's buffer (rl4rs_policy).
struct OptBlock {
    float *params, *grad, *m, *v;
    int64_t n, t;          // element count; Adam steps taken
};

// ---- bodies of the exported accessors; `who` is the exported function's message prefix, b is null when its handle is
inline int opt_params(OptBlock* b, float** params_dev, float** grad_dev, int64_t* count, const char* who) {
    RL4RS_REQUIRE(b, "%s: null handle", who);
    if (params_dev) *params_dev = b->params;
    if (grad_dev) *grad_dev = b->grad;
    if (count) *count = b->n;
    return RL4RS_OK;
}
inline int opt_adam_state(OptBlock* b, float** m_dev, float** v_dev, int64_t* step, const char* who) {
    RL4RS_REQUIRE(b, "%s: null handle", who);
    if (m_dev) *m_dev = b->m;
    if (v_dev) *v_dev = b->v;
    if (step) *step = b->t;
    return RL4RS_OK;
}
inline int opt_set_adam_step(OptBlock* b, int64_t step, const char* who) {
    RL4RS_REQUIRE(b && step >= 0, "%s: bad argument", who);
    b->t = step;
    return RL4RS_OK;
}
inline int opt_copy_params(OptBlock* dst, const OptBlock* src, void* stream, const char* who) {
    RL4RS_REQUIRE(dst && src && dst->n == src->n, "%s: handles differ", who);
    RL4RS_HIP_TRY(hipMemcpyAsync(dst->params, src->params, (size_t)src->n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return RL4RS_OK;
}
#define RL4RS_OPT(h) ((h) ? &(h)->opt : nullptr)

// ---- bias correction on the host, in double, cast to float last.  Three forms, each kept as its learners' parity tests pin it
// (they round differently and are not to be merged):
//   ADAM_TF         tf.train.AdamOptimizer: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), eps as given
//   ADAM_TORCH      torch.optim.Adam, p -= lr / (1 - b1^t) m / (sqrt(v / (1 - b2^t)) + eps), as the TF kernel with eps sqrt(1 - b2^t)
//   ADAM_TORCH_DIV  torch.optim.Adam for k_adam_div: lr_t = lr / (1 - b1^t), eps_or_bc2 = 1 / sqrt(1 - b2^t)
enum AdamForm { ADAM_TF, ADAM_TORCH, ADAM_TORCH_DIV };
struct AdamTerms { float lr_t, eps_or_bc2; };
// advances the block's step counter and returns the terms of the step being taken
inline AdamTerms adam_advance(OptBlock& b, AdamForm form, float lr, float beta1, float beta2, float eps) {
    b.t += 1;
    const double t = (double)b.t;
    if (form == ADAM_TF) return {(float)(lr * sqrt(1.0 - pow((double)beta2, t)) / (1.0 - pow((double)beta1, t))), eps};
    if (form == ADAM_TORCH) {
        const double c2 = sqrt(1.0 - pow((double)beta2, t));
        return {(float)(lr * c2 / (1.0 - pow((double)beta1, t))), (float)(eps * c2)};
    }
    return {(float)((double)lr / (1.0 - std::pow((double)beta1, t))), (float)(1.0 / std::sqrt(1.0 - std::pow((double)beta2, t)))};
}

// ---- small reductions and fills
// dst[i] = sum_z part[z][i] in chunk order (fixed order => reproducible)
__global__ void k_reduce_chunks(const float* __restrict__ part, int count, int nz, float* __restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    float s = 0.f;
    for (int z = 0; z < nz; ++z) s += part[(size_t)z * count + i];
    dst[i] = s;
}

__global__ void k_fill(float* __restrict__ x, int n, float v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = v;
}

// sum of squares of a flat buffer -> out[0] (single block, fixed order)
__global__ __launch_bounds__(256) void k_sumsq(const float* __restrict__ g, int count, float* __restrict__ out) {
    __shared__ float sm[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < count; i += 256) s += g[i] * g[i];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sm[0];
}
// the same per VARIABLE: sumsq[v] of four consecutive segments (ends relative to g), one workgroup each, fixed order
struct VarSegs { int end[4]; };
__global__ __launch_bounds__(256) void k_sumsq_vars(const float* __restrict__ g, VarSegs sg, float* __restrict__ out) {
    __shared__ float sm[256];
    const int v = blockIdx.x, lo = v == 0 ? 0 : sg.end[v - 1], hi = sg.end[v];
    float s = 0.f;
    for (int i = lo + threadIdx.x; i < hi; i += 256) s += g[i] * g[i];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[v] = sm[0];
}

// ---- Adam, element-wise
// moments of element i from its (clipped) gradient: stored, and returned as (m, v)
__device__ __forceinline__ float2 adam_moments(float* __restrict__ m, float* __restrict__ v, int64_t i, float gi, float b1, float b2) {
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    return make_float2(mi, vi);
}
// TF form: the new value of a parameter that was pi (k_adam, k_adam_vars, k_adam_multi)
__device__ __forceinline__ float adam_elem(float pi, float* __restrict__ m, float* __restrict__ v, int64_t i, float gi, float lr_t, float b1,
                                           float b2, float eps) {
    const float2 mv = adam_moments(m, v, i, gi, b1, b2);
    return pi - lr_t * mv.x / (sqrtf(mv.y) + eps);
}

// clip > 0: tf.clip_by_global_norm with the norm^2 in sumsq[0] (k_sumsq).  skip != null and *skip != 0: nothing is written.
__global__ void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int64_t count,
                       float lr_t, float b1, float b2, float eps, const float* __restrict__ sumsq, float clip,
                       const int32_t* __restrict__ skip) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count || (skip && *skip)) return;
    float gi = g[i];
    if (clip > 0.f) {
        const float norm = sqrtf(sumsq[0]);
        if (norm > clip) gi *= clip / norm;
    }
    p[i] = adam_elem(p[i], m, v, i, gi, lr_t, b1, b2, eps);
}
// tf.clip_by_norm per VARIABLE (RLlib's minimize_and_clip) with the norms^2 of k_sumsq_vars: the element's own variable's norm
__global__ void k_adam_vars(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int count,
                            VarSegs sg, float lr_t, float b1, float b2, float eps, const float* __restrict__ sumsq, float clip) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    float gi = g[i];
    if (clip > 0.f) {
        const int var = (i >= sg.end[0]) + (i >= sg.end[1]) + (i >= sg.end[2]);
        const float norm = sqrtf(sumsq[var]);
        if (norm > clip) gi *= clip / norm;
    }
    p[i] = adam_elem(p[i], m, v, i, gi, lr_t, b1, b2, eps);
}
// torch.optim.Adam in its own division form: p -= (lr / (1 - b1^t)) * (m / (sqrt(v) / sqrt(1 - b2^t) + eps)), another fp32 expression
__global__ void k_adam_div(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int64_t count,
                           float step_size, float inv_sqrt_bc2, float b1, float b2, float eps) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float2 mv = adam_moments(m, v, i, g[i], b1, b2);
    p[i] -= step_size * (mv.x / (sqrtf(mv.y) * inv_sqrt_bc2 + eps));
}

// One step of a block on gradient g (the block's own or the caller's): advance, the norm when clip > 0 (sumsq: one device float),
// k_adam.  Two launches with a clip, else one.
inline void adam_step(OptBlock& b, const float* g, AdamForm form, float lr, float beta1, float beta2, float eps, float* sumsq, float clip,
                      const int32_t* skip, hipStream_t st) {
    const AdamTerms a = adam_advance(b, form, lr, beta1, beta2, eps);
    if (clip > 0.f) hipLaunchKernelGGL(k_sumsq, dim3(1), dim3(256), 0, st, g, (int)b.n, sumsq);
    hipLaunchKernelGGL(k_adam, dim3((unsigned)((b.n + 255) / 256)), dim3(256), 0, st, b.params, g, b.m, b.v, b.n, a.lr_t, beta1, beta2,
                       a.eps_or_bc2, sumsq, clip, skip);
}

}  // namespace
}  // namespace rl4rs
