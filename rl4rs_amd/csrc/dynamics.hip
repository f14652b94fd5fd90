// Probabilistic ensemble dynamics model (d3rlpy 0.91's ProbabilisticEnsembleDynamics, restated in DESIGN.md) and the SAC target
// MOPO trains on: the rl4rs_dyn_* handle of include/rl4rs_hip.h.
//
// M members share the input xa = [scaled x | a] [N, D + E].  Per member:
//   z1 = relu(xa W1 / sigma1 + b1);  h1 = dropout(bn1(z1));  z2 = relu([h1 | xa] W2 / sigma2 + b2);  h2 = dropout(bn2(z2));
//   mu = h2 Wmu / sigma3 + bmu;  ls = h2 Wls + bls, then the two softplus bounds.
// The dense products run through the library's fp32 MFMA GEMMs (gemm.hip, policy.hip) WITHOUT bias or activation: the 1 / sigma
// scale of a spectrally normalised matrix is a device scalar that the kernel behind the product applies (k_dyn_bn_fwd, k_dyn_head,
// k_dyn_nll), so W / sigma never exists in memory.  [h1 | xa] W2 is h1 W2[:H1] + xa W2[H1:]: the second product is the addend of the
// first.  Every reduction has a fixed order and there is no float atomic: identical calls give identical bits.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "optim.hpp"

namespace rl4rs {
namespace {

constexpr float DYN_BN_EPS = 1e-5f, DYN_BN_MOM = 0.1f, DYN_SN_EPS = 1e-12f, DYN_PENALTY = 0.01f;
constexpr size_t DYN_LDS_MAX = 160 * 1024;
constexpr int DYN_NLL_WAVES = 8;
constexpr int DYN_MAX_MEMBERS = 16;
// sites of the counter RNG (the `a` argument of uniform01 is site * 65536 + column): dropout of member m, layer l = 2 m + l
constexpr uint32_t DYN_SITE_INDEX = 1000, DYN_SITE_NOISE = 1001;

// One member's slice of the flat parameter / state buffers.  Matrix k = 0, 1, 2 is W1, W2, Wmu (the first O columns of the head).
struct DynDims {
    int D, E, H1, H2, M, O, K1, K2;
    int use_bn, use_dense, spectral;
    float rate;
    // parameters (offsets inside a member's block of psize floats)
    int64_t w1, b1, g1, be1, w2, b2, g2, be2, wh, bh, maxls, minls, psize;
    // non-trained state (offsets inside a member's block of ssize floats); the scaler constants follow the last member
    int64_t u[3], v[3], rm1, rv1, rm2, rv2, ssize;
    int64_t sc_min, sc_range, sc_rew;          // absolute offsets: obs min [D], obs range [D], {reward mean, reward scale}
    // per-member statistics of the last forward: sigma[3], batch mean / biased variance of both layers
    int64_t st_mean1, st_var1, st_mean2, st_var2, stsize;
    int64_t mw[3]; int min_[3], mout[3], mld[3];
};

__device__ __forceinline__ float dyn_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// fixed-order sum over a workgroup of 256 threads
__device__ __forceinline__ float dyn_block_sum(float v, float* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ float dyn_softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float dyn_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// xa[n] = [(x[n] - min) / range | a[n]]; a constant column (range 0) maps to 0
__global__ void k_dyn_prep(const float* __restrict__ x, const float* __restrict__ a, const float* __restrict__ omin,
                           const float* __restrict__ orange, float* __restrict__ xa, int N, int D, int E) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int K = D + E;
    if (i >= (int64_t)N * K) return;
    const int n = (int)(i / K), c = (int)(i - (int64_t)n * K);
    float v;
    if (c < D) {
        const float rg = orange[c];
        v = rg > 0.f ? (x[(size_t)n * D + c] - omin[c]) / rg : 0.f;
    } else {
        v = a[(size_t)n * E + (c - D)];
    }
    xa[i] = v;
}

// Spectral norm of matrix blockIdx.x of member blockIdx.y, torch's [out, in] orientation on the library's [in, out] storage:
// training: v <- normalize(W u) (our W, rows = in), u <- normalize(W^T v), both written back; then sigma = u . (W^T v).
// One workgroup, 256 threads; dynamic LDS: us[out] | vs[in] | red[256].
__global__ __launch_bounds__(256) void k_dyn_power(DynDims d, const float* __restrict__ params, float* __restrict__ state,
                                                   float* __restrict__ stats, float* __restrict__ inv_sigma, int train) {
    extern __shared__ float dyn_sm[];
    const int k = blockIdx.x, m = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int in = d.min_[k], out = d.mout[k], ld = d.mld[k];
    const float* W = params + (size_t)m * d.psize + d.mw[k];
    float* u = state + (size_t)m * d.ssize + d.u[k];
    float* v = state + (size_t)m * d.ssize + d.v[k];
    float *us = dyn_sm, *vs = dyn_sm + out, *red = vs + in;
    for (int j = tid; j < out; j += 256) us[j] = u[j];
    for (int i = tid; i < in; i += 256) vs[i] = v[i];
    __syncthreads();
    if (train) {
        for (int i = wave; i < in; i += 4) {
            float s = 0.f;
            for (int j = lane; j < out; j += 64) s += W[(size_t)i * ld + j] * us[j];
            s = dyn_wave_sum(s);
            if (lane == 0) vs[i] = s;
        }
        __syncthreads();
        float p = 0.f;
        for (int i = tid; i < in; i += 256) p += vs[i] * vs[i];
        float inv = 1.f / fmaxf(sqrtf(dyn_block_sum(p, red)), DYN_SN_EPS);
        for (int i = tid; i < in; i += 256) { vs[i] *= inv; v[i] = vs[i]; }
        __syncthreads();
        for (int j = tid; j < out; j += 256) {
            float s = 0.f;
            for (int i = 0; i < in; ++i) s += W[(size_t)i * ld + j] * vs[i];
            us[j] = s;
        }
        __syncthreads();
        p = 0.f;
        for (int j = tid; j < out; j += 256) p += us[j] * us[j];
        inv = 1.f / fmaxf(sqrtf(dyn_block_sum(p, red)), DYN_SN_EPS);
        for (int j = tid; j < out; j += 256) { us[j] *= inv; u[j] = us[j]; }
        __syncthreads();
    }
    float p = 0.f;
    for (int j = tid; j < out; j += 256) {
        float s = 0.f;
        for (int i = 0; i < in; ++i) s += W[(size_t)i * ld + j] * vs[i];
        p += us[j] * s;
    }
    const float sigma = dyn_block_sum(p, red);
    if (tid == 0) {
        stats[(size_t)m * d.stsize + k] = sigma;
        inv_sigma[m * 3 + k] = 1.f / sigma;
    }
}

// A layer behind its raw product P [M, N, H]: z = relu(P / sigma + b) (written back over P), batch norm over the N rows of the
// member (training: batch statistics, biased variance; running statistics move with the unbiased one; eval: running statistics),
// dropout keep mask of site 2 m + layer.  Workgroup = 64 columns x 4 row groups; the four partial sums join in group order.
__global__ __launch_bounds__(256) void k_dyn_bn_fwd(DynDims d, int layer, int N, int H, const float* __restrict__ params,
                                                    float* __restrict__ state, float* __restrict__ stats,
                                                    const float* __restrict__ inv_sigma, float* __restrict__ P, float* __restrict__ xhat,
                                                    float* __restrict__ Y, int train, uint32_t seed, uint32_t step) {
    __shared__ float red[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, m = blockIdx.y;
    const int col = blockIdx.x * 64 + tx;
    const bool ok = col < H;
    const int c = ok ? col : H - 1;
    const float* pm = params + (size_t)m * d.psize;
    const float bias = pm[(layer ? d.b2 : d.b1) + c], g = pm[(layer ? d.g2 : d.g1) + c], be = pm[(layer ? d.be2 : d.be1) + c];
    const float is = inv_sigma[m * 3 + layer];
    float* Pm = P + (size_t)m * N * H;
    float mean = 0.f, var = 1.f;
    if (d.use_bn) {
        float* rm = state + (size_t)m * d.ssize + (layer ? d.rm2 : d.rm1);
        float* rv = state + (size_t)m * d.ssize + (layer ? d.rv2 : d.rv1);
        if (train) {
            float s = 0.f;
            for (int r = ty; r < N; r += 4) s += fmaxf(Pm[(size_t)r * H + c] * is + bias, 0.f);
            red[ty][tx] = s;
            __syncthreads();
            mean = (((red[0][tx] + red[1][tx]) + red[2][tx]) + red[3][tx]) / (float)N;
            __syncthreads();
            s = 0.f;
            for (int r = ty; r < N; r += 4) {
                const float dz = fmaxf(Pm[(size_t)r * H + c] * is + bias, 0.f) - mean;
                s += dz * dz;
            }
            red[ty][tx] = s;
            __syncthreads();
            const float ss = ((red[0][tx] + red[1][tx]) + red[2][tx]) + red[3][tx];
            var = ss / (float)N;
            if (ok && ty == 0) {
                float* stm = stats + (size_t)m * d.stsize;
                stm[(layer ? d.st_mean2 : d.st_mean1) + col] = mean;
                stm[(layer ? d.st_var2 : d.st_var1) + col] = var;
                rm[col] = (1.f - DYN_BN_MOM) * rm[col] + DYN_BN_MOM * mean;
                rv[col] = (1.f - DYN_BN_MOM) * rv[col] + DYN_BN_MOM * (ss / (float)(N - 1));
            }
        } else {
            mean = rm[c];
            var = rv[c];
        }
    }
    if (!ok) return;
    const float rstd = 1.f / sqrtf(var + DYN_BN_EPS);
    const bool drop = train && d.rate > 0.f;
    const float keep_scale = 1.f / (1.f - d.rate);
    const uint32_t site = (uint32_t)(2 * m + layer) * 65536u + (uint32_t)col;
    for (int r = ty; r < N; r += 4) {
        const size_t o = (size_t)r * H + col;
        const float z = fmaxf(Pm[o] * is + bias, 0.f);
        Pm[o] = z;
        float y = z;
        if (d.use_bn) {
            const float xh = (z - mean) * rstd;
            if (xhat) xhat[(size_t)m * N * H + o] = xh;
            y = xh * g + be;
        }
        if (drop) y = uniform01(seed, step, (uint32_t)r, site) >= d.rate ? y * keep_scale : 0.f;
        Y[(size_t)m * N * H + o] = y;
    }
}

// The backward of k_dyn_bn_fwd: dY [M, N, H] (gradient of the layer's output) becomes dP (gradient of the raw product) in place;
// d gamma, d beta and d bias go to the gradient buffer.  Same workgroup shape and summation order as the forward.
__global__ __launch_bounds__(256) void k_dyn_bn_bwd(DynDims d, int layer, int N, int H, const float* __restrict__ params,
                                                    const float* __restrict__ stats, const float* __restrict__ inv_sigma,
                                                    const float* __restrict__ Z, const float* __restrict__ xhat, float* __restrict__ dY,
                                                    float* __restrict__ grad, uint32_t seed, uint32_t step) {
    __shared__ float red[2][4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, m = blockIdx.y;
    const int col = blockIdx.x * 64 + tx;
    const bool ok = col < H;
    const int c = ok ? col : H - 1;
    const float g = params[(size_t)m * d.psize + (layer ? d.g2 : d.g1) + c];
    const float is = inv_sigma[m * 3 + layer];
    const float var = d.use_bn ? stats[(size_t)m * d.stsize + (layer ? d.st_var2 : d.st_var1) + c] : 1.f;
    const float rstd = 1.f / sqrtf(var + DYN_BN_EPS);
    const bool drop = d.rate > 0.f;
    const float keep_scale = 1.f / (1.f - d.rate);
    const uint32_t site = (uint32_t)(2 * m + layer) * 65536u + (uint32_t)c;
    const size_t base = (size_t)m * N * H;
    float s1 = 0.f, s2 = 0.f;
    if (d.use_bn) {
        for (int r = ty; r < N; r += 4) {
            const size_t o = base + (size_t)r * H + c;
            float dy = dY[o];
            if (drop) dy = uniform01(seed, step, (uint32_t)r, site) >= d.rate ? dy * keep_scale : 0.f;
            s1 += dy;
            s2 += dy * xhat[o];
        }
    }
    red[0][ty][tx] = s1;
    red[1][ty][tx] = s2;
    __syncthreads();
    s1 = ((red[0][0][tx] + red[0][1][tx]) + red[0][2][tx]) + red[0][3][tx];
    s2 = ((red[1][0][tx] + red[1][1][tx]) + red[1][2][tx]) + red[1][3][tx];
    __syncthreads();
    const float m1 = g * s1 / (float)N, m2 = g * s2 / (float)N;
    float sb = 0.f;
    for (int r = ty; r < N; r += 4) {
        const size_t o = base + (size_t)r * H + c;
        float dy = dY[o];
        if (drop) dy = uniform01(seed, step, (uint32_t)r, site) >= d.rate ? dy * keep_scale : 0.f;
        float dz = d.use_bn ? rstd * ((dy * g - m1) - xhat[o] * m2) : dy;
        dz = Z[o] > 0.f ? dz : 0.f;
        sb += dz;
        if (ok) dY[o] = dz * is;
    }
    red[0][ty][tx] = sb;
    __syncthreads();
    if (ok && ty == 0) {
        float* gm = grad + (size_t)m * d.psize;
        gm[(layer ? d.b2 : d.b1) + col] = ((red[0][0][tx] + red[0][1][tx]) + red[0][2][tx]) + red[0][3][tx];
        gm[(layer ? d.g2 : d.g1) + col] = d.use_bn ? s2 : 0.f;
        gm[(layer ? d.be2 : d.be1) + col] = d.use_bn ? s1 : 0.f;
    }
}

// out [M, N, 2 O] = [mu | bounded ls] from the raw head product PH [M, N, 2 O]
__global__ void k_dyn_head(DynDims d, int N, const float* __restrict__ params, const float* __restrict__ inv_sigma,
                           const float* PH, float* out) {       // out may be PH itself (rl4rs_dyn_predict)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int O = d.O;
    if (i >= (int64_t)d.M * N * O) return;
    const int m = (int)(i / ((int64_t)N * O));
    const int64_t rem = i - (int64_t)m * N * O;
    const int n = (int)(rem / O), o = (int)(rem - (int64_t)n * O);
    const float* pm = params + (size_t)m * d.psize;
    const size_t row = ((size_t)m * N + n) * 2 * O;
    const float mu = PH[row + o] * inv_sigma[m * 3 + 2] + pm[d.bh + o];
    const float l = PH[row + O + o] + pm[d.bh + O + o];
    const float mx = pm[d.maxls + o], mn = pm[d.minls + o];
    const float a = mx - dyn_softplus(mx - l);
    out[row + o] = mu;
    out[row + O + o] = mn + dyn_softplus(a - mn);
}

// The loss of member blockIdx.x and its gradient with respect to the raw head product, in one pass over PH [M, N, 2 O] (overwritten
// with the gradient: the mu half already carries the 1 / sigma of the product, so one NT / TN GEMM pair serves both halves).
// Also d bias (both halves), d max_ls, d min_ls and loss[m].  Wave w takes rows w, w + W, ...; its column sums live in its own LDS
// slice and the slices join in wave order.  Dynamic LDS: acc[4][W][O] | wl[W] | red[256].
__global__ __launch_bounds__(DYN_NLL_WAVES * 64) void k_dyn_nll(DynDims d, int N, const float* __restrict__ params,
                                                                const float* __restrict__ state, const float* __restrict__ inv_sigma,
                                                                const float* __restrict__ xa, const float* __restrict__ next_x,
                                                                const float* __restrict__ next_r, const float* __restrict__ mask,
                                                                float* __restrict__ PH, float* __restrict__ grad, float* __restrict__ loss) {
    extern __shared__ float dyn_sm[];
    constexpr int NW = DYN_NLL_WAVES;
    const int m = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int O = d.O, D = d.D, K1 = d.K1;
    float* acc = dyn_sm;                            // [4][NW][O]
    float* wl = acc + (size_t)4 * NW * O;           // [NW]
    float* red = wl + NW;                           // [256]
    const float* pm = params + (size_t)m * d.psize;
    const float* bh = pm + d.bh;
    const float* mxp = pm + d.maxls;
    const float* mnp = pm + d.minls;
    const float* omin = state + d.sc_min;
    const float* orange = state + d.sc_range;
    const float rmean = state[d.sc_rew], rscale = state[d.sc_rew + 1];
    const float is = inv_sigma[m * 3 + 2];
    for (int i = tid; i < 4 * NW * O; i += NW * 64) acc[i] = 0.f;
    float p = 0.f;
    if (tid < 256)
        for (int o = tid; o < O; o += 256) p += mxp[o] - mnp[o];
    __syncthreads();
    float pen = 0.f;
    if (tid < 256) {                                // the first four waves reduce; the others wait at the barriers below
        red[tid] = p;
    }
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    pen = DYN_PENALTY * red[0];
    const float invD = 1.f / (float)D;
    float wloss = 0.f;
    float* a_bmu = acc + ((size_t)0 * NW + wave) * O;
    float* a_bls = acc + ((size_t)1 * NW + wave) * O;
    float* a_max = acc + ((size_t)2 * NW + wave) * O;
    float* a_min = acc + ((size_t)3 * NW + wave) * O;
    for (int b = wave; b < N; b += NW) {
        const float w = mask[(size_t)m * N + b] / (float)N;
        const size_t row = ((size_t)m * N + b) * 2 * O;
        float like = 0.f, sls = 0.f;
        for (int o = lane; o < O; o += 64) {
            const float mu = PH[row + o] * is + bh[o];
            const float l = PH[row + O + o] + bh[O + o];
            const float mx = mxp[o], mn = mnp[o];
            const float t1 = mx - l;
            const float a = mx - dyn_softplus(t1);
            const float t2 = a - mn;
            const float ls = mn + dyn_softplus(t2);
            float tgt, pred, cw;
            if (o < D) {
                const float rg = orange[o];
                tgt = rg > 0.f ? (next_x[(size_t)b * D + o] - omin[o]) / rg : 0.f;
                pred = xa[(size_t)b * K1 + o] + mu;
                cw = invD;
            } else {
                tgt = (next_r[b] - rmean) / rscale;
                pred = mu;
                cw = 1.f;
            }
            const float diff = pred - tgt;
            const float e = expf(-ls);
            const float q = diff * diff * e * cw;
            like += q;
            sls += ls;
            const float dmu = w * (2.f * diff * e * cw);
            const float dls = w * (1.f - q);
            const float s1 = dyn_sigmoid(t1), s2 = dyn_sigmoid(t2);
            const float dl = dls * s2 * s1;
            PH[row + o] = dmu * is;
            PH[row + O + o] = dl;
            a_bmu[o] += dmu;
            a_bls[o] += dl;
            a_max[o] += dls * s2 * (1.f - s1) + DYN_PENALTY * w;
            a_min[o] += dls * (1.f - s2) - DYN_PENALTY * w;
        }
        like = dyn_wave_sum(like);
        sls = dyn_wave_sum(sls);
        wloss += w * ((like + sls) + pen);
    }
    if (lane == 0) wl[wave] = wloss;
    __syncthreads();
    float* gm = grad + (size_t)m * d.psize;
    for (int o = tid; o < O; o += NW * 64) {
        float s[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float x = 0.f;
            for (int w = 0; w < NW; ++w) x += acc[((size_t)t * NW + w) * O + o];
            s[t] = x;
        }
        gm[d.bh + o] = s[0];
        gm[d.bh + O + o] = s[1];
        gm[d.maxls + o] = s[2];
        gm[d.minls + o] = s[3];
    }
    if (tid == 0) {
        float x = 0.f;
        for (int w = 0; w < NW; ++w) x += wl[w];
        loss[m] = x;
    }
}

// Spectral-norm correction of the gradient G' = G / sigma that the TN GEMM left for matrix blockIdx.x of member blockIdx.y:
// dW = G' - (sum(G' * W) / sigma) v u^T  (storage [in, out]; u, v are the vectors the forward used)
__global__ __launch_bounds__(256) void k_dyn_sn_bwd(DynDims d, const float* __restrict__ params, const float* __restrict__ state,
                                                    const float* __restrict__ inv_sigma, float* __restrict__ grad) {
    __shared__ float red[256];
    const int k = blockIdx.x, m = blockIdx.y, tid = threadIdx.x;
    const int in = d.min_[k], out = d.mout[k], ld = d.mld[k];
    const float* W = params + (size_t)m * d.psize + d.mw[k];
    float* G = grad + (size_t)m * d.psize + d.mw[k];
    const float* u = state + (size_t)m * d.ssize + d.u[k];
    const float* v = state + (size_t)m * d.ssize + d.v[k];
    const int total = in * out;
    float p = 0.f;
    for (int idx = tid; idx < total; idx += 256) {
        const int i = idx / out, j = idx - i * out;
        p += G[(size_t)i * ld + j] * W[(size_t)i * ld + j];
    }
    const float coef = dyn_block_sum(p, red) * inv_sigma[m * 3 + k];
    for (int idx = tid; idx < total; idx += 256) {
        const int i = idx / out, j = idx - i * out;
        G[(size_t)i * ld + j] -= coef * v[i] * u[j];
    }
}

__device__ __forceinline__ float dyn_gauss(uint32_t seed, uint32_t step, uint32_t row, int m, int o) {
    const float u1 = uniform01(seed, step, row, (DYN_SITE_NOISE + 2u * (uint32_t)m) * 65536u + (uint32_t)o);
    const float u2 = uniform01(seed, step, row, (DYN_SITE_NOISE + 2u * (uint32_t)m + 1u) * 65536u + (uint32_t)o);
    return sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

// One wave per row, from every member's [mu | ls] (out [M, N, 2 O], eval forward): the sample of member idx (given, or
// floor(uniform01(seed, step, row, site 1000) * M)), next_x = reverse(x_scaled + delta), reward = reverse(pred[D]), the variance
// (vtype 0: max over members of sum_o exp(2 ls); 1: sum_o of the unbiased variance over members of the sampled [next_x | r],
// scaled units) and optionally reward -= lam * variance.  noise (optional) [M, N, O].
__global__ __launch_bounds__(256) void k_dyn_predict(DynDims d, int N, const float* __restrict__ state, const float* __restrict__ xa,
                                                     const float* __restrict__ out, const int32_t* __restrict__ indices,
                                                     const float* __restrict__ noise, uint32_t seed, uint32_t step, int deterministic,
                                                     int vtype, int penalise, float lam, float* __restrict__ next_x,
                                                     float* __restrict__ reward, float* __restrict__ variance, int32_t* __restrict__ idx_out) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= N) return;
    const int O = d.O, D = d.D, M = d.M;
    int idx = indices ? indices[b] : (int)(uniform01(seed, step, (uint32_t)b, DYN_SITE_INDEX * 65536u) * (float)M);
    idx = min(max(idx, 0), M - 1);
    const float* omin = state + d.sc_min;
    const float* orange = state + d.sc_range;
    const float rmean = state[d.sc_rew], rscale = state[d.sc_rew + 1];
    float var = 0.f;
    if (vtype == 0) {
        for (int m = 0; m < M; ++m) {
            const size_t row = ((size_t)m * N + b) * 2 * O;
            float s = 0.f;
            for (int o = lane; o < O; o += 64) s += expf(2.f * out[row + O + o]);
            s = dyn_wave_sum(s);
            var = m == 0 ? s : fmaxf(var, s);
        }
    } else {
        float s = 0.f;
        for (int o = lane; o < O; o += 64) {
            float sum = 0.f, val[DYN_MAX_MEMBERS];
#pragma unroll
            for (int m = 0; m < DYN_MAX_MEMBERS; ++m) {
                val[m] = 0.f;
                if (m < M) {
                    const size_t row = ((size_t)m * N + b) * 2 * O;
                    const float eps = deterministic ? 0.f : (noise ? noise[((size_t)m * N + b) * O + o] : dyn_gauss(seed, step, (uint32_t)b, m, o));
                    const float pred = out[row + o] + expf(out[row + O + o]) * eps;
                    val[m] = o < D ? xa[(size_t)b * d.K1 + o] + pred : pred;
                    sum += val[m];
                }
            }
            const float mean = sum / (float)M;
            float ss = 0.f;
#pragma unroll
            for (int m = 0; m < DYN_MAX_MEMBERS; ++m)
                if (m < M) ss += (val[m] - mean) * (val[m] - mean);
            s += M > 1 ? ss / (float)(M - 1) : 0.f;
        }
        var = dyn_wave_sum(s);
    }
    const size_t row = ((size_t)idx * N + b) * 2 * O;
    for (int o = lane; o < O; o += 64) {
        const float eps = deterministic ? 0.f : (noise ? noise[((size_t)idx * N + b) * O + o] : dyn_gauss(seed, step, (uint32_t)b, idx, o));
        const float pred = out[row + o] + expf(out[row + O + o]) * eps;
        if (o < D) {
            next_x[(size_t)b * D + o] = (xa[(size_t)b * d.K1 + o] + pred) * orange[o] + omin[o];
        } else {
            float r = pred * rscale + rmean;
            if (penalise) r -= lam * var;
            reward[b] = r;
        }
    }
    if (lane == 0) {
        variance[b] = var;
        if (idx_out) idx_out[b] = idx;
    }
}

// SAC's soft target: y = r + gamma (1 - terminal) (min(q1, q2) - exp(log_temp) logp)
__global__ void k_sac_target(const float* __restrict__ q1, const float* __restrict__ q2, const float* __restrict__ logp,
                             const float* __restrict__ log_temp, const float* __restrict__ rew, const float* __restrict__ ter,
                             float gamma, int N, float* __restrict__ y) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float soft = fminf(q1[i], q2[i]) - expf(log_temp[0]) * logp[i];
    y[i] = rew[i] + gamma * (1.f - ter[i]) * soft;
}

inline dim3 dyn_ew(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace
}  // namespace rl4rs

using namespace rl4rs;

struct rl4rs_dyn {
    rl4rs_dyn_cfg c;
    DynDims d;
    int64_t n_state;
    OptBlock opt;
    void* arena;
    float *state, *stats, *inv_sigma;
    float *xa, *P1, *h1, *T, *P2, *h2, *PH, *xhat1, *xhat2, *part;
    int tn_chunks;
};

static size_t dyn_power_lds(const DynDims& d) {
    size_t w = 0;
    for (int k = 0; k < 3; ++k) w = std::max(w, (size_t)d.min_[k] + d.mout[k]);
    return (w + 256) * 4;
}
static size_t dyn_nll_lds(const DynDims& d) { return ((size_t)4 * DYN_NLL_WAVES * d.O + DYN_NLL_WAVES + 256) * 4; }
static int dyn_tn_chunk(int Ns) { return std::max(256, ((Ns + 63) / 64 + 15) / 16 * 16); }

static int dyn_check_cfg(const rl4rs_dyn_cfg* c, DynDims* out) {
    RL4RS_REQUIRE(c, "dyn: null config");
    RL4RS_REQUIRE(c->obs_dim >= 1 && c->obs_dim <= 65534, "dyn: obs_dim %d out of range [1, 65534]", c->obs_dim);
    RL4RS_REQUIRE(c->act_dim >= 1 && c->act_dim <= 65536, "dyn: act_dim %d out of range [1, 65536] (continuous actions only)", c->act_dim);
    RL4RS_REQUIRE(c->hidden1 >= 1 && c->hidden1 <= 65536 && c->hidden2 >= 1 && c->hidden2 <= 65536,
                  "dyn: hidden_units (%d, %d) out of range [1, 65536]", c->hidden1, c->hidden2);
    RL4RS_REQUIRE(c->members >= 1 && c->members <= DYN_MAX_MEMBERS, "dyn: n_ensembles %d out of range [1, %d]", c->members, DYN_MAX_MEMBERS);
    RL4RS_REQUIRE(c->max_rows >= 1 && c->max_grad_rows >= 0 && c->max_grad_rows <= c->max_rows,
                  "dyn: max_rows %d / max_grad_rows %d (0 <= max_grad_rows <= max_rows)", c->max_rows, c->max_grad_rows);
    RL4RS_REQUIRE(c->dropout_rate >= 0.f && c->dropout_rate < 1.f, "dyn: dropout_rate must be in [0, 1)");
    DynDims d;
    memset(&d, 0, sizeof(d));
    d.D = c->obs_dim; d.E = c->act_dim; d.H1 = c->hidden1; d.H2 = c->hidden2; d.M = c->members; d.O = d.D + 1;
    d.K1 = d.D + d.E; d.K2 = c->use_dense ? d.H1 + d.K1 : d.H1;
    d.use_bn = c->use_batch_norm ? 1 : 0; d.use_dense = c->use_dense ? 1 : 0; d.spectral = c->spectral_norm ? 1 : 0;
    d.rate = c->dropout_rate;
    int64_t o = 0;
    auto take = [&](int64_t n) { int64_t r = o; o += n; return r; };
    d.w1 = take((int64_t)d.K1 * d.H1); d.b1 = take(d.H1); d.g1 = take(d.H1); d.be1 = take(d.H1);
    d.w2 = take((int64_t)d.K2 * d.H2); d.b2 = take(d.H2); d.g2 = take(d.H2); d.be2 = take(d.H2);
    d.wh = take((int64_t)d.H2 * 2 * d.O); d.bh = take(2 * d.O); d.maxls = take(d.O); d.minls = take(d.O);
    d.psize = o;
    d.mw[0] = d.w1; d.min_[0] = d.K1; d.mout[0] = d.H1; d.mld[0] = d.H1;
    d.mw[1] = d.w2; d.min_[1] = d.K2; d.mout[1] = d.H2; d.mld[1] = d.H2;
    d.mw[2] = d.wh; d.min_[2] = d.H2; d.mout[2] = d.O; d.mld[2] = 2 * d.O;
    o = 0;
    for (int k = 0; k < 3; ++k) { d.u[k] = take(d.mout[k]); d.v[k] = take(d.min_[k]); }
    d.rm1 = take(d.H1); d.rv1 = take(d.H1); d.rm2 = take(d.H2); d.rv2 = take(d.H2);
    d.ssize = o;
    d.sc_min = d.ssize * d.M; d.sc_range = d.sc_min + d.D; d.sc_rew = d.sc_range + d.D;
    o = 3;
    d.st_mean1 = take(d.H1); d.st_var1 = take(d.H1); d.st_mean2 = take(d.H2); d.st_var2 = take(d.H2);
    d.stsize = o;
    // the widest fp32 array of a call is [members, max_rows, max(2 O, H1, H2)]: its byte offsets stay inside 31 bits
    const int64_t widest = std::max<int64_t>(std::max<int64_t>(2 * d.O, d.K1), std::max(d.H1, d.H2));
    const int64_t per_row = (int64_t)d.M * widest * 4;
    const int64_t cap = (((int64_t)1 << 31) - 1) / per_row;
    RL4RS_REQUIRE((int64_t)c->max_rows <= cap,
                  "dyn: max_rows %d: the widest fp32 scratch array [%d members, max_rows, %lld] (%lld bytes per row) would reach 2^31 "
                  "bytes (most rows: %lld)", c->max_rows, d.M, (long long)widest, (long long)per_row, (long long)cap);
    RL4RS_REQUIRE(d.psize * d.M * 4 < ((int64_t)1 << 31), "dyn: %lld parameters would reach 2^31 bytes", (long long)(d.psize * d.M));
    RL4RS_REQUIRE(dyn_power_lds(d) <= DYN_LDS_MAX, "dyn: the power-iteration kernel needs %zu bytes of LDS for these widths (limit %zu)",
                  dyn_power_lds(d), DYN_LDS_MAX);
    RL4RS_REQUIRE(dyn_nll_lds(d) <= DYN_LDS_MAX, "dyn: the loss kernel needs %zu bytes of LDS for obs_dim %d (limit %zu)", dyn_nll_lds(d),
                  d.D, DYN_LDS_MAX);
    if (out) *out = d;
    return RL4RS_OK;
}

// every member's forward up to the raw head product PH; training also moves u / v and the running statistics
static int dyn_forward(rl4rs_dyn* p, int N, const float* x, const float* a, int train, uint32_t seed, uint32_t step, hipStream_t st) {
    const DynDims& d = p->d;
    hipLaunchKernelGGL(k_dyn_prep, dyn_ew((int64_t)N * d.K1), dim3(256), 0, st, x, a, p->state + d.sc_min, p->state + d.sc_range, p->xa, N,
                       d.D, d.E);
    if (d.spectral) {
        const size_t lds = dyn_power_lds(d);
        int rc = raise_dyn_smem(reinterpret_cast<const void*>(&k_dyn_power), lds);
        if (rc) return rc;
        hipLaunchKernelGGL(k_dyn_power, dim3(3, d.M), dim3(256), lds, st, d, p->opt.params, p->state, p->stats, p->inv_sigma, train);
    }
    RL4RS_LAUNCH_CHECK();
    const bool keep = train && p->c.max_grad_rows > 0;
    for (int m = 0; m < d.M; ++m) {
        const float* pm = p->opt.params + (size_t)m * d.psize;
        int rc = launch_gemm_f32(p->xa, d.K1, pm + d.w1, d.H1, nullptr, p->P1 + (size_t)m * N * d.H1, d.H1, N, d.H1, d.K1, ACT_NONE, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_dyn_bn_fwd, dim3((d.H1 + 63) / 64, d.M), dim3(256), 0, st, d, 0, N, d.H1, p->opt.params, p->state, p->stats,
                       p->inv_sigma, p->P1, keep ? p->xhat1 : (float*)nullptr, p->h1, train, seed, step);
    RL4RS_LAUNCH_CHECK();
    for (int m = 0; m < d.M; ++m) {
        const float* pm = p->opt.params + (size_t)m * d.psize;
        float* P2 = p->P2 + (size_t)m * N * d.H2;
        const float* h1 = p->h1 + (size_t)m * N * d.H1;
        int rc;
        if (d.use_dense) {
            float* T = p->T + (size_t)m * N * d.H2;
            rc = launch_gemm_f32(p->xa, d.K1, pm + d.w2 + (size_t)d.H1 * d.H2, d.H2, nullptr, T, d.H2, N, d.H2, d.K1, ACT_NONE, st);
            if (rc) return rc;
            rc = launch_gemm_f32(h1, d.H1, pm + d.w2, d.H2, nullptr, P2, d.H2, N, d.H2, d.H1, ACT_NONE, st, T, d.H2, 1);
        } else {
            rc = launch_gemm_f32(h1, d.H1, pm + d.w2, d.H2, nullptr, P2, d.H2, N, d.H2, d.H1, ACT_NONE, st);
        }
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_dyn_bn_fwd, dim3((d.H2 + 63) / 64, d.M), dim3(256), 0, st, d, 1, N, d.H2, p->opt.params, p->state, p->stats,
                       p->inv_sigma, p->P2, keep ? p->xhat2 : (float*)nullptr, p->h2, train, seed, step);
    RL4RS_LAUNCH_CHECK();
    for (int m = 0; m < d.M; ++m) {
        const float* pm = p->opt.params + (size_t)m * d.psize;
        int rc = launch_gemm_f32(p->h2 + (size_t)m * N * d.H2, d.H2, pm + d.wh, 2 * d.O, nullptr, p->PH + (size_t)m * N * 2 * d.O, 2 * d.O, N,
                                 2 * d.O, d.H2, ACT_NONE, st);
        if (rc) return rc;
    }
    return RL4RS_OK;
}

static int dyn_tn(rl4rs_dyn* p, const float* A_, int lda, int Mr, const float* B_, int ldb, int Nc, int Ns, float* dW, hipStream_t st) {
    return launch_gemm_tn(A_, lda, Mr, B_, ldb, Nc, Ns, dyn_tn_chunk(Ns), p->part, nullptr, dW, nullptr, st);
}

extern "C" {

int64_t rl4rs_dyn_param_count(const rl4rs_dyn_cfg* cfg) {
    DynDims d;
    if (dyn_check_cfg(cfg, &d)) return -1;
    return d.psize * d.M;
}
int64_t rl4rs_dyn_state_count(const rl4rs_dyn_cfg* cfg) {
    DynDims d;
    if (dyn_check_cfg(cfg, &d)) return -1;
    return d.sc_rew + 2;
}
int64_t rl4rs_dyn_stats_count(const rl4rs_dyn_cfg* cfg) {
    DynDims d;
    if (dyn_check_cfg(cfg, &d)) return -1;
    return d.stsize * d.M;
}

int rl4rs_dyn_destroy(rl4rs_dyn* p) {
    if (!p) return RL4RS_OK;
    if (p->arena) (void)hipFree(p->arena);
    delete p;
    return RL4RS_OK;
}

int rl4rs_dyn_create(const rl4rs_dyn_cfg* cfg, const float* params_host, const float* state_host, void* stream, rl4rs_dyn** out) {
    DynDims d;
    int rc = dyn_check_cfg(cfg, &d);
    if (rc) return rc;
    RL4RS_REQUIRE(params_host && state_host && out, "dyn_create: null argument");
    *out = nullptr;
    if (rl4rs_device_count() <= 0) {
        set_error("no HIP device visible: librl4rs_hip has no CPU fallback");
        return RL4RS_EHIP;
    }
    rl4rs_dyn* p = new rl4rs_dyn();
    p->c = *cfg; p->d = d; p->arena = nullptr; p->opt.t = 0;
    p->opt.n = d.psize * d.M; p->n_state = d.sc_rew + 2;
    const size_t R = (size_t)cfg->max_rows, G = (size_t)cfg->max_grad_rows, M = d.M, np = (size_t)p->opt.n;
    std::vector<std::pair<void**, size_t>> reqs;
    auto req = [&](float** slot, size_t n) { reqs.emplace_back(reinterpret_cast<void**>(slot), n * sizeof(float)); };
    req(&p->opt.params, np); req(&p->opt.grad, np); req(&p->opt.m, np); req(&p->opt.v, np);
    req(&p->state, (size_t)p->n_state); req(&p->stats, (size_t)d.stsize * M); req(&p->inv_sigma, 3 * M);
    req(&p->xa, R * d.K1); req(&p->P1, M * R * d.H1); req(&p->h1, M * R * d.H1); req(&p->T, d.use_dense ? M * R * d.H2 : 1);
    req(&p->P2, M * R * d.H2); req(&p->h2, M * R * d.H2); req(&p->PH, M * R * 2 * d.O);
    req(&p->xhat1, M * G * d.H1); req(&p->xhat2, M * G * d.H2);
    p->tn_chunks = G > 256 ? 64 : 1;            // dyn_tn_chunk never gives more than 64 chunks; up to 256 rows are one chunk
    const size_t widest = std::max(std::max((size_t)d.K1 * d.H1, (size_t)std::max(d.H1, d.K1) * d.H2), (size_t)d.H2 * 2 * d.O);
    req(&p->part, p->tn_chunks > 1 ? (size_t)p->tn_chunks * widest : 1);
    size_t total = 0;
    for (auto& r : reqs) total += (r.second + 255) / 256 * 256;
    hipError_t e = hipMalloc(&p->arena, total);
    if (e != hipSuccess) {
        set_error("dyn_create: hipMalloc(%zu bytes) failed: %s", total, hipGetErrorString(e));
        p->arena = nullptr;
        rl4rs_dyn_destroy(p);
        return RL4RS_ENOMEM;
    }
    size_t off = 0;
    for (auto& r : reqs) { *r.first = static_cast<char*>(p->arena) + off; off += (r.second + 255) / 256 * 256; }
    hipStream_t st = (hipStream_t)stream;
    e = hipMemcpyAsync(p->opt.params, params_host, np * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(p->state, state_host, (size_t)p->n_state * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(p->opt.grad, 0, np * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(p->opt.m, 0, np * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(p->opt.v, 0, np * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(p->stats, 0, (size_t)d.stsize * M * 4, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_fill, dim3(1), dim3(64), 0, st, p->inv_sigma, 3 * d.M, 1.f);     // spectral_norm off: sigma = 1
        for (int m = 0; m < d.M; ++m) hipLaunchKernelGGL(k_fill, dim3(1), dim3(64), 0, st, p->stats + (size_t)m * d.stsize, 3, 1.f);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        set_error("dyn_create: initialisation failed: %s", hipGetErrorString(e));
        rl4rs_dyn_destroy(p);
        return RL4RS_EHIP;
    }
    *out = p;
    return RL4RS_OK;
}

int rl4rs_dyn_params(rl4rs_dyn* p, float** params_dev, float** grad_dev, int64_t* count) {
    return opt_params(RL4RS_OPT(p), params_dev, grad_dev, count, "dyn_params");
}
int rl4rs_dyn_adam_state(rl4rs_dyn* p, float** m_dev, float** v_dev, int64_t* step) {
    return opt_adam_state(RL4RS_OPT(p), m_dev, v_dev, step, "dyn_adam_state");
}
int rl4rs_dyn_set_adam_step(rl4rs_dyn* p, int64_t step) {
    return opt_set_adam_step(RL4RS_OPT(p), step, "dyn_set_adam_step");
}
int rl4rs_dyn_state(rl4rs_dyn* p, float** state_dev, int64_t* count, float** stats_dev, int64_t* stats_count) {
    RL4RS_REQUIRE(p, "dyn_state: null handle");
    if (state_dev) *state_dev = p->state;
    if (count) *count = p->n_state;
    if (stats_dev) *stats_dev = p->stats;
    if (stats_count) *stats_count = p->d.stsize * p->d.M;
    return RL4RS_OK;
}

int rl4rs_dyn_forward(rl4rs_dyn* p, int32_t N, const float* x_dev, const float* a_dev, int32_t train, uint32_t seed, uint32_t step,
                      float* out_dev, void* stream) {
    RL4RS_REQUIRE(p && x_dev && a_dev && out_dev && N > 0, "dyn_forward: bad argument");
    const int cap = train ? (p->c.max_grad_rows > 0 ? p->c.max_grad_rows : p->c.max_rows) : p->c.max_rows;
    RL4RS_REQUIRE(N <= cap, "dyn_forward: N=%d exceeds the handle's %d rows", N, cap);
    RL4RS_REQUIRE(!(train && p->d.use_bn) || N >= 2, "dyn_forward: batch norm in training needs at least 2 rows");
    hipStream_t st = (hipStream_t)stream;
    int rc = dyn_forward(p, N, x_dev, a_dev, train ? 1 : 0, seed, step, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_dyn_head, dyn_ew((int64_t)p->d.M * N * p->d.O), dim3(256), 0, st, p->d, N, p->opt.params, p->inv_sigma, p->PH, out_dev);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

int rl4rs_dyn_loss_grad(rl4rs_dyn* p, int32_t N, const float* x_dev, const float* a_dev, const float* next_x_dev, const float* next_r_dev,
                        const float* mask_dev, uint32_t seed, uint32_t step, float* loss_dev, void* stream) {
    RL4RS_REQUIRE(p && x_dev && a_dev && next_x_dev && next_r_dev && mask_dev && loss_dev && N > 0 && N <= p->c.max_grad_rows,
                  "dyn_loss_grad: bad argument (N=%d, max_grad_rows=%d)", N, p ? p->c.max_grad_rows : -1);
    RL4RS_REQUIRE(!p->d.use_bn || N >= 2, "dyn_loss_grad: batch norm in training needs at least 2 rows");
    const DynDims& d = p->d;
    hipStream_t st = (hipStream_t)stream;
    int rc = dyn_forward(p, N, x_dev, a_dev, 1, seed, step, st);
    if (rc) return rc;
    const size_t lds = dyn_nll_lds(d);
    rc = raise_dyn_smem(reinterpret_cast<const void*>(&k_dyn_nll), lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k_dyn_nll, dim3(d.M), dim3(DYN_NLL_WAVES * 64), lds, st, d, N, p->opt.params, p->state, p->inv_sigma, p->xa, next_x_dev,
                       next_r_dev, mask_dev, p->PH, p->opt.grad, loss_dev);
    RL4RS_LAUNCH_CHECK();
    // head: dWh = h2^T dPH; dh2 = dPH Wh^T (into the h2 buffer's place: P2 keeps z2, xhat2 keeps the normalised values)
    for (int m = 0; m < d.M; ++m) {
        const float* pm = p->opt.params + (size_t)m * d.psize;
        float* gm = p->opt.grad + (size_t)m * d.psize;
        const float* dPH = p->PH + (size_t)m * N * 2 * d.O;
        float* h2 = p->h2 + (size_t)m * N * d.H2;
        rc = dyn_tn(p, h2, d.H2, d.H2, dPH, 2 * d.O, 2 * d.O, N, gm + d.wh, st);
        if (rc) return rc;
        rc = launch_gemm_nt(dPH, 2 * d.O, pm + d.wh, 2 * d.O, h2, d.H2, N, d.H2, 2 * d.O, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_dyn_bn_bwd, dim3((d.H2 + 63) / 64, d.M), dim3(256), 0, st, d, 1, N, d.H2, p->opt.params, p->stats, p->inv_sigma, p->P2,
                       p->xhat2, p->h2, p->opt.grad, seed, step);
    RL4RS_LAUNCH_CHECK();
    // layer 2: dW2[:H1] = h1^T dP2, dW2[H1:] = xa^T dP2, dh1 = dP2 W2[:H1]^T (h1 is read by the TN product before it is overwritten)
    for (int m = 0; m < d.M; ++m) {
        const float* pm = p->opt.params + (size_t)m * d.psize;
        float* gm = p->opt.grad + (size_t)m * d.psize;
        const float* dP2 = p->h2 + (size_t)m * N * d.H2;
        float* h1 = p->h1 + (size_t)m * N * d.H1;
        rc = dyn_tn(p, h1, d.H1, d.H1, dP2, d.H2, d.H2, N, gm + d.w2, st);
        if (rc) return rc;
        if (d.use_dense) {
            rc = dyn_tn(p, p->xa, d.K1, d.K1, dP2, d.H2, d.H2, N, gm + d.w2 + (size_t)d.H1 * d.H2, st);
            if (rc) return rc;
        }
        rc = launch_gemm_nt(dP2, d.H2, pm + d.w2, d.H2, h1, d.H1, N, d.H1, d.H2, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_dyn_bn_bwd, dim3((d.H1 + 63) / 64, d.M), dim3(256), 0, st, d, 0, N, d.H1, p->opt.params, p->stats, p->inv_sigma, p->P1,
                       p->xhat1, p->h1, p->opt.grad, seed, step);
    RL4RS_LAUNCH_CHECK();
    for (int m = 0; m < d.M; ++m) {
        float* gm = p->opt.grad + (size_t)m * d.psize;
        rc = dyn_tn(p, p->xa, d.K1, d.K1, p->h1 + (size_t)m * N * d.H1, d.H1, d.H1, N, gm + d.w1, st);
        if (rc) return rc;
    }
    if (d.spectral) {
        hipLaunchKernelGGL(k_dyn_sn_bwd, dim3(3, d.M), dim3(256), 0, st, d, p->opt.params, p->state, p->inv_sigma, p->opt.grad);
        RL4RS_LAUNCH_CHECK();
    }
    return RL4RS_OK;
}

int rl4rs_dyn_adam_step(rl4rs_dyn* p, float lr, float beta1, float beta2, float eps, void* stream) {
    RL4RS_REQUIRE(p && lr >= 0.f, "dyn_adam_step: bad argument");
    const AdamTerms s = adam_advance(p->opt, ADAM_TORCH_DIV, lr, beta1, beta2, eps);
    hipLaunchKernelGGL(k_adam_div, dyn_ew(p->opt.n), dim3(256), 0, (hipStream_t)stream, p->opt.params, p->opt.grad, p->opt.m, p->opt.v,
                       p->opt.n, s.lr_t, s.eps_or_bc2, beta1, beta2, eps);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

int rl4rs_dyn_predict(rl4rs_dyn* p, int32_t N, const float* x_dev, const float* a_dev, const int32_t* indices_dev, const float* noise_dev,
                      uint32_t seed, uint32_t step, int32_t deterministic, int32_t variance_type, int32_t penalise, float lam,
                      float* next_x_dev, float* reward_dev, float* variance_dev, int32_t* indices_out_dev, void* stream) {
    RL4RS_REQUIRE(p && x_dev && a_dev && next_x_dev && reward_dev && variance_dev && N > 0 && N <= p->c.max_rows,
                  "dyn_predict: bad argument (N=%d, max_rows=%d)", N, p ? p->c.max_rows : -1);
    RL4RS_REQUIRE(variance_type == 0 || variance_type == 1, "dyn_predict: variance_type %d (0 = max, 1 = data)", variance_type);
    hipStream_t st = (hipStream_t)stream;
    int rc = dyn_forward(p, N, x_dev, a_dev, 0, seed, step, st);
    if (rc) return rc;
    // the bounded [mu | ls] of every member take the place of the raw product
    hipLaunchKernelGGL(k_dyn_head, dyn_ew((int64_t)p->d.M * N * p->d.O), dim3(256), 0, st, p->d, N, p->opt.params, p->inv_sigma, p->PH, p->PH);
    hipLaunchKernelGGL(k_dyn_predict, dim3((N + 3) / 4), dim3(256), 0, st, p->d, N, p->state, p->xa, p->PH, indices_dev, noise_dev, seed, step,
                       deterministic ? 1 : 0, variance_type, penalise ? 1 : 0, lam, next_x_dev, reward_dev, variance_dev, indices_out_dev);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

int rl4rs_sac_target(const float* q1_dev, const float* q2_dev, const float* logp_dev, const float* log_temp_dev, const float* rew_dev,
                     const float* ter_dev, float gamma, int32_t N, float* y_dev, void* stream) {
    RL4RS_REQUIRE(q1_dev && q2_dev && logp_dev && log_temp_dev && rew_dev && ter_dev && y_dev && N > 0, "sac_target: bad argument");
    hipLaunchKernelGGL(k_sac_target, dyn_ew(N), dim3(256), 0, (hipStream_t)stream, q1_dev, q2_dev, logp_dev, log_temp_dev, rew_dev, ter_dev,
                       gamma, N, y_dev);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

}  // extern "C"
