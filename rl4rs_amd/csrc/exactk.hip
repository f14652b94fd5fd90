// Exact-K on gfx950: the pointer-network slate generator (self-attention encoder over the candidate items, LSTM pointer decoder
// under the location / no-repeat / special-item masks) and its critic, forward + sampling, REINFORCE loss + full backward, Adam.
//
// Reference: rl4rs/nets/exact_k/{model,layers,modules}.py (Generator, Discriminator), script/exact_k_train.py.  TensorFlow 1.15
// is not available: parity is unpinned, the yardstick is the float64 restatement tests/exactk_ref.py.
//
// Every dense product goes through the fp32 MFMA GEMMs of gemm.hip (launch_gemm_f32 / launch_gemm_nt) and the trainers'
// weight-gradient reduction (launch_gemm_tn, policy.hip); the kernels here are what has no counterpart there: attention per
// (row, head), layer norm, the decoder's cell / intra-attention / glimpse / pointer steps and their reverse pass.  The attention
// kernels' own inner products (Q K^T, P V and their transposes, head width 32) run on the vector ALU.
// Nothing is reduced with float atomics: the gradient of two identical calls is bit-identical.
//
// Decoder layout: one launch sequence per step t = 0..8; each per-row kernel streams the row's encoded references
// R = enc W_ref [A, D] from global memory (145 KB per row at A = 284, D = 128: it would fill a CU's LDS on its own, and the
// LSTM / query products of a step are batched over the rows as GEMMs between the per-row kernels, so nothing stays resident).
// Beam search (rl4rs_exactk_decode_beam) runs the same sequence over N * beam decoder rows; its per-USER kernels, which read a
// user's R tile once for all of its beams, are in exactk_beam.hpp.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "optim.hpp"

namespace rl4rs {

namespace {

constexpr int XK_T = 9;                        // slate length
constexpr float XK_PAD = -4294967295.0f;       // -2^32 + 1 (rounds to -2^32 in fp32, as in the reference)
constexpr size_t XK_LDS_MAX = 160 * 1024;
constexpr int XK_COLSUM_CHUNKS = 1024;

struct XkDims { int OD, H, D, F, heads, dh, blocks, A, vocab; };

// dropout keep factor of (site, row, col): 0 or 1 / (1 - rate)
__device__ __forceinline__ float xk_keep(float rate, uint32_t seed, uint32_t step, uint32_t site, uint32_t row, uint32_t col) {
    if (rate <= 0.f) return 1.f;
    return uniform01(seed, step, row, site * 65536u + col) >= rate ? 1.f / (1.f - rate) : 0.f;
}
__device__ __forceinline__ float xk_wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float xk_wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float xk_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// ---------------------------------------------------------------- encoder
// X0[n, a, :] = dropout(concat(enc_user[n], table[a] * sqrt(H)))
__global__ void k_xk_build_enc(const float* __restrict__ eu, const float* __restrict__ table, float* __restrict__ X, int N, int A, int H,
                               float scale, float rate, uint32_t seed, uint32_t step, uint32_t site) {
    const int D = 2 * H;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)N * A * D) return;
    const uint32_t row = (uint32_t)(i / D);
    const int d = (int)(i - (size_t)row * D), n = row / A, a = row - n * A;
    const float v = d < H ? eu[(size_t)n * H + d] : table[(size_t)a * H + (d - H)] * scale;
    X[i] = v * xk_keep(rate, seed, step, site, row, (uint32_t)d);
}
// backward of the same: d enc_user[n, h] = sum_a dX0[n, a, h] keep; d table[a, h] = scale * sum_n dX0[n, a, H + h] keep (fixed order)
__global__ void k_xk_build_enc_bwd(const float* __restrict__ dX, float* __restrict__ d_eu, const float* __restrict__ eu,
                                   float* __restrict__ d_table, int N, int A, int H, float scale, float rate, uint32_t seed,
                                   uint32_t step, uint32_t site) {
    const int D = 2 * H;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N * H) {
        const int n = i / H, h = i - n * H;
        float s = 0.f;
        for (int a = 0; a < A; ++a) {
            const uint32_t row = (uint32_t)(n * A + a);
            s += dX[(size_t)row * D + h] * xk_keep(rate, seed, step, site, row, (uint32_t)h);
        }
        d_eu[i] = eu[i] > 0.f ? s : 0.f;                       // relu of the user layer folded in
    } else if (i < N * H + A * H) {
        const int j = i - N * H, a = j / H, h = j - a * H;
        float s = 0.f;
        for (int n = 0; n < N; ++n) {
            const uint32_t row = (uint32_t)(n * A + a);
            s += dX[(size_t)row * D + H + h] * xk_keep(rate, seed, step, site, row, (uint32_t)(H + h));
        }
        d_table[j] = s * scale;
    }
}

// flag[r] = 1 where the row's feature sum is not exactly 0 (key and query masking), one wave per row
__global__ __launch_bounds__(256) void k_xk_rowflag(const float* __restrict__ X, uint8_t* __restrict__ flag, int M, int D) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= M) return;
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s += X[(size_t)r * D + d];
    s = xk_wave_sum(s);
    if (lane == 0) flag[r] = s != 0.f ? 1 : 0;
}

// Attention forward of one (row, head): S = Q K^T / sqrt(dh), key mask, softmax, query mask, dropout, O = P V.
// P [N, heads, A, A] keeps the softmax (before query mask and dropout).  LDS: K, V head slices [A][dh + 1], 4 x (A + dh).
__global__ __launch_bounds__(256) void k_xk_attn_fwd(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
                                                     const uint8_t* __restrict__ flag, float* __restrict__ P, float* __restrict__ O,
                                                     int A, int D, int heads, int dh, float rate, uint32_t seed, uint32_t step,
                                                     uint32_t site) {
    extern __shared__ float sm[];
    const int ld = dh + 1;
    float* Ks = sm;
    float* Vs = Ks + (size_t)A * ld;
    float* sc = Vs + (size_t)A * ld;           // [4][A]
    float* qv = sc + 4 * A;                    // [4][dh]
    const int n = blockIdx.x / heads, h = blockIdx.x - n * heads;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t base = (size_t)n * A * D + (size_t)h * dh;
    for (int i = threadIdx.x; i < A * dh; i += 256) {
        const int a = i / dh, d = i - a * dh;
        Ks[a * ld + d] = K[base + (size_t)a * D + d];
        Vs[a * ld + d] = V[base + (size_t)a * D + d];
    }
    const float root = sqrtf((float)dh);
    float* scw = sc + wave * A;
    float* qw = qv + wave * dh;
    for (int q0 = 0; q0 < A; q0 += 4) {
        const int q = q0 + wave;
        const bool on = q < A;
        __syncthreads();
        if (on)
            for (int d = lane; d < dh; d += 64) qw[d] = Q[base + (size_t)q * D + d];
        __syncthreads();
        if (on) {
            float mx = -3.4028235e38f;
            for (int k = lane; k < A; k += 64) {
                float s = 0.f;
                for (int d = 0; d < dh; ++d) s = fmaf(qw[d], Ks[k * ld + d], s);
                s = s / root;
                if (!flag[(size_t)n * A + k]) s = XK_PAD;
                scw[k] = s;
                mx = fmaxf(mx, s);
            }
            mx = xk_wave_max(mx);
            float se = 0.f;
            for (int k = lane; k < A; k += 64) {
                const float e = expf(scw[k] - mx);
                scw[k] = e;
                se += e;
            }
            se = xk_wave_sum(se);
            const float qm = flag[(size_t)n * A + q] ? 1.f : 0.f;
            const uint32_t row = (uint32_t)((n * heads + h) * A + q);
            float* Pr = P + (size_t)row * A;
            for (int k = lane; k < A; k += 64) {
                const float p = scw[k] / se;
                Pr[k] = p;
                scw[k] = p * qm * xk_keep(rate, seed, step, site, row, (uint32_t)k);
            }
        }
        __syncthreads();
        if (on)
            for (int d = lane; d < dh; d += 64) {
                float s = 0.f;
                for (int k = 0; k < A; ++k) s = fmaf(scw[k], Vs[k * ld + d], s);
                O[base + (size_t)q * D + d] = s;
            }
    }
}

// out[k, d] = sum_q W[q, k] X[q, d] of one (row, head), masked by relu_of > 0:  dV = Pd^T dO (DROP: W = P * query mask * keep) and
// dK = dS^T Q.  Lanes over k (coalesced rows of W), X's head slice in LDS [A][dh], eight columns of d per sweep over q.
template <bool DROP>
__global__ __launch_bounds__(256) void k_xk_attn_tn(const float* __restrict__ W, const float* __restrict__ X, const float* __restrict__ relu_of,
                                                    const uint8_t* __restrict__ flag, float* __restrict__ out, int A, int D, int heads, int dh,
                                                    float rate, uint32_t seed, uint32_t step, uint32_t site) {
    extern __shared__ float sm[];
    float* Xs = sm;                            // [A][dh]
    const int n = blockIdx.x / heads, h = blockIdx.x - n * heads;
    const size_t base = (size_t)n * A * D + (size_t)h * dh;
    for (int i = threadIdx.x; i < A * dh; i += 256) {
        const int a = i / dh, d = i - a * dh;
        Xs[i] = X[base + (size_t)a * D + d];
    }
    __syncthreads();
    const uint32_t row0 = (uint32_t)((n * heads + h) * A);
    const float* Wb = W + (size_t)row0 * A;
    for (int k = threadIdx.x; k < A; k += 256) {
        for (int d0 = 0; d0 < dh; d0 += 8) {
            float acc[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[u] = 0.f;
            for (int q = 0; q < A; ++q) {
                float w = Wb[(size_t)q * A + k];
                if (DROP) w = w * (flag[(size_t)n * A + q] ? 1.f : 0.f) * xk_keep(rate, seed, step, site, row0 + q, (uint32_t)k);
#pragma unroll
                for (int u = 0; u < 8; ++u) acc[u] = fmaf(w, Xs[q * dh + d0 + u], acc[u]);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const size_t o = base + (size_t)k * D + d0 + u;
                out[o] = relu_of[o] > 0.f ? acc[u] : 0.f;
            }
        }
    }
}

// Attention backward of one (row, head), query side: dPd = dO V^T, dP = dPd * query mask * keep, dS = P (dP - sum P dP) / sqrt(dh)
// (0 at masked keys) written over P, dQ = dS K masked by relu(Q) > 0.
__global__ __launch_bounds__(256) void k_xk_attn_bwd_q(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
                                                       const float* __restrict__ dO, const uint8_t* __restrict__ flag, float* __restrict__ P,
                                                       float* __restrict__ dQ, int A, int D, int heads, int dh, float rate, uint32_t seed,
                                                       uint32_t step, uint32_t site) {
    extern __shared__ float sm[];
    const int ld = dh + 1;
    float* Ks = sm;
    float* Vs = Ks + (size_t)A * ld;
    float* sc = Vs + (size_t)A * ld;           // [4][A]
    float* qv = sc + 4 * A;                    // [4][dh]
    const int n = blockIdx.x / heads, h = blockIdx.x - n * heads;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t base = (size_t)n * A * D + (size_t)h * dh;
    for (int i = threadIdx.x; i < A * dh; i += 256) {
        const int a = i / dh, d = i - a * dh;
        Ks[a * ld + d] = K[base + (size_t)a * D + d];
        Vs[a * ld + d] = V[base + (size_t)a * D + d];
    }
    const float root = sqrtf((float)dh);
    float* scw = sc + wave * A;
    float* gw = qv + wave * dh;
    for (int q0 = 0; q0 < A; q0 += 4) {
        const int q = q0 + wave;
        const bool on = q < A;
        __syncthreads();
        if (on)
            for (int d = lane; d < dh; d += 64) gw[d] = dO[base + (size_t)q * D + d];
        __syncthreads();
        if (on) {
            const float qm = flag[(size_t)n * A + q] ? 1.f : 0.f;
            const uint32_t row = (uint32_t)((n * heads + h) * A + q);
            float* Pr = P + (size_t)row * A;
            float dot = 0.f;
            for (int k = lane; k < A; k += 64) {
                float s = 0.f;
                for (int d = 0; d < dh; ++d) s = fmaf(gw[d], Vs[k * ld + d], s);
                const float dp = s * qm * xk_keep(rate, seed, step, site, row, (uint32_t)k);
                scw[k] = dp;
                dot += Pr[k] * dp;
            }
            dot = xk_wave_sum(dot);
            for (int k = lane; k < A; k += 64) {
                const float ds = flag[(size_t)n * A + k] ? Pr[k] * (scw[k] - dot) / root : 0.f;
                Pr[k] = ds;
                scw[k] = ds;
            }
        }
        __syncthreads();
        if (on)
            for (int d = lane; d < dh; d += 64) {
                float s = 0.f;
                for (int k = 0; k < A; ++k) s = fmaf(scw[k], Ks[k * ld + d], s);
                const size_t o = base + (size_t)q * D + d;
                dQ[o] = Q[o] > 0.f ? s : 0.f;
            }
    }
}

// Y = gamma * xhat + beta, xhat = (s - mean) * rstd, s = X (+ R), population variance, eps under the root; one wave per row
__global__ __launch_bounds__(256) void k_xk_add_ln(const float* __restrict__ X, const float* __restrict__ R, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, float* __restrict__ Y, float* __restrict__ xhat,
                                                   float* __restrict__ rstd, int M, int D) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= M) return;
    const size_t o = (size_t)r * D;
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s += X[o + d] + (R ? R[o + d] : 0.f);
    const float mean = xk_wave_sum(s) / (float)D;
    float v = 0.f;
    for (int d = lane; d < D; d += 64) {
        const float c = X[o + d] + (R ? R[o + d] : 0.f) - mean;
        v += c * c;
    }
    const float rs = 1.f / sqrtf(xk_wave_sum(v) / (float)D + 1e-8f);
    for (int d = lane; d < D; d += 64) {
        const float xh = (X[o + d] + (R ? R[o + d] : 0.f) - mean) * rs;
        xhat[o + d] = xh;
        Y[o + d] = gamma[d] * xh + beta[d];
    }
    if (lane == 0) rstd[r] = rs;
}
// dX = rstd * (g dY - mean(g dY) - xhat * mean(g dY xhat)) (+ addend)
__global__ __launch_bounds__(256) void k_xk_ln_bwd(const float* __restrict__ dY, const float* __restrict__ xhat, const float* __restrict__ rstd,
                                                   const float* __restrict__ gamma, const float* __restrict__ addend, float* __restrict__ dX,
                                                   int M, int D) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= M) return;
    const size_t o = (size_t)r * D;
    float a = 0.f, b = 0.f;
    for (int d = lane; d < D; d += 64) {
        const float g = gamma[d] * dY[o + d];
        a += g;
        b += g * xhat[o + d];
    }
    a = xk_wave_sum(a) / (float)D;
    b = xk_wave_sum(b) / (float)D;
    const float rs = rstd[r];
    for (int d = lane; d < D; d += 64)
        dX[o + d] = rs * (gamma[d] * dY[o + d] - a - xhat[o + d] * b) + (addend ? addend[o + d] : 0.f);
}

// part[z][j] = sum over the rows of chunk z of X[n][j] (* Y[n][j]), rows in order (eight loads in flight, added in row order)
__global__ void k_xk_colsum(const float* __restrict__ X, const float* __restrict__ Y, int ld, int Nc, int Ns, int chunk,
                            float* __restrict__ part) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int z = blockIdx.y;
    if (j >= Nc) return;
    const int lo = z * chunk, hi = min(lo + chunk, Ns);
    float s = 0.f;
    for (int n = lo; n < hi; n += 8) {
        float x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const size_t o = (size_t)min(n + u, hi - 1) * ld + j;
            x[u] = Y ? X[o] * Y[o] : X[o];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (n + u < hi) s += x[u];
    }
    part[(size_t)z * Nc + j] = s;
}
// y += a (+ b)
__global__ void k_xk_add(float* __restrict__ y, const float* __restrict__ a, const float* __restrict__ b, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = y[i] + a[i] + (b ? b[i] : 0.f);
}

// ---------------------------------------------------------------- decoder, forward
// XH[t] = [x_t | h_{t-1}]: x_0 = first input, h_{-1} = initial h (step 0); x_t = enc[n, path[n, t-1]] (h_{t-1} came from k_xk_cell_fwd)
__global__ void k_xk_gather_x(int t, int N, int A, int D, const float* __restrict__ enc, const int32_t* __restrict__ path,
                              const float* __restrict__ first, const float* __restrict__ init_h, float* __restrict__ XH) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * D) return;
    const int n = i / D, d = i - n * D;
    float* row = XH + (size_t)n * 2 * D;
    if (t == 0) {
        row[d] = first[d];
        row[D + d] = init_h[d];
    } else {
        int a = path[n * XK_T + t - 1];
        a = min(max(a, 0), A - 1);
        row[d] = enc[((size_t)n * A + a) * D + d];
    }
}
// TF LSTMCell: gates [i | j | f | o], forget bias 1
__global__ void k_xk_cell_fwd(int N, int D, const float* __restrict__ G, const float* __restrict__ cprev, int cprev_ld,
                              float* __restrict__ C, float* __restrict__ Hout, float* __restrict__ XHnext) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * D) return;
    const int n = idx / D, d = idx - n * D;
    const float* g = G + (size_t)n * 4 * D;
    const float i = xk_sigmoid(g[d]), j = tanhf(g[D + d]), f = xk_sigmoid(g[2 * D + d] + 1.f), o = xk_sigmoid(g[3 * D + d]);
    const float c = f * cprev[(size_t)n * cprev_ld + d] + i * j;
    const float h = o * tanhf(c);
    C[idx] = c;
    Hout[idx] = h;
    if (XHnext) XHnext[(size_t)n * 2 * D + D + d] = h;
}

// intra-attention of step t over the earlier cell outputs; all-step arrays are [T][N][D], pI [T][N][T]
__global__ __launch_bounds__(256) void k_xk_intra_fwd(int t, int N, int D, const float* __restrict__ Bef, const float* __restrict__ Qb,
                                                      const float* __restrict__ Hout, const float* __restrict__ v_dec,
                                                      float* __restrict__ pI, float* __restrict__ intra) {
    __shared__ float s_sc[XK_T];
    const int n = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t ND = (size_t)N * D;
    float* out = intra + (size_t)t * ND + (size_t)n * D;
    if (t == 0) {
        for (int d = threadIdx.x; d < D; d += 256) out[d] = 0.f;
        return;
    }
    if (t == 1) {
        for (int d = threadIdx.x; d < D; d += 256) out[d] = Hout[(size_t)n * D + d];
        return;
    }
    const float* qb = Qb + (size_t)t * ND + (size_t)n * D;
    for (int j = wave; j < t; j += 4) {
        const float* bef = Bef + (size_t)j * ND + (size_t)n * D;
        float s = 0.f;
        for (int d = lane; d < D; d += 64) s += v_dec[d] * tanhf(bef[d] + qb[d]);
        s = xk_wave_sum(s);
        if (lane == 0) s_sc[j] = s;
    }
    __syncthreads();
    float mx = s_sc[0];
    for (int j = 1; j < t; ++j) mx = fmaxf(mx, s_sc[j]);
    float p[XK_T], se = 0.f;
    for (int j = 0; j < t; ++j) { p[j] = expf(s_sc[j] - mx); se += p[j]; }
    for (int j = 0; j < t; ++j) p[j] = p[j] / se;
    if (threadIdx.x < t) pI[((size_t)t * N + n) * XK_T + threadIdx.x] = p[threadIdx.x];
    for (int d = threadIdx.x; d < D; d += 256) {
        float s = 0.f;
        for (int j = 0; j < t; ++j) s += p[j] * Hout[(size_t)j * ND + (size_t)n * D + d];
        out[d] = s;
    }
}

// scores of one row into LDS: sc[a] = sum_d v[d] tanh(R[n, a, d] + c[d]); a wave per candidate
__device__ __forceinline__ void xk_scores(const float* __restrict__ Rn, const float* cs, const float* vs, float* sc, int A, int D) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int a = wave; a < A; a += 4) {
        const float* r = Rn + (size_t)a * D;
        float s = 0.f;
        for (int d = lane; d < D; d += 64) s += vs[d] * tanhf(r[d] + cs[d]);
        s = xk_wave_sum(s);
        if (lane == 0) sc[a] = s;
    }
}
// max and sum of exp(sc - max) over the row, by wave 0 -> red[0], red[1]
__device__ __forceinline__ void xk_softmax_stats(const float* sc, int A, float* red) {
    if (threadIdx.x < 64) {
        float mx = -3.4028235e38f;
        for (int a = threadIdx.x; a < A; a += 64) mx = fmaxf(mx, sc[a]);
        mx = xk_wave_max(mx);
        float se = 0.f;
        for (int a = threadIdx.x; a < A; a += 64) se += expf(sc[a] - mx);
        se = xk_wave_sum(se);
        if (threadIdx.x == 0) { red[0] = mx; red[1] = se; }
    }
}

// LDS of the per-row decoder kernels: sc [A] | cs [D] | vs [D] | xs [D] | red [16] | acc [2][parts * D] (backward)
// glimpse: p = softmax over ALL candidates, q = sum_a p_a enc[n, a]
__global__ __launch_bounds__(256) void k_xk_glimpse_fwd(int N, int A, int D, const float* __restrict__ R, const float* __restrict__ Cg,
                                                        const float* __restrict__ v, const float* __restrict__ enc, float* __restrict__ pg,
                                                        float* __restrict__ qout) {
    extern __shared__ float sm[];
    float *sc = sm, *cs = sc + A, *vs = cs + D, *red = vs + 2 * D, *acc = red + 16;
    const int n = blockIdx.x;
    for (int d = threadIdx.x; d < D; d += 256) { cs[d] = Cg[(size_t)n * D + d]; vs[d] = v[d]; }
    __syncthreads();
    xk_scores(R + (size_t)n * A * D, cs, vs, sc, A, D);
    __syncthreads();
    xk_softmax_stats(sc, A, red);
    __syncthreads();
    const float mx = red[0], se = red[1];
    for (int a = threadIdx.x; a < A; a += 256) {
        const float p = expf(sc[a] - mx) / se;
        pg[(size_t)n * A + a] = p;
    }
    __syncthreads();                                   // every thread has read sc before it is overwritten
    for (int a = threadIdx.x; a < A; a += 256) sc[a] = pg[(size_t)n * A + a];
    __syncthreads();
    const int parts = D >= 256 ? 1 : 256 / D, Dw = D >= 256 ? 256 : D;
    const int part = threadIdx.x / Dw, dl = threadIdx.x - part * Dw;
    const float* en = enc + (size_t)n * A * D;
    if (part < parts)
        for (int d = dl; d < D; d += Dw) {
            float s = 0.f;
            for (int a = part; a < A; a += parts) s = fmaf(sc[a], en[(size_t)a * D + d], s);
            acc[part * D + d] = s;
        }
    __syncthreads();
    for (int d = threadIdx.x; d < D; d += 256) {
        float s = 0.f;
        for (int pp = 0; pp < parts; ++pp) s += acc[pp * D + d];
        qout[(size_t)n * D + d] = s;
    }
}

// allowed set of step t given the picks before it
__device__ __forceinline__ bool xk_allowed(int a, int t, int A, const uint8_t* __restrict__ loc, const uint8_t* __restrict__ special,
                                           const int* prev, bool any_special) {
    if (!loc[(t / 3) * A + a]) return false;
    for (int j = 0; j < t; ++j)
        if (prev[j] == a) return false;
    return !(any_special && special[a]);
}

// pointer scores, allowed set, then: mode 0 inverse-CDF draw, 1 first maximum, 2 teacher-forced cross-entropy and d logits
__global__ __launch_bounds__(256) void k_xk_pointer_fwd(int t, int N, int A, int D, const float* __restrict__ R, const float* __restrict__ Cp,
                                                        const float* __restrict__ v, const uint8_t* __restrict__ loc,
                                                        const uint8_t* __restrict__ special, int32_t* __restrict__ path, int mode,
                                                        uint32_t seed, uint32_t step, float* __restrict__ logits_out,
                                                        float* __restrict__ dlogit, const float* __restrict__ w, float* __restrict__ ce,
                                                        float* __restrict__ invalid) {
    extern __shared__ float sm[];
    float *sc = sm, *cs = sc + A, *vs = cs + D, *red = vs + 2 * D;
    __shared__ int s_prev[XK_T];
    __shared__ int s_any;
    const int n = blockIdx.x;
    for (int d = threadIdx.x; d < D; d += 256) { cs[d] = Cp[(size_t)n * D + d]; vs[d] = v[d]; }
    if (threadIdx.x == 0) {
        int any = 0;
        for (int j = 0; j < t; ++j) {
            const int a = min(max(path[n * XK_T + j], 0), A - 1);
            s_prev[j] = a;
            any |= special[a];
        }
        s_any = any;
    }
    __syncthreads();
    xk_scores(R + (size_t)n * A * D, cs, vs, sc, A, D);
    __syncthreads();
    for (int a = threadIdx.x; a < A; a += 256) {
        if (!xk_allowed(a, t, A, loc, special, s_prev, s_any != 0)) sc[a] = XK_PAD;
        if (logits_out) logits_out[((size_t)n * XK_T + t) * A + a] = sc[a];
    }
    __syncthreads();
    xk_softmax_stats(sc, A, red);
    __syncthreads();
    const float mx = red[0], se = red[1];
    if (mode == 2) {
        const int raw = path[n * XK_T + t];
        const int tgt = min(max(raw, 0), A - 1);
        const float wn = w[n] / (float)N;
        for (int a = threadIdx.x; a < A; a += 256) {
            const float l = sc[a];
            const float p = expf(l - mx) / se;
            dlogit[(size_t)n * A + a] = l == XK_PAD ? 0.f : wn * (p - (a == tgt ? 1.f : 0.f));
        }
        if (threadIdx.x == 0) {
            ce[n] = (logf(se) + mx) - sc[tgt];
            invalid[n] = (raw != tgt || sc[tgt] == XK_PAD) ? 1.f : 0.f;
        }
    } else if (mode == 1) {
        if (threadIdx.x < 64) {
            float best = -3.4028235e38f;
            int bi = 0x7fffffff;
            for (int a = threadIdx.x; a < A; a += 64)
                if (sc[a] > best) { best = sc[a]; bi = a; }
            for (int o = 32; o > 0; o >>= 1) {
                const float ob = __shfl_xor(best, o);
                const int oi = __shfl_xor(bi, o);
                if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
            }
            if (threadIdx.x == 0) path[n * XK_T + t] = min(bi, A - 1);
        }
    } else if (threadIdx.x == 0) {
        // the smallest allowed a whose inclusive prefix sum of exp(l - max), in candidate order, exceeds u * total
        const float u = uniform01(seed, step, (uint32_t)n, (uint32_t)t);
        const float target = u * se;
        float run = 0.f;
        int pick = -1, last = 0;
        for (int a = 0; a < A; ++a) {
            if (sc[a] == XK_PAD) continue;
            last = a;
            run += expf(sc[a] - mx);
            if (run > target) { pick = a; break; }
        }
        path[n * XK_T + t] = pick >= 0 ? pick : last;
    }
}

// ---------------------------------------------------------------- decoder, backward
// Shared tail of the glimpse / pointer backward of one row: ds[a] (LDS) is the gradient of the scores.
//   g[a, d] = ds_a v_d (1 - tanh^2(R + c));  dR[n, a, d] += g;  dC[d] = sum_a g;  dvpart[d] = sum_a ds_a tanh(..)
//   glimpse only (pw != null): dEnc[n, a, d] += p_a dq_d
__device__ __forceinline__ void xk_attn_bwd_tail(int n, int A, int D, const float* __restrict__ R, float* __restrict__ dR, const float* ds,
                                                 const float* cs, const float* vs, float* acc, float* __restrict__ dC,
                                                 float* __restrict__ dvpart, const float* pw, const float* dq, float* __restrict__ dEnc) {
    const int parts = D >= 256 ? 1 : 256 / D, Dw = D >= 256 ? 256 : D;
    const int part = threadIdx.x / Dw, dl = threadIdx.x - part * Dw;
    float* accC = acc;
    float* accV = acc + parts * D;
    if (part < parts)
        for (int d = dl; d < D; d += Dw) {
            float sC = 0.f, sV = 0.f;
            for (int a = part; a < A; a += parts) {
                const size_t o = ((size_t)n * A + a) * D + d;
                const float th = tanhf(R[o] + cs[d]);
                const float g = ds[a] * vs[d] * (1.f - th * th);
                dR[o] += g;
                sC += g;
                sV += ds[a] * th;
                if (pw) dEnc[o] += pw[a] * dq[d];
            }
            accC[part * D + d] = sC;
            accV[part * D + d] = sV;
        }
    __syncthreads();
    for (int d = threadIdx.x; d < D; d += 256) {
        float sC = 0.f, sV = 0.f;
        for (int pp = 0; pp < parts; ++pp) { sC += accC[pp * D + d]; sV += accV[pp * D + d]; }
        dC[(size_t)n * D + d] = sC;
        dvpart[(size_t)n * D + d] = sV;
    }
}
__global__ __launch_bounds__(256) void k_xk_pointer_bwd(int N, int A, int D, const float* __restrict__ R, float* __restrict__ dR,
                                                        const float* __restrict__ Cp, const float* __restrict__ v,
                                                        const float* __restrict__ dlogit, float* __restrict__ dC, float* __restrict__ dvpart) {
    extern __shared__ float sm[];
    float *sc = sm, *cs = sc + A, *vs = cs + D, *red = vs + 2 * D, *acc = red + 16;
    const int n = blockIdx.x;
    for (int d = threadIdx.x; d < D; d += 256) { cs[d] = Cp[(size_t)n * D + d]; vs[d] = v[d]; }
    for (int a = threadIdx.x; a < A; a += 256) sc[a] = dlogit[(size_t)n * A + a];
    __syncthreads();
    xk_attn_bwd_tail(n, A, D, R, dR, sc, cs, vs, acc, dC, dvpart, nullptr, nullptr, nullptr);
}
__global__ __launch_bounds__(256) void k_xk_glimpse_bwd(int N, int A, int D, const float* __restrict__ R, float* __restrict__ dR,
                                                        const float* __restrict__ Cg, const float* __restrict__ v, const float* __restrict__ pg,
                                                        const float* __restrict__ dq, const float* __restrict__ enc, float* __restrict__ dEnc,
                                                        float* __restrict__ dC, float* __restrict__ dvpart) {
    extern __shared__ float sm[];
    float *sc = sm, *cs = sc + A, *vs = cs + D, *xs = vs + D, *red = xs + D, *acc = red + 16;
    const int n = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int d = threadIdx.x; d < D; d += 256) { cs[d] = Cg[(size_t)n * D + d]; vs[d] = v[d]; xs[d] = dq[(size_t)n * D + d]; }
    __syncthreads();
    const float* en = enc + (size_t)n * A * D;
    for (int a = wave; a < A; a += 4) {
        float s = 0.f;
        for (int d = lane; d < D; d += 64) s += xs[d] * en[(size_t)a * D + d];
        s = xk_wave_sum(s);
        if (lane == 0) sc[a] = s;                      // dp_a
    }
    __syncthreads();
    const float* p = pg + (size_t)n * A;
    if (threadIdx.x < 64) {
        float s = 0.f;
        for (int a = threadIdx.x; a < A; a += 64) s += p[a] * sc[a];
        s = xk_wave_sum(s);
        if (threadIdx.x == 0) red[0] = s;
    }
    __syncthreads();
    const float dot = red[0];
    for (int a = threadIdx.x; a < A; a += 256) sc[a] = p[a] * (sc[a] - dot);      // ds_a
    __syncthreads();
    xk_attn_bwd_tail(n, A, D, R, dR, sc, cs, vs, acc, dC, dvpart, p, xs, dEnc);
}

// intra-attention backward of step t (t >= 1); dI = dI1 + dI2
__global__ __launch_bounds__(256) void k_xk_intra_bwd(int t, int N, int D, const float* __restrict__ dI1, const float* __restrict__ dI2,
                                                      const float* __restrict__ pI, const float* __restrict__ Hout, const float* __restrict__ Bef,
                                                      const float* __restrict__ Qb, const float* __restrict__ v_dec, float* __restrict__ dHacc,
                                                      float* __restrict__ dBefAcc, float* __restrict__ dQb, float* __restrict__ dvpart) {
    __shared__ float s_dp[XK_T];
    const int n = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t ND = (size_t)N * D, rn = (size_t)n * D;
    if (t == 1) {
        for (int d = threadIdx.x; d < D; d += 256) dHacc[rn + d] += dI1[rn + d] + dI2[rn + d];
        return;
    }
    for (int j = wave; j < t; j += 4) {
        float s = 0.f;
        for (int d = lane; d < D; d += 64) s += (dI1[rn + d] + dI2[rn + d]) * Hout[(size_t)j * ND + rn + d];
        s = xk_wave_sum(s);
        if (lane == 0) s_dp[j] = s;
    }
    __syncthreads();
    float p[XK_T], ds[XK_T], dot = 0.f;
    for (int j = 0; j < t; ++j) { p[j] = pI[((size_t)t * N + n) * XK_T + j]; dot += p[j] * s_dp[j]; }
    for (int j = 0; j < t; ++j) ds[j] = p[j] * (s_dp[j] - dot);
    const float* qb = Qb + (size_t)t * ND + rn;
    for (int d = threadIdx.x; d < D; d += 256) {
        const float di = dI1[rn + d] + dI2[rn + d];
        float sQ = 0.f, sV = 0.f;
        for (int j = 0; j < t; ++j) {
            const size_t o = (size_t)j * ND + rn + d;
            const float th = tanhf(Bef[o] + qb[d]);
            const float g = ds[j] * v_dec[d] * (1.f - th * th);
            dBefAcc[o] += g;
            dHacc[o] += p[j] * di;
            sQ += g;
            sV += ds[j] * th;
        }
        dQb[(size_t)t * ND + rn + d] = sQ;
        dvpart[(size_t)t * ND + rn + d] = sV;
    }
}

// LSTM cell backward of one step: dh = dHacc + the four product pieces (+ the next step's recurrent gradient)
__global__ void k_xk_cell_bwd(int N, int D, const float* __restrict__ dHacc, const float* __restrict__ pc0, const float* __restrict__ pc1,
                              const float* __restrict__ pc2, const float* __restrict__ dXHnext, const float* __restrict__ G,
                              const float* __restrict__ cprev, int cprev_ld, const float* __restrict__ C, float* __restrict__ dCnext,
                              float* __restrict__ dG) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * D) return;
    const int n = idx / D, d = idx - n * D;
    float dh = dHacc[idx] + pc0[idx] + pc1[idx] + pc2[idx];
    if (dXHnext) dh += dXHnext[(size_t)n * 2 * D + D + d];
    const float* g = G + (size_t)n * 4 * D;
    const float i = xk_sigmoid(g[d]), j = tanhf(g[D + d]), f = xk_sigmoid(g[2 * D + d] + 1.f), o = xk_sigmoid(g[3 * D + d]);
    const float tc = tanhf(C[idx]);
    const float dc = dh * o * (1.f - tc * tc) + dCnext[idx];
    float* dg = dG + (size_t)n * 4 * D;
    dg[d] = dc * j * i * (1.f - i);
    dg[D + d] = dc * i * (1.f - j * j);
    dg[2 * D + d] = dc * cprev[(size_t)n * cprev_ld + d] * f * (1.f - f);
    dg[3 * D + d] = dh * tc * o * (1.f - o);
    dCnext[idx] = dc * f;
}
// dXH[:, :D] goes to the gathered encoder row (t >= 1: a slate's picks are distinct and the steps run one after the other, so no
// two writers meet) or to the per-row parts of the first input / initial state (t == 0)
__global__ void k_xk_input_bwd(int t, int N, int A, int D, const float* __restrict__ dXH, const float* __restrict__ dCnext,
                               const int32_t* __restrict__ path, float* __restrict__ dEnc, float* __restrict__ part3) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * D) return;
    const int n = i / D, d = i - n * D;
    const float* row = dXH + (size_t)n * 2 * D;
    if (t == 0) {
        const size_t ND = (size_t)N * D;
        part3[i] = dCnext[i];              // d init_c
        part3[ND + i] = row[D + d];        // d init_h
        part3[2 * ND + i] = row[d];        // d first input
    } else {
        const int a = min(max(path[n * XK_T + t - 1], 0), A - 1);
        dEnc[((size_t)n * A + a) * D + d] += row[d];
    }
}

// out[0] = mean_n w_n sum_t ce[t][n], out[1] = number of (row, step) targets outside the allowed set; one block, fixed order
__global__ __launch_bounds__(256) void k_xk_loss(const float* __restrict__ ce, const float* __restrict__ invalid, const float* __restrict__ w,
                                                 int N, float* __restrict__ out) {
    __shared__ float s0[256], s1[256];
    float a = 0.f, b = 0.f;
    for (int n = threadIdx.x; n < N; n += 256) {
        float s = 0.f;
        for (int t = 0; t < XK_T; ++t) { s += ce[(size_t)t * N + n]; b += invalid[(size_t)t * N + n]; }
        a += w[n] * s;
    }
    s0[threadIdx.x] = a;
    s1[threadIdx.x] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { s0[threadIdx.x] += s0[threadIdx.x + o]; s1[threadIdx.x] += s1[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out[0] = s0[0] / (float)N; out[1] = s1[0]; }
}

// critic: dv = 2 (v - target) (gradient of the SUM of the squared errors), err = (v - target)^2
__global__ void k_xk_critic_err(const float* __restrict__ v, const float* __restrict__ target, float* __restrict__ dv, float* __restrict__ err,
                                int N) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float e = v[i] - target[i];
    dv[i] = 2.f * e;
    if (err) err[i] = e * e;
}

#include "exactk_beam.hpp"

inline dim3 ew(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

}  // namespace rl4rs

using namespace rl4rs;

// ---------------------------------------------------------------- handles
enum { XB_WQ, XB_BQ, XB_WK, XB_BK, XB_WV, XB_BV, XB_G1, XB_B1, XB_W1, XB_BF1, XB_W2, XB_BF2, XB_G2, XB_B2, XB_COUNT };

struct XkLayout {
    size_t wu, bu, table, blk0, blk_size, bo[XB_COUNT];
    size_t wl, bl, init_c, init_h, first, ia_wb, ia_v, ia_wbef, ia_bias;
    size_t a_wq[2], a_wdec[2], a_v[2], a_bias[2], a_wref[2];      // 0 = glimpse, 1 = pointer
    size_t total;
};

static XkLayout xk_layout(const XkDims& d) {
    XkLayout L;
    const size_t D = d.D, F = d.F, H = d.H;
    size_t o = 0;
    auto take = [&](size_t n) { size_t r = o; o += n; return r; };
    L.wu = take((size_t)d.OD * H); L.bu = take(H); L.table = take((size_t)d.vocab * H);
    L.blk0 = o;
    {
        size_t b = 0;
        auto tb = [&](size_t n) { size_t r = b; b += n; return r; };
        L.bo[XB_WQ] = tb(D * D); L.bo[XB_BQ] = tb(D); L.bo[XB_WK] = tb(D * D); L.bo[XB_BK] = tb(D); L.bo[XB_WV] = tb(D * D); L.bo[XB_BV] = tb(D);
        L.bo[XB_G1] = tb(D); L.bo[XB_B1] = tb(D); L.bo[XB_W1] = tb(D * F); L.bo[XB_BF1] = tb(F); L.bo[XB_W2] = tb(F * D); L.bo[XB_BF2] = tb(D);
        L.bo[XB_G2] = tb(D); L.bo[XB_B2] = tb(D);
        L.blk_size = b;
    }
    o += L.blk_size * d.blocks;
    L.wl = take(2 * D * 4 * D); L.bl = take(4 * D); L.init_c = take(D); L.init_h = take(D); L.first = take(D);
    L.ia_wb = take(D * D); L.ia_v = take(D); L.ia_wbef = take(D * D); L.ia_bias = take(D);
    for (int k = 0; k < 2; ++k) {
        L.a_wq[k] = take(D * D); L.a_wdec[k] = take(D * D); L.a_v[k] = take(D); L.a_bias[k] = take(D); L.a_wref[k] = take(D * D);
    }
    L.total = o;
    return L;
}

struct XkBlockAct { float *Q, *K, *V, *P, *xhat1, *rstd1, *Y, *Hf, *xhat2, *rstd2, *Xout; uint8_t* flag; };

// beam search's own scratch (rl4rs_exactk_decode_beam): one allocation, apart from the arena, sized by the N * beam of the largest call
struct XkBeamScratch {
    void* mem = nullptr;
    size_t bytes = 0;
    float *XH, *G, *C, *Cin, *Hout, *Bef, *Qb, *intra, *tmp1, *Cg, *q, *Cp, *acc[2];
    int32_t *prefix[2], *anc[2];
};

struct rl4rs_exactk {
    rl4rs_exactk_cfg c;
    XkDims d;
    XkLayout L;
    OptBlock opt;
    uint8_t *loc, *special;
    void* arena;
    // encoder
    float *EU, *dEU, *X0, *AO, *Z;
    std::vector<XkBlockAct> blk;
    // decoder (all-step arrays [T][N][..] for the N of the call)
    float *Rg, *Rp, *XH, *G, *C, *Hout, *Bef, *Qb, *intra, *pI, *Cg, *pg, *q, *Cp, *tmp1, *dlogit, *ce, *invalid;
    // backward
    float *dEnc, *dRg, *dRp, *dCp, *dCg, *dq, *dI1, *dI2, *dHacc, *dBefAcc, *dQb, *dvp, *dvg, *dvd, *pc0, *pc1, *pc2, *dCnext, *dG, *dXH,
        *part3, *dA, *dB, *dC3, *dF, *tA, *tB, *part, *part_b;
    int32_t* path_tmp;
    int chunk_cap;
    XkBeamScratch beam;
};

struct rl4rs_exactk_critic {
    int OD, HC, max_rows;
    OptBlock opt;
    float *h[3], *dh[3], *v, *dv, *part, *part_b;
    std::vector<void*> owned;
};

static int xk_check_cfg(const rl4rs_exactk_cfg* c, XkDims* out) {
    RL4RS_REQUIRE(c, "exactk: null config");
    RL4RS_REQUIRE(c->obs_dim >= 1 && c->obs_dim <= 65536, "exactk: obs_dim %d out of range", c->obs_dim);
    RL4RS_REQUIRE(c->hidden >= 16 && c->hidden % 16 == 0 && c->hidden <= 1024, "exactk: hidden_units %d must be a multiple of 16 in [16, 1024]",
                  c->hidden);
    const int D = 2 * c->hidden;
    RL4RS_REQUIRE(c->heads >= 1 && D % c->heads == 0 && (D / c->heads) % 8 == 0,
                  "exactk: num_heads %d must divide the model width %d into a head width that is a multiple of 8", c->heads, D);
    RL4RS_REQUIRE(c->blocks >= 1 && c->blocks <= 16, "exactk: num_blocks %d out of range [1, 16]", c->blocks);
    RL4RS_REQUIRE(c->vocab >= 1 && c->action_size >= XK_T && c->action_size <= c->vocab && c->vocab <= 65536,
                  "exactk: action_size %d must be in [9, vocab = %d] (vocab <= 65536)", c->action_size, c->vocab);
    RL4RS_REQUIRE(c->max_rows >= 1, "exactk: max_rows %d", c->max_rows);
    RL4RS_REQUIRE(c->dropout_rate >= 0.f && c->dropout_rate < 1.f, "exactk: dropout_rate must be in [0, 1)");
    // the widest arrays - the activations [max_rows * A, 4H], the logits [max_rows, 9, A] and the decoder's gates [9 * max_rows, 4D] -
    // go through GEMMs with 32-bit row counts
    const int64_t per_row = std::max((int64_t)c->action_size * std::max(2 * D, XK_T), (int64_t)XK_T * 4 * D) * 4;
    const int64_t cap = (((int64_t)1 << 31) - 1) / per_row;       // the most rows that stay under 2^31 bytes
    RL4RS_REQUIRE((int64_t)c->max_rows <= cap,
                  "exactk: max_rows %d: its widest fp32 array (%lld bytes per row: [max_rows * %d, %d] or the decoder's [9 * max_rows, %d]) "
                  "would reach 2^31 bytes (most rows: %lld)", c->max_rows, (long long)per_row, c->action_size, 2 * D, 4 * D, (long long)cap);
    const int dh = D / c->heads;
    const size_t lds = ((size_t)2 * c->action_size * (dh + 1) + 4 * (size_t)(c->action_size + dh)) * 4;
    RL4RS_REQUIRE(lds <= XK_LDS_MAX, "exactk: the attention kernels need %zu bytes of LDS for action_size %d, head width %d (limit %zu)", lds,
                  c->action_size, dh, XK_LDS_MAX);
    const size_t lds_dec = ((size_t)c->action_size + 3 * D + 16 + 2 * (size_t)std::max(D, 256)) * 4;
    RL4RS_REQUIRE(lds_dec <= XK_LDS_MAX, "exactk: the decoder kernels need %zu bytes of LDS (limit %zu)", lds_dec, XK_LDS_MAX);
    if (out) {
        out->OD = c->obs_dim; out->H = c->hidden; out->D = D; out->F = 4 * c->hidden; out->heads = c->heads; out->dh = dh;
        out->blocks = c->blocks; out->A = c->action_size; out->vocab = c->vocab;
    }
    return RL4RS_OK;
}

static int xk_colsum(rl4rs_exactk* p, const float* X, const float* Y, int ld, int Nc, int Ns, float* dst, hipStream_t st) {
    const int chunk = std::max(64, (Ns + XK_COLSUM_CHUNKS - 1) / XK_COLSUM_CHUNKS);       // at most XK_COLSUM_CHUNKS partials
    const int nz = (Ns + chunk - 1) / chunk;
    hipLaunchKernelGGL(k_xk_colsum, dim3((Nc + 63) / 64, nz), dim3(64), 0, st, X, Y, ld, Nc, Ns, chunk, nz == 1 ? dst : p->part_b);
    if (nz > 1) hipLaunchKernelGGL(k_reduce_chunks, dim3((Nc + 255) / 256), dim3(256), 0, st, p->part_b, Nc, nz, dst);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}
static int xk_tn(rl4rs_exactk* p, const float* A_, int lda, int M, const float* B_, int ldb, int Nc, int Ns, float* dW, float* db,
                 hipStream_t st) {
    const int chunk = std::max(256, ((Ns + 63) / 64 + 15) / 16 * 16);
    return launch_gemm_tn(A_, lda, M, B_, ldb, Nc, Ns, chunk, p->part, p->part_b, dW, db, st);
}

static size_t xk_attn_lds(const XkDims& d) { return ((size_t)2 * d.A * (d.dh + 1) + 4 * (size_t)(d.A + d.dh)) * 4; }
static size_t xk_dec_lds(const XkDims& d) { return ((size_t)d.A + 3 * d.D + 16 + 2 * (size_t)std::max(d.D, 256)) * 4; }

// encoder forward of N rows and the two W_ref products (p->Rg, p->Rp) -> *enc_out = enc [N * A, D]
static int xk_encode(rl4rs_exactk* p, int N, const float* obs, uint32_t seed, uint32_t step, uint32_t pass, const float** enc_out,
                     hipStream_t st) {
    const XkDims& d = p->d;
    const XkLayout& L = p->L;
    const float* P = p->opt.params;
    const int A = d.A, D = d.D, H = d.H, F = d.F, M = N * A;
    const float rate = p->c.dropout_rate;
    const uint32_t site0 = pass * 32u;
    int rc;
    if ((rc = launch_gemm_f32(obs, d.OD, P + L.wu, H, P + L.bu, p->EU, H, N, H, d.OD, ACT_RELU, st))) return rc;
    hipLaunchKernelGGL(k_xk_build_enc, ew((size_t)M * D), dim3(256), 0, st, p->EU, P + L.table, p->X0, N, A, H, sqrtf((float)H), rate, seed,
                       step, site0);
    const size_t lds_a = xk_attn_lds(d);
    if ((rc = raise_dyn_smem(reinterpret_cast<const void*>(&k_xk_attn_fwd), lds_a))) return rc;
    const float* X = p->X0;
    for (int b = 0; b < d.blocks; ++b) {
        XkBlockAct& a = p->blk[b];
        const float* B = P + L.blk0 + (size_t)b * L.blk_size;
        hipLaunchKernelGGL(k_xk_rowflag, dim3((M + 3) / 4), dim3(256), 0, st, X, a.flag, M, D);
        if ((rc = launch_gemm_f32(X, D, B + L.bo[XB_WQ], D, B + L.bo[XB_BQ], a.Q, D, M, D, D, ACT_RELU, st))) return rc;
        if ((rc = launch_gemm_f32(X, D, B + L.bo[XB_WK], D, B + L.bo[XB_BK], a.K, D, M, D, D, ACT_RELU, st))) return rc;
        if ((rc = launch_gemm_f32(X, D, B + L.bo[XB_WV], D, B + L.bo[XB_BV], a.V, D, M, D, D, ACT_RELU, st))) return rc;
        hipLaunchKernelGGL(k_xk_attn_fwd, dim3(N * d.heads), dim3(256), lds_a, st, a.Q, a.K, a.V, a.flag, a.P, p->AO, A, D, d.heads, d.dh,
                           rate, seed, step, site0 + 1u + (uint32_t)b);
        hipLaunchKernelGGL(k_xk_add_ln, dim3((M + 3) / 4), dim3(256), 0, st, p->AO, X, B + L.bo[XB_G1], B + L.bo[XB_B1], a.Y, a.xhat1,
                           a.rstd1, M, D);
        if ((rc = launch_gemm_f32(a.Y, D, B + L.bo[XB_W1], F, B + L.bo[XB_BF1], a.Hf, F, M, F, D, ACT_RELU, st))) return rc;
        if ((rc = launch_gemm_f32(a.Hf, F, B + L.bo[XB_W2], D, B + L.bo[XB_BF2], p->Z, D, M, D, F, ACT_NONE, st, a.Y, D, 1))) return rc;
        hipLaunchKernelGGL(k_xk_add_ln, dim3((M + 3) / 4), dim3(256), 0, st, p->Z, (const float*)nullptr, B + L.bo[XB_G2], B + L.bo[XB_B2],
                           a.Xout, a.xhat2, a.rstd2, M, D);
        X = a.Xout;
    }
    RL4RS_LAUNCH_CHECK();
    if ((rc = launch_gemm_f32(X, D, P + L.a_wref[0], D, nullptr, p->Rg, D, M, D, D, ACT_NONE, st))) return rc;
    if ((rc = launch_gemm_f32(X, D, P + L.a_wref[1], D, nullptr, p->Rp, D, M, D, D, ACT_NONE, st))) return rc;
    *enc_out = X;
    return RL4RS_OK;
}

// encoder + decoder forward.  mode 0 sample / 1 greedy (path written) / 2 teacher-forced (path read; ce, dlogit written)
static int xk_forward(rl4rs_exactk* p, int N, const float* obs, int mode, int32_t* path, const float* w, uint32_t seed, uint32_t step,
                      uint32_t pass, float* logits_out, hipStream_t st) {
    const XkDims& d = p->d;
    const XkLayout& L = p->L;
    const float* P = p->opt.params;
    const int A = d.A, D = d.D;
    int rc;
    const float* enc = nullptr;
    if ((rc = xk_encode(p, N, obs, seed, step, pass, &enc, st))) return rc;
    const size_t lds_d = xk_dec_lds(d);
    if ((rc = raise_dyn_smem(reinterpret_cast<const void*>(&k_xk_glimpse_fwd), lds_d))) return rc;
    if ((rc = raise_dyn_smem(reinterpret_cast<const void*>(&k_xk_pointer_fwd), lds_d))) return rc;
    const size_t ND = (size_t)N * D;
    for (int t = 0; t < XK_T; ++t) {
        float* XHt = p->XH + (size_t)t * N * 2 * D;
        float* Gt = p->G + (size_t)t * N * 4 * D;
        float* Ht = p->Hout + t * ND;
        float* It = p->intra + t * ND;
        hipLaunchKernelGGL(k_xk_gather_x, ew(ND), dim3(256), 0, st, t, N, A, D, enc, path, P + L.first, P + L.init_h, XHt);
        if ((rc = launch_gemm_f32(XHt, 2 * D, P + L.wl, 4 * D, P + L.bl, Gt, 4 * D, N, 4 * D, 2 * D, ACT_NONE, st))) return rc;
        hipLaunchKernelGGL(k_xk_cell_fwd, ew(ND), dim3(256), 0, st, N, D, Gt, t == 0 ? P + L.init_c : p->C + (t - 1) * ND, t == 0 ? 0 : D,
                           p->C + t * ND, Ht, t + 1 < XK_T ? XHt + (size_t)N * 2 * D : (float*)nullptr);
        if ((rc = launch_gemm_f32(Ht, D, P + L.ia_wbef, D, nullptr, p->Bef + t * ND, D, N, D, D, ACT_NONE, st))) return rc;
        if ((rc = launch_gemm_f32(Ht, D, P + L.ia_wb, D, P + L.ia_bias, p->Qb + t * ND, D, N, D, D, ACT_NONE, st))) return rc;
        hipLaunchKernelGGL(k_xk_intra_fwd, dim3(N), dim3(256), 0, st, t, N, D, p->Bef, p->Qb, p->Hout, P + L.ia_v, p->pI, p->intra);
        // glimpse
        if ((rc = launch_gemm_f32(Ht, D, P + L.a_wq[0], D, P + L.a_bias[0], p->tmp1, D, N, D, D, ACT_NONE, st))) return rc;
        if ((rc = launch_gemm_f32(It, D, P + L.a_wdec[0], D, nullptr, p->Cg + t * ND, D, N, D, D, ACT_NONE, st, p->tmp1, D, 1))) return rc;
        hipLaunchKernelGGL(k_xk_glimpse_fwd, dim3(N), dim3(256), lds_d, st, N, A, D, p->Rg, p->Cg + t * ND, P + L.a_v[0], enc,
                           p->pg + (size_t)t * N * A, p->q + t * ND);
        // pointer
        if ((rc = launch_gemm_f32(p->q + t * ND, D, P + L.a_wq[1], D, P + L.a_bias[1], p->tmp1, D, N, D, D, ACT_NONE, st))) return rc;
        if ((rc = launch_gemm_f32(It, D, P + L.a_wdec[1], D, nullptr, p->Cp + t * ND, D, N, D, D, ACT_NONE, st, p->tmp1, D, 1))) return rc;
        hipLaunchKernelGGL(k_xk_pointer_fwd, dim3(N), dim3(256), lds_d, st, t, N, A, D, p->Rp, p->Cp + t * ND, P + L.a_v[1], p->loc,
                           p->special, path, mode, seed, step, logits_out, mode == 2 ? p->dlogit + (size_t)t * N * A : (float*)nullptr, w,
                           p->ce + (size_t)t * N, p->invalid + (size_t)t * N);
    }
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

// LDS of the per-user beam kernels for `beam` live beams (the glimpse kernel's, the larger of the two)
static size_t xk_beam_lds(const XkDims& d, int beam) {
    return ((size_t)beam * d.A + (size_t)beam * d.D + d.D + 16 + (size_t)beam * std::max(d.D, 256)) * 4;
}

// carve the beam scratch for rows = N * beam decoder rows, (re)allocating when the call needs more than the handle holds
static int xk_beam_reserve(rl4rs_exactk* p, size_t rows) {
    XkBeamScratch& s = p->beam;
    const size_t D = p->d.D, T = XK_T;
    std::vector<std::pair<void**, size_t>> reqs;
    auto req = [&](auto** slot, size_t n) { reqs.emplace_back(reinterpret_cast<void**>(slot), n * sizeof(**slot)); };
    req(&s.XH, rows * 2 * D); req(&s.G, rows * 4 * D); req(&s.C, rows * D); req(&s.Cin, rows * D); req(&s.Hout, T * rows * D);
    req(&s.Bef, T * rows * D); req(&s.Qb, rows * D); req(&s.intra, rows * D); req(&s.tmp1, rows * D); req(&s.Cg, rows * D);
    req(&s.q, rows * D); req(&s.Cp, rows * D);
    for (int k = 0; k < 2; ++k) { req(&s.acc[k], rows); req(&s.prefix[k], rows * T); req(&s.anc[k], rows * T); }
    size_t total = 0;
    for (auto& r : reqs) total += (r.second + 255) / 256 * 256;
    if (total > s.bytes) {
        if (s.mem) (void)hipFree(s.mem);           // (waits for the work that still reads it)
        s.mem = nullptr;
        s.bytes = 0;
        hipError_t e = hipMalloc(&s.mem, total);
        if (e != hipSuccess) {
            set_error("exactk_decode_beam: hipMalloc(%zu bytes) failed: %s", total, hipGetErrorString(e));
            s.mem = nullptr;
            return RL4RS_ENOMEM;
        }
        s.bytes = total;
    }
    size_t off = 0;
    for (auto& r : reqs) { *r.first = static_cast<char*>(s.mem) + off; off += (r.second + 255) / 256 * 256; }
    return RL4RS_OK;
}

// encoder (pass 1, as rl4rs_exactk_decode) + beam search over the decoder: rows r = n * live + b, live = 1 at step 0, B afterwards
static int xk_beam_forward(rl4rs_exactk* p, int N, const float* obs, int B, uint32_t seed, uint32_t step, int32_t* path, float* score,
                           int32_t* parent_tr, int32_t* token_tr, float* score_tr, hipStream_t st) {
    const XkDims& d = p->d;
    const XkLayout& L = p->L;
    const float* P = p->opt.params;
    const int A = d.A, D = d.D, NB = N * B;
    int rc;
    if ((rc = xk_beam_reserve(p, (size_t)NB))) return rc;
    XkBeamScratch& s = p->beam;
    const float* enc = nullptr;
    if ((rc = xk_encode(p, N, obs, seed, step, 1u, &enc, st))) return rc;
    const size_t lds = xk_beam_lds(d, B);
    if ((rc = raise_dyn_smem(reinterpret_cast<const void*>(&k_xk_beam_glimpse), lds))) return rc;
    if ((rc = raise_dyn_smem(reinterpret_cast<const void*>(&k_xk_beam_select), lds))) return rc;
    for (int t = 0; t < XK_T; ++t) {
        const int live = t == 0 ? 1 : B, rows = N * live;
        const int in = t & 1, out = in ^ 1;                    // ping-pong of prefix / acc / anc: step t reads [in], writes [out]
        const size_t RD = (size_t)rows * D;
        float* Ht = s.Hout + (size_t)t * NB * D;
        float* Bt = s.Bef + (size_t)t * NB * D;
        if (t == 0)
            hipLaunchKernelGGL(k_xk_gather_x, ew(RD), dim3(256), 0, st, 0, rows, A, D, enc, (const int32_t*)nullptr, P + L.first, P + L.init_h,
                               s.XH);
        else
            hipLaunchKernelGGL(k_xk_beam_gather, ew(RD), dim3(256), 0, st, t, rows, B, NB, A, D, enc, s.prefix[in], s.anc[in],
                               s.Hout + (size_t)(t - 1) * NB * D, s.C, s.XH, s.Cin);
        if ((rc = launch_gemm_f32(s.XH, 2 * D, P + L.wl, 4 * D, P + L.bl, s.G, 4 * D, rows, 4 * D, 2 * D, ACT_NONE, st))) return rc;
        hipLaunchKernelGGL(k_xk_cell_fwd, ew(RD), dim3(256), 0, st, rows, D, s.G, t == 0 ? P + L.init_c : s.Cin, t == 0 ? 0 : D, s.C, Ht,
                           (float*)nullptr);
        if ((rc = launch_gemm_f32(Ht, D, P + L.ia_wbef, D, nullptr, Bt, D, rows, D, D, ACT_NONE, st))) return rc;
        if ((rc = launch_gemm_f32(Ht, D, P + L.ia_wb, D, P + L.ia_bias, s.Qb, D, rows, D, D, ACT_NONE, st))) return rc;
        hipLaunchKernelGGL(k_xk_beam_intra, dim3(rows), dim3(256), 0, st, t, NB, D, s.Bef, s.Qb, s.Hout, s.anc[in], P + L.ia_v, s.intra);
        // glimpse
        if ((rc = launch_gemm_f32(Ht, D, P + L.a_wq[0], D, P + L.a_bias[0], s.tmp1, D, rows, D, D, ACT_NONE, st))) return rc;
        if ((rc = launch_gemm_f32(s.intra, D, P + L.a_wdec[0], D, nullptr, s.Cg, D, rows, D, D, ACT_NONE, st, s.tmp1, D, 1))) return rc;
        hipLaunchKernelGGL(k_xk_beam_glimpse, dim3(N), dim3(256), lds, st, A, D, live, p->Rg, s.Cg, P + L.a_v[0], enc, s.q);
        // pointer, selection and the new beams' prefixes / ancestor rows; the last step writes the caller's arrays
        if ((rc = launch_gemm_f32(s.q, D, P + L.a_wq[1], D, P + L.a_bias[1], s.tmp1, D, rows, D, D, ACT_NONE, st))) return rc;
        if ((rc = launch_gemm_f32(s.intra, D, P + L.a_wdec[1], D, nullptr, s.Cp, D, rows, D, D, ACT_NONE, st, s.tmp1, D, 1))) return rc;
        const bool last = t + 1 == XK_T;
        hipLaunchKernelGGL(k_xk_beam_select, dim3(N), dim3(256), lds, st, t, A, D, live, B, NB, p->Rp, s.Cp, P + L.a_v[1], p->loc, p->special,
                           s.prefix[in], s.acc[in], s.anc[in], last ? path : s.prefix[out], last ? score : s.acc[out], s.anc[out], parent_tr,
                           token_tr, score_tr);
    }
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

static int xk_backward(rl4rs_exactk* p, int N, const float* obs, const int32_t* path, uint32_t seed, uint32_t step, uint32_t pass,
                       hipStream_t st) {
    const XkDims& d = p->d;
    const XkLayout& L = p->L;
    const float* P = p->opt.params;
    float* Gd = p->opt.grad;
    const int A = d.A, D = d.D, H = d.H, F = d.F, M = N * A, TN = XK_T * N;
    const float rate = p->c.dropout_rate;
    const uint32_t site0 = pass * 32u;
    const size_t ND = (size_t)N * D, MD = (size_t)M * D;
    int rc;
    const float* enc = p->blk[d.blocks - 1].Xout;
    RL4RS_HIP_TRY(hipMemsetAsync(p->dEnc, 0, MD * 4, st));
    RL4RS_HIP_TRY(hipMemsetAsync(p->dRg, 0, MD * 4, st));
    RL4RS_HIP_TRY(hipMemsetAsync(p->dRp, 0, MD * 4, st));
    RL4RS_HIP_TRY(hipMemsetAsync(p->dHacc, 0, XK_T * ND * 4, st));
    RL4RS_HIP_TRY(hipMemsetAsync(p->dBefAcc, 0, XK_T * ND * 4, st));
    RL4RS_HIP_TRY(hipMemsetAsync(p->dQb, 0, XK_T * ND * 4, st));
    RL4RS_HIP_TRY(hipMemsetAsync(p->dvd, 0, XK_T * ND * 4, st));
    RL4RS_HIP_TRY(hipMemsetAsync(p->dCnext, 0, ND * 4, st));
    const size_t lds_d = xk_dec_lds(d);
    if ((rc = raise_dyn_smem(reinterpret_cast<const void*>(&k_xk_glimpse_bwd), lds_d))) return rc;
    if ((rc = raise_dyn_smem(reinterpret_cast<const void*>(&k_xk_pointer_bwd), lds_d))) return rc;
    for (int t = XK_T - 1; t >= 0; --t) {
        float* dCpt = p->dCp + t * ND;
        float* dCgt = p->dCg + t * ND;
        hipLaunchKernelGGL(k_xk_pointer_bwd, dim3(N), dim3(256), lds_d, st, N, A, D, p->Rp, p->dRp, p->Cp + t * ND, P + L.a_v[1],
                           p->dlogit + (size_t)t * N * A, dCpt, p->dvp + t * ND);
        if ((rc = launch_gemm_nt(dCpt, D, P + L.a_wq[1], D, p->dq, D, N, D, D, st))) return rc;
        if ((rc = launch_gemm_nt(dCpt, D, P + L.a_wdec[1], D, p->dI1, D, N, D, D, st))) return rc;
        hipLaunchKernelGGL(k_xk_glimpse_bwd, dim3(N), dim3(256), lds_d, st, N, A, D, p->Rg, p->dRg, p->Cg + t * ND, P + L.a_v[0],
                           p->pg + (size_t)t * N * A, p->dq, enc, p->dEnc, dCgt, p->dvg + t * ND);
        if ((rc = launch_gemm_nt(dCgt, D, P + L.a_wq[0], D, p->pc2, D, N, D, D, st))) return rc;
        if ((rc = launch_gemm_nt(dCgt, D, P + L.a_wdec[0], D, p->dI2, D, N, D, D, st))) return rc;
        if (t >= 1)
            hipLaunchKernelGGL(k_xk_intra_bwd, dim3(N), dim3(256), 0, st, t, N, D, p->dI1, p->dI2, p->pI, p->Hout, p->Bef, p->Qb, P + L.ia_v,
                               p->dHacc, p->dBefAcc, p->dQb, p->dvd);
        if ((rc = launch_gemm_nt(p->dQb + t * ND, D, P + L.ia_wb, D, p->pc1, D, N, D, D, st))) return rc;
        if ((rc = launch_gemm_nt(p->dBefAcc + t * ND, D, P + L.ia_wbef, D, p->pc0, D, N, D, D, st))) return rc;
        float* dGt = p->dG + (size_t)t * N * 4 * D;
        hipLaunchKernelGGL(k_xk_cell_bwd, ew(ND), dim3(256), 0, st, N, D, p->dHacc + t * ND, p->pc0, p->pc1, p->pc2,
                           t + 1 < XK_T ? p->dXH : (const float*)nullptr, p->G + (size_t)t * N * 4 * D,
                           t == 0 ? P + L.init_c : p->C + (t - 1) * ND, t == 0 ? 0 : D, p->C + t * ND, p->dCnext, dGt);
        if ((rc = launch_gemm_nt(dGt, 4 * D, P + L.wl, 4 * D, p->dXH, 2 * D, N, 2 * D, 4 * D, st))) return rc;
        hipLaunchKernelGGL(k_xk_input_bwd, ew(ND), dim3(256), 0, st, t, N, A, D, p->dXH, p->dCnext, path, p->dEnc, p->part3);
    }
    RL4RS_LAUNCH_CHECK();
    // decoder parameter gradients: one reduction over the 9 N (step, row) pairs each
    if ((rc = xk_tn(p, p->q, D, D, p->dCp, D, D, TN, Gd + L.a_wq[1], Gd + L.a_bias[1], st))) return rc;
    if ((rc = xk_tn(p, p->intra, D, D, p->dCp, D, D, TN, Gd + L.a_wdec[1], nullptr, st))) return rc;
    if ((rc = xk_tn(p, p->Hout, D, D, p->dCg, D, D, TN, Gd + L.a_wq[0], Gd + L.a_bias[0], st))) return rc;
    if ((rc = xk_tn(p, p->intra, D, D, p->dCg, D, D, TN, Gd + L.a_wdec[0], nullptr, st))) return rc;
    if ((rc = xk_tn(p, p->Hout, D, D, p->dQb, D, D, TN, Gd + L.ia_wb, Gd + L.ia_bias, st))) return rc;
    if ((rc = xk_tn(p, p->Hout, D, D, p->dBefAcc, D, D, TN, Gd + L.ia_wbef, nullptr, st))) return rc;
    if ((rc = xk_tn(p, p->XH, 2 * D, 2 * D, p->dG, 4 * D, 4 * D, TN, Gd + L.wl, Gd + L.bl, st))) return rc;
    if ((rc = xk_colsum(p, p->dvp, nullptr, D, D, TN, Gd + L.a_v[1], st))) return rc;
    if ((rc = xk_colsum(p, p->dvg, nullptr, D, D, TN, Gd + L.a_v[0], st))) return rc;
    if ((rc = xk_colsum(p, p->dvd, nullptr, D, D, TN, Gd + L.ia_v, st))) return rc;
    if ((rc = xk_colsum(p, p->part3, nullptr, D, D, N, Gd + L.init_c, st))) return rc;
    if ((rc = xk_colsum(p, p->part3 + ND, nullptr, D, D, N, Gd + L.init_h, st))) return rc;
    if ((rc = xk_colsum(p, p->part3 + 2 * ND, nullptr, D, D, N, Gd + L.first, st))) return rc;
    if ((rc = xk_tn(p, enc, D, D, p->dRg, D, D, M, Gd + L.a_wref[0], nullptr, st))) return rc;
    if ((rc = xk_tn(p, enc, D, D, p->dRp, D, D, M, Gd + L.a_wref[1], nullptr, st))) return rc;
    if ((rc = launch_gemm_nt(p->dRg, D, P + L.a_wref[0], D, p->tA, D, M, D, D, st))) return rc;
    if ((rc = launch_gemm_nt(p->dRp, D, P + L.a_wref[1], D, p->tB, D, M, D, D, st))) return rc;
    hipLaunchKernelGGL(k_xk_add, ew(MD), dim3(256), 0, st, p->dEnc, p->tA, p->tB, MD);
    // encoder, last block first; dX = gradient of the block's output
    const size_t lds_a = xk_attn_lds(d), lds_tn = (size_t)A * d.dh * 4;
    if ((rc = raise_dyn_smem(reinterpret_cast<const void*>(&k_xk_attn_bwd_q), lds_a))) return rc;
    if ((rc = raise_dyn_smem(reinterpret_cast<const void*>(&k_xk_attn_tn<true>), lds_tn))) return rc;
    if ((rc = raise_dyn_smem(reinterpret_cast<const void*>(&k_xk_attn_tn<false>), lds_tn))) return rc;
    float* dX = p->dEnc;
    for (int b = d.blocks - 1; b >= 0; --b) {
        XkBlockAct& a = p->blk[b];
        const float* B = P + L.blk0 + (size_t)b * L.blk_size;
        float* GB = Gd + L.blk0 + (size_t)b * L.blk_size;
        const float* Xin = b == 0 ? p->X0 : p->blk[b - 1].Xout;
        const uint32_t site = site0 + 1u + (uint32_t)b;
        // layer norm 2: dZ -> dA
        if ((rc = xk_colsum(p, dX, a.xhat2, D, D, M, GB + L.bo[XB_G2], st))) return rc;
        if ((rc = xk_colsum(p, dX, nullptr, D, D, M, GB + L.bo[XB_B2], st))) return rc;
        hipLaunchKernelGGL(k_xk_ln_bwd, dim3((M + 3) / 4), dim3(256), 0, st, dX, a.xhat2, a.rstd2, B + L.bo[XB_G2], (const float*)nullptr,
                           p->dA, M, D);
        // feed-forward: Z = Hf W2 + b2 + Y
        if ((rc = xk_tn(p, a.Hf, F, F, p->dA, D, D, M, GB + L.bo[XB_W2], GB + L.bo[XB_BF2], st))) return rc;
        if ((rc = launch_gemm_nt(p->dA, D, B + L.bo[XB_W2], D, p->dF, F, M, F, D, st, a.Hf, F))) return rc;
        if ((rc = xk_tn(p, a.Y, D, D, p->dF, F, F, M, GB + L.bo[XB_W1], GB + L.bo[XB_BF1], st))) return rc;
        if ((rc = launch_gemm_nt(p->dF, F, B + L.bo[XB_W1], F, p->tA, D, M, D, F, st))) return rc;
        hipLaunchKernelGGL(k_xk_add, ew(MD), dim3(256), 0, st, p->dA, p->tA, (const float*)nullptr, MD);          // dA = dY
        // layer norm 1: dS (= d attention output = residual gradient of X) -> dB
        if ((rc = xk_colsum(p, p->dA, a.xhat1, D, D, M, GB + L.bo[XB_G1], st))) return rc;
        if ((rc = xk_colsum(p, p->dA, nullptr, D, D, M, GB + L.bo[XB_B1], st))) return rc;
        hipLaunchKernelGGL(k_xk_ln_bwd, dim3((M + 3) / 4), dim3(256), 0, st, p->dA, a.xhat1, a.rstd1, B + L.bo[XB_G1], (const float*)nullptr,
                           p->dB, M, D);
        // attention: dV (needs P before it is overwritten), then dS over P and dQ, then dK; relu masks folded in
        hipLaunchKernelGGL(k_xk_attn_tn<true>, dim3(N * d.heads), dim3(256), lds_tn, st, a.P, p->dB, a.V, a.flag, p->dC3, A, D, d.heads, d.dh,
                           rate, seed, step, site);
        hipLaunchKernelGGL(k_xk_attn_bwd_q, dim3(N * d.heads), dim3(256), lds_a, st, a.Q, a.K, a.V, p->dB, a.flag, a.P, p->dA, A, D, d.heads,
                           d.dh, rate, seed, step, site);                                                         // dA = dQ
        hipLaunchKernelGGL(k_xk_attn_tn<false>, dim3(N * d.heads), dim3(256), lds_tn, st, a.P, a.Q, a.K, a.flag, p->dF, A, D, d.heads, d.dh,
                           0.f, 0u, 0u, 0u);                                                                      // dF[:, :D] = dK (ld D)
        RL4RS_LAUNCH_CHECK();
        if ((rc = xk_tn(p, Xin, D, D, p->dA, D, D, M, GB + L.bo[XB_WQ], GB + L.bo[XB_BQ], st))) return rc;
        if ((rc = xk_tn(p, Xin, D, D, p->dF, D, D, M, GB + L.bo[XB_WK], GB + L.bo[XB_BK], st))) return rc;
        if ((rc = xk_tn(p, Xin, D, D, p->dC3, D, D, M, GB + L.bo[XB_WV], GB + L.bo[XB_BV], st))) return rc;
        // d X_in = dS (residual) + dQ Wq^T + dK Wk^T + dV Wv^T
        if ((rc = launch_gemm_nt(p->dA, D, B + L.bo[XB_WQ], D, p->tA, D, M, D, D, st))) return rc;
        if ((rc = launch_gemm_nt(p->dF, D, B + L.bo[XB_WK], D, p->tB, D, M, D, D, st))) return rc;
        hipLaunchKernelGGL(k_xk_add, ew(MD), dim3(256), 0, st, p->dB, p->tA, p->tB, MD);
        if ((rc = launch_gemm_nt(p->dC3, D, B + L.bo[XB_WV], D, p->tA, D, M, D, D, st))) return rc;
        hipLaunchKernelGGL(k_xk_add, ew(MD), dim3(256), 0, st, p->dB, p->tA, (const float*)nullptr, MD);
        dX = p->dB;                       // read by the next block's first layer-norm backward before dB is written again
    }
    // input: dropout, the user layer and the item table (its first A rows; the others keep the zero of the memset)
    hipLaunchKernelGGL(k_xk_build_enc_bwd, ew((size_t)(N + A) * H), dim3(256), 0, st, dX, p->dEU, p->EU, Gd + L.table, N, A, H,
                       sqrtf((float)H), rate, seed, step, site0);
    RL4RS_LAUNCH_CHECK();
    return xk_tn(p, obs, d.OD, d.OD, p->dEU, H, H, N, Gd + L.wu, Gd + L.bu, st);
}

extern "C" {

int64_t rl4rs_exactk_param_count(const rl4rs_exactk_cfg* cfg) {
    XkDims d;
    if (xk_check_cfg(cfg, &d)) return -1;
    return (int64_t)xk_layout(d).total;
}

int rl4rs_exactk_destroy(rl4rs_exactk* p) {
    if (!p) return RL4RS_OK;
    if (p->arena) (void)hipFree(p->arena);
    if (p->beam.mem) (void)hipFree(p->beam.mem);
    delete p;
    return RL4RS_OK;
}

int rl4rs_exactk_create(const rl4rs_exactk_cfg* cfg, const float* params_host, const uint8_t* location_mask, const uint8_t* is_special,
                        void* stream, rl4rs_exactk** out) {
    XkDims d;
    int rc = xk_check_cfg(cfg, &d);
    if (rc) return rc;
    RL4RS_REQUIRE(params_host && location_mask && is_special && out, "exactk_create: null argument");
    *out = nullptr;
    for (int l = 0; l < 3; ++l) {
        int usable = 0;
        for (int a = 0; a < d.A; ++a) usable += (location_mask[l * d.A + a] && !is_special[a]) ? 1 : 0;
        RL4RS_REQUIRE(usable >= XK_T, "exactk_create: location mask %d allows %d non-special items, fewer than the 9 that keep every "
                      "position's allowed set non-empty", l, usable);
    }
    if (rl4rs_device_count() <= 0) {
        set_error("no HIP device visible: librl4rs_hip has no CPU fallback");
        return RL4RS_EHIP;
    }
    rl4rs_exactk* p = new rl4rs_exactk();
    p->c = *cfg; p->d = d; p->L = xk_layout(d);
    p->opt.n = (int64_t)p->L.total; p->opt.t = 0; p->arena = nullptr;
    p->blk.resize(d.blocks);
    const size_t R = (size_t)cfg->max_rows, A = d.A, D = d.D, F = d.F, M = R * A, MD = M * D, ND = R * D, np = p->L.total, T = XK_T;
    std::vector<std::pair<void**, size_t>> reqs;                 // (pointer slot, bytes)
    auto req = [&](auto** slot, size_t n) { reqs.emplace_back(reinterpret_cast<void**>(slot), n * sizeof(**slot)); };
    req(&p->opt.params, np); req(&p->opt.grad, np); req(&p->opt.m, np); req(&p->opt.v, np);
    req(&p->loc, 3 * A); req(&p->special, A);
    req(&p->EU, R * d.H); req(&p->dEU, R * d.H); req(&p->X0, MD); req(&p->AO, MD); req(&p->Z, MD);
    for (auto& b : p->blk) {
        req(&b.Q, MD); req(&b.K, MD); req(&b.V, MD); req(&b.P, R * d.heads * A * A); req(&b.xhat1, MD); req(&b.rstd1, M); req(&b.Y, MD);
        req(&b.Hf, M * F); req(&b.xhat2, MD); req(&b.rstd2, M); req(&b.Xout, MD); req(&b.flag, M);
    }
    req(&p->Rg, MD); req(&p->Rp, MD); req(&p->XH, T * R * 2 * D); req(&p->G, T * R * 4 * D); req(&p->C, T * ND); req(&p->Hout, T * ND);
    req(&p->Bef, T * ND); req(&p->Qb, T * ND); req(&p->intra, T * ND); req(&p->pI, T * R * T); req(&p->Cg, T * ND); req(&p->pg, T * M);
    req(&p->q, T * ND); req(&p->Cp, T * ND); req(&p->tmp1, ND); req(&p->dlogit, T * M); req(&p->ce, T * R); req(&p->invalid, T * R);
    req(&p->dEnc, MD); req(&p->dRg, MD); req(&p->dRp, MD); req(&p->dCp, T * ND); req(&p->dCg, T * ND); req(&p->dq, ND); req(&p->dI1, ND);
    req(&p->dI2, ND); req(&p->dHacc, T * ND); req(&p->dBefAcc, T * ND); req(&p->dQb, T * ND); req(&p->dvp, T * ND); req(&p->dvg, T * ND);
    req(&p->dvd, T * ND); req(&p->pc0, ND); req(&p->pc1, ND); req(&p->pc2, ND); req(&p->dCnext, ND); req(&p->dG, T * R * 4 * D);
    req(&p->dXH, R * 2 * D); req(&p->part3, 3 * ND); req(&p->dA, MD); req(&p->dB, MD); req(&p->dC3, MD); req(&p->dF, M * F);
    req(&p->tA, MD); req(&p->tB, MD); req(&p->path_tmp, R * T);
    p->chunk_cap = 64;
    const size_t widest = std::max(std::max((size_t)d.OD * d.H, 8 * D * D), D * F);
    req(&p->part, (size_t)p->chunk_cap * widest); req(&p->part_b, (size_t)XK_COLSUM_CHUNKS * 4 * D);
    size_t total = 0;
    for (auto& r : reqs) total += (r.second + 255) / 256 * 256;
    hipError_t e = hipMalloc(&p->arena, total);
    if (e != hipSuccess) {
        set_error("exactk_create: hipMalloc(%zu bytes) failed: %s", total, hipGetErrorString(e));
        p->arena = nullptr;
        rl4rs_exactk_destroy(p);
        return RL4RS_ENOMEM;
    }
    size_t off = 0;
    for (auto& r : reqs) { *r.first = static_cast<char*>(p->arena) + off; off += (r.second + 255) / 256 * 256; }
    hipStream_t st = (hipStream_t)stream;
    e = hipMemcpyAsync(p->opt.params, params_host, np * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(p->loc, location_mask, 3 * A, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(p->special, is_special, A, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(p->opt.grad, 0, np * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(p->opt.m, 0, np * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(p->opt.v, 0, np * 4, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        set_error("exactk_create: initialisation failed: %s", hipGetErrorString(e));
        rl4rs_exactk_destroy(p);
        return RL4RS_EHIP;
    }
    *out = p;
    return RL4RS_OK;
}

int rl4rs_exactk_params(rl4rs_exactk* p, float** params_dev, float** grad_dev, int64_t* count) {
    return opt_params(RL4RS_OPT(p), params_dev, grad_dev, count, "exactk_params");
}
int rl4rs_exactk_adam_state(rl4rs_exactk* p, float** m_dev, float** v_dev, int64_t* step) {
    return opt_adam_state(RL4RS_OPT(p), m_dev, v_dev, step, "exactk_adam_state");
}
int rl4rs_exactk_set_adam_step(rl4rs_exactk* p, int64_t step) {
    return opt_set_adam_step(RL4RS_OPT(p), step, "exactk_set_adam_step");
}

int rl4rs_exactk_decode(rl4rs_exactk* p, int32_t N, const float* obs_dev, int32_t greedy, uint32_t seed, uint32_t step, int32_t* path_dev,
                        float* logits_out_dev, void* stream) {
    RL4RS_REQUIRE(p && obs_dev && path_dev && N > 0 && N <= p->c.max_rows, "exactk_decode: bad argument (N=%d, max_rows=%d)", N,
                  p ? p->c.max_rows : -1);
    return xk_forward(p, N, obs_dev, greedy ? 1 : 0, path_dev, nullptr, seed, step, 1u, logits_out_dev, (hipStream_t)stream);
}

int rl4rs_exactk_decode_beam(rl4rs_exactk* p, int32_t N, const float* obs_dev, int32_t beam, uint32_t seed, uint32_t step, int32_t* path_dev,
                             float* score_dev, int32_t* parent_dev, int32_t* token_dev, float* step_score_dev, void* stream) {
    RL4RS_REQUIRE(p && obs_dev, "exactk_decode_beam: null handle or observations");
    RL4RS_REQUIRE(beam >= 1 && beam <= XK_BEAM_MAX, "exactk_decode_beam: beam %d outside [1, %d]", beam, XK_BEAM_MAX);
    RL4RS_REQUIRE(N >= 1 && N <= p->c.max_rows, "exactk_decode_beam: N %d outside [1, max_rows = %d]", N, p->c.max_rows);
    RL4RS_REQUIRE(path_dev && score_dev, "exactk_decode_beam: null output (path_dev, score_dev)");
    const size_t lds = xk_beam_lds(p->d, beam);
    RL4RS_REQUIRE(lds <= XK_LDS_MAX, "exactk_decode_beam: beam %d over action_size %d, width %d needs %zu bytes of LDS per workgroup "
                  "(limit %zu)", beam, p->d.A, p->d.D, lds, XK_LDS_MAX);
    return xk_beam_forward(p, N, obs_dev, beam, seed, step, path_dev, score_dev, parent_dev, token_dev, step_score_dev, (hipStream_t)stream);
}

int rl4rs_exactk_loss_grad(rl4rs_exactk* p, int32_t N, const float* obs_dev, const int32_t* path_dev, const float* weights_dev, uint32_t seed,
                           uint32_t step, float* logits_out_dev, float* loss_dev, void* stream) {
    RL4RS_REQUIRE(p && obs_dev && path_dev && weights_dev && loss_dev && N > 0 && N <= p->c.max_rows,
                  "exactk_loss_grad: bad argument (N=%d, max_rows=%d)", N, p ? p->c.max_rows : -1);
    hipStream_t st = (hipStream_t)stream;
    RL4RS_HIP_TRY(hipMemcpyAsync(p->path_tmp, path_dev, (size_t)N * XK_T * 4, hipMemcpyDeviceToDevice, st));
    int rc = xk_forward(p, N, obs_dev, 2, p->path_tmp, weights_dev, seed, step, 0u, logits_out_dev, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_xk_loss, dim3(1), dim3(256), 0, st, p->ce, p->invalid, weights_dev, N, loss_dev);
    RL4RS_HIP_TRY(hipMemsetAsync(p->opt.grad, 0, (size_t)p->opt.n * 4, st));
    return xk_backward(p, N, obs_dev, p->path_tmp, seed, step, 0u, st);
}

int rl4rs_exactk_adam_step(rl4rs_exactk* p, float lr, float beta1, float beta2, float eps, const int32_t* skip_dev, void* stream) {
    RL4RS_REQUIRE(p && lr >= 0.f, "exactk_adam_step: bad argument");
    // the step counter advances on the host whether or not the device flag skips the update: a skipped update keeps its slot
    adam_step(p->opt, p->opt.grad, ADAM_TF, lr, beta1, beta2, eps, nullptr, 0.f, skip_dev, (hipStream_t)stream);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

// ---------------------------------------------------------------- critic: obs -> HC relu -> HC relu -> HC relu -> 1
static void xkc_ptrs(const rl4rs_exactk_critic* c, float* base, float** W, float** b) {
    const size_t OD = c->OD, HC = c->HC;
    size_t o = 0;
    W[0] = base + o; o += OD * HC; b[0] = base + o; o += HC;
    W[1] = base + o; o += HC * HC; b[1] = base + o; o += HC;
    W[2] = base + o; o += HC * HC; b[2] = base + o; o += HC;
    W[3] = base + o; o += HC; b[3] = base + o;
}

int64_t rl4rs_exactk_critic_param_count(int32_t obs_dim, int32_t hidden) {
    if (obs_dim < 1 || hidden < 1) return -1;
    return (int64_t)obs_dim * hidden + hidden + 2 * ((int64_t)hidden * hidden + hidden) + hidden + 1;
}

int rl4rs_exactk_critic_destroy(rl4rs_exactk_critic* c) {
    if (!c) return RL4RS_OK;
    for (void* q : c->owned) (void)hipFree(q);
    delete c;
    return RL4RS_OK;
}

int rl4rs_exactk_critic_create(int32_t obs_dim, int32_t hidden, int32_t max_rows, const float* params_host, void* stream,
                               rl4rs_exactk_critic** out) {
    RL4RS_REQUIRE(params_host && out, "exactk_critic_create: null argument");
    RL4RS_REQUIRE(obs_dim >= 1 && obs_dim <= 65536 && hidden >= 1 && hidden <= 4096 && max_rows >= 1,
                  "exactk_critic_create: bad shape (obs_dim=%d, hidden=%d, max_rows=%d)", obs_dim, hidden, max_rows);
    RL4RS_REQUIRE((int64_t)max_rows * std::max(obs_dim, hidden) * 4 < ((int64_t)1 << 31),
                  "exactk_critic_create: max_rows %d: the activations would reach 2^31 bytes", max_rows);
    *out = nullptr;
    if (rl4rs_device_count() <= 0) {
        set_error("no HIP device visible: librl4rs_hip has no CPU fallback");
        return RL4RS_EHIP;
    }
    rl4rs_exactk_critic* c = new rl4rs_exactk_critic();
    c->OD = obs_dim; c->HC = hidden; c->max_rows = max_rows; c->opt.t = 0;
    c->opt.n = rl4rs_exactk_critic_param_count(obs_dim, hidden);
    int rc = RL4RS_OK;
    auto alloc = [&](float** dst, size_t n) {
        if (rc) return;
        rc = dev_alloc(dst, n);
        if (rc == RL4RS_OK) c->owned.push_back(*dst);
    };
    const size_t np = (size_t)c->opt.n, R = (size_t)max_rows, HC = (size_t)hidden;
    alloc(&c->opt.params, np); alloc(&c->opt.grad, np); alloc(&c->opt.m, np); alloc(&c->opt.v, np);
    for (int i = 0; i < 3; ++i) { alloc(&c->h[i], R * HC); alloc(&c->dh[i], R * HC); }
    alloc(&c->v, R); alloc(&c->dv, R);
    alloc(&c->part, 64 * std::max((size_t)obs_dim * HC, HC * HC)); alloc(&c->part_b, 64 * HC);
    if (rc) { rl4rs_exactk_critic_destroy(c); return rc; }
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(c->opt.params, params_host, np * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(c->opt.grad, 0, np * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(c->opt.m, 0, np * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(c->opt.v, 0, np * 4, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        set_error("exactk_critic_create: initialisation failed: %s", hipGetErrorString(e));
        rl4rs_exactk_critic_destroy(c);
        return RL4RS_EHIP;
    }
    *out = c;
    return RL4RS_OK;
}

int rl4rs_exactk_critic_params(rl4rs_exactk_critic* c, float** params_dev, float** grad_dev, int64_t* count) {
    return opt_params(RL4RS_OPT(c), params_dev, grad_dev, count, "exactk_critic_params");
}
int rl4rs_exactk_critic_adam_state(rl4rs_exactk_critic* c, float** m_dev, float** v_dev, int64_t* step) {
    return opt_adam_state(RL4RS_OPT(c), m_dev, v_dev, step, "exactk_critic_adam_state");
}
int rl4rs_exactk_critic_set_adam_step(rl4rs_exactk_critic* c, int64_t step) {
    return opt_set_adam_step(RL4RS_OPT(c), step, "exactk_critic_set_adam_step");
}

static int xkc_forward(rl4rs_exactk_critic* c, int N, const float* obs, float* out, hipStream_t st) {
    float *W[4], *b[4];
    xkc_ptrs(c, c->opt.params, W, b);
    const int HC = c->HC;
    int rc;
    if ((rc = launch_gemm_f32(obs, c->OD, W[0], HC, b[0], c->h[0], HC, N, HC, c->OD, ACT_RELU, st))) return rc;
    if ((rc = launch_gemm_f32(c->h[0], HC, W[1], HC, b[1], c->h[1], HC, N, HC, HC, ACT_RELU, st))) return rc;
    if ((rc = launch_gemm_f32(c->h[1], HC, W[2], HC, b[2], c->h[2], HC, N, HC, HC, ACT_RELU, st))) return rc;
    return launch_gemm_f32(c->h[2], HC, W[3], 1, b[3], out, 1, N, 1, HC, ACT_NONE, st);
}

int rl4rs_exactk_critic_forward(rl4rs_exactk_critic* c, int32_t N, const float* obs_dev, float* value_dev, void* stream) {
    RL4RS_REQUIRE(c && obs_dev && value_dev && N > 0 && N <= c->max_rows, "exactk_critic_forward: bad argument (N=%d, max_rows=%d)", N,
                  c ? c->max_rows : -1);
    return xkc_forward(c, N, obs_dev, value_dev, (hipStream_t)stream);
}

int rl4rs_exactk_critic_loss_grad(rl4rs_exactk_critic* c, int32_t N, const float* obs_dev, const float* target_dev, float* value_out_dev,
                                  float* err_out_dev, void* stream) {
    RL4RS_REQUIRE(c && obs_dev && target_dev && N > 0 && N <= c->max_rows, "exactk_critic_loss_grad: bad argument (N=%d, max_rows=%d)", N,
                  c ? c->max_rows : -1);
    hipStream_t st = (hipStream_t)stream;
    int rc = xkc_forward(c, N, obs_dev, c->v, st);
    if (rc) return rc;
    if (value_out_dev) RL4RS_HIP_TRY(hipMemcpyAsync(value_out_dev, c->v, (size_t)N * 4, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_xk_critic_err, ew((size_t)N), dim3(256), 0, st, c->v, target_dev, c->dv, err_out_dev, N);
    float *W[4], *b[4], *gW[4], *gb[4];
    xkc_ptrs(c, c->opt.params, W, b);
    xkc_ptrs(c, c->opt.grad, gW, gb);
    const int HC = c->HC;
    const int chunk = std::max(256, ((N + 63) / 64 + 15) / 16 * 16);
    if ((rc = launch_gemm_tn(c->h[2], HC, HC, c->dv, 1, 1, N, chunk, c->part, c->part_b, gW[3], gb[3], st))) return rc;
    if ((rc = launch_gemm_nt(c->dv, 1, W[3], 1, c->dh[2], HC, N, HC, 1, st, c->h[2], HC))) return rc;
    if ((rc = launch_gemm_tn(c->h[1], HC, HC, c->dh[2], HC, HC, N, chunk, c->part, c->part_b, gW[2], gb[2], st))) return rc;
    if ((rc = launch_gemm_nt(c->dh[2], HC, W[2], HC, c->dh[1], HC, N, HC, HC, st, c->h[1], HC))) return rc;
    if ((rc = launch_gemm_tn(c->h[0], HC, HC, c->dh[1], HC, HC, N, chunk, c->part, c->part_b, gW[1], gb[1], st))) return rc;
    if ((rc = launch_gemm_nt(c->dh[1], HC, W[1], HC, c->dh[0], HC, N, HC, HC, st, c->h[0], HC))) return rc;
    return launch_gemm_tn(obs_dev, c->OD, c->OD, c->dh[0], HC, HC, N, chunk, c->part, c->part_b, gW[0], gb[0], st);
}

int rl4rs_exactk_critic_adam_step(rl4rs_exactk_critic* c, float lr, float beta1, float beta2, float eps, void* stream) {
    RL4RS_REQUIRE(c && lr >= 0.f, "exactk_critic_adam_step: bad argument");
    adam_step(c->opt, c->opt.grad, ADAM_TF, lr, beta1, beta2, eps, nullptr, 0.f, nullptr, (hipStream_t)stream);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

}  // extern "C"
