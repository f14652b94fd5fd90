// The training pass of the MDP checker's seq2seq transformer: teacher-forced forward with dropout that keeps what the reverse pass
// needs, masked cross-entropy, the hand-written backward of every block, the two tables' row gradients.  Included by seq2seq.hip
// after its inference kernels and host helpers.
//
// Dropout sits where keras_transformer's block wrapper puts it, LayerNorm(x + Dropout(f(x))), one site per block: 0 encoder
// attention, 1 encoder ffn, 2 decoder self-attention, 3 decoder cross-attention, 4 decoder ffn.  An element (row, col) of a block's
// [rows, d] output is kept when uniform01(seed, step, row, site * 65536 + col) >= rate and then scaled by 1 / (1 - rate).
// Nothing is reduced with float atomics: weight gradients go through launch_gemm_tn (chunk partials summed in a fixed order), a
// table row's gradient is summed over the batch's positions in position order by one workgroup, so two identical calls give
// identical bits.  The tied decoder table gets two terms: the output layer's (dlogits^T h, written first) and the embedding's.
#pragma once

namespace {

constexpr int S2S_PA = 65;                     // saved attention row: 64 probabilities, then the arg-max key of the raw scores

__device__ __forceinline__ float s2s_keep(float rate, uint32_t seed, uint32_t step, uint32_t site, uint32_t row, uint32_t col) {
    if (rate <= 0.f) return 1.f;
    return uniform01(seed, step, row, site * 65536u + col) >= rate ? 1.f / (1.f - rate) : 0.f;
}

// k_s2s_add_ln with the dropout of R and the saved normalised rows: Y = gamma xhat + beta, xhat = (X + keep R - mean) rstd
__global__ __launch_bounds__(256) void k_s2s_add_ln_train(const float* __restrict__ X, const float* __restrict__ R,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float* __restrict__ Y, float* __restrict__ xhat, float* __restrict__ rstd, int M,
                                                          int D, float rate, uint32_t seed, uint32_t step, uint32_t site) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= M) return;
    const size_t o = (size_t)r * D;
    float s = 0.f;
    for (int d = lane; d < D; d += 64) {
        const float v = X[o + d] + R[o + d] * s2s_keep(rate, seed, step, site, (uint32_t)r, (uint32_t)d);
        xhat[o + d] = v;
        s += v;
    }
    const float mean = s2s_wave_sum(s) / (float)D;
    float v = 0.f;
    for (int d = lane; d < D; d += 64) {
        const float c = xhat[o + d] - mean;
        v += c * c;
    }
    const float rs = 1.f / sqrtf(s2s_wave_sum(v) / (float)D + S2S_LN_EPS);
    for (int d = lane; d < D; d += 64) {
        const float xh = (xhat[o + d] - mean) * rs;
        xhat[o + d] = xh;
        Y[o + d] = gamma[d] * xh + beta[d];
    }
    if (lane == 0) rstd[r] = rs;
}

// dS = rstd (g dY - mean(g dY) - xhat mean(g dY xhat)): the gradient of the block's input (residual) - and, times the keep factor,
// of the sub-layer's output: dO
__global__ __launch_bounds__(256) void k_s2s_ln_bwd(const float* __restrict__ dY, const float* __restrict__ xhat, const float* __restrict__ rstd,
                                                    const float* __restrict__ gamma, float* __restrict__ dS, float* __restrict__ dO, int M,
                                                    int D, float rate, uint32_t seed, uint32_t step, uint32_t site) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= M) return;
    const size_t o = (size_t)r * D;
    float a = 0.f, b = 0.f;
    for (int d = lane; d < D; d += 64) {
        const float g = gamma[d] * dY[o + d];
        a += g;
        b += g * xhat[o + d];
    }
    a = s2s_wave_sum(a) / (float)D;
    b = s2s_wave_sum(b) / (float)D;
    const float rs = rstd[r];
    for (int d = lane; d < D; d += 64) {
        const float v = rs * (gamma[d] * dY[o + d] - a - xhat[o + d] * b);
        dS[o + d] = v;
        dO[o + d] = v * s2s_keep(rate, seed, step, site, (uint32_t)r, (uint32_t)d);
    }
}

// part[z][d] = sum over the rows of chunk z of dY xhat (d gamma), part[z][D + d] = of dY (d beta); rows in order
__global__ void k_s2s_ln_colsum(const float* __restrict__ dY, const float* __restrict__ xhat, int M, int D, int chunk, float* __restrict__ part) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x, z = blockIdx.y;
    if (d >= D) return;
    const int m0 = z * chunk, m1 = min(M, m0 + chunk);
    float g = 0.f, b = 0.f;
    for (int m = m0; m < m1; ++m) {
        const float y = dY[(size_t)m * D + d];
        g += y * xhat[(size_t)m * D + d];
        b += y;
    }
    part[(size_t)z * 2 * D + d] = g;
    part[(size_t)z * 2 * D + D + d] = b;
}

// Reverse of k_s2s_attn<false> for one query row per wave.  a = e / (Z + eps) with e = mask exp(s - m), m the max over ALL keys:
//   dL/ds_k = a_k (da_k - dot) - [k = arg-max] (1 - sum a) dot,   da_k = dAO . V_k,  dot = sum_j a_j da_j
// (the second term is the max shift, which the "+ eps" keeps from cancelling; it matters when the largest key is a masked one).
// -> dsc [Mq, 65] (already divided by sqrt(D)) and dQ = sum_k dsc_k K_k.
// The dsc of a row sum to zero (the two terms cancel): q . bk moves every score of a query alike, and exp(s - max s) does not see a
// shift.  So the key bias has NO gradient, exactly; the host writes zeros there instead of the column sum of dK, which would be that
// sum's rounding error (and which Adam, dividing by its own size, would turn into steps of +- lr).
__global__ __launch_bounds__(256) void k_s2s_attn_bwd_q(const float* __restrict__ K, const float* __restrict__ V, int ldkv,
                                                        const float* __restrict__ Pa, const float* __restrict__ dAO, float* __restrict__ dsc,
                                                        float* __restrict__ dQ, int Mq, int Lq, int Lk, int D) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= Mq) return;
    const int kb = r / Lq;
    const float* go = dAO + (size_t)r * D;
    const float a = lane < Lk ? Pa[(size_t)r * S2S_PA + lane] : 0.f;
    const int amax = (int)Pa[(size_t)r * S2S_PA + 64];
    float da = 0.f;
    for (int k = 0; k < Lk; ++k) {
        const float* vr = V + ((size_t)kb * Lk + k) * ldkv;
        float s = 0.f;
        for (int d = lane; d < D; d += 64) s = fmaf(go[d], vr[d], s);
        s = s2s_wave_sum(s);
        if (lane == k) da = s;
    }
    // (1 - sum a) dot is taken as the sum of the first terms, which it equals: sum_k a_k (da_k - dot) = dot - dot sum a.  The row's
    // dsc then cancel to the rounding of that one sum, and with a single key - where the scores cannot matter - dsc is exactly 0.
    // As (1.f - sa) * dot the two terms each carried a rounding of da's size and left a gradient of noise in Wq / Wk at src_len = 1
    // or L = 1 (1e-8 of the gradient's largest element), which Adam would have stepped by +- lr like any other.
    const float dot = s2s_wave_sum(a * da);
    float ds = a * (da - dot);
    const float shift = s2s_wave_sum(ds);
    if (lane == amax) ds -= shift;
    ds = ds / sqrtf((float)D);
    if (lane < Lk) dsc[(size_t)r * S2S_PA + lane] = ds;
    for (int d0 = 0; d0 < D; d0 += 64) {
        const int d = d0 + lane;
        float o = 0.f;
        for (int k = 0; k < Lk; ++k) {
            const float dk = __shfl(ds, k);
            if (d < D) o = fmaf(dk, K[((size_t)kb * Lk + k) * ldkv + d], o);
        }
        if (d < D) dQ[(size_t)r * D + d] = o;
    }
}
// ... and for one key row (sequence kb, key k) per wave: dK = sum_q dsc[q, k] Q_q, dV = sum_q a[q, k] dAO_q over the sequence's
// queries in order -> dKV [Mk, 2 D]
__global__ __launch_bounds__(256) void k_s2s_attn_bwd_kv(const float* __restrict__ Q, const float* __restrict__ Pa, const float* __restrict__ dsc,
                                                         const float* __restrict__ dAO, float* __restrict__ dKV, int Mk, int Lq, int Lk,
                                                         int D) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= Mk) return;
    const int kb = r / Lk, k = r - kb * Lk;
    for (int d = lane; d < D; d += 64) {
        float dk = 0.f, dv = 0.f;
        for (int q = 0; q < Lq; ++q) {
            const size_t row = (size_t)kb * Lq + q;
            dk = fmaf(dsc[row * S2S_PA + k], Q[row * D + d], dk);
            dv = fmaf(Pa[row * S2S_PA + k], dAO[row * D + d], dv);
        }
        dKV[(size_t)r * 2 * D + d] = dk;
        dKV[(size_t)r * 2 * D + D + d] = dv;
    }
}

// y = a + b (+ c) (+ e)
__global__ void k_s2s_sum4(float* __restrict__ y, const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c,
                           const float* __restrict__ e, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = a[i] + b[i];
    if (c) s += c[i];
    if (e) s += e[i];
    y[i] = s;
}

// out[0] = number of rows whose decoder-input token is not PAD (single workgroup, fixed order)
__global__ __launch_bounds__(256) void k_s2s_count(const int32_t* __restrict__ dec_in, int M, float* __restrict__ out) {
    __shared__ float sm[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < M; i += 256) s += dec_in[i] != 0 ? 1.f : 0.f;
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sm[0];
}
// row m: rowloss = -w log p[target], P[m, :] <- w (p - onehot(target)) / count, w = (dec_in[m] != PAD)
__global__ __launch_bounds__(256) void k_s2s_ce(float* __restrict__ P, int64_t ld, int V, const int32_t* __restrict__ dec_in,
                                                const int32_t* __restrict__ dec_out, const float* __restrict__ count,
                                                float* __restrict__ rowloss) {
    const int m = blockIdx.x;
    float* p = P + (size_t)m * ld;
    const int tgt = min(max(dec_out[m], 0), V - 1);
    const float w = dec_in[m] != 0 ? 1.f : 0.f, cnt = fmaxf(count[0], 1.f);
    if (threadIdx.x == 0) rowloss[m] = w > 0.f ? -logf(p[tgt]) : 0.f;
    __syncthreads();
    for (int v = threadIdx.x; v < V; v += 256) p[v] = w * (p[v] - (v == tgt ? 1.f : 0.f)) / cnt;
}
// loss[0] = sum(rowloss) / count (single workgroup, fixed order)
__global__ __launch_bounds__(256) void k_s2s_loss(const float* __restrict__ rowloss, int M, const float* __restrict__ count, float* __restrict__ loss) {
    __shared__ float sm[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < M; i += 256) s += rowloss[i];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = sm[0] / fmaxf(count[0], 1.f);
}

// dE[v, :] (+)= sum of dX[m, :] over the positions m that hold token v, in position order; one workgroup per token
__global__ __launch_bounds__(256) void k_s2s_embed_bwd(const int32_t* __restrict__ tok, int M, const float* __restrict__ dX, float* __restrict__ dE,
                                                       int D, int V, int accumulate) {
    const int v = blockIdx.x;
    for (int d = threadIdx.x; d < D; d += 256) {
        float s = accumulate ? dE[(size_t)v * D + d] : 0.f;
        for (int m = 0; m < M; ++m)
            if (min(max(tok[m], 0), V - 1) == v) s += dX[(size_t)m * D + d];
        dE[(size_t)v * D + d] = s;
    }
}

}  // namespace
