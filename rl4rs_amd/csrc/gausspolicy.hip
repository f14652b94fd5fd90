// Gaussian actor-critic for the continuous-action env (include/rl4rs_hip.h, "Gaussian policy"): the stochastic continuous policy
// the on-policy learners (A2C / PPO / PG / IMPALA) train on support_conti_env.
//
// Reference: script/modelfree_train.py:219-234,271-286,315-330,362-377 (the `is_conti` branches: RLlib 1.5.1 falls back to its
// default model and a diagonal-Gaussian action distribution).  RLlib's FullyConnectedNetwork under MODEL_DEFAULTS (fcnet_hiddens
// [256, 256], tanh, vf_share_layers False, free_log_std False), DiagGaussian and StochasticSampling are third-party and absent:
// restated from their published 1.5.1 form, PARITY UNPINNED, checked against the fp64 restatement in tests/gauss_ref.py.
//
//   actor   h1 = tanh(x W1 + b1), h2 = tanh(h1 W2 + b2), head = h2 W3 + b3 = [mean (E) | log_std (E)]
//   critic  V  = tanh(tanh(x V1 + c1) V2 + c2) V3 + c3                      (its own tower)
//   flat    [W1 | b1 | W2 | b2 | W3 (H x 2E) | b3 | V1 | c1 | V2 | c2 | V3 (H x 1) | c3], matrices [in, out]
//
// Kernel mapping.  A workgroup of four waves owns a tile of 16 rows of ONE tower (grid.y = tower: actor and critic share a
// launch); all three layers run in that launch with the tile's activations in LDS, as v_mfma_f32_16x16x4_f32 products (exact
// fp32: logp enters importance ratios) against weights read row-major as they are (they change every update).  4096 rows are
// 512 workgroups, a 256-row minibatch is 32.  A row's arithmetic does not depend on which other rows share its call.  The
// backward is the same tile walk against transposed weights with the 1 - h^2 factors in the epilogues; weight gradients are
// sample-axis reductions in fixed chunks (launch_gemm_tn), bias gradients, statistics and the norm of the gradient clip are
// float64-carried sums in a fixed order: no float atomics, two identical calls give identical bits.
#include <cmath>
#include <vector>

#include "common.hpp"
#include "optim.hpp"
#include "mfma4.hpp"

namespace rl4rs {
namespace {

constexpr int GP_ROWS = 16;          // rows of a tile
constexpr int GP_KC = 256;           // observation columns staged per pass
constexpr int GP_LDX = GP_KC + 4;    // LDS row strides (+ 4: the 16 rows of an A fragment start in different banks)
constexpr int GP_HMAX = 256, GP_LDH = GP_HMAX + 4;
constexpr int GP_E2MAX = 128, GP_LDO = GP_E2MAX + 4;
constexpr float GP_HALF_LOG_2PI = 0.91893853320467274178f;      // 0.5 log(2 pi)
constexpr float GP_HALF_LOG_2PIE = 1.41893853320467274178f;     // 0.5 log(2 pi e)

struct GpDims { int D, H, E; };
struct GpOffsets { int64_t W1, b1, W2, b2, W3, b3, V1, c1, V2, c2, V3, c3, n; };
inline GpOffsets gp_offsets(int D, int H, int E) {
    GpOffsets o;
    o.W1 = 0; o.b1 = o.W1 + (int64_t)D * H; o.W2 = o.b1 + H; o.b2 = o.W2 + (int64_t)H * H; o.W3 = o.b2 + H;
    o.b3 = o.W3 + (int64_t)H * 2 * E; o.V1 = o.b3 + 2 * E; o.c1 = o.V1 + (int64_t)D * H; o.V2 = o.c1 + H;
    o.c2 = o.V2 + (int64_t)H * H; o.V3 = o.c2 + H; o.c3 = o.V3 + H; o.n = o.c3 + 1;
    return o;
}

// acc[t] += A [16 x K] (LDS, row stride lda, K a multiple of 4, zeros past the valid columns) * W[k][col] for this wave's t-th
// column tile (tiles wave, wave + 4, ...); rows of W from kvalid on and columns from Nc on count as zero.  Four k-steps are fetched
// together (their weight loads are in flight at once: one step at a time paid an L2 round trip per MFMA group) and multiplied in
// ascending k, the order of the plain loop.
template <int NT>
__device__ __forceinline__ void gp_mma(f32x4_t (&acc)[NT], int ntw, const float* sA, int lda, int K, const float* __restrict__ W, int ldw,
                                       int kvalid, int Nc, int wave, int lane) {
    const int i = lane & 15, kq = lane >> 4;
    for (int k = 0; k < K; k += 16) {
        float a[4], b[4][NT];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int kk = k + 4 * u + kq;
            a[u] = kk < K ? sA[i * lda + kk] : 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int col = (wave + 4 * t) * 16 + i;
                b[u][t] = (t < ntw && kk < kvalid && col < Nc) ? W[(size_t)kk * ldw + col] : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (k + 4 * u < K) {
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    if (t < ntw) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b[u][t], acc[t], 0, 0, 0);
            }
        }
    }
}

template <int NT>
__device__ __forceinline__ void gp_zero(f32x4_t (&acc)[NT]) {
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
}

// sum over the 16 lanes that share a row (lanes 16 r .. 16 r + 15 of a wave): a fixed butterfly
__device__ __forceinline__ float gp_sum16(float x) {
    x += __shfl_xor(x, 8);
    x += __shfl_xor(x, 4);
    x += __shfl_xor(x, 2);
    x += __shfl_xor(x, 1);
    return x;
}
__device__ __forceinline__ float gp_sum64(float x) {
    x += __shfl_xor(x, 32);
    x += __shfl_xor(x, 16);
    return gp_sum16(x);
}

struct GpFwd {
    GpDims d;
    int N, deterministic;
    uint32_t seed, step;
    const float* prm; const float* obs;
    const float* actions_in;                 // evaluate: the actions to score; NULL: draw
    float *action, *env_action, *logp, *value, *entropy, *head, *eps;      // each may be NULL
    float *H1[2], *H2[2];                    // training: the towers' activations [N, H], or NULL
};

// One launch: both towers (blockIdx.y), three layers, the distribution.
__global__ __launch_bounds__(256) void k_gp_fwd(GpFwd a) {
    __shared__ float s_x[GP_ROWS * GP_LDX];
    __shared__ float s_h1[GP_ROWS * GP_LDH];
    __shared__ float s_h2[GP_ROWS * GP_LDH];
    __shared__ float s_o[GP_ROWS * GP_LDO];
    const int D = a.d.D, H = a.d.H, E = a.d.E, E2 = 2 * E;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int tower = blockIdx.y, row0 = blockIdx.x * GP_ROWS;
    const int64_t tower_n = (int64_t)D * H + H + (int64_t)H * H + H;
    const float* W1 = a.prm + (tower ? tower_n + (int64_t)H * E2 + E2 : 0);
    const float* b1 = W1 + (size_t)D * H;
    const float* W2 = b1 + H;
    const float* b2 = W2 + (size_t)H * H;
    const float* W3 = b2 + H;
    const float* b3 = W3 + (size_t)H * (tower ? 1 : E2);
    const int ntw = H / 64;                  // column tiles of a hidden layer per wave
    const int ci = lane & 15, rq = lane >> 4;
    f32x4_t acc[4];

    // ---- layer 1: the observation goes through LDS GP_KC columns at a time
    gp_zero(acc);
    for (int k0 = 0; k0 < D; k0 += GP_KC) {
        if (k0) __syncthreads();
        for (int idx = tid; idx < GP_ROWS * GP_KC; idx += 256) {
            const int r = idx / GP_KC, c = idx - r * GP_KC;
            const int n = row0 + r, k = k0 + c;
            s_x[r * GP_LDX + c] = (n < a.N && k < D) ? a.obs[(size_t)n * D + k] : 0.f;
        }
        __syncthreads();
        const int kv = min(GP_KC, D - k0);
        gp_mma<4>(acc, ntw, s_x, GP_LDX, (kv + 3) & ~3, W1 + (size_t)k0 * H, H, kv, H, wave, lane);
    }
    float* gH1 = a.H1[tower];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (t < ntw) {
            const int col = (wave + 4 * t) * 16 + ci;
            const float b = b1[col];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = rq * 4 + r;
                const float h = tanhf(acc[t][r] + b);
                s_h1[row * GP_LDH + col] = h;
                if (gH1 && row0 + row < a.N) gH1[(size_t)(row0 + row) * H + col] = h;
            }
        }
    }
    __syncthreads();
    // ---- layer 2
    gp_zero(acc);
    gp_mma<4>(acc, ntw, s_h1, GP_LDH, H, W2, H, H, H, wave, lane);
    float* gH2 = a.H2[tower];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (t < ntw) {
            const int col = (wave + 4 * t) * 16 + ci;
            const float b = b2[col];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = rq * 4 + r;
                const float h = tanhf(acc[t][r] + b);
                s_h2[row * GP_LDH + col] = h;
                if (gH2 && row0 + row < a.N) gH2[(size_t)(row0 + row) * H + col] = h;
            }
        }
    }
    __syncthreads();
    // ---- critic: V = h2 . V3 + c3, four rows per wave
    if (tower) {
        for (int r = 0; r < 4; ++r) {
            const int row = wave * 4 + r;
            float s = 0.f;
            for (int j = lane; j < H; j += 64) s += s_h2[row * GP_LDH + j] * W3[j];
            s = gp_sum64(s);
            if (lane == 0 && a.value && row0 + row < a.N) a.value[row0 + row] = s + b3[0];
        }
        return;
    }
    // ---- actor head [16 x 2E]
    f32x4_t ao[2];
    gp_zero(ao);
    const int nto = ((E2 + 15) / 16 - wave + 3) / 4;          // of the ceil(2E / 16) column tiles, those this wave takes
    gp_mma<2>(ao, nto, s_h2, GP_LDH, H, W3, E2, H, E2, wave, lane);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int col = (wave + 4 * t) * 16 + ci;
        if (t < nto && col < E2) {
            const float b = b3[col];
#pragma unroll
            for (int r = 0; r < 4; ++r) s_o[(rq * 4 + r) * GP_LDO + col] = ao[t][r] + b;
        }
    }
    __syncthreads();
    // ---- the distribution: 16 threads per row
    const int row = tid >> 4, sub = tid & 15, n = row0 + row;
    const bool live = n < a.N;
    float lp = 0.f, en = 0.f;
    for (int e = sub; e < E; e += 16) {
        const float mean = s_o[row * GP_LDO + e], ls = s_o[row * GP_LDO + E + e];
        float act;
        if (a.actions_in) {
            act = live ? a.actions_in[(size_t)n * E + e] : 0.f;
        } else {
            const float eps = normal01(a.seed, a.step, (uint32_t)n, (uint32_t)e);
            act = a.deterministic ? mean : mean + expf(ls) * eps;
            if (live && a.eps) a.eps[(size_t)n * E + e] = eps;
        }
        const float z = (act - mean) * expf(-ls);
        lp += -0.5f * z * z - ls;
        en += ls + GP_HALF_LOG_2PIE;
        if (live) {
            if (a.action) a.action[(size_t)n * E + e] = act;
            if (a.env_action) a.env_action[(size_t)n * E + e] = fminf(fmaxf(act, -1.f), 1.f);
            if (a.head) {
                a.head[(size_t)n * E2 + e] = mean;
                a.head[(size_t)n * E2 + E + e] = ls;
            }
        }
    }
    lp = gp_sum16(lp);
    en = gp_sum16(en);
    if (live && sub == 0) {
        if (a.logp) a.logp[n] = lp - (float)E * GP_HALF_LOG_2PI;
        if (a.entropy) a.entropy[n] = en;
    }
}

struct GpLoss {
    GpDims d;
    int N, algo;
    float vf_coeff, ent_coeff, clip, vf_clip, kl_coeff, scale;
    const float *head, *value, *actions, *adv, *ret, *old_logp, *old_value, *old_head;
    float *dhead, *dvalue;
    float4* terms;
};

// One wave per row, lane e < E: per-row loss terms, d loss / d head [N, 2E] and d loss / d value [N].  The A2C and PPO forms are
// those of rl4rs_policy_loss_grad (policy_row_loss) with the diagonal Gaussian in place of the masked softmax.
__global__ __launch_bounds__(256) void k_gp_loss(GpLoss L) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + wave;
    if (n >= L.N) return;
    const int E = L.d.E, E2 = 2 * E;
    const bool on = lane < E;
    const int e = on ? lane : 0;
    const float mean = L.head[(size_t)n * E2 + e], ls = L.head[(size_t)n * E2 + E + e];
    const float act = L.actions[(size_t)n * E + e];
    const float inv = expf(-ls);
    const float z = (act - mean) * inv;
    float dm = 0.f, inv2 = 0.f, so = 0.f, kl_e = 0.f;
    if (L.algo == 1) {
        const float mo = L.old_head[(size_t)n * E2 + e], lo = L.old_head[(size_t)n * E2 + E + e];
        dm = mo - mean;
        inv2 = expf(-2.f * ls);
        so = expf(2.f * lo) + dm * dm;
        kl_e = ls - lo + so * (0.5f * inv2) - 0.5f;
    }
    const float lp_a = gp_sum64(on ? -0.5f * z * z - ls : 0.f) - (float)E * GP_HALF_LOG_2PI;
    const float ent = gp_sum64(on ? ls + GP_HALF_LOG_2PIE : 0.f);
    const float kl = gp_sum64(on ? kl_e : 0.f);
    const float adv = L.adv[n], ret = L.ret[n], v = L.value[n];
    float g_lp, g_v, pi_loss, vf_loss;
    if (L.algo == 0) {
        pi_loss = -lp_a * adv;
        vf_loss = 0.5f * (v - ret) * (v - ret);
        g_lp = -adv;
        g_v = L.vf_coeff * (v - ret);
    } else {
        const float ratio = expf(lp_a - L.old_logp[n]);
        const float clipped = fminf(fmaxf(ratio, 1.f - L.clip), 1.f + L.clip);
        const float s1 = adv * ratio, s2 = adv * clipped;
        pi_loss = -fminf(s1, s2);
        g_lp = (s1 <= s2) ? -adv * ratio : 0.f;        // the clipped branch has zero gradient
        const float pv = L.old_value[n];
        const float l1 = (v - ret) * (v - ret);
        const float vc = pv + fminf(fmaxf(v - pv, -L.vf_clip), L.vf_clip);
        const float l2 = (vc - ret) * (vc - ret);
        vf_loss = fmaxf(l1, l2);
        const float dv = (l1 >= l2) ? 2.f * (v - ret) : ((fabsf(v - pv) < L.vf_clip) ? 2.f * (vc - ret) : 0.f);
        g_v = L.vf_coeff * dv;
    }
    g_lp *= L.scale;
    g_v *= L.scale;
    const float ce = L.ent_coeff * L.scale, ck = (L.algo == 1) ? L.kl_coeff * L.scale : 0.f;
    if (on) {
        // d logp / d mean = z exp(-ls), d logp / d ls = z^2 - 1, d H / d ls = 1,
        // d KL / d mean = -(mean_old - mean) exp(-2 ls), d KL / d ls = 1 - (exp(2 ls_old) + (mean_old - mean)^2) exp(-2 ls)
        float gm = g_lp * (z * inv);
        float gl = g_lp * (z * z - 1.f) - ce;
        if (L.algo == 1) {
            gm -= ck * (dm * inv2);
            gl += ck * (1.f - so * inv2);
        }
        L.dhead[(size_t)n * E2 + e] = gm;
        L.dhead[(size_t)n * E2 + E + e] = gl;
    }
    if (lane == 0) {
        L.dvalue[n] = g_v;
        L.terms[n] = make_float4(pi_loss, vf_loss, ent, kl);
    }
}

struct GpBwd {
    GpDims d;
    int N;
    const float* V3;                         // [H]: read from the parameters as it is
    const float *W3t, *W2t[2];               // transposed weights: [2E, H], [H, H] per tower
    const float *dhead, *dvalue;
    const float *H1[2], *H2[2];
    float *dH1[2], *dH2[2];                  // out: gradients of the hidden layers' pre-activations [N, H]
};

// d head -> d h2 -> d h1 of one tower's tile, the 1 - h^2 factors in the epilogues
__global__ __launch_bounds__(256) void k_gp_bwd(GpBwd a) {
    __shared__ float s_o[GP_ROWS * GP_LDO];
    __shared__ float s_d2[GP_ROWS * GP_LDH];
    const int H = a.d.H, E2 = 2 * a.d.E;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int tower = blockIdx.y, row0 = blockIdx.x * GP_ROWS;
    const int ntw = H / 64, ci = lane & 15, rq = lane >> 4;
    const float* gH1 = a.H1[tower];
    const float* gH2 = a.H2[tower];
    float* dH1 = a.dH1[tower];
    float* dH2 = a.dH2[tower];
    f32x4_t acc[4];
    if (tower == 0) {
        const int K3 = (E2 + 3) & ~3;
        for (int idx = tid; idx < GP_ROWS * K3; idx += 256) {
            const int r = idx / K3, c = idx - r * K3;
            s_o[r * GP_LDO + c] = (row0 + r < a.N && c < E2) ? a.dhead[(size_t)(row0 + r) * E2 + c] : 0.f;
        }
        __syncthreads();
        gp_zero(acc);
        gp_mma<4>(acc, ntw, s_o, GP_LDO, K3, a.W3t, H, E2, H, wave, lane);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t < ntw) {
                const int col = (wave + 4 * t) * 16 + ci;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = rq * 4 + r, n = row0 + row;
                    float g = 0.f;
                    if (n < a.N) {
                        const float h = gH2[(size_t)n * H + col];
                        g = acc[t][r] * (1.f - h * h);
                        dH2[(size_t)n * H + col] = g;
                    }
                    s_d2[row * GP_LDH + col] = g;
                }
            }
        }
    } else {
        const float* V3 = a.V3;
        for (int idx = tid; idx < GP_ROWS * H; idx += 256) {
            const int r = idx / H, c = idx - r * H, n = row0 + r;
            float g = 0.f;
            if (n < a.N) {
                const float h = gH2[(size_t)n * H + c];
                g = a.dvalue[n] * V3[c] * (1.f - h * h);
                dH2[(size_t)n * H + c] = g;
            }
            s_d2[r * GP_LDH + c] = g;
        }
    }
    __syncthreads();
    gp_zero(acc);
    gp_mma<4>(acc, ntw, s_d2, GP_LDH, H, a.W2t[tower], H, H, H, wave, lane);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (t < ntw) {
            const int col = (wave + 4 * t) * 16 + ci;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = row0 + rq * 4 + r;
                if (n < a.N) {
                    const float h = gH1[(size_t)n * H + col];
                    dH1[(size_t)n * H + col] = acc[t][r] * (1.f - h * h);
                }
            }
        }
    }
}

// dst [C, R] = src [R, C]^T
__global__ void k_gp_transpose(const float* __restrict__ src, int R, int Cn, float* __restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R * Cn) return;
    const int c = i / R, r = i - c * R;
    dst[i] = src[(size_t)r * Cn + c];
}

// stats[0..3] = sums of the per-row terms: one workgroup, every thread its rows in index order, then a fixed tree; the sums are
// carried in float64 and rounded once
__global__ __launch_bounds__(256) void k_gp_terms(const float4* __restrict__ terms, int N, float* __restrict__ stats) {
    __shared__ double sm[4][256];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int n = threadIdx.x; n < N; n += 256) {
        const float4 t = terms[n];
        s0 += (double)t.x; s1 += (double)t.y; s2 += (double)t.z; s3 += (double)t.w;
    }
    sm[0][threadIdx.x] = s0; sm[1][threadIdx.x] = s1; sm[2][threadIdx.x] = s2; sm[3][threadIdx.x] = s3;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int k = 0; k < 4; ++k) sm[k][threadIdx.x] += sm[k][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x < 4) stats[threadIdx.x] = (float)sm[threadIdx.x][0];
}

// Bias gradients: out[j] = sum over the N rows of X[n][j] for up to six matrices in one launch (blockIdx.y).  16 columns x 16 row
// groups per workgroup; a thread adds its rows (n = group, group + 16, ...) in float64, the groups meet in LDS in group order:
// a fixed order, and a sum that does not lose the small rows of a long batch.
struct GpColsums { const float* X[6]; float* out[6]; int ld[6], Nc[6]; int N; };
__global__ __launch_bounds__(256) void k_gp_colsums(GpColsums a) {
    __shared__ double sm[16][16];
    const int w = blockIdx.y, c = threadIdx.x & 15, q = threadIdx.x >> 4;
    const int j = blockIdx.x * 16 + c;
    const int Nc = a.Nc[w], ld = a.ld[w];
    const float* X = a.X[w];
    double s = 0.0;
    if (j < Nc) {
        int n = q;
        for (; n + 48 < a.N; n += 64) {          // four loads in flight
            const float x0 = X[(size_t)n * ld + j], x1 = X[(size_t)(n + 16) * ld + j], x2 = X[(size_t)(n + 32) * ld + j],
                        x3 = X[(size_t)(n + 48) * ld + j];
            s += (double)x0; s += (double)x1; s += (double)x2; s += (double)x3;
        }
        for (; n < a.N; n += 16) s += (double)X[(size_t)n * ld + j];
    }
    sm[q][c] = s;
    __syncthreads();
    if (q == 0 && j < Nc) {
        double t = 0.0;
#pragma unroll
        for (int g = 0; g < 16; ++g) t += sm[g][c];
        a.out[w][j] = (float)t;
    }
}

// out[0] = sum of squares of a flat buffer (the global norm of tf.clip_by_global_norm), carried in float64: one workgroup, fixed order
__global__ __launch_bounds__(256) void k_gp_sumsq(const float* __restrict__ g, int64_t count, float* __restrict__ out) {
    __shared__ double sm[256];
    double s = 0.0;
    int64_t i = threadIdx.x;
    for (; i + 768 < count; i += 1024) {
        const float x0 = g[i], x1 = g[i + 256], x2 = g[i + 512], x3 = g[i + 768];
        s += (double)x0 * x0; s += (double)x1 * x1; s += (double)x2 * x2; s += (double)x3 * x3;
    }
    for (; i < count; i += 256) s += (double)g[i] * g[i];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)sm[0];
}

// acc[0..3] += x[0..3] (a pass's sums over its minibatches, in minibatch order)
__global__ void k_gp_add4(const float* __restrict__ x, float* __restrict__ acc) {
    if (threadIdx.x < 4) acc[threadIdx.x] += x[threadIdx.x];
}

// out[0..3] = sum over r of part[r][0..3], in order of r
__global__ void k_gp_sum_stats(const double* __restrict__ part, int R, double* __restrict__ out) {
    if (threadIdx.x >= 4) return;
    double s = 0.0;
    for (int r = 0; r < R; ++r) s += part[4 * r + threadIdx.x];
    out[threadIdx.x] = s;
}

constexpr int GP_NZ_MAX = 16;        // sample chunks of a weight-gradient reduction

}  // namespace
}  // namespace rl4rs

using namespace rl4rs;

struct rl4rs_gpolicy {
    GpDims d;
    GpOffsets o;
    int max_rows;
    OptBlock opt;              // grad stays null: the gradient is the caller's buffer
    float *H1[2], *H2[2], *dH1[2], *dH2[2];
    float *head, *value, *dhead, *dvalue, *W3t, *W2t[2], *part, *sumsq;
    float4* terms;
    // scratch of rl4rs_gpolicy_vtrace_loss_grad, allocated by its first call
    float *vt_logp, *vt_val, *vt_vs, *vt_pg, *vt_obs, *vt_act;
    double* vt_stats;          // [vt_stats_cap, 4]: per-rollout V-trace sums
    int vt_stats_cap;
    std::vector<void*> owned;
};

namespace {

int gp_alloc(rl4rs_gpolicy* p, float** dst, size_t n) {
    int r = dev_alloc(dst, n);
    if (r == RL4RS_OK) p->owned.push_back(*dst);
    return r;
}

int gp_forward(rl4rs_gpolicy* p, GpFwd& a, hipStream_t st) {
    a.d = p->d;
    a.prm = p->opt.params;
    hipLaunchKernelGGL(k_gp_fwd, dim3((a.N + GP_ROWS - 1) / GP_ROWS, 2), dim3(256), 0, st, a);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

int gp_loss_grad(rl4rs_gpolicy* p, int algo, int N, const float* obs, const float* actions, const float* adv, const float* ret,
                 const float* old_logp, const float* old_value, const float* old_head, float vf_coeff, float ent_coeff, float clip,
                 float vf_clip, float kl_coeff, float* grad, float* stats, hipStream_t st) {
    const int D = p->d.D, H = p->d.H, E2 = 2 * p->d.E;
    const GpOffsets& o = p->o;
    int rc;
    // 1. training forward: activations of both towers, head and value
    GpFwd f;
    memset(&f, 0, sizeof(f));
    f.N = N; f.obs = obs; f.actions_in = actions; f.head = p->head; f.value = p->value;
    for (int t = 0; t < 2; ++t) { f.H1[t] = p->H1[t]; f.H2[t] = p->H2[t]; }
    if ((rc = gp_forward(p, f, st))) return rc;
    // 2. per-row loss
    GpLoss L;
    memset(&L, 0, sizeof(L));
    L.d = p->d; L.N = N; L.algo = algo;
    L.vf_coeff = vf_coeff; L.ent_coeff = ent_coeff; L.clip = clip; L.vf_clip = vf_clip; L.kl_coeff = kl_coeff;
    L.scale = algo == 0 ? 1.0f : 1.0f / (float)N;
    L.head = p->head; L.value = p->value; L.actions = actions; L.adv = adv; L.ret = ret;
    L.old_logp = old_logp; L.old_value = old_value; L.old_head = old_head;
    L.dhead = p->dhead; L.dvalue = p->dvalue; L.terms = p->terms;
    hipLaunchKernelGGL(k_gp_loss, dim3((N + 3) / 4), dim3(256), 0, st, L);
    RL4RS_LAUNCH_CHECK();
    // 3. backward through the hidden layers against transposed weights
    const float* prm = p->opt.params;
    hipLaunchKernelGGL(k_gp_transpose, dim3((H * E2 + 255) / 256), dim3(256), 0, st, prm + o.W3, H, E2, p->W3t);
    hipLaunchKernelGGL(k_gp_transpose, dim3((H * H + 255) / 256), dim3(256), 0, st, prm + o.W2, H, H, p->W2t[0]);
    hipLaunchKernelGGL(k_gp_transpose, dim3((H * H + 255) / 256), dim3(256), 0, st, prm + o.V2, H, H, p->W2t[1]);
    GpBwd b;
    memset(&b, 0, sizeof(b));
    b.d = p->d; b.N = N; b.V3 = prm + o.V3; b.W3t = p->W3t; b.dhead = p->dhead; b.dvalue = p->dvalue;
    for (int t = 0; t < 2; ++t) { b.W2t[t] = p->W2t[t]; b.H1[t] = p->H1[t]; b.H2[t] = p->H2[t]; b.dH1[t] = p->dH1[t]; b.dH2[t] = p->dH2[t]; }
    hipLaunchKernelGGL(k_gp_bwd, dim3((N + GP_ROWS - 1) / GP_ROWS, 2), dim3(256), 0, st, b);
    RL4RS_LAUNCH_CHECK();
    // 4. weight gradients: sample-axis reductions in at most GP_NZ_MAX chunks (of at least 64 rows: short accumulation chains, and
    // a 256-row minibatch is still several workgroups per tile), summed in chunk order; bias gradients: k_gp_colsums
    const int chunk = (((N + GP_NZ_MAX - 1) / GP_NZ_MAX) + 63) / 64 * 64;
    auto tn = [&](const float* A, int lda, int M, const float* B, int ldb, int Nc, int64_t oW) {
        return launch_gemm_tn(A, lda, M, B, ldb, Nc, N, chunk, p->part, nullptr, grad + oW, nullptr, st);
    };
    if ((rc = tn(obs, D, D, p->dH1[0], H, H, o.W1))) return rc;
    if ((rc = tn(p->H1[0], H, H, p->dH2[0], H, H, o.W2))) return rc;
    if ((rc = tn(p->H2[0], H, H, p->dhead, E2, E2, o.W3))) return rc;
    if ((rc = tn(obs, D, D, p->dH1[1], H, H, o.V1))) return rc;
    if ((rc = tn(p->H1[1], H, H, p->dH2[1], H, H, o.V2))) return rc;
    if ((rc = tn(p->H2[1], H, H, p->dvalue, 1, 1, o.V3))) return rc;
    GpColsums cs;
    const float* bx[6] = {p->dH1[0], p->dH2[0], p->dhead, p->dH1[1], p->dH2[1], p->dvalue};
    const int64_t bo[6] = {o.b1, o.b2, o.b3, o.c1, o.c2, o.c3};
    const int bn[6] = {H, H, E2, H, H, 1};
    for (int k = 0; k < 6; ++k) { cs.X[k] = bx[k]; cs.out[k] = grad + bo[k]; cs.ld[k] = bn[k]; cs.Nc[k] = bn[k]; }
    cs.N = N;
    hipLaunchKernelGGL(k_gp_colsums, dim3(((H > E2 ? H : E2) + 15) / 16, 6), dim3(256), 0, st, cs);
    RL4RS_LAUNCH_CHECK();
    if (stats) {
        hipLaunchKernelGGL(k_gp_terms, dim3(1), dim3(256), 0, st, p->terms, N, stats);
        RL4RS_LAUNCH_CHECK();
    }
    return RL4RS_OK;
}

int gp_vtrace_scratch(rl4rs_gpolicy* p, bool compact) {
    int rc;
    if (!p->vt_logp) {
        if ((rc = gp_alloc(p, &p->vt_val, (size_t)p->max_rows))) return rc;
        if ((rc = gp_alloc(p, &p->vt_vs, (size_t)p->max_rows))) return rc;
        if ((rc = gp_alloc(p, &p->vt_pg, (size_t)p->max_rows))) return rc;
        if ((rc = gp_alloc(p, &p->vt_logp, (size_t)p->max_rows))) return rc;
    }
    if (compact && !p->vt_obs) {       // the kept rows of R > 1 rollouts with a dropped last step are not one row range
        if ((rc = gp_alloc(p, &p->vt_act, (size_t)p->max_rows * p->d.E))) return rc;
        if ((rc = gp_alloc(p, &p->vt_obs, (size_t)p->max_rows * p->d.D))) return rc;
    }
    return RL4RS_OK;
}

}  // namespace

extern "C" {

int64_t rl4rs_gpolicy_param_count(int32_t obs_dim, int32_t hidden, int32_t act_dim) {
    if (obs_dim < 1 || hidden < 1 || act_dim < 1) return 0;
    return gp_offsets(obs_dim, hidden, act_dim).n;
}

int rl4rs_gpolicy_create(int32_t obs_dim, int32_t hidden, int32_t act_dim, int32_t max_rows, const float* params_host, void* stream,
                         rl4rs_gpolicy** out) {
    RL4RS_REQUIRE(out && params_host, "gpolicy_create: null argument");
    RL4RS_REQUIRE(obs_dim >= 1 && obs_dim <= 4096, "gpolicy_create: obs_dim %d is outside [1, 4096]", obs_dim);
    RL4RS_REQUIRE(hidden == 64 || hidden == 128 || hidden == 256, "gpolicy_create: hidden %d is not one of 64, 128, 256", hidden);
    RL4RS_REQUIRE(act_dim >= 1 && act_dim <= 64, "gpolicy_create: act_dim %d is outside [1, 64]", act_dim);
    RL4RS_REQUIRE(max_rows >= 1, "gpolicy_create: max_rows %d must be >= 1", max_rows);
    if (rl4rs_device_count() <= 0) {
        set_error("no HIP device visible: librl4rs_hip has no CPU fallback");
        return RL4RS_EHIP;
    }
    rl4rs_gpolicy* p = new rl4rs_gpolicy();
    p->d.D = obs_dim; p->d.H = hidden; p->d.E = act_dim;
    p->o = gp_offsets(obs_dim, hidden, act_dim);
    p->max_rows = max_rows;
    p->opt.n = p->o.n; p->opt.t = 0; p->opt.grad = nullptr;
    p->vt_logp = p->vt_val = p->vt_vs = p->vt_pg = p->vt_obs = p->vt_act = nullptr;
    p->vt_stats = nullptr; p->vt_stats_cap = 0;
    const size_t H = hidden, E2 = 2 * (size_t)act_dim, R = max_rows;
    int rc = RL4RS_OK;
    auto need = [&](float** dst, size_t n) { if (rc == RL4RS_OK) rc = gp_alloc(p, dst, n); };
    need(&p->opt.params, p->opt.n); need(&p->opt.m, p->opt.n); need(&p->opt.v, p->opt.n);
    for (int t = 0; t < 2; ++t) {
        need(&p->H1[t], R * H); need(&p->H2[t], R * H); need(&p->dH1[t], R * H); need(&p->dH2[t], R * H); need(&p->W2t[t], H * H);
    }
    need(&p->head, R * E2); need(&p->dhead, R * E2); need(&p->value, R); need(&p->dvalue, R); need(&p->W3t, H * E2);
    const size_t mmax = (size_t)obs_dim > H ? (size_t)obs_dim : H, nmax = H > E2 ? H : E2;
    need(&p->part, (size_t)GP_NZ_MAX * mmax * nmax); need(&p->sumsq, 4);
    float* t4 = nullptr;
    need(&t4, R * 4);
    p->terms = reinterpret_cast<float4*>(t4);
    if (rc != RL4RS_OK) { rl4rs_gpolicy_destroy(p); return rc; }
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(p->opt.params, params_host, (size_t)p->opt.n * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(p->opt.m, 0, (size_t)p->opt.n * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(p->opt.v, 0, (size_t)p->opt.n * 4, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        set_error("gpolicy_create: copying the parameters failed: %s", hipGetErrorString(e));
        rl4rs_gpolicy_destroy(p);
        return RL4RS_EHIP;
    }
    *out = p;
    return RL4RS_OK;
}

int rl4rs_gpolicy_destroy(rl4rs_gpolicy* p) {
    if (!p) return RL4RS_OK;
    for (void* q : p->owned) (void)hipFree(q);
    delete p;
    return RL4RS_OK;
}

int rl4rs_gpolicy_params(rl4rs_gpolicy* p, float** params_dev, float** grad_dev, int64_t* count) {
    return opt_params(RL4RS_OPT(p), params_dev, grad_dev, count, "gpolicy_params");
}
int rl4rs_gpolicy_adam_state(rl4rs_gpolicy* p, float** m_dev, float** v_dev, int64_t* step) {
    return opt_adam_state(RL4RS_OPT(p), m_dev, v_dev, step, "gpolicy_adam_state");
}
int rl4rs_gpolicy_set_adam_step(rl4rs_gpolicy* p, int64_t step) {
    return opt_set_adam_step(RL4RS_OPT(p), step, "gpolicy_set_adam_step");
}
int rl4rs_gpolicy_copy_params(rl4rs_gpolicy* dst, const rl4rs_gpolicy* src, void* stream) {
    return opt_copy_params(RL4RS_OPT(dst), RL4RS_OPT(src), stream, "gpolicy_copy_params");
}

int rl4rs_gpolicy_act(rl4rs_gpolicy* p, int32_t N, const float* obs_dev, uint32_t seed, uint32_t step, int32_t deterministic,
                      float* action_dev, float* env_action_dev, float* logp_dev, float* value_dev, float* entropy_dev, float* head_dev,
                      float* eps_dev, void* stream) {
    RL4RS_REQUIRE(p && obs_dev && action_dev, "gpolicy_act: null argument");
    RL4RS_REQUIRE(N >= 1 && N <= p->max_rows, "gpolicy_act: bad row count (N=%d, max_rows=%d)", N, p->max_rows);
    GpFwd f;
    memset(&f, 0, sizeof(f));
    f.N = N; f.obs = obs_dev; f.seed = seed; f.step = step; f.deterministic = deterministic != 0;
    f.action = action_dev; f.env_action = env_action_dev; f.logp = logp_dev; f.value = value_dev; f.entropy = entropy_dev;
    f.head = head_dev; f.eps = eps_dev;
    return gp_forward(p, f, (hipStream_t)stream);
}

int rl4rs_gpolicy_evaluate(rl4rs_gpolicy* p, int32_t N, const float* obs_dev, const float* actions_dev, float* logp_dev,
                           float* value_dev, float* entropy_dev, float* head_dev, void* stream) {
    RL4RS_REQUIRE(p && obs_dev && actions_dev, "gpolicy_evaluate: null argument");
    RL4RS_REQUIRE(N >= 1 && N <= p->max_rows, "gpolicy_evaluate: bad row count (N=%d, max_rows=%d)", N, p->max_rows);
    GpFwd f;
    memset(&f, 0, sizeof(f));
    f.N = N; f.obs = obs_dev; f.actions_in = actions_dev;
    f.logp = logp_dev; f.value = value_dev; f.entropy = entropy_dev; f.head = head_dev;
    return gp_forward(p, f, (hipStream_t)stream);
}

int rl4rs_gpolicy_loss_grad(rl4rs_gpolicy* p, int32_t algo, int32_t N, const float* obs_dev, const float* actions_dev,
                            const float* adv_dev, const float* ret_dev, const float* old_logp_dev, const float* old_value_dev,
                            const float* old_head_dev, float vf_coeff, float ent_coeff, float clip, float vf_clip, float kl_coeff,
                            float* grad_dev, float* stats_dev, void* stream) {
    RL4RS_REQUIRE(p && obs_dev && actions_dev && adv_dev && ret_dev && grad_dev, "gpolicy_loss_grad: null argument");
    RL4RS_REQUIRE(N >= 1 && N <= p->max_rows, "gpolicy_loss_grad: bad row count (N=%d, max_rows=%d)", N, p->max_rows);
    RL4RS_REQUIRE(algo == 0 || (algo == 1 && old_logp_dev && old_value_dev && old_head_dev),
                  "gpolicy_loss_grad: algo must be 0 (A2C) or 1 (PPO, which needs the old_* inputs)");
    return gp_loss_grad(p, algo, N, obs_dev, actions_dev, adv_dev, ret_dev, old_logp_dev, old_value_dev, old_head_dev, vf_coeff,
                        ent_coeff, clip, vf_clip, kl_coeff, grad_dev, stats_dev, (hipStream_t)stream);
}

int rl4rs_gpolicy_adam_step(rl4rs_gpolicy* p, const float* grad_dev, float lr, float beta1, float beta2, float eps, float grad_clip,
                            void* stream) {
    RL4RS_REQUIRE(p && grad_dev, "gpolicy_adam_step: null argument");
    // the shared Adam kernel (optim.hpp) behind this unit's float64-carried norm
    hipStream_t st = (hipStream_t)stream;
    const AdamTerms a = adam_advance(p->opt, ADAM_TF, lr, beta1, beta2, eps);
    if (grad_clip > 0.f) hipLaunchKernelGGL(k_gp_sumsq, dim3(1), dim3(256), 0, st, grad_dev, p->opt.n, p->sumsq);
    hipLaunchKernelGGL(k_adam, dim3((unsigned)((p->opt.n + 255) / 256)), dim3(256), 0, st, p->opt.params, grad_dev, p->opt.m, p->opt.v,
                       p->opt.n, a.lr_t, beta1, beta2, a.eps_or_bc2, p->sumsq, grad_clip, (const int32_t*)nullptr);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

int rl4rs_gpolicy_ppo_epoch(rl4rs_gpolicy* p, int32_t N, int32_t minibatch, const float* obs_dev, const float* actions_dev,
                            const float* adv_dev, const float* ret_dev, const float* old_logp_dev, const float* old_value_dev,
                            const float* old_head_dev, float vf_coeff, float ent_coeff, float clip, float vf_clip, float kl_coeff,
                            float lr, float beta1, float beta2, float eps, float grad_clip, float* grad_dev, float* stats_dev,
                            void* stream) {
    RL4RS_REQUIRE(p && obs_dev && actions_dev && adv_dev && ret_dev && old_logp_dev && old_value_dev && old_head_dev && grad_dev,
                  "gpolicy_ppo_epoch: null argument");
    RL4RS_REQUIRE(minibatch > 0 && N >= minibatch && N <= p->max_rows,
                  "gpolicy_ppo_epoch: bad sizes (N=%d, minibatch=%d, max_rows=%d)", N, minibatch, p->max_rows);
    hipStream_t st = (hipStream_t)stream;
    const size_t D = p->d.D, E = p->d.E;
    if (stats_dev) RL4RS_HIP_TRY(hipMemsetAsync(stats_dev + 4, 0, 16, st));
    for (int lo = 0; lo + minibatch <= N; lo += minibatch) {
        int rc = gp_loss_grad(p, 1, minibatch, obs_dev + lo * D, actions_dev + lo * E, adv_dev + lo, ret_dev + lo, old_logp_dev + lo,
                              old_value_dev + lo, old_head_dev + lo * 2 * E, vf_coeff, ent_coeff, clip, vf_clip, kl_coeff, grad_dev,
                              stats_dev, st);
        if (rc) return rc;
        if (stats_dev) {
            hipLaunchKernelGGL(k_gp_add4, dim3(1), dim3(64), 0, st, stats_dev, stats_dev + 4);
            RL4RS_LAUNCH_CHECK();
        }
        if ((rc = rl4rs_gpolicy_adam_step(p, grad_dev, lr, beta1, beta2, eps, grad_clip, stream))) return rc;
    }
    return RL4RS_OK;
}

int rl4rs_gpolicy_vtrace_loss_grad(rl4rs_gpolicy* p, int32_t R, int32_t T, int32_t B, const float* obs_dev, const float* actions_dev,
                                   const float* behaviour_logp_dev, const double* rewards_dev, float gamma, float clip_rho,
                                   float clip_pg_rho, int32_t drop_last, float vf_coeff, float ent_coeff, float* grad_dev,
                                   float* stats_dev, double* vtrace_stats_dev, void* stream) {
    RL4RS_REQUIRE(p && obs_dev && actions_dev && behaviour_logp_dev && rewards_dev && grad_dev, "gpolicy_vtrace_loss_grad: null argument");
    RL4RS_REQUIRE(R >= 1 && T >= 1 && B >= 1 && (int64_t)R * T * B <= (int64_t)p->max_rows,
                  "gpolicy_vtrace_loss_grad: bad sizes (R=%d, T=%d, B=%d, max_rows=%d)", R, T, B, p->max_rows);
    RL4RS_REQUIRE(!(drop_last && T < 2), "gpolicy_vtrace_loss_grad: drop_last needs T >= 2 (the dropped step's value is the bootstrap)");
    hipStream_t st = (hipStream_t)stream;
    const size_t D = p->d.D, E = p->d.E;
    const int N = R * T * B;
    const int Te = drop_last ? T - 1 : T;                  // steps the loss runs over
    const size_t per = (size_t)T * B, kept = (size_t)Te * B;
    const bool compact = drop_last && R > 1;
    int rc;
    if ((rc = gp_vtrace_scratch(p, compact))) return rc;
    // 1. the learner's forward on every row (the dropped step's value is the bootstrap)
    if ((rc = rl4rs_gpolicy_evaluate(p, N, obs_dev, actions_dev, p->vt_logp, p->vt_val, nullptr, nullptr, stream))) return rc;
    // 2. V-trace per rollout (the float64 scan of rl4rs_vtrace); vs / pg_adv of the kept rows are written back to back ([R, Te, B])
    if (vtrace_stats_dev && R > 1 && p->vt_stats_cap < R) {      // per-rollout sums, added in rollout order below
        float* s8;
        if ((rc = gp_alloc(p, &s8, (size_t)8 * R))) return rc;
        p->vt_stats = reinterpret_cast<double*>(s8);
        p->vt_stats_cap = R;
    }
    for (int r = 0; r < R; ++r) {
        const size_t o = r * per;
        double* vst = !vtrace_stats_dev ? nullptr : (R == 1 ? vtrace_stats_dev : p->vt_stats + 4 * r);
        if ((rc = rl4rs_vtrace(Te, B, behaviour_logp_dev + o, p->vt_logp + o, p->vt_val + o, drop_last ? p->vt_val + o + kept : nullptr,
                               rewards_dev + o, nullptr, gamma, clip_rho, clip_pg_rho, p->vt_vs + r * kept, p->vt_pg + r * kept, vst,
                               stream)))
            return rc;
    }
    if (vtrace_stats_dev && R > 1) {
        hipLaunchKernelGGL(k_gp_sum_stats, dim3(1), dim3(64), 0, st, p->vt_stats, R, vtrace_stats_dev);
        RL4RS_LAUNCH_CHECK();
    }
    // 3. the A2C-form loss on the kept rows only.  One rollout's kept rows are a prefix of its buffers; those of several rollouts
    // are copied together first.
    const float* obs_k = obs_dev;
    const float* act_k = actions_dev;
    if (compact) {
        for (int r = 0; r < R; ++r) {
            RL4RS_HIP_TRY(hipMemcpyAsync(p->vt_obs + r * kept * D, obs_dev + r * per * D, kept * D * 4, hipMemcpyDeviceToDevice, st));
            RL4RS_HIP_TRY(hipMemcpyAsync(p->vt_act + r * kept * E, actions_dev + r * per * E, kept * E * 4, hipMemcpyDeviceToDevice, st));
        }
        obs_k = p->vt_obs; act_k = p->vt_act;
    }
    return gp_loss_grad(p, 0, (int)(R * kept), obs_k, act_k, p->vt_pg, p->vt_vs, nullptr, nullptr, nullptr, vf_coeff, ent_coeff, 0.f, 0.f,
                        0.f, grad_dev, stats_dev, st);
}

}  // extern "C"
