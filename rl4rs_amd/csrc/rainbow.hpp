// On-device Rainbow (include/rl4rs_hip.h, "On-device Rainbow"): the distributional (C51) dueling Q network on a handle of its own
// (rl4rs_distq), its fused head (MFMA GEMM + dueling centring + softmax over atoms + sum z p + SoftQ draw / first maximum), the
// categorical Bellman projection with the cross-entropy loss and its rank-sparse backward, and the n-step form of the replay draw.
// Compiled into policy.hip behind dqn.hpp: the replay ring, masked_first_max, the sample-axis
// reductions (k_gemm_tn, k_reduce_chunks, k_reduce_terms), uniform01 and the wave reductions live there.
//
// Reference: script/modelfree_train.py:50-53,146-178 (algo "RAINBOW": num_atoms 8 over [0, 1000], everything else RLlib 1.5.1's DQN
// defaults: dueling, double_q, n_step 3, hiddens [256] -> here the two 128-wide streams, fcnet_hiddens [256, 256] tanh, no custom
// model, support_rllib_mask forced False).  RLlib's dqn_tf_policy / distributional_q_tf_model are third-party and absent: restated
// from their published 1.5.1 form, PARITY UNPINNED, checked against the fp64 restatement in tests/rainbow_ref.py.
//
// Flat parameters: W1 [OD, TR] | b1 | W2 [TR, TR] | b2 | Wa1 [TR, SH] | ba1 | Wa2 [SH, A * AT] | ba2 [| Wv1 [TR, SH] | bv1 | Wv2 [SH, AT] | bv2]
// (column a * AT + j of Wa2 is atom j of action a; the value stream exists with dueling only).
//   logits[a, j] = V[j] + Adv[a, j] - mean_a' Adv[a', j],   p[a, :] = softmax_j,   Q[a] = sum_j z_j p[a, j]
// The dense layers up to the two stream activations are the generic MFMA GEMMs.  The head never writes its [rows, A * AT] logits:
//   * mean_a' Adv[a', j] = h_a . Wbar[:, j] + bbar[j] with Wbar = the mean of Wa2 over the actions ([SH, AT], k_distq_wbar, once per
//     parameter version), so a tile of actions is centred without having seen the others;
//   * an update needs the logits of ONE action per row at s and the target distribution of ONE action per row at s', and its
//     gradient is one AT-vector g per row: dV = g, dAdv[a', :] = g (delta(a' = a) - 1 / A).  dWa2 is gathered column by column
//     (k_dqn_w2_grad's form) plus -(1 / A) h_a^T g on every action; d h_a = sum_j g[j] (Wa2[:, a, j] - Wbar[:, j]).
// Every sum runs in a fixed order: bit-identical from run to run.
#pragma once

namespace rl4rs {

enum { DISTQ_SOFTQ = 0, DISTQ_GREEDY = 1 };
constexpr int DISTQ_CHUNK_COLS = 256;     // logits columns of one action chunk of the head kernel (whole actions, >= 1)

struct DistqDims { int OD, TR, SH, A, AT, W, dueling; float vmin, dz; };

// pointers into one flat parameter (or gradient) buffer
template <typename T>
struct DistqPtrs { T *W1, *b1, *W2, *b2, *Wa1, *ba1, *Wa2, *ba2, *Wv1, *bv1, *Wv2, *bv2; };
template <typename T>
static inline DistqPtrs<T> distq_ptrs(T* p, const DistqDims& d) {
    DistqPtrs<T> q;
    q.W1 = p; q.b1 = q.W1 + (size_t)d.OD * d.TR;
    q.W2 = q.b1 + d.TR; q.b2 = q.W2 + (size_t)d.TR * d.TR;
    q.Wa1 = q.b2 + d.TR; q.ba1 = q.Wa1 + (size_t)d.TR * d.SH;
    q.Wa2 = q.ba1 + d.SH; q.ba2 = q.Wa2 + (size_t)d.SH * d.A * d.AT;
    q.Wv1 = q.ba2 + (size_t)d.A * d.AT; q.bv1 = q.Wv1 + (size_t)d.TR * d.SH;
    q.Wv2 = q.bv1 + d.SH; q.bv2 = q.Wv2 + (size_t)d.SH * d.AT;
    if (!d.dueling) { q.Wv1 = nullptr; q.bv1 = nullptr; q.Wv2 = nullptr; q.bv2 = nullptr; }
    return q;
}

// wbar[k, j] = mean over a of Wa2[k, a * AT + j] for k < SH; row SH is the same mean of ba2.  One thread per output, actions in order.
__global__ void k_distq_wbar(int SH, int A, int AT, const float* __restrict__ Wa2, const float* __restrict__ ba2, float* __restrict__ wbar) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (SH + 1) * AT) return;
    const int k = i / AT, j = i - k * AT;
    const float* src = k < SH ? Wa2 + (size_t)k * A * AT : ba2;
    float s = 0.f;
    for (int a = 0; a < A; ++a) s += src[(size_t)a * AT + j];
    wbar[i] = s / (float)A;
}

__device__ __forceinline__ bool distq_allowed(const uint32_t* mrow, int a) { return mrow ? ((mrow[a >> 5] >> (a & 31)) & 1u) != 0 : true; }

struct DistqHead {
    DistqDims d;
    int N, mode, ac, ld;                  // ac = actions per chunk, ld = row stride of the chunk's logits in LDS (odd)
    float inv_temp;
    uint32_t seed, step;
    const float* Ha; const float* Hv;     // [N, SH] stream activations (Hv: dueling only)
    const float* Wa2; const float* ba2; const float* Wv2; const float* bv2; const float* wbar;
    const uint32_t* mask;
    int32_t* actions; float* u_out; float* q_out;
};

// The fused head: a workgroup owns 32 rows.  Its advantage activations sit in LDS transposed (MFMA A fragments are then
// conflict-free reads), base[r, j] = V[j] - mean_a' Adv[a', j] is made once, then chunks of whole actions go through
// [32 x SH] x [SH x 32] fp32 MFMA tiles (one tile per wave and trip) into LDS, where (row, action) pairs take the softmax over
// their atoms and leave Q[a] = sum z p in the row's LDS Q vector.  The finish of a row (one wave): mask, then the SoftQ
// inverse-CDF draw or the first maximum.
__global__ __launch_bounds__(256) void k_distq_head(DistqHead a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const DistqDims& d = a.d;
    float* sHa = reinterpret_cast<float*>(smem);              // [SH][32]
    float* sBase = sHa + (size_t)d.SH * 32;                   // [32][AT]
    float* sL = sBase + 32 * d.AT;                            // [32][ld]
    float* sQ = sL + 32 * a.ld;                               // [32][A]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = lane >> 5, li = lane & 31;
    const int r0 = blockIdx.x * 32;
    for (int i = tid; i < 32 * d.SH; i += 256) {
        const int r = i / d.SH, k = i - r * d.SH;
        sHa[k * 32 + r] = (r0 + r < a.N) ? a.Ha[(size_t)(r0 + r) * d.SH + k] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < 32 * d.AT; i += 256) {
        const int r = i / d.AT, j = i - r * d.AT;
        float base = 0.f;
        if (d.dueling && r0 + r < a.N) {
            float v = a.bv2[j], m = a.wbar[d.SH * d.AT + j];
            const float* hv = a.Hv + (size_t)(r0 + r) * d.SH;
            for (int k = 0; k < d.SH; ++k) {
                v = fmaf(hv[k], a.Wv2[k * d.AT + j], v);
                m = fmaf(sHa[k * 32 + r], a.wbar[k * d.AT + j], m);
            }
            base = v - m;
        }
        sBase[i] = base;
    }
    const int ldw = d.A * d.AT;
    for (int a0 = 0; a0 < d.A; a0 += a.ac) {
        const int na = min(a.ac, d.A - a0), ncols = na * d.AT, c0 = a0 * d.AT;
        for (int t = wave; t * 32 < ncols; t += 4) {
            const bool c_ok = t * 32 + li < ncols;
            const float* wcol = a.Wa2 + c0 + t * 32 + li;
            f32x16 acc;
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            for (int k = 0; k < d.SH; k += 16) {              // 8 operand pairs requested together, then the 8 MFMAs
                float av[8], bv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int kk = k + 2 * u + half;
                    av[u] = sHa[kk * 32 + li];
                    bv[u] = c_ok ? wcol[(size_t)kk * ldw] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
            }
            if (c_ok) {
                const float bias = a.ba2[c0 + t * 32 + li];
                for (int r = 0; r < 16; ++r) sL[((r & 3) + 8 * (r >> 2) + 4 * half) * a.ld + t * 32 + li] = acc[r] + bias;
            }
        }
        __syncthreads();
        for (int p = tid; p < 32 * na; p += 256) {
            const int al = p >> 5, r = p & 31;
            const float* l = sL + r * a.ld + al * d.AT;
            const float* bs = sBase + r * d.AT;
            float mx = -3.4028235e38f;
            for (int j = 0; j < d.AT; ++j) mx = fmaxf(mx, l[j] + bs[j]);
            float se = 0.f, sz = 0.f;
            for (int j = 0; j < d.AT; ++j) {
                const float e = expf((l[j] + bs[j]) - mx);
                se += e;
                sz = fmaf(d.vmin + (float)j * d.dz, e, sz);
            }
            sQ[r * d.A + a0 + al] = sz / se;
        }
        __syncthreads();
    }
    // finish: one wave per row; lane l owns actions l, l + 64, ... of the row's Q vector from here on
    for (int r = wave; r < 32; r += 4) {
        const int n = r0 + r;
        if (n >= a.N) break;
        float* q = sQ + r * d.A;
        const uint32_t* mrow = a.mask ? a.mask + (size_t)n * d.W : nullptr;
        for (int c = lane; c < d.A; c += 64) {
            float v = q[c];
            if (!distq_allowed(mrow, c)) v = -3.4028235e38f;
            q[c] = v;
            if (a.q_out) a.q_out[(size_t)n * d.A + c] = v;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        bool legal;
        const int best = masked_first_max(q, mrow, d.A, lane, false, &legal);
        int act = best;
        if (a.mode == DISTQ_SOFTQ) {
            const float u = uniform01(a.seed, a.step, (uint32_t)n, 0u);
            if (a.u_out && lane == 0) a.u_out[n] = u;
            if (!legal) {
                act = 0;
            } else {
                const float mx = q[best];
                float run = 0.f;
                for (int c0 = 0; c0 < d.A; c0 += 64) {         // inclusive prefix of exp((Q - max) / temperature) in action order
                    const int c = c0 + lane;
                    float e = (c < d.A && distq_allowed(mrow, c)) ? expf((q[c] - mx) * a.inv_temp) : 0.f;
                    for (int o = 1; o < 64; o <<= 1) {
                        const float up = __shfl_up(e, o);
                        if (lane >= o) e += up;
                    }
                    const float cdf = run + e;
                    if (c < d.A) q[c] = cdf;
                    run = __shfl(cdf, 63);
                }
                const float target = u * run;
                for (int c0 = 0; c0 < d.A; c0 += 64) {         // the smallest action whose prefix exceeds u * total
                    const int c = c0 + lane;
                    const unsigned long long hit = __ballot(c < d.A && q[c] > target);
                    if (hit) { act = c0 + __ffsll((long long)hit) - 1; break; }
                }
            }
        }
        if (lane == 0) a.actions[n] = act;
    }
}

struct DistqRows {
    DistqDims d;
    int N, AP;                            // AP = the power of two >= AT: lane = (k group) * AP + atom
    float gamma_n, vmax;
    const float* Wa2; const float* ba2; const float* Wv2; const float* bv2; const float* wbar;          // online
    const float* tWa2; const float* tba2; const float* tWv2; const float* tbv2; const float* twbar;     // target
    const float* Ha; const float* Hv; const float* tHa; const float* tHv;
    const int32_t* act; const float* rew; const int32_t* done; const float* w; const uint32_t* next_mask; const int32_t* astar_in;
    float* G; float* dHa; float* dHv; float* td; int32_t* astar_out; float4* terms;
};

// dot of one hidden row with column col0 + j of a [SH, ld] matrix for every atom j at once: k is split over the 64 / AP lane groups
// (group g takes k = g, g + ng, ...), the group partials meet in a fixed butterfly.  Valid in every lane with j < AT.
__device__ __forceinline__ float distq_dot(const float* __restrict__ h, const float* __restrict__ Wm, int ld, int col0, int SH, int AT,
                                           int AP, int lane) {
    const int j = lane & (AP - 1), g = lane / AP, ng = 64 / AP;
    float s = 0.f;
    if (j < AT)
        for (int k = g; k < SH; k += ng) s = fmaf(h[k], Wm[(size_t)k * ld + col0 + j], s);
    for (int o = AP; o < 64; o <<= 1) s += __shfl_xor(s, o);
    return s;
}

// logits of ONE action of one row (lane j < AT of every group holds atom j)
__device__ __forceinline__ float distq_logit(const DistqDims& d, const float* ha, const float* hv, const float* Wa2, const float* ba2,
                                             const float* Wv2, const float* bv2, const float* wbar, int action, int AP, int lane) {
    const int j = lane & (AP - 1);
    float l = distq_dot(ha, Wa2, d.A * d.AT, action * d.AT, d.SH, d.AT, AP, lane);
    if (j < d.AT) l += ba2[action * d.AT + j];
    if (d.dueling) {
        float v = distq_dot(hv, Wv2, d.AT, 0, d.SH, d.AT, AP, lane);
        float m = distq_dot(ha, wbar, d.AT, 0, d.SH, d.AT, AP, lane);
        if (j < d.AT) l = (v + bv2[j]) + (l - (m + wbar[d.SH * d.AT + j]));
    }
    return l;
}

// One wave per row: the taken action's logits at s, the target distribution of a* at s', the categorical projection, the
// cross-entropy, g = w / N (softmax - m) and the gradient of the two stream activations' pre-activations.  A row that does not
// bootstrap (terminal, or a successor that allows nothing) projects the single point clip(R): a select, nothing of the successor
// (NaN included) is read into any output.
__global__ __launch_bounds__(256) void k_distq_rows(DistqRows a) {
    __shared__ float s_p[4][64], s_g[4][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + wave;
    if (n >= a.N) return;
    const DistqDims& d = a.d;
    const int AT = d.AT, j = lane & (a.AP - 1);
    const bool own = lane < AT;                                // group 0 holds each atom once
    const int act = max(0, min(a.act[n], d.A - 1));
    const bool done = a.done[n] != 0;
    int astar = -1;
    bool boot = false;
    if (!done) {
        astar = max(0, min(a.astar_in[n], d.A - 1));
        bool any = a.next_mask == nullptr;
        if (a.next_mask)
            for (int c = lane; c < d.A; c += 64) any = any || distq_allowed(a.next_mask + (size_t)n * d.W, c);
        boot = __any(any ? 1 : 0) != 0;
    }
    const float* ha = a.Ha + (size_t)n * d.SH;
    const float* hv = d.dueling ? a.Hv + (size_t)n * d.SH : nullptr;
    // target distribution p'(s')[a*, :]
    float pj = 0.f;
    if (boot) {
        const float lt = distq_logit(d, a.tHa + (size_t)n * d.SH, d.dueling ? a.tHv + (size_t)n * d.SH : nullptr, a.tWa2, a.tba2, a.tWv2,
                                     a.tbv2, a.twbar, astar, a.AP, lane);
        const float mx = wave_max(j < AT ? lt : -3.4028235e38f);
        const float e = own ? expf(lt - mx) : 0.f;
        pj = e / wave_sum(e);
    }
    s_p[wave][lane] = pj;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // projection, gathered: lane i sums what every source atom sends to atom i, sources in order
    const float R = a.rew[n], top = (float)(AT - 1);
    float m = 0.f;
    if (own) {
        const float fi = (float)lane;
        const int nsrc = boot ? AT : 1;
        for (int s = 0; s < nsrc; ++s) {
            const float zt = boot ? R + a.gamma_n * (d.vmin + (float)s * d.dz) : R;
            const float rt = fminf(fmaxf(zt, d.vmin), a.vmax);
            const float b = fminf(fmaxf((rt - d.vmin) / d.dz, 0.f), top);
            const float lo = floorf(b), up = ceilf(b), eq = (up - lo < 0.5f) ? 1.f : 0.f;
            const float ps = boot ? s_p[wave][s] : 1.f;
            if (fi == lo) m += ps * (up - b + eq);
            if (fi == up) m += ps * (b - lo);
        }
    }
    // online logits of the taken action, log-softmax, cross-entropy
    const float l = distq_logit(d, ha, hv, a.Wa2, a.ba2, a.Wv2, a.bv2, a.wbar, act, a.AP, lane);
    const float mx = wave_max(j < AT ? l : -3.4028235e38f);
    const float se = wave_sum(own ? expf(l - mx) : 0.f);
    const float lsm = (l - mx) - logf(se);
    const float sm = own ? expf(lsm) : 0.f;
    const float zi = d.vmin + (float)lane * d.dz;
    const float td = -wave_sum(own ? m * lsm : 0.f);
    const float qsa = wave_sum(own ? zi * sm : 0.f);
    const float ez = wave_sum(own ? zi * m : 0.f);
    const float wgt = a.w ? a.w[n] : 1.f;
    const float g = own ? wgt / (float)a.N * (sm - m) : 0.f;
    s_g[wave][lane] = g;
    if (own) a.G[(size_t)n * AT + lane] = g;
    if (lane == 0) {
        a.td[n] = td;
        if (a.astar_out) a.astar_out[n] = astar;
        a.terms[n] = make_float4(wgt * td, qsa, ez, td);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const int ldw = d.A * AT;
    for (int k = lane; k < d.SH; k += 64) {
        float da = 0.f, dv = 0.f;
        for (int s = 0; s < AT; ++s) {
            const float gs = s_g[wave][s];
            const float wa = a.Wa2[(size_t)k * ldw + act * AT + s];
            da = fmaf(gs, d.dueling ? wa - a.wbar[k * AT + s] : wa, da);
            if (d.dueling) dv = fmaf(gs, a.Wv2[k * AT + s], dv);
        }
        a.dHa[(size_t)n * d.SH + k] = ha[k] > 0.f ? da : 0.f;
        if (d.dueling) a.dHv[(size_t)n * d.SH + k] = hv[k] > 0.f ? dv : 0.f;
    }
}

// dWa2[:, c] for column c = a' * AT + j: the sum over the rows that took a' of g[n, j] * h_a[n, :], rows in order (k_dqn_w2_grad's
// walk), plus the dueling term -(1 / A) S[:, j] that every action gets (S = h_a^T g, sg = the column sums of g); dba2 likewise.
// Every column is written whole.
__global__ __launch_bounds__(256) void k_distq_wa2_grad(int N, int SH, int A, int AT, const int32_t* __restrict__ act,
                                                        const float* __restrict__ G, const float* __restrict__ H,
                                                        const float* __restrict__ S, const float* __restrict__ sg, float minus_inv_a,
                                                        float* __restrict__ gW, float* __restrict__ gb) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + wave;
    if (c >= A * AT) return;
    const int ap = c / AT, j = c - ap * AT;
    for (int k0 = 0; k0 < SH; k0 += 64) {
        const int k = k0 + lane;
        float acc = 0.f, bsum = 0.f;
        for (int n0 = 0; n0 < N; n0 += 64) {
            const int an = (n0 + lane < N) ? max(0, min(act[n0 + lane], A - 1)) : -1;
            unsigned long long mm = __ballot(an == ap);
            while (mm) {
                const int n = n0 + __ffsll((long long)mm) - 1;
                mm &= mm - 1;
                const float gn = G[(size_t)n * AT + j];
                bsum += gn;
                if (k < SH) acc = fmaf(gn, H[(size_t)n * SH + k], acc);
            }
        }
        if (k < SH) gW[(size_t)k * A * AT + c] = S ? acc + minus_inv_a * S[k * AT + j] : acc;
        if (k0 == 0 && lane == 0) gb[c] = S ? bsum + minus_inv_a * sg[j] : bsum;
    }
}

// out = (x [+ y]) * (1 - h * h): the gradient through a tanh layer whose output is h
__global__ void k_distq_tanh_grad(int n, const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ h,
                                  float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = y ? x[i] + y[i] : x[i], t = h[i];
    out[i] = v * (1.f - t * t);
}

struct ReplayNstep {
    int M, B, T, rows_per, OD, W, n_step, vec4;
    double gamma;
    const float* obs; const uint32_t* mask; const float* rew; const int32_t* idx;
    float* next_obs_out; uint32_t* next_mask_out; float* rew_out; int32_t* done_out;
};

// The n-step form of a draw k_replay_sample has made (RLlib's adjust_nstep on complete episodes): one wave per draw rewrites the
// reward (k = min(n, T - t) terms, accumulated in float64 in step order), done = (t + n >= T) and the successor = row idx + k B.
__global__ __launch_bounds__(256) void k_replay_nstep(ReplayNstep a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + wave;
    if (m >= a.M) return;
    const int idx = a.idx[m];
    const int t = (idx % a.rows_per) / a.B;
    const int k = min(a.n_step, a.T - t);
    const bool done = t + a.n_step >= a.T;
    const int nxt = done ? idx : idx + k * a.B;               // a terminal row has no successor: any finite row will do
    const float* sn = a.obs + (size_t)nxt * a.OD;
    float* d_n = a.next_obs_out + (size_t)m * a.OD;
    if (a.vec4) {
        typedef float f4 __attribute__((ext_vector_type(4)));
        for (int c = lane; c < a.OD / 4; c += 64) reinterpret_cast<f4*>(d_n)[c] = reinterpret_cast<const f4*>(sn)[c];
    } else {
        for (int c = lane; c < a.OD; c += 64) d_n[c] = sn[c];
    }
    for (int c = lane; c < a.W; c += 64) a.next_mask_out[(size_t)m * a.W + c] = a.mask[(size_t)nxt * a.W + c];
    if (lane == 0) {
        double R = 0.0, disc = 1.0;
        for (int s = 0; s < k; ++s) {
            R += disc * (double)a.rew[idx + s * a.B];
            disc *= a.gamma;
        }
        a.rew_out[m] = (float)R;
        a.done_out[m] = done ? 1 : 0;
    }
}

}  // namespace rl4rs

struct rl4rs_distq {
    rl4rs_distq_cfg c;
    DistqDims d;
    int nseg, AP, chunk_cap;              // Adam variables (8 or 12); pow2 >= atoms; most sample chunks of a reduction
    int64_t seg_end[12];
    OptBlock opt;
    float* sumsq;
    float *wbar, *twbar;                  // [(SH + 1) * AT] of the handle's parameters / of the last loss call's target parameters
    bool wbar_valid;
    float *H1, *H2, *Ha, *Hv, *tH1, *tH2, *tHa, *tHv, *nH1, *nH2, *nHa, *nHv;
    float *G, *dHa, *dHv, *T1, *T2, *dH2, *dH1, *S, *sg, *part, *part_b;
    float4* terms;
    int32_t* astar;
    std::vector<void*> owned;
};

static int64_t distq_layout(const rl4rs_distq_cfg& c, int64_t* seg_end) {
    const int64_t OD = c.obs_dim, TR = c.trunk, SH = c.stream_hidden, A = c.action_size, AT = c.atoms;
    const int64_t sizes[12] = {OD * TR, TR, TR * TR, TR, TR * SH, SH, SH * A * AT, A * AT, TR * SH, SH, SH * AT, AT};
    const int nseg = c.dueling ? 12 : 8;
    int64_t o = 0;
    for (int i = 0; i < nseg; ++i) { o += sizes[i]; if (seg_end) seg_end[i] = o; }
    return o;
}

static int distq_check_cfg(const rl4rs_distq_cfg* c) {
    RL4RS_REQUIRE(c, "distq: null config");
    RL4RS_REQUIRE(c->obs_dim > 0 && c->action_size > 1 && c->action_size <= 512 && c->atoms >= 2 && c->atoms <= 64 && c->max_rows > 0 &&
                  c->max_rows <= (1 << 20) && c->obs_dim <= 2048,
                  "distq: 0 < obs_dim <= 2048, 2 <= action_size <= 512, 2 <= atoms <= 64, 0 < max_rows <= 2^20 (got %d, %d, %d, %d)", c->obs_dim,
                  c->action_size, c->atoms, c->max_rows);
    RL4RS_REQUIRE(c->trunk > 0 && c->trunk % 32 == 0 && c->stream_hidden > 0 && c->stream_hidden % 32 == 0 && c->stream_hidden <= 256 &&
                  c->trunk <= 1024, "distq: trunk (<= 1024) and stream_hidden (<= 256) must be multiples of 32 (got %d, %d)", c->trunk,
                  c->stream_hidden);
    RL4RS_REQUIRE(c->v_max > c->v_min, "distq: v_max must exceed v_min");
    RL4RS_REQUIRE(c->dueling == 0 || c->dueling == 1, "distq: dueling is 0 or 1");
    return RL4RS_OK;
}

// head launch geometry: actions per chunk, LDS row stride of a chunk's logits, dynamic LDS bytes
static void distq_head_geom(const DistqDims& d, int* ac, int* ld, size_t* smem) {
    *ac = std::max(1, DISTQ_CHUNK_COLS / d.AT);
    *ld = (std::min(*ac, d.A) * d.AT + 31) / 32 * 32 + 1;
    *smem = ((size_t)d.SH * 32 + (size_t)32 * d.AT + (size_t)32 * *ld + (size_t)32 * d.A) * 4;
}

static int distq_wbar(rl4rs_distq* p, const float* prm, float* out, hipStream_t st) {
    const DistqDims& d = p->d;
    const DistqPtrs<const float> q = distq_ptrs<const float>(prm, d);
    const int n = (d.SH + 1) * d.AT;
    hipLaunchKernelGGL(k_distq_wbar, dim3((n + 255) / 256), dim3(256), 0, st, d.SH, d.A, d.AT, q.Wa2, q.ba2, out);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

// trunk and streams of N rows with the parameters prm: H1, H2 tanh, Ha (and Hv) relu
static int distq_hidden(rl4rs_distq* p, const float* prm, int N, const float* obs, float* H1, float* H2, float* Ha, float* Hv, hipStream_t st) {
    const DistqDims& d = p->d;
    const DistqPtrs<const float> q = distq_ptrs<const float>(prm, d);
    int rc;
    if ((rc = launch_gemm_f32(obs, d.OD, q.W1, d.TR, q.b1, H1, d.TR, N, d.TR, d.OD, ACT_TANH, st))) return rc;
    if ((rc = launch_gemm_f32(H1, d.TR, q.W2, d.TR, q.b2, H2, d.TR, N, d.TR, d.TR, ACT_TANH, st))) return rc;
    if ((rc = launch_gemm_f32(H2, d.TR, q.Wa1, d.SH, q.ba1, Ha, d.SH, N, d.SH, d.TR, ACT_RELU, st))) return rc;
    if (d.dueling && (rc = launch_gemm_f32(H2, d.TR, q.Wv1, d.SH, q.bv1, Hv, d.SH, N, d.SH, d.TR, ACT_RELU, st))) return rc;
    return RL4RS_OK;
}

static int distq_head(rl4rs_distq* p, const float* prm, const float* wbar, int N, const float* Ha, const float* Hv, const uint32_t* mask,
                      int mode, float temperature, uint32_t seed, uint32_t step, int32_t* actions, float* u_out, float* q_out, hipStream_t st) {
    DistqHead a;
    memset(&a, 0, sizeof(a));
    const DistqPtrs<const float> q = distq_ptrs<const float>(prm, p->d);
    size_t smem;
    a.d = p->d; a.N = N; a.mode = mode;
    distq_head_geom(p->d, &a.ac, &a.ld, &smem);
    a.inv_temp = 1.f / temperature; a.seed = seed; a.step = step;
    a.Ha = Ha; a.Hv = Hv; a.Wa2 = q.Wa2; a.ba2 = q.ba2; a.Wv2 = q.Wv2; a.bv2 = q.bv2; a.wbar = wbar;
    a.mask = mask; a.actions = actions; a.u_out = u_out; a.q_out = q_out;
    int rc = raise_dyn_smem(reinterpret_cast<const void*>(&k_distq_head), smem);
    if (rc) return rc;
    hipLaunchKernelGGL(k_distq_head, dim3((N + 31) / 32), dim3(256), smem, st, a);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

static int distq_forward_act(rl4rs_distq* p, int N, const float* obs, const uint32_t* mask, int mode, float temperature, uint32_t seed,
                             uint32_t step, int32_t* actions, float* u_out, float* q_out, hipStream_t st) {
    int rc;
    if (!p->wbar_valid) {
        if ((rc = distq_wbar(p, p->opt.params, p->wbar, st))) return rc;
        p->wbar_valid = true;
    }
    if ((rc = distq_hidden(p, p->opt.params, N, obs, p->nH1, p->nH2, p->nHa, p->nHv, st))) return rc;
    return distq_head(p, p->opt.params, p->wbar, N, p->nHa, p->nHv, mask, mode, temperature, seed, step, actions, u_out, q_out, st);
}

extern "C" {

int64_t rl4rs_distq_param_count(const rl4rs_distq_cfg* cfg) {
    if (distq_check_cfg(cfg) != RL4RS_OK) return -1;
    return distq_layout(*cfg, nullptr);
}

int rl4rs_distq_destroy(rl4rs_distq* p) {
    if (!p) return RL4RS_OK;
    for (void* q : p->owned) (void)hipFree(q);
    delete p;
    return RL4RS_OK;
}

int rl4rs_distq_create(const rl4rs_distq_cfg* cfg, const float* params_host, void* stream, rl4rs_distq** out) {
    int rc = distq_check_cfg(cfg);
    if (rc) return rc;
    RL4RS_REQUIRE(params_host && out, "distq_create: null argument");
    DistqDims d;
    d.OD = cfg->obs_dim; d.TR = cfg->trunk; d.SH = cfg->stream_hidden; d.A = cfg->action_size; d.AT = cfg->atoms;
    d.W = (cfg->action_size + 31) / 32; d.dueling = cfg->dueling; d.vmin = cfg->v_min;
    d.dz = (cfg->v_max - cfg->v_min) / (float)(cfg->atoms - 1);
    {
        int ac, ld;
        size_t smem;
        distq_head_geom(d, &ac, &ld, &smem);
        RL4RS_REQUIRE(smem <= POLICY_LDS_MAX, "distq_create: the head kernel needs %zu bytes of LDS for this shape (limit %zu)", smem,
                      POLICY_LDS_MAX);
    }
    if (rl4rs_device_count() <= 0) {
        set_error("no HIP device visible: librl4rs_hip has no CPU fallback");
        return RL4RS_EHIP;
    }
    rl4rs_distq* p = new rl4rs_distq();
    p->c = *cfg; p->d = d;
    p->nseg = cfg->dueling ? 12 : 8;
    p->opt.n = distq_layout(*cfg, p->seg_end);
    p->opt.t = 0;
    p->wbar_valid = false;
    p->AP = 2;
    while (p->AP < d.AT) p->AP <<= 1;
    const size_t R = (size_t)cfg->max_rows;
    p->chunk_cap = (int)std::min<size_t>(64, (R + 255) / 256);
    rc = RL4RS_OK;
    auto alloc = [&](auto** dst, size_t n) {
        if (rc) return;
        rc = dev_alloc(dst, n);
        if (rc == RL4RS_OK) p->owned.push_back(*dst);
    };
    const size_t np = (size_t)p->opt.n, TR = (size_t)d.TR, SH = (size_t)d.SH, AT = (size_t)d.AT;
    alloc(&p->opt.params, np); alloc(&p->opt.grad, np); alloc(&p->opt.m, np); alloc(&p->opt.v, np); alloc(&p->sumsq, 12);
    alloc(&p->wbar, (SH + 1) * AT); alloc(&p->twbar, (SH + 1) * AT);
    float** trunk[6] = {&p->H1, &p->H2, &p->tH1, &p->tH2, &p->nH1, &p->nH2};
    for (float** b : trunk) alloc(b, R * TR);
    float** streams[6] = {&p->Ha, &p->Hv, &p->tHa, &p->tHv, &p->nHa, &p->nHv};
    for (float** b : streams) alloc(b, R * SH);
    alloc(&p->G, R * AT); alloc(&p->dHa, R * SH); alloc(&p->dHv, R * SH);
    alloc(&p->T1, R * TR); alloc(&p->T2, R * TR); alloc(&p->dH2, R * TR); alloc(&p->dH1, R * TR);
    alloc(&p->S, SH * AT); alloc(&p->sg, AT);
    const size_t widest = std::max(std::max((size_t)d.OD * TR, TR * TR), std::max(TR * SH, SH * AT));      // the largest reduced matrix
    alloc(&p->part, (size_t)p->chunk_cap * widest);
    alloc(&p->part_b, (size_t)p->chunk_cap * std::max(std::max(TR, SH), AT));
    alloc(&p->terms, R); alloc(&p->astar, R);
    if (rc) { rl4rs_distq_destroy(p); return rc; }
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(p->opt.params, params_host, np * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(p->opt.m, 0, np * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(p->opt.v, 0, np * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(p->opt.grad, 0, np * 4, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        set_error("distq_create: initialisation failed: %s", hipGetErrorString(e));
        rl4rs_distq_destroy(p);
        return RL4RS_EHIP;
    }
    *out = p;
    return RL4RS_OK;
}

int rl4rs_distq_params(rl4rs_distq* p, float** params_dev, float** grad_dev, int64_t* count) {
    if (p) p->wbar_valid = false;          // the caller may write through the pointer
    return opt_params(RL4RS_OPT(p), params_dev, grad_dev, count, "distq_params");
}

int rl4rs_distq_copy_params(rl4rs_distq* dst, const rl4rs_distq* src, void* stream) {
    RL4RS_REQUIRE(dst && src && dst->opt.n == src->opt.n && dst->c.dueling == src->c.dueling && dst->c.atoms == src->c.atoms &&
                  dst->c.action_size == src->c.action_size, "distq_copy_params: the two networks differ in shape");
    dst->wbar_valid = false;
    return opt_copy_params(&dst->opt, &src->opt, stream, "distq_copy_params");
}

int rl4rs_distq_adam_state(rl4rs_distq* p, float** m_dev, float** v_dev, int64_t* step) {
    return opt_adam_state(RL4RS_OPT(p), m_dev, v_dev, step, "distq_adam_state");
}

int rl4rs_distq_set_adam_step(rl4rs_distq* p, int64_t step) {
    return opt_set_adam_step(RL4RS_OPT(p), step, "distq_set_adam_step");
}

int rl4rs_distq_act(rl4rs_distq* p, int32_t N, const float* obs, const uint32_t* mask_bits, float temperature, uint32_t seed, uint32_t step,
                    int32_t* actions, float* u_out, float* q_out, void* stream) {
    RL4RS_REQUIRE(p && obs && actions && N > 0 && N <= p->c.max_rows && temperature > 0.f, "distq_act: bad argument (N=%d, max_rows=%d)", N,
                  p ? p->c.max_rows : -1);
    return distq_forward_act(p, N, obs, mask_bits, DISTQ_SOFTQ, temperature, seed, step, actions, u_out, q_out, (hipStream_t)stream);
}

int rl4rs_distq_greedy(rl4rs_distq* p, int32_t N, const float* obs, const uint32_t* mask_bits, int32_t* actions, float* q_out, void* stream) {
    RL4RS_REQUIRE(p && obs && actions && N > 0 && N <= p->c.max_rows, "distq_greedy: bad argument (N=%d, max_rows=%d)", N,
                  p ? p->c.max_rows : -1);
    return distq_forward_act(p, N, obs, mask_bits, DISTQ_GREEDY, 1.f, 0u, 0u, actions, nullptr, q_out, (hipStream_t)stream);
}

int rl4rs_distq_loss_grad(rl4rs_distq* p, const float* target_params_dev, int32_t N, const float* obs, const int32_t* actions,
                          const float* rewards, const int32_t* dones, const float* next_obs, const uint32_t* next_mask_bits,
                          const float* weights, float gamma_n, int32_t double_q, float* grad_dev, float* td_dev, int32_t* next_action_dev,
                          float* stats_dev, void* stream) {
    RL4RS_REQUIRE(p && target_params_dev && obs && actions && rewards && dones && next_obs && grad_dev && td_dev && N > 0 &&
                  N <= p->c.max_rows, "distq_loss_grad: bad argument (N=%d, max_rows=%d)", N, p ? p->c.max_rows : -1);
    hipStream_t st = (hipStream_t)stream;
    const DistqDims& d = p->d;
    int rc;
    if (!p->wbar_valid) {
        if ((rc = distq_wbar(p, p->opt.params, p->wbar, st))) return rc;
        p->wbar_valid = true;
    }
    if ((rc = distq_wbar(p, target_params_dev, p->twbar, st))) return rc;
    // forwards: the online net on s, the target net on s', and a* from the online net on s' (double_q) or from the target's
    if ((rc = distq_hidden(p, p->opt.params, N, obs, p->H1, p->H2, p->Ha, p->Hv, st))) return rc;
    if ((rc = distq_hidden(p, target_params_dev, N, next_obs, p->tH1, p->tH2, p->tHa, p->tHv, st))) return rc;
    if (double_q) {
        if ((rc = distq_hidden(p, p->opt.params, N, next_obs, p->nH1, p->nH2, p->nHa, p->nHv, st))) return rc;
        if ((rc = distq_head(p, p->opt.params, p->wbar, N, p->nHa, p->nHv, next_mask_bits, DISTQ_GREEDY, 1.f, 0u, 0u, p->astar, nullptr, nullptr, st)))
            return rc;
    } else {
        if ((rc = distq_head(p, target_params_dev, p->twbar, N, p->tHa, p->tHv, next_mask_bits, DISTQ_GREEDY, 1.f, 0u, 0u, p->astar, nullptr,
                             nullptr, st)))
            return rc;
    }
    const DistqPtrs<const float> q = distq_ptrs<const float>(p->opt.params, d);
    const DistqPtrs<const float> tq = distq_ptrs<const float>(target_params_dev, d);
    DistqRows a;
    memset(&a, 0, sizeof(a));
    a.d = d; a.N = N; a.AP = p->AP; a.gamma_n = gamma_n; a.vmax = p->c.v_max;
    a.Wa2 = q.Wa2; a.ba2 = q.ba2; a.Wv2 = q.Wv2; a.bv2 = q.bv2; a.wbar = p->wbar;
    a.tWa2 = tq.Wa2; a.tba2 = tq.ba2; a.tWv2 = tq.Wv2; a.tbv2 = tq.bv2; a.twbar = p->twbar;
    a.Ha = p->Ha; a.Hv = p->Hv; a.tHa = p->tHa; a.tHv = p->tHv;
    a.act = actions; a.rew = rewards; a.done = dones; a.w = weights; a.next_mask = next_mask_bits; a.astar_in = p->astar;
    a.G = p->G; a.dHa = p->dHa; a.dHv = p->dHv; a.td = td_dev; a.astar_out = next_action_dev; a.terms = p->terms;
    hipLaunchKernelGGL(k_distq_rows, dim3((N + 3) / 4), dim3(256), 0, st, a);
    RL4RS_LAUNCH_CHECK();
    // parameter gradients: "A^T B" reductions over fixed chunks of the sample axis, summed in chunk order
    int chunk = 256;
    if ((N + chunk - 1) / chunk > p->chunk_cap) chunk = ((N + p->chunk_cap - 1) / p->chunk_cap + 63) / 64 * 64;
    const int nz = (N + chunk - 1) / chunk;
    auto tn = [&](const float* A_, int lda, int Mr, const float* B_, int ldb, int Nc, float* dW, float* db) {
        const int tiles = ((Mr + 31) / 32) * ((Nc + 31) / 32);
        hipLaunchKernelGGL(k_gemm_tn, dim3((tiles + 3) / 4, nz), dim3(256), 0, st, A_, lda, Mr, B_, ldb, Nc, N, chunk, nz == 1 ? dW : p->part,
                           db ? (nz == 1 ? db : p->part_b) : (float*)nullptr);
        if (nz > 1) {
            hipLaunchKernelGGL(k_reduce_chunks, dim3((Mr * Nc + 255) / 256), dim3(256), 0, st, p->part, Mr * Nc, nz, dW);
            if (db) hipLaunchKernelGGL(k_reduce_chunks, dim3((Nc + 255) / 256), dim3(256), 0, st, p->part_b, Nc, nz, db);
        }
    };
    const DistqPtrs<float> g = distq_ptrs<float>(grad_dev, d);
    const int nTR = N * d.TR;
    // head: S = h_a^T g and its column sums (dueling), dWv2 = h_v^T g, dWa2 / dba2 column by column
    if (d.dueling) {
        tn(p->Ha, d.SH, d.SH, p->G, d.AT, d.AT, p->S, p->sg);
        tn(p->Hv, d.SH, d.SH, p->G, d.AT, d.AT, g.Wv2, g.bv2);
    }
    hipLaunchKernelGGL(k_distq_wa2_grad, dim3((d.A * d.AT + 3) / 4), dim3(256), 0, st, N, d.SH, d.A, d.AT, actions, p->G, p->Ha,
                       d.dueling ? p->S : (const float*)nullptr, p->sg, -1.f / (float)d.A, g.Wa2, g.ba2);
    // streams -> trunk
    tn(p->H2, d.TR, d.TR, p->dHa, d.SH, d.SH, g.Wa1, g.ba1);
    if ((rc = launch_gemm_nt(p->dHa, d.SH, q.Wa1, d.SH, p->T1, d.TR, N, d.TR, d.SH, st))) return rc;
    if (d.dueling) {
        tn(p->H2, d.TR, d.TR, p->dHv, d.SH, d.SH, g.Wv1, g.bv1);
        if ((rc = launch_gemm_nt(p->dHv, d.SH, q.Wv1, d.SH, p->T2, d.TR, N, d.TR, d.SH, st))) return rc;
    }
    hipLaunchKernelGGL(k_distq_tanh_grad, dim3((nTR + 255) / 256), dim3(256), 0, st, nTR, p->T1, d.dueling ? p->T2 : (const float*)nullptr,
                       p->H2, p->dH2);
    tn(p->H1, d.TR, d.TR, p->dH2, d.TR, d.TR, g.W2, g.b2);
    if ((rc = launch_gemm_nt(p->dH2, d.TR, q.W2, d.TR, p->T1, d.TR, N, d.TR, d.TR, st))) return rc;
    hipLaunchKernelGGL(k_distq_tanh_grad, dim3((nTR + 255) / 256), dim3(256), 0, st, nTR, p->T1, (const float*)nullptr, p->H1, p->dH1);
    tn(obs, d.OD, d.OD, p->dH1, d.TR, d.TR, g.W1, g.b1);
    RL4RS_LAUNCH_CHECK();
    if (stats_dev) {
        hipLaunchKernelGGL(k_reduce_terms, dim3(1), dim3(256), 0, st, p->terms, N, stats_dev);
        RL4RS_LAUNCH_CHECK();
    }
    return RL4RS_OK;
}

int rl4rs_distq_adam_step_clip_by_var(rl4rs_distq* p, const float* grad_dev, float lr, float beta1, float beta2, float eps, float var_clip,
                                      void* stream) {
    RL4RS_REQUIRE(p && grad_dev, "distq_adam_step_clip_by_var: null argument");
    hipStream_t st = (hipStream_t)stream;
    const float lr_t = adam_advance(p->opt, ADAM_TF, lr, beta1, beta2, eps).lr_t;
    // k_sumsq_vars / k_adam_vars take four variables: the 8 (12) of this layout go through them four at a time
    for (int v0 = 0; v0 < p->nseg; v0 += 4) {
        const int64_t base = v0 == 0 ? 0 : p->seg_end[v0 - 1];
        const int count = (int)(p->seg_end[v0 + 3] - base);
        VarSegs sg;
        for (int i = 0; i < 4; ++i) sg.end[i] = (int)(p->seg_end[v0 + i] - base);
        if (var_clip > 0.f) hipLaunchKernelGGL(k_sumsq_vars, dim3(4), dim3(256), 0, st, grad_dev + base, sg, p->sumsq + v0);
        hipLaunchKernelGGL(k_adam_vars, dim3((count + 255) / 256), dim3(256), 0, st, p->opt.params + base, grad_dev + base, p->opt.m + base,
                           p->opt.v + base, count, sg, lr_t, beta1, beta2, eps, p->sumsq + v0, var_clip);
    }
    RL4RS_LAUNCH_CHECK();
    p->wbar_valid = false;
    return RL4RS_OK;
}

int rl4rs_replay_sample_nstep(rl4rs_replay* h, int32_t M, int32_t n_step, double gamma, int32_t prioritized, double beta, uint32_t seed,
                              uint32_t step, float* obs_out, float* next_obs_out, uint32_t* next_mask_out, int32_t* action_out,
                              float* reward_out, int32_t* done_out, int32_t* idx_out, float* weight_out, float* u_out, void* stream) {
    RL4RS_REQUIRE(n_step >= 1, "replay_sample_nstep: n_step must be at least 1 (got %d)", n_step);
    int rc = rl4rs_replay_sample(h, M, prioritized, beta, seed, step, obs_out, next_obs_out, next_mask_out, action_out, reward_out, done_out,
                                 idx_out, weight_out, u_out, stream);
    if (rc || n_step == 1) return rc;
    ReplayNstep a;
    a.M = M; a.B = h->B; a.T = h->T; a.rows_per = h->rows_per; a.OD = h->OD; a.W = h->W; a.n_step = n_step;
    a.vec4 = (h->OD % 4 == 0 && (reinterpret_cast<uintptr_t>(next_obs_out) & 15) == 0) ? 1 : 0;
    a.gamma = gamma;
    a.obs = h->obs; a.mask = h->mask; a.rew = h->rew; a.idx = idx_out;
    a.next_obs_out = next_obs_out; a.next_mask_out = next_mask_out; a.rew_out = reward_out; a.done_out = done_out;
    hipLaunchKernelGGL(k_replay_nstep, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, a);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

}  // extern "C"
