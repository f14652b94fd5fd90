// DQN on the trainable raw-state policy (include/rl4rs_hip.h, "On-device raw-state DQN"): the packed raw-state record that lets
// the replay ring of dqn.hpp hold raw observations, the (double-)Q Huber loss of rl4rs_policy_dqn_loss_grad on the rl4rs_rawtrain
// handle, the masked greedy action, and an Adam step that clips each of the ten variables by its own norm.  Included by
// policy.hip after rawtrain.hpp (the handle, rawtrain_layers, rawtrain_backward_from_ctx, RecLayout) and dqn.hpp
// (masked_first_max, dqn_row_finish, k_dqn_w2_grad, k_greedy_rows).
//
// Reference: script/modelfree_train.py:55-56,63-66,106-133 (algo "DQN_rawstate": RLlib DQN with hiddens [], dueling False on
// mask_model_rawstate = rllib_mask_model.py:67-115 over rllib_rawstate_model.py:25-86).  As for DQN, the Q values are the masked
// logits of the net; RLlib 1.5.1 is absent, parity unpinned, checked against a float64 restatement (tests/rawdqn_ref.py).
#pragma once

namespace rl4rs {

struct SeqPtrs { const uint32_t* p[4]; };         // the handle admits seq_num <= 4

// [dense | cat | seq_0 .. seq_{S-1} | 0 pad] of every row, word by word: nothing is converted, an id keeps its int32 bit pattern
__global__ void k_rawstate_pack(RecLayout r, int N, const uint32_t* __restrict__ cat, const uint32_t* __restrict__ dense, SeqPtrs seq,
                                uint32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)N * r.REC) return;
    const int row = (int)(i / r.REC), c = (int)(i - (int64_t)row * r.REC);
    uint32_t v = 0u;
    if (c < r.Dn) {
        v = dense[(size_t)row * r.Dn + c];
    } else if (c < r.Dn + r.Cn) {
        v = cat[(size_t)row * r.Cn + (c - r.Dn)];
    } else if (c < r.Dn + r.Cn + r.S * r.L) {
        const int k = c - r.Dn - r.Cn, s = k / r.L;
        const uint32_t* q = s == 0 ? seq.p[0] : s == 1 ? seq.p[1] : s == 2 ? seq.p[2] : seq.p[3];
        v = q[(size_t)row * r.L + (k - s * r.L)];
    }
    out[i] = v;
}

// the S + 1 mean-poolings of a forward in one launch, ids read from the records (grid.y = field: S sequences, then the categories);
// k_emb_mean's arithmetic in k_emb_mean's order, so a forward from records gives the bits of a forward from the unpacked arrays
__global__ __launch_bounds__(256) void k_rec_emb_mean(const float* __restrict__ rec, RecLayout r, int n, int H, int E, int U,
                                                      const float* __restrict__ seq_table, const float* __restrict__ cat_table,
                                                      float* __restrict__ out, int64_t ld) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + wave, f = blockIdx.y;
    if (row >= n) return;
    const bool is_cat = f == r.S;
    const int len = is_cat ? r.Cn : r.L;
    const int32_t* ids = reinterpret_cast<const int32_t*>(rec + (size_t)row * r.REC) + (is_cat ? r.Dn : r.Dn + r.Cn + f * r.L);
    const float* table = is_cat ? cat_table : seq_table;
    float* dst = out + (size_t)row * ld + (is_cat ? r.S * E + U : f * E);
    const float inv = 1.0f / (float)len;
    for (int k = lane; k < E; k += 64) {
        float s = 0.f;
        for (int j = 0; j < len; ++j) {
            const int id = min(max(ids[j], 0), H - 1);
            s += table[(size_t)id * E + k];
        }
        dst[k] = s * inv;
    }
}

struct RawDqnRows {
    DqnRows r;                                    // d, N, double_q, gamma, next_mask, act, rew, done, w, Qn / ldq, g, td, astar, terms
    const float* hw; const float* hb;             // online head [256, AE], [AE]
    const float* thw; const float* thb;           // target head
    const float* ctx; const float* ctx_t;         // context rows of s (online) and of s' (target)
    float* d_ctx;
};

// One wave per row, after k_dqn_rows: a* from the Q(s') rows of the selecting net, the two single-column products over the 256-wide
// context, the row's outputs (dqn_row_finish), and d loss / d (pre-activation of the context layer) = g * head_w[:, a] * ELU'(ctx).
// Nothing of a terminal row's successor is read.
__global__ __launch_bounds__(256) void k_rawdqn_rows(RawDqnRows a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + wave;
    if (n >= a.r.N) return;
    const PolDims& d = a.r.d;
    const int act = max(0, min(a.r.act[n], d.A - 1));
    const bool done = a.r.done[n] != 0;
    int astar = -1;
    float qt = 0.f;
    bool boot = false;
    if (!done) {
        bool legal;
        astar = masked_first_max(a.r.Qn + (size_t)n * a.r.ldq, a.r.next_mask ? a.r.next_mask + (size_t)n * d.W : nullptr, d.A, lane, true, &legal);
        boot = legal;
        if (a.r.double_q) {
            float s = 0.f;
            for (int j = lane; j < 256; j += 64) s = fmaf(a.ctx_t[(size_t)n * 256 + j], a.thw[(size_t)j * d.AE + astar], s);
            qt = wave_sum(s) + a.thb[astar];
        } else {
            qt = a.r.Qn[(size_t)n * a.r.ldq + astar];
        }
    }
    float s = 0.f;
    for (int j = lane; j < 256; j += 64) s = fmaf(a.ctx[(size_t)n * 256 + j], a.hw[(size_t)j * d.AE + act], s);
    const float qsa = wave_sum(s) + a.hb[act];
    const float g = dqn_row_finish(a.r, n, lane, qsa, qt, boot, astar);
    for (int j = lane; j < 256; j += 64) {
        const float c = a.ctx[(size_t)n * 256 + j];
        a.d_ctx[(size_t)n * 256 + j] = g * a.hw[(size_t)j * d.AE + act] * (c > 0.f ? 1.f : c + 1.f);
    }
}

// ---- per-variable clip over ten variables of very different sizes ---------------------------------------------------------------
constexpr int VS_TILE = 16384;      // gradient elements per workgroup of the first stage: 256 threads x 64
struct VarEnds10 { int64_t end[RT_COUNT]; };

// Stage 1: part[tile][v] = sum of squares of the elements of variable v inside the tile, for every variable the tile meets (a tile
// may hold the end of one variable, several whole small ones and the start of the next).  Thread t takes the elements lo + t,
// lo + t + 256, ... of the intersection, the 256 sums meet in an LDS tree: a fixed order.
__global__ __launch_bounds__(256) void k_sumsq_tiles(const float* __restrict__ g, int64_t count, VarEnds10 ve, float* __restrict__ part) {
    __shared__ float sm[256];
    const int64_t t_lo = (int64_t)blockIdx.x * VS_TILE, t_hi = min(t_lo + VS_TILE, count);
    for (int v = 0; v < RT_COUNT; ++v) {
        const int64_t lo = max(t_lo, v == 0 ? (int64_t)0 : ve.end[v - 1]), hi = min(t_hi, ve.end[v]);
        if (lo >= hi) continue;                                   // block-uniform
        float s = 0.f;
        for (int64_t i = lo + threadIdx.x; i < hi; i += 256) s += g[i] * g[i];
        sm[threadIdx.x] = s;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) part[(size_t)blockIdx.x * RT_COUNT + v] = sm[0];
        __syncthreads();
    }
}
// Stage 2: one wave per variable adds its tiles' partial sums in tile order (64 loaded at a time, added one after the other).
__global__ __launch_bounds__(64) void k_sumsq_tiles_finish(const float* __restrict__ part, VarEnds10 ve, float* __restrict__ out) {
    const int v = blockIdx.x, lane = threadIdx.x;
    const int64_t lo = v == 0 ? (int64_t)0 : ve.end[v - 1], hi = ve.end[v];
    float s = 0.f;
    if (hi > lo) {
        const int first = (int)(lo / VS_TILE), last = (int)((hi - 1) / VS_TILE);
        for (int t0 = first; t0 <= last; t0 += 64) {
            const float x = (t0 + lane <= last) ? part[(size_t)(t0 + lane) * RT_COUNT + v] : 0.f;
            const int cnt = min(64, last - t0 + 1);
            for (int k = 0; k < cnt; ++k) s += __shfl(x, k);
        }
    }
    if (lane == 0) out[v] = s;
}
// k_adam_vars for ten variables and 64-bit offsets
__global__ void k_adam_vars10(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int64_t count,
                              VarEnds10 ve, float lr_t, float b1, float b2, float eps, const float* __restrict__ sumsq, float clip) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    float gi = g[i];
    if (clip > 0.f) {
        int var = 0;
#pragma unroll
        for (int k = 0; k < RT_COUNT - 1; ++k) var += (i >= ve.end[k]) ? 1 : 0;
        const float norm = sqrtf(sumsq[var]);
        if (norm > clip) gi *= clip / norm;
    }
    p[i] = adam_elem(p[i], m, v, i, gi, lr_t, b1, b2, eps);
}

}  // namespace rl4rs

namespace {

int rawdqn_scratch(rl4rs_rawtrain* p) {
    if (p->dq_g) return RL4RS_OK;
    int rc;
    auto alloc = [&](float** dst, size_t n) {
        int r = dev_alloc(dst, n);
        if (r == RL4RS_OK) p->owned.push_back(*dst);
        return r;
    };
    const size_t B = (size_t)p->c.max_rows;
    if ((rc = alloc(&p->dq_feat, B * p->F))) return rc;
    if ((rc = alloc(&p->dq_h1, B * p->c.hidden_units))) return rc;
    if ((rc = alloc(&p->dq_ctx_t, B * 256))) return rc;
    if ((rc = alloc(&p->dq_ctx_n, B * 256))) return rc;
    if ((rc = alloc(&p->dq_g, B))) return rc;
    return RL4RS_OK;
}

inline void rawdqn_mark(rl4rs_rawtrain* p, int i, hipStream_t st) {
    if (p->prof) (void)hipEventRecord(p->prof_ev[i], st);
}

// forward on the parameters at P from records read in place: one pooling launch, then the GEMMs (dense operand lda = REC)
int rawdqn_forward(rl4rs_rawtrain* p, const float* P, int N, const float* rec, float* feat, float* h1, float* ctx, float* ext, int n_out,
                   hipStream_t st) {
    const RecLayout r = rec_layout(p->c);
    hipLaunchKernelGGL(k_rec_emb_mean, dim3((N + 3) / 4, r.S + 1), dim3(256), 0, st, rec, r, N, p->c.category_hash_size, p->c.emb_size,
                       p->c.hidden_units, P + p->off[RT_SEQ_EMB], P + p->off[RT_CAT_EMB], feat, (int64_t)p->F);
    RL4RS_LAUNCH_CHECK();
    return rawtrain_layers(p, P, N, rec, r.REC, feat, h1, ctx, ext, n_out, st);
}

}  // namespace

extern "C" {

int32_t rl4rs_rawstate_record_words(const rl4rs_rawpolicy_cfg* c) {
    if (!c || c->dense_feature_num <= 0 || c->category_feature_num < 1 || c->seq_num < 1 || c->seq_num > 4 || c->maxlen < 1) return 0;
    return rec_layout(*c).REC;
}

int rl4rs_rawstate_pack(const rl4rs_rawpolicy_cfg* c, int32_t N, const int32_t* cat, const float* dense, const int32_t* const* seq,
                        float* rec_out, void* stream) {
    RL4RS_REQUIRE(c && cat && dense && seq && rec_out && N > 0, "rawstate_pack: bad argument");
    RL4RS_REQUIRE(c->dense_feature_num > 0 && c->category_feature_num >= 1 && c->seq_num >= 1 && c->seq_num <= 4 && c->maxlen >= 1,
                  "rawstate_pack: bad sizes");
    const RecLayout r = rec_layout(*c);
    SeqPtrs sp;
    for (int s = 0; s < 4; ++s) sp.p[s] = reinterpret_cast<const uint32_t*>(s < r.S ? seq[s] : nullptr);
    for (int s = 0; s < r.S; ++s) RL4RS_REQUIRE(seq[s], "rawstate_pack: sequence %d is null", s);
    const int64_t total = (int64_t)N * r.REC;
    hipLaunchKernelGGL(k_rawstate_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, r, N,
                       reinterpret_cast<const uint32_t*>(cat), reinterpret_cast<const uint32_t*>(dense), sp, reinterpret_cast<uint32_t*>(rec_out));
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

int rl4rs_rawtrain_dqn_loss_grad(rl4rs_rawtrain* p, const float* target_params_dev, int32_t N, const float* rec, const int32_t* actions,
                                 const float* rewards, const int32_t* dones, const float* next_rec, const uint32_t* next_mask_bits,
                                 const float* weights, float gamma, int32_t double_q, float* td_dev, int32_t* next_action_dev,
                                 float* stats_dev, void* stream) {
    RL4RS_REQUIRE(p && target_params_dev && rec && actions && rewards && dones && next_rec && td_dev && N > 0 && N <= p->c.max_rows,
                  "rawtrain_dqn_loss_grad: bad argument (N=%d, max_rows=%d)", N, p ? p->c.max_rows : -1);
    hipStream_t st = (hipStream_t)stream;
    int rc = rawdqn_scratch(p);
    if (rc) return rc;
    const PolDims& d = p->d;
    const float* P = p->opt.params;
    const float* TP = target_params_dev;
    float* G = p->opt.grad;
    const int64_t* o = p->off;
    rawdqn_mark(p, 0, st);
    // s through the online net keeps feat / h1 / ctx for the backward (no head GEMM: the row kernel takes the one column it needs);
    // s' through the target net keeps its context rows, and through the selecting net the A unmasked Q columns (p->ext)
    if ((rc = rawdqn_forward(p, P, N, rec, p->feat, p->h1, p->ctx, nullptr, 0, st))) return rc;
    if ((rc = rawdqn_forward(p, TP, N, next_rec, p->dq_feat, p->dq_h1, p->dq_ctx_t, double_q ? nullptr : p->ext, d.A, st))) return rc;
    if (double_q && (rc = rawdqn_forward(p, P, N, next_rec, p->dq_feat, p->dq_h1, p->dq_ctx_n, p->ext, d.A, st))) return rc;
    rawdqn_mark(p, 1, st);
    RawDqnRows a;
    memset(&a, 0, sizeof(a));
    a.r.d = d; a.r.N = N; a.r.double_q = double_q ? 1 : 0; a.r.gamma = gamma;
    a.r.next_mask = next_mask_bits; a.r.act = actions; a.r.rew = rewards; a.r.done = dones; a.r.w = weights;
    a.r.Qn = p->ext; a.r.ldq = d.AE;
    a.r.g = p->dq_g; a.r.td = td_dev; a.r.astar = next_action_dev; a.r.terms = p->terms;
    a.hw = P + o[RT_HEAD_W]; a.hb = P + o[RT_HEAD_B]; a.thw = TP + o[RT_HEAD_W]; a.thb = TP + o[RT_HEAD_B];
    a.ctx = p->ctx; a.ctx_t = p->dq_ctx_t; a.d_ctx = p->d_ctx;
    hipLaunchKernelGGL(k_rawdqn_rows, dim3((N + 3) / 4), dim3(256), 0, st, a);
    rawdqn_mark(p, 2, st);
    hipLaunchKernelGGL(k_dqn_w2_grad, dim3((d.AE + 3) / 4), dim3(256), 0, st, N, 256, d.A, d.AE, actions, p->dq_g, p->ctx, G + o[RT_HEAD_W],
                       G + o[RT_HEAD_B]);
    RL4RS_LAUNCH_CHECK();
    if ((rc = rawtrain_backward_from_ctx(p, N, rec, rec_layout(p->c).REC, nullptr, nullptr, rec, st))) return rc;
    if (stats_dev) hipLaunchKernelGGL(k_reduce_terms, dim3(1), dim3(256), 0, st, p->terms, N, stats_dev);
    rawdqn_mark(p, 3, st);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

int rl4rs_rawtrain_greedy(rl4rs_rawtrain* p, int32_t N, const int32_t* cat, const float* dense, const int32_t* const* seq,
                          const uint32_t* mask_bits, int32_t* actions, float* q_dev, void* stream) {
    RL4RS_REQUIRE(p && cat && dense && seq && actions && N > 0 && N <= p->c.max_rows, "rawtrain_greedy: bad argument (N=%d, max_rows=%d)", N,
                  p ? p->c.max_rows : -1);
    hipStream_t st = (hipStream_t)stream;
    int rc = rawtrain_forward(p, N, cat, dense, seq, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_greedy_rows, dim3((N + 3) / 4), dim3(256), 0, st, N, p->d.A, p->d.W, p->ext, p->d.AE, mask_bits, actions, q_dev);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

int rl4rs_rawtrain_adam_step_clip_by_var(rl4rs_rawtrain* p, float lr, float beta1, float beta2, float eps, float var_clip, void* stream) {
    RL4RS_REQUIRE(p, "rawtrain_adam_step_clip_by_var: null handle");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = p->opt.n;
    const int tiles = (int)((n + VS_TILE - 1) / VS_TILE);
    VarEnds10 ve;
    for (int i = 0; i < RT_COUNT; ++i) ve.end[i] = i + 1 < RT_COUNT ? p->off[i + 1] : n;
    rawdqn_mark(p, 4, st);
    if (var_clip > 0.f) {
        if (!p->vs_part) {
            int rc;
            if ((rc = dev_alloc(&p->vs_part, (size_t)tiles * RT_COUNT))) return rc;
            p->owned.push_back(p->vs_part);
            if ((rc = dev_alloc(&p->vs_sumsq, (size_t)RT_COUNT))) return rc;
            p->owned.push_back(p->vs_sumsq);
        }
        hipLaunchKernelGGL(k_sumsq_tiles, dim3(tiles), dim3(256), 0, st, p->opt.grad, n, ve, p->vs_part);
        hipLaunchKernelGGL(k_sumsq_tiles_finish, dim3(RT_COUNT), dim3(64), 0, st, p->vs_part, ve, p->vs_sumsq);
    }
    rawdqn_mark(p, 5, st);
    const float lr_t = adam_advance(p->opt, ADAM_TF, lr, beta1, beta2, eps).lr_t;
    hipLaunchKernelGGL(k_adam_vars10, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p->opt.params, p->opt.grad, p->opt.m, p->opt.v, n, ve,
                       lr_t, beta1, beta2, eps, p->vs_sumsq, var_clip);
    rawdqn_mark(p, 6, st);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

int rl4rs_rawtrain_set_profiling(rl4rs_rawtrain* p, int32_t on) {
    RL4RS_REQUIRE(p, "rawtrain_set_profiling: null handle");
    if (on)
        for (hipEvent_t& e : p->prof_ev)
            if (!e) RL4RS_HIP_TRY(hipEventCreate(&e));
    p->prof = on != 0;
    return RL4RS_OK;
}

int rl4rs_rawtrain_profile(rl4rs_rawtrain* p, float* ms_out) {
    RL4RS_REQUIRE(p && ms_out && p->prof, "rawtrain_profile: profiling is off (rl4rs_rawtrain_set_profiling)");
    RL4RS_HIP_TRY(hipEventSynchronize(p->prof_ev[3]));
    RL4RS_HIP_TRY(hipEventSynchronize(p->prof_ev[6]));
    const int from[5] = {0, 1, 2, 4, 5};
    for (int i = 0; i < 5; ++i) RL4RS_HIP_TRY(hipEventElapsedTime(&ms_out[i], p->prof_ev[from[i]], p->prof_ev[from[i] + 1]));
    return RL4RS_OK;
}

}  // extern "C"
