// Trainable raw-state policy (rl4rs/nets/rllib/rllib_rawstate_model.py:25-86 + mask wrapper rllib_mask_model.py:67-115) with
// RLlib's A2C / PPO losses: the forward of rl4rs_rawpolicy on raw (unpacked) weights, the loss core of the FC mask policy
// (policy_row_loss), and a hand-written backward through the two heads, the 256-wide context layer, the dense tower and the
// mean-pooled embeddings of both tables.  Included at the end of policy.hip after simtrain.hpp (reduction helpers).
// Flat parameter / gradient layout:
//   [ cat_emb | seq_emb | dense_w1 | dense_b1 | dense_w2 | dense_b2 | ctx_w | ctx_b | head_w 256 x (A+1) = [out_w | value_w] |
//     head_b (A+1) ]
#pragma once

#include "rawtrain_scratch.hpp"      // RT_* variable indices, the ten sizes, the sizing of cx.wt / cx.part

namespace rl4rs {

// loss + gradient wrt [logits | value] of one sample per wave, from the head outputs `ext`
__global__ __launch_bounds__(256) void k_rawpolicy_loss(PolDims d, int N, const float* __restrict__ ext, const uint32_t* __restrict__ mask,
                                                        LossArgs L, float* __restrict__ dOut, float4* __restrict__ terms) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* s_out = reinterpret_cast<float*>(smem) + (size_t)wave * 2 * d.AE;
    float* s_d = s_out + d.AE;
    const int n = blockIdx.x * 4 + wave;
    if (n >= N) return;
    const uint32_t* mrow = mask ? mask + (size_t)n * d.W : nullptr;
    float mx = -3.4028235e38f;
    for (int a = lane; a < d.AE; a += 64) {
        float v = ext[(size_t)n * d.AE + a];
        if (a < d.A) {
            bool ok = mrow ? ((mrow[a >> 5] >> (a & 31)) & 1u) : true;
            if (!ok) v = v + (-3.4028235e38f);
            mx = fmaxf(mx, v);
        }
        s_out[a] = v;
    }
    mx = wave_max(mx);
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    float se = 0.f;
    for (int a = lane; a < d.A; a += 64) se += expf(s_out[a] - mx);
    const float2 lse = row_lse(mx, wave_sum(se));
    const float4 tm = policy_row_loss(d, L, s_out, lse, n, lane, s_d, dOut);
    if (lane == 0) terms[n] = tm;
}

}  // namespace rl4rs

struct rl4rs_rawtrain {
    rl4rs_rawpolicy_cfg c;
    PolDims d;
    int F;
    int64_t off[RT_COUNT];
    TrainCtx cx;
    OptBlock opt;
    float* sumsq;
    float *feat, *h1, *ctx, *ext, *dOut, *d_ctx, *d_feat, *d_h1;
    float4* terms;
    // DQN on the raw handle (rawdqn.hpp), allocated by the first call that needs them: activations of the two s' forwards, the
    // per-row d loss / d Q, the per-tile sums of squares of the per-variable clip and its ten norms^2
    float *dq_feat = nullptr, *dq_h1 = nullptr, *dq_ctx_t = nullptr, *dq_ctx_n = nullptr, *dq_g = nullptr;
    float *vs_part = nullptr, *vs_sumsq = nullptr;
    // rl4rs_rawtrain_set_profiling: events at the stage boundaries of the last dqn_loss_grad ([0..3]) and clipped Adam step ([4..6])
    hipEvent_t prof_ev[7] = {};
    bool prof = false;
    std::vector<void*> owned;
};

namespace {

// the four GEMMs of a forward on the parameters at P: dense tower (rows of `dense` ldd floats apart) into feat's middle block,
// context layer, and - ext != null - the first n_out head columns.  The pooled embeddings are in feat already.
int rawtrain_layers(rl4rs_rawtrain* p, const float* P, int N, const float* dense, int64_t ldd, float* feat, float* h1, float* ctx, float* ext,
                    int n_out, hipStream_t st) {
    const int E = p->c.emb_size, U = p->c.hidden_units, S = p->c.seq_num, Dn = p->c.dense_feature_num, F = p->F, AE = p->d.AE;
    const int64_t* o = p->off;
    int rc;
    if ((rc = launch_gemm_f32(dense, ldd, P + o[RT_DW1], U, P + o[RT_DB1], h1, U, N, U, Dn, 1, st))) return rc;
    if ((rc = launch_gemm_f32(h1, U, P + o[RT_DW2], U, P + o[RT_DB2], feat + S * E, F, N, U, U, 1, st))) return rc;
    if ((rc = launch_gemm_f32(feat, F, P + o[RT_CTX_W], 256, P + o[RT_CTX_B], ctx, 256, N, 256, F, 1, st))) return rc;
    if (!ext) return RL4RS_OK;
    return launch_gemm_f32(ctx, 256, P + o[RT_HEAD_W], AE, P + o[RT_HEAD_B], ext, AE, N, n_out, 256, 0, st);
}

int rawtrain_forward(rl4rs_rawtrain* p, int N, const int32_t* cat, const float* dense, const int32_t* const* seq, hipStream_t st) {
    const int E = p->c.emb_size, U = p->c.hidden_units, H = p->c.category_hash_size, S = p->c.seq_num, Dn = p->c.dense_feature_num;
    const int F = p->F, L = p->c.maxlen, Cn = p->c.category_feature_num;
    const float* P = p->opt.params;
    const int64_t* o = p->off;
    const dim3 g4((N + 3) / 4), b256(256);
    for (int s = 0; s < S; ++s)
        hipLaunchKernelGGL(k_emb_mean, g4, b256, 0, st, seq[s], N, L, H, E, P + o[RT_SEQ_EMB], p->feat, (int64_t)F, s * E);
    hipLaunchKernelGGL(k_emb_mean, g4, b256, 0, st, cat, N, Cn, H, E, P + o[RT_CAT_EMB], p->feat, (int64_t)F, S * E + U);
    RL4RS_LAUNCH_CHECK();
    return rawtrain_layers(p, P, N, dense, Dn, p->feat, p->h1, p->ctx, p->ext, p->d.AE, st);
}

// Packed raw-state record (include/rl4rs_hip.h): [ dense Dn | cat Cn | seq_0 L | ... | seq_{S-1} L | zero pad ] 32-bit words
struct RecLayout { int Dn, Cn, L, S, REC; };
inline RecLayout rec_layout(const rl4rs_rawpolicy_cfg& c) {
    const int w = c.dense_feature_num + c.category_feature_num + c.seq_num * c.maxlen;
    return {c.dense_feature_num, c.category_feature_num, c.maxlen, c.seq_num, (w + 3) / 4 * 4};
}

// gradient of the S + 1 mean-poolings of a forward in ONE launch, ids read from the records (grid.y = field: S sequences, then
// the categories); the arithmetic of k_emb_mean_bwd (float atomics)
__global__ __launch_bounds__(256) void k_rec_emb_mean_bwd(const float* __restrict__ rec, RecLayout r, int n, int H, int E, int U,
                                                          const float* __restrict__ d_feat, int64_t ld, float* __restrict__ g_seq,
                                                          float* __restrict__ g_cat) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + wave, f = blockIdx.y;
    if (row >= n) return;
    const bool is_cat = f == r.S;
    const int len = is_cat ? r.Cn : r.L;
    const int32_t* ids = reinterpret_cast<const int32_t*>(rec + (size_t)row * r.REC) + (is_cat ? r.Dn : r.Dn + r.Cn + f * r.L);
    const float* d = d_feat + (size_t)row * ld + (is_cat ? r.S * E + U : f * E);
    float* g_table = is_cat ? g_cat : g_seq;
    const float inv = 1.0f / (float)len;
    for (int j = 0; j < len; ++j) {
        const int id = min(max(ids[j], 0), H - 1);
        for (int k = lane; k < E; k += 64) atomicAdd(&g_table[(size_t)id * E + k], d[k] * inv);
    }
}

// Backward from d_ctx (= d loss / d pre-activation of the context layer, in p->d_ctx) down to the tables, with the activations of
// the last forward in p->feat / h1 / ctx.  The ids come from the unpacked arrays (cat / seq: one scatter launch per field) or -
// rec != null - from the records in one launch; dense rows are ldd floats apart.
int rawtrain_backward_from_ctx(rl4rs_rawtrain* p, int N, const float* dense, int ldd, const int32_t* cat, const int32_t* const* seq,
                               const float* rec, hipStream_t st) {
    const int E = p->c.emb_size, U = p->c.hidden_units, H = p->c.category_hash_size, S = p->c.seq_num, Dn = p->c.dense_feature_num;
    const int F = p->F, L = p->c.maxlen, Cn = p->c.category_feature_num;
    const float* P = p->opt.params;
    float* G = p->opt.grad;
    const int64_t* o = p->off;
    const dim3 g4((N + 3) / 4), b256(256);
    auto ew = [](int n) { return dim3((n + 255) / 256); };
    int rc;
    st_tn(p->cx, st, p->feat, F, F, p->d_ctx, 256, 256, N, G + o[RT_CTX_W]);
    st_cs(p->cx, st, p->d_ctx, 256, 256, N, G + o[RT_CTX_B]);
    if ((rc = st_back(p->cx, st, p->d_ctx, 256, 256, P + o[RT_CTX_W], 256, F, p->d_feat, F, N))) return rc;
    RL4RS_HIP_TRY(hipMemsetAsync(G + o[RT_CAT_EMB], 0, (size_t)H * E * 4, st));
    RL4RS_HIP_TRY(hipMemsetAsync(G + o[RT_SEQ_EMB], 0, (size_t)H * E * 4, st));
    if (rec) {
        hipLaunchKernelGGL(k_rec_emb_mean_bwd, dim3((N + 3) / 4, S + 1), b256, 0, st, rec, rec_layout(p->c), N, H, E, U, p->d_feat, (int64_t)F,
                           G + o[RT_SEQ_EMB], G + o[RT_CAT_EMB]);
    } else {
        for (int s = 0; s < S; ++s)
            hipLaunchKernelGGL(k_emb_mean_bwd, g4, b256, 0, st, seq[s], N, L, H, E, p->d_feat + s * E, (int64_t)F, G + o[RT_SEQ_EMB]);
        hipLaunchKernelGGL(k_emb_mean_bwd, g4, b256, 0, st, cat, N, Cn, H, E, p->d_feat + S * E + U, (int64_t)F, G + o[RT_CAT_EMB]);
    }
    // dense tower (inference-mode Dropout: RLlib calls the keras base model without the training flag)
    float* d_tower = p->d_feat + S * E;
    hipLaunchKernelGGL(k_elu_bwd, ew(N * U), b256, 0, st, d_tower, (int64_t)F, p->feat + S * E, (int64_t)F, (const uint8_t*)nullptr, 0.f, N * U, U);
    st_tn(p->cx, st, p->h1, U, U, d_tower, F, U, N, G + o[RT_DW2]);
    st_cs(p->cx, st, d_tower, F, U, N, G + o[RT_DB2]);
    if ((rc = st_back(p->cx, st, d_tower, F, U, P + o[RT_DW2], U, U, p->d_h1, U, N))) return rc;
    hipLaunchKernelGGL(k_elu_bwd, ew(N * U), b256, 0, st, p->d_h1, (int64_t)U, p->h1, (int64_t)U, (const uint8_t*)nullptr, 0.f, N * U, U);
    st_tn(p->cx, st, dense, ldd, Dn, p->d_h1, U, U, N, G + o[RT_DW1]);
    st_cs(p->cx, st, p->d_h1, U, U, N, G + o[RT_DB1]);
    return RL4RS_OK;
}

}  // namespace

extern "C" {

int rl4rs_rawtrain_destroy(rl4rs_rawtrain* p) {
    if (!p) return RL4RS_OK;
    for (void* q : p->owned) (void)hipFree(q);
    for (hipEvent_t e : p->prof_ev)
        if (e) (void)hipEventDestroy(e);
    delete p;
    return RL4RS_OK;
}

int rl4rs_rawtrain_create(const rl4rs_rawpolicy_cfg* c, const rl4rs_rawpolicy_weights* w, void* stream, rl4rs_rawtrain** out) {
    RL4RS_REQUIRE(c && w && out, "rawtrain_create: null argument");
    RL4RS_REQUIRE(c->emb_size > 0 && c->hidden_units > 0 && c->maxlen >= 1 && c->seq_num >= 1 && c->seq_num <= 4 &&
                  c->category_feature_num >= 1 && c->category_hash_size > 0 && c->dense_feature_num > 0 && c->action_size > 1 &&
                  c->max_rows > 0, "rawtrain_create: bad sizes");
    RL4RS_REQUIRE(w->cat_emb && w->seq_emb && w->dense_w1 && w->dense_b1 && w->dense_w2 && w->dense_b2 && w->ctx_w && w->ctx_b &&
                  w->out_w && w->out_b && w->value_w && w->value_b, "rawtrain_create: weights missing");
    if (rl4rs_device_count() <= 0) {
        set_error("no HIP device visible: librl4rs_hip has no CPU fallback");
        return RL4RS_EHIP;
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t E = c->emb_size, U = c->hidden_units, H = c->category_hash_size, S = c->seq_num, Dn = c->dense_feature_num;
    const int64_t A = c->action_size, AE = A + 1;
    rl4rs_rawtrain* p = new rl4rs_rawtrain();
    p->c = *c;
    p->d.OD = 256; p->d.HID = 0; p->d.A = (int)A; p->d.AE = (int)AE; p->d.W = (int)((A + 31) / 32);
    p->F = (int)(S * E + U + E);
    p->opt.t = 0;
    const RawTrainScratch sc = rawtrain_scratch(RawTrainDims{E, U, H, S, Dn, c->category_feature_num, c->maxlen, A, c->max_rows});
    const int64_t* sizes = sc.sizes;
    int64_t o = 0;
    for (int i = 0; i < RT_COUNT; ++i) { p->off[i] = o; o += sizes[i]; }
    p->opt.n = o;
    int rc;
    auto al = [&](float** dst, size_t n) {
        int r = dev_alloc(dst, n);
        if (r == RL4RS_OK) p->owned.push_back(*dst);
        return r;
    };
#define RT_FAIL(expr) do { if ((rc = (expr)) != RL4RS_OK) { rl4rs_rawtrain_destroy(p); return rc; } } while (0)
#define RT_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { set_error("%s failed: %s", #expr, hipGetErrorString(e_)); \
        rl4rs_rawtrain_destroy(p); return RL4RS_EHIP; } } while (0)
    RT_FAIL(al(&p->opt.params, p->opt.n)); RT_FAIL(al(&p->opt.grad, p->opt.n)); RT_FAIL(al(&p->opt.m, p->opt.n));
    RT_FAIL(al(&p->opt.v, p->opt.n)); RT_FAIL(al(&p->sumsq, 4));
    const float* src[8] = {w->cat_emb, w->seq_emb, w->dense_w1, w->dense_b1, w->dense_w2, w->dense_b2, w->ctx_w, w->ctx_b};
    for (int i = 0; i < 8; ++i) RT_HIP(hipMemcpyAsync(p->opt.params + p->off[i], src[i], (size_t)sizes[i] * 4, hipMemcpyHostToDevice, st));
    std::vector<float> hw((size_t)256 * AE), hb(AE);       // [out_w | value_w], [out_b | value_b]
    for (int k = 0; k < 256; ++k) {
        for (int a = 0; a < A; ++a) hw[(size_t)k * AE + a] = w->out_w[(size_t)k * A + a];
        hw[(size_t)k * AE + A] = w->value_w[k];
    }
    for (int a = 0; a < A; ++a) hb[a] = w->out_b[a];
    hb[A] = w->value_b[0];
    RT_HIP(hipMemcpyAsync(p->opt.params + p->off[RT_HEAD_W], hw.data(), hw.size() * 4, hipMemcpyHostToDevice, st));
    RT_HIP(hipMemcpyAsync(p->opt.params + p->off[RT_HEAD_B], hb.data(), hb.size() * 4, hipMemcpyHostToDevice, st));
    RT_HIP(hipMemsetAsync(p->opt.m, 0, (size_t)p->opt.n * 4, st));
    RT_HIP(hipMemsetAsync(p->opt.v, 0, (size_t)p->opt.n * 4, st));
    const size_t B = c->max_rows;
    RT_FAIL(al(&p->feat, B * p->F)); RT_FAIL(al(&p->h1, B * U)); RT_FAIL(al(&p->ctx, B * 256)); RT_FAIL(al(&p->ext, B * AE));
    RT_FAIL(al(&p->dOut, B * AE)); RT_FAIL(al(&p->d_ctx, B * 256)); RT_FAIL(al(&p->d_feat, B * p->F)); RT_FAIL(al(&p->d_h1, B * U));
    { float* t4; RT_FAIL(al(&t4, B * 4)); p->terms = reinterpret_cast<float4*>(t4); }
    // the widest of the four weights, dense_w2 [U, U] included: every chunked gradient and every transposed st_back of a call of
    // up to max_rows rows fits (rawtrain_scratch.hpp)
    p->cx.chunk = RAWTRAIN_CHUNK;
    RT_FAIL(al(&p->cx.wt, (size_t)sc.wt_floats));
    RT_FAIL(al(&p->cx.part, (size_t)sc.part_floats));
    RT_HIP(hipStreamSynchronize(st));
#undef RT_HIP
#undef RT_FAIL
    *out = p;
    return RL4RS_OK;
}

int rl4rs_rawtrain_params(rl4rs_rawtrain* p, float** params_dev, float** grad_dev, int64_t* count) {
    return opt_params(RL4RS_OPT(p), params_dev, grad_dev, count, "rawtrain_params");
}

int rl4rs_rawtrain_act(rl4rs_rawtrain* p, int32_t N, const int32_t* cat, const float* dense, const int32_t* const* seq,
                       const uint32_t* mask_bits, uint32_t seed, uint32_t step, int32_t* actions, float* logp, float* value,
                       float* entropy, float* logits, void* stream) {
    RL4RS_REQUIRE(p && cat && dense && seq && actions && N > 0 && N <= p->c.max_rows, "rawtrain_act: bad argument (N=%d, max_rows=%d)", N,
                  p ? p->c.max_rows : -1);
    hipStream_t st = (hipStream_t)stream;
    int rc = rawtrain_forward(p, N, cat, dense, seq, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_rawpolicy_head<true>, dim3((N + 3) / 4), dim3(256), (size_t)4 * p->d.AE * 4, st, p->d, N, p->ext, (int64_t)p->d.AE,
                       mask_bits, seed, step, actions, logp, value, entropy, logits);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

int rl4rs_rawtrain_evaluate(rl4rs_rawtrain* p, int32_t N, const int32_t* cat, const float* dense, const int32_t* const* seq,
                            const uint32_t* mask_bits, const int32_t* actions, float* logp, float* value, float* entropy, float* logits,
                            void* stream) {
    RL4RS_REQUIRE(p && cat && dense && seq && actions && N > 0 && N <= p->c.max_rows, "rawtrain_evaluate: bad argument (N=%d, max_rows=%d)",
                  N, p ? p->c.max_rows : -1);
    hipStream_t st = (hipStream_t)stream;
    int rc = rawtrain_forward(p, N, cat, dense, seq, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_rawpolicy_head<false>, dim3((N + 3) / 4), dim3(256), (size_t)4 * p->d.AE * 4, st, p->d, N, p->ext, (int64_t)p->d.AE,
                       mask_bits, 0u, 0u, const_cast<int32_t*>(actions), logp, value, entropy, logits);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

// A2C (algo 0) / PPO (algo 1) loss and its gradient into the handle's flat gradient buffer (arguments as rl4rs_policy_loss_grad)
int rl4rs_rawtrain_loss_grad(rl4rs_rawtrain* p, int32_t algo, int32_t N, const int32_t* cat, const float* dense,
                             const int32_t* const* seq, const uint32_t* mask_bits, const int32_t* actions, const float* adv,
                             const float* ret, const float* old_logp, const float* old_value, const float* old_logits, float vf_coeff,
                             float ent_coeff, float clip, float vf_clip, float kl_coeff, float* stats_dev, void* stream) {
    RL4RS_REQUIRE(p && cat && dense && seq && actions && adv && ret && N > 0 && N <= p->c.max_rows,
                  "rawtrain_loss_grad: bad argument (N=%d, max_rows=%d)", N, p ? p->c.max_rows : -1);
    RL4RS_REQUIRE(algo == 0 || (algo == 1 && old_logp && old_value && old_logits), "rawtrain_loss_grad: PPO needs old_* inputs");
    hipStream_t st = (hipStream_t)stream;
    const int Dn = p->c.dense_feature_num, AE = p->d.AE;
    const float* P = p->opt.params;
    float* G = p->opt.grad;
    const int64_t* o = p->off;
    int rc = rawtrain_forward(p, N, cat, dense, seq, st);
    if (rc) return rc;
    LossArgs La;
    La.algo = algo; La.vf_coeff = vf_coeff; La.ent_coeff = ent_coeff; La.clip = clip; La.vf_clip = vf_clip; La.kl_coeff = kl_coeff;
    La.scale = algo == 0 ? 1.0f : 1.0f / (float)N;
    La.actions = actions; La.adv = adv; La.ret = ret; La.old_logp = old_logp; La.old_value = old_value; La.old_logits = old_logits;
    hipLaunchKernelGGL(k_rawpolicy_loss, dim3((N + 3) / 4), dim3(256), (size_t)4 * 2 * AE * 4, st, p->d, N, p->ext, mask_bits, La, p->dOut,
                       p->terms);
    const dim3 b256(256);
    auto ew = [](int n) { return dim3((n + 255) / 256); };
    st_tn(p->cx, st, p->ctx, 256, 256, p->dOut, AE, AE, N, G + o[RT_HEAD_W]);
    st_cs(p->cx, st, p->dOut, AE, AE, N, G + o[RT_HEAD_B]);
    if ((rc = st_back(p->cx, st, p->dOut, AE, AE, P + o[RT_HEAD_W], AE, 256, p->d_ctx, 256, N))) return rc;
    hipLaunchKernelGGL(k_elu_bwd, ew(N * 256), b256, 0, st, p->d_ctx, (int64_t)256, p->ctx, (int64_t)256, (const uint8_t*)nullptr, 0.f, N * 256, 256);
    if ((rc = rawtrain_backward_from_ctx(p, N, dense, Dn, cat, seq, nullptr, st))) return rc;
    if (stats_dev) hipLaunchKernelGGL(k_reduce_terms, dim3(1), dim3(256), 0, st, p->terms, N, stats_dev);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

int rl4rs_rawtrain_adam_step(rl4rs_rawtrain* p, float lr, float beta1, float beta2, float eps, float grad_clip, void* stream) {
    RL4RS_REQUIRE(p, "rawtrain_adam_step: null handle");
    adam_step(p->opt, p->opt.grad, ADAM_TF, lr, beta1, beta2, eps, p->sumsq, grad_clip, nullptr, (hipStream_t)stream);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

}  // extern "C"
