// COMBO (d3rlpy.algos.COMBO, 'COMBO' of script/batchrl_trainer.py:130-151): SAC whose critic loss is TD + a conservative term over
// a minibatch of n_real real rows followed by F = B - n_real model-generated rows,
//     TD            = sum_c mean_{b < B} (Q_c(s_b, a_b) - y_b)^2,   y_b = r_b + gamma (1 - ter_b) min_c Qtarg_c(s'_b, tanh(mu(s'_b)))
//     conservative  = w [ sum_c mean_{f generated} logsumexp_j (Q_c(s_f, a_fj) - off_fj)  -  sum_c mean_{b real} Q_c(s_b, a_b) ]
// with the 3n sampled actions per generated row of CQL's conservative term (n of pi(.|s_f), n of pi(.|s'_f), n uniform) and no
// learned alpha.  d3rlpy 0.91 is absent: restated as published, PARITY UNPINNED, checked against tests/combo_ref.py.
//
// The critic step does not take CQL's [B][1 + 3n] layout: the real rows have no sampled actions, and at real_ratio 0.5 that layout
// would carry n_real * 3n rows (48 % of all rows at n = 10) through three layers both ways for nothing.  Two passes instead:
//     pass T   the B rows (s, a), rep = 1, the fused twin launches;  dq_c[b] = 2 (q_c[b] - y_b) / B - [b < n_real] w / n_real
//              (the data term needs no forward of its own: Q(s_real, a_real) is among these rows)
//     pass C   the F * 3n sample rows, rep = 3n (observation side of the first layer once per generated observation);
//              dq_c[f, j] = (w / F) softmax_j(q_c[f, j] - off[f, j])
// rl4rs_amlp_backward WRITES the handle's flat gradient, so the passes are joined by rl4rs_amlp_grad_stash: forward T, backward T,
// stash, forward C, backward C, add - a handle's activations are those of its last forward, which this order respects.  Every
// reduction is in a fixed order (no float atomics): an update is bit-reproducible given its noise.
// Compiled into policy.hip behind contirl.hpp (the rl4rs_amlp handle and the entry points composed here).
#pragma once

namespace rl4rs {

// pass T, one thread per row b < B: the TD and data-term gradient and the row's addends rows_t[b] = {(q1 - y)^2, (q2 - y)^2,
// [b < n_real] q1, [b < n_real] q2}
__global__ void k_combo_td(int B, int n_real, const float* __restrict__ q1, const float* __restrict__ q2, const float* __restrict__ y,
                           const float* __restrict__ w_dev, float* __restrict__ dq1, float* __restrict__ dq2, float* __restrict__ rows_t) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const bool real = b < n_real;
    const float k = real ? w_dev[0] / (float)n_real : 0.f;
    const float a = q1[b], c = q2[b];
    const float d1 = a - y[b], d2 = c - y[b];
    dq1[b] = 2.0f * d1 / (float)B - k;
    dq2[b] = 2.0f * d2 / (float)B - k;
    rows_t[(size_t)b * 4 + 0] = d1 * d1;
    rows_t[(size_t)b * 4 + 1] = d2 * d2;
    rows_t[(size_t)b * 4 + 2] = real ? a : 0.f;
    rows_t[(size_t)b * 4 + 3] = real ? c : 0.f;
}

// pass C, one wave per generated row f < F over its k = 3n samples (a lane loop where k > 64): rows_c[f] = {logsumexp_j (q1 - off),
// same for q2};  dq_c[f, j] = (w / F) softmax_j
__global__ __launch_bounds__(256) void k_combo_lse(int F, int k, const float* __restrict__ q1, const float* __restrict__ q2,
                                                   const float* __restrict__ offs, const float* __restrict__ w_dev, float* __restrict__ dq1,
                                                   float* __restrict__ dq2, float* __restrict__ rows_c) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f = blockIdx.x * 4 + wave;
    if (f >= F) return;
    const float g = w_dev[0] / (float)F;
    const float* off = offs + (size_t)f * k;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float* q = (c == 0 ? q1 : q2) + (size_t)f * k;
        float* dq = (c == 0 ? dq1 : dq2) + (size_t)f * k;
        float mx = -3.4028235e38f;
        for (int j = lane; j < k; j += 64) mx = fmaxf(mx, q[j] - off[j]);
        mx = wave_max(mx);
        float se = 0.f;
        for (int j = lane; j < k; j += 64) se += expf(q[j] - off[j] - mx);
        se = wave_sum(se);
        const float lse = mx + logf(se);
        for (int j = lane; j < k; j += 64) dq[j] = g * expf(q[j] - off[j] - lse);
        if (lane == 0) rows_c[(size_t)f * 2 + c] = lse;
    }
}

// sums[0..1] = sum_b (q_c - y)^2, sums[2..3] = sum_f logsumexp, sums[4..5] = sum_{b < n_real} q_c (single block, fixed order)
__global__ __launch_bounds__(256) void k_combo_sum6(const float* __restrict__ rows_t, int B, const float* __restrict__ rows_c, int F,
                                                    float* __restrict__ sums) {
    __shared__ float sm[6][256];
    float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int b = threadIdx.x; b < B; b += 256) {
        s[0] += rows_t[(size_t)b * 4 + 0];
        s[1] += rows_t[(size_t)b * 4 + 1];
        s[4] += rows_t[(size_t)b * 4 + 2];
        s[5] += rows_t[(size_t)b * 4 + 3];
    }
    for (int f = threadIdx.x; f < F; f += 256) {
        s[2] += rows_c[(size_t)f * 2 + 0];
        s[3] += rows_c[(size_t)f * 2 + 1];
    }
    for (int c = 0; c < 6; ++c) sm[c][threadIdx.x] = s[c];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
            for (int c = 0; c < 6; ++c) sm[c][threadIdx.x] += sm[c][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x < 6) sums[threadIdx.x] = sm[threadIdx.x][0];
}

// n <= 4 flat gradients in one launch: mode 0 buf <- gradient, mode 1 gradient <- gradient + buf
struct GradStash { float* g[4]; float* buf[4]; long long start[5]; int n, mode; };
__global__ void k_grad_stash(GradStash a) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.start[a.n]) return;
    int t = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k) t += (k < a.n && i >= a.start[k]) ? 1 : 0;
    const long long j = i - a.start[t];
    if (a.mode == 0) a.buf[t][j] = a.g[t][j];
    else a.g[t][j] = a.g[t][j] + a.buf[t][j];
}

// the uniform third of pass C's rows: acts [F, k, A] columns 2n .. 3n - 1 <- uni [F, n, A], their importance offset A log 0.5; and
// the conservative weight as the device scalar the loss kernels read
__global__ void k_combo_fill_rows(float* __restrict__ acts, float* __restrict__ offs, const float* __restrict__ uni, int F, int n, int A,
                                  float log_uniform, float weight, float* __restrict__ w_dev) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) w_dev[0] = weight;
    if (i >= F * n * A) return;
    const int a = i % A, j = (i / A) % n, f = i / (A * n);
    const int k = 3 * n, col = 2 * n + j;
    acts[((size_t)f * k + col) * A + a] = uni[i];
    if (a == 0) offs[(size_t)f * k + col] = log_uniform;
}

// metrics[0] = critic loss = (s0 + s1) / B + conservative,  metrics[3] = conservative = w ((s2 + s3) / F - (s4 + s5) / n_real);
// with logp: metrics[1] = actor loss = mean_b (e^log_temp logp_b - qmin_b)
__global__ __launch_bounds__(256) void k_combo_metrics(const float* __restrict__ sums, int B, int n_real, const float* __restrict__ w_dev,
                                                       const float* __restrict__ log_temp, const float* __restrict__ logp,
                                                       const float* __restrict__ qmin, float* __restrict__ metrics) {
    __shared__ float sm[256];
    if (threadIdx.x == 0) {
        // (combined in double and rounded once: in float the sum of the two logsumexp totals alone costs half an ulp at a few hundred,
        // more than the float32-to-float64 difference of the whole loss)
        const double cons = (double)w_dev[0] * (((double)sums[2] + (double)sums[3]) / (double)(B - n_real) - ((double)sums[4] + (double)sums[5]) / (double)n_real);
        metrics[0] = (float)(((double)sums[0] + (double)sums[1]) / (double)B + cons);
        metrics[3] = (float)cons;
    }
    if (!logp) return;
    const float et = expf(log_temp[0]);
    float s = 0.f;
    for (int i = threadIdx.x; i < B; i += 256) s += et * logp[i] - qmin[i];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) metrics[1] = sm[0] / (float)B;
}

}  // namespace rl4rs

// the refusals of the split: in d3rlpy the mean over an empty half is NaN, here it is an error (no device is needed to say so)
#define RL4RS_COMBO_SPLIT(who, B, n_real, k)                                                                                              \
    do {                                                                                                                                  \
        RL4RS_REQUIRE((B) > 0, who ": B=%d: the minibatch is empty", (int)(B));                                                           \
        RL4RS_REQUIRE((n_real) > 0, who ": n_real=%d: no real row, the data term's mean is over nothing", (int)(n_real));                  \
        RL4RS_REQUIRE((n_real) < (B), who ": n_real=%d of B=%d: no generated row, the logsumexp term's mean is over nothing", (int)(n_real), (int)(B)); \
        RL4RS_REQUIRE((k) >= 1, who ": %d action samples per generated row: the logsumexp is over nothing", (int)(k));                     \
    } while (0)

extern "C" {

int rl4rs_amlp_grad_stash(int32_t n, rl4rs_amlp* const* nets, float* const* bufs, int32_t mode, void* stream) {
    RL4RS_REQUIRE(n >= 1 && n <= 4 && nets && bufs, "amlp_grad_stash: bad argument (n=%d)", n);
    RL4RS_REQUIRE(mode == 0 || mode == 1, "amlp_grad_stash: mode %d (0 = copy out, 1 = add in)", mode);
    GradStash a;
    memset(&a, 0, sizeof(a));
    a.n = n;
    a.mode = mode;
    for (int i = 0; i < n; ++i) {
        RL4RS_REQUIRE(nets[i] && bufs[i], "amlp_grad_stash: null handle / buffer %d", i);
        a.g[i] = nets[i]->opt.grad;
        a.buf[i] = bufs[i];
        a.start[i + 1] = a.start[i] + nets[i]->opt.n;
    }
    hipLaunchKernelGGL(k_grad_stash, dim3((unsigned)((a.start[n] + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

int rl4rs_combo_critic_loss(int32_t B, int32_t n_real, int32_t k, const float* q1t, const float* q2t, const float* y, const float* q1c,
                            const float* q2c, const float* offs, const float* w, float* dq1t, float* dq2t, float* dq1c, float* dq2c,
                            float* rows_scratch, float* sums6, void* stream) {
    RL4RS_COMBO_SPLIT("combo_critic_loss", B, n_real, k);
    const bool half_t = q1t || q2t || y || dq1t || dq2t, half_c = q1c || q2c || offs || dq1c || dq2c;
    RL4RS_REQUIRE(w && rows_scratch && (half_t || half_c), "combo_critic_loss: null argument (the weight, the scratch rows, or both halves)");
    RL4RS_REQUIRE(!half_t || (q1t && q2t && y && dq1t && dq2t), "combo_critic_loss: null argument in the pass-T half");
    RL4RS_REQUIRE(!half_c || (q1c && q2c && offs && dq1c && dq2c && sums6), "combo_critic_loss: null argument in the pass-C half");
    hipStream_t st = (hipStream_t)stream;
    const int F = B - n_real;
    float* rows_t = rows_scratch;
    float* rows_c = rows_scratch + (size_t)B * 4;
    if (half_t) hipLaunchKernelGGL(k_combo_td, dim3((B + 255) / 256), dim3(256), 0, st, B, n_real, q1t, q2t, y, w, dq1t, dq2t, rows_t);
    if (half_c) {
        hipLaunchKernelGGL(k_combo_lse, dim3((F + 3) / 4), dim3(256), 0, st, F, k, q1c, q2c, offs, w, dq1c, dq2c, rows_c);
        hipLaunchKernelGGL(k_combo_sum6, dim3(1), dim3(256), 0, st, rows_t, B, rows_c, F, sums6);
    }
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

namespace {
struct ComboWs : SacWs {
    float *acts, *offs, *q1t, *q2t, *dq1t, *dq2t, *q1c, *q2c, *dq1c, *dq2c, *rows, *sums, *w, *head_new, *logp_t;
    int64_t total, off_y, off_sums;
    ComboWs(float* base, int64_t B, int64_t n_real, int64_t n, int64_t A);
};
ComboWs::ComboWs(float* base, int64_t B, int64_t n_real, int64_t n, int64_t A) {
    ComboWs& w = *this;
    WsTake take{base};
    const int64_t F = B - n_real, R = F * 3 * n;
    w.head_nxt = take(B * 2 * A); w.head_obs = take(B * 2 * A); w.a_next = take(B * A); w.q1n = take(B); w.q2n = take(B);
    w.off_y = take.o; w.yq = take(B);
    w.acts = take(R * A); w.offs = take(R);
    w.q1t = take(B); w.q2t = take(B); w.dq1t = take(B); w.dq2t = take(B);
    w.q1c = take(R); w.q2c = take(R); w.dq1c = take(R); w.dq2c = take(R);
    w.rows = take(B * 4 + F * 2);
    w.off_sums = take.o; w.sums = take(8); w.w = take(4);
    w.a_pi = take(B * A); w.logp = take(B); w.q1p = take(B); w.q2p = take(B); w.qmin = take(B); w.dqa = take(B); w.dqb = take(B);
    w.g1 = take(B * A); w.g2 = take(B * A); w.d_head = take(B * 2 * A); w.head_new = take(B * 2 * A); w.a_tmp = take(B * A); w.logp_t = take(B);
    w.total = take.o;
}
}  // namespace

int64_t rl4rs_combo_workspace_floats(int32_t B, int32_t n_real, int32_t n, int32_t A) {
    if (B <= 0 || n_real <= 0 || n_real >= B || n < 1 || A <= 0) {
        set_error("combo_workspace_floats: bad sizes (B=%d, n_real=%d, n=%d, A=%d)", B, n_real, n, A);
        return -1;
    }
    return ComboWs(nullptr, B, n_real, n, A).total;
}

int64_t rl4rs_combo_workspace_offset(int32_t B, int32_t n_real, int32_t n, int32_t A, int32_t what) {
    if (rl4rs_combo_workspace_floats(B, n_real, n, A) < 0) return -1;
    const ComboWs w(nullptr, B, n_real, n, A);
    if (what == 0) return w.off_y;
    if (what == 1) return w.off_sums;
    set_error("combo_workspace_offset: what=%d (0 = y, 1 = the six sums)", what);
    return -1;
}

int rl4rs_combo_update(const rl4rs_combo_step* s, void* stream) {
    RL4RS_REQUIRE(s, "combo_update: null step");
    RL4RS_COMBO_SPLIT("combo_update", s->B, s->n_real, 3 * (int64_t)s->n);
    RL4RS_REQUIRE(s->policy && s->q1 && s->q2 && s->q1_targ && s->q2_targ, "combo_update: null handle");
    RL4RS_REQUIRE(s->A > 0 && s->log_temp_dev && s->obs_dev && s->act_dev && s->rew_dev && s->nxt_dev && s->ter_dev && s->normal_dev && s->uniform_dev &&
                  s->stash_dev && s->workspace_dev && s->metrics_dev, "combo_update: null argument");
    RL4RS_REQUIRE(((uintptr_t)s->workspace_dev & 15) == 0, "combo_update: workspace_dev is not 16-byte aligned");
    RL4RS_REQUIRE(((uintptr_t)s->normal_dev & 15) == 0 && ((uintptr_t)s->stash_dev & 15) == 0, "combo_update: normal_dev / stash_dev is not 16-byte aligned");
    RL4RS_REQUIRE(s->policy->c.act_dim == 0 && s->policy->c.out_dim == 2 * s->A, "combo_update: the policy must be a plain encoder with a [mu | logstd] head");
    RL4RS_REQUIRE(s->q1->opt.n == s->q2->opt.n && s->q1->c.act_dim == s->A && s->q1->c.obs_dim == s->policy->c.obs_dim,
                  "combo_update: the critics do not match each other or the policy");
    hipStream_t st = (hipStream_t)stream;
    const int B = s->B, n_real = s->n_real, n = s->n, A = s->A, D = s->policy->c.obs_dim, F = B - n_real, k = 3 * n, R = F * k;
    const ComboWs w(s->workspace_dev, B, n_real, n, A);
    const float lo = SAC_MIN_LOGSTD, hi = SAC_MAX_LOGSTD;
    const float* eps_t = s->normal_dev;
    const float* eps_tp1 = eps_t + (size_t)F * n * A;
    const float* eps_actor = eps_tp1 + (size_t)F * n * A;
    const float* eps_temp = eps_actor + (size_t)B * A;
    const float* obs_f = s->obs_dev + (size_t)n_real * D;
    const float log_uniform = (float)((double)A * log(0.5));
    rl4rs_amlp* twin[2] = {s->q1, s->q2};
    // (the generated rows' heads are rows n_real .. B - 1 of the two forwards)
    RL4RS_TRY(sac_policy_heads(s, w, stream));
    RL4RS_TRY(sac_deterministic_target(s, w, stream));
    // --- the F * 3n rows of pass C: [pi(s_f) | pi(s'_f) | uniform] with their importance offsets
    hipLaunchKernelGGL(k_combo_fill_rows, dim3((F * n * A + 255) / 256), dim3(256), 0, st, w.acts, w.offs, s->uniform_dev, F, n, A, log_uniform,
                       s->conservative_weight, w.w);
    RL4RS_TRY(rl4rs_squashed_sample(F * n, n, A, w.head_obs + (size_t)n_real * 2 * A, eps_t, lo, hi, k, 0, w.acts, w.offs, stream));
    RL4RS_TRY(rl4rs_squashed_sample(F * n, n, A, w.head_nxt + (size_t)n_real * 2 * A, eps_tp1, lo, hi, k, n, w.acts, w.offs, stream));
    // --- critic, pass T
    {
        float* qv[2] = {w.q1t, w.q2t};
        RL4RS_TRY(rl4rs_amlp_forward_multi(2, twin, B, s->obs_dev, s->act_dev, qv, stream));
        RL4RS_TRY(rl4rs_combo_critic_loss(B, n_real, k, w.q1t, w.q2t, w.yq, nullptr, nullptr, nullptr, w.w, w.dq1t, w.dq2t, nullptr, nullptr, w.rows, nullptr, stream));
        const float* dq[2] = {w.dq1t, w.dq2t};
        RL4RS_TRY(rl4rs_amlp_backward_multi(2, twin, B, s->obs_dev, s->act_dev, dq, nullptr, 1, stream));
    }
    float* stash[2] = {s->stash_dev, s->stash_dev + (s->q1->opt.n + 3) / 4 * 4};
    RL4RS_TRY(rl4rs_amlp_grad_stash(2, twin, stash, 0, stream));
    // --- critic, pass C
    RL4RS_TRY(rl4rs_amlp_forward(s->q1, R, k, obs_f, w.acts, w.q1c, stream));
    RL4RS_TRY(rl4rs_amlp_forward(s->q2, R, k, obs_f, w.acts, w.q2c, stream));
    RL4RS_TRY(rl4rs_combo_critic_loss(B, n_real, k, nullptr, nullptr, nullptr, w.q1c, w.q2c, w.offs, w.w, nullptr, nullptr, w.dq1c, w.dq2c, w.rows, w.sums, stream));
    RL4RS_TRY(rl4rs_amlp_backward(s->q1, R, k, obs_f, w.acts, w.dq1c, nullptr, 1, stream));
    RL4RS_TRY(rl4rs_amlp_backward(s->q2, R, k, obs_f, w.acts, w.dq2c, nullptr, 1, stream));
    RL4RS_TRY(rl4rs_amlp_grad_stash(2, twin, stash, 1, stream));
    RL4RS_TRY(amlp_adam_pair(s->q1, s->q2, s->critic_lr, stream));
    if (!s->do_actor) {
        hipLaunchKernelGGL(k_combo_metrics, dim3(1), dim3(256), 0, st, w.sums, B, n_real, w.w, s->log_temp_dev, nullptr, nullptr, s->metrics_dev);
        RL4RS_LAUNCH_CHECK();
        return RL4RS_OK;
    }
    // --- actor through the stepped critics; the metrics read logp and qmin before the Adam (which reads neither, nor what the
    // temperature step writes)
    RL4RS_TRY(sac_actor_phase(s, w, eps_actor, stream));
    hipLaunchKernelGGL(k_combo_metrics, dim3(1), dim3(256), 0, st, w.sums, B, n_real, w.w, s->log_temp_dev, w.logp, w.qmin, s->metrics_dev);
    RL4RS_TRY(sac_actor_adam(s, stream));
    // --- temperature (SACImpl.update_temp) on the STEPPED policy, as MOPO.update orders it
    if (s->temp_lr > 0.f) {
        RL4RS_TRY(rl4rs_amlp_forward(s->policy, B, 1, s->obs_dev, nullptr, w.head_new, stream));
        RL4RS_TRY(sac_temp_step(s, w.head_new, eps_temp, w.a_tmp, w.logp_t, stream));
    }
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

}  // extern "C"
