// On-device TD3 / DDPG for the continuous-action env (include/rl4rs_hip.h, "On-device TD3 / DDPG"): Ornstein-Uhlenbeck exploration,
// target-policy smoothing, the (twin) critic loss, the tanh head's derivative, the L2 term on the weight matrices and one whole
// update as one host call.  Compiled into policy.hip behind contirl.hpp (the rl4rs_amlp handle and its forward / backward / Adam)
// and dqn.hpp (the replay ring); uniform01 is the policy net's counter RNG.
//
// Reference: script/modelfree_train.py:46-48,79-105 (algo "TD3" / "DDPG" on support_conti_env: RLlib 1.5.1 DDPGTrainer / TD3Trainer,
// twin_q, policy_delay 2, smooth_target_policy, actor_hiddens = critic_hiddens = [400, 300], OrnsteinUhlenbeckNoise).  The driver's
// DDPG branch is an `if` in front of a separate `if TD3 / elif ... / else: raise` chain, so algo == "DDPG" raises there; TD3 is the
// one that runs, and DDPG is TD3 with twin_q, the delay and the smoothing off.  RLlib's ddpg_tf_policy / ddpg_tf_model /
// OrnsteinUhlenbeckNoise are third-party and absent: restated from their published 1.5.1 form, PARITY UNPINNED, checked
// against the fp64 restatement in tests/td3_ref.py.
//
// The networks are two amlps (contirl.hpp): the actor obs -> relu -> relu -> tanh (RLlib's sigmoid(2x) * (high - low) + low on
// Box(-1, 1)), the critics cat([obs, action]) -> relu -> relu -> 1.  Nothing here multiplies matrices: every kernel below is an
// element-wise or one-workgroup pass over at most a minibatch, with sums in a fixed order (bit-identical from run to run).
#pragma once

namespace rl4rs {

// (normal01, the Box-Muller draw on the counter RNG, lives beside uniform01 in common.hpp: gausspolicy.hip draws from it too)

struct ExploreOu {
    int N, E, state_rows, random_phase, advance;
    float theta, sigma, scale;
    uint32_t seed, step;
    const float* det; float* ou; float* out; float* eps_out;
};

// state_rows = 1: the one shared [E] state advances ONCE, in front of the per-row kernel (which then only reads it)
__global__ void k_ou_advance_shared(ExploreOu a) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.E) return;
    const float s = a.ou[e];
    a.ou[e] = s + a.theta * (-s) + a.sigma * normal01(a.seed, a.step, 0u, (uint32_t)e);
}

// One thread per action element.  random_phase: a = 2u - 1, the state is not touched.  Otherwise the element's state advances
// (advance = 1: every row owns its state) and a = clip(det + scale * state * (high - low), -1, 1), high - low = 2.
__global__ void k_explore_ou(ExploreOu a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.N * a.E) return;
    const int n = i / a.E, e = i - n * a.E;
    if (a.random_phase) {
        a.out[i] = 2.f * uniform01(a.seed, a.step, (uint32_t)n, (uint32_t)e) - 1.f;
        return;
    }
    const int srow = a.state_rows == 1 ? 0 : n;
    const float eps = normal01(a.seed, a.step, (uint32_t)srow, (uint32_t)e);
    float s = a.ou[(size_t)srow * a.E + e];
    if (a.advance) {
        s = s + a.theta * (-s) + a.sigma * eps;
        a.ou[(size_t)srow * a.E + e] = s;
    }
    if (a.eps_out) a.eps_out[i] = eps;
    a.out[i] = fminf(fmaxf(a.det[i] + a.scale * s * 2.f, -1.f), 1.f);
}

// TD3 target-policy smoothing: out = clip(a + clip(target_noise * eps, -c, c), -1, 1)
__global__ void k_td3_smooth(int n, const float* a, const float* __restrict__ eps, float target_noise, float c, float* out) {   // (out may be a)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float z = fminf(fmaxf(target_noise * eps[i], -c), c);
    out[i] = fminf(fmaxf(a[i] + z, -1.f), 1.f);
}

// d_pre = d_out * (1 - tanh_out^2)
__global__ void k_tanh_head_grad(int n, const float* __restrict__ t, const float* __restrict__ d_out, float* __restrict__ d_pre) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) d_pre[i] = d_out[i] * (1.f - t[i] * t[i]);
}

// grad += l2 * W on the three weight matrices (segments [w0, w0e) | [w1, w1e) | [w2, w2e) of the flat layout); biases untouched
__global__ void k_amlp_add_l2(float* __restrict__ g, const float* __restrict__ p, long long n, long long b1, long long w2, long long b2,
                              long long w3, long long b3, float l2) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool weight = i < b1 || (i >= w2 && i < b2) || (i >= w3 && i < b3);
    if (weight) g[i] += l2 * p[i];
}

struct Td3Loss {
    int N, use_huber;
    float gamma, delta;
    const float *q1, *q2, *q1t, *q2t, *rew, *w;
    const int32_t* done;
    float *dq1, *dq2, *y, *td, *stats;
};

__device__ __forceinline__ float td3_err(float td, int use_huber, float delta, float* d) {
    if (!use_huber) { *d = td; return 0.5f * td * td; }
    const float ad = fabsf(td);
    *d = fminf(fmaxf(td, -delta), delta);
    return ad < delta ? 0.5f * td * td : delta * (ad - 0.5f * delta);
}

// RLlib ddpg_tf_policy's critic loss on one minibatch: one workgroup, every thread walks its rows in order, the 256 partial sums
// meet in a fixed tree: stats = sums of {w * error, q1, y, |td1|}.  y is a SELECT on done: nothing of a terminal row's target Q
// (NaN included) reaches any output.
__global__ __launch_bounds__(256) void k_td3_critic_loss(Td3Loss a) {
    __shared__ float4 sm[256];
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    const float inv = 1.0f / (float)a.N;
    for (int n = threadIdx.x; n < a.N; n += 256) {
        const float r = a.rew[n];
        float y = r;
        if (a.done[n] == 0) {
            const float qn = a.q2t ? fminf(a.q1t[n], a.q2t[n]) : a.q1t[n];
            y = r + a.gamma * qn;
        }
        const float wgt = a.w ? a.w[n] : 1.f;
        const float q1 = a.q1[n], td1 = q1 - y;
        float d1, d2 = 0.f;
        float err = td3_err(td1, a.use_huber, a.delta, &d1);
        a.dq1[n] = wgt * d1 * inv;
        if (a.q2) {
            err += td3_err(a.q2[n] - y, a.use_huber, a.delta, &d2);
            a.dq2[n] = wgt * d2 * inv;
        }
        if (a.y) a.y[n] = y;
        if (a.td) a.td[n] = td1;
        s.x += wgt * err; s.y += q1; s.z += y; s.w += fabsf(td1);
    }
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const float4 t = sm[threadIdx.x + o];
            sm[threadIdx.x].x += t.x; sm[threadIdx.x].y += t.y; sm[threadIdx.x].z += t.z; sm[threadIdx.x].w += t.w;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && a.stats) { a.stats[0] = sm[0].x; a.stats[1] = sm[0].y; a.stats[2] = sm[0].z; a.stats[3] = sm[0].w; }
}

// out[0] = -sum_n q[n] (the actor loss is out[0] / N): one workgroup, fixed order
__global__ __launch_bounds__(256) void k_neg_sum(const float* __restrict__ q, int N, float* __restrict__ out) {
    __shared__ float sm[256];
    float s = 0.f;
    for (int n = threadIdx.x; n < N; n += 256) s += q[n];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = -sm[0];
}

}  // namespace rl4rs

extern "C" {

int rl4rs_explore_ou(int32_t N, int32_t E, int32_t state_rows, const float* det_action_dev, float* ou_state_dev, float theta, float sigma,
                     float scale, uint32_t seed, uint32_t step, int32_t random_phase, float* action_out_dev, float* eps_out_dev,
                     void* stream) {
    RL4RS_REQUIRE(N > 0 && E > 0 && (int64_t)N * E < ((int64_t)1 << 31) && action_out_dev && (random_phase || (det_action_dev && ou_state_dev)),
                  "explore_ou: bad argument");
    RL4RS_REQUIRE(state_rows == 1 || state_rows == N, "explore_ou: state_rows must be 1 or N (got %d, N = %d)", state_rows, N);
    hipStream_t st = (hipStream_t)stream;
    ExploreOu a;
    a.N = N; a.E = E; a.state_rows = state_rows; a.random_phase = random_phase ? 1 : 0; a.advance = state_rows == 1 ? 0 : 1;
    a.theta = theta; a.sigma = sigma; a.scale = scale; a.seed = seed; a.step = step;
    a.det = det_action_dev; a.ou = ou_state_dev; a.out = action_out_dev; a.eps_out = eps_out_dev;
    if (!a.random_phase && state_rows == 1) hipLaunchKernelGGL(k_ou_advance_shared, dim3((E + 255) / 256), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_explore_ou, dim3((N * E + 255) / 256), dim3(256), 0, st, a);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

int rl4rs_td3_smooth_action(int32_t N, int32_t E, const float* action_dev, const float* eps_dev, float target_noise, float noise_clip,
                            float* out_dev, void* stream) {
    RL4RS_REQUIRE(N > 0 && E > 0 && (int64_t)N * E < ((int64_t)1 << 31) && action_dev && eps_dev && out_dev && noise_clip >= 0.f,
                  "td3_smooth_action: bad argument");
    hipLaunchKernelGGL(k_td3_smooth, dim3((N * E + 255) / 256), dim3(256), 0, (hipStream_t)stream, N * E, action_dev, eps_dev, target_noise,
                       noise_clip, out_dev);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

int rl4rs_td3_critic_loss(int32_t N, const float* q1_dev, const float* q2_dev, const float* q1_targ_dev, const float* q2_targ_dev,
                          const float* rewards_dev, const int32_t* dones_dev, const float* weights_dev, float gamma, int32_t use_huber,
                          float huber_threshold, float* dq1_dev, float* dq2_dev, float* y_out_dev, float* td_out_dev, float* stats4_dev,
                          void* stream) {
    RL4RS_REQUIRE(N > 0 && q1_dev && q1_targ_dev && rewards_dev && dones_dev && dq1_dev, "td3_critic_loss: bad argument");
    RL4RS_REQUIRE((q2_dev != nullptr) == (dq2_dev != nullptr), "td3_critic_loss: q2 and dq2 go together");
    RL4RS_REQUIRE(!use_huber || huber_threshold > 0.f, "td3_critic_loss: huber_threshold must be positive");
    Td3Loss a;
    a.N = N; a.use_huber = use_huber ? 1 : 0; a.gamma = gamma; a.delta = huber_threshold;
    a.q1 = q1_dev; a.q2 = q2_dev; a.q1t = q1_targ_dev; a.q2t = q2_targ_dev; a.rew = rewards_dev; a.w = weights_dev; a.done = dones_dev;
    a.dq1 = dq1_dev; a.dq2 = dq2_dev; a.y = y_out_dev; a.td = td_out_dev; a.stats = stats4_dev;
    hipLaunchKernelGGL(k_td3_critic_loss, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

int rl4rs_tanh_head_grad(int32_t N, int32_t E, const float* tanh_out_dev, const float* d_out_dev, float* d_pre_dev, void* stream) {
    RL4RS_REQUIRE(N > 0 && E > 0 && (int64_t)N * E < ((int64_t)1 << 31) && tanh_out_dev && d_out_dev && d_pre_dev, "tanh_head_grad: bad argument");
    hipLaunchKernelGGL(k_tanh_head_grad, dim3((N * E + 255) / 256), dim3(256), 0, (hipStream_t)stream, N * E, tanh_out_dev, d_out_dev, d_pre_dev);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

int rl4rs_amlp_add_l2(rl4rs_amlp* p, float l2, void* stream) {
    RL4RS_REQUIRE(p, "amlp_add_l2: null handle");
    if (l2 == 0.f) return RL4RS_OK;
    const int64_t* o = p->off;
    hipLaunchKernelGGL(k_amlp_add_l2, dim3((unsigned)((p->opt.n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p->opt.grad, p->opt.params,
                       (long long)p->opt.n, (long long)o[AP_B1], (long long)o[AP_W2], (long long)o[AP_B2], (long long)o[AP_W3],
                       (long long)o[AP_B3], l2);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

// ---- one whole TD3 / DDPG update as one host call (include/rl4rs_hip.h: rl4rs_td3_step)
namespace {
struct Td3Ws {
    float *a_next, *q1n, *q2n, *q1v, *q2v, *dq1, *dq2, *y, *a_pi, *qv, *minus_inv_m, *da, *d_pre;
    int64_t total;
};
Td3Ws td3_ws(float* base, int64_t M, int64_t E) {
    Td3Ws w;
    int64_t o = 0;
    auto take = [&](int64_t cnt) { float* p = base ? base + o : nullptr; o += (cnt + 3) / 4 * 4; return p; };
    w.a_next = take(M * E); w.q1n = take(M); w.q2n = take(M); w.q1v = take(M); w.q2v = take(M); w.dq1 = take(M); w.dq2 = take(M);
    w.y = take(M); w.a_pi = take(M * E); w.qv = take(M); w.minus_inv_m = take(M); w.da = take(M * E); w.d_pre = take(M * E);
    w.total = o;
    return w;
}
}  // namespace

int64_t rl4rs_td3_workspace_floats(int32_t M, int32_t E) { return td3_ws(nullptr, M, E).total; }

int rl4rs_td3_update(const rl4rs_td3_step* s, void* stream) {
    RL4RS_REQUIRE(s && s->actor && s->actor_targ && s->q1 && s->q1_targ, "td3_update: null handle");
    RL4RS_REQUIRE((s->q2 != nullptr) == (s->q2_targ != nullptr), "td3_update: q2 and q2_targ go together (both NULL: DDPG's single critic)");
    RL4RS_REQUIRE(s->M > 0 && s->E > 0 && s->obs_dev && s->act_dev && s->rew_dev && s->done_dev && s->nxt_dev && s->workspace_dev &&
                  s->td_out_dev && s->metrics_dev && ((uintptr_t)s->workspace_dev & 15) == 0 && (!s->smooth_target_policy || s->noise_dev),
                  "td3_update: bad argument");
    // every handle is read with the layout its role implies: the targets have their online network's shape, the critics share the
    // actor's observation width, and M fits every handle that sees the minibatch
    {
        const rl4rs_amlp_cfg& ac = s->actor->c;
        const rl4rs_amlp_cfg& qc = s->q1->c;
        RL4RS_REQUIRE(ac.out_dim == s->E && ac.act_dim == 0 && ac.head_act == ACT_TANH && qc.act_dim == s->E && qc.out_dim == 1 &&
                      qc.head_act == ACT_NONE && qc.obs_dim == ac.obs_dim,
                      "td3_update: the actor must be obs -> tanh [E], the critics (obs, action [E]) -> 1 on the same observations");
        auto same = [](const rl4rs_amlp_cfg& x, const rl4rs_amlp_cfg& y) {
            return x.obs_dim == y.obs_dim && x.act_dim == y.act_dim && x.hidden1 == y.hidden1 && x.hidden2 == y.hidden2 && x.out_dim == y.out_dim &&
                   x.head_act == y.head_act;
        };
        RL4RS_REQUIRE(same(s->actor_targ->c, ac), "td3_update: actor_targ has another shape than actor");
        RL4RS_REQUIRE(same(s->q1_targ->c, qc), "td3_update: q1_targ has another shape than q1");
        RL4RS_REQUIRE(!s->q2 || (same(s->q2->c, qc) && same(s->q2_targ->c, qc)), "td3_update: q2 / q2_targ have another shape than q1");
        const rl4rs_amlp* all[6] = {s->actor, s->actor_targ, s->q1, s->q1_targ, s->q2, s->q2_targ};
        for (int i = 0; i < 6; ++i)
            RL4RS_REQUIRE(!all[i] || s->M <= all[i]->c.max_rows, "td3_update: M = %d exceeds max_rows = %d of handle %d", s->M, all[i]->c.max_rows, i);
        RL4RS_REQUIRE(s->M <= ac.max_grad_rows && s->M <= qc.max_grad_rows && (!s->q2 || s->M <= s->q2->c.max_grad_rows),
                      "td3_update: M = %d exceeds max_grad_rows of an online network", s->M);
    }
    hipStream_t st = (hipStream_t)stream;
    const int M = s->M, E = s->E, nq = s->q2 ? 2 : 1;
    const Td3Ws w = td3_ws(s->workspace_dev, M, E);
    int rc;
#define TU(expr) do { if ((rc = (expr)) != RL4RS_OK) return rc; } while (0)
    // --- target: a' = actor_targ(s') (+ clipped noise), q' = min over the target critics
    TU(rl4rs_amlp_forward(s->actor_targ, M, 1, s->nxt_dev, nullptr, w.a_next, stream));
    if (s->smooth_target_policy) TU(rl4rs_td3_smooth_action(M, E, w.a_next, s->noise_dev, s->target_noise, s->target_noise_clip, w.a_next, stream));
    rl4rs_amlp* targ[2] = {s->q1_targ, s->q2_targ};
    float* qn[2] = {w.q1n, w.q2n};
    TU(rl4rs_amlp_forward_multi(nq, targ, M, s->nxt_dev, w.a_next, qn, stream));
    // --- critics: both gradients of an update come from the parameters BEFORE its step (RLlib's TF policy: one session run)
    rl4rs_amlp* twin[2] = {s->q1, s->q2};
    float* qv2[2] = {w.q1v, w.q2v};
    TU(rl4rs_amlp_forward_multi(nq, twin, M, s->obs_dev, s->act_dev, qv2, stream));
    TU(rl4rs_td3_critic_loss(M, w.q1v, s->q2 ? w.q2v : nullptr, w.q1n, s->q2 ? w.q2n : nullptr, s->rew_dev, s->done_dev, s->weights_dev,
                             s->gamma, s->use_huber, s->huber_threshold, w.dq1, s->q2 ? w.dq2 : nullptr, w.y, s->td_out_dev, s->metrics_dev,
                             stream));
    const float* dq[2] = {w.dq1, w.dq2};
    TU(rl4rs_amlp_backward_multi(nq, twin, M, s->obs_dev, s->act_dev, dq, nullptr, 1, stream));
    for (int i = 0; i < nq; ++i) TU(rl4rs_amlp_add_l2(twin[i], s->l2_reg, stream));
    if (s->do_actor) {
        // --- actor: -mean Q_1(s, pi(s)) through the critic's action-input gradient and the tanh head
        hipLaunchKernelGGL(k_fill, dim3((M + 255) / 256), dim3(256), 0, st, w.minus_inv_m, M, -1.0f / (float)M);
        TU(rl4rs_amlp_forward(s->actor, M, 1, s->obs_dev, nullptr, w.a_pi, stream));
        TU(rl4rs_amlp_forward(s->q1, M, 1, s->obs_dev, w.a_pi, w.qv, stream));
        TU(rl4rs_amlp_backward(s->q1, M, 1, s->obs_dev, w.a_pi, w.minus_inv_m, w.da, 0, stream));
        TU(rl4rs_tanh_head_grad(M, E, w.a_pi, w.da, w.d_pre, stream));
        TU(rl4rs_amlp_backward(s->actor, M, 1, s->obs_dev, nullptr, w.d_pre, nullptr, 1, stream));
        TU(rl4rs_amlp_add_l2(s->actor, s->l2_reg, stream));
        hipLaunchKernelGGL(k_neg_sum, dim3(1), dim3(256), 0, st, w.qv, M, s->metrics_dev + 4);
    }
    // --- one optimiser launch: Adam of the critics (and the actor when it stepped) + ALL soft target updates
    {
        rl4rs_amlp* nets[3] = {s->q1, s->q2 ? s->q2 : s->actor, s->actor};
        rl4rs_amlp* tg[3] = {s->q1_targ, s->q2 ? s->q2_targ : s->actor_targ, s->actor_targ};
        const float lr[3] = {s->critic_lr, s->q2 ? s->critic_lr : s->actor_lr, s->actor_lr};
        const int32_t on[3] = {1, s->q2 ? 1 : (s->do_actor ? 1 : 0), s->do_actor ? 1 : 0};
        TU(rl4rs_amlp_adam_multi(nq + 1, nets, lr, on, tg, 0.9f, 0.999f, 1e-7f, s->tau, stream));
    }
#undef TU
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

}  // extern "C"
