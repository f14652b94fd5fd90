// On-device IMPALA (include/rl4rs_hip.h, "V-trace"): the V-trace off-policy correction as a backward scan over time per env, and
// the one-call V-trace loss and gradient on the masked policy (evaluate -> V-trace per rollout -> the A2C-form loss with
// adv = pg_adv, ret = vs).  Compiled into policy.hip: rl4rs_policy, rl4rs_policy_evaluate and rl4rs_policy_loss_grad live there.
//
// Reference: script/modelfree_train.py:345-390 (algo "IMPALA": RLlib 1.5.1's impala on the mask model, gamma 1, grad_clip 10, Adam,
// lr 1e-4, vf_loss_coeff 0.5, entropy_coeff 0.01).  RLlib's vtrace_tf.from_importance_weights / VTraceLoss are third-party and absent:
// restated from their published 1.5.1 form, PARITY UNPINNED, checked against the fp64 restatement in tests/vtrace_ref.py.
//
// Arrays are time-major [T, B] (row stride B): one thread owns one env column b and walks t from T - 1 down to 0, so every load and
// store of a step is coalesced over b.  The scan state (acc, V_{t+1}, vs_{t+1}) is float64 and the outputs are rounded once on the
// store.  The inputs of a step do not depend on the scan state: they are fetched VT_U steps at a time, the next group's loads in
// flight while the current group's dependent chain (one double exp + a dozen double operations per step) runs.
#pragma once

namespace rl4rs {

constexpr int VT_U = 8;       // steps of one column fetched together (5 loads each)

__global__ __launch_bounds__(64) void k_vtrace(int T, int B, const float* __restrict__ blp, const float* __restrict__ tlp,
                                               const float* __restrict__ values, const float* __restrict__ boot,
                                               const double* __restrict__ rewards, const int32_t* __restrict__ dones, float gamma_f,
                                               float clip_rho_f, float clip_pg_f, float* __restrict__ vs_out, float* __restrict__ pg_out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const double gamma = (double)gamma_f, clip_rho = (double)clip_rho_f, clip_pg = (double)clip_pg_f;
    double v_next = boot ? (double)boot[b] : 0.0;       // V_{t+1}; the bootstrap at t = T - 1
    double vs_next = v_next;                            // vs_{t+1}; the bootstrap at t = T - 1
    double acc = 0.0;                                   // acc_{t+1}; acc_T = 0
    float nb[VT_U], nt[VT_U], nv[VT_U];
    double nr[VT_U];
    int32_t nd[VT_U];
    auto fetch = [&](int t_hi) {                        // steps t_hi, t_hi - 1, ... (clamped at 0: unconditional loads issue together)
#pragma unroll
        for (int u = 0; u < VT_U; ++u) {
            const int t = t_hi - u;
            const size_t i = (size_t)(t > 0 ? t : 0) * B + b;
            nb[u] = blp[i]; nt[u] = tlp[i]; nv[u] = values[i]; nr[u] = rewards[i];
            nd[u] = dones ? dones[i] : 0;
        }
    };
    fetch(T - 1);
    for (int t_hi = T - 1; t_hi >= 0; t_hi -= VT_U) {
        float cb[VT_U], ct[VT_U], cv[VT_U];
        double cr[VT_U];
        int32_t cd[VT_U];
#pragma unroll
        for (int u = 0; u < VT_U; ++u) { cb[u] = nb[u]; ct[u] = nt[u]; cv[u] = nv[u]; cr[u] = nr[u]; cd[u] = nd[u]; }
        if (t_hi - VT_U >= 0) fetch(t_hi - VT_U);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < VT_U; ++u) {
            const int t = t_hi - u;
            if (t >= 0) {
                const double rho = exp((double)ct[u] - (double)cb[u]);
                const double disc = gamma * (cd[u] != 0 ? 0.0 : 1.0);
                const double V = (double)cv[u], r = cr[u];
                const double delta = fmin(clip_rho, rho) * (r + disc * v_next - V);
                acc = delta + disc * fmin(1.0, rho) * acc;
                const double vs = V + acc;
                const double pg = fmin(clip_pg, rho) * (r + disc * vs_next - V);
                const size_t i = (size_t)t * B + b;
                vs_out[i] = (float)vs;
                pg_out[i] = (float)pg;
                v_next = V;
                vs_next = vs;
            }
        }
    }
}

// stats[0..3] (+)= {sum rho, sum min(rho, clip_rho), sum vs, sum pg_adv} over the n = T * B entries, in float64: single block, every
// thread sums its entries in index order through eight accumulators joined in a fixed order, then a fixed tree - bit-identical
// from run to run.  vs / pg_adv are the float32 values the scan stored.
__global__ __launch_bounds__(256) void k_vtrace_stats(size_t n, const float* __restrict__ blp, const float* __restrict__ tlp,
                                                      const float* __restrict__ vs, const float* __restrict__ pg, float clip_rho_f,
                                                      int accumulate, double* __restrict__ stats) {
    __shared__ double sm[4][256];
    const double clip_rho = (double)clip_rho_f;
    double a0[8], a1[8], a2[8], a3[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { a0[u] = 0.0; a1[u] = 0.0; a2[u] = 0.0; a3[u] = 0.0; }
    for (size_t i0 = threadIdx.x; i0 < n; i0 += 256 * 8) {
        float xb[8], xt[8], xv[8], xp[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const size_t i = i0 + 256 * u < n ? i0 + 256 * u : n - 1;
            xb[u] = blp[i]; xt[u] = tlp[i]; xv[u] = vs[i]; xp[u] = pg[i];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (i0 + 256 * u < n) {
                const double rho = exp((double)xt[u] - (double)xb[u]);
                a0[u] += rho; a1[u] += fmin(rho, clip_rho); a2[u] += (double)xv[u]; a3[u] += (double)xp[u];
            }
    }
    sm[0][threadIdx.x] = ((a0[0] + a0[1]) + (a0[2] + a0[3])) + ((a0[4] + a0[5]) + (a0[6] + a0[7]));
    sm[1][threadIdx.x] = ((a1[0] + a1[1]) + (a1[2] + a1[3])) + ((a1[4] + a1[5]) + (a1[6] + a1[7]));
    sm[2][threadIdx.x] = ((a2[0] + a2[1]) + (a2[2] + a2[3])) + ((a2[4] + a2[5]) + (a2[6] + a2[7]));
    sm[3][threadIdx.x] = ((a3[0] + a3[1]) + (a3[2] + a3[3])) + ((a3[4] + a3[5]) + (a3[6] + a3[7]));
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int k = 0; k < 4; ++k) sm[k][threadIdx.x] += sm[k][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x < 4) stats[threadIdx.x] = (accumulate ? stats[threadIdx.x] : 0.0) + sm[threadIdx.x][0];
}

static int launch_vtrace(int32_t T, int32_t B, const float* blp, const float* tlp, const float* values, const float* boot,
                         const double* rewards, const int32_t* dones, float gamma, float clip_rho, float clip_pg_rho, float* vs_out,
                         float* pg_adv_out, double* stats_out, int accumulate, hipStream_t st) {
    hipLaunchKernelGGL(k_vtrace, dim3((B + 63) / 64), dim3(64), 0, st, T, B, blp, tlp, values, boot, rewards, dones, gamma, clip_rho,
                       clip_pg_rho, vs_out, pg_adv_out);
    if (stats_out)
        hipLaunchKernelGGL(k_vtrace_stats, dim3(1), dim3(256), 0, st, (size_t)T * B, blp, tlp, vs_out, pg_adv_out, clip_rho, accumulate,
                           stats_out);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

// scratch of the V-trace loss on a policy handle, allocated by the first call that needs it (A2C / PPO / DQN users never pay for it)
static int vtrace_scratch(rl4rs_policy* p, bool compact) {
    int rc;
    auto alloc = [&](float** dst, size_t n) {
        int r = dev_alloc(dst, n);
        if (r == RL4RS_OK) p->owned.push_back(*dst);
        return r;
    };
    if (!p->vt_logp) {
        if ((rc = alloc(&p->vt_val, (size_t)p->max_rows))) return rc;
        if ((rc = alloc(&p->vt_vs, (size_t)p->max_rows))) return rc;
        if ((rc = alloc(&p->vt_pg, (size_t)p->max_rows))) return rc;
        if ((rc = alloc(&p->vt_logp, (size_t)p->max_rows))) return rc;
    }
    if (compact && !p->vt_obs) {       // the kept rows of R > 1 rollouts with a dropped last step are not one row range
        float *m4, *a4;
        if ((rc = alloc(&m4, (size_t)p->max_rows * p->d.W))) return rc;
        if ((rc = alloc(&a4, (size_t)p->max_rows))) return rc;
        p->vt_mask = reinterpret_cast<uint32_t*>(m4);
        p->vt_act = reinterpret_cast<int32_t*>(a4);
        if ((rc = alloc(&p->vt_obs, (size_t)p->max_rows * p->d.OD))) return rc;
    }
    return RL4RS_OK;
}

}  // namespace rl4rs

extern "C" {

int rl4rs_vtrace(int32_t T, int32_t B, const float* behaviour_logp, const float* target_logp, const float* values,
                 const float* bootstrap_value, const double* rewards, const int32_t* dones, float gamma, float clip_rho,
                 float clip_pg_rho, float* vs_out, float* pg_adv_out, double* stats_out, void* stream) {
    RL4RS_REQUIRE(T >= 1 && B >= 1, "vtrace: T = %d and B = %d must both be >= 1", T, B);
    RL4RS_REQUIRE(behaviour_logp && target_logp && values && rewards && vs_out && pg_adv_out, "vtrace: null argument");
    return launch_vtrace(T, B, behaviour_logp, target_logp, values, bootstrap_value, rewards, dones, gamma, clip_rho, clip_pg_rho, vs_out,
                         pg_adv_out, stats_out, 0, (hipStream_t)stream);
}

int rl4rs_policy_vtrace_loss_grad(rl4rs_policy* p, int32_t R, int32_t T, int32_t B, const float* obs_dev, const uint32_t* mask_bits_dev,
                                  const int32_t* actions_dev, const float* behaviour_logp_dev, const double* rewards_dev,
                                  const int32_t* dones_dev, float gamma, float clip_rho, float clip_pg_rho, int32_t drop_last,
                                  float vf_coeff, float ent_coeff, float* grad_dev, float* stats_dev, double* vtrace_stats_dev,
                                  float* vs_out, float* pg_adv_out, void* stream) {
    RL4RS_REQUIRE(p && obs_dev && actions_dev && behaviour_logp_dev && rewards_dev && grad_dev, "policy_vtrace_loss_grad: null argument");
    RL4RS_REQUIRE(R >= 1 && T >= 1 && B >= 1 && (int64_t)R * T * B <= (int64_t)p->max_rows,
                  "policy_vtrace_loss_grad: bad sizes (R=%d, T=%d, B=%d, max_rows=%d)", R, T, B, p->max_rows);
    RL4RS_REQUIRE(!(drop_last && T < 2), "policy_vtrace_loss_grad: drop_last needs T >= 2 (the dropped step's value is the bootstrap)");
    hipStream_t st = (hipStream_t)stream;
    const PolDims& d = p->d;
    const int N = R * T * B;
    const int Te = drop_last ? T - 1 : T;                  // steps the loss runs over
    const size_t per = (size_t)T * B, kept = (size_t)Te * B;
    const bool compact = drop_last && R > 1;
    int rc;
    if ((rc = vtrace_scratch(p, compact))) return rc;
    // 1. the learner's forward on every row (the dropped step's value is the bootstrap)
    if ((rc = rl4rs_policy_evaluate(p, N, obs_dev, mask_bits_dev, actions_dev, p->vt_logp, p->vt_val, nullptr, nullptr, stream))) return rc;
    // 2. V-trace per rollout; vs / pg_adv of the kept rows are written back to back ([R, Te, B])
    for (int r = 0; r < R; ++r) {
        const size_t o = r * per;
        if ((rc = launch_vtrace(Te, B, behaviour_logp_dev + o, p->vt_logp + o, p->vt_val + o, drop_last ? p->vt_val + o + kept : nullptr,
                                rewards_dev + o, dones_dev ? dones_dev + o : nullptr, gamma, clip_rho, clip_pg_rho, p->vt_vs + r * kept,
                                p->vt_pg + r * kept, vtrace_stats_dev, r > 0, st)))
            return rc;
    }
    if (vs_out || pg_adv_out) {                           // [R, T, B]; zeros on the rows of a dropped step
        for (float* out : {vs_out, pg_adv_out}) {
            if (!out) continue;
            const float* src = out == vs_out ? p->vt_vs : p->vt_pg;
            if (drop_last) RL4RS_HIP_TRY(hipMemsetAsync(out, 0, (size_t)N * 4, st));
            for (int r = 0; r < R; ++r) RL4RS_HIP_TRY(hipMemcpyAsync(out + r * per, src + r * kept, kept * 4, hipMemcpyDeviceToDevice, st));
        }
    }
    // 3. the A2C-form loss on the kept rows only: a dropped row takes no part in the gradient, the entropy sum or stats_dev.
    // One rollout's kept rows are a prefix of its buffers; those of several rollouts are copied together first.
    const float* obs_k = obs_dev;
    const uint32_t* mask_k = mask_bits_dev;
    const int32_t* act_k = actions_dev;
    if (compact) {
        for (int r = 0; r < R; ++r) {
            RL4RS_HIP_TRY(hipMemcpyAsync(p->vt_obs + r * kept * d.OD, obs_dev + r * per * d.OD, kept * d.OD * 4, hipMemcpyDeviceToDevice, st));
            RL4RS_HIP_TRY(hipMemcpyAsync(p->vt_act + r * kept, actions_dev + r * per, kept * 4, hipMemcpyDeviceToDevice, st));
            if (mask_bits_dev)
                RL4RS_HIP_TRY(hipMemcpyAsync(p->vt_mask + r * kept * d.W, mask_bits_dev + r * per * d.W, kept * d.W * 4, hipMemcpyDeviceToDevice, st));
        }
        obs_k = p->vt_obs; act_k = p->vt_act; mask_k = mask_bits_dev ? p->vt_mask : nullptr;
    }
    return rl4rs_policy_loss_grad(p, 0, (int32_t)(R * kept), obs_k, mask_k, act_k, p->vt_pg, p->vt_vs, nullptr, nullptr, nullptr, vf_coeff,
                                  ent_coeff, 0.f, 0.f, 0.f, grad_dev, stats_dev, stream);
}

}  // extern "C"
