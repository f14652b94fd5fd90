// On-device DQN for the action-masked FC net (include/rl4rs_hip.h, "On-device DQN"): a replay ring of whole rollouts with
// uniform / proportional-prioritized sampling, the (double-)Q Huber loss and its rank-sparse backward on rl4rs_policy, the masked
// greedy action, and an Adam step that clips every variable by its own norm.  The same ring stores the continuous actions of TD3 /
// DDPG (td3.hpp): rl4rs_replay_*_conti share the handle, the scans, the draw rule and k_replay_sample.  Compiled into policy.hip (uniform01, wave
// reductions, policy_row_forward, the fixed-order sample-axis reductions and the rl4rs_policy handle live there).
//
// Reference: script/modelfree_train.py:106-133 (algo "DQN": hiddens [], dueling False, double_q True, n_step 1,
// target_network_update_freq 200, buffer_size 100000, custom_model mask_model = rllib_mask_model.py:7-64).  With no extra hidden
// layer and no dueling head the Q values ARE the masked logits of the net.  RLlib 1.5.1's dqn_tf_policy / PrioritizedReplayBuffer
// are third-party and absent: restated from their published form, parity unpinned, checked against an fp64 restatement.
#pragma once

namespace rl4rs {

// ---------------------------------------------------------------------------------------------------------------------------
// Replay memory
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int PRIO_TILE = 1024;           // priorities per workgroup of the prefix scan: 256 threads x 4 consecutive values

// One pushed rollout's derived columns: reward float64 -> float32, done = last step of the rollout, priority = max_priority ^ alpha.
__global__ void k_replay_push(int rows, int B, int T, const double* __restrict__ rew, float* __restrict__ rew_out,
                              int32_t* __restrict__ done_out, double* __restrict__ prio_out, const double* __restrict__ max_prio,
                              double alpha) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    rew_out[i] = (float)rew[i];
    done_out[i] = (i / B == T - 1) ? 1 : 0;
    prio_out[i] = pow(max_prio[0], alpha);
}

// Inclusive float64 prefix sums of the priorities, fixed order.  Pass 1, per tile of 1024: every thread adds its 4 consecutive values
// in order, the 256 thread totals go through a Hillis-Steele scan in LDS; local[i] = (sum of the threads in front) + (own partial):
// the tile-local inclusive prefix.  tile_sum[t] = local of the tile's last element, tile_min[t] = its smallest priority.
__global__ __launch_bounds__(256) void k_prio_scan_tiles(const double* __restrict__ p, int n, double* __restrict__ local,
                                                         double* __restrict__ tile_sum, double* __restrict__ tile_min) {
    __shared__ double sm[2][256];
    __shared__ double mn[256];
    const int tid = threadIdx.x;
    const int base = blockIdx.x * PRIO_TILE + tid * 4;
    double s[4], run = 0.0, lo = INFINITY;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double v = (base + k < n) ? p[base + k] : 0.0;
        if (base + k < n) lo = fmin(lo, v);
        run += v;
        s[k] = run;
    }
    sm[0][tid] = run;
    mn[tid] = lo;
    __syncthreads();
    int cur = 0;
    for (int o = 1; o < 256; o <<= 1) {
        const double v = sm[cur][tid] + (tid >= o ? sm[cur][tid - o] : 0.0);
        sm[cur ^ 1][tid] = v;
        cur ^= 1;
        __syncthreads();
    }
    const double front = tid > 0 ? sm[cur][tid - 1] : 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (base + k < n) local[base + k] = front + s[k];
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) mn[tid] = fmin(mn[tid], mn[tid + o]);
        __syncthreads();
    }
    // the tile's sum is the local prefix of its LAST row, bit for bit (not the scan's own total, which associates differently): the
    // global prefix then never steps down across a tile boundary
    const int last = min(n, (int)(blockIdx.x + 1) * PRIO_TILE) - 1;
    if (last >= base && last < base + 4) tile_sum[blockIdx.x] = front + s[last - base];
    if (tid == 0) tile_min[blockIdx.x] = mn[0];
}

// Pass 2: tile_off[t] = sum of the tiles in front, in tile order (tile_off[nt] = total); tot[0] = total, tot[1] = smallest priority.
__global__ void k_prio_scan_offsets(const double* __restrict__ tile_sum, const double* __restrict__ tile_min, int nt,
                                    double* __restrict__ tile_off, double* __restrict__ tot) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double run = 0.0, lo = INFINITY;
    tile_off[0] = 0.0;
    for (int t = 0; t < nt; ++t) {
        run += tile_sum[t];
        lo = fmin(lo, tile_min[t]);
        tile_off[t + 1] = run;
    }
    tot[0] = run;
    tot[1] = lo;
}

struct ReplaySample {
    int M, n, B, OD, W, E, prioritized, vec4;      // E > 0: a ring of continuous actions (no mask words, no int32 action)
    double beta;
    uint32_t seed, step;
    const float* obs; const uint32_t* mask; const int32_t* act; const float* actf; const float* rew; const int32_t* done;
    const double* prio; const double* local; const double* tile_off; const double* tot;
    float* obs_out; float* next_obs_out; uint32_t* next_mask_out; int32_t* act_out; float* actf_out; float* rew_out; int32_t* done_out;
    int32_t* idx_out; float* w_out; float* u_out;
};

// One wave per draw: select a row, then gather it and its successor (row idx + B of the same rollout) into the minibatch.
// prefix(i) = tile_off[i / 1024] + local[i] is non-decreasing in i (both additions are monotone and tile_off[t + 1] is the prefix of
// tile t's last row), so two binary searches find the smallest i with prefix(i) > u * total.
__global__ __launch_bounds__(256) void k_replay_sample(ReplaySample a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + wave;
    if (m >= a.M) return;
    const float u = uniform01(a.seed, a.step, (uint32_t)m, 0u);
    int idx;
    float wgt = 1.f;
    if (!a.prioritized) {
        idx = (int)floor((double)u * (double)a.n);
    } else {
        const double total = a.tot[0], target = (double)u * total;
        const int nt = (a.n + PRIO_TILE - 1) / PRIO_TILE;
        int lo = 0, hi = nt - 1;                      // smallest tile whose last prefix exceeds the target
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (a.tile_off[mid + 1] > target) hi = mid; else lo = mid + 1;
        }
        const double off = a.tile_off[lo];
        int l2 = lo * PRIO_TILE, h2 = min(l2 + PRIO_TILE, a.n) - 1;
        while (l2 < h2) {
            const int mid = (l2 + h2) >> 1;
            if (off + a.local[mid] > target) h2 = mid; else l2 = mid + 1;
        }
        idx = l2;
    }
    idx = max(0, min(idx, a.n - 1));
    if (a.prioritized) {
        const double total = a.tot[0], nn = (double)a.n;
        wgt = (float)(pow(nn * a.prio[idx] / total, -a.beta) / pow(nn * a.tot[1] / total, -a.beta));
    }
    const int dn = a.done[idx];
    const int nxt = (dn || idx + a.B >= a.n) ? idx : idx + a.B;       // a terminal row has no successor: any finite row will do
    const float* so = a.obs + (size_t)idx * a.OD;
    const float* sn = a.obs + (size_t)nxt * a.OD;
    float* d_o = a.obs_out + (size_t)m * a.OD;
    float* d_n = a.next_obs_out + (size_t)m * a.OD;
    if (a.vec4) {
        typedef float f4 __attribute__((ext_vector_type(4)));
        for (int k = lane; k < a.OD / 4; k += 64) {
            const f4 x = reinterpret_cast<const f4*>(so)[k], y = reinterpret_cast<const f4*>(sn)[k];
            reinterpret_cast<f4*>(d_o)[k] = x;
            reinterpret_cast<f4*>(d_n)[k] = y;
        }
    } else {
        for (int k = lane; k < a.OD; k += 64) {
            const float x = so[k], y = sn[k];
            d_o[k] = x;
            d_n[k] = y;
        }
    }
    for (int k = lane; k < a.W; k += 64) a.next_mask_out[(size_t)m * a.W + k] = a.mask[(size_t)nxt * a.W + k];
    for (int k = lane; k < a.E; k += 64) a.actf_out[(size_t)m * a.E + k] = a.actf[(size_t)idx * a.E + k];
    if (lane == 0) {
        if (a.act) a.act_out[m] = a.act[idx];
        a.rew_out[m] = a.rew[idx];
        a.done_out[m] = dn;
        a.idx_out[m] = idx;
        if (a.w_out) a.w_out[m] = wgt;
        if (a.u_out) a.u_out[m] = u;
    }
}

// Priority update.  Rows that repeat inside one batch: the HIGHEST batch position wins, found with an integer atomicMax per row
// (order independent), so the result does not depend on which thread arrives first.  claim[] is -1 between calls.
__global__ void k_prio_claim(int M, int n, const int32_t* __restrict__ idx, int32_t* __restrict__ claim) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const int r = idx[i];
    if (r >= 0 && r < n) atomicMax(&claim[r], i);
}
__global__ void k_prio_write(int M, int n, const int32_t* __restrict__ idx, const float* __restrict__ td, int32_t* __restrict__ claim,
                             double* __restrict__ prio, double* __restrict__ max_prio, double alpha) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const int r = idx[i];
    if (r < 0 || r >= n) return;
    const double pr = fabs((double)td[i]) + 1e-6;
    const bool ok = pr < (double)INFINITY;            // a NaN / inf TD error leaves the row's priority alone
    // positive doubles order like their bit patterns: an integer max is the float64 max, in any arrival order
    if (ok) atomicMax(reinterpret_cast<unsigned long long*>(max_prio), (unsigned long long)__double_as_longlong(pr));
    if (claim[r] == i) {
        if (ok) prio[r] = pow(pr, alpha);
        claim[r] = -1;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Loss
// ---------------------------------------------------------------------------------------------------------------------------
struct DqnRows {
    PolDims d;
    int N, double_q;
    float gamma;
    const float* prm; const float* tprm;              // online / target parameters, same flat layout
    const float* obs; const float* next_obs; const uint32_t* next_mask;
    const int32_t* act; const float* rew; const int32_t* done; const float* w;
    // GEMM path: hidden rows of s (online), of s' (target), and the UNMASKED Q(s') rows of the net that picks a* (row stride ldq)
    const float* Hs; const float* Hnt; const float* Qn; int ldq;
    float* H; float* dHpre; float* g; float* td; int32_t* astar; float4* terms;
};

// first maximum of one row's masked values (q + max(log(mask), float32.min): q for an allowed action, q + -3.4028235e38 else), one
// wave; returns the action, *legal = does the row allow any action at all.  q may live in LDS or in memory.
__device__ __forceinline__ int masked_first_max(const float* q, const uint32_t* mrow, int A, int lane, bool add_mask, bool* legal) {
    float best = 0.f;
    int best_a = 0x7fffffff;
    bool any = mrow == nullptr;
    for (int a = lane; a < A; a += 64) {
        float v = q[a];
        const bool ok = mrow ? ((mrow[a >> 5] >> (a & 31)) & 1u) : true;
        any = any || ok;
        if (add_mask && !ok) v = v + (-3.4028235e38f);
        if (best_a == 0x7fffffff || v > best) { best = v; best_a = a; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const int oa = __shfl_xor(best_a, o);
        if (oa != 0x7fffffff && (best_a == 0x7fffffff || ob > best || (ob == best && oa < best_a))) { best = ob; best_a = oa; }
    }
    *legal = __any(any ? 1 : 0) != 0;
    return best_a;
}

// TD error, Huber loss and the one non-zero d loss / d Q of a row; lane-uniform inputs.  Writes the row's outputs from lane 0 and
// returns g = w * clip(td, -1, 1) / N.
__device__ __forceinline__ float dqn_row_finish(const DqnRows& a, int n, int lane, float qsa, float qt, bool boot, int astar) {
    const float r = a.rew[n];
    const float y = boot ? r + a.gamma * qt : r;      // a select: nothing of a terminal row's successor reaches y
    const float td = qsa - y, ad = fabsf(td);
    const float hub = ad < 1.f ? 0.5f * td * td : ad - 0.5f;
    const float wgt = a.w ? a.w[n] : 1.f;
    const float g = wgt * fminf(fmaxf(td, -1.f), 1.f) / (float)a.N;
    if (lane == 0) {
        a.g[n] = g;
        a.td[n] = td;
        if (a.astar) a.astar[n] = astar;
        a.terms[n] = make_float4(wgt * hub, qsa, y, ad);
    }
    return g;
}

// GEMM path: the three hidden layers and the Q(s') rows come from the MFMA GEMMs; one wave per row picks a*, takes the two
// single-column products Q(s)[a] and Q_target(s')[a*], and goes back to the hidden layer's pre-activation.
__global__ __launch_bounds__(256) void k_dqn_rows(DqnRows a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + wave;
    if (n >= a.N) return;
    const PolDims& d = a.d;
    const float* W2 = a.prm + (size_t)d.OD * d.HID + d.HID;
    const float* b2 = W2 + (size_t)d.HID * d.AE;
    const float* tW2 = a.tprm + (size_t)d.OD * d.HID + d.HID;
    const float* tb2 = tW2 + (size_t)d.HID * d.AE;
    const int act = max(0, min(a.act[n], d.A - 1));
    const bool done = a.done[n] != 0;
    int astar = -1;
    float qt = 0.f;
    bool boot = false;
    if (!done) {
        bool legal;
        astar = masked_first_max(a.Qn + (size_t)n * a.ldq, a.next_mask ? a.next_mask + (size_t)n * d.W : nullptr, d.A, lane, true, &legal);
        boot = legal;
        if (a.double_q) {
            float s = 0.f;
            for (int j = lane; j < d.HID; j += 64) s = fmaf(a.Hnt[(size_t)n * d.HID + j], tW2[(size_t)j * d.AE + astar], s);
            qt = wave_sum(s) + tb2[astar];
        } else {
            qt = a.Qn[(size_t)n * a.ldq + astar];
        }
    }
    float s = 0.f;
    for (int j = lane; j < d.HID; j += 64) s = fmaf(a.Hs[(size_t)n * d.HID + j], W2[(size_t)j * d.AE + act], s);
    const float qsa = wave_sum(s) + b2[act];
    const float g = dqn_row_finish(a, n, lane, qsa, qt, boot, astar);
    for (int j = lane; j < d.HID; j += 64) {
        const float h = a.Hs[(size_t)n * d.HID + j];
        a.dHpre[(size_t)n * d.HID + j] = g * W2[(size_t)j * d.AE + act] * (1.f - h * h);
    }
}

// Simple path (any shape rl4rs_policy_create admits): one wave per row runs the forwards it needs itself with scalar FMAs
// (policy_row_forward), nothing of a terminal row's successor is even read.
__global__ __launch_bounds__(256) void k_dqn_rows_simple(DqnRows a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const PolDims& d = a.d;
    const int per = d.OD + d.HID + d.AE;
    float* s_obs = reinterpret_cast<float*>(smem) + (size_t)wave * per;
    float* s_h = s_obs + d.OD;
    float* s_out = s_h + d.HID;
    const int n = blockIdx.x * 4 + wave;
    if (n >= a.N) return;
    const int act = max(0, min(a.act[n], d.A - 1));
    const bool done = a.done[n] != 0;
    int astar = -1;
    float qt = 0.f;
    bool boot = false;
    if (!done) {
        const float* xo = a.next_obs + (size_t)n * d.OD;
        const uint32_t* mrow = a.next_mask ? a.next_mask + (size_t)n * d.W : nullptr;
        bool legal;
        (void)policy_row_forward(d, a.double_q ? a.prm : a.tprm, xo, mrow, s_obs, s_h, s_out, lane);
        astar = masked_first_max(s_out, mrow, d.A, lane, false, &legal);       // s_out is masked already
        boot = legal;
        if (a.double_q) {
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            (void)policy_row_forward(d, a.tprm, xo, nullptr, s_obs, s_h, s_out, lane);
        }
        qt = s_out[astar];                  // (target picks a*: a masked value only where the row allows nothing, and then boot is off)
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    (void)policy_row_forward(d, a.prm, a.obs + (size_t)n * d.OD, nullptr, s_obs, s_h, s_out, lane);
    const float qsa = s_out[act];
    const float g = dqn_row_finish(a, n, lane, qsa, qt, boot, astar);
    const float* W2 = a.prm + (size_t)d.OD * d.HID + d.HID;
    for (int j = lane; j < d.HID; j += 64) {
        const float h = s_h[j];
        a.H[(size_t)n * d.HID + j] = h;
        a.dHpre[(size_t)n * d.HID + j] = g * W2[(size_t)j * d.AE + act] * (1.f - h * h);
    }
}

// dW2e[:, c] = sum over the rows n with action c of g[n] * H[n, :], db2e[c] = sum of their g[n]: one wave per output column walks the
// batch in row order (64 actions per ballot), so every column is a fixed-order sum and is written whole - columns nobody chose, the
// value head (column A) among them, get exactly 0.
__global__ __launch_bounds__(256) void k_dqn_w2_grad(int N, int HID, int A, int AE, const int32_t* __restrict__ act,
                                                     const float* __restrict__ g, const float* __restrict__ H,
                                                     float* __restrict__ gW2, float* __restrict__ gb2) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + wave;
    if (c >= AE) return;
    for (int j0 = 0; j0 < HID; j0 += 64) {
        const int j = j0 + lane;
        float acc = 0.f, bsum = 0.f;
        for (int n0 = 0; n0 < N; n0 += 64) {
            const int an = (n0 + lane < N) ? max(0, min(act[n0 + lane], A - 1)) : -1;
            unsigned long long m = __ballot(an == c);
            while (m) {
                const int n = n0 + __ffsll((long long)m) - 1;
                m &= m - 1;
                const float gn = g[n];
                bsum += gn;
                if (j < HID) acc = fmaf(gn, H[(size_t)n * HID + j], acc);
            }
        }
        if (j < HID) gW2[(size_t)j * AE + c] = acc;
        if (j0 == 0 && lane == 0) gb2[c] = bsum;
    }
}

// Greedy action: first maximum of the masked Q row (explore: False), optionally the masked row itself.
__global__ __launch_bounds__(256) void k_greedy_rows(int N, int A, int W, const float* __restrict__ q, int ldq,
                                                     const uint32_t* __restrict__ mask, int32_t* __restrict__ actions,
                                                     float* __restrict__ q_out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + wave;
    if (n >= N) return;
    const uint32_t* mrow = mask ? mask + (size_t)n * W : nullptr;
    bool legal;
    const int best = masked_first_max(q + (size_t)n * ldq, mrow, A, lane, true, &legal);
    if (q_out)
        for (int c = lane; c < A; c += 64) {
            float v = q[(size_t)n * ldq + c];
            if (mrow && !((mrow[c >> 5] >> (c & 31)) & 1u)) v = v + (-3.4028235e38f);
            q_out[(size_t)n * A + c] = v;
        }
    if (lane == 0) actions[n] = best;
}
__global__ __launch_bounds__(256) void k_greedy_simple(PolDims d, const float* __restrict__ prm, int N, const float* __restrict__ obs,
                                                       const uint32_t* __restrict__ mask, int32_t* __restrict__ actions,
                                                       float* __restrict__ q_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int per = d.OD + d.HID + d.AE;
    float* s_obs = reinterpret_cast<float*>(smem) + (size_t)wave * per;
    float* s_h = s_obs + d.OD;
    float* s_out = s_h + d.HID;
    const int n = blockIdx.x * 4 + wave;
    if (n >= N) return;
    const uint32_t* mrow = mask ? mask + (size_t)n * d.W : nullptr;
    (void)policy_row_forward(d, prm, obs + (size_t)n * d.OD, mrow, s_obs, s_h, s_out, lane);
    bool legal;
    const int best = masked_first_max(s_out, mrow, d.A, lane, false, &legal);
    if (q_out)
        for (int c = lane; c < d.A; c += 64) q_out[(size_t)n * d.A + c] = s_out[c];
    if (lane == 0) actions[n] = best;
}

}  // namespace rl4rs

struct rl4rs_replay {
    int OD, A, W, E, T, B, cap_rollouts, rows_per, cap_rows, n_tiles;      // E > 0: continuous actions float32 [E] (then A = W = 0)
    int64_t pushes;
    double alpha;
    float* obs; uint32_t* mask; int32_t* act; float* actf; float* rew; int32_t* done; double* prio;
    double* state;          // [0] max_priority, [1] total, [2] smallest priority (of the last prioritized sample)
    double *local, *tile_sum, *tile_min, *tile_off;
    int32_t* claim;
    std::vector<void*> owned;
};

// scratch of the DQN loss on a policy handle, allocated by the first call that needs it (A2C / PPO users never pay for it)
static int dqn_scratch(rl4rs_policy* p) {
    if (p->dqn_Hn) return RL4RS_OK;
    int rc;
    auto alloc = [&](float** dst, size_t n) {
        int r = dev_alloc(dst, n);
        if (r == RL4RS_OK) p->owned.push_back(*dst);
        return r;
    };
    if ((rc = alloc(&p->dqn_Hnt, (size_t)p->max_rows * p->d.HID))) return rc;
    if ((rc = alloc(&p->dqn_g, (size_t)p->max_rows))) return rc;
    if ((rc = alloc(&p->dqn_Hn, (size_t)p->max_rows * p->d.HID))) return rc;
    return RL4RS_OK;
}

extern "C" {

// one ring for both action kinds: action_size > 1 and act_dim = 0 (discrete: mask words + int32 action), or act_dim > 0 (continuous)
static int replay_create(int32_t obs_dim, int32_t action_size, int32_t act_dim, int32_t max_steps, int32_t batch_size, int64_t buffer_size,
                         double alpha, rl4rs_replay** out) {
    const int64_t per = (int64_t)max_steps * batch_size;
    const int64_t cap = std::max<int64_t>(1, buffer_size / per);
    RL4RS_REQUIRE(cap * per < ((int64_t)1 << 30), "replay_create: %lld rollouts of %lld rows exceed 2^30 rows", (long long)cap, (long long)per);
    if (rl4rs_device_count() <= 0) {
        set_error("no HIP device visible: librl4rs_hip has no CPU fallback");
        return RL4RS_EHIP;
    }
    rl4rs_replay* h = new rl4rs_replay();
    h->OD = obs_dim; h->A = action_size; h->W = (action_size + 31) / 32; h->E = act_dim; h->T = max_steps; h->B = batch_size;
    h->cap_rollouts = (int)cap; h->rows_per = (int)per; h->cap_rows = (int)(cap * per);
    h->n_tiles = (h->cap_rows + PRIO_TILE - 1) / PRIO_TILE;
    h->pushes = 0;
    h->alpha = alpha;
    h->mask = nullptr; h->act = nullptr; h->actf = nullptr;
    int rc = RL4RS_OK;
    auto alloc = [&](auto** dst, size_t n) {
        if (rc) return;
        rc = dev_alloc(dst, n);
        if (rc == RL4RS_OK) h->owned.push_back(*dst);
    };
    const size_t R = (size_t)h->cap_rows;
    alloc(&h->obs, R * obs_dim);
    if (act_dim > 0) {
        alloc(&h->actf, R * act_dim);
    } else {
        alloc(&h->mask, R * h->W);
        alloc(&h->act, R);
    }
    alloc(&h->rew, R);
    alloc(&h->done, R);
    alloc(&h->prio, R);
    alloc(&h->state, 4);
    alloc(&h->local, R);
    alloc(&h->tile_sum, (size_t)h->n_tiles);
    alloc(&h->tile_min, (size_t)h->n_tiles);
    alloc(&h->tile_off, (size_t)h->n_tiles + 1);
    alloc(&h->claim, R);
    if (rc) { rl4rs_replay_destroy(h); return rc; }
    const double st0[4] = {1.0, 0.0, 0.0, 0.0};
    hipError_t e = hipMemcpy(h->state, st0, sizeof(st0), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(h->claim, 0xff, R * 4);
    if (e != hipSuccess) {
        set_error("replay_create: initialisation failed: %s", hipGetErrorString(e));
        rl4rs_replay_destroy(h);
        return RL4RS_EHIP;
    }
    *out = h;
    return RL4RS_OK;
}

int rl4rs_replay_create(int32_t obs_dim, int32_t action_size, int32_t max_steps, int32_t batch_size, int64_t buffer_size, double alpha,
                        rl4rs_replay** out) {
    RL4RS_REQUIRE(out && obs_dim > 0 && action_size > 1 && max_steps > 0 && batch_size > 0 && buffer_size > 0 && alpha >= 0.0,
                  "replay_create: bad argument");
    return replay_create(obs_dim, action_size, 0, max_steps, batch_size, buffer_size, alpha, out);
}

int rl4rs_replay_create_conti(int32_t obs_dim, int32_t act_dim, int32_t max_steps, int32_t batch_size, int64_t buffer_size, double alpha,
                              rl4rs_replay** out) {
    RL4RS_REQUIRE(out && obs_dim > 0 && act_dim > 0 && max_steps > 0 && batch_size > 0 && buffer_size > 0 && alpha >= 0.0,
                  "replay_create_conti: bad argument");
    return replay_create(obs_dim, 0, act_dim, max_steps, batch_size, buffer_size, alpha, out);
}

int rl4rs_replay_destroy(rl4rs_replay* h) {
    if (!h) return RL4RS_OK;
    for (void* q : h->owned) (void)hipFree(q);
    delete h;
    return RL4RS_OK;
}

int rl4rs_replay_rows(rl4rs_replay* h, int32_t* rows, int32_t* capacity_rows, int64_t* pushes) {
    RL4RS_REQUIRE(h, "replay_rows: null handle");
    if (rows) *rows = (int32_t)(std::min<int64_t>(h->pushes, h->cap_rollouts) * h->rows_per);
    if (capacity_rows) *capacity_rows = h->cap_rows;
    if (pushes) *pushes = h->pushes;
    return RL4RS_OK;
}

int rl4rs_replay_buffer(rl4rs_replay* h, int32_t which, void** dev, int64_t* count) {
    RL4RS_REQUIRE(h && dev, "replay_buffer: null argument");
    const int64_t R = h->cap_rows;
    switch (which) {
        case RL4RS_REPLAY_BUF_OBS: *dev = h->obs; if (count) *count = R * h->OD; break;
        case RL4RS_REPLAY_BUF_MASK:
            RL4RS_REQUIRE(h->E == 0, "replay_buffer: a ring of continuous actions has no mask column");
            *dev = h->mask; if (count) *count = R * h->W; break;
        case RL4RS_REPLAY_BUF_ACTION:
            RL4RS_REQUIRE(h->E == 0, "replay_buffer: a ring of continuous actions has no int32 action column (RL4RS_REPLAY_BUF_ACTION_F32)");
            *dev = h->act; if (count) *count = R; break;
        case RL4RS_REPLAY_BUF_ACTION_F32:
            RL4RS_REQUIRE(h->E > 0, "replay_buffer: a ring of discrete actions has no float32 action column (RL4RS_REPLAY_BUF_ACTION)");
            *dev = h->actf; if (count) *count = R * h->E; break;
        case RL4RS_REPLAY_BUF_REWARD: *dev = h->rew; if (count) *count = R; break;
        case RL4RS_REPLAY_BUF_DONE: *dev = h->done; if (count) *count = R; break;
        case RL4RS_REPLAY_BUF_PRIORITY: *dev = h->prio; if (count) *count = R; break;
        case RL4RS_REPLAY_BUF_MAX_PRIORITY: *dev = h->state; if (count) *count = 1; break;
        default: set_error("replay_buffer: unknown buffer %d", which); return RL4RS_EINVAL;
    }
    return RL4RS_OK;
}

// shared by the two action kinds: the rollout's columns into the slot, derived columns by k_replay_push
static int replay_push(rl4rs_replay* h, const float* obs_dev, const uint32_t* mask_dev, const int32_t* action_dev, const float* actf_dev,
                       const double* reward_dev, hipStream_t st) {
    const size_t slot = (size_t)(h->pushes % h->cap_rollouts), r0 = slot * h->rows_per, R = (size_t)h->rows_per;
    RL4RS_HIP_TRY(hipMemcpyAsync(h->obs + r0 * h->OD, obs_dev, R * h->OD * 4, hipMemcpyDeviceToDevice, st));
    if (h->E > 0) {
        RL4RS_HIP_TRY(hipMemcpyAsync(h->actf + r0 * h->E, actf_dev, R * h->E * 4, hipMemcpyDeviceToDevice, st));
    } else {
        RL4RS_HIP_TRY(hipMemcpyAsync(h->mask + r0 * h->W, mask_dev, R * h->W * 4, hipMemcpyDeviceToDevice, st));
        RL4RS_HIP_TRY(hipMemcpyAsync(h->act + r0, action_dev, R * 4, hipMemcpyDeviceToDevice, st));
    }
    hipLaunchKernelGGL(k_replay_push, dim3((h->rows_per + 255) / 256), dim3(256), 0, st, h->rows_per, h->B, h->T, reward_dev,
                       h->rew + r0, h->done + r0, h->prio + r0, h->state, h->alpha);
    RL4RS_LAUNCH_CHECK();
    h->pushes += 1;
    return RL4RS_OK;
}

int rl4rs_replay_push(rl4rs_replay* h, const float* obs_dev, const uint32_t* mask_dev, const int32_t* action_dev,
                      const double* reward_dev, void* stream) {
    RL4RS_REQUIRE(h && obs_dev && mask_dev && action_dev && reward_dev, "replay_push: null argument");
    RL4RS_REQUIRE(h->E == 0, "replay_push: this ring stores continuous actions (rl4rs_replay_push_conti)");
    return replay_push(h, obs_dev, mask_dev, action_dev, nullptr, reward_dev, (hipStream_t)stream);
}

int rl4rs_replay_push_conti(rl4rs_replay* h, const float* obs_dev, const float* action_dev, const double* reward_dev, void* stream) {
    RL4RS_REQUIRE(h && obs_dev && action_dev && reward_dev, "replay_push_conti: null argument");
    RL4RS_REQUIRE(h->E > 0, "replay_push_conti: this ring stores discrete actions (rl4rs_replay_push)");
    return replay_push(h, obs_dev, nullptr, nullptr, action_dev, reward_dev, (hipStream_t)stream);
}

static int replay_sample(rl4rs_replay* h, int32_t M, int32_t prioritized, double beta, uint32_t seed, uint32_t step, float* obs_out,
                         float* next_obs_out, uint32_t* next_mask_out, int32_t* action_out, float* actf_out, float* reward_out,
                         int32_t* done_out, int32_t* idx_out, float* weight_out, float* u_out, hipStream_t st) {
    RL4RS_REQUIRE(h->pushes > 0, "replay_sample: the memory is empty");
    const int n = (int)(std::min<int64_t>(h->pushes, h->cap_rollouts) * h->rows_per);
    if (prioritized) {
        const int nt = (n + PRIO_TILE - 1) / PRIO_TILE;
        hipLaunchKernelGGL(k_prio_scan_tiles, dim3(nt), dim3(256), 0, st, h->prio, n, h->local, h->tile_sum, h->tile_min);
        hipLaunchKernelGGL(k_prio_scan_offsets, dim3(1), dim3(64), 0, st, h->tile_sum, h->tile_min, nt, h->tile_off, h->state + 1);
        RL4RS_LAUNCH_CHECK();
    }
    ReplaySample a;
    a.M = M; a.n = n; a.B = h->B; a.OD = h->OD; a.W = h->W; a.E = h->E; a.prioritized = prioritized ? 1 : 0;
    a.vec4 = (h->OD % 4 == 0 && ((reinterpret_cast<uintptr_t>(obs_out) | reinterpret_cast<uintptr_t>(next_obs_out)) & 15) == 0) ? 1 : 0;
    a.beta = beta; a.seed = seed; a.step = step;
    a.obs = h->obs; a.mask = h->mask; a.act = h->act; a.actf = h->actf; a.rew = h->rew; a.done = h->done;
    a.prio = h->prio; a.local = h->local; a.tile_off = h->tile_off; a.tot = h->state + 1;
    a.obs_out = obs_out; a.next_obs_out = next_obs_out; a.next_mask_out = next_mask_out; a.act_out = action_out; a.actf_out = actf_out;
    a.rew_out = reward_out; a.done_out = done_out; a.idx_out = idx_out; a.w_out = weight_out; a.u_out = u_out;
    hipLaunchKernelGGL(k_replay_sample, dim3((M + 3) / 4), dim3(256), 0, st, a);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

int rl4rs_replay_sample(rl4rs_replay* h, int32_t M, int32_t prioritized, double beta, uint32_t seed, uint32_t step, float* obs_out,
                        float* next_obs_out, uint32_t* next_mask_out, int32_t* action_out, float* reward_out, int32_t* done_out,
                        int32_t* idx_out, float* weight_out, float* u_out, void* stream) {
    RL4RS_REQUIRE(h && M > 0 && obs_out && next_obs_out && next_mask_out && action_out && reward_out && done_out && idx_out,
                  "replay_sample: bad argument");
    RL4RS_REQUIRE(h->E == 0, "replay_sample: this ring stores continuous actions (rl4rs_replay_sample_conti)");
    return replay_sample(h, M, prioritized, beta, seed, step, obs_out, next_obs_out, next_mask_out, action_out, nullptr, reward_out, done_out,
                         idx_out, weight_out, u_out, (hipStream_t)stream);
}

int rl4rs_replay_sample_conti(rl4rs_replay* h, int32_t M, int32_t prioritized, double beta, uint32_t seed, uint32_t step, float* obs_out,
                              float* next_obs_out, float* action_out, float* reward_out, int32_t* done_out, int32_t* idx_out,
                              float* weight_out, float* u_out, void* stream) {
    RL4RS_REQUIRE(h && M > 0 && obs_out && next_obs_out && action_out && reward_out && done_out && idx_out, "replay_sample_conti: bad argument");
    RL4RS_REQUIRE(h->E > 0, "replay_sample_conti: this ring stores discrete actions (rl4rs_replay_sample)");
    return replay_sample(h, M, prioritized, beta, seed, step, obs_out, next_obs_out, nullptr, nullptr, action_out, reward_out, done_out,
                         idx_out, weight_out, u_out, (hipStream_t)stream);
}

int rl4rs_replay_update_priorities(rl4rs_replay* h, int32_t M, const int32_t* idx_dev, const float* td_dev, void* stream) {
    RL4RS_REQUIRE(h && M > 0 && idx_dev && td_dev, "replay_update_priorities: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const int n = (int)(std::min<int64_t>(h->pushes, h->cap_rollouts) * h->rows_per);
    hipLaunchKernelGGL(k_prio_claim, dim3((M + 255) / 256), dim3(256), 0, st, M, n, idx_dev, h->claim);
    hipLaunchKernelGGL(k_prio_write, dim3((M + 255) / 256), dim3(256), 0, st, M, n, idx_dev, td_dev, h->claim, h->prio, h->state, h->alpha);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

int rl4rs_policy_dqn_loss_grad(rl4rs_policy* p, const float* target_params_dev, int32_t N, const float* obs, const int32_t* actions,
                               const float* rewards, const int32_t* dones, const float* next_obs, const uint32_t* next_mask_bits,
                               const float* weights, float gamma, int32_t double_q, float* grad_dev, float* td_dev, int32_t* next_action_dev,
                               float* stats_dev, void* stream) {
    RL4RS_REQUIRE(p && target_params_dev && obs && actions && rewards && dones && next_obs && grad_dev && td_dev && N > 0 &&
                  N <= p->max_rows, "policy_dqn_loss_grad: bad argument (N=%d, max_rows=%d)", N, p ? p->max_rows : -1);
    hipStream_t st = (hipStream_t)stream;
    const PolDims& d = p->d;
    int rc = dqn_scratch(p);
    if (rc) return rc;
    DqnRows a;
    memset(&a, 0, sizeof(a));
    a.d = d; a.N = N; a.double_q = double_q ? 1 : 0; a.gamma = gamma;
    a.prm = p->opt.params; a.tprm = target_params_dev;
    a.obs = obs; a.next_obs = next_obs; a.next_mask = next_mask_bits; a.act = actions; a.rew = rewards; a.done = dones; a.w = weights;
    a.H = p->H; a.dHpre = p->dHpre; a.g = p->dqn_g; a.td = td_dev; a.astar = next_action_dev; a.terms = p->terms;
    const float* W1 = p->opt.params;
    const float* b1 = W1 + (size_t)d.OD * d.HID;
    const float* W2 = b1 + d.HID;
    const float* b2 = W2 + (size_t)d.HID * d.AE;
    const float* tW1 = target_params_dev;
    const float* tb1 = tW1 + (size_t)d.OD * d.HID;
    const float* tW2 = tb1 + d.HID;
    const float* tb2 = tW2 + (size_t)d.HID * d.AE;
    if (p->opt_tile) {
        // hidden rows on the matrix cores: s through the online layer 1, s' through the target's and (double-Q) the online one;
        // then the full Q(s') rows of the net that picks a* (A columns: the value head is not a Q value).  p->dOut holds them.
        if ((rc = launch_gemm_f32(obs, d.OD, W1, d.HID, b1, p->H, d.HID, N, d.HID, d.OD, ACT_TANH, st))) return rc;
        if ((rc = launch_gemm_f32(next_obs, d.OD, tW1, d.HID, tb1, p->dqn_Hnt, d.HID, N, d.HID, d.OD, ACT_TANH, st))) return rc;
        if (double_q) {
            if ((rc = launch_gemm_f32(next_obs, d.OD, W1, d.HID, b1, p->dqn_Hn, d.HID, N, d.HID, d.OD, ACT_TANH, st))) return rc;
            if ((rc = launch_gemm_f32(p->dqn_Hn, d.HID, W2, d.AE, b2, p->dOut, d.AE, N, d.A, d.HID, ACT_NONE, st))) return rc;
        } else {
            if ((rc = launch_gemm_f32(p->dqn_Hnt, d.HID, tW2, d.AE, tb2, p->dOut, d.AE, N, d.A, d.HID, ACT_NONE, st))) return rc;
        }
        a.Hs = p->H; a.Hnt = p->dqn_Hnt; a.Qn = p->dOut; a.ldq = d.AE;
        hipLaunchKernelGGL(k_dqn_rows, dim3((N + 3) / 4), dim3(256), 0, st, a);
    } else {
        const size_t smem = fwd_smem(d, 0);
        if ((rc = raise_dyn_smem(reinterpret_cast<const void*>(&k_dqn_rows_simple), smem))) return rc;
        hipLaunchKernelGGL(k_dqn_rows_simple, dim3((N + 3) / 4), dim3(256), smem, st, a);
    }
    RL4RS_LAUNCH_CHECK();
    // parameter gradients: W1 / b1 as in rl4rs_policy_loss_grad (fixed chunks of the sample axis, summed in chunk order), W2e / b2e
    // column by column from the one non-zero d loss / d Q of every row
    int chunk = p->chunk;
    if ((N + chunk - 1) / chunk > 64) chunk = (((N + 63) / 64) + 63) / 64 * 64;
    const int nz = (N + chunk - 1) / chunk;
    float* gW1 = grad_dev;
    float* gb1 = gW1 + (size_t)d.OD * d.HID;
    float* gW2 = gb1 + d.HID;
    float* gb2 = gW2 + (size_t)d.HID * d.AE;
    {
        const int tiles = ((d.OD + 31) / 32) * ((d.HID + 31) / 32);
        hipLaunchKernelGGL(k_gemm_tn, dim3((tiles + 3) / 4, nz), dim3(256), 0, st, obs, d.OD, d.OD, p->dHpre, d.HID, d.HID, N, chunk,
                           nz == 1 ? gW1 : p->part, (float*)nullptr);
        if (nz > 1) hipLaunchKernelGGL(k_reduce_chunks, dim3((d.OD * d.HID + 255) / 256), dim3(256), 0, st, p->part, d.OD * d.HID, nz, gW1);
        hipLaunchKernelGGL(k_colsum, dim3((d.HID + 63) / 64, nz), dim3(64), 0, st, p->dHpre, d.HID, d.HID, N, chunk, nz == 1 ? gb1 : p->part);
        if (nz > 1) hipLaunchKernelGGL(k_reduce_chunks, dim3((d.HID + 255) / 256), dim3(256), 0, st, p->part, d.HID, nz, gb1);
    }
    hipLaunchKernelGGL(k_dqn_w2_grad, dim3((d.AE + 3) / 4), dim3(256), 0, st, N, d.HID, d.A, d.AE, actions, p->dqn_g, p->H, gW2, gb2);
    RL4RS_LAUNCH_CHECK();
    if (stats_dev) {
        hipLaunchKernelGGL(k_reduce_terms, dim3(1), dim3(256), 0, st, p->terms, N, stats_dev);
        RL4RS_LAUNCH_CHECK();
    }
    return RL4RS_OK;
}

int rl4rs_policy_greedy(rl4rs_policy* p, int32_t N, const float* obs, const uint32_t* mask_bits, int32_t* actions, float* q_out,
                        void* stream) {
    RL4RS_REQUIRE(p && obs && actions && N > 0, "policy_greedy: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const PolDims& d = p->d;
    if (p->opt_tile && N <= p->max_rows) {
        const float* W1 = p->opt.params;
        const float* b1 = W1 + (size_t)d.OD * d.HID;
        const float* W2 = b1 + d.HID;
        const float* b2 = W2 + (size_t)d.HID * d.AE;
        int rc;
        if ((rc = launch_gemm_f32(obs, d.OD, W1, d.HID, b1, p->H, d.HID, N, d.HID, d.OD, ACT_TANH, st))) return rc;
        if ((rc = launch_gemm_f32(p->H, d.HID, W2, d.AE, b2, p->dOut, d.AE, N, d.A, d.HID, ACT_NONE, st))) return rc;
        hipLaunchKernelGGL(k_greedy_rows, dim3((N + 3) / 4), dim3(256), 0, st, N, d.A, d.W, p->dOut, d.AE, mask_bits, actions, q_out);
    } else {
        const size_t smem = fwd_smem(d, 0);
        int rc = raise_dyn_smem(reinterpret_cast<const void*>(&k_greedy_simple), smem);
        if (rc) return rc;
        hipLaunchKernelGGL(k_greedy_simple, dim3((N + 3) / 4), dim3(256), smem, st, d, p->opt.params, N, obs, mask_bits, actions, q_out);
    }
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

int rl4rs_policy_ope_step(rl4rs_policy* p, int32_t N, const float* obs, const uint32_t* mask_bits, const int32_t* logged, int32_t q_mode,
                          int32_t* actions, double* pi, double* q, float* masked_out, void* stream) {
    RL4RS_REQUIRE(p && obs && actions && N > 0, "policy_ope_step: bad argument");
    RL4RS_REQUIRE(q_mode == 0 || q_mode == 1, "policy_ope_step: q_mode %d is neither 0 (value head) nor 1 (masked Q)", q_mode);
    RL4RS_REQUIRE(N <= p->max_rows, "policy_ope_step: %d rows exceed the handle's max_rows %d", N, p->max_rows);
    hipStream_t st = (hipStream_t)stream;
    const PolDims& d = p->d;
    const float* W1 = p->opt.params;
    const float* b1 = W1 + (size_t)d.OD * d.HID;
    const float* W2 = b1 + d.HID;
    const float* b2 = W2 + (size_t)d.HID * d.AE;
    int rc;
    if ((rc = launch_gemm_f32(obs, d.OD, W1, d.HID, b1, p->H, d.HID, N, d.HID, d.OD, ACT_TANH, st))) return rc;
    if ((rc = launch_gemm_f32(p->H, d.HID, W2, d.AE, b2, p->dOut, d.AE, N, q_mode ? d.A : d.AE, d.HID, ACT_NONE, st))) return rc;
    return rl4rs_ope_greedy_rows(N, p->dOut, d.A, d.AE, mask_bits, 0, logged, q_mode ? nullptr : p->dOut + d.A, d.AE, actions, pi, q,
                                 masked_out, stream);
}

int rl4rs_policy_adam_step_clip_by_var(rl4rs_policy* p, const float* grad_dev, float lr, float beta1, float beta2, float eps,
                                       float var_clip, void* stream) {
    RL4RS_REQUIRE(p && grad_dev, "policy_adam_step_clip_by_var: null argument");
    hipStream_t st = (hipStream_t)stream;
    const PolDims& d = p->d;
    VarSegs sg;
    sg.end[0] = d.OD * d.HID;
    sg.end[1] = sg.end[0] + d.HID;
    sg.end[2] = sg.end[1] + d.HID * d.AE;
    sg.end[3] = sg.end[2] + d.AE;
    const float lr_t = adam_advance(p->opt, ADAM_TF, lr, beta1, beta2, eps).lr_t;
    if (var_clip > 0.f) hipLaunchKernelGGL(k_sumsq_vars, dim3(4), dim3(256), 0, st, grad_dev, sg, p->sumsq);
    hipLaunchKernelGGL(k_adam_vars, dim3((p->opt.n + 255) / 256), dim3(256), 0, st, p->opt.params, grad_dev, p->opt.m, p->opt.v,
                       p->opt.n, sg, lr_t, beta1, beta2, eps, p->sumsq, var_clip);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

}  // extern "C"
