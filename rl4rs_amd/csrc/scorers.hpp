// Offline scorers on the device (include/rl4rs_hip.h, "Offline scorers"): d3rlpy 0.91's metrics/scorer.py and the
// reference's rl4rs/utils/d3rlpy_scorer.py over evaluation episodes, as ONE pass.
//
//   k_score_rows      a wave per score row, four rows per workgroup (the shape of k_ope_greedy_rows): the row - and the imitator's,
//                     for the BCQ rule - is staged into the wave's share of LDS, so memory is read once; from LDS come
//                     qd = row[logged], a_pi = q_best_action (qlearn.hpp: the learners' own greedy rule, called, not restated),
//                     qp = row[a_pi] and a_mask = the predict_with_mask rule of env.hip (k_predict_with_mask) under the catalogue
//                     tables of an rl4rs_env, its observation tail converted by truncation like DeviceEnv.predict_with_mask.
//   k_score_diff      continuous actions: diff = sum_k (a_k - pi(o)_k)^2 per row, float64.
//   k_score_episodes  a lane per episode of any length: return, success flag, first-row value, the squared TD errors, the
//                     backward scan of the advantages with its restart every SCORE_WINDOW rows, the matches - all float64 - then
//                     lane -> wave (shuffle tree) -> block (LDS, wave order) partials.
//   k_score_fold      one thread per sum adds the block partials in block order.  No float atomics anywhere: two runs give the same
//                     bytes, and a one-name call gives the bytes of its slot of an all-names call.
// The kernels carry no scaler arithmetic: r_td / qd arrive transformed where the learner has a reward scaler.
#pragma once

#include <limits>

namespace rl4rs {

constexpr int SCORE_WINDOW = 1024;                // d3rlpy's WINDOW_SIZE: _make_batches cuts an episode into windows of this many rows
constexpr int SCORE_ROW_LDS_FLOATS = 4096;        // per wave: 4 waves x 16 KB = the 64 KB a workgroup gets without asking
constexpr int SCORE_BLOCK = 256;
constexpr int SCORE_WAVES = SCORE_BLOCK / 64;
enum { SS_TD, SS_DSA, SS_QP, SS_QP0, SS_QD, SS_QDS, SS_NS, SS_MPI, SS_MMASK, SS_DIFF, SS_N, SS_K };

struct ScoreRowsIn {
    int N, A;
    const float* scores; int64_t ld;
    const float* imit; int64_t imit_ld; float log_flex;
    const int32_t* logged;
    const float* obs; int64_t obs_ld; int obs_dim;         // the mask rule's tail: the last P + 1 columns of an observation row
    int use_mask; EnvMaskTables tab;
    float* qd; int32_t* a_pi; float* qp; int32_t* a_mask;
};

template <bool STAGED>
__global__ __launch_bounds__(SCORE_BLOCK) void k_score_rows(ScoreRowsIn in) {
    extern __shared__ __attribute__((aligned(16))) float score_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.x * SCORE_WAVES + wave;
    if (n >= in.N) return;                           // whole waves leave together: everything below is wave-local
    const int A = in.A;
    const float* q = in.scores + (int64_t)n * in.ld;
    const float* im = in.imit ? in.imit + (int64_t)n * in.imit_ld : nullptr;
    if (STAGED) {
        float* s = score_lds + (size_t)wave * (in.imit ? 2 : 1) * A;
        for (int c = lane; c < A; c += 64) s[c] = q[c];
        if (im)
            for (int c = lane; c < A; c += 64) s[A + c] = im[c];
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        q = s;
        if (im) im = s + A;
    }
    const int a_pi = q_best_action(q, im, A, lane, in.log_flex);
    int a_mask = 0;
    if (in.use_mask) {
        // k_predict_with_mask (env.hip), on this row: mask = location_mask[cur_step % P // 3] without the previous actions; a
        // forbidden score = -2^15; once a special item was chosen every special item = -2^15; first maximum
        const int P = in.tab.P;
        const float* tail = in.obs + (int64_t)n * in.obs_ld + in.obs_dim - (P + 1);
        int layer = ((int)tail[P] % P) / 3;
        layer = layer < 0 ? 0 : (layer > 3 ? 3 : layer);          // (the table has four rows)
        bool sp = false;
        for (int j = lane; j < P; j += 64) {
            const int id = (int)tail[j];
            if (id >= 0 && id < A) sp |= in.tab.is_special[id] != 0;
        }
        const bool any_special = __any(sp);
        float best = 0.f;
        int best_k = 0x7fffffff;
        for (int k = lane; k < A; k += 64) {
            bool ok = (in.tab.loc_bits[layer * in.tab.W + (k >> 5)] >> (k & 31)) & 1u;
            for (int j = 0; j < P; ++j) ok = ok && ((int)tail[j] != k);
            float s = q[k];
            if (!ok) s = -32768.0f;
            if (any_special && in.tab.is_special[k]) s = -32768.0f;
            if (best_k == 0x7fffffff || s > best) { best = s; best_k = k; }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float os = __shfl_xor(best, off);
            const int ok = __shfl_xor(best_k, off);
            if (ok != 0x7fffffff && (best_k == 0x7fffffff || os > best || (os == best && ok < best_k))) { best = os; best_k = ok; }
        }
        a_mask = best_k;
    }
    if (lane == 0) {
        if (in.a_pi) in.a_pi[n] = a_pi;
        if (in.qp) in.qp[n] = q[a_pi];
        if (in.qd) {
            const int l = in.logged[n];
            in.qd[n] = (l >= 0 && l < A) ? q[l] : __int_as_float(0x7fc00000);
        }
        if (in.a_mask) in.a_mask[n] = a_mask;
    }
}

__global__ void k_score_diff(int N, int E, const float* __restrict__ a, const float* __restrict__ p, double* __restrict__ out) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double s = 0.0;
    for (int k = 0; k < E; ++k) {
        const double d = (double)a[(int64_t)n * E + k] - (double)p[(int64_t)n * E + k];
        s += d * d;
    }
    out[n] = s;
}

struct ScoreEpIn {
    const int64_t* starts; int E; int64_t rows;
    rl4rs_score_cols c;
    double gamma, thr; int has_thr;
};

__device__ __forceinline__ double score_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__global__ __launch_bounds__(SCORE_BLOCK) void k_score_episodes(ScoreEpIn in, double* __restrict__ part) {
    __shared__ double lds[SS_K * SCORE_WAVES];
    const int e = blockIdx.x * SCORE_BLOCK + threadIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const rl4rs_score_cols& c = in.c;
    double v[SS_K];
#pragma unroll
    for (int k = 0; k < SS_K; ++k) v[k] = 0.0;
    if (e < in.E) {
        int64_t s = in.starts[e], t = in.starts[e + 1];
        s = s < 0 ? 0 : (s > in.rows ? in.rows : s);             // (offsets are the caller's: never walk outside the columns)
        t = t < s ? s : (t > in.rows ? in.rows : t);
        double ret = 0.0, td = 0.0, qp = 0.0, qd = 0.0, mpi = 0.0, mmask = 0.0, diff = 0.0;
        for (int64_t i = s; i < t; ++i) {
            const double qdi = c.qd ? (double)c.qd[i] : nan;
            ret += c.r_raw ? (double)c.r_raw[i] : nan;
            const double y = (c.r_td ? (double)c.r_td[i] : nan) + in.gamma * (c.qn ? (double)c.qn[i] : nan) * (1.0 - (c.ter ? (double)c.ter[i] : nan));
            td += (qdi - y) * (qdi - y);
            qp += c.qp ? (double)c.qp[i] : nan;
            qd += qdi;
            if (c.a && c.a_pi) mpi += c.a[i] == c.a_pi[i] ? 1.0 : 0.0;
            if (c.a && c.a_mask) mmask += c.a[i] == c.a_mask[i] ? 1.0 : 0.0;
            diff += c.diff ? c.diff[i] : nan;
        }
        // discounted sum of advantages: inside each window of SCORE_WINDOW rows of the episode, S_last = adv_last, S_j = adv_j + gamma S_{j+1}
        double dsa = 0.0, S = 0.0;
        for (int64_t i = t - 1; i >= s; --i) {
            const double adv = (c.qd ? (double)c.qd[i] : nan) - (c.qp ? (double)c.qp[i] : nan);
            const bool last = i == t - 1 || ((i - s) % SCORE_WINDOW) == SCORE_WINDOW - 1;
            S = last ? adv : adv + in.gamma * S;
            dsa += S;
        }
        const bool success = in.has_thr && ret >= in.thr;
        v[SS_TD] = td; v[SS_DSA] = dsa; v[SS_QP] = qp; v[SS_QD] = qd;
        v[SS_QP0] = t > s ? (c.qp ? (double)c.qp[s] : nan) : 0.0;
        v[SS_QDS] = success ? qd : 0.0;
        v[SS_NS] = success ? (double)(t - s) : 0.0;
        v[SS_MPI] = mpi; v[SS_MMASK] = mmask; v[SS_DIFF] = diff;
        v[SS_N] = (double)(t - s);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < SS_K; ++k) {
        const double s = score_wave_sum(v[k]);
        if (lane == 0) lds[k * SCORE_WAVES + wave] = s;
    }
    __syncthreads();
    if (threadIdx.x < SS_K) {
        double s = lds[threadIdx.x * SCORE_WAVES];
        for (int w = 1; w < SCORE_WAVES; ++w) s += lds[threadIdx.x * SCORE_WAVES + w];
        part[(int64_t)blockIdx.x * SS_K + threadIdx.x] = s;
    }
}

__global__ void k_score_fold(const double* __restrict__ part, int nblocks, double* __restrict__ sums) {
    const int k = threadIdx.x;
    if (k >= SS_K) return;
    double s = 0.0;
    for (int j = 0; j < nblocks; ++j) s += part[(int64_t)j * SS_K + k];
    sums[k] = s;
}

}  // namespace rl4rs

extern "C" {

int rl4rs_score_rows(int32_t N, const float* scores_dev, int32_t A, int64_t ld, const float* imitator_dev, int64_t imitator_ld,
                     float action_flexibility, const int32_t* logged_dev, const rl4rs_env* env, const float* obs_dev, int32_t obs_dim,
                     int64_t obs_ld, float* qd_dev, int32_t* a_pi_dev, float* qp_dev, int32_t* a_mask_dev, void* stream) {
    RL4RS_REQUIRE(N >= 1 && scores_dev && A >= 1 && ld >= A, "score_rows: bad scores (N %d, A %d, ld %lld)", N, A, (long long)ld);
    RL4RS_REQUIRE(!imitator_dev || (imitator_ld >= A && action_flexibility > 0.f), "score_rows: bad imitator rows (ld %lld, action_flexibility %g)",
                  (long long)imitator_ld, (double)action_flexibility);
    RL4RS_REQUIRE(!qd_dev || logged_dev, "score_rows: qd needs the logged actions");
    RL4RS_REQUIRE(!a_mask_dev || (env && obs_dev), "score_rows: a_mask needs the env's catalogue tables and the observation rows");
    ScoreRowsIn in = {};
    in.N = N; in.A = A;
    in.scores = scores_dev; in.ld = ld;
    in.imit = imitator_dev; in.imit_ld = imitator_ld;
    in.log_flex = imitator_dev ? logf(action_flexibility) : 0.f;
    in.logged = logged_dev;
    in.qd = qd_dev; in.a_pi = a_pi_dev; in.qp = qp_dev; in.a_mask = a_mask_dev;
    if (a_mask_dev) {
        int rc = env_mask_tables(env, &in.tab);
        if (rc) return rc;
        RL4RS_REQUIRE(in.tab.A == A, "score_rows: %d score columns, the env's catalogue has %d items", A, in.tab.A);
        RL4RS_REQUIRE(in.tab.P >= 1 && obs_dim >= in.tab.P + 1 && obs_ld >= obs_dim, "score_rows: observation rows of %d columns (stride %lld) hold no tail of %d",
                      obs_dim, (long long)obs_ld, in.tab.P + 1);
        in.use_mask = 1;
        in.obs = obs_dev; in.obs_ld = obs_ld; in.obs_dim = obs_dim;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(ceil_div(N, SCORE_WAVES)), block(SCORE_BLOCK);
    const int per_wave = (imitator_dev ? 2 : 1) * A;
    if (per_wave <= SCORE_ROW_LDS_FLOATS)
        hipLaunchKernelGGL(k_score_rows<true>, grid, block, (size_t)SCORE_WAVES * per_wave * sizeof(float), st, in);
    else
        hipLaunchKernelGGL(k_score_rows<false>, grid, block, 0, st, in);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

int rl4rs_score_action_diff(int32_t N, int32_t E, const float* actions_dev, const float* predicted_dev, double* diff_dev, void* stream) {
    RL4RS_REQUIRE(N >= 1 && E >= 1 && actions_dev && predicted_dev && diff_dev, "score_action_diff: bad argument (N %d, E %d)", N, E);
    hipLaunchKernelGGL(k_score_diff, dim3(ceil_div(N, 256)), dim3(256), 0, (hipStream_t)stream, N, E, actions_dev, predicted_dev, diff_dev);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

int rl4rs_score_episodes(int32_t E, const int64_t* starts_dev, int64_t rows, const rl4rs_score_cols* cols, double gamma, int32_t has_threshold,
                         double threshold, double* stats_host, void* stream) {
    RL4RS_REQUIRE(E >= 1 && starts_dev && rows >= 1 && cols && stats_host, "score_episodes: bad argument (E %d, rows %lld)", E, (long long)rows);
    if (rl4rs_device_count() <= 0) {
        set_error("no HIP device visible: librl4rs_hip has no CPU fallback");
        return RL4RS_EHIP;
    }
    hipStream_t st = (hipStream_t)stream;
    const int nb = ceil_div(E, SCORE_BLOCK);
    double* scratch = nullptr;
    int rc = dev_alloc(&scratch, (size_t)nb * SS_K + SS_K);
    if (rc) return rc;
    ScoreEpIn in = {};
    in.starts = starts_dev; in.E = E; in.rows = rows;
    in.c = *cols;
    in.gamma = gamma; in.thr = threshold; in.has_thr = has_threshold ? 1 : 0;
    double S[SS_K];
    hipLaunchKernelGGL(k_score_episodes, dim3(nb), dim3(SCORE_BLOCK), 0, st, in, scratch);
    hipLaunchKernelGGL(k_score_fold, dim3(1), dim3(64), 0, st, scratch, nb, scratch + (size_t)nb * SS_K);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipMemcpyAsync(S, scratch + (size_t)nb * SS_K, sizeof(S), hipMemcpyDeviceToHost, st);
    const hipError_t err_sync = hipStreamSynchronize(st);
    (void)hipFree(scratch);
    if (err == hipSuccess) err = err_sync;
    if (err != hipSuccess) {
        set_error("score_episodes failed: %s", hipGetErrorString(err));
        return RL4RS_EHIP;
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const rl4rs_score_cols& c = in.c;
    const double n = S[SS_N];
    for (int i = 0; i < RL4RS_SCORE_N_STATS; ++i) stats_host[i] = nan;
    if (c.qd && c.qn && c.r_td && c.ter) stats_host[RL4RS_SCORE_TD_ERROR] = S[SS_TD] / n;
    if (c.qd && c.qp) stats_host[RL4RS_SCORE_DSA] = S[SS_DSA] / n;
    if (c.qp) {
        stats_host[RL4RS_SCORE_AVG_VALUE] = S[SS_QP] / n;
        stats_host[RL4RS_SCORE_INIT_VALUE] = S[SS_QP0] / (double)E;
    }
    if (c.qd && c.r_raw && has_threshold) {
        // np.mean(success_values) - np.mean(all_values): NaN when no episode succeeds; exactly 0 when all do (the same sum twice)
        stats_host[RL4RS_SCORE_SOFT_OPC] = S[SS_NS] > 0.0 ? S[SS_QDS] / S[SS_NS] - S[SS_QD] / n : nan;
        stats_host[RL4RS_SCORE_N_SUCCESS_ROWS] = S[SS_NS];
    }
    if (c.a && c.a_pi) stats_host[RL4RS_SCORE_ACTION_MATCH] = S[SS_MPI] / n;
    if (c.a && c.a_mask) stats_host[RL4RS_SCORE_ACTION_MATCH_MASK] = S[SS_MMASK] / n;
    if (c.diff) stats_host[RL4RS_SCORE_ACTION_DIFF] = S[SS_DIFF] / n;
    stats_host[RL4RS_SCORE_N_ROWS] = n;
    stats_host[RL4RS_SCORE_N_EPISODES] = (double)E;
    return RL4RS_OK;
}

}  // extern "C"
