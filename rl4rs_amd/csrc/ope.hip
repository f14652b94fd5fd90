// Off-policy evaluation on the device (include/rl4rs_hip.h, "Off-policy evaluation"): propensity gathers into a [T, B] float64
// log, per-episode estimator terms, fixed-order reductions, and the Student-t quantile on the host.
//
// Launches of one estimate: k_ope_terms (one lane per episode) -> k_ope_fold (block partials, fixed order; the four means) ->
// k_ope_centred (second pass of the variances) -> k_ope_fold.  Every sum over episodes goes lane -> wave (shuffle tree) -> block
// (LDS, wave order) -> grid (one thread per statistic adds the block partials in block order): the grid shape depends on B alone,
// so the handle form and the array forms of the same numbers are bit-identical, and so are two runs.
#include "common.hpp"

#include <cfloat>
#include <limits>

namespace rl4rs {
namespace {

constexpr int OPE_MAX_T = 256;
constexpr int OPE_BLOCK = 256;          // 4 waves
constexpr int OPE_WAVES = OPE_BLOCK / 64;
// first-pass sums
enum { S_P, S_P2, S_RP, S_PC, S_PC2, S_RPC, S_DR, S_R, S_VPREV, S_VWIS, S_SEQDR, S_RSUM, S_SIM, K1 };
// second-pass (centred) sums and the means they are centred on
enum { C_IPS, C_CIPS, C_SNIPS, C_DR, K2 };
// per-episode values kept between the passes
enum { E_P, E_PC, E_R, E_DR, KE };
constexpr int OPE_FOLD_THREADS = 64;      // k_ope_fold: one thread per statistic
static_assert(K1 <= OPE_FOLD_THREADS && K2 <= OPE_FOLD_THREADS, "k_ope_fold would drop statistics");

struct OpeIn {
    // per-step arrays, element (b, t) at p[b * sb + t * st]; any may be null (its terms are NaN)
    const double *pi, *mu, *q, *rhat, *rlog;
    int64_t sb, st;
    // per-episode arrays [B]; with derive != 0 they are built from the per-step ones like offline_evaluation.py:38-57
    const double *e_r, *e_pp, *e_bp, *e_a, *e_s;
    int B, T, derive;
    double gamma;
};

__device__ __forceinline__ double clip_ratio(double x) {          // np.clip(x, 0.1, 10): NaN stays NaN
    return x < 0.1 ? 0.1 : (x > 10.0 ? 10.0 : x);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// block sum of K per-lane values -> part[blockIdx.x * K + k]; lds [K][OPE_WAVES]
template <int K>
__device__ __forceinline__ void block_sums(const double (&v)[K], double* lds, double* part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double s = wave_sum(v[k]);
        if (lane == 0) lds[k * OPE_WAVES + wave] = s;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double s = lds[threadIdx.x * OPE_WAVES];
        for (int w = 1; w < OPE_WAVES; ++w) s += lds[threadIdx.x * OPE_WAVES + w];
        part[(int64_t)blockIdx.x * K + threadIdx.x] = s;
    }
}

// One lane per episode: everything the estimators need of it (offline_policy_metrics.py:8-184).
//   ep  [KE, B]   ratio, clipped ratio, reward, dr term (for the centred pass)
//   ws  [T, B]    clip(cumprod(clip(pi / mu)) / B): the sequential weights (_calc_sequential_weigths, :8-20)
__global__ __launch_bounds__(OPE_BLOCK) void k_ope_terms(OpeIn in, double* __restrict__ ep, double* __restrict__ ws,
                                                         double* __restrict__ part) {
    __shared__ double lds[K1 * OPE_WAVES];
    const int b = blockIdx.x * OPE_BLOCK + threadIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double v[K1];
#pragma unroll
    for (int k = 0; k < K1; ++k) v[k] = 0.0;
    if (b < in.B) {
        const int T = in.T;
        const int64_t o = (int64_t)b * in.sb;
        double r, pp, bp, a, s;
        if (in.derive) {
            // offline_evaluation.py:44-57: sums over the steps in step order, products of probs * 100
            r = 0.0; a = 0.0; s = 0.0; pp = 1.0; bp = 1.0;
            for (int t = 0; t < T; ++t) {
                const int64_t i = o + (int64_t)t * in.st;
                r += in.rlog ? in.rlog[i] : nan;
                a += in.rhat ? in.rhat[i] : nan;
                s += in.q ? in.q[i] : nan;
                const double x = (in.pi ? in.pi[i] : nan) * 100.0, y = (in.mu ? in.mu[i] : nan) * 100.0;
                pp = t == 0 ? x : pp * x;
                bp = t == 0 ? y : bp * y;
            }
            s = s / (double)T;
        } else {
            r = in.e_r ? in.e_r[b] : nan;
            pp = in.e_pp ? in.e_pp[b] : nan;
            bp = in.e_bp ? in.e_bp[b] : nan;
            a = in.e_a ? in.e_a[b] : nan;
            s = in.e_s ? in.e_s[b] : nan;
        }
        const double p = pp / bp, pc = clip_ratio(p);
        const double dr = s + pc * (r - a);                     // eval_doubly_robust :155
        ep[(int64_t)E_P * in.B + b] = p;
        ep[(int64_t)E_PC * in.B + b] = pc;
        ep[(int64_t)E_R * in.B + b] = r;
        ep[(int64_t)E_DR * in.B + b] = dr;
        v[S_P] = p; v[S_P2] = p * p; v[S_RP] = r * p;
        v[S_PC] = pc; v[S_PC2] = pc * pc; v[S_RPC] = r * pc;
        v[S_DR] = dr; v[S_R] = r;
        // the per-step estimators
        double rho = 1.0, wsum = 0.0, vprev = 0.0, vwis = 0.0, rsum = 0.0, sim = 0.0;
        const double nB = (double)in.B;
        for (int t = 0; t < T; ++t) {
            const int64_t i = o + (int64_t)t * in.st;
            const double c = clip_ratio((in.pi ? in.pi[i] : nan) / (in.mu ? in.mu[i] : nan));
            rho = t == 0 ? c : rho * c;
            const double w = clip_ratio(rho / nB);
            ws[(int64_t)t * in.B + b] = w;
            wsum += w;
            const double wt = wsum / (double)(t + 1);           // eval_WIPS :133-134
            const double rl = in.rlog ? in.rlog[i] : nan;
            const double g = pow(in.gamma, (double)t);
            vprev += rl * g;                                    // :139
            vwis += w / wt * rl * g;                            // :140
            rsum += rl;
            sim += in.rhat ? in.rhat[i] : nan;
        }
        double sdr = 0.0;                                       // eval_seq_doubly_robust :171-175
        for (int t = T - 1; t >= 0; --t) {
            const int64_t i = o + (int64_t)t * in.st;
            const double w = ws[(int64_t)t * in.B + b];
            sdr = (in.q ? in.q[i] : nan) + w * ((in.rlog ? in.rlog[i] : nan) + sdr - (in.rhat ? in.rhat[i] : nan));
        }
        if (T == 0) { vprev = nan; vwis = nan; sdr = nan; rsum = nan; sim = in.derive ? 0.0 : nan; }
        v[S_VPREV] = vprev; v[S_VWIS] = vwis; v[S_SEQDR] = sdr; v[S_RSUM] = rsum; v[S_SIM] = sim;
    }
    block_sums<K1>(v, lds, part);
}

// Adds the block partials in block order (one thread per statistic).  first != 0: also the four means of the centred pass.
__global__ void k_ope_fold(const double* __restrict__ part, int nblocks, int K, double* __restrict__ sums, int first, int B) {
    const int k = threadIdx.x;
    if (k < K) {
        double s = 0.0;
        for (int j = 0; j < nblocks; ++j) s += part[(int64_t)j * K + k];
        sums[k] = s;
    }
    if (!first) return;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double n = (double)B;
        double* m = sums + K1 + K2;
        m[C_IPS] = sums[S_RP] / n;                   // np.mean(rewards * p_ratio)
        m[C_CIPS] = sums[S_RPC] / n;
        m[C_SNIPS] = sums[S_RPC] / sums[S_PC];       // eval_SNIPS :105
        m[C_DR] = sums[S_DR] / n;
    }
}

__global__ __launch_bounds__(OPE_BLOCK) void k_ope_centred(const double* __restrict__ ep, const double* __restrict__ means, int B,
                                                           double* __restrict__ part) {
    __shared__ double lds[K2 * OPE_WAVES];
    const int b = blockIdx.x * OPE_BLOCK + threadIdx.x;
    double v[K2] = {0.0, 0.0, 0.0, 0.0};
    if (b < B) {
        const double p = ep[(int64_t)E_P * B + b], pc = ep[(int64_t)E_PC * B + b], r = ep[(int64_t)E_R * B + b],
                     dr = ep[(int64_t)E_DR * B + b];
        const double d0 = r * p - means[C_IPS], d1 = r * pc - means[C_CIPS], d2 = r - means[C_SNIPS], d3 = dr - means[C_DR];
        v[C_IPS] = d0 * d0;                          // :57
        v[C_CIPS] = d1 * d1;                         // :83
        v[C_SNIPS] = (d2 * d2) * (pc * pc);          // :108
        v[C_DR] = d3 * d3;                           // scipy.stats.sem
    }
    block_sums<K2>(v, lds, part);
}

// Propensity of one action per row, a wave per row, VEC-wide row loads (VEC floats per lane and trip).
//   mode 0: out = x[idx];  1: x[idx] / sum(x[lo:hi]);  2: exp(x[idx] - m) / sum(exp(x[lo:hi] - m)), m = max(x[lo:hi])
//   clip != 0: idx = lo + clip(a - lo, 0, hi - lo - 1) (behavior_model.py:50,53,56); else an action outside [lo, hi) gives NaN
template <int VEC>
__global__ __launch_bounds__(OPE_BLOCK) void k_ope_propensity(const float* __restrict__ x, int64_t ld, int lo, int hi,
                                                              const int32_t* __restrict__ action, int mode, int clip, int B,
                                                              double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * OPE_WAVES + (threadIdx.x >> 6);
    if (b >= B) return;                              // whole waves leave together: the shuffles below are wave-local
    const float* row = x + (int64_t)b * ld;
    int a = action[b];
    bool ok = true;
    if (clip) a = lo + min(max(a - lo, 0), hi - lo - 1);
    else ok = a >= lo && a < hi;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if (mode == 0) {
        if (lane == 0) out[b] = ok ? (double)row[a] : nan;
        return;
    }
    // the aligned chunks that cover [lo, hi): chunk c holds elements [c * VEC, c * VEC + VEC)
    const int c0 = lo / VEC, c1 = (hi + VEC - 1) / VEC;
    float m = -FLT_MAX;
    if (mode == 2) {
        for (int c = c0 + lane; c < c1; c += 64) {
            float e[VEC];
            if (VEC == 4) *reinterpret_cast<float4*>(e) = *reinterpret_cast<const float4*>(row + c * VEC);
            else if (VEC == 2) *reinterpret_cast<float2*>(e) = *reinterpret_cast<const float2*>(row + c * VEC);
            else e[0] = row[c];
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const int i = c * VEC + j;
                if (i >= lo && i < hi) m = fmaxf(m, e[j]);
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    }
    double s = 0.0;
    for (int c = c0 + lane; c < c1; c += 64) {
        float e[VEC];
        if (VEC == 4) *reinterpret_cast<float4*>(e) = *reinterpret_cast<const float4*>(row + c * VEC);
        else if (VEC == 2) *reinterpret_cast<float2*>(e) = *reinterpret_cast<const float2*>(row + c * VEC);
        else e[0] = row[c];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const int i = c * VEC + j;
            if (i >= lo && i < hi) s += mode == 2 ? exp((double)e[j] - (double)m) : (double)e[j];
        }
    }
    s = wave_sum(s);
    if (lane == 0) {
        double num = nan;
        if (ok) num = mode == 2 ? exp((double)row[a] - (double)m) : (double)row[a];
        out[b] = num / s;
    }
}

// One OPE step of a score-matrix policy (rl4rs_ope_greedy_rows): masked row m, its first maximum, softmax(m)[logged] in float64 and
// the value, a wave per row.  STAGED: the row is read from memory once - a scalar head up to the row's first 16-byte boundary, float4
// chunks, a scalar tail - into the wave's share of LDS, element c at s[mis + c] with mis = the row's misalignment in floats, so a
// chunk lands on a 16-byte LDS slot whatever the row stride is; the only cross-lane hand-off is that staging (one barrier).  Every
// later pass walks c = lane, lane + 64, ...: a lane re-reads what it wrote itself.  !STAGED (a row beyond the LDS share): the
// same passes recompute m from memory.  Sums: lane (increasing c), then the shuffle tree of wave_sum; no atomics.
constexpr int OPE_ROW_LDS_FLOATS = 4096;          // per wave: 4 waves x 16 KB = the 64 KB a workgroup gets without asking

__device__ __forceinline__ float ope_masked(float v, const uint32_t* mrow, int c, int mask_set) {
    if (mrow && !((mrow[c >> 5] >> (c & 31)) & 1u)) v = mask_set ? -3.4028235e38f : v + (-3.4028235e38f);
    return v;
}

template <bool STAGED>
__global__ __launch_bounds__(OPE_BLOCK) void k_ope_greedy_rows(int N, const float* __restrict__ scores, int A, int64_t ld, int stride,
                                                               const uint32_t* __restrict__ mask, int mask_set,
                                                               const int32_t* __restrict__ logged, const float* __restrict__ value,
                                                               int64_t value_ld, int32_t* __restrict__ actions,
                                                               double* __restrict__ pi, double* __restrict__ q,
                                                               float* __restrict__ masked_out) {
    extern __shared__ __attribute__((aligned(16))) float ope_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * OPE_WAVES + wave;
    const bool live = b < N;                         // (no early return: the staging barrier is the workgroup's)
    const float* row = scores + (int64_t)(live ? b : 0) * ld;
    const uint32_t* mrow = mask ? mask + (int64_t)(live ? b : 0) * ((A + 31) >> 5) : nullptr;
    float* s = ope_lds;
    if (STAGED) {
        const int mis = (int)((reinterpret_cast<uintptr_t>(row) >> 2) & 3);
        s = ope_lds + (size_t)wave * stride + mis;
        if (live) {
            const int head = min(A, (4 - mis) & 3), nchunk = (A - head) >> 2, tail = head + 4 * nchunk;
            if (lane < head) s[lane] = row[lane];
            for (int k = lane; k < nchunk; k += 64)
                *reinterpret_cast<float4*>(s + head + 4 * k) = *reinterpret_cast<const float4*>(row + head + 4 * k);
            if (tail + lane < A) s[tail + lane] = row[tail + lane];
        }
        __syncthreads();
    }
    if (!live) return;
    // pass 1: the masked row (kept in LDS, written out on request), its first maximum
    float best = 0.f;
    int best_a = 0x7fffffff;
    for (int c = lane; c < A; c += 64) {
        const float v = ope_masked(STAGED ? s[c] : row[c], mrow, c, mask_set);
        if (STAGED) s[c] = v;
        if (masked_out) masked_out[(int64_t)b * A + c] = v;
        if (best_a == 0x7fffffff || v > best) { best = v; best_a = c; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off, 64);
        const int oa = __shfl_xor(best_a, off, 64);
        if (oa != 0x7fffffff && (best_a == 0x7fffffff || ob > best || (ob == best && oa < best_a))) { best = ob; best_a = oa; }
    }
    // pass 2: sum_c exp(m[c] - max) in float64, and m[l] from the lane that holds it
    const int l = logged ? logged[b] : -1;
    const bool ok = l >= 0 && l < A;
    double sum = 0.0;
    float ml = 0.f;
    for (int c = lane; c < A; c += 64) {
        const float v = STAGED ? s[c] : ope_masked(row[c], mrow, c, mask_set);
        if (c == l) ml = v;
        sum += exp((double)v - (double)best);
    }
    sum = wave_sum(sum);
    ml = __shfl(ml, ok ? (l & 63) : 0, 64);
    if (lane == 0) {
        actions[b] = best_a;
        if (pi) pi[b] = ok ? exp((double)ml - (double)best) / sum : __longlong_as_double(0x7ff8000000000000LL);
        if (q) q[b] = value ? (double)value[(int64_t)b * value_ld] : (double)best;
    }
}

template <typename T>
__global__ void k_ope_column(const T* __restrict__ src, int B, double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) out[b] = (double)src[b];
}

int64_t scratch_doubles(int B, int T) {
    const int64_t nb = ceil_div(B, OPE_BLOCK);
    return (int64_t)KE * B + (int64_t)(T > 0 ? T : 1) * B + nb * K1 + nb * K2 + (K1 + K2 + K2);
}

// ---- host arithmetic: Student's t quantile ------------------------------------------------------------------------------

// lgamma(a + 1/2) - lgamma(a): directly for small a, from Stirling's series for large a (the difference of two lgamma values of
// magnitude 6e6 at a = 5e5 would keep 9 digits)
double lgamma_half_step(double a) {
    if (a < 64.0) return std::lgamma(a + 0.5) - std::lgamma(a);
    auto tail = [](double z) {
        const double z2 = z * z;
        return (1.0 / 12.0 - (1.0 / 360.0 - (1.0 / 1260.0 - 1.0 / (1680.0 * z2)) / z2) / z2) / z;
    };
    return a * std::log1p(0.5 / a) + 0.5 * std::log(a) - 0.5 + (tail(a + 0.5) - tail(a));
}

// continued fraction of the incomplete beta function (modified Lentz)
double betacf(double a, double b, double x) {
    const double tiny = 1e-300, eps = 1e-16;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (std::fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= 2000000; ++m) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d; if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d; if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (std::fabs(del - 1.0) <= eps) break;
    }
    return h;
}

// P(T > t) for t >= 0: I_x(df / 2, 1 / 2) / 2 with x = df / (df + t^2)
double t_upper_tail(double t, double df) {
    if (!(t > 0.0)) return 0.5;
    const double a = 0.5 * df, t2 = t * t;
    if (std::isinf(t2)) return 0.0;
    const double x = df / (df + t2), y = t2 / (df + t2);                  // y = 1 - x, without the cancellation
    const double lnx = -std::log1p(t2 / df), lny = -std::log1p(df / t2);
    const double lnB = 0.5 * std::log(M_PI) - lgamma_half_step(a);         // ln B(a, 1/2)
    const double front = std::exp(a * lnx + 0.5 * lny - lnB);
    double I;
    if (x < (a + 1.0) / (a + 2.5)) I = front * betacf(a, 0.5, x) / a;
    else I = 1.0 - front * betacf(0.5, a, y) / 0.5;
    return 0.5 * I;
}

double student_t_ppf(double p, double df) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (!(df > 0.0) || !(p >= 0.0 && p <= 1.0) || std::isinf(df)) return nan;
    if (p == 0.5) return 0.0;
    if (p == 0.0) return -std::numeric_limits<double>::infinity();
    if (p == 1.0) return std::numeric_limits<double>::infinity();
    const bool upper = p > 0.5;
    const double q = upper ? 1.0 - p : p;                                 // tail mass beyond the answer's magnitude
    double lo = 0.0, hi = 1.0;
    while (t_upper_tail(hi, df) > q && hi < 1e300) { lo = hi; hi *= 2.0; }
    for (int it = 0; it < 200; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (mid <= lo || mid >= hi) break;
        if (t_upper_tail(mid, df) > q) lo = mid; else hi = mid;
    }
    const double t = 0.5 * (lo + hi);
    return upper ? t : -t;
}

// offline_policy_metrics.py:34-38 and the tails of the six functions, from the reduced sums
void finish_stats(const double* S, const double* Cn, int B, bool have_ep, bool have_step, double* out) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int i = 0; i < RL4RS_OPE_N_STATS; ++i) out[i] = nan;
    const double n = (double)B;
    if (have_ep) {
        auto ess = [&](double sp, double sp2, double* n_e, double* cv, double* root) {
            const double mean = sp / n, mean2 = sp2 / n;
            *n_e = n * (mean * mean) / mean2;
            if (std::isfinite(*n_e)) {
                const double whole = std::trunc(*n_e);                      // int(n_e)
                *cv = student_t_ppf(1.0 - 0.00125, whole - 1.0);
                *root = std::sqrt(whole);
            } else {                                                        // (the reference raises on int(nan) / int(inf))
                *cv = nan; *root = nan;
            }
        };
        double root_raw, root;
        ess(S[S_P], S[S_P2], &out[RL4RS_OPE_N_E_RAW], &out[RL4RS_OPE_CV_RAW], &root_raw);
        ess(S[S_PC], S[S_PC2], &out[RL4RS_OPE_N_E], &out[RL4RS_OPE_CV], &root);
        out[RL4RS_OPE_IPS] = S[S_RP] / n;
        out[RL4RS_OPE_IPS_C] = out[RL4RS_OPE_CV_RAW] * std::sqrt(Cn[C_IPS] / n) / root_raw;
        out[RL4RS_OPE_CIPS] = S[S_RPC] / n;
        out[RL4RS_OPE_CIPS_C] = out[RL4RS_OPE_CV] * std::sqrt(Cn[C_CIPS] / n) / root;
        out[RL4RS_OPE_SNIPS] = S[S_RPC] / S[S_PC];
        out[RL4RS_OPE_SNIPS_C] = out[RL4RS_OPE_CV] * std::sqrt(Cn[C_SNIPS] / (S[S_PC] * S[S_PC])) / root;
        out[RL4RS_OPE_DR] = (S[S_DR] / n) / (S[S_R] / n);
        out[RL4RS_OPE_DR_SE] = std::sqrt(Cn[C_DR] / (n - 1.0)) / std::sqrt(n);
    }
    if (have_step) {
        const double vprev = S[S_VPREV];
        out[RL4RS_OPE_WIPS] = S[S_VWIS] / (vprev < 1e-8 ? 1e-8 : vprev);      // np.clip(V_prev, 1e-8, None): NaN stays NaN
        out[RL4RS_OPE_WIPS_2] = 0.0;
        out[RL4RS_OPE_SEQDR] = (S[S_SEQDR] / n) / (S[S_RSUM] / n);
        out[RL4RS_OPE_SEQDR_2] = 0.0;
        out[RL4RS_OPE_SIM_REWARD] = S[S_SIM] / n;
    }
}

int run_estimate(const OpeIn& in, double* scratch, bool have_ep, bool have_step, double* stats_host, hipStream_t st) {
    const int B = in.B, nb = ceil_div(B, OPE_BLOCK);
    double* ep = scratch;
    double* ws = ep + (int64_t)KE * B;
    double* part1 = ws + (int64_t)(in.T > 0 ? in.T : 1) * B;
    double* part2 = part1 + (int64_t)nb * K1;
    double* sums = part2 + (int64_t)nb * K2;                 // K1 sums | K2 centred sums | K2 means
    hipLaunchKernelGGL(k_ope_terms, dim3(nb), dim3(OPE_BLOCK), 0, st, in, ep, ws, part1);
    RL4RS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ope_fold, dim3(1), dim3(OPE_FOLD_THREADS), 0, st, part1, nb, (int)K1, sums, 1, B);
    RL4RS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ope_centred, dim3(nb), dim3(OPE_BLOCK), 0, st, ep, sums + K1 + K2, B, part2);
    RL4RS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ope_fold, dim3(1), dim3(OPE_FOLD_THREADS), 0, st, part2, nb, (int)K2, sums + K1, 0, B);
    RL4RS_LAUNCH_CHECK();
    double host[K1 + K2];
    RL4RS_HIP_TRY(hipMemcpyAsync(host, sums, sizeof(host), hipMemcpyDeviceToHost, st));
    RL4RS_HIP_TRY(hipStreamSynchronize(st));
    finish_stats(host, host + K1, B, have_ep, have_step, stats_host);
    return RL4RS_OK;
}

// vector loads only where every chunk of every row lies inside its A elements and is aligned
int launch_propensity(const float* x, int A, int64_t ld, int lo, int hi, const int32_t* action, int mode, int clip, int B, double* out,
                      hipStream_t st) {
    const dim3 grid(ceil_div(B, OPE_WAVES)), block(OPE_BLOCK);
    const uintptr_t addr = reinterpret_cast<uintptr_t>(x);
    if (A % 4 == 0 && ld % 4 == 0 && addr % 16 == 0) hipLaunchKernelGGL(k_ope_propensity<4>, grid, block, 0, st, x, ld, lo, hi, action, mode, clip, B, out);
    else if (A % 2 == 0 && ld % 2 == 0 && addr % 8 == 0) hipLaunchKernelGGL(k_ope_propensity<2>, grid, block, 0, st, x, ld, lo, hi, action, mode, clip, B, out);
    else hipLaunchKernelGGL(k_ope_propensity<1>, grid, block, 0, st, x, ld, lo, hi, action, mode, clip, B, out);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

int check_shape(const char* who, int64_t B, int64_t T) {
    RL4RS_REQUIRE(B >= 1, "%s: batch size %lld < 1", who, (long long)B);
    RL4RS_REQUIRE(T >= 1, "%s: %lld steps < 1", who, (long long)T);
    RL4RS_REQUIRE(T <= OPE_MAX_T, "%s: %lld steps > %d (one lane walks an episode's steps)", who, (long long)T, OPE_MAX_T);
    RL4RS_REQUIRE(B * T < ((int64_t)1 << 28), "%s: %lld x %lld log entries >= 2^28", who, (long long)B, (long long)T);
    return RL4RS_OK;
}

int need_device() {
    if (rl4rs_device_count() <= 0) {
        set_error("no HIP device visible: librl4rs_hip has no CPU fallback");
        return RL4RS_EHIP;
    }
    return RL4RS_OK;
}

}  // namespace
}  // namespace rl4rs

using namespace rl4rs;

struct rl4rs_ope {
    int max_B = 0, max_T = 0, B = 0, T = 0;
    double* log = nullptr;          // [N_COLS][T][B] of the current epoch (column stride max_T * max_B)
    double* scratch = nullptr;
    uint8_t seen[RL4RS_OPE_N_COLS][OPE_MAX_T];
    double* col(int c, int t) const { return log + (int64_t)c * max_T * max_B + (int64_t)t * B; }
    bool complete(int c) const {
        for (int t = 0; t < T; ++t)
            if (!seen[c][t]) return false;
        return T > 0;
    }
};

extern "C" {

double rl4rs_student_t_ppf(double p, double df) { return student_t_ppf(p, df); }

int rl4rs_ope_create(int32_t max_batch, int32_t max_steps, rl4rs_ope** out) {
    RL4RS_REQUIRE(out, "ope_create: null argument");
    *out = nullptr;
    int rc = check_shape("ope_create", max_batch, max_steps);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    rl4rs_ope* h = new rl4rs_ope();
    h->max_B = max_batch;
    h->max_T = max_steps;
    memset(h->seen, 0, sizeof(h->seen));
    if ((rc = dev_alloc(&h->log, (size_t)RL4RS_OPE_N_COLS * max_batch * max_steps)) ||
        (rc = dev_alloc(&h->scratch, (size_t)scratch_doubles(max_batch, max_steps)))) {
        rl4rs_ope_destroy(h);
        return rc;
    }
    *out = h;
    return RL4RS_OK;
}

int rl4rs_ope_destroy(rl4rs_ope* h) {
    if (!h) return RL4RS_OK;
    if (h->log) (void)hipFree(h->log);
    if (h->scratch) (void)hipFree(h->scratch);
    delete h;
    return RL4RS_OK;
}

int rl4rs_ope_begin(rl4rs_ope* h, int32_t B, int32_t T) {
    RL4RS_REQUIRE(h, "ope_begin: null handle");
    int rc = check_shape("ope_begin", B, T);
    if (rc) return rc;
    RL4RS_REQUIRE(B <= h->max_B && T <= h->max_T, "ope_begin: (%d, %d) exceeds the handle's (%d, %d)", B, T, h->max_B, h->max_T);
    h->B = B;
    h->T = T;
    memset(h->seen, 0, sizeof(h->seen));
    return RL4RS_OK;
}

#define OPE_STEP_CHECK(who)                                                                            \
    RL4RS_REQUIRE(h, who ": null handle");                                                             \
    if (h->B < 1) { set_error(who ": no epoch begun"); return RL4RS_ESTATE; }                          \
    RL4RS_REQUIRE(t >= 0 && t < h->T, who ": step %d outside [0, %d)", t, h->T)

int rl4rs_ope_record_policy(rl4rs_ope* h, int32_t t, const float* scores_dev, int32_t A, int64_t ld, const int32_t* action_dev,
                            int32_t is_logits, void* stream) {
    OPE_STEP_CHECK("ope_record_policy");
    RL4RS_REQUIRE(scores_dev && action_dev && A >= 1 && ld >= A, "ope_record_policy: bad scores (A %d, ld %lld)", A, (long long)ld);
    int rc = launch_propensity(scores_dev, A, ld, 0, A, action_dev, is_logits ? 2 : 0, 0, h->B, h->col(RL4RS_OPE_COL_PI, t), (hipStream_t)stream);
    if (!rc) h->seen[RL4RS_OPE_COL_PI][t] = 1;
    return rc;
}

int rl4rs_ope_record_behavior(rl4rs_ope* h, int32_t t, const float* y_dev, int32_t A_b, int64_t ld, int32_t lo, int32_t hi,
                              const int32_t* action_dev, int32_t is_logits, void* stream) {
    OPE_STEP_CHECK("ope_record_behavior");
    RL4RS_REQUIRE(y_dev && action_dev && A_b >= 1 && ld >= A_b, "ope_record_behavior: bad scores (A_b %d, ld %lld)", A_b, (long long)ld);
    RL4RS_REQUIRE(lo >= 0 && lo < hi && hi <= A_b, "ope_record_behavior: range [%d, %d) outside [0, %d)", lo, hi, A_b);
    int rc = launch_propensity(y_dev, A_b, ld, lo, hi, action_dev, is_logits ? 2 : 1, 1, h->B, h->col(RL4RS_OPE_COL_MU, t), (hipStream_t)stream);
    if (!rc) h->seen[RL4RS_OPE_COL_MU][t] = 1;
    return rc;
}

int rl4rs_ope_record_q(rl4rs_ope* h, int32_t t, const float* scores_dev, int32_t A, int64_t ld, const int32_t* action_dev,
                       void* stream) {
    OPE_STEP_CHECK("ope_record_q");
    RL4RS_REQUIRE(scores_dev && action_dev && A >= 1 && ld >= A, "ope_record_q: bad scores (A %d, ld %lld)", A, (long long)ld);
    int rc = launch_propensity(scores_dev, A, ld, 0, A, action_dev, 0, 0, h->B, h->col(RL4RS_OPE_COL_Q, t), (hipStream_t)stream);
    if (!rc) h->seen[RL4RS_OPE_COL_Q][t] = 1;
    return rc;
}

int rl4rs_ope_record_column(rl4rs_ope* h, int32_t t, int32_t col, const void* src_dev, int32_t src_is_f64, void* stream) {
    OPE_STEP_CHECK("ope_record_column");
    RL4RS_REQUIRE(col >= 0 && col < RL4RS_OPE_N_COLS && src_dev, "ope_record_column: bad column %d or null source", col);
    const dim3 grid(ceil_div(h->B, 256)), block(256);
    if (src_is_f64) hipLaunchKernelGGL(k_ope_column<double>, grid, block, 0, (hipStream_t)stream, static_cast<const double*>(src_dev), h->B, h->col(col, t));
    else hipLaunchKernelGGL(k_ope_column<float>, grid, block, 0, (hipStream_t)stream, static_cast<const float*>(src_dev), h->B, h->col(col, t));
    RL4RS_LAUNCH_CHECK();
    h->seen[col][t] = 1;
    return RL4RS_OK;
}

int rl4rs_ope_greedy_rows(int32_t N, const float* scores_dev, int32_t A, int64_t ld, const uint32_t* mask_bits_dev, int32_t mask_set,
                          const int32_t* logged_dev, const float* value_dev, int64_t value_ld, int32_t* actions_dev,
                          double* pi_dev, double* q_dev, float* masked_out_dev, void* stream) {
    RL4RS_REQUIRE(N >= 1 && scores_dev && actions_dev && A >= 1 && ld >= A, "ope_greedy_rows: bad scores (N %d, A %d, ld %lld)", N, A,
                  (long long)ld);
    RL4RS_REQUIRE(mask_set == 0 || mask_set == 1, "ope_greedy_rows: mask_set %d is neither 0 (add) nor 1 (set)", mask_set);
    RL4RS_REQUIRE(!pi_dev || logged_dev, "ope_greedy_rows: pi needs the logged actions");
    RL4RS_REQUIRE(!value_dev || value_ld >= 1, "ope_greedy_rows: value stride %lld < 1", (long long)value_ld);
    RL4RS_REQUIRE(reinterpret_cast<uintptr_t>(scores_dev) % 4 == 0, "ope_greedy_rows: scores not aligned to a float");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(ceil_div(N, OPE_WAVES)), block(OPE_BLOCK);
    const int stride = (A + 3) / 4 * 4 + 4;              // floats of one wave's LDS share: the row behind its misalignment (<= 3)
    if (stride <= OPE_ROW_LDS_FLOATS)
        hipLaunchKernelGGL(k_ope_greedy_rows<true>, grid, block, (size_t)OPE_WAVES * stride * sizeof(float), st, N, scores_dev, A, ld, stride,
                           mask_bits_dev, mask_set, logged_dev, value_dev, value_ld, actions_dev, pi_dev, q_dev, masked_out_dev);
    else
        hipLaunchKernelGGL(k_ope_greedy_rows<false>, grid, block, 0, st, N, scores_dev, A, ld, 0, mask_bits_dev, mask_set, logged_dev,
                           value_dev, value_ld, actions_dev, pi_dev, q_dev, masked_out_dev);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

int rl4rs_ope_log(rl4rs_ope* h, int32_t col, double** dev_out, int64_t* n_out) {
    RL4RS_REQUIRE(h && dev_out && n_out && col >= 0 && col < RL4RS_OPE_N_COLS, "ope_log: bad argument");
    *dev_out = h->col(col, 0);
    *n_out = (int64_t)h->T * h->B;
    return RL4RS_OK;
}

int rl4rs_ope_mark_recorded(rl4rs_ope* h, int32_t t, int32_t col) {
    OPE_STEP_CHECK("ope_mark_recorded");
    RL4RS_REQUIRE(col >= 0 && col < RL4RS_OPE_N_COLS, "ope_mark_recorded: bad column %d", col);
    h->seen[col][t] = 1;
    return RL4RS_OK;
}

int rl4rs_ope_estimate(rl4rs_ope* h, double gamma, double* stats_host, void* stream) {
    RL4RS_REQUIRE(h && stats_host, "ope_estimate: null argument");
    if (h->B < 1) { set_error("ope_estimate: no epoch begun"); return RL4RS_ESTATE; }
    OpeIn in = {};
    auto col = [&](int c) -> const double* { return h->complete(c) ? h->col(c, 0) : nullptr; };
    in.pi = col(RL4RS_OPE_COL_PI);
    in.mu = col(RL4RS_OPE_COL_MU);
    in.q = col(RL4RS_OPE_COL_Q);
    in.rhat = col(RL4RS_OPE_COL_REWARD);
    in.rlog = col(RL4RS_OPE_COL_LOGGED_REWARD);
    in.sb = 1;
    in.st = h->B;
    in.B = h->B;
    in.T = h->T;
    in.derive = 1;
    in.gamma = gamma;
    return run_estimate(in, h->scratch, true, true, stats_host, (hipStream_t)stream);
}

static int array_estimate(OpeIn& in, bool have_ep, bool have_step, double* stats_host, void* stream) {
    int rc = need_device();
    if (rc) return rc;
    double* scratch = nullptr;
    if ((rc = dev_alloc(&scratch, (size_t)scratch_doubles(in.B, in.T)))) return rc;
    rc = run_estimate(in, scratch, have_ep, have_step, stats_host, (hipStream_t)stream);
    if (rc) (void)hipStreamSynchronize((hipStream_t)stream);
    (void)hipFree(scratch);
    return rc;
}

int rl4rs_ope_episode_stats(int32_t B, const double* rewards_dev, const double* policy_prob_dev, const double* behavior_prob_dev,
                            const double* rhat_dev, const double* state_dev, double* stats_host, void* stream) {
    RL4RS_REQUIRE(B >= 1, "ope_episode_stats: batch size %d < 1", B);
    RL4RS_REQUIRE(B < (1 << 28), "ope_episode_stats: batch size %d >= 2^28", B);
    RL4RS_REQUIRE(rewards_dev && policy_prob_dev && behavior_prob_dev && stats_host, "ope_episode_stats: null argument");
    OpeIn in = {};
    in.e_r = rewards_dev;
    in.e_pp = policy_prob_dev;
    in.e_bp = behavior_prob_dev;
    in.e_a = rhat_dev;
    in.e_s = state_dev;
    in.B = B;
    in.T = 0;
    in.gamma = 1.0;
    return array_estimate(in, true, false, stats_host, stream);
}

int rl4rs_ope_step_stats(int32_t B, int32_t T, const double* step_rewards_dev, const double* policy_prob_dev,
                         const double* behavior_prob_dev, const double* rhat_dev, const double* state_dev, double gamma,
                         double* stats_host, void* stream) {
    int rc = check_shape("ope_step_stats", B, T);
    if (rc) return rc;
    RL4RS_REQUIRE(step_rewards_dev && policy_prob_dev && behavior_prob_dev && stats_host, "ope_step_stats: null argument");
    OpeIn in = {};
    in.rlog = step_rewards_dev;
    in.pi = policy_prob_dev;
    in.mu = behavior_prob_dev;
    in.rhat = rhat_dev;
    in.q = state_dev;
    in.sb = T;
    in.st = 1;
    in.B = B;
    in.T = T;
    in.gamma = gamma;
    return array_estimate(in, false, true, stats_host, stream);
}

}  // extern "C"
