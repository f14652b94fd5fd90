// Duplicate row groups of one scorer forward: k_row_dedup finds them at the top of the forward, k_din_x / k_augru_x
// then work on the representatives only (RecurArgs / DinArgs::order = the active list, ::n_active = its length), and
// k_row_expand copies a representative's AUGRU final states and attention scores to its duplicates in front of the head GEMM.
// RL4RS_DIEN_OPT_DUP_STORE: both producers store them to the same row of each duplicate themselves (the compaction pass of
// k_row_dedup then leaves the duplicates of every representative as a CSR list) and k_row_expand is not launched - measured
// slower than the copy launch and therefore off by default.
//
// Unit: the row group (`group` consecutive rows that share their cache slots - one row of an observation forward, the 8
// complete-state rows of an env in the reward forward).  Two groups are duplicates iff their slot-table entries are equal for
// every sequence input, their group * Cn category ids are equal and their group * Dn dense values are equal AS BIT PATTERNS
// (+0 != -0, equal NaN payloads are equal).  The decision is that comparison itself, no hash.  The scorer is batch-position
// invariant (tests/test_gpu_dien.py::test_dien_is_batch_position_invariant), so bitwise-equal inputs give bitwise-equal outputs.
//
// Search: positions in processing order (rl4rs_dien_set_row_order sorts the envs by history slot, so groups with equal slots
// are neighbours; no order = natural order).  A run = consecutive positions with equal slot entries.  Position p is compared,
// earliest first, with the positions of its run among the ROW_DEDUP_CAP - 1 in front of it and takes the first equal one.  In a
// run longer than the cap that choice may itself be a duplicate of a still earlier group: the compaction pass follows such
// chains to their root (equality is transitive), so no representative points to another one.  A duplicate further away than
// the cap from every equal group is simply kept as distinct.  `dense` and `cat` are read only at positions whose predecessor has
// the same slots: a batch without shared slots costs the look at the slot table alone.
//
// A forward whose caller hands it the partition (rl4rs_dien_set_row_partition; step.hip carries the env batch's partition from step to
// step, row_refine.hpp) launches no k_row_dedup: its consumers read the caller's rep / active / n_active instead.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rl4rs {

constexpr int ROW_DEDUP_CAP = 64;           // look-back window inside a run, in positions (own position included)
constexpr int ROW_DEDUP_THREADS = 1024;     // 16 waves = 16 positions per workgroup
constexpr int ROW_DEDUP_PER_THREAD = 8;     // compaction: positions per thread and pass (8192 per pass)

struct RowDedupArgs {
    int n_groups, group, Cn, Dn, S;
    const int32_t* slots; int64_t slots_stride;     // [S][n_groups]
    const int32_t* cat;                             // [n_groups * group, Cn]
    const float* dense;                             // [n_groups * group, Dn]
    const int32_t* order;                           // processing order of the groups, or NULL
    int32_t* rep;                                   // out [n_groups]: representative of every group (rep[g] == g: it is one)
    int32_t* active;                                // out [n_active]: the representatives in processing order
    int32_t* n_active;                              // out [0]: their number;  [1]: ticket of the finished workgroups (0 between launches)
    // duplicate lists (NULL = not built): the duplicates of active[i] are dup_list[dup_start[i] .. dup_start[i + 1]), chains resolved.
    // A list holds the groups whose rep[] is active[i]; its order is the order its writers arrived in (every reader stores the same
    // values to all of them).
    int32_t* dup_start;                             // out [n_active + 1]
    int32_t* dup_list;                              // out [n_groups - n_active]
    int32_t* dup_cur;                               // scratch [n_groups], by group: duplicates of a root, then its fill cursor; zero between launches
};

// n 32-bit words at x and y equal?  (wave-wide, uniform result; 16-byte loads when the layout allows).  `seed`: differences the
// caller has already collected per lane (the category ids), folded into the first vote instead of costing one of their own
__device__ __forceinline__ bool row_words_equal(const uint32_t* __restrict__ x, const uint32_t* __restrict__ y, int n, int lane, uint32_t seed = 0u) {
    if (((n & 3) | (int)((uintptr_t)x & 15) | (int)((uintptr_t)y & 15)) == 0) {
        const uint4* x4 = reinterpret_cast<const uint4*>(x);
        const uint4* y4 = reinterpret_cast<const uint4*>(y);
        const int n4 = n >> 2;
        for (int i0 = 0; i0 < n4; i0 += 256) {              // 4 loads per lane and side in flight, then one vote
            uint32_t d = i0 == 0 ? seed : 0u;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + u * 64 + lane;
                if (i < n4) {
                    const uint4 p = x4[i], q = y4[i];
                    d |= (p.x ^ q.x) | (p.y ^ q.y) | (p.z ^ q.z) | (p.w ^ q.w);
                }
            }
            if (__any(d != 0u)) return false;
        }
        return n4 > 0 || !__any(seed != 0u);
    }
    for (int i0 = 0; i0 < n; i0 += 256) {
        uint32_t d = i0 == 0 ? seed : 0u;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * 64 + lane;
            if (i < n) d |= x[i] ^ y[i];
        }
        if (__any(d != 0u)) return false;
    }
    return n > 0 || !__any(seed != 0u);
}

// Hand-off of rep[] from every workgroup to the one that compacts, and what a look at a candidate costs: a wave's
// work is a chain of dependent memory round trips, so the candidates' group ids come from the lanes that already hold them and
// a candidate's category ids and dense values are requested together and decided by one vote; ONE lane per workgroup releases
// at agent scope behind the workgroup's barrier (and one lane of the compacting workgroup acquires) instead of every thread.
__global__ __launch_bounds__(ROW_DEDUP_THREADS) void k_row_dedup(RowDedupArgs a) {
    __shared__ int s_last;
    __shared__ int s_wave[ROW_DEDUP_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = a.n_groups;
    auto group_at = [&](int p) { return a.order ? a.order[p] : p; };
    // ---- pass 1: one wave per position
    const int p = blockIdx.x * (ROW_DEDUP_THREADS / 64) + wave;
    if (p < n) {
        const int g = __builtin_amdgcn_readfirstlane(group_at(p));
        // lane l looks at position p - 1 - l (at most CAP - 1 positions back); its group id is requested with g
        const int pl = p - 1 - lane;
        const bool cand = lane < ROW_DEDUP_CAP - 1 && pl >= 0;
        const int gl = cand ? group_at(pl) : 0;
        int own[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) own[s] = s < a.S ? a.slots[(size_t)s * a.slots_stride + g] : 0;
        auto same_slots = [&](int g2) {
            bool e = true;
#pragma unroll
            for (int s = 0; s < 4; ++s)
                if (s < a.S) e = e && a.slots[(size_t)s * a.slots_stride + g2] == own[s];
            return e;
        };
        int found = g;
        // how far back the run goes: every lane compares its candidate's slot entries (the slot table of a forward is a few
        // cache lines per sequence input, so the 63 lanes cost what the one look at position p - 1 would)
        const unsigned long long m = __ballot(cand && same_slots(gl));
        const int back = __builtin_ctzll(~m);                 // lane 63 never votes: ~m != 0
        if (back > 0) {
            const int nc = a.group * a.Cn, nd = a.group * a.Dn;
            const uint32_t* c0 = reinterpret_cast<const uint32_t*>(a.cat) + (size_t)g * nc;
            const uint32_t* d0 = reinterpret_cast<const uint32_t*>(a.dense) + (size_t)g * nd;
            for (int k = back; k >= 1; --k) {                 // earliest first
                const int g2 = __builtin_amdgcn_readlane(gl, k - 1);
                const uint32_t* c2 = reinterpret_cast<const uint32_t*>(a.cat) + (size_t)g2 * nc;
                uint32_t dc = 0u;
                for (int i = lane; i < nc; i += 64) dc |= c0[i] ^ c2[i];
                if (!row_words_equal(d0, reinterpret_cast<const uint32_t*>(a.dense) + (size_t)g2 * nd, nd, lane, dc)) continue;
                found = g2;
                break;
            }
        }
        if (lane == 0) a.rep[g] = found;
    }
    // ---- the workgroup that finishes last compacts.  Every rep[] store of this workgroup is complete in front of the barrier; one
    // lane then releases them at agent scope and takes the ticket, and the lane that drew the last ticket acquires for its workgroup
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int last = atomicAdd(&a.n_active[1], 1) == (int)gridDim.x - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    auto rep_ld = [&](int g) { return __hip_atomic_load(a.rep + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    auto cur_ld = [&](int g) { return __hip_atomic_load(a.dup_cur + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    auto cur_st = [&](int g, int v) { __hip_atomic_store(a.dup_cur + g, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    // exclusive scan of one count per thread over the workgroup -> (offset of this thread, total); ends behind a barrier
    auto wg_scan = [&](int cnt, int& off, int& total) {
        int inc = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(inc, d);
            if (lane >= d) inc += v;
        }
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        int woff = 0;
        total = 0;
#pragma unroll
        for (int w2 = 0; w2 < ROW_DEDUP_THREADS / 64; ++w2) {
            const int v = s_wave[w2];
            woff += w2 < wave ? v : 0;
            total += v;
        }
        off = woff + inc - cnt;
        __syncthreads();
    };
    int base = 0;
    for (int p0 = 0; p0 < n; p0 += ROW_DEDUP_THREADS * ROW_DEDUP_PER_THREAD) {
        int gs[ROW_DEDUP_PER_THREAD], rs[ROW_DEDUP_PER_THREAD];
        const int q0 = p0 + tid * ROW_DEDUP_PER_THREAD;
#pragma unroll
        for (int i = 0; i < ROW_DEDUP_PER_THREAD; ++i) gs[i] = q0 + i < n ? group_at(q0 + i) : -1;
#pragma unroll
        for (int i = 0; i < ROW_DEDUP_PER_THREAD; ++i) rs[i] = gs[i] >= 0 ? rep_ld(gs[i]) : -2;
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < ROW_DEDUP_PER_THREAD; ++i) {
            if (gs[i] >= 0 && rs[i] != gs[i]) {               // follow a chain to its root (runs longer than the cap only)
                int r = rs[i], r2;
                while ((r2 = rep_ld(r)) != r) r = r2;
                if (r != rs[i]) __hip_atomic_store(a.rep + gs[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (a.dup_start) atomicAdd(&a.dup_cur[r], 1);     // one more duplicate of root r (dup_cur[] is all zero between launches)
            }
            cnt += rs[i] == gs[i];
        }
        int off, total;
        wg_scan(cnt, off, total);
        int o = base + off;
#pragma unroll
        for (int i = 0; i < ROW_DEDUP_PER_THREAD; ++i)
            if (rs[i] == gs[i]) a.active[o++] = gs[i];
        base += total;
    }
    if (tid == 0) {
        a.n_active[0] = base;
        a.n_active[1] = 0;
    }
    if (!a.dup_start) return;
    // ---- duplicate lists, indexed like active[]: exclusive scan of the counts in the order of the active list, then every duplicate
    // takes the next place of its root's list.  Written and read by this workgroup only (barriers order them; dup_cur through L2).
    const int n_act = base;
    if (n_act == n) {                                         // no duplicates: empty lists, no count was added
        for (int i = tid; i <= n_act; i += ROW_DEDUP_THREADS) a.dup_start[i] = 0;
        return;
    }
    __syncthreads();                                          // active[] and the counts are complete
    base = 0;
    for (int i0 = 0; i0 < n_act; i0 += ROW_DEDUP_THREADS * ROW_DEDUP_PER_THREAD) {
        const int q0 = i0 + tid * ROW_DEDUP_PER_THREAD;
        int ga[ROW_DEDUP_PER_THREAD], c[ROW_DEDUP_PER_THREAD];
#pragma unroll
        for (int i = 0; i < ROW_DEDUP_PER_THREAD; ++i) ga[i] = q0 + i < n_act ? a.active[q0 + i] : -1;
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < ROW_DEDUP_PER_THREAD; ++i) {
            c[i] = ga[i] >= 0 ? cur_ld(ga[i]) : 0;
            cnt += c[i];
        }
        int off, total;
        wg_scan(cnt, off, total);
        int o = base + off;
#pragma unroll
        for (int i = 0; i < ROW_DEDUP_PER_THREAD; ++i)
            if (ga[i] >= 0) {
                a.dup_start[q0 + i] = o;
                cur_st(ga[i], o);                             // the count becomes the fill cursor
                o += c[i];
            }
        base += total;
    }
    if (tid == 0) a.dup_start[n_act] = base;
    __syncthreads();
    for (int q = tid; q < n; q += ROW_DEDUP_THREADS) {
        const int g = group_at(q), r = rep_ld(g);
        if (r != g) a.dup_list[atomicAdd(&a.dup_cur[r], 1)] = g;
    }
    __syncthreads();                                          // every cursor has been used: zero again for the next launch
    for (int i = tid; i < n_act; i += ROW_DEDUP_THREADS) cur_st(a.active[i], 0);
}

struct RowExpandArgs {
    int R, group, n_groups, S, L, ncol;             // ncol: the leading columns of an all-feature row to copy (S * NH2 = the AUGRU final
                                                    // states; second tier on the active rows: S * NH2 + U + E = the whole row)
    const int32_t* rep;
    const int32_t* n_active;
    float* allf; int64_t ld;
    float* scores; int64_t scores_stride;           // [S][scores_stride] rows of L
    // second tier on the active rows (NULL otherwise): the query row [R, E] and the head output [R, obs_dim] as well
    float* q; int E;
    float* obs; int obs_dim;
};

// one wave per row: a row of a non-representative group takes its AUGRU states and attention scores from the same row of the
// representative - and, when the second tier ran on the active rows only (the launch then sits behind the head GEMM), the rest of
// its all-feature row, its query row and its head output.  Nothing to do (one scalar load per wave) when every group is its own
// representative.
__global__ __launch_bounds__(256) void k_row_expand(RowExpandArgs a) {
    if (a.n_active[0] == a.n_groups) return;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (row >= a.R) return;
    const int g = row / a.group;
    const int r = a.rep[g];
    if (r == g) return;
    const int src = r * a.group + (row - g * a.group);
    float* d = a.allf + (int64_t)row * a.ld;
    const float* s = a.allf + (int64_t)src * a.ld;
    if (((a.ncol | (int)a.ld) & 3) == 0) {
        for (int i = lane; i < a.ncol / 4; i += 64) reinterpret_cast<float4*>(d)[i] = reinterpret_cast<const float4*>(s)[i];
    } else {
        for (int i = lane; i < a.ncol; i += 64) d[i] = s[i];
    }
    for (int sq = 0; sq < a.S; ++sq) {
        float* sc = a.scores + (int64_t)sq * a.scores_stride;
        for (int i = lane; i < a.L; i += 64) sc[(int64_t)row * a.L + i] = sc[(int64_t)src * a.L + i];
    }
    if (a.q) {
        for (int i = lane; i < a.E; i += 64) a.q[(int64_t)row * a.E + i] = a.q[(int64_t)src * a.E + i];
    }
    if (a.obs) {
        float* od = a.obs + (int64_t)row * a.obs_dim;
        const float* os = a.obs + (int64_t)src * a.obs_dim;
        if ((a.obs_dim & 3) == 0 && ((uintptr_t)a.obs & 15) == 0) {
            for (int i = lane; i < a.obs_dim / 4; i += 64) reinterpret_cast<float4*>(od)[i] = reinterpret_cast<const float4*>(os)[i];
        } else {
            for (int i = lane; i < a.obs_dim; i += 64) od[i] = os[i];
        }
    }
}

}  // namespace rl4rs
