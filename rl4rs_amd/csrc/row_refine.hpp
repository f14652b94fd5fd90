// The duplicate-row partition of the env batch, carried from one forward of an episode to the next instead of being
// found again by k_row_dedup's comparison of whole rows.  Two envs whose state rows were bitwise equal at the previous forward
// (equal user features, equal cache slots, equal prev_actions) have equal rows now iff they have just taken the same action, and
// two envs whose rows differed can never become equal again: the partition only ever refines, and one integer per env - the
// resolved action id - decides how.
//
// row_refine_env (one wave per env, inside the act kernel): rep[g] = rep_prev[g] when g took the action of its representative;
// otherwise g is MARKED (rep[g] = ROW_REFINE_MARK) and cnt[2] counts it.  row_refine_finish (behind the row loop): the workgroup
// that finishes last - the ticket pattern of k_row_dedup - reads the count.  Zero: the active list and its length stand.  Non-zero:
// every marked position searches, in processing order and earliest first, the ROW_DEDUP_CAP - 1 positions in front of it for a
// group with the same previous representative and the same action (k_row_dedup's window, on two integers instead of 453 words) and
// takes the first; none: the group is its own representative.  Chains are then followed to their roots and active / n_active are
// rebuilt exactly as k_row_dedup's compaction pass builds them.
//
// Every representative this leaves is one k_row_dedup would leave on the same rows (a group with an equal row inside the window
// was, by induction, in its class at the previous forward as well, and is found by the search above), so the carried partition
// never has more representatives than the content search; it may have fewer: groups that stay with their representative stay
// merged however far apart they are.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rl4rs {

constexpr int ROW_REFINE_CAP = 64;           // = ROW_DEDUP_CAP of row_dedup.hpp, whose kernels live in dien.hip alone (checked there)
constexpr int ROW_REFINE_MARK = -1;
constexpr int ROW_REFINE_PER_THREAD = 8;     // compaction: positions per thread and pass

struct RowRefineArgs {
    int n;                        // envs (= row groups of the forwards the partition is handed to)
    const int32_t* rep_prev;      // [n] representative of every env at the previous forward (rep_prev[rep_prev[g]] == rep_prev[g])
    int32_t* rep;                 // out [n]: the same for the rows this act builds (a buffer of its own: other workgroups still read rep_prev)
    int32_t* active;              // in / out [n_active]: the representatives in processing order
    int32_t* cnt;                 // [0] n_active (in / out), [1] ticket of the finished workgroups, [2] marked envs; [1], [2] zero between launches
    const int32_t* order;         // processing order of the envs (the scorer's row order), or NULL
    // the first act behind an adopted partition (step.hip): active / cnt[0] are not the stepper's yet - every wave copies its entry
    // of the adopted active list, and the last workgroup the adopted length when nothing split.  NULL otherwise
    const int32_t* active_src; const int32_t* n_active_src;
};

// dynamic LDS row_refine_finish needs in a workgroup of `threads` threads: (previous representative, action) and the env of one
// chunk of positions plus the window in front of it
inline size_t row_refine_smem(int threads) { return (size_t)(threads + ROW_REFINE_CAP) * 12; }

__device__ __forceinline__ int row_refine_key(const int32_t* __restrict__ actions, int A, int g) {
    const int k = actions[g];
    return (k < 0 || k >= A) ? 0 : k;      // the act kernel plays item 0 for an id out of range (and raises the error flag)
}

// env g has just taken action `a` (resolved: inside [0, A)); r = rep_prev[g] and ar = the resolved action of r were requested next
// to the act's own loads (the act kernel asks for r with its action and for ar behind it, and comes here when the row is built:
// the two round trips run beside the row's gathers instead of in front of them)
__device__ __forceinline__ void row_refine_env(const RowRefineArgs& rf, int g, int a, int r, int ar, int lane) {
    if (lane == 0) {
        if (rf.active_src) rf.active[g] = rf.active_src[g];   // (entries behind the adopted length are never read)
        if (ar == a) {
            rf.rep[g] = r;
        } else {
            rf.rep[g] = ROW_REFINE_MARK;
            atomicAdd(&rf.cnt[2], 1);
        }
    }
}

// behind the row loop, by every thread of every workgroup; `smem`: row_refine_smem(blockDim.x) bytes no wave uses any more
__device__ __forceinline__ void row_refine_finish(const RowRefineArgs& rf, const int32_t* __restrict__ actions, int A, char* smem) {
    __shared__ int s_last;
    __shared__ int s_wave[16];
    const int tid = threadIdx.x, lane = tid & 63, nt = blockDim.x, nw = nt >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = rf.n;
    // every rep[] store and count of this workgroup is complete in front of the barrier; one lane releases them at agent scope and
    // takes the ticket, the lane that drew the last one acquires for its workgroup (k_row_dedup's hand-off)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int last = atomicAdd(&rf.cnt[1], 1) == (int)gridDim.x - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    const int splits = __hip_atomic_load(rf.cnt + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (splits == 0) {                                        // nothing split: the active list and its length stand
        if (tid == 0) {
            if (rf.n_active_src) rf.cnt[0] = rf.n_active_src[0];
            rf.cnt[1] = 0;
        }
        return;
    }
    auto group_at = [&](int p) { return rf.order ? rf.order[p] : p; };
    auto rep_ld = [&](int g) { return __hip_atomic_load(rf.rep + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    auto rep_st = [&](int g, int v) { __hip_atomic_store(rf.rep + g, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    {
        // ---- resolve the marked positions: a chunk of nt positions and the CAP - 1 in front of it in LDS, one thread per position
        int2* s_cls = reinterpret_cast<int2*>(smem);                      // [nt + CAP] (previous representative, action)
        int* s_g = reinterpret_cast<int*>(s_cls + nt + ROW_REFINE_CAP);    // [nt + CAP] the env at the position, -1 = none
        for (int p0 = 0; p0 < n; p0 += nt) {
            __syncthreads();                                  // the previous chunk has been read
            for (int i = tid; i < nt + ROW_REFINE_CAP - 1; i += nt) {
                const int p = p0 - (ROW_REFINE_CAP - 1) + i;
                int g = -1;
                int2 c = make_int2(-2, -2);
                if (p >= 0 && p < n) {
                    g = group_at(p);
                    c = make_int2(rf.rep_prev[g], row_refine_key(actions, A, g));
                }
                s_g[i] = g;
                s_cls[i] = c;
            }
            __syncthreads();
            const int i = tid + ROW_REFINE_CAP - 1;
            if (p0 + tid < n) {
                const int g = s_g[i];
                if (rep_ld(g) == ROW_REFINE_MARK) {
                    const int2 c = s_cls[i];
                    int back = 0;                             // the match furthest in front wins: earliest first
#pragma unroll 9
                    for (int d = 1; d < ROW_REFINE_CAP; ++d) {
                        const int2 c2 = s_cls[i - d];
                        if (c2.x == c.x && c2.y == c.y) back = d;
                    }
                    rep_st(g, back ? s_g[i - back] : g);
                }
            }
        }
        __syncthreads();                                      // every candidate is stored (a candidate is itself a marked group: chains)
    }
    // ---- follow chains to their roots and rebuild active / n_active (the compaction pass of k_row_dedup)
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
        for (int w2 = 0; w2 < nw; ++w2) {
            const int v = s_wave[w2];
            woff += w2 < wave ? v : 0;
            total += v;
        }
        off = woff + inc - cnt;
        __syncthreads();
    };
    int base = 0;
    for (int p0 = 0; p0 < n; p0 += nt * ROW_REFINE_PER_THREAD) {
        int gs[ROW_REFINE_PER_THREAD], rs[ROW_REFINE_PER_THREAD];
        const int q0 = p0 + tid * ROW_REFINE_PER_THREAD;
#pragma unroll
        for (int i = 0; i < ROW_REFINE_PER_THREAD; ++i) gs[i] = q0 + i < n ? group_at(q0 + i) : -1;
#pragma unroll
        for (int i = 0; i < ROW_REFINE_PER_THREAD; ++i) rs[i] = gs[i] >= 0 ? rep_ld(gs[i]) : -2;
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < ROW_REFINE_PER_THREAD; ++i) {
            if (gs[i] >= 0 && rs[i] != gs[i]) {
                int r = rs[i], r2;
                while ((r2 = rep_ld(r)) != r) r = r2;
                if (r != rs[i]) rep_st(gs[i], r);
            }
            cnt += rs[i] == gs[i];
        }
        int off, total;
        wg_scan(cnt, off, total);
        int o = base + off;
#pragma unroll
        for (int i = 0; i < ROW_REFINE_PER_THREAD; ++i)
            if (rs[i] == gs[i]) rf.active[o++] = gs[i];
        base += total;
    }
    if (tid == 0) {
        rf.cnt[0] = base;
        rf.cnt[1] = 0;
        rf.cnt[2] = 0;
    }
}

}  // namespace rl4rs
