// k_din_x: DIN attention scores of the DIEN scorer in fp16x2 form, second generation (included by dien.hip).
//
// Same arithmetic as k_din_scores<*, true> (deepctr LocalActivationUnit, rl4rs/nets/utils.py:112-119: hidden (64, 16), sigmoid,
// raw scores; layer 1 as q(W1a+W1c) [GEMM] + k_t(W1b-W1c) [cache] + (q*k_t)W1d [here], operands split into fp16 hi + lo, three
// v_mfma_f32_32x32x16_f16 per product), different machine mapping.  What bounded the first form (one row per wave, 144
// registers = 3 waves per SIMD): each wave alternated a VALU-only stretch (building the split (q*k_t) operand, the sigmoids)
// with an MFMA-only stretch, every wave pulled its own copy of the 32 KB of W1d fragments through the L1 return path, and
// the AK rows arrived in the epilogue.
//
//   * W1d fragments (32 KB, both planes) are staged ONCE per workgroup in LDS and read with ds_read_b128 right behind their
//     use; a workgroup is 8 waves and takes rows_per_wg rows (obs-sized launches: 16, so that
//     two workgroups per CU = 4 waves per SIMD cover the launch in one round, no tail; 8 when the rows the row dedup leaves
//     fit that round at one row per wave - half the workgroup life, the staging being per workgroup either way).
//   * one 32-step tile at a time (32 accumulator registers instead of 64) and no double buffers, so that the kernel fits 128
//     registers = 4 waves per SIMD, which overlap each other's VALU (operand split, sigmoids) and MFMA stretches; the cache
//     rows are requested RING k-blocks ahead.
//   * the accumulators START as AK_t + qa (the cached k-side term and the q-side GEMM term), loaded while the first operands
//     are built: no loads in the epilogue.
//   * fp16 split by v_cvt_pk_f16_f32 + v_fma_mix_f32 (split_h16_pair): 2.5 VALU instructions per element.
//   * the first-GRU states are read from a second, FRAGMENT-ORDER copy of the cache (k_h1_frag, once per encode):
//     h1f[slot][step tile n][k-block kb][lane][8 floats], lane (li, kg) = step n*32 + li, k = kb*16 + kg*8 + 0..7 - exactly
//     the 32 bytes a lane multiplies by q, so a wave's request is one contiguous 2 KB piece (16 full cache lines) instead of
//     32 lines of which it uses a quarter each; the rows of a reward group (same slot) hit in L1, no LDS tile needed.
#pragma once

#ifndef RL4RS_DINX_AB
#define RL4RS_DINX_AB 0         // timing ablations of k_din_x (results are WRONG when non-zero): 1 all rows on cache slot 0, 2 no layer-1 sigmoids
#endif

namespace rl4rs {

#ifdef RL4RS_DINX_TRACE    // s_memtime marks of workgroup (40, 0): [wave][tile 0..3 | 4 = workgroup marks][mark] (tools/dinx_trace.py)
#define DINX_TR(tile, k) do { if (a.trace && blockIdx.x == 40 && blockIdx.y == 0 && lane == 0) \
        a.trace[(wave * 5 + (tile)) * 8 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define DINX_TR(tile, k) do { } while (0)
#endif

// h1 [slot, L, E = 128] -> fragment order [slot][NT][8][64][8]; steps >= L of the last tile are zero
__global__ __launch_bounds__(256) void k_h1_frag(const float* __restrict__ h1, float* __restrict__ h1f, int slot_base, int cnt, int L) {
    const int NT = (L + 31) / 32;
    const int64_t total = (int64_t)cnt * NT * 8 * 64 * 2;          // float4 pieces
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int q4 = (int)(i & 1), lane = (int)((i >> 1) & 63), kb = (int)((i >> 7) & 7);
        const int64_t sn = i >> 10;
        const int n = (int)(sn % NT);
        const int64_t slot = slot_base + sn / NT;
        const int t = n * 32 + (lane & 31), e = kb * 16 + (lane >> 5) * 8 + q4 * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < L) v = *reinterpret_cast<const float4*>(h1 + (slot * L + t) * 128 + e);
        *reinterpret_cast<float4*>(h1f + (((slot * NT + n) * 8 + kb) * 64 + lane) * 8 + q4 * 4) = v;
    }
}

__global__ __launch_bounds__(512, RL4RS_DINX_WPE) void k_din_x(DinArgs a, int rows_per_wg, int n_cu) {
#define RL4RS_DINX_QSELF 0
#include "din_x_body.inc"
#undef RL4RS_DINX_QSELF
}

__global__ __launch_bounds__(512, RL4RS_DINX_WPE) void k_din_xq(DinArgs a, int rows_per_wg, int n_cu, DinQArgs qx) {
#define RL4RS_DINX_QSELF 1
#include "din_x_body.inc"
#undef RL4RS_DINX_QSELF
}



// Round 4, measured and dropped - "k_din_x2": both 32-step tiles of a row in one wave (one W1d fragment read feeding two tiles,
// twelve MFMAs per k-block on four accumulators, next k-block's fragments / split operands requested and built a k-block
// ahead, 172 registers = two waves per SIMD).  Bit-identical scores, but 1.15 ms per episode-batch against 0.925 ms for this
// kernel (same box): what bounds the DIN scores is VALU issue, not the LDS / cache waits the wave-level counters suggested
// (SQ_ACTIVE_INST_VALU = 42 k cycles per SIMD and obs-sized launch against 30.7 k cycles of MFMA; timing ablations: all rows on
// one cache slot -9 %, no layer-1 sigmoids -4 %), and eight waves per CU overlap the two pipes worse than sixteen.
// A finding worth keeping from that attempt: split_h16_pair is INLINE ASM, invisible to the compiler's MFMA hazard recogniser.
// With double-buffered operands the register allocator gave a just-dead MFMA B-operand register to the next asm conversion
// issued right behind that MFMA, and the 8-pass v_mfma_f32_32x32x16_f16 was still reading it: wrong scores in 4-lane groups
// (tests/test_gpu_dien.py::test_dien_rowwise_matches_oracle caught it).  In this kernel every asm definition sits behind an LDS
// or cache wait; keep it that way, or write the split with compiler-visible conversions where a definition can follow an MFMA.
//
// Round 5, measured and dropped (same-box A/Bs of the DIN ms per episode-batch; head = this kernel, 0.90 ms):
//   * the ring of first-GRU states 3 / 4 / 8 k-blocks deep instead of 2: 0.909 / 0.919 / (18 spills); the ring running ACROSS tiles and
//     rows (the slots freed by a tile's last k-blocks take the next tile's first ones): 0.908.  The s_memtime marks
//     (tools/dinx_trace.py, -DRL4RS_DINX_TRACE) do show 1 - 4 k cycles of waiting at every tile start on a workload with 4096
//     distinct histories (HBM-bound there: 537 MB per launch), but on the bench's sharing (1 771 distinct, duplicates adjacent) the
//     wait only moves into the first k-blocks: a tile is ~4 k cycles of requests + first operand, ~10.5 k of k loop (1.3 k per
//     k-block), 2.3 k of epilogue whichever way the requests are arranged; workgroup life 85 - 95 k cycles of which 11 k staging.
//   * W1d's hi planes (or both planes) resident in registers, two waves per SIMD, 32 rows per workgroup (4 instead of 6 / 2
//     instead of 6 ds_read_b128 per k-block): 1.01 / 0.99 ms - fewer LDS reads do not pay for half the waves.
//   So the k loop runs at ~325 cycles per wave and k-block on a SIMD whose matrix pipe needs 192, whose VALU ~160 and whose LDS
//   issue ~120 for it: three comparably loaded resources overlapping at ~60 %, four waves per SIMD being what makes them overlap
//   at all.  Neither more bytes in flight nor fewer LDS reads nor fewer, fatter waves moves it.

inline size_t din_x_smem() { return 40960 + 48 * 4 + (size_t)8 * (128 + ATT_H1) * 4; }

}  // namespace rl4rs
