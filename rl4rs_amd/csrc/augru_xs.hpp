// k_augru_xs: k_augru_x's observation-sized 32-row form with a shadow plane (included by augru_xs.hip; dien.hip takes the argument block).
#pragma once
#include "common.hpp"
#include "recur_args.hpp"
#include "cat_attn2_row.hpp"
#include "gemm_h16_defs.hpp"
#include "augru_x.hpp"

namespace rl4rs {

// -------------------------------------------------------------------------------------------------
// k_augru_xs: the observation-sized 32-row launch with a SHADOW PLANE.  An observation-sized launch after the row dedup is
// ~110 workgroups x S on 256 CUs, each bound by its own 64-step chain: the other CUs idle for the whole launch.  The part of an
// observation forward that only the head GEMM reads - category self-attention, pooled row and head-table sum (k_cat_attn2<21, true>),
// both layers of the dense tower (the chain form of k_gemm_h16_map<1>) - runs there: grid (tiles, S + 1), the workgroups of plane
// blockIdx.y == S never touch the recurrence.  Shadow workgroup x takes positions 32 x .. 32 x + 31 of the active list (the tile
// the recurrence workgroups (x, 0 .. S - 1) work on):
//   1. eight waves, four positions each, one row at a time through cat_attn2_row (cat_attn2_row.hpp: the text of k_cat_attn2, 5.8 KB
//      of LDS per wave); positions behind the active rows are skipped;
//   2. waves 4 - 7 end; waves 0 - 3 - from here on a 256-thread workgroup, a barrier counts the waves that have not ended - run the
//      tile text of k_gemm_h16 (gemm_h16_tile.inc, WM = 1, MAP, chained) on the tile's rows of the dense features.
// Same operation sequence per element as the two kernels it replaces, so allf and tsum keep their bits.  A shadow workgroup behind
// n_active leaves before its first barrier, it never synchronises with another workgroup, and the kernel boundary in front of
// the head GEMM orders its stores.  It is dispatched behind the recurrence workgroups (higher linear id) and holds a whole CU
// (the launch's dynamic LDS): the host launches this form only where tiles * (S + 1) workgroups fit the chip.
struct AugruShadowArgs {
    // category branch (the arguments of k_cat_attn2<21, true>)
    const int32_t* cat; int Cn, H; const float* cat_emb; const float* seq_emb; float* allf; int ldf, off_c; float* q; int write_flat, h16;
    const float* ptab; const float* obs_b; float* tsum;
    // dense tower (the arguments of k_gemm_h16_map<1, VEC>, chained)
    const float* dense; int64_t lda; const char* w1; int kb1; const float* b1; int N1, K1, act1, vec; G16Chain chain;
    int R; G16RowMap rmap;       // rows of the forward and its active list (group == 1)
};

constexpr int XS_CAT_LDS = (21 * (64 + 4) + 32) * 4;          // per wave (k_cat_attn2)
constexpr int XS_TILE_LDS = 8 * XS_CAT_LDS;                   // the GEMM tile buffers (2 x 2 planes of 4224 bytes), then s_row[32]

template <bool VEC>
__device__ __forceinline__ void augru_shadow_dense(const AugruShadowArgs& sh, char* lds) {
    constexpr int WM = 1;
    constexpr bool MAP = true;
    const float* __restrict__ A = sh.dense; const int64_t lda = sh.lda; const char* __restrict__ Wp = sh.w1; const int KB = sh.kb1;
    const float* __restrict__ bias = sh.b1; float* __restrict__ C = nullptr; const int64_t ldc = 0;
    const int M = sh.R, N = sh.N1, K = sh.K1, act = sh.act1;
    const float* __restrict__ addend = nullptr; const int64_t ldadd = 0; const G16Chain chain = sh.chain;
    const G16RowMap rmap = sh.rmap;
    int* const s_row = reinterpret_cast<int*>(lds + XS_TILE_LDS + 4 * 4224);
#define RL4RS_G16_BX blockIdx.x
#define RL4RS_G16_BY 0
#define RL4RS_G16_AS_LDS (lds + XS_TILE_LDS)
#include "gemm_h16_tile.inc"
#undef RL4RS_G16_AS_LDS
#undef RL4RS_G16_BY
#undef RL4RS_G16_BX
}

__device__ __forceinline__ void augru_shadow_plane(const AugruShadowArgs& sh) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_act = min(sh.R, sh.rmap.n_active[0]);
    const int p0 = blockIdx.x * 32;
    if (p0 >= n_act) return;
    float* sE = reinterpret_cast<float*>(smem + wave * XS_CAT_LDS);
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
        const int p = p0 + wave * 4 + i;
        if (p >= n_act) break;
        const int row = sh.rmap.active[p];
        cat_attn2_row<21, true>(sE, row, lane, sh.cat, sh.Cn, sh.H, sh.cat_emb, sh.seq_emb, sh.allf, sh.ldf, sh.off_c, sh.q, sh.write_flat, sh.h16,
                                sh.ptab, sh.obs_b, sh.tsum);
        __builtin_amdgcn_wave_barrier();           // the next row rewrites this wave's image
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    if (wave >= 4) return;
    if (sh.vec) augru_shadow_dense<true>(sh, smem);
    else augru_shadow_dense<false>(sh, smem);
}

template <bool PAD>
__global__ __launch_bounds__(512) void k_augru_xs(RecurArgs a, AugruShadowArgs sh) {
    if (blockIdx.y + 1 == gridDim.y) { augru_shadow_plane(sh); return; }
    constexpr int MT = 1, NRES = RL4RS_X_NRES, RING = RL4RS_X_RING, GRP = 8;
#include "augru_x_body.inc"
}

}  // namespace rl4rs
