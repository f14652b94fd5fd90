// The tile body of k_gemm_h16 and k_gemm_h16_pair (gemm.hip), included into both kernels as TEXT so that k_gemm_h16 compiles to
// exactly the code it had as a single kernel.  Expects in scope: WM, VEC; A, lda, Wp, KB, bias, C, ldc, M, N, K, act, addend,
// ldadd, chain (all wave-uniform) and RL4RS_G16_BX = the workgroup's row-tile index within its problem (RL4RS_G16_BY, optional: its column-group
// index instead of blockIdx.y; RL4RS_G16_AS_LDS, optional: where the tile buffers lie instead of in static LDS); MAP (constexpr bool), rmap
// (G16RowMap) and s_row (int[BM] in LDS when MAP).  MAP = false (k_gemm_h16, k_gemm_h16_pair): every `if constexpr (MAP)` below is
// no code and the kernels compile to the instruction text they had without it.  MAP = true (k_gemm_h16_map, k_gemm_h16_pair_map;
// DESIGN 25): tile position p works on physical row active[p / group] * group + p % group of A, C, c2 and the addend, the row
// bound is min(M, n_active * group) read here, a workgroup whose first position lies behind it leaves before its first barrier,
// positions of a partial last tile behind the bound recompute the last active row and store nothing.  Per output element the
// k-blocks, the MFMA order and the epilogue expression are those of the unmapped form.
// RL4RS_G16_GATHER (optional, with MAP; k_gemm_h16_gather, DESIGN 31; no chain): rmap.active is the REPRESENTATIVE map of all M
// rows (group 1) - tile position p reads row active[p] of A and of the addend and writes row p of C, the row bound is M itself.
    constexpr int BM = 32 * WM, BK = 64, KBT = BK / 16;
    constexpr int SLAB = BM * 16 + 16, PLANE = 2 * KBT * SLAB;
#ifdef RL4RS_G16_AS_LDS        // the shadow plane of k_augru_xs: the tile buffers are a piece of the launch's dynamic LDS
    char (*const As)[2][PLANE] = reinterpret_cast<char (*)[2][PLANE]>(RL4RS_G16_AS_LDS);
#else
    __shared__ __attribute__((aligned(16))) char As[2][2][PLANE];          // [buffer][hi / lo]
#endif
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, li = lane & 31;
    const int m0 = RL4RS_G16_BX * BM;
    int Mb = M;
    int arow[WM];                                  // MAP: the physical rows of this thread's A chunks
    if constexpr (MAP) {
        // the list entries of this thread's positions are requested BESIDE the bound, not behind it (the list is allocated for
        // every group; entries behind n_active are stale and then unused): one memory round trip in front of the first A tile
        int apos[WM], agrp[WM], aent[WM];
#pragma unroll
        for (int p = 0; p < WM; ++p) {
            apos[p] = min(m0 + ((tid + p * 256) >> 3), M - 1);
            agrp[p] = rmap.group == 1 ? apos[p] : apos[p] / rmap.group;
            aent[p] = rmap.active[agrp[p]];
        }
#ifdef RL4RS_G16_GATHER
        Mb = M;
#else
        Mb = min(M, rmap.n_active[0] * rmap.group);
#endif
        if (m0 >= Mb) return;
#pragma unroll
        for (int p = 0; p < WM; ++p) {
            if (apos[p] >= Mb) {                   // a position behind the bound (partial last tile only): the last active row
                apos[p] = Mb - 1;
                agrp[p] = apos[p] / rmap.group;
                aent[p] = rmap.active[agrp[p]];
            }
            arow[p] = aent[p] * rmap.group + (apos[p] - agrp[p] * rmap.group);
            if ((tid & 7) == 0) s_row[(tid + p * 256) >> 3] = arow[p];       // for the epilogue, behind the main loop's barriers
        }
    }
#ifndef RL4RS_G16_BY
#define RL4RS_G16_BY blockIdx.y
#endif
    const int nt = RL4RS_G16_BY * 4 + wave;
    const int NT = (N + 31) / 32;
    const bool tile_ok = nt < NT;
    const int col = nt * 32 + li;
    const char* wtile = Wp + (size_t)(tile_ok ? nt : 0) * KB * 2048;
    const float inv_s = reinterpret_cast<const float*>(Wp)[(size_t)NT * KB * 512 + (tile_ok ? col : 0)];     // 1 / (this column's power-of-two prescale)
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(wtile), 0, KB * 2048, 0x00020000);
    const int vl16 = lane * 16;

    f32x16 acc[WM];
#pragma unroll
    for (int w = 0; w < WM; ++w)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[w][i] = 0.f;

    // A tiles in flight: 2 register stages of 8 consecutive k of one row per chunk.  WEIGHT fragments: a ring of NB k-tiles
    // (measured: with one tile of lookahead a 32-row launch waited ~1 us of L2 latency per k-tile - 17 us for the head's 12
    // k-tiles of 2.4 us of MFMA work; requesting the A tiles deeper changed nothing).  32-row tiles (small launches, one or
    // two workgroups per CU) keep 4 k-tiles of fragments in flight, 64-row tiles 2.
    constexpr int NS = 2, NB = WM == 1 ? 4 : 2;
    float4 stage[NS][WM][2];
    // A through a buffer descriptor over this workgroup's rows: rows >= M and everything past the last element read as
    // zero, so the loads are UNCONDITIONAL (no divergent branches: the compiler keeps every requested tile in flight and
    // waits with exact counts; guarded loads had forced a full drain of the weight ring at every k-tile); columns >= K of
    // a row (they exist when lda > K) are cleared with selects
    const int rows_here = min(BM, M - m0);
    // (MAP: the descriptor spans all M rows, the launcher has checked that they fit its 32-bit offsets)
    const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(A + (size_t)(MAP ? 0 : m0) * lda), 0, (int)((((int64_t)(MAP ? M : rows_here) - 1) * lda + K) * 4), 0x00020000);
    auto gload = [&](float4 (&st)[WM][2], int kt) {
#pragma unroll
        for (int p = 0; p < WM; ++p) {
            const int c = tid + p * 256;
            const int r = MAP ? arow[p] : c >> 3, gk = kt * BK + (c & 7) * 8;
            const int voff = (int)(((int64_t)r * lda + gk) * 4);
            float x[8];
            if (VEC) {
                const float4 v0 = gbuf_load4(rs_a, voff, 0), v1 = gbuf_load4(rs_a, voff + 16, 0);
                x[0] = v0.x; x[1] = v0.y; x[2] = v0.z; x[3] = v0.w; x[4] = v1.x; x[5] = v1.y; x[6] = v1.z; x[7] = v1.w;
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_a, voff + e * 4, 0, 0));
            }
            st[p][0] = make_float4(x[0], x[1], x[2], x[3]);        // raw: the K-tail selects wait for the data, so they run in lstore
            st[p][1] = make_float4(x[4], x[5], x[6], x[7]);
        }
    };
    auto lstore = [&](const float4 (&st)[WM][2], int buf, int kt) {
#pragma unroll
        for (int p = 0; p < WM; ++p) {
            const int c = tid + p * 256;
            const int off = (c & 7) * SLAB + (c >> 3) * 16;
            const int gk = kt * BK + (c & 7) * 8;
            float x[8] = {st[p][0].x, st[p][0].y, st[p][0].z, st[p][0].w, st[p][1].x, st[p][1].y, st[p][1].z, st[p][1].w};
            if (gk + 7 >= K) {                   // only the last k-tile of a K that is not a multiple of 8 has such a chunk
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] = (gk + e < K) ? x[e] : 0.f;
            }
            ghalf8_t hi, lo;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const _Float16 h = (_Float16)x[e];
                hi[e] = h;
                lo[e] = (_Float16)(x[e] - (float)h);
            }
            *reinterpret_cast<ghalf8_t*>(&As[buf][0][off]) = hi;
            *reinterpret_cast<ghalf8_t*>(&As[buf][1][off]) = lo;
        }
    };
    ghalf8_t bh[NB][KBT], bl[NB][KBT];
    auto load_b = [&](ghalf8_t (&h)[KBT], ghalf8_t (&l)[KBT], int kt) {
#pragma unroll
        for (int j = 0; j < KBT; ++j) {
            h[j] = gbuf_load_h8(rs_w, vl16, (kt * KBT + j) * 2048);
            l[j] = gbuf_load_h8(rs_w, vl16 + 1024, (kt * KBT + j) * 2048);
        }
    };
    auto compute = [&](const ghalf8_t (&h)[KBT], const ghalf8_t (&l)[KBT], int buf) {
#pragma unroll
        for (int j = 0; j < KBT; ++j) {
            ghalf8_t ah[WM], al[WM];
#pragma unroll
            for (int w = 0; w < WM; ++w) {
                const int off = (j * 2 + half) * SLAB + (w * 32 + li) * 16;
                ah[w] = *reinterpret_cast<const ghalf8_t*>(&As[buf][0][off]);
                al[w] = *reinterpret_cast<const ghalf8_t*>(&As[buf][1][off]);
            }
#pragma unroll
            for (int w = 0; w < WM; ++w) acc[w] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[w], h[j], acc[w], 0, 0, 0);
#pragma unroll
            for (int w = 0; w < WM; ++w) acc[w] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[w], h[j], acc[w], 0, 0, 0);
#pragma unroll
            for (int w = 0; w < WM; ++w) acc[w] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[w], l[j], acc[w], 0, 0, 0);
        }
    };

    const int nkt = (K + BK - 1) / BK;
#pragma unroll
    for (int i = 0; i < NS; ++i) gload(stage[i], i);
#pragma unroll
    for (int i = 0; i < NB - 1; ++i) load_b(bh[i], bl[i], i);
    lstore(stage[0], 0, 0);
    __syncthreads();
    // at the top of step kt: LDS[kt&1] = tile kt, stage[(kt+1)&1] = tile kt+1 (in flight), stage[kt&1] free,
    // bh/bl[kt%NB .. (kt+NB-2)%NB] = fragments of tiles kt .. kt+NB-2 (in flight)
    for (int kt0 = 0; kt0 < nkt; kt0 += NB) {
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int kt = kt0 + i;
            if (kt < nkt) {
                gload(stage[i & 1], kt + NS);           // A first: its wait (in-order counter) must not cover the newest B tile
                load_b(bh[(i + NB - 1) % NB], bl[(i + NB - 1) % NB], kt + NB - 1);
                compute(bh[i], bl[i], i & 1);
                lstore(stage[(i & 1) ^ 1], (i & 1) ^ 1, kt + 1);
                __syncthreads();
            }
        }
    }
    if (chain.wp2) {        // uniform: chained second layer (gridDim.y == 1, N <= 128, N % 16 == 0: checked by the launcher)
        const int NT2 = (chain.n2 + 31) / 32;
        const bool tile2_ok = wave < NT2;
        const float inv_s2 = reinterpret_cast<const float*>(chain.wp2)[(size_t)NT2 * chain.kb2 * 512 + (tile2_ok ? wave * 32 + li : 0)];
        const __amdgpu_buffer_rsrc_t rs_w2 = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<char*>(chain.wp2 + (size_t)(tile2_ok ? wave : 0) * chain.kb2 * 2048), 0, chain.kb2 * 2048, 0x00020000);
        ghalf8_t b2h[8], b2l[8];                       // K2 <= 128: every fragment of the second layer requested up front
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            b2h[j] = gbuf_load_h8(rs_w2, vl16, j * 2048);
            b2l[j] = gbuf_load_h8(rs_w2, vl16 + 1024, j * 2048);
        }
        char* p_hi = &As[0][0][0];                     // the main loop's last barrier has passed: its tiles are dead
        char* p_lo = p_hi + 16 * SLAB;                 // 16 slabs (k / 8) per plane = exactly the two tile buffers
        if (tile_ok) {
            const float bv = (bias && col < N) ? bias[col] : 0.f;
#pragma unroll
            for (int w = 0; w < WM; ++w)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rl = 32 * w + (r & 3) + 8 * (r >> 2) + 4 * half;
                    const float v = (col < N && m0 + rl < M) ? apply_act(acc[w][r] * inv_s + bv, act) : 0.f;
                    const _Float16 hi = (_Float16)v;
                    const int off = (col >> 3) * SLAB + rl * 16 + (col & 7) * 2;
                    *reinterpret_cast<_Float16*>(p_hi + off) = hi;
                    *reinterpret_cast<_Float16*>(p_lo + off) = (_Float16)(v - (float)hi);
                }
        }
        __syncthreads();
        f32x16 acc2[WM];
#pragma unroll
        for (int w = 0; w < WM; ++w)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc2[w][i] = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j < chain.kb2) {
#pragma unroll
                for (int w = 0; w < WM; ++w) {
                    const int off = (j * 2 + half) * SLAB + (w * 32 + li) * 16;
                    const ghalf8_t ah = *reinterpret_cast<const ghalf8_t*>(p_hi + off);
                    const ghalf8_t al = *reinterpret_cast<const ghalf8_t*>(p_lo + off);
                    acc2[w] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, b2h[j], acc2[w], 0, 0, 0);
                    acc2[w] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, b2h[j], acc2[w], 0, 0, 0);
                    acc2[w] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, b2l[j], acc2[w], 0, 0, 0);
                }
            }
        }
        const int col2 = wave * 32 + li;
        if constexpr (MAP) {
            if (tile2_ok && col2 < chain.n2) {
                const float bv2 = chain.bias2 ? chain.bias2[col2] : 0.f;
                const __amdgpu_buffer_rsrc_t rs_c2 = __builtin_amdgcn_make_buffer_rsrc(chain.c2, 0, (int)((((int64_t)M - 1) * chain.ldc2 + chain.n2) * 4), 0x00020000);
#pragma unroll
                for (int w = 0; w < WM; ++w)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int rl = 32 * w + (r & 3) + 8 * (r >> 2) + 4 * half;
                        if (m0 + rl < Mb)
                            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, apply_act(acc2[w][r] * inv_s2 + bv2, chain.act2)), rs_c2,
                                                                  (s_row[rl] * (int)chain.ldc2 + col2) * 4, 0, 0);
                    }
            }
            return;
        }
        if (tile2_ok && col2 < chain.n2) {
            const float bv2 = chain.bias2 ? chain.bias2[col2] : 0.f;
            const __amdgpu_buffer_rsrc_t rs_c2 = __builtin_amdgcn_make_buffer_rsrc(chain.c2 + (size_t)m0 * chain.ldc2, 0,
                                                                                   (int)((((int64_t)rows_here - 1) * chain.ldc2 + chain.n2) * 4), 0x00020000);
            const int l24 = (int)chain.ldc2 * 4, v2 = (4 * half * (int)chain.ldc2 + col2) * 4;
#pragma unroll
            for (int w = 0; w < WM; ++w)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, apply_act(acc2[w][r] * inv_s2 + bv2, chain.act2)), rs_c2, v2,
                                                          (32 * w + (r & 3) + 8 * (r >> 2)) * l24, 0);
        }
        return;
    }
    if (tile_ok && col < N) {
        // C (and the addend) through buffer descriptors over this workgroup's valid rows: rows >= M are dropped (read as zero) by
        // the hardware and the row part of an address is a scalar - one instruction per element instead of a compare, an exec
        // mask and a 64-bit address (see k_gemm_h16_wres: that VALU work was comparable to the tile's MFMA time)
        const float bv = bias ? bias[col] : 0.f;
        if constexpr (MAP) {                       // (no mirror in this form: the launcher keeps such launches unmapped)
            const __amdgpu_buffer_rsrc_t rs_c = __builtin_amdgcn_make_buffer_rsrc(C, 0, (int)((((int64_t)M - 1) * ldc + N) * 4), 0x00020000);
#ifdef RL4RS_G16_GATHER                            // the C row of tile row rl: the position itself / the physical row its A row came from
#define RL4RS_G16_CROW(rl) (m0 + (rl))
#else
#define RL4RS_G16_CROW(rl) s_row[rl]
#endif
            float add[WM][16];
            if (addend) {
                const __amdgpu_buffer_rsrc_t rs_d = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(addend), 0, (int)((((int64_t)M - 1) * ldadd + N) * 4), 0x00020000);
#pragma unroll
                for (int w = 0; w < WM; ++w)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        add[w][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                            rs_d, (s_row[32 * w + (r & 3) + 8 * (r >> 2) + 4 * half] * (int)ldadd + col) * 4, 0, 0));
            } else {
#pragma unroll
                for (int w = 0; w < WM; ++w)
#pragma unroll
                    for (int r = 0; r < 16; ++r) add[w][r] = 0.f;
            }
#pragma unroll
            for (int w = 0; w < WM; ++w)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rl = 32 * w + (r & 3) + 8 * (r >> 2) + 4 * half;
                    if (m0 + rl < Mb)
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, apply_act(acc[w][r] * inv_s + bv + add[w][r], act)), rs_c,
                                                              (RL4RS_G16_CROW(rl) * (int)ldc + col) * 4, 0, 0);
                }
#undef RL4RS_G16_CROW
            return;
        }
        const __amdgpu_buffer_rsrc_t rs_c = __builtin_amdgcn_make_buffer_rsrc(C + (size_t)m0 * ldc, 0, (int)((((int64_t)rows_here - 1) * ldc + N) * 4), 0x00020000);
        const int ldc4 = (int)ldc * 4, c_voff = (4 * half * (int)ldc + col) * 4;
        if (addend) {
            const __amdgpu_buffer_rsrc_t rs_d = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(addend + (size_t)m0 * ldadd), 0,
                                                                                  (int)((((int64_t)rows_here - 1) * ldadd + N) * 4), 0x00020000);
            const int ldd4 = (int)ldadd * 4, d_voff = (4 * half * (int)ldadd + col) * 4;
            float add[WM][16];
#pragma unroll
            for (int w = 0; w < WM; ++w)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    add[w][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_d, d_voff, (32 * w + (r & 3) + 8 * (r >> 2)) * ldd4, 0));
#pragma unroll
            for (int w = 0; w < WM; ++w)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, apply_act(acc[w][r] * inv_s + bv + add[w][r], act)), rs_c, c_voff,
                                                          (32 * w + (r & 3) + 8 * (r >> 2)) * ldc4, 0);
        } else {
#pragma unroll
            for (int w = 0; w < WM; ++w)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, apply_act(acc[w][r] * inv_s + bv + 0.f, act)), rs_c, c_voff,
                                                          (32 * w + (r & 3) + 8 * (r >> 2)) * ldc4, 0);
        }
        if (chain.mirror) {
            // the same values (recomputed from the registers: same expression, same bits) to the host block
            const __amdgpu_buffer_rsrc_t rs_m = __builtin_amdgcn_make_buffer_rsrc(chain.mirror + (size_t)m0 * chain.ldm, 0,
                                                                                  (int)((((int64_t)rows_here - 1) * chain.ldm + N) * 4), 0x00020000);
            const int ldm4 = (int)chain.ldm * 4, m_voff = (4 * half * (int)chain.ldm + col) * 4;
            if (addend) {
                const __amdgpu_buffer_rsrc_t rs_d = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(addend + (size_t)m0 * ldadd), 0,
                                                                                      (int)((((int64_t)rows_here - 1) * ldadd + N) * 4), 0x00020000);
                const int ldd4 = (int)ldadd * 4, d_voff = (4 * half * (int)ldadd + col) * 4;
#pragma unroll
                for (int w = 0; w < WM; ++w)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float ad = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_d, d_voff, (32 * w + (r & 3) + 8 * (r >> 2)) * ldd4, 0));
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, apply_act(acc[w][r] * inv_s + bv + ad, act)), rs_m, m_voff,
                                                              (32 * w + (r & 3) + 8 * (r >> 2)) * ldm4, 0);
                    }
            } else {
#pragma unroll
                for (int w = 0; w < WM; ++w)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, apply_act(acc[w][r] * inv_s + bv + 0.f, act)), rs_m, m_voff,
                                                              (32 * w + (r & 3) + 8 * (r >> 2)) * ldm4, 0);
            }
        }
    }
