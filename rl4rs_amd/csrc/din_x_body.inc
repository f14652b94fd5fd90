// The text of k_din_x (din_x.hpp), included into k_din_x (RL4RS_DINX_QSELF 0: the kernel as it was) and into k_din_xq (1, DESIGN 26:
// the workgroup forms the query row q and the q-side term qa = q W1ac of its own rows instead of reading what the category kernel
// and the q-side GEMM left - see "QSELF" in the row loop).  Expects in scope: DinArgs a, rows_per_wg, n_cu and, with QSELF, DinQArgs qx.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int E = 128, KB = 8, NW = 8;
    const int L = a.L;
    const int sq = blockIdx.y;
    // row dedup (row_dedup.hpp): only the first n_active entries of a.order are scored; the grid is sized for a.R on the host
    const int n_rows = a.n_active ? min(a.R, a.n_active[0] * a.group) : a.R;
    // n_cu > 0 (group == 1 launches, grid sized for 8 rows per workgroup): one row per wave while that still fits one round of two
    // workgroups per CU, otherwise two rows per wave as before; decided here because the row count is a device value.  A row's
    // arithmetic does not depend on the mapping.
    if (n_cu > 0) rows_per_wg = ((n_rows + 7) / 8) * (int)gridDim.y <= 2 * n_cu ? 8 : 16;
    if (blockIdx.x * rows_per_wg >= n_rows) return;
    char* s_w1 = smem;                                                 // [(m*8 + kb)*2 + plane][lane][8 halfs]: 32 KB
    char* s_w2b = smem + 32768;                                         // [(m*2 + kb2)*2 + plane][lane][8 halfs]: 8 KB
    float* s_misc = reinterpret_cast<float*>(smem + 40960);             // b2[16] w3[16] b3 pad -> 48
    float* s_wave = s_misc + 48;                                        // per wave: q[E] + qa[64]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, li = lane & 31;
    DINX_TR(4, 0);
    {
        // staging: every request of the workgroup's 40 KB of weights goes out before the first is stored.  (As two plain loops the
        // ISA was "load, s_waitcnt vmcnt(0), store" per iteration: eight serialised memory round trips = 11 k of a workgroup's
        // ~88 k cycles, tools/dinx_trace.py.)  W2 entries beyond the 16 real output units read a clamped address and are zeroed.
        // (ext_vector_type, not HIP's uint4 struct: a struct copied out of global memory is a memcpy the optimiser leaves in scratch)
        typedef float stage4_t __attribute__((ext_vector_type(4)));
        const stage4_t* src = reinterpret_cast<const stage4_t*>(a.w1d16[sq]);
        stage4_t* dst = reinterpret_cast<stage4_t*>(s_w1);
        stage4_t wv[4];
        float w2v[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) wv[p] = src[tid + p * 512];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int i = tid + p * 512, e = i & 7, ln = (i >> 3) & 63, f = i >> 9, o = ln & 31;
            w2v[p] = a.w2[sq][((f >> 1) * 32 + crow((f & 1) * 8 + e, ln >> 5)) * ATT_H2 + min(o, ATT_H2 - 1)];
        }
        float m0 = 0.f, m1 = 0.f, m2 = 0.f;
        if (tid < ATT_H2) { m0 = a.b2[sq][tid]; m1 = a.w3[sq][tid]; }
        if (tid == 0) m2 = a.b3[sq][0];
#pragma unroll
        for (int p = 0; p < 4; ++p) dst[tid + p * 512] = wv[p];
        _Float16* s_w2h = reinterpret_cast<_Float16*>(s_w2b);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int i = tid + p * 512, e = i & 7, ln = (i >> 3) & 63, f = i >> 9, o = ln & 31;
            const float v = o < ATT_H2 ? w2v[p] : 0.f;
            const _Float16 hi = (_Float16)v;
            s_w2h[(f * 2) * 512 + ln * 8 + e] = hi;
            s_w2h[(f * 2 + 1) * 512 + ln * 8 + e] = (_Float16)(v - (float)hi);
        }
        if (tid < ATT_H2) { s_misc[tid] = m0; s_misc[16 + tid] = m1; }
        if (tid == 0) s_misc[32] = m2;
    }
    __syncthreads();
    DINX_TR(4, 1);
    float* s_q = s_wave + (size_t)wave * (E + ATT_H1);
    float* s_qa = s_q + E;
    const int ntile = (L + 31) / 32;
    const int grp = a.group;

    for (int j = wave; j < rows_per_wg; j += NW) {
        // row groups (rows that share a cache slot) in the caller's processing order, rows of a group consecutive
        const int idx = blockIdx.x * rows_per_wg + j;
        if (idx >= n_rows) break;
        const int g = idx / grp;
        // the duplicates of this row's group (row_dedup.hpp): their rows take the score where the row's own is stored.  Requested
        // with the order entry, first looked at behind the first tile
        int dup0 = 0, dup1 = 0;
        if (a.dup_start) { dup0 = a.dup_start[g]; dup1 = a.dup_start[g + 1]; }
        const int gs = a.order ? a.order[g] : g;
        const int row = gs * grp + (idx - g * grp);
#if RL4RS_DINX_AB & 1       // timing ablation (results WRONG): every row reads cache slot 0 - the cache traffic becomes L1 / L2 hits
        const int slot = 0 * a.slots[(size_t)sq * a.slots_stride + gs];
#else
        const int slot = a.slots[(size_t)sq * a.slots_stride + gs];
#endif
        const int lead = a.lead[sq] ? a.lead[sq][slot] : 0;
        __builtin_amdgcn_wave_barrier();
        // the row's q and q-side term are requested here and staged in LDS inside the first tile, behind that tile's own
        // requests: one memory round trip at the start of a row instead of two
#if !RL4RS_DINX_QSELF
        const float q_lo = a.q[(size_t)row * E + lane], q_hi = a.q[(size_t)row * E + lane + 64];
        const float qa_v = a.qa[(size_t)sq * a.qa_stride + (size_t)row * a.qa_ld + lane];
#else
        {
            // ---- QSELF.  q = mean of the sequence-embedding rows of the row's last ten category ids, in the operation order of the
            // category kernel (cat_attn2_row: ids clamped, ten rows summed in id order from 0, times 1 / 10); lane e holds columns
            // e and e + 64.  The plane sq == 0 stores it (rl4rs_dien_buffer, k_row_expand and the head's readers see a complete q).
            const int Cn = qx.Cn;
            const int myid = (lane < Cn) ? min(max(qx.cat[(size_t)row * Cn + lane], 0), qx.H - 1) : 0;
            float qv0[10], qv1[10];
#pragma unroll
            for (int u = 0; u < 10; ++u) {
                const float* src = qx.seq_emb + (size_t)__builtin_amdgcn_readlane(myid, Cn - 10 + u) * E;
                qv0[u] = src[lane];
                qv1[u] = src[lane + 64];
            }
            float q0 = 0.f, q1 = 0.f;
#pragma unroll
            for (int u = 0; u < 10; ++u) { q0 += qv0[u]; q1 += qv1[u]; }
            const float invq = 1.f / 10.f;
            const float q_lo = q0 * invq, q_hi = q1 * invq;
            if (sq == 0) {
                qx.q_out[(size_t)row * E + lane] = q_lo;
                qx.q_out[(size_t)row * E + lane + 64] = q_hi;
            }
            s_q[lane] = q_lo;
            s_q[lane + 64] = q_hi;
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            // qa = q W1ac for this plane's 64 hidden units: the tile of k_gemm_h16 (gemm_h16_tile.inc) with the row at tile row 0
            // and zeros in the other 31 - per output element the same k-blocks (0 .. 7), the same three products per k-block in
            // the same order (A_hi W_hi, A_lo W_hi, A_hi W_lo), the same split of the A operand (C++ conversions) and the same
            // epilogue expression, so the same bits as the q-side half of k_gemm_h16_pair_map<1>.  Column tile m of this plane is
            // tile sq * 2 + m of the packed weights; register 0 of lane li (half 0) is tile row 0, column li.
            const int NTq = (int)gridDim.y * 2;
            const __amdgpu_buffer_rsrc_t rs_wq = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(qx.w1ac_all), 0, NTq * KB * 2048, 0x00020000);
            f32x16 qacc[2];
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) qacc[m][r] = 0.f;
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                half8_t wqh[2], wql[2];
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    wqh[m] = buf_load_h8(rs_wq, lane * 16, ((sq * 2 + m) * KB + kb) * 2048);
                    wql[m] = buf_load_h8(rs_wq, lane * 16 + 1024, ((sq * 2 + m) * KB + kb) * 2048);
                }
                float4 f0 = make_float4(0.f, 0.f, 0.f, 0.f), f1 = f0;
                if (li == 0) {
                    f0 = *reinterpret_cast<const float4*>(s_q + kb * 16 + half * 8);
                    f1 = *reinterpret_cast<const float4*>(s_q + kb * 16 + half * 8 + 4);
                }
                const float x[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
                half8_t ah, al;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const _Float16 h = (_Float16)x[e];
                    ah[e] = h;
                    al[e] = (_Float16)(x[e] - (float)h);
                }
#pragma unroll
                for (int m = 0; m < 2; ++m) qacc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, wqh[m], qacc[m], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < 2; ++m) qacc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, wqh[m], qacc[m], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < 2; ++m) qacc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, wql[m], qacc[m], 0, 0, 0);
            }
            const float* inv_sq = reinterpret_cast<const float*>(qx.w1ac_all) + (size_t)NTq * KB * 512 + sq * 64;
            const float qa0 = qacc[0][0] * inv_sq[li] + 0.f + 0.f, qa1 = qacc[1][0] * inv_sq[32 + li] + 0.f + 0.f;
            if (half == 0) {
                s_qa[li] = qa0;
                s_qa[32 + li] = qa1;
                qx.qa_out[(size_t)row * a.qa_ld + sq * 64 + li] = qa0;
                qx.qa_out[(size_t)row * a.qa_ld + sq * 64 + 32 + li] = qa1;
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_sched_barrier(0);
        }
#endif
        const float* qp = s_q + half * 8;

        for (int n = 0; n < ntile; ++n) {
            DINX_TR((j / NW) * 2 + n, 0);
            const int t = n * 32 + li;
            const int tc = min(t, L - 1);                  // steps >= L re-read the last row (results never stored)
            const int slot_t = t < lead ? a.pad_slot : slot;      // (a lane = a step of the tile: front padding comes from the pad slot)
            const float* hp = a.h1f[sq] + (((size_t)slot_t * ntile + n) * KB * 64 + lane) * 8;
            const float* akp = a.proj[sq] + ((size_t)slot_t * L + tc) * a.pld;
            float4 hr[RL4RS_DINX_RING][2];
            auto ldh = [&](int s, int kb) {
                hr[s][0] = *reinterpret_cast<const float4*>(hp + kb * 512);
                hr[s][1] = *reinterpret_cast<const float4*>(hp + kb * 512 + 4);
            };
            half8_t wh[2], wl[2];
            auto ldw = [&](int m, int kb) {
                wh[m] = *reinterpret_cast<const half8_t*>(s_w1 + ((m * KB + kb) * 2) * 1024 + lane * 16);
                wl[m] = *reinterpret_cast<const half8_t*>(s_w1 + ((m * KB + kb) * 2 + 1) * 1024 + lane * 16);
            };
            half8_t bh, bl;
            auto mkb = [&](int s, int kb) {
                const float4 qa4 = *reinterpret_cast<const float4*>(qp + kb * 16);
                const float4 qb4 = *reinterpret_cast<const float4*>(qp + kb * 16 + 4);
                const float pr[8] = {hr[s][0].x * qa4.x, hr[s][0].y * qa4.y, hr[s][0].z * qa4.z, hr[s][0].w * qa4.w,
                                     hr[s][1].x * qb4.x, hr[s][1].y * qb4.y, hr[s][1].z * qb4.z, hr[s][1].w * qb4.w};
#pragma unroll
                for (int e = 0; e < 8; e += 2) {
                    half2_t h2, l2;
                    split_h16_pair(pr[e], pr[e + 1], h2, l2);
                    bh[e] = h2[0]; bh[e + 1] = h2[1];
                    bl[e] = l2[0]; bl[e + 1] = l2[1];
                }
            };
            // accumulators start as AK_t + qa: register r of tile m = hidden unit m*32 + crow(r, half)
            f32x16 acc[2];
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const float4 ak = *reinterpret_cast<const float4*>(akp + m * 32 + 8 * r4 + 4 * half);
                    acc[m][r4 * 4 + 0] = ak.x; acc[m][r4 * 4 + 1] = ak.y; acc[m][r4 * 4 + 2] = ak.z; acc[m][r4 * 4 + 3] = ak.w;
                }
#pragma unroll
            for (int kb = 0; kb < RL4RS_DINX_RING; ++kb) ldh(kb, kb);
            __builtin_amdgcn_sched_barrier(0);
#if !RL4RS_DINX_QSELF       // (QSELF: staged in front of the tile loop)
            if (n == 0) {
                s_q[lane] = q_lo;
                s_q[lane + 64] = q_hi;
                s_qa[lane] = qa_v;
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            }
#endif
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const float4 qv = *reinterpret_cast<const float4*>(s_qa + m * 32 + 8 * r4 + 4 * half);
                    acc[m][r4 * 4 + 0] += qv.x; acc[m][r4 * 4 + 1] += qv.y; acc[m][r4 * 4 + 2] += qv.z; acc[m][r4 * 4 + 3] += qv.w;
                }
            __builtin_amdgcn_sched_barrier(0);
            // per k-block: weight fragments (LDS) requested first, the split operand built behind them, then the six MFMAs; the
            // cache rows of k-block kb + RING are requested as soon as kb's have been consumed.  A wave alternates a VALU and an
            // MFMA stretch; the four waves of a SIMD fill each other's gaps (registers kept under 128 for that).
            DINX_TR((j / NW) * 2 + n, 1);
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                ldw(0, kb);
                ldw(1, kb);
                mkb(kb % RL4RS_DINX_RING, kb);
                __builtin_amdgcn_sched_barrier(0);
                if (kb == 0) DINX_TR((j / NW) * 2 + n, 2);
                if (kb == 4) DINX_TR((j / NW) * 2 + n, 3);
                if (kb + RL4RS_DINX_RING < KB) ldh(kb % RL4RS_DINX_RING, kb + RL4RS_DINX_RING);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[0], bh, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[1], bh, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[0], bh, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[1], bh, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[0], bl, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[1], bl, acc[1], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            DINX_TR((j / NW) * 2 + n, 4);
            // epilogue: hid1 = sigmoid(acc); layer 2 on the matrix pipe in the same split form; layer 3 in registers
            f32x16 acc2;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc2[r] = 0.f;
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int kb2 = 0; kb2 < 2; ++kb2) {
                    half8_t bh2, bl2;
#pragma unroll
                    for (int e = 0; e < 8; e += 2) {
                        half2_t h2, l2;
#if RL4RS_DINX_AB & 2       // timing ablation (results WRONG): no layer-1 sigmoids
                        split_h16_pair(acc[m][kb2 * 8 + e], acc[m][kb2 * 8 + e + 1], h2, l2);
#else
                        split_h16_pair(gate_sigmoid(acc[m][kb2 * 8 + e]), gate_sigmoid(acc[m][kb2 * 8 + e + 1]), h2, l2);
#endif
                        bh2[e] = h2[0]; bh2[e + 1] = h2[1];
                        bl2[e] = l2[0]; bl2[e + 1] = l2[1];
                    }
                    const half8_t ah2 = *reinterpret_cast<const half8_t*>(s_w2b + ((m * 2 + kb2) * 2) * 1024 + lane * 16);
                    const half8_t al2 = *reinterpret_cast<const half8_t*>(s_w2b + ((m * 2 + kb2) * 2 + 1) * 1024 + lane * 16);
                    acc2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah2, bh2, acc2, 0, 0, 0);
                    acc2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al2, bh2, acc2, 0, 0, 0);
                    acc2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah2, bl2, acc2, 0, 0, 0);
                }
            // acc2 register r < 8 of this lane = hid2 pre-activation of output unit crow(r, half) at this lane's step
            float sc = 0.f;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int o = crow(r, half);
                const float h2 = gate_sigmoid(acc2[r] + s_misc[o]);
                sc = fmaf(h2, s_misc[16 + o], sc);
            }
            sc += __shfl_xor(sc, 32);
            sc += s_misc[32];
            if (half == 0 && t < L) a.scores[(size_t)sq * a.scores_stride + (size_t)row * L + t] = sc;
            for (int d = __builtin_amdgcn_readfirstlane(dup0), d1 = __builtin_amdgcn_readfirstlane(dup1); d < d1; ++d) {
                const int drow = a.dup_list[d] * grp + (idx - g * grp);
                if (half == 0 && t < L) a.scores[(size_t)sq * a.scores_stride + (size_t)drow * L + t] = sc;
            }
            DINX_TR((j / NW) * 2 + n, 5);
        }
    }
    DINX_TR(4, 2);
