// The text of k_augru_x (augru_x.hpp), included into k_augru_x and - beside its shadow plane - into k_augru_xs (augru_xs.hpp) so that
// both compile from the same lines.  Expects in scope: MT, NRES, RING, PAD, GRP (compile-time constants) and RecurArgs a.
    using namespace xk;
    constexpr int NH = 256, KB = 16, PLANE = 32 * NH * 2;          // bytes per plane (16 KB)
#if defined(RL4RS_X_RESMASK) && defined(RL4RS_X_WINDOW)
    constexpr int NS = NI - NRES, LA = RING - 1, WINDOW = (MT == 1) ? RL4RS_X_WINDOW : 40 - NRES;
#else
    constexpr int NS = NI - NRES, LA = RING - 1, WINDOW = 40 - NRES;     // WINDOW: the item the projection requests are issued in front of
#endif
    constexpr Sched SC = make_sched<NRES>();
    constexpr bool PEEL = MT == 1 ? RL4RS_X_PEEL != 0 : RL4RS_X_PEEL_MT2 != 0;
    constexpr bool USPLIT = RL4RS_X_USPLIT == 2 || (RL4RS_X_USPLIT == 1 && MT == 2);      // role-specialised step (role_item, augru_x.hpp)
    constexpr Sched SE = make_sched<NRES>(true);                   // the early role's streamed sequence under USPLIT
    static_assert(!USPLIT || (PEEL && !RL4RS_X_SPREAD && !is_res<NRES>(40) && !is_res<NRES>(23) && RING <= 8 && RL4RS_X_XU_AT == 8),
                  "the split schedule: rotated loop, resident items in front of item 40, look-ahead inside a stretch of 8");
    static_assert(GRP == 8 || (GRP == 9 && MT == 2 && !PAD), "rows per cache slot of the 64-row form");
    constexpr int ROWS = GRP == 9 ? 63 : 32 * MT;                  // positions a workgroup stores
    static_assert(NS > 0 && NS % RING == 0 && RING >= 2 && NRES >= 1 && NRES <= 14 && (!RL4RS_X_SPREAD || NI % NRES == 0), "weight ring / resident items");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // planes in slab order [kb 16][k-half 2][row 32][8 halfs]; tile m's four planes (h hi/lo, r*h hi/lo) at m * 4 * PLANE
    char* hp_hi = smem;
    char* hp_lo = smem + PLANE;
    char* rp_hi = smem + 2 * PLANE;
    char* rp_lo = smem + 3 * PLANE;
    constexpr int TILE = 4 * PLANE, STG = MT == 1 ? 3 * 4096 : 3 * 1024;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, li = lane & 31;
    const int row0 = blockIdx.x * ROWS;
    const int sq = blockIdx.y;
    // row dedup (row_dedup.hpp): the launch works on the first n_active entries of a.order only - the grid is sized for a.n_rows
    // on the host, a workgroup behind the bound leaves here
    // (read again in the epilogue rather than kept across the recurrence: the 64-row form has no register to spare)
    int n_rows = a.n_active ? min(a.n_rows, a.n_active[0] * a.group) : a.n_rows;
    if (row0 >= n_rows) return;
    const int L = a.L;
    const int xld4 = (int)a.xld * 4;
    char* stage = smem + MT * TILE + wave * STG;                   // this wave's projection staging: gate g at + g * STG / 3
    // packed fp16 planes: [ntile][KB][plane hi/lo][64 lanes][8 halfs] -> 1 KB per (ntile, kb, plane) (pack_frag_h16)
    const __amdgpu_buffer_rsrc_t rs_wg = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wg[sq]), 0, 2 * NH * NH * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_wc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wc[sq]), 0, NH * NH * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.xbase[sq]), 0, (int)a.xbytes, 0x00020000);
    const int vl16 = lane * 16;

#pragma unroll
    for (int m = 0; m < MT; ++m)
        for (int i = tid; i < 2 * PLANE / 16; i += 512) reinterpret_cast<uint4*>(hp_hi + m * TILE)[i] = make_uint4(0u, 0u, 0u, 0u);     // h = 0
    // ---- projection staging geometry.  DMA instruction j (0..3) of a gate covers rows 8j .. 8j+7: lane l fetches, for row
    // r = 8j + l/8, the 16-byte chunk c = (l%8 - r/2) mod 8 of the wave's 128 bytes of that row; it lands at slot + r*128 +
    // (l%8)*16.  The reader (row li, column run q of half `half`: chunk 2q + half) finds it at position (2q + half + li/2) mod 8.
    // processing order: tile position p works on batch row phys(p) - with a row order (rl4rs_dien_set_row_order: env groups sorted
    // by their history's cache slot) the rows of a tile, and of tiles that run at the same time, share projection rows in L2
    auto phys = [&](int p) {
        p = min(p, n_rows - 1);
        return a.order ? a.order[p / a.group] * a.group + p % a.group : p;
    };
    int dma_off[4];
    int pad_delta[4] = {0, 0, 0, 0}, lead_j[4] = {0, 0, 0, 0};     // PAD: (pad slot - own slot) in bytes, leading zero ids of the lane's row
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // MT = 1: row r = 8j + l/8, rotated chunk.  MT = 2 (only j = 0 is used): lane l fetches chunk l%8 of distinct row d = l/8,
        // i.e. of batch row row0 + GRP d (rows GRP d .. GRP d + GRP - 1 share its cache slot)
        const int r = MT == 1 ? 8 * j + (lane >> 3) : GRP * (lane >> 3);
        const int gr = phys(row0 + r);
        const int c = MT == 1 ? (((lane & 7) - (r >> 1)) & 7) : (lane & 7);
        const uint32_t slot = (uint32_t)a.slots[(size_t)sq * a.slots_stride + gr / a.group];
        dma_off[j] = (int)(slot * (uint32_t)L * (uint32_t)xld4) + c * 16;
        if constexpr (PAD) {
            lead_j[j] = a.lead[sq][slot];
            pad_delta[j] = (int)(((uint32_t)a.pad_slot - slot) * (uint32_t)L * (uint32_t)xld4);
        }
    }
    const float* att_row[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
        att_row[m] = a.att + (size_t)sq * a.att_stride + (size_t)phys(row0 + m * 32 + li) * L;
    const int xs_base = wave * 128 + a.xoff * 4;                  // byte offset of the wave's 32 columns inside a gate block
    auto x_dma = [&](int t) {                                      // the three gates' rows of step t -> staging
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int j = 0; j < (MT == 1 ? 4 : 1); ++j) {
                int voff = dma_off[j];
                if constexpr (PAD) voff += t < lead_j[j] ? pad_delta[j] : 0;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x, (lds_ptr_t)(stage + g * (STG / 3) + j * 1024), 16, voff,
                                                         t * xld4 + xs_base + g * NH * 4, 0, RL4RS_X_DMA_AUX);
            }
    };
    auto x_read = [&](f32x16& dst, int g, int m) {                 // staged projection rows -> accumulator (MFMA C-in)
        const int rot = half + (li >> 1);
        int srow = 4 * m + (li >> 3);                              // staged row of tile row 32 m + li
        if constexpr (GRP == 9) {
            int tr = 32 * m + li;
            asm volatile("" : "+v"(tr));                           // recomputed at every read: held across the step it costs a register the form does not have
            srow = (tr * 57) >> 9;                                 // tr / 9 for tr < 64
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const char* src = MT == 1 ? stage + g * 4096 + li * 128 + (((2 * q + rot) & 7) << 4)
                                      : stage + g * 1024 + srow * 128 + ((2 * q + half) << 4);
            const float4 v = *reinterpret_cast<const float4*>(src);
            dst[4 * q + 0] = v.x; dst[4 * q + 1] = v.y; dst[4 * q + 2] = v.z; dst[4 * q + 3] = v.w;
        }
    };
    // weight item i of a step -> buffer + scalar byte offset (the lo plane sits 1 KB behind the hi plane: immediate offset)
    int sb_r = wave * KB * 2048, sb_u = (8 + wave) * KB * 2048, sb_c = wave * KB * 2048;
    auto wload = [&](int i, half8_t& hi, half8_t& lo) {
        const int g = gate(i), off = (RL4RS_X_AB & 32) ? 0 : kb(i) * 2048;       // 32: every streamed load hits the same (L1-resident) fragment
        if (g == 0) { hi = buf_load_h8(rs_wg, vl16, sb_r + off); lo = buf_load_h8(rs_wg, vl16 + 1024, sb_r + off); }
        else if (g == 1) { hi = buf_load_h8(rs_wg, vl16, sb_u + off); lo = buf_load_h8(rs_wg, vl16 + 1024, sb_u + off); }
        else { hi = buf_load_h8(rs_wc, vl16, sb_c + off); lo = buf_load_h8(rs_wc, vl16 + 1024, sb_c + off); }
    };
    const int foff = half * 512 + li * 16;                         // this lane's fragment inside a (plane, k-block) slab

    f32x16 acc_r[MT], acc_u[MT], acc_c[MT], h_own[MT];
    half8_t res_h[NRES], res_l[NRES], ring_h[RING], ring_l[RING];
    half8_t bh[2][MT], bl[2][MT];
    float amax[MT], att_cur[MT], att_next[MT], oma[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        amax[m] = 0.f;
        att_next[m] = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) h_own[m][r] = 0.f;
    }
    x_dma(0);
#pragma unroll
    for (int i = 0; i < NI; ++i)
        if (is_res<NRES>(i)) wload(i, res_h[SC.res_idx[i]], res_l[SC.res_idx[i]]);
    if constexpr (!PEEL) {
#pragma unroll
        for (int k = 0; k < LA; ++k) {
            const int js = (SC.js_first + k) % NS;
            wload(SC.item_of[js], ring_h[js % RING], ring_l[js % RING]);
        }
    }                                                              // (PEEL: step 0's first streamed item is 40; its look-ahead requests ride in step 0's own slots)
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        att_cur[m] = att_row[m][0];
        if constexpr (!USPLIT) x_read(acc_r[m], 0, m);             // h = 0: the R products of step 0 vanish, acc_r = x_r(0)
    }                                                              // (USPLIT: read per role, see `recur`)
    __syncthreads();

    auto hfrag = [&](int buf, int i) {                             // state fragments (B operand) of item i's k-block
        const char* ph = from_rh(i) ? rp_hi : hp_hi;
        const char* pl = from_rh(i) ? rp_lo : hp_lo;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            bh[buf][m] = *reinterpret_cast<const half8_t*>(ph + m * TILE + kb(i) * 1024 + foff);
            bl[buf][m] = *reinterpret_cast<const half8_t*>(pl + m * TILE + kb(i) * 1024 + foff);
        }
    };
    // four consecutive hidden columns (run q) of this lane's row -> the fp16 hi / lo planes (8-byte LDS writes)
    auto plane_store = [&](char* p_hi, char* p_lo, int m, int q, const float* v) {
        half4_t vh, vl;
#if RL4RS_X_SPLITPAIR
#pragma unroll
        for (int j = 0; j < 4; j += 2) {
            half2_t h2, l2;
            split_h16_pair(v[j], v[j + 1], h2, l2);        // same roundings: hi = RNE(x), lo = RNE(x - hi) from ONE fp32 value each
            vh[j] = h2[0]; vh[j + 1] = h2[1];
            vl[j] = l2[0]; vl[j + 1] = l2[1];
        }
#else
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // the value must be ONE rounded fp32 number for both uses below: left transparent, the compiler contracts the
            // producing multiply into the fp16 conversion for one of them (v_fma_mixlo_f16: single rounding from the exact
            // product) but not for the other, and hi + lo then misses v by an fp16 ulp in the double-rounding cases
            float x = v[j];
            asm volatile("" : "+v"(x));
            const _Float16 h = (_Float16)x;
            vh[j] = h;
            vl[j] = (_Float16)(x - (float)h);
        }
#endif
        // column 32w + 8q + 4half + j -> k-block 2w + q/2, k-half q%2, element 4half + j
        const int o = m * TILE + (2 * wave + (q >> 1)) * 1024 + (q & 1) * 512 + li * 16 + half * 8;
        *reinterpret_cast<half4_t*>(p_hi + o) = vh;
        *reinterpret_cast<half4_t*>(p_lo + o) = vl;
    };
    const float k_r = a.k_r[sq][wave], k_u = a.k_u[sq][wave], k_c = a.k_c[sq][wave];   // activations of prescaled pre-activations (RecurArgs)
    float quad[MT][4];
    auto reset_gate = [&](int r) {                                 // element r of the reset gate: r*h -> planes
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            quad[m][r & 3] = ((RL4RS_X_AB & 1) ? acc_r[m][r] : gate_sigmoid_k(acc_r[m][r], k_r)) * h_own[m][r];
            if ((r & 3) == 3) plane_store(rp_hi, rp_lo, m, r >> 2, quad[m]);
        }
    };
    auto update_gate = [&](int r) {
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            float pre = acc_u[m][r];
            asm volatile("" : "+v"(pre));                          // keeps this element's chain where it is written
            acc_u[m][r] = oma[m] * ((RL4RS_X_AB & 1) ? pre : gate_sigmoid_k(pre, k_u));
        }
    };
    auto blend = [&](int r) {                                      // candidate + state update of element r -> h planes
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const float cnd = (RL4RS_X_AB & 1) ? acc_c[m][r] : gate_tanh_k(acc_c[m][r], k_c);
            const float hn = __builtin_fmaf(acc_u[m][r], h_own[m][r] - cnd, cnd);       // u h + (1-u) c
#if RL4RS_X_AMAX
            amax[m] = fmaxf(amax[m], fabsf(hn));
#endif
            h_own[m][r] = hn;
            quad[m][r & 3] = hn;
            if ((r & 3) == 3) plane_store(hp_hi, hp_lo, m, r >> 2, quad[m]);
        }
    };

    const bool early = wave < 4;
#if RL4RS_X_PRIO == 1 || RL4RS_X_PRIO == 2
    // the late waves carry their candidate epilogue next to their own MFMAs (R-early phase) and are the younger half of the
    // workgroup (the arbitration losers): one static priority raise, no per-phase flips (MI355X_MICROARCH.md, two waves per SIMD #4)
    if (!early) __builtin_amdgcn_s_setprio(RL4RS_X_PRIO);
#endif
    const int TL = a.steps > 0 ? a.steps : L;
    // items [lo, hi) of step t.  light: the items' matrix products are known to vanish or to be dead (BOUNDARY STEPS below) - no
    // MFMAs, no state-fragment reads and no weight requests for them; projections, epilogues, plane stores, barriers and the
    // projection issue window stay in their slots
    // role: 0 = one schedule, the role is the run-time value `early`; 1 / 2 = the early / late role of the split schedule (USPLIT), known
    // at compile time: [lo, hi) are sequence positions of role_item (for roles 0 and 2 position = item)
    auto items = [&](const int t, const int lo, const int hi, const bool light, const int role) __attribute__((always_inline)) {
        const bool ea = role == 0 ? early : role == 1;
        const bool se = role == 1;
#pragma unroll
        for (int s = lo; s < hi; ++s) {
            const int i = role_item(se, s), nxt = s + 1 < NI ? role_item(se, s + 1) : NI;
            const int g = gate(i), cur = i & 1;
            if (i == (se ? 16 : 8)) RL4RS_XT(1);
            // (split early role: x_u(t) was read behind barrier a of the step before - except in step 0, which has no such window)
            if (se ? i == 16 && light : i == RL4RS_X_XU_AT) {
                if (!(RL4RS_X_AB & (4 | 128))) {                  // x_u(t)   (128: no staging reads, DMA keeps going): staged one step ago
#pragma unroll
                    for (int m = 0; m < MT; ++m) x_read(acc_u[m], 1, m);
                }
            }
            if (i == RL4RS_X_XC_AT && RL4RS_X_XC_AT != 24) {
                if (!(RL4RS_X_AB & (4 | 128))) {                  // x_c(t), ahead of the barrier
#pragma unroll
                    for (int m = 0; m < MT; ++m) x_read(acc_c[m], 2, m);
                }
            }
            if (i == 24) {
                RL4RS_XT(2);
                if (!(RL4RS_X_AB & 16)) __syncthreads();           // r*h planes complete
                RL4RS_XT(3);
                if (RL4RS_X_XC_AT == 24 && !(RL4RS_X_AB & (4 | 128))) {                  // x_c(t)
#pragma unroll
                    for (int m = 0; m < MT; ++m) x_read(acc_c[m], 2, m);
                }
                if (!ea && !RL4RS_X_LATE_UPD_SHADOW) {
                    // late role: the whole update gate first (VALU only) - its partner on the SIMD is already in its C items
#pragma unroll
                    for (int r = 0; r < 16; ++r) update_gate(r);
#if RL4RS_X_PRIO == 3
                    __builtin_amdgcn_s_setprio(1);        // ... and then must not lose every MFMA arbitration to the (older) early wave
#endif
                }
                if (!light) hfrag(cur, i);
            }
            if (i == 40) {
                if (ea) {
                    // early role: candidate + blend after its C items, while its partner runs C on the matrix pipe
#pragma unroll
                    for (int r = 0; r < 16; ++r) blend(r);
                }
                RL4RS_XT(4);
#if RL4RS_X_PRIO == 3
                if (!ea) __builtin_amdgcn_s_setprio(0);
#endif
                if (!(RL4RS_X_AB & 16)) __syncthreads();           // early half of the new state complete
                RL4RS_XT(5);
                if (!(RL4RS_X_AB & (4 | 128)) && !light) {        // x_r(t+1) (requested 12+ items ago)
#pragma unroll
                    for (int m = 0; m < MT; ++m) x_read(acc_r[m], 0, m);
                }
                if (se && !light && !(RL4RS_X_AB & (4 | 128))) {  // x_u(t+1) behind the same wait: acc_u is dead since the blend above
#pragma unroll
                    for (int m = 0; m < MT; ++m) x_read(acc_u[m], 1, m);
                }
                if (!light) hfrag(cur, i);
            }
            if (i == WINDOW && t + 1 < L && !(RL4RS_X_AB & (4 | 64))) {       // 64: no projection DMA (reads keep going)
                // ---- the ONE projection issue window of the step: the register-resident items follow (no vector-memory wait)
                // (light: no MFMA has waited for the x_u / x_c reads above yet - they must have left the staging before it is rewritten)
                if (light) __builtin_amdgcn_s_waitcnt(0xc07f);            // lgkmcnt(0)
                x_dma(t + 1);
#pragma unroll
                for (int m = 0; m < MT; ++m) att_next[m] = att_row[m][t + 1];
            }
            // ---- fetch ahead: state fragments of the next item, streamed weights LA items ahead
            if (nxt < NI && !after_barrier(nxt) && !(RL4RS_X_AB & 8) && !light) hfrag(cur ^ 1, nxt);
            const bool resident = is_res<NRES>(i);
            const int js = resident ? 0 : (se ? SE.js_of[i] : SC.js_of[i]);      // position in the streamed sequence (if streamed)
            const int ridx = resident ? SC.res_idx[i] : 0;
            const int ahead = resident ? 0 : (se ? SE.item_of[(js + LA) % NS] : SC.item_of[(js + LA) % NS]);
            // light: nothing for an item that is skipped itself (below 40 in the first step; the last step's tail requests nothing at all)
            // (split early role: step 0's stretch ends in front of item 40 as well and its look-ahead stays inside it or reaches 40 ..)
            const bool fetch = !resident && !(RL4RS_X_AB & 2) && !(light && (i >= 40 || (se ? ahead < 40 : ahead > i && ahead < 40)));
            if (fetch) wload(ahead, ring_h[(js + LA) % RING], ring_l[(js + LA) % RING]);
            __builtin_amdgcn_sched_barrier(0);
            const half8_t wh = resident ? res_h[ridx] : ring_h[js % RING];
            const half8_t wl = resident ? res_l[ridx] : ring_l[js % RING];
            // product terms outermost: with two row tiles the dependent MFMAs of one accumulator are a tile apart
#pragma unroll
            for (int term = 0; term < (light ? 0 : 3); ++term)
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    f32x16& acc = g == 0 ? acc_r[m] : (g == 1 ? acc_u[m] : acc_c[m]);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(term == 1 ? wl : wh, term == 2 ? bl[cur][m] : bh[cur][m], acc, 0, 0, 0);
                }
            // ---- epilogue work in this item's MFMA shadow
            if (se && i >= 16 && i < 24) {                         // the eight U items the stretch keeps carry the reset gate, two elements each
                reset_gate(2 * (i - 16));
                reset_gate(2 * (i - 16) + 1);
            } else if (!se && i >= 8 && i < 24) {
                reset_gate(i - 8);
            } else if ((ea || RL4RS_X_LATE_UPD_SHADOW) && i >= 24 && i < 32) {
                update_gate(2 * (i - 24));
                update_gate(2 * (i - 24) + 1);
            } else if (!ea && i >= 40) {
                blend(2 * (i - 40));
                blend(2 * (i - 40) + 1);
            }
#if RL4RS_X_SGB
            if ((i >= (se ? 16 : 8) && i < 24) || (ea && i >= 24 && i < 32) || (!ea && i >= 40)) {
                // a wave issues in order: spread the VALU chunk over the item's three MFMAs instead of behind the last one
#pragma unroll
                for (int q = 0; q < 3 * MT; ++q) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);         // one MFMA
                    __builtin_amdgcn_sched_group_barrier(0x002, RL4RS_X_SGB, 0);     // VALU in its shadow
                }
            }
#endif
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto step_begin = [&](const int t, const bool light) __attribute__((always_inline)) {
        RL4RS_XT(0);
#pragma unroll
        for (int m = 0; m < MT; ++m) oma[m] = 1.0f - att_cur[m];
        if (!light) hfrag(0, 0);
    };
    auto step_end = [&](const int t) __attribute__((always_inline)) {
#pragma unroll
        for (int m = 0; m < MT; ++m) att_cur[m] = att_next[m];
        RL4RS_XT(6);
        if (!(RL4RS_X_AB & 16)) __syncthreads();                   // late half of the new state complete
        RL4RS_XT(7);
    };
    if constexpr (PEEL) {
        // ---- BOUNDARY STEPS.  The recurrence starts from h = 0, so in step 0 the B operand of items 0-39 (h planes, r*h planes) is
        // all zeros: each of their MFMAs would add w * 0 to an accumulator element that already holds x_u(0) / x_c(0) / x_r(0).
        // Weights are finite (non-finite checkpoints never reach this mode), so every such sum of products is a zero and x + 0 = x
        // bit for bit for x != 0; where x is itself a zero only its sign can differ, and exp2(k * x) in both gate functions
        // (gate_sigmoid_k / gate_tanh_k) maps +0, -0 - and a subnormal x, should the matrix pipe flush one on its way through an
        // accumulator - to exactly 1.  Items 40-47 of the LAST step are the reset-gate product of a step that does not exist: they
        // only write acc_r, which nothing reads after the loop.  So the loop is rotated - its body is items 40-47 of step t followed
        // by items 0-39 of step t + 1, the same code in the same order as the plain loop - and the two boundary stretches run
        // `light`: 48 of the 64 x 48 items' MFMAs, weight fragments and state-fragment reads are not issued.  Step 0 enters the
        // streamed weight sequence at item 40 (position 0): the LA requests in front of it are the ones the slots below 40 issue
        // in every step, so the ring reaches the loop in its steady state and no slot index depends on the step.  One step
        // (maxlen 1, RecurArgs::steps = 1) is both stretches back to back.
        // USPLIT: the recurrence exists once per role behind ONE wave-uniform branch (with a branch per stretch the values that live
        // across the joins - accumulators, state, weight ring - must agree on their registers between the roles: 100 spilled
        // registers in the 64-row form, DESIGN 34).  Both roles count the same three barriers per step.  `sb`: the role's first
        // position behind barrier a (role_stretch).  The early role's first stretch has no U items on k-blocks 0..7 at all (they were
        // light in step 0 anyway) and reads x_u(0) in front of item 16; its tail (`tail`: end position) is items 40-47 alone - no U
        // items, and no weight requests, of a step that does not exist.
        auto recur = [&](const int role, const int sb, const int tail) __attribute__((always_inline)) {
            // x_r(0) behind the branch: read in front of it, the 16 MT registers that the other role's step 0 still reads stay
            // live through this role's whole loop (the two paths are laid out one behind the other) and are spilled around it
            // (the two markers differ, so that the reads - and the reset gate's prescale behind them - are not hoisted back as common code)
            if (role == 1) asm volatile("; early role"); else asm volatile("; late role");
#pragma unroll
            for (int m = 0; m < MT; ++m) x_read(acc_r[m], 0, m);
            int t = 0;
            step_begin(0, true);
            items(0, 0, sb, true, role);
#pragma unroll 1
            while (t + 1 < TL) {
                asm volatile("" : "+s"(sb_r), "+s"(sb_u), "+s"(sb_c));     // keep the per-item scalar offsets out of SGPR-hoisting
                items(t, sb, NI, false, role);
                step_end(t);
                ++t;
                step_begin(t, false);
                items(t, 0, sb, false, role);
            }
            items(t, sb, tail, true, role);
            step_end(t);
        };
        if constexpr (USPLIT) {
            if (early) recur(1, role_stretch(true), 40);
            else recur(2, 40, NI);
        } else {
            int t = 0;
            step_begin(0, true);
            items(0, 0, 40, true, 0);
#pragma unroll 1
            while (t + 1 < TL) {
                asm volatile("" : "+s"(sb_r), "+s"(sb_u), "+s"(sb_c));     // keep the per-item scalar offsets out of SGPR-hoisting
                items(t, 40, NI, false, 0);
                step_end(t);
                ++t;
                step_begin(t, false);
                items(t, 0, 40, false, 0);
            }
            items(t, 40, NI, true, 0);
            step_end(t);
        }
    } else {
#pragma unroll 1
        for (int t = 0; t < TL; ++t) {
            asm volatile("" : "+s"(sb_r), "+s"(sb_u), "+s"(sb_c));     // keep the per-item scalar offsets out of SGPR-hoisting
            step_begin(t, false);
            items(t, 0, NI, false, 0);
            step_end(t);
        }
    }
    // ---- poison rows that left the fp16 range (or went NaN) and write the final state (16-byte stores).  The final state alone
    // decides: a state element beyond the largest finite fp16 number becomes +-inf in the hi plane and -+inf in the lo plane at
    // the step it appears; from then on its row's accumulators hold inf - inf = NaN or a saturated gate times inf, i.e. the
    // state stays inf / NaN to the end (nothing maps them back to a finite number: sigmoid / tanh of +-inf give 0 / 1 / +-1 and
    // the blend multiplies the non-finite h by them or by 0), so |h_final| < 6e4 fails for exactly those rows - no per-step
    // running maximum needed (16 v_max3 per wave and step).  Rows that pass through [6e4, 65504] and come back were carried
    // exactly and are not errors.
    uint32_t* s_bad = reinterpret_cast<uint32_t*>(rp_hi);          // the planes are dead now
    if (tid < 32 * MT) s_bad[tid] = 0u;
    __syncthreads();
    bool any_bad = false;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        bool bad = !(amax[m] < 6.0e4f);
#pragma unroll
        for (int r = 0; r < 16; ++r) bad |= !(fabsf(h_own[m][r]) < 6.0e4f);
        if (bad) atomicOr(&s_bad[m * 32 + li], 1u);
        any_bad |= bad;
    }
    __syncthreads();
    if (a.n_active) n_rows = min(a.n_rows, *const_cast<const volatile int32_t*>(a.n_active) * a.group);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int row = phys(row0 + m * 32 + li);
        const bool poison = s_bad[m * 32 + li] != 0u;
        if (row0 + m * 32 + li < n_rows && m * 32 + li < ROWS) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float4 v = make_float4(h_own[m][4 * q], h_own[m][4 * q + 1], h_own[m][4 * q + 2], h_own[m][4 * q + 3]);
                if (poison) v = make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));
                *reinterpret_cast<float4*>(a.out + (int64_t)row * a.out_ld + a.out_off + sq * a.out_seq_off + wave * 32 + 8 * q + 4 * half) = v;
            }
            if (a.dup_start) {      // row dedup: the same pieces to the same row of every duplicate of this row's group
                const int pos = row0 + m * 32 + li, gi = pos / a.group, sub = pos - gi * a.group;
                const int d1 = a.dup_start[gi + 1];
                for (int d = a.dup_start[gi]; d < d1; ++d) {
                    const int drow = a.dup_list[d] * a.group + sub;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        float4 v = make_float4(h_own[m][4 * q], h_own[m][4 * q + 1], h_own[m][4 * q + 2], h_own[m][4 * q + 3]);
                        if (poison) v = make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));
                        *reinterpret_cast<float4*>(a.out + (int64_t)drow * a.out_ld + a.out_off + sq * a.out_seq_off + wave * 32 + 8 * q + 4 * half) = v;
                    }
                }
            }
        }
    }
    if (any_bad && a.range_flag) atomicOr(a.range_flag, 1);
