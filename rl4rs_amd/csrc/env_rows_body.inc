// The body of k_env_rows<MODE, USE_LDS> (env.hip), as text: k_env_rows_refine compiles the same lines with two hooks filled in
// (ENV_ROWS_BEGIN at the top of env b's iteration, ENV_ROWS_ACTED behind its act, ENV_ROWS_BUILT behind its row, ENV_ROWS_DONE
// behind the row loop; all empty in k_env_rows itself).
// In scope: EnvDev e, actions, cur, n_complete, j_base, ActTail tail; MODE and USE_LDS as compile-time constants.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* s_item_lds = reinterpret_cast<float*>(smem);
    const size_t item_bytes = USE_LDS ? (((size_t)e.A * e.D * 4 + 15) & ~size_t(15)) : 0;
    int32_t* s_prev_all = reinterpret_cast<int32_t*>(smem + item_bytes);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    int32_t* s_prev = s_prev_all + wave * e.T;
    if (USE_LDS && MODE != 0) {
        stage_items(e, s_item_lds);
        __syncthreads();
    }
    const float* s_item = USE_LDS ? s_item_lds : e.item_vec;
    const int R = (MODE == 2) ? e.B * n_complete : e.B;
    const int total_waves = gridDim.x * nw;
    if (MODE == 2 && RL4RS_ROWS_PER_ENV) {
        // complete rows: one wave writes ALL n_complete rows of its env - prev_actions and the user columns are fetched once,
        // then the wave only issues stores (a row per wave paid one dependent global round trip per 1.8 KB row)
        for (int b = blockIdx.x * nw + wave; b < e.B; b += total_waves) {
            for (int j = lane; j < e.T; j += 64) s_prev[j] = e.prev[(size_t)b * e.T + j];
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            for (int jj = 0; jj < n_complete; ++jj) {
                const int j = j_base + jj;
                const size_t r = (size_t)b * n_complete + jj;
                int page_init = 0, npage = e.T, seq_id = 1;
                if (e.is_seq) {
                    page_init = j / e.P * e.P;
                    npage = min(e.P, e.T - page_init);
                    seq_id = j / e.P + 1;
                }
                build_row(e, s_item, s_prev, b, page_init, npage, seq_id, s_prev[j], e.c_dense + r * e.Dn, e.c_cat + r * e.Cn, lane);
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // s_prev is rewritten for the next env
        }
        return;
    }
    for (int r = blockIdx.x * nw + wave; r < R; r += total_waves) {
        const int b = (MODE == 2) ? r / n_complete : r;
        int a = 0;
        ENV_ROWS_BEGIN(b);
        for (int j = lane; j < e.T; j += 64) s_prev[j] = e.prev[(size_t)b * e.T + j];
        if (MODE == 1) {
            a = actions[b];
            if (a < 0 || a >= e.A) {      // numpy would raise IndexError (slate.py:199)
                if (lane == 0) atomicExch(e.err, 1);
                a = 0;
            }
            s_prev[cur] = a;   // every lane writes the same value
            ENV_ROWS_ACTED(b, a, lane);
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (MODE == 0) {
            // RecState.__init__: dense = user_dense, category = user_cat, both padded (base.py:30-31)
            build_row(e, s_item, s_prev, b, 0, -1, 0, 0, e.dense + (size_t)b * e.Dn, e.cat + (size_t)b * e.Cn, lane);
            for (int l = lane; l < e.L; l += 64) e.seq1[(size_t)b * e.L + l] = 0;
        } else if (MODE == 1) {
            // ---- act (slate.py:198-202 / seqslate.py:98-102)
            if (lane == 0) {
                e.prev[(size_t)b * e.T + cur] = a;
                e.amask[(size_t)b * e.W + (a >> 5)] &= ~(1u << (a & 31));
                // the transition's constant outputs and the next step's logged action (ActTail): this wave owns env b
                if (tail.done) tail.done[b] = tail.done_v;
                if (tail.zero_reward) tail.zero_reward[b] = 0.0;
                if (tail.next_action) tail.next_action[b] = offline_action_id(e, b, tail.next_cur);
            }
            bool hit = false;
            for (int j = lane; j < e.T; j += 64) hit |= (e.is_special[s_prev[j]] != 0);
            const bool any_hit = __any(hit);
            const bool page_end = e.is_seq && ((cur + 1) % e.P == 0);
            for (int w = lane; w < e.W; w += 64) {
                if (page_end) {          // seqslate.py:124-126
                    uint32_t f = full_word(e.A, w);
                    e.amask[(size_t)b * e.W + w] = f;
                    e.smask[(size_t)b * e.W + w] = f;
                } else if (any_hit) {
                    e.smask[(size_t)b * e.W + w] &= ~e.special_bits[w];
                }
            }
            // ---- rebuild the state row (slate.py:203-213 / seqslate.py:103-122)
            int page_init = 0, npage = e.T, seq_id = 1;
            if (e.is_seq) {
                page_init = cur / e.P * e.P;
                npage = min(e.P, e.T - page_init);
                seq_id = cur / e.P + 1;
                // second sequence = items of the previous pages, pre-padded (seqslate.py:107-108)
                for (int l = lane; l < e.L; l += 64) {
                    int v = 0;
                    if (page_init > 0) {
                        int idx = page_init - e.L + l;
                        if (idx >= 0) v = s_prev[idx];
                    }
                    e.seq1[(size_t)b * e.L + l] = v;
                }
            }
            build_row(e, s_item, s_prev, b, page_init, npage, seq_id, a, e.dense + (size_t)b * e.Dn,
                      e.cat + (size_t)b * e.Cn, lane);
            ENV_ROWS_BUILT(b, a, lane);
        } else {
            // ---- complete-state row j of env b (slate.py:117-131 / seqslate.py:27-50)
            const int j = j_base + (r - b * n_complete);
            int page_init = 0, npage = e.T, seq_id = 1;
            if (e.is_seq) {
                page_init = j / e.P * e.P;
                npage = min(e.P, e.T - page_init);
                seq_id = j / e.P + 1;
            }
            a = s_prev[j];
            build_row(e, s_item, s_prev, b, page_init, npage, seq_id, a, e.c_dense + (size_t)r * e.Dn,
                      e.c_cat + (size_t)r * e.Cn, lane);
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // s_prev is rewritten by the next row
    }
    ENV_ROWS_DONE(smem);
