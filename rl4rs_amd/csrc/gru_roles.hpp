// k_gru_h16r: the first-layer GRU of the fp16x2 scorer (k_gru_h16, dien.hip) with two wave roles per SIMD (included by dien.hip).
//
// Same arithmetic, same bits: NH = E = 128, 32 rows per workgroup, every accumulator element = its table projection as MFMA C-in,
// then k-blocks 0..7 ascending, per k-block (h_hi, W_hi), (h_hi, W_lo), (h_lo, W_hi); blend fma(u, h - c, c); the fp16 planes split
// from the ROUNDED fp32 state.  What changes is who does what.  8 waves: wave w < 4 ("rc") and wave w + 4 ("u") share a SIMD and
// the hidden columns [32w, 32w + 32).
//   rc, step t:  acc_r <- xr staging ; slot R (Wr in registers) ; reset gate, r*h -> r planes ; BARRIER 1 ;
//                acc_c <- xc staging ; slot C (Wc in registers) ; tanh ; u <- u plane ; blend ; h planes + fp32 state plane ; BARRIER 2
//   u,  step t:  slot U (Wu in registers, the accumulator holds its projection) ; sigmoid -> u plane ; state plane of step t - 1
//                -> h1 row and fragment-order copy (16-byte stores) ; BARRIER 1 ;
//                the gathered table rows of step t + 1 -> xr staging, xc staging ; gathers of step t + 2 requested ; BARRIER 2
// The r -> r*h -> candidate chain carries no gather, no global store and no update-gate work; the update gate, the 48 table
// gathers per lane (requested a whole step before they are consumed) and every store to memory run beside it.  The update gate
// and the projections cross LDS as fp32 in the lane's own accumulator order (16-byte accesses, exact), so both roles index them
// alike: plane[w][r / 4][lane][r % 4].
//
// LDS hand-offs (B1(t), B2(t) = the two barriers of step t; B2(t0 - 1) = the barrier in front of the loop):
//   plane            written by                     read by
//   h hi/lo (fp16)   rc   B1(t)   .. B2(t)          rc, u  B2(t)   .. B1(t+1)      (slots R and U of step t + 1)
//   r*h hi/lo        rc   B2(t-1) .. B1(t)          rc     B1(t)   .. B2(t)        (slot C)
//   u (fp32)         u    B2(t-1) .. B1(t)          rc     B1(t)   .. B2(t)        (blend)
//   state (fp32)     rc   B1(t)   .. B2(t)          u      B2(t)   .. B1(t+1)      (stores; the reads are complete at B1: the
//                                                                                   barrier's release fence waits for LDS)
//   xr staging       u    B1(t)   .. B2(t)  (t+1)   rc     B2(t)   .. B1(t+1)      (C-in of slot R of step t + 1)
//   xc staging[p]    u    B1(t)   .. B2(t)  (t+1)   rc     B1(t+1) .. B2(t+1)      (p = (t + 1) & 1: the rc waves read buffer t & 1
//                                                                                   in the window in which buffer (t + 1) & 1 is written)
// Front padding (RecurArgs::pad) as in k_gru_h16: the tile's shortest zero prefix t0 comes from the handle's table, rows 0 .. t0 - 1
// of it are copied to h1 AND to the fragment copy, the recurrence starts from row t0 - 1, lead_out[slot] is written.
// Fragment copy (a.h1f != NULL): written here, k_h1_frag is not launched.  The steps L .. 32 NT - 1 of the last step tile are
// WRITTEN as zeros by every launch (the allocation is not cleared and k_din_x multiplies those lanes).
#pragma once
#include "gru_frag_map.hpp"

namespace rl4rs {

// (RL4RS_TRG: the s_memtime marks of tools/h16_trace.py --gru, defined in front of k_gru_h16 in dien.hip.  rc role: 0 step start |
//  1 slot R done | 2 reset gate done | 3 behind barrier 1 | 4 slot C done | 5 blend done | 6 behind barrier 2.  u role: 0 step start |
//  1 slot U done | 2 update gate done | 3 stores issued | 4 behind barrier 1 | 5 stagings written, gathers requested | 6 behind barrier 2)

inline size_t gru_h16r_smem(int L) {
    return (((size_t)4 * 32 * (128 + 8) * 2 + (size_t)32 * (L + 1) * 4 + 15) & ~(size_t)15) + (size_t)4 * 16384 + (size_t)32 * gfm::LDH * 4;
}

__global__ __launch_bounds__(512) void k_gru_h16r(RecurArgs a) {
    constexpr int NH = 128, NW = 4, KB = NH / 16, LDP = NH + 8, LDH = gfm::LDH;
    typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) char smem[];
    _Float16* hp_hi = reinterpret_cast<_Float16*>(smem);     // [32][LDP] each
    _Float16* hp_lo = hp_hi + 32 * LDP;
    _Float16* rp_hi = hp_lo + 32 * LDP;
    _Float16* rp_lo = rp_hi + 32 * LDP;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool urole = wave >= 4;                             // waves w and w + 4 share a SIMD
    const int w = wave & 3;
    const int half = lane >> 5, li = lane & 31;
    const int row0 = blockIdx.x * 32;
    const int L = a.L, LDT = L + 1, NT = (L + 31) >> 5;
    const int col = w * 32 + li;
    const int xld4 = (int)a.xld * 4;
    int32_t* s_ids = reinterpret_cast<int32_t*>(rp_lo + 32 * LDP);                  // [32][LDT]
    float* s_u = reinterpret_cast<float*>(smem + ((4 * 32 * LDP * 2 + 32 * LDT * 4 + 15) & ~15));    // [4 waves][4][64 lanes][4]
    float* s_xr = s_u + 4096;
    float* s_xc = s_xr + 4096;                                // two buffers
    float* s_h = s_xc + 8192;                                 // [32][LDH]
    const int fo = w * 1024 + lane * 4;                       // this lane's elements 4q .. 4q + 3 of a plane: fo + 256 q
    const __amdgpu_buffer_rsrc_t rs_wg = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wg[0]), 0, 2 * NW * KB * 2048, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_wc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wc[0]), 0, NW * KB * 2048, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.xbase[0]), 0, (int)a.xbytes, 0x00020000);
    const int vl16 = lane * 16;

    for (int i = tid; i < 2 * 32 * LDP; i += 512) hp_hi[i] = (_Float16)0.f;          // hi and lo planes of h
    for (int i = tid; i < 32 * L; i += 512) {
        const int r = i / L, t = i - r * L;
        s_ids[r * LDT + t] = a.ids[(size_t)min(row0 + r, a.n_rows - 1) * L + t];
    }
    // outputs: descriptors over the valid rows [row0, row0 + rows_here) of h1 and of the fragment copy - a row past n_rows falls
    // outside and the hardware drops its stores; no fragment copy = an empty descriptor (every store dropped)
    const int rows_here = min(32, a.n_rows - row0);
    auto uniform_ptr = [](float* p) {         // (the 64-bit product runs on the vector ALU: without the readfirstlanes the descriptor
        const uint64_t b = reinterpret_cast<uint64_t>(p);                  // counts as divergent and every store becomes a waterfall loop)
        return reinterpret_cast<float*>(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(b >> 32)) << 32) |
                                        (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b));
    };
    const __amdgpu_buffer_rsrc_t rs_o = __builtin_amdgcn_make_buffer_rsrc(
        uniform_ptr(a.out + ((int64_t)a.slot_base + row0) * L * NH), 0, __builtin_amdgcn_readfirstlane(rows_here * L * NH * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_f = __builtin_amdgcn_make_buffer_rsrc(
        uniform_ptr(a.h1f ? a.h1f + ((int64_t)a.slot_base + row0) * NT * 4096 : nullptr), 0,
        __builtin_amdgcn_readfirstlane(a.h1f ? rows_here * NT * 16384 : 0), 0x00020000);
    auto store_piece = [&](const float4& v, int lane_h, int lane_f, int step_h, int step_f) {
        const u32x4_t pk = {__builtin_bit_cast(unsigned, v.x), __builtin_bit_cast(unsigned, v.y), __builtin_bit_cast(unsigned, v.z),
                            __builtin_bit_cast(unsigned, v.w)};
        __builtin_amdgcn_raw_buffer_store_b128(pk, rs_o, lane_h, step_h, 0);
        __builtin_amdgcn_raw_buffer_store_b128(pk, rs_f, lane_f, step_f, 0);
    };
    // zero tail of the fragment copy's last step tile
    for (int z = tid; z < (32 * NT - L) * 1024; z += 512) {
        const u32x4_t zero = {0u, 0u, 0u, 0u};
        __builtin_amdgcn_raw_buffer_store_b128(zero, rs_f, gfm::h1f_off(gfm::tail_row(z), gfm::tail_t(z, L), gfm::tail_c4(z), NT), 0, 0);
    }
    __syncthreads();

    const int xcol4 = (a.xoff + col) * 4;
    auto load_x = [&](f32x16& dst, int t, int block) {       // table row of each of the lane's 16 rows (u role: for its rc partner too)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            dst[r] = buf_load1(rs_x, s_ids[crow(r, half) * LDT + t] * xld4 + xcol4, block * NH * 4);
    };
    auto put_plane = [&](float* plane, const f32x16& v) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *reinterpret_cast<float4*>(plane + fo + 256 * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    };
    auto get_plane = [&](f32x16& v, const float* plane) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 x = *reinterpret_cast<const float4*>(plane + fo + 256 * q);
            v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
        }
    };

    int t0 = 0;
    float hv0 = 0.f;
    if (a.pad) {                                                          // (uniform)
        __shared__ int s_lead[32];
        __shared__ int s_t0;
        if (tid < 32) s_lead[tid] = L;
        if (tid == 0) s_t0 = L;
        __syncthreads();
        if (tid < 256) {
            const int r = tid >> 3, c = tid & 7, cl = (L + 7) >> 3;       // 8 threads per row, a chunk of the row's ids each
            int first = L;
            for (int t = min(L, (c + 1) * cl) - 1; t >= c * cl; --t)
                if (s_ids[r * LDT + t] != 0) first = t;
            if (first < L) atomicMin(&s_lead[r], first);
        }
        __syncthreads();
        if (tid < 32) {
            atomicMin(&s_t0, s_lead[tid]);                                // (rows past n_rows repeat the last valid row)
            if (a.lead_out && row0 + tid < a.n_rows) a.lead_out[a.slot_base + row0 + tid] = s_lead[tid];
        }
        __syncthreads();
        t0 = __builtin_amdgcn_readfirstlane(s_t0);
        if (t0 > 0) {
            hv0 = a.pad[(size_t)(t0 - 1) * NH + col];
            if (!urole) {
                const _Float16 vh = (_Float16)hv0, vl = (_Float16)(hv0 - (float)vh);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    hp_hi[crow(r, half) * LDP + col] = vh;
                    hp_lo[crow(r, half) * LDP + col] = vl;
                }
            }
            // table rows 0 .. t0 - 1 -> every row of the tile, h1 and fragment copy: 16 steps x 32 pieces per pass, 4 pieces a thread
            // (all four requested before the first store)
            for (int tb = 0; tb < t0; tb += 16) {
                float4 pv[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int tt = min(tb + ((k * 512 + tid) >> 5), t0 - 1);
                    pv[k] = *reinterpret_cast<const float4*>(a.pad + (size_t)tt * NH + (tid & 31) * 4);
                }
#pragma unroll 1
                for (int row = 0; row < 32; ++row) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int tt = tb + ((k * 512 + tid) >> 5);
                        if (tt < t0) store_piece(pv[k], gfm::h1_off(0, tt, tid & 31, L), gfm::h1f_off(0, tt, tid & 31, NT),
                                                 gfm::h1_lane(row, 0, L), gfm::h1f_lane(row, 0, NT));
                    }
                }
            }
        }
    }
    const int aoff = li * LDP + half * 8;

    if (urole) {
        // ------------------------------------------------------------------------------------------ u role
        half8_t wu_h[KB], wu_l[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            wu_h[kb] = buf_load_h8(rs_wg, vl16, ((NW + w) * KB + kb) * 2048);
            wu_l[kb] = buf_load_h8(rs_wg, vl16, ((NW + w) * KB + kb) * 2048 + 1024);
        }
        const int j = tid - 256;
        int lane_h[gfm::PIECES], lane_f[gfm::PIECES], pl[gfm::PIECES];
#pragma unroll
        for (int i = 0; i < gfm::PIECES; ++i) {
            lane_h[i] = gfm::h1_lane(gfm::piece_row(j, i), gfm::piece_c4(j, i), L);
            lane_f[i] = gfm::h1f_lane(gfm::piece_row(j, i), gfm::piece_c4(j, i), NT);
            pl[i] = gfm::piece_row(j, i) * LDH + gfm::piece_c4(j, i) * 4;
        }
        auto store_state = [&](int t) {                      // the fp32 state plane = the states after step t
            float4 v[gfm::PIECES];
#pragma unroll
            for (int i = 0; i < gfm::PIECES; ++i) v[i] = *reinterpret_cast<const float4*>(s_h + pl[i]);
#pragma unroll
            for (int i = 0; i < gfm::PIECES; ++i) store_piece(v[i], lane_h[i], lane_f[i], gfm::h1_step(t, L), gfm::h1f_step(t, NT));
        };
        // The gathered rows of a step sit in one of two register sets from the window behind B1 two steps earlier until they are
        // consumed: set t & 1 holds step t.  (Two sets and a loop unrolled by two, not one set and a copy: the compiler places the
        // copy of a loop-carried set at the END of the iteration that requested it and waits for the loads there.)
        struct XSet { f32x16 xr, xu, xc; };
        XSet xa, xb;
        auto gather = [&](XSet& x, int t) {
            load_x(x.xr, t, 0);
            load_x(x.xu, t, 1);
            load_x(x.xc, t, 2);
        };
        auto ustep = [&](const int t, XSet& cur, XSet& nxt) __attribute__((always_inline)) {
            RL4RS_TRG(0);
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                const half8_t ah = *reinterpret_cast<const half8_t*>(hp_hi + aoff + kb * 16);
                const half8_t al = *reinterpret_cast<const half8_t*>(hp_lo + aoff + kb * 16);
                cur.xu = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, wu_h[kb], cur.xu, 0, 0, 0);
                cur.xu = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, wu_l[kb], cur.xu, 0, 0, 0);
                cur.xu = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, wu_h[kb], cur.xu, 0, 0, 0);
            }
            RL4RS_TRG(1);
#pragma unroll
            for (int r = 0; r < 16; ++r) cur.xu[r] = gate_sigmoid(cur.xu[r]);
            put_plane(s_u, cur.xu);
            RL4RS_TRG(2);
            // (behind the update gate, so that no wait of slot U's operands sits behind fresh stores; the rc waves are still in
            // their reset-gate stretch)
            if (t > t0) store_state(t - 1);
            RL4RS_TRG(3);
            __syncthreads();                                 // B1(t)
            RL4RS_TRG(4);
            if (t + 1 < L) {
                put_plane(s_xr, nxt.xr);
                put_plane(s_xc + ((t + 1) & 1) * 4096, nxt.xc);
                if (t + 2 < L) gather(cur, t + 2);
            }
            RL4RS_TRG(5);
            __syncthreads();                                 // B2(t)
            RL4RS_TRG(6);
        };
        if (t0 < L) {
            gather(xa, t0);
            put_plane(s_xr, xa.xr);
            put_plane(s_xc + (t0 & 1) * 4096, xa.xc);
        }
        if (t0 + 1 < L) gather(xb, t0 + 1);
        __syncthreads();                                     // B2(t0 - 1)
#pragma unroll 1
        for (int t = t0; t < L; t += 2) {
            ustep(t, xa, xb);
            if (t + 1 < L) ustep(t + 1, xb, xa);
        }
        if (t0 < L) store_state(L - 1);
    } else {
        // ------------------------------------------------------------------------------------------ rc role
        half8_t wr_h[KB], wr_l[KB], wc_h[KB], wc_l[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            wr_h[kb] = buf_load_h8(rs_wg, vl16, (w * KB + kb) * 2048);
            wr_l[kb] = buf_load_h8(rs_wg, vl16, (w * KB + kb) * 2048 + 1024);
            wc_h[kb] = buf_load_h8(rs_wc, vl16, (w * KB + kb) * 2048);
            wc_l[kb] = buf_load_h8(rs_wc, vl16, (w * KB + kb) * 2048 + 1024);
        }
        f32x16 acc_r, acc_c, h_own, ug;
#pragma unroll
        for (int r = 0; r < 16; ++r) h_own[r] = hv0;
        __syncthreads();                                     // B2(t0 - 1)
#pragma unroll 1
        for (int t = t0; t < L; ++t) {
            RL4RS_TRG(0);
            get_plane(acc_r, s_xr);
            // ---- slot R: acc_r += h Wr
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                const half8_t ah = *reinterpret_cast<const half8_t*>(hp_hi + aoff + kb * 16);
                const half8_t al = *reinterpret_cast<const half8_t*>(hp_lo + aoff + kb * 16);
                acc_r = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, wr_h[kb], acc_r, 0, 0, 0);
                acc_r = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, wr_l[kb], acc_r, 0, 0, 0);
                acc_r = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, wr_h[kb], acc_r, 0, 0, 0);
            }
            RL4RS_TRG(1);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = gate_sigmoid(acc_r[r]) * h_own[r];
                const _Float16 vh = (_Float16)v;
                rp_hi[crow(r, half) * LDP + col] = vh;
                rp_lo[crow(r, half) * LDP + col] = (_Float16)(v - (float)vh);
            }
            RL4RS_TRG(2);
            __syncthreads();                                 // B1(t)
            RL4RS_TRG(3);
            get_plane(acc_c, s_xc + (t & 1) * 4096);
            get_plane(ug, s_u);
            // ---- slot C: acc_c += (r*h) Wc
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                const half8_t ah = *reinterpret_cast<const half8_t*>(rp_hi + aoff + kb * 16);
                const half8_t al = *reinterpret_cast<const half8_t*>(rp_lo + aoff + kb * 16);
                acc_c = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, wc_h[kb], acc_c, 0, 0, 0);
                acc_c = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, wc_l[kb], acc_c, 0, 0, 0);
                acc_c = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, wc_h[kb], acc_c, 0, 0, 0);
            }
            RL4RS_TRG(4);
            // ---- candidate, blend, new state planes
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float c = gate_tanh(acc_c[r]);
                float hn = __builtin_fmaf(ug[r], h_own[r] - c, c);           // u h + (1-u) c
                // the planes are a function of the ROUNDED fp32 state (k_gru_h16: left alone, the compiler fuses the fma with the
                // conversion and the hi plane then differs from (_Float16)hn in the rare double-rounding cases)
                asm volatile("" : "+v"(hn));
                h_own[r] = hn;
                const _Float16 vh = (_Float16)hn;
                hp_hi[crow(r, half) * LDP + col] = vh;
                hp_lo[crow(r, half) * LDP + col] = (_Float16)(hn - (float)vh);
                s_h[crow(r, half) * LDH + col] = hn;
            }
            RL4RS_TRG(5);
            __syncthreads();                                 // B2(t)
            RL4RS_TRG(6);
        }
    }
}

}  // namespace rl4rs
