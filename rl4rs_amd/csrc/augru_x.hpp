// k_augru_x: the AUGRU recurrence of the DIEN scorer in fp16x2 form, second generation (included by dien.hip).
//
// Same arithmetic as k_augru_h16 (rl4rs/nets/utils.py:120-124 via deepctr VecAttGRUCell; operands split into fp16 hi + lo,
// every product as W_hi*h_hi + W_lo*h_hi + W_hi*h_lo on v_mfma_f32_32x32x16_f16, fp32 accumulation), different machine
// mapping.  What bounded k_augru_h16 (profiles/r01g_pmc.md: matrix pipe 47-52 % busy): the two waves of a SIMD moved through
// the step in lock step, so neither's epilogue hid behind the other's MFMAs (a ~6K-cycle exposed candidate epilogue per
// ~20K-cycle step), 786 KB of weight fragments per step through the 64 B/clk L1 return path, and 384 dword-per-lane
// projection loads per step whose HBM latency sat in the in-order vector-memory queue in front of the weight ring.
//
//   * TRANSPOSED tiles: the MFMA computes (W^T h^T) - A = weight fragment, B = state fragment - so a lane owns ONE batch row and
//     16 hidden columns in runs of 4: the attention score is one scalar per lane and step, new state leaves as packed 8-byte
//     LDS writes (4 fp16 values), the final state as 16-byte stores.
//   * ROLES: 8 waves, wave w owns hidden columns [32w, 32w+32) of all three gates.  Waves 0-3 ("early": k-blocks 0..7 of the
//     state) and 4-7 ("late") land pairwise on the same SIMD (wave k and k+4) and run the candidate phase out of step:
//         all    R (late k-blocks) , U            || reset gate r = sigmoid(acc_r), r*h -> fp16 planes
//         -- barrier 1 (r*h planes complete)
//         early  C || update gate, then candidate + blend -> early columns of h'    (VALU while its partner runs C)
//         late   update gate, then C                                                 (MFMA while its partner blends)
//         -- barrier a (early half of h' complete)
//         all    R of the NEXT step on the early k-blocks;  late: || candidate + blend -> late columns of h'
//         -- barrier b
//     so whenever one wave of a SIMD is in an epilogue its partner keeps the matrix pipe busy, and the next step's reset-gate
//     product starts on the half of the new state that is already written.  RL4RS_X_USPLIT: between barrier a and barrier b the
//     early waves - whose blend, and with it acc_u, is done - also run the next step's update-gate products on that half (role_item).
//   * cached input projections through LDS-DMA: one issue window per step (right in front of the register-resident weight
//     items, i.e. in front of a stretch without vector-memory waits) requests the three gates' rows of step t+1 with
//     buffer_load ... lds: 4 instructions per gate, each one 8 rows x 128 contiguous bytes (8 cache lines instead of the 32 a
//     row-per-lane register load touches), no staging registers; a chunk rotation in the SOURCE address makes the lane-linear
//     LDS image conflict-free for the row-per-lane reads that feed the accumulators (MFMA C-in).
//   * LDS (all 160 KB): state planes in slab order [k-block][k-half][row][8 halfs] - fragment reads and 8-byte writes are
//     conflict-free without padding (64 KB) - and 3 x 4 KB of projection staging per wave (96 KB).
//   * out-of-range rows (|h| >= 6e4: the fp16 planes cannot carry them; or NaN) are POISONED: the whole output row becomes NaN,
//     so the observation / click probability / reward of that env is NaN on the device without any host synchronisation, and
//     the sticky status bit is raised as before (rl4rs_dien_status).
#pragma once

namespace rl4rs {
namespace xk {
constexpr int NI = 48;                                       // weight items per wave and step
constexpr int gate(int i) { return i < 8 ? 0 : (i < 24 ? 1 : (i < 40 ? 2 : 0)); }
constexpr int kb(int i) { return i < 8 ? 8 + i : (i < 24 ? i - 8 : (i < 40 ? i - 24 : i - 40)); }
constexpr bool from_rh(int i) { return i >= 24 && i < 40; }  // B operand: r*h planes (candidate) or h planes
constexpr bool after_barrier(int i) { return i == 0 || i == 24 || i == 40; }
#ifndef RL4RS_X_DMA_AUX
#define RL4RS_X_DMA_AUX 2        // cache-policy bits of the projection DMA (1 sc0, 2 nt, 16 sc1).  nt: a projection row is used once (by the
                                // envs of one history, which run side by side), so it should not push the weight fragments - re-read 64
                                // times per launch - out of L2.  Same-box A/B, 5 alternating pairs: 11.41 -> 11.32 ms per episode-batch
                                // (+0.8 %), SeqSlate T=32 38.55 -> 38.12 ms (+1.1 %); sc0 flat, nt|sc0 like nt.  0 = round 2 .. 5's default
#endif
#ifndef RL4RS_X_AB
#define RL4RS_X_AB 0            // timing ablations (results are WRONG when non-zero): 1 no epilogue math, 2 no weight streaming,
#endif                          // 4 no projection DMA / reads, 8 no state-fragment reads, 16 no barriers
#ifndef RL4RS_X_SGB
#define RL4RS_X_SGB 0           // VALU instructions pinned behind each MFMA of an item that carries epilogue work (0 = compiler's order)
#endif
#ifndef RL4RS_X_PRIO
#define RL4RS_X_PRIO 0
#endif
#ifndef RL4RS_X_SPREAD
#define RL4RS_X_SPREAD 0
#endif
// where in a step the staged projections of the update gate / the candidate are read into their accumulators (MFMA C-in): right
// in front of the gate's first item (8 / 24) or some items earlier, so that the LDS round trip is not in front of that item's MFMAs
// (both accumulators are free from item 0; the staging is per wave and was filled one step ago; must stay below the DMA window)
#ifndef RL4RS_X_LATE_UPD_SHADOW
#define RL4RS_X_LATE_UPD_SHADOW 0   // 1: the late waves also compute their update gate in the shadow of their first C items (like the early
#endif                              // waves) instead of as a VALU-only stretch in front of them (round 4 A/B)
#ifndef RL4RS_X_XU_AT
#define RL4RS_X_XU_AT 8
#endif
#ifndef RL4RS_X_XC_AT
#define RL4RS_X_XC_AT 24
#endif
#ifndef RL4RS_X_SPLITPAIR
#define RL4RS_X_SPLITPAIR 1     // plane_store through split_h16_pair (v_cvt_pk_f16_f32 + v_fma_mix_f32: 2 VALU per element instead of
#endif                          // ~3; same roundings, bit-identical planes; same-box A/B: 0.8595 -> 0.8503 ms per launch) - 0: the C++ casts
#ifndef RL4RS_X_PEEL
#define RL4RS_X_PEEL 1          // boundary steps without their vanishing products (see "BOUNDARY STEPS" at the step loop); 0: every step runs all
#endif                          // 48 items.  RL4RS_X_PEEL_MT2: the same switch for the 64-row form alone
#ifndef RL4RS_X_PEEL_MT2
#define RL4RS_X_PEEL_MT2 RL4RS_X_PEEL
#endif
#ifndef RL4RS_X_USPLIT
#define RL4RS_X_USPLIT 2        // role-specialised step (needs the rotated loop of RL4RS_X_PEEL): the early waves run the NEXT step's update-gate
#endif                          // items on k-blocks 0..7 between barrier a and barrier b (see role_item).  0: one schedule for both roles,
                                // 1: the 64-row form alone, 2: both forms and k_augru_xs.  Same-box A/B, 5 alternating rounds
                                // (profiles/r22_ab.md): value 1 flat (7.405 -> 7.384 ms per episode-batch, inside the noise), value 2
                                // 7.405 -> 7.184 ms (-3.0 %): the gain is the 32-row form's
#ifndef RL4RS_X_AMAX
#define RL4RS_X_AMAX 0          // 1: track max |h| over the steps for the range check (0: the final state alone decides, see the epilogue)
#endif
// which items of a step keep their weight fragments in registers: a contiguous stretch behind the projection issue window
// (RL4RS_X_SPREAD = 0) or every (48 / NRES)-th item (1: uniform load on the L1 return path)
// (RL4RS_X_RESMASK: an explicit 48-bit item mask for experiments, 32-row form only, with RL4RS_X_WINDOW = the item the
// projection requests are issued in front of)
template <int NRES> constexpr bool is_res(int i) {
#ifdef RL4RS_X_RESMASK
    if (NRES == RL4RS_X_NRES) return ((RL4RS_X_RESMASK >> i) & 1ull) != 0;
#endif
    return RL4RS_X_SPREAD ? ((i % (NI / NRES)) == (NI / NRES) - 1 && i / (NI / NRES) < NRES) : (i >= 40 - NRES && i < 40);
}
// order of a step's items by role (RL4RS_X_USPLIT).  Sequence position s of a step counts from barrier b: positions [0, SB) run
// between barrier b and barrier a, positions [SB, 48) between barrier a and barrier b (SB = role_stretch).  One schedule for both
// roles (split = false): position = item.  The early role of the split schedule: the update-gate items on k-blocks 0..7 (items
// 8..15: the early half of the new state is complete at barrier a and the early waves' acc_u is dead from their blend on) run
// behind the reset-gate items of the same - next - step, and the stretch behind barrier b keeps the update-gate items 16..23:
//     0..7 (R late)  16..23 (U late)  24..39 (C)  |  40..47 (R early of step t+1)  8..15 (U early of step t+1)
// Every accumulator keeps its operation order (C-in projection, then k-blocks 0..15 ascending); all moves are by multiples of 8, so
// the parity of an item (its state-fragment buffer) still alternates along the sequence.
constexpr int role_item(bool split, int s) { return !split ? s : (s < 8 ? s : (s < 40 ? s + 8 : s - 32)); }
constexpr int role_stretch(bool split) { return split ? 32 : 40; }
// compile-time tables of a step's schedule: index of a resident item in the register file, position of a streamed item in
// the (cyclic) streamed sequence that starts at the first streamed item behind barrier a, and its inverse
struct Sched { int res_idx[NI]; int js_of[NI]; int item_of[NI]; int js_first; };
template <int NRES> constexpr Sched make_sched(bool split = false) {
    Sched s = {};
    int n = 0;
    for (int i = 0; i < NI; ++i) { s.res_idx[i] = n; n += is_res<NRES>(i) ? 1 : 0; }
    int k = role_stretch(split);
    while (is_res<NRES>(role_item(split, k % NI))) ++k;
    int js = 0;
    for (int c = 0; c < NI; ++c) {
        const int i = role_item(split, (k + c) % NI);
        s.js_of[i] = js;
        if (!is_res<NRES>(i)) { s.item_of[js] = i; ++js; }
    }
    int f = 0;
    while (is_res<NRES>(role_item(split, f))) ++f;
    s.js_first = s.js_of[role_item(split, f)];             // step 0 enters the sequence at its first streamed item >= 0
    return s;
}
}  // namespace xk

typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

#ifdef RL4RS_X_TRACE       // s_memtime marks of workgroup (0,0), steps 8..11: [wave][step][mark]
#define RL4RS_XT(k) do { if (a.trace && blockIdx.x == 0 && blockIdx.y == 0 && lane == 0 && t >= 8 && t < 12) \
        a.trace[(wave * 4 + (t - 8)) * 8 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define RL4RS_XT(k) do { } while (0)
#endif

// MT = 1: 32-row workgroups, per-row projection staging (any row -> slot map).  MT = 2: 64-row workgroups for launches whose
// rows come in groups of 8 consecutive rows per cache slot (the reward forward: 8 complete-state rows per env): every weight
// fragment feeds two row tiles (half the weight bytes per row through the L1 return path), and the 8 distinct projection rows
// of the workgroup are staged once (1 KB per gate and wave, one DMA instruction).
// PAD (instantiated for MT = 1): steps below a row's count of leading zero ids read the projections of the pad slot (RecurArgs::lead / pad_slot).
// GRP (MT = 2 only): consecutive rows per cache slot.  8: a tile is 8 whole groups.  9 (a reward forward that also scores the state
// row: 9 complete-state rows per env): a tile is 7 whole groups = 63 positions, row0 advances by 63, tile row r reads staged row
// r / 9, and tile position 63 is a clamped position - it computes batch position min(row0 + 63, n_rows - 1), whose slot lane group
// 7 of the projection DMA stages, and is not stored (the workgroup of the next tile stores that row).  The step loop is the same.
template <int MT, int NRES, int RING, bool PAD = false, int GRP = 8>
__global__ __launch_bounds__(512) void k_augru_x(RecurArgs a) {
#include "augru_x_body.inc"
}

// MT = 1: 64 KB planes + 96 KB staging = all 160 KB;  MT = 2: 128 KB planes + 24 KB staging
static size_t augru_x_smem(int mt) { return (size_t)mt * 4 * 32 * 256 * 2 + (size_t)8 * (mt == 1 ? 3 * 4096 : 3 * 1024); }

}  // namespace rl4rs
