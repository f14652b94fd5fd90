// Shared host-side helpers for librl4rs_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rl4rs_hip.h"
#include "step_lanes.hpp"      // LaneHook, lanes_join, lanes_gone (plain C++)

namespace rl4rs {

void set_error(const char* fmt, ...);

#define RL4RS_HIP_TRY(expr)                                                              \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess) {                                                          \
            ::rl4rs::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),    \
                               __FILE__, __LINE__);                                      \
            return RL4RS_EHIP;                                                           \
        }                                                                                \
    } while (0)

#define RL4RS_REQUIRE(cond, ...)                 \
    do {                                         \
        if (!(cond)) {                           \
            ::rl4rs::set_error(__VA_ARGS__);     \
            return RL4RS_EINVAL;                 \
        }                                        \
    } while (0)

#define RL4RS_LAUNCH_CHECK() RL4RS_HIP_TRY(hipGetLastError())

template <typename T>
inline int dev_alloc(T** p, size_t n) {
    *p = nullptr;
    if (n == 0) n = 1;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(p), n * sizeof(T));
    if (e != hipSuccess) {
        set_error("hipMalloc(%zu bytes) failed: %s", n * sizeof(T), hipGetErrorString(e));
        return RL4RS_ENOMEM;
    }
    return RL4RS_OK;
}

// The library's counter RNG (policy.hip's sampling, the trainers' dropout and noise, exactk.hip): one definition for every unit.
__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
// counter-based uniform STRICTLY inside (0,1): a pure function of (seed, step, row, action).  23 random bits + 0.5 is exactly
// representable in fp32, so the largest value is 1 - 2^-24; with 24 bits the top value rounded to 1.0f, and the Gumbel draw
// logit - log(-log(u)) became +inf - which let a MASKED action (logit -3.4e38) win about once per 2^24 draws
// (tests/test_gpu_policy.py::test_wider_hidden_layer_takes_the_same_paths caught it).
__device__ __forceinline__ float uniform01(uint32_t seed, uint32_t step, uint32_t row, uint32_t a) {
    uint32_t h = mix32(seed ^ mix32(step * 0x9E3779B9U + 0x85EBCA6BU) ^ mix32(row * 0xC2B2AE35U + a * 0x27D4EB2FU + 1U));
    h = mix32(h + a);
    return ((float)(h >> 9) + 0.5f) * (1.0f / 8388608.0f);
}
// N(0, 1) from the counter RNG by Box-Muller: a pure function of (seed, step, row, column).  u1 is strictly inside (0, 1).
__device__ __forceinline__ float normal01(uint32_t seed, uint32_t step, uint32_t row, uint32_t col) {
    const float u1 = uniform01(seed, step, row, 2u * col);
    const float u2 = uniform01(seed, step, row, 2u * col + 1u);
    return sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// activation codes of the GEMM epilogues (the `act` argument of rl4rs_gemm_f32 in include/rl4rs_hip.h)
enum { ACT_NONE = 0, ACT_ELU = 1, ACT_SIGMOID = 2, ACT_TANH = 3, ACT_RELU = 4 };

// Launches of the generic fp32 MFMA GEMM (gemm.hip); ldw = leading dim of W [K,N].  Optional addend: row (m / add_div) of a
// row-major [ceil(M / add_div), ldadd] array is added before the activation.
int launch_gemm_f32(const float* a, int64_t lda, const float* w, int64_t ldw, const float* bias,
                    float* c, int64_t ldc, int M, int N, int K, int act, hipStream_t st, const float* addend = nullptr,
                    int64_t ldadd = 0, int add_div = 1);

// Small-M form (one 32 x 32 tile per workgroup, K split over its four waves; launch_gemm_f32 picks it by itself when the big
// tiling would leave most CUs idle) with an optional SECOND operand pair: C = act(A W + A2 W2 + bias + addend).
int launch_gemm_small(const float* a, int64_t lda, const float* w, int64_t ldw, int K, const float* a2, int64_t lda2, const float* w2,
                      int64_t ldw2, int K2, const float* bias, float* c, int64_t ldc, int M, int N, int act, hipStream_t st,
                      const float* addend = nullptr, int64_t ldadd = 0, int add_div = 1);
// dX [M, Kin] = dY [M, Nout] W[Kin, Nout]^T, zeroed where relu_of [M, Kin] (optional: the layer's forward output) is not > 0
int launch_gemm_nt(const float* dy, int64_t ldy, const float* w, int64_t ldw, float* dx, int64_t ldx, int M, int Kin, int Nout,
                   hipStream_t st, const float* relu_of = nullptr, int64_t ldr = 0);

// dW [M, Nc] = A^T B over the Ns rows of A [Ns, lda] and B [Ns, ldb], db [Nc] (optional) = column sums of B: the trainers'
// weight-gradient reduction (policy.hip), chunk partials summed in a fixed order.  part / part_b: ceil(Ns / chunk) * M * Nc / * Nc floats.
int launch_gemm_tn(const float* A, int lda, int M, const float* B, int ldb, int Nc, int Ns, int chunk, float* part, float* part_b,
                   float* dW, float* db, hipStream_t st);

// GEMM against a weight matrix pre-packed by pack_gemm_weight (gemm.hip); C = act(A W + bias + addend) with an optional
// row-major addend [M, ldadd]
int launch_gemm_packed(const float* a, int64_t lda, const float* wp, const float* bias, float* c, int64_t ldc,
                       int M, int N, int K, int act, hipStream_t st, const float* addend = nullptr, int64_t ldadd = 0);
std::vector<float> pack_gemm_weight(const float* w, int64_t ldw, int K, int N);
// fp16x2 form (scorer_mode FP16X2): weights pre-split into fp16 hi / lo fragment planes, activations split while staged
// mirror (optional): device-visible HOST memory that receives the same output elements from the epilogue, row stride ldm
// map (optional, the three launchers below): the row map of a scorer forward (row_dedup.hpp) - tile position p works on
// row active[p / group] * group + p % group of a, c / c2 and the addend, only the first min(M, n_active[0] * group) positions are
// computed (bound read on the device, grid sized for M).  Ignored - every row computed - where a launch cannot take it (the
// weights-resident kernel, a mirror, matrices beyond 2 GB)
struct G16RowMap { const int32_t* active; const int32_t* n_active; int group; };
int launch_gemm_h16(const float* a, int64_t lda, const float* wp16, const float* bias, float* c, int64_t ldc,
                    int M, int N, int K, int act, hipStream_t st, const float* addend = nullptr, int64_t ldadd = 0,
                    float* mirror = nullptr, int64_t ldm = 0, const G16RowMap* map = nullptr);
// gather form: c[i] = act(a[rep[i]] W + addend[rep[i]]) for EVERY row i of [0, M) - rep: a scorer forward's
// representative map at group 1 (device, M entries in [0, M)).  RL4RS_EINVAL where the matrices do not fit the form
int launch_gemm_h16_gather(const float* a, int64_t lda, const float* wp16, float* c, int64_t ldc, int M, int N, int K, int act,
                           hipStream_t st, const float* addend, int64_t ldadd, const int32_t* rep);
std::vector<float> pack_gemm_weight_h16(const float* w, int64_t ldw, int K, int N);
// two chained layers in one launch (N1 <= 128, N1 % 16 == 0, N2 <= 128): c2 = act2(act1(a W1 + b1) W2 + b2)
int launch_gemm_h16_chain(const float* a, int64_t lda, const float* wp1, const float* bias1, int N1, int K1, int act1,
                          const float* wp2, const float* bias2, float* c2, int64_t ldc2, int N2, int act2, int M, hipStream_t st,
                          const G16RowMap* map = nullptr);
// two independent fp16x2 GEMMs in one launch when both take the same tile form of k_gemm_h16 (else two launches); wp2 != null:
// the problem is a chained pair of layers as in launch_gemm_h16_chain (c / ldc unused, N = N1, output c2 [M, N2])
struct GemmH16Desc {
    const float* a; int64_t lda; const float* wp; const float* bias; float* c; int64_t ldc; int M, N, K, act;
    const float* addend; int64_t ldadd;
    const float* wp2; const float* bias2; float* c2; int64_t ldc2; int N2, act2;
};
int launch_gemm_h16_pair(const GemmH16Desc& x, const GemmH16Desc& y, hipStream_t st, const G16RowMap* map = nullptr);

// device-side pack_gemm_weight_h16 (weights that change between launches): up to 4 matrices per launch, out = NT * KB * 512 + NT * 32 floats
struct PackH16Desc { const float* w; float* out; int ldw, K, N; };
struct PackH16Args { PackH16Desc d[4]; };
int launch_pack_h16_dev(const PackH16Desc* d, int n, hipStream_t st);
// whole no-grad forward of an amlp (contirl.hpp; hidden 256 x 256) in one launch, fp16x2 arithmetic; w*p = device-packed planes,
// proj [N / rep, 256] = x W1[:D] + b1, act [N, E] (E % 8 == 0, <= 64), out [N, K3] (K3 <= 64)
struct AmlpFwdH16 {
    const float* act; const float* proj; const char* w1p; const char* w2p; const char* w3p;
    const float* b2; const float* b3; float* out;
    int N, E, rep, K3, head_act;
};
int launch_amlp_fwd_h16(const AmlpFwdH16& a, hipStream_t st);

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of the FUNCTION, shared by every handle of the process: it is only ever
// raised (a second handle with a smaller shape must not lower the limit under the first one's launches - ADVICE r2 on k_ppo_pass,
// applied to every kernel whose LDS size depends on a handle's shape).  Defined in env.hip.
int raise_dyn_smem(const void* fn, size_t bytes);
int current_device();

// What the act kernel writes besides the act itself when a fused transition asks for it (step.hip; env.hip k_env_rows<1>, one wave
// per env, lane 0): the constant outputs of the transition and the logged action of the step after it.  A NULL member is left out.
struct ActTail {
    uint8_t* done; uint8_t done_v;       // done[b] = done_v
    double* zero_reward;                 // zero_reward[b] = 0.0: the reward of a step on which none is due
    int32_t* next_action; int next_cur;  // next_action[b] = the logged item id of step next_cur (the rule of rl4rs_env_offline_action)
};
// rl4rs_env_act_discrete with that tail (defined in env.hip).  rf != NULL: the act also carries the duplicate-row partition of the
// batch over to the rows it builds (row_refine.hpp; the key of an env is its resolved action id) - env_refine_fits: that launch's LDS fits
struct RowRefineArgs;
int env_act_discrete_tail(rl4rs_env* e, const int32_t* actions, const ActTail& tail, void* stream, const RowRefineArgs* rf = nullptr);
int env_act_conti_refine(rl4rs_env* e, const void* actions, int is_f64, int32_t* chosen, void* stream, const RowRefineArgs* rf);
bool env_refine_fits(const rl4rs_env* e);
// The catalogue tables of the predict_with_mask rule (env.hip k_predict_with_mask), read-only after rl4rs_env_set_catalog: what the
// offline scorers' row kernel (scorers.hpp) masks a score row with.  RL4RS_ESTATE before the catalogue is loaded
struct EnvMaskTables { int A, W, P; const uint32_t* loc_bits; const uint8_t* is_special; };      // loc_bits [4, W], is_special [A]
int env_mask_tables(const rl4rs_env* e, EnvMaskTables* out);
// Process-wide order of the calls that write an env's state rows (or the data they are built from) and of the scorer forwards that
// looked for duplicate rows: a forward's partition describes an env's rows iff its stamp is the later one (step.hip)
uint64_t next_stamp();
uint64_t env_rows_stamp(const rl4rs_env* e);
// What the last content dedup (k_row_dedup) of a scorer handle ran on, and where it left the partition
struct DienPartition {
    uint64_t stamp;                      // 0 = none
    int n_groups, group;
    const float* dense; const int32_t* cat; const int32_t* slots; const int32_t* order;
    const int32_t* rep; const int32_t* active; const int32_t* n_active;
};
void dien_last_partition(const rl4rs_dien* n, DienPartition* out);
bool dien_takes_partition(const rl4rs_dien* n);                          // row dedup on, in a form rl4rs_dien_set_row_partition serves
const int32_t* dien_row_order(const rl4rs_dien* n, int n_groups);         // the order a forward of n_groups groups would process them in

// The NEXT rl4rs_dien_forward's observation also goes to `host_visible` (device-visible pinned host memory, [R, 256] floats) from
// the head GEMM's epilogue - step.hip's reference-shaped records (dien.hip); dien_obs_mirror_used: did that forward take it?
void dien_set_obs_mirror(rl4rs_dien* n, float* host_visible);
bool dien_obs_mirror_used(const rl4rs_dien* n);
// The NEXT forward (one call) scores groups whose rows share the cache slot but not the category columns - the observation rows of
// one env at consecutive steps of a replay (step.hip): the per-row category kernel runs, and with obs == NULL the head
// output of the representatives' rows lands in `head_out` [R, 256] (row rep * group + k), not in the handle's own scratch
void dien_set_group_rows(rl4rs_dien* n, float* head_out);
// The last forward left the duplicates' internal rows (all-feature, scores, query) to rl4rs_dien_buffer (PlanExpand::Lazy): forget
// that - the caller is about to rewrite the partition arrays that forward ran on (step.hip, in front of an act that refines them)
void dien_drop_pending_expand(rl4rs_dien* n);
// Rounds (waves of workgroups over the chip's CUs) of the k_augru_x launch of a forward of B groups of `group` rows of which `live`
// are expected to be distinct (row_dedup.hpp), under the row-tile form rl4rs_dien_forward would pick for it; -1: the forward does not
// run k_augru_x (fp32 mode, augru_h16) or does not fit the handle's max_rows.  step.hip decides with it whether a reward step
// scores the state row inside the reward forward.
int64_t dien_augru_rounds(const rl4rs_dien* n, int B, int live, int group);
// Would that forward's k_augru_x launch run the 64-row form (automatic rule or pinned)?
bool dien_augru_rows64(const rl4rs_dien* n, int B, int group);
// ... and would the automatic rule alone choose it (enough workgroups to fill the chip twice over), whatever the pin says?
bool dien_augru_rows64_auto(const rl4rs_dien* n, int B, int group);

// The stepper's two lanes (step.hip, step_lanes.hpp) may have a transition in flight on streams of their own.  The env and
// the scorer a stepper is attached to hold a pointer to its hook, and every entry point that reads or writes what a lane may still
// touch calls lanes_join first: with a stream, that stream waits for the lanes (nothing blocks); without one (an entry point that
// is given none) the host waits.  Idle lanes cost a null check and a flag.  LaneHook and the rules of who tells whom when a handle
// or the stepper is destroyed: step_lanes.hpp.  These return where the handle keeps its pointer to the hook
const LaneHook** env_lane_slot(rl4rs_env* e);
const LaneHook** dien_lane_slot(rl4rs_dien* n);
// The env keeps two sets of state rows (BUF_DENSE / BUF_CATEGORY): env_flip_rows makes the other one current for the acts that
// follow, so that an act may build its rows while the previous transition's forward still reads the set before.  *dense / *cat: the
// current set (what rl4rs_env_buffer returns)
void env_flip_rows(rl4rs_env* e);
void env_rows_current(const rl4rs_env* e, const float** dense, const int32_t** cat);
// A second set of the scratch an observation-sized forward writes (query, q-side term, scores, all-feature rows, table addend), for
// `rows` rows: dien_forward_lane(.., set = 1, ..) runs on it, beside a forward on the handle's first set.  The lane forwards join
// nothing themselves (the stepper orders them); `home`: the caller's stream, on which rl4rs_dien_buffer completes what they left
int dien_reserve_lane_scratch(rl4rs_dien* n, int rows);
// what that set holds, in bytes: padded rows x (Fld + U + E + S * ATT_H1 + S * L [+ OBS_DIM]) floats; 0 = none reserved
int64_t dien_lane_scratch_bytes(const rl4rs_dien* n);
int dien_forward_lane(rl4rs_dien* n, int set, int32_t R, const float* dense, const int32_t* cat, const int32_t* slots, float* obs,
                      void* stream, void* home);
// The same with every argument of a forward: `group` rows per env and probabilities for the reward step's forward (set 0,
// or set 1 once the stepper has reserved it at that forward's size: DESIGN 42), and `after_dedup` (a hipEvent_t, or NULL) recorded on `stream` behind the
// duplicate-row stage - the reset's observation forward looks for its duplicates itself, and the partition is all the next act needs;
// `before_augru` (a hipEvent_t, or NULL): `stream` waits for it in front of the AUGRU launch (the reward step's, which wants the whole chip)
int dien_forward_lane_full(rl4rs_dien* n, int set, int32_t R, int32_t group, const float* dense, const int32_t* cat, const int32_t* slots,
                           float* obs, float* prob, void* stream, void* home, void* after_dedup, void* before_augru);
// rl4rs_env_build_complete_rows / rl4rs_env_reward_split without the join of the lanes (env.hip): a lane's own launches
int env_build_complete_rows_lane(rl4rs_env* e, int32_t rows_per_env, void* stream);
int env_reward_split_lane(rl4rs_env* e, const float* probs, const float* p_last, double* reward, void* stream);
// The state rows "after act c under the logged actions" of every env for c in [c0, c0 + n), env-major [B * n] (env.hip, DESIGN 40;
// Slate only, no join: step.hip orders it behind the act of c0).  prev_actions up to c0 are the env's, behind c0 the log's.
// `part` (or NULL): the partition the act of c0 left, copied for the forward of these rows - an env whose logged actions behind c0
// differ from its representative's becomes a representative of its own (appended to the copy of the active list)
struct AheadPart {
    const int32_t* rep; const int32_t* active; const int32_t* cnt;      // [B], [cnt[0]], [0] n_active
    int32_t* rep_out; int32_t* active_out; int32_t* cnt_out;            // the copies; cnt_out[0] holds cnt[0] when the kernel starts
};
int env_build_ahead_rows_lane(rl4rs_env* e, int32_t c0, int32_t n, float* dense_out, int32_t* cat_out, const AheadPart* part, void* stream);
bool dien_lane_path(const rl4rs_dien* n, int rows);      // fp16x2 on k_augru_x / k_augru_xs, and the second set holds `rows` rows
int dien_n_cu(const rl4rs_dien* n);

// Training-mode recurrences as persistent kernels (recur_train.hpp, compiled into dien.hip; called from dientrain.hpp).
// Arrays are per sequence input (S <= 4 inputs run in ONE launch, grid.y = S); saved tensors are [N * L, Hd] row-major.
struct RecurTrainFwd {
    int N, L, S, Hd;
    const int32_t* iota;                  // device [N]: 0, 1, 2, ... (row n reads row block n of its input's pre-activations)
    const float* a1[4];                   // x-side pre-activations incl. bias, [N * L, 3 Hd] = [r | u | c]
    const float* wg[4]; const float* wc[4];      // h-side weights in MFMA fragment order (launch_pack_frag): [Hd x 2Hd], [Hd x Hd]
    const float* att[4];                  // attention rows [N, L] (AUGRU) or NULL (GRU)
    float *R[4], *U[4], *C[4], *H[4], *RH[4];    // out
    int hard;                             // keras recurrent_activation = hard_sigmoid for r / u (the lstm family's GRUs)
    int xblk[3];                          // column block of the r / u / c pre-activations in a1 (TF cells 0,1,2; keras [z|r|h]: 1,0,2)
};
struct RecurTrainBwd {
    int N, L, S, Hd;
    const float *R[4], *U[4], *C[4], *H[4];
    const float* att[4];
    const float* up_last[4]; int64_t ld_up;      // gradient of the final state (row stride ld_up) or NULL
    const float* up_all[4];               // gradient of every state or NULL
    const float* wcT[4]; const float* wgT[4];    // transposed h-side weights in fragment order: [Hd x Hd], [2Hd x Hd]
    // out: pre-activation gradients of the reset / update gates (row stride ld_g) and of the candidate (row stride ld_c), one
    // row per (sample, step).  TF cells: dr = dAg, du = dAg + Hd, ld_g = 2Hd; dc = dAc, ld_c = Hd.  keras [z|r|h] rows of
    // width 3Hd: du = dA, dr = dA + Hd, dc = dA + 2Hd, ld_g = ld_c = 3Hd.
    float *dr[4], *du[4], *dc[4];
    int64_t ld_g, ld_c;
    float* d_score[4];                    // out (AUGRU): d a_t [N, L] or NULL
    int hard;                             // hard_sigmoid gates: derivative 0.2 inside (0, 1), 0 at the clamps
};
int launch_recur_train_fwd(const RecurTrainFwd& f, hipStream_t st);
int launch_recur_train_bwd(const RecurTrainBwd& b, hipStream_t st);
// W rows k_off.. (leading dim ld) -> fragment order; transpose = 1 packs W^T (K = columns of W, N = rows taken)
int launch_pack_frag(const float* w, int64_t ld, int k_off, int K, int N, int transpose, float* out, hipStream_t st);
// the same for a K-slice of a taller operand: rows [k_dst, k_dst + K) of a [K_total x N] fragment buffer
int launch_pack_frag_slice(const float* w, int64_t ld, int k_off, int K, int N, int transpose, float* out, int K_total, int k_dst,
                           hipStream_t st);

// Power-of-two prescale of a weight tile that goes through the fp16 hi + lo split: s = 1 while the tile sits comfortably inside
// fp16 (2^-6 <= max |w| < 2^14), else s = 2^k with max |w| * s in [2^13, 2^14) - multiplying by s is exact in fp32, hi = fp16(w s)
// is then neither out of range (large tiles) nor a subnormal with a handful of significant bits (tiny tiles), and the kernels
// divide the accumulator by s (exactly) in their epilogues: the split form has no weight-range condition.  ORDINARY tiles are
// left alone on purpose.  Normalising every tile (so that every lo part becomes a normal fp16 number with all 10 mantissa bits
// in use) was measured: nothing to gain against the fp64 oracle (obs 2.2e-6 either way - the fp32 accumulation dominates),
// and the denser operand bits cost 2 % of the recurrence's speed on this power-limited kernel (same-box A/B);
// -DRL4RS_PRESCALE_UP builds that form.
inline float pow2_prescale(float maxabs) {
    if (!(maxabs > 0.f) || !(maxabs < 3.0e38f)) return 1.f;
    int e = 0;
    (void)frexpf(maxabs, &e);             // maxabs = m * 2^e, m in [0.5, 1)  ->  maxabs * 2^(14 - e) in [2^13, 2^14)
    int k = 14 - e;
#ifndef RL4RS_PRESCALE_UP
    if (e <= 14 && e > -6) k = 0;         // 2^-6 <= maxabs < 2^14: as is
#endif
    if (k > 100) k = 100;                 // keep s (and s * other weights) far from the fp32 range ends
    if (k < -100) k = -100;
    return ldexpf(1.f, k);
}

// fp32 -> fp16 bits, round to nearest even (subnormals kept)
inline uint16_t f32_to_f16(float f) {
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (x > 0x7f800000u ? 0x200u : 0));
    if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                 // overflow -> inf
    if (x < 0x38800000u) {                                                   // subnormal half (or zero)
        if (x < 0x33000000u) return (uint16_t)sign;
        const int e = (int)(x >> 23);
        uint32_t m = (x & 0x7fffffu) | 0x800000u;
        const int shift = 126 - e;                                           // 14..24
        uint32_t r = m >> shift;
        const uint32_t rem = m & ((1u << shift) - 1), halfway = 1u << (shift - 1);
        if (rem > halfway || (rem == halfway && (r & 1))) ++r;
        return (uint16_t)(sign | r);
    }
    uint32_t r = ((x - 0x38000000u) >> 13);
    const uint32_t rem = x & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (r & 1))) ++r;
    return (uint16_t)(sign | r);
}
inline float f16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    uint32_t e = (h >> 10) & 0x1f, m = h & 0x3ffu, x;
    if (e == 0) {
        if (m == 0) x = sign;
        else { int s = 0; while (!(m & 0x400u)) { m <<= 1; ++s; } m &= 0x3ffu; x = sign | ((uint32_t)(113 - s) << 23) | (m << 13); }
    } else if (e == 31) x = sign | 0x7f800000u | (m << 13);
    else x = sign | ((e + 112) << 23) | (m << 13);
    float f;
    memcpy(&f, &x, 4);
    return f;
}

}  // namespace rl4rs
