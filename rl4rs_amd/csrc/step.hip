// One batched env transition as ONE library call: RecSimBase._step (rl4rs/env/base.py:157-170) =
//   samples.act(action)            slate.py:193-214 / seqslate.py:92-126
//   next_obs = obs_fn(state)       slate.py:244-279   (simulator_obs layer of the scorer)
//   reward   = forward(model, ..)  slate.py:281-308 / seqslate.py:136-160 (only when a reward is due)
//   done     = step >= max_steps-1 base.py:165-168
// composed from the same entry points the host facade uses one by one (rl4rs_env_act_*, rl4rs_dien_forward / rl4rs_simnet_forward,
// rl4rs_env_build_complete_rows, *_head_prob, rl4rs_env_reward_split, rl4rs_env_obs_mask): identical kernels in identical order,
// so the results are bit-identical to the composed path (tests/test_gpu_facade.py::test_fused_step_is_bit_identical).  One
// exception in order, not in results: a reward step may score the state row inside the reward forward (fold_obs below).  Nothing is
// allocated and nothing synchronises inside: all scratch belongs to the binding created by rl4rs_env_attach_scorer.
#include "common.hpp"
#include "row_refine.hpp"
#include "step_lanes.hpp"

using namespace rl4rs;

// One of the stepper's two lanes (step_lanes.hpp): a stream, its events and its own copy of what a transition hands out
struct StepLane {
    hipStream_t st;
    hipEvent_t act_done;       // behind the act: env state, partition and logged-action row of the transition are written
    hipEvent_t done;           // behind the lane's last launch
    hipEvent_t handed;         // on the CALLER's stream, behind the copy of obs / reward out of the lane's buffers
    float* obs;                // [B, 256]
    double* reward;            // [B]
};

struct rl4rs_stepper {
    rl4rs_env* env;
    rl4rs_dien* dien;          // exactly one of dien / simnet is set
    rl4rs_simnet* simnet;
    const int32_t* slots;      // [seq_num, B] cache slot of every env row per sequence input (caller-owned device memory)
    int32_t seq_num;
    rl4rs_env_cfg cfg;
    int n_complete;
    float* probs;              // [B * n_complete] click probabilities of the complete-state rows (n_complete - 1 per env in the two-forward order)
    float* p_last;             // [B] probability of the state row just scored (= the last complete-state row)
    const float* dense; const int32_t* cat; const int32_t* seq1; const float* c_dense; const int32_t* c_cat;
    // rl4rs_env_step_discrete: the act kernel also writes done, the zero reward and the NEXT step's logged action (ActTail) - no
    // k_step_tail launch, and a replay loop needs no rl4rs_env_offline_action launch between two steps
    bool act_tail;             // rl4rs_stepper_set_act_tail (default on)
    bool obs_fold;             // rl4rs_stepper_set_obs_fold (default on): a reward step scores the state row inside the reward forward
    int distinct_hint;         // rl4rs_stepper_set_distinct_hint: envs expected to stay distinct under the scorer's row dedup (default B)
    int probs_rows;            // rows per env the last reward step left in `probs`: n_complete (folded), n_complete - 1 (+ p_last), 0 = none yet
    int32_t* next_off;         // [max_steps + 1][B]: row c = the logged item ids of step c, written by the step that led to it - a row
                               // of its own per step of an episode, so a caller may hold what it was handed until the episode ends
    int next_off_cur;          // the step whose row the last transition wrote, -1 = none
    // The duplicate-row partition of the env batch, carried from forward to forward (row_refine.hpp): valid from the act
    // behind a content dedup of the state rows (the reset observation) until a reset, a page turn (the slot table changes) or a
    // changed row order.  While it is valid every scorer forward of a transition gets it (rl4rs_dien_set_row_partition).
    bool carry;                // rl4rs_stepper_set_partition_carry (default on)
    bool part_valid;           // part_rep[part_cur] / part_active / part_cnt describe the rows the last act built
    bool part_now;             // ... and the transition in flight hands them to its forwards
    int part_cur;
    int32_t* part_rep[2];      // [B] each, used in turn: an act reads one and writes the other
    int32_t* part_active;      // [B]
    int32_t* part_cnt;         // [0] n_active, [1] ticket, [2] envs that split off in the act in flight
    const int32_t* part_order; // the scorer's row order the active list was built in
    uint64_t part_stamp;       // the env's row stamp behind the act that left the partition
    // Two lanes for consecutive transitions (rl4rs_stepper_set_step_overlap, default on).  A lane transition flips the env's state-row
    // set and the active list / counter pair below, so that its act writes none of what the previous forward still reads.
    bool overlap;
    bool reset_lane;           // rl4rs_stepper_set_reset_lane (default on): rl4rs_stepper_observe runs the reset's forward on a lane
    bool reward_lane;          // rl4rs_stepper_set_reward_lane (default on): a folded reward step runs on lane 0 beside the transition before it
    bool lanes_made;
    StepLane lane[2];
    hipEvent_t ev_entry;       // recorded on the caller's stream where a lane has to wait for it
    LaneState lstate;
    LaneHook hook;             // what the env and the scorer call before they touch anything a lane may have in flight
    LaneLinks links;           // where the env / the scorer keep their pointer to `hook`; forgotten when that handle goes first
    int32_t* part_active_alt;  // [B]   the pair a lane transition's act writes (then exchanged with part_active / part_cnt)
    int32_t* part_cnt_alt;     // [4]
    // Replay-ahead (step_lanes.hpp): the observation rows of the remaining transitions of a replay episode in one forward.
    // Buffers of their own, made by the first forward (ensure_ahead): nothing the acts, the lanes' forwards or the reward step write.
    int replay_ahead;          // rl4rs_stepper_set_replay_ahead: 0 off, 1 where the automatic rule runs the 64-row form (default), 2 also where it is pinned
    AheadState ahead;
    float* ah_dense;           // [B * 9, Dn]   the rows (k_env_rows_ahead)
    int32_t* ah_cat;           // [B * 9, Cn]
    float* ah_obs;             // [B * 9, 256]  the head output of the representatives' rows, until the last hand-out
    int32_t* ah_rep;           // [B]  the partition the forward ran on: the act's, envs whose logged actions part later split off
    int32_t* ah_active;        // [B]
    int32_t* ah_cnt;           // [4]
    // The reward step beside the group forward (step_lanes.hpp): with the scorer's second scratch set at B * n_complete
    // rows the folded reward step behind a group forward takes lane 1 and set 1
    bool reward_beside;        // rl4rs_stepper_set_reward_beside (default on)
    bool beside_tried;         // ensure_ahead has asked for the full-size set ...
    bool beside_ready;         // ... and got it; false for good where the allocation failed
    hipStream_t copy_stream;   // rl4rs_env_step_record_host: early device-to-host copies run here, beside the scorer's kernels
    hipEvent_t ev_ready, ev_copied;
};

namespace {

int scorer_forward(rl4rs_stepper* s, int R, int group, const float* dense, const int32_t* cat, float* obs, float* prob, void* stream) {
    if (s->part_now && s->dien) {      // groups are per env in every forward of a transition: the env partition is the group partition
        int rc = rl4rs_dien_set_row_partition(s->dien, s->part_rep[s->part_cur], s->part_active, s->part_cnt, s->cfg.batch_size);
        if (rc) return rc;
    }
    return s->dien ? rl4rs_dien_forward(s->dien, R, group, dense, cat, s->slots, obs, prob, stream)
                   : rl4rs_simnet_forward(s->simnet, R, group, dense, cat, s->slots, obs, prob, stream);
}
int scorer_head_prob(rl4rs_stepper* s, int R, const float* obs, float* prob, void* stream) {
    return s->dien ? rl4rs_dien_head_prob(s->dien, R, obs, prob, stream) : rl4rs_simnet_head_prob(s->simnet, R, obs, prob, stream);
}
int scorer_encode(rl4rs_stepper* s, int q, const int32_t* ids, int n, void* stream) {
    return s->dien ? rl4rs_dien_encode(s->dien, q, ids, n, 0, stream) : rl4rs_simnet_encode(s->simnet, q, ids, n, 0, stream);
}

// rl4rs_set_host_mirror(1): the head GEMM's epilogue writes the observation to the pinned host block itself.  OFF by default:
// measured on one box, 2 alternating pairs of 12 episode-batches (profiles/r06h_host_mirror.txt): 13.10 / 13.16 ms with the copy
// engine, 13.20 / 13.21 ms with the mirror - stores to host memory drain no faster than the copy engine moves the same 4 MB, and
// the GEMM's waves hold their CUs while they do.
int g_host_mirror = 0;

int ensure_copy_stream(rl4rs_stepper* s) {
    if (!s->copy_stream) {
        RL4RS_HIP_TRY(hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking));
        RL4RS_HIP_TRY(hipEventCreateWithFlags(&s->ev_ready, hipEventDisableTiming));
        RL4RS_HIP_TRY(hipEventCreateWithFlags(&s->ev_copied, hipEventDisableTiming));
    }
    return RL4RS_OK;
}

// the constant outputs of a transition in one launch: done flags, and the zero reward of a step on which none is due
__global__ void k_step_tail(uint8_t* done, uint8_t v, double* zero_reward, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        if (done) done[i] = v;
        if (zero_reward) zero_reward[i] = 0.0;
    }
}

// what a lane transition hands out: observation and reward from the lane's buffers into the caller's, on the caller's stream
__global__ void k_lane_handout(const float* __restrict__ obs_src, float* __restrict__ obs_dst, int64_t n_obs,
                               const double* __restrict__ reward_src, double* __restrict__ reward_dst, int B) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_obs) obs_dst[i] = obs_src[i];
    if (reward_dst && i < B) reward_dst[i] = reward_src[i];
}

// what a replay-ahead transition hands out: row k of every env's representative in the group forward's head output, and
// the zero reward of a step on which none is due.  One float4 per thread, 64 threads per env.
__global__ void k_ahead_handout(const float* __restrict__ src, const int32_t* __restrict__ rep, int n, int k, float* __restrict__ obs_dst,
                                double* __restrict__ reward_dst, int B) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * 64) return;
    const int b = (int)(i >> 6), q = (int)(i & 63);
    reinterpret_cast<float4*>(obs_dst)[i] = reinterpret_cast<const float4*>(src + ((size_t)rep[b] * n + k) * 256)[q];
    if (reward_dst && i < B) reward_dst[i] = 0.0;
}

// ---- lanes
// the stream a caller gave waits for everything in flight on the lanes (have_stream == 0: the host does)
int lanes_wait(rl4rs_stepper* s, void* stream, int have_stream) {
    (void)ahead_cancel(s->ahead);      // whoever joins is about to touch the env or the scorer: the rows not handed out yet are dropped
    const bool used[2] = {s->lstate.used[0], s->lstate.used[1]};
    if (!lane_join(s->lstate)) return RL4RS_OK;
    for (int i = 0; i < 2; ++i) {
        if (!used[i]) continue;
        if (have_stream) RL4RS_HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, s->lane[i].done, 0));
        else RL4RS_HIP_TRY(hipStreamSynchronize(s->lane[i].st));
    }
    return RL4RS_OK;
}
int hook_join(void* ctx, void* stream, int have_stream) { return lanes_wait(reinterpret_cast<rl4rs_stepper*>(ctx), stream, have_stream); }
// the env or the scorer is being destroyed, or another stepper took it over (it has joined the lanes first): this stepper no longer
// touches that handle - not in its own destroy either - and runs no lane transition from here on
void hook_gone(void* ctx, int which) {
    rl4rs_stepper* s = reinterpret_cast<rl4rs_stepper*>(ctx);
    lane_links_gone(s->links, which);
    s->overlap = false;
}

int make_lanes(rl4rs_stepper* s) {
    const size_t B = (size_t)s->cfg.batch_size;
    RL4RS_HIP_TRY(hipEventCreateWithFlags(&s->ev_entry, hipEventDisableTiming));
    for (int i = 0; i < 2; ++i) {
        StepLane& l = s->lane[i];
        RL4RS_HIP_TRY(hipStreamCreateWithFlags(&l.st, hipStreamNonBlocking));
        RL4RS_HIP_TRY(hipEventCreateWithFlags(&l.act_done, hipEventDisableTiming));
        RL4RS_HIP_TRY(hipEventCreateWithFlags(&l.done, hipEventDisableTiming));
        RL4RS_HIP_TRY(hipEventCreateWithFlags(&l.handed, hipEventDisableTiming));
        int rc;
        if ((rc = dev_alloc(&l.obs, B * 256)) || (rc = dev_alloc(&l.reward, B))) return rc;
    }
    s->lanes_made = true;
    return RL4RS_OK;
}

// everything after the act: observation, reward (when due), done, packed obs-side mask.  `on_obs` runs right after the
// observation forward has been enqueued (the record form sends the observation home from there on a reward step, beside the
// reward forward).
struct NoHook { int operator()() const { return RL4RS_OK; } };

// A reward step's observation row is the last complete-state row of its env (same prev_actions, its action the item just played):
// ONE forward of n_complete rows per env gives the probabilities of all rows and, through rl4rs_dien_set_obs_last, the observation -
// the observation-sized forward (bound by one workgroup's 64-step chain, the chip mostly idle) is not launched.  Taken when the
// scorer is the DIEN with k_augru_x, the n-row forward runs the 64-row form of k_augru_x (where a row costs about a quarter of what it
// costs in the chain-bound observation launch: the regime the fold was measured in; a small batch, whose n-row launch falls to 32-row
// workgroups, keeps the two-forward order) and the n-row launch needs no more rounds over the chip than the (n - 1)-row one.
// What the act of the transition about to start does for the partition: *rf filled and true = it refines (the partition the last
// act left, or the one the scorer's last content dedup found on exactly these rows: the reset observation forward).  False: the
// forwards of this transition look for duplicates themselves.
bool plan_refine(rl4rs_stepper* s, int cur, RowRefineArgs* rf) {
    s->part_now = false;
    env_rows_current(s->env, &s->dense, &s->cat);
    const int B = s->cfg.batch_size;
    const bool was_valid = s->part_valid;
    s->part_valid = false;
    if (!s->carry || !s->dien || !s->part_cnt || !dien_takes_partition(s->dien) || !env_refine_fits(s->env)) return false;
    // the first act of a page re-encodes the second sequence input into a slot per env: the slot table changes under the partition
    if (s->cfg.is_seq && cur > 0 && cur % s->cfg.page_items == 0) return false;
    const int32_t* order = dien_row_order(s->dien, B);
    memset(rf, 0, sizeof(*rf));
    if (was_valid && s->part_stamp == env_rows_stamp(s->env) && s->part_order == order) {
        rf->rep_prev = s->part_rep[s->part_cur];
    } else {
        DienPartition d;
        dien_last_partition(s->dien, &d);
        if (!(d.stamp > env_rows_stamp(s->env) && d.n_groups == B && d.group == 1 && d.dense == s->dense && d.cat == s->cat &&
              d.slots == s->slots && d.order == order)) return false;
        rf->rep_prev = d.rep;           // adopted where it lies: this act writes the stepper's own copy of everything
        rf->active_src = d.active;
        rf->n_active_src = d.n_active;
    }
    // the act rewrites the active list and the count in place (and, one act later, the rep array) the scorer's last forward ran
    // on: what that forward left to rl4rs_dien_buffer (PlanExpand::Lazy) can no longer be completed from them
    dien_drop_pending_expand(s->dien);
    rf->n = B;
    rf->rep = s->part_rep[s->part_cur ^ 1];
    rf->active = s->part_active;
    rf->cnt = s->part_cnt;
    rf->order = order;
    return true;
}
void refined(rl4rs_stepper* s) {
    s->part_cur ^= 1;
    s->part_order = dien_row_order(s->dien, s->cfg.batch_size);
    s->part_stamp = env_rows_stamp(s->env);
    s->part_valid = s->part_now = true;
}

bool fold_obs(const rl4rs_stepper* s) {
    const int n = s->n_complete, B = s->cfg.batch_size;
    if (!s->obs_fold || !s->dien || n < 2) return false;
    if (!rl4rs::dien_augru_rows64(s->dien, B, n)) return false;
    const int64_t with = rl4rs::dien_augru_rounds(s->dien, B, s->distinct_hint, n);
    const int64_t without = rl4rs::dien_augru_rounds(s->dien, B, s->distinct_hint, n - 1);
    return with > 0 && without > 0 && with <= without;
}

template <typename Hook = NoHook>
int after_act(rl4rs_stepper* s, int cur_before, float* obs, double* reward, uint8_t* done, uint32_t* mask_bits, void* stream,
              Hook on_obs = Hook(), bool tail_done = false, bool may_fold = false) {
    hipStream_t st = (hipStream_t)stream;
    rl4rs_env* e = s->env;
    const int B = s->cfg.batch_size;
    int rc;
    if (s->cfg.is_seq && cur_before > 0 && cur_before % s->cfg.page_items == 0) {
        // first act of a page: the second sequence input (items of the previous pages, seqslate.py:107-108) changed - on every page
        // but the first (prev_actions[:0] is the [0] the episode started with: nothing to re-encode)
        for (int q = 1; q < s->seq_num; ++q)
            if ((rc = scorer_encode(s, q, s->seq1, B, stream))) return rc;
    }
    if (may_fold && reward && rl4rs_env_is_reward_step(e) == 1 && fold_obs(s)) {
        const int n = s->n_complete;
        if ((rc = rl4rs_env_build_complete_rows(e, n, stream))) return rc;
        if ((rc = rl4rs_dien_set_obs_last(s->dien, obs))) return rc;
        if ((rc = scorer_forward(s, B * n, n, s->c_dense, s->c_cat, nullptr, s->probs, stream))) return rc;
        if ((rc = rl4rs_env_reward_split(e, s->probs, nullptr, reward, stream))) return rc;
        s->probs_rows = n;
        if (done && !tail_done) {
            hipLaunchKernelGGL(k_step_tail, dim3((B + 255) / 256), dim3(256), 0, st, done, (uint8_t)(cur_before >= s->cfg.max_steps - 1 ? 1 : 0),
                               (double*)nullptr, B);
            RL4RS_LAUNCH_CHECK();
        }
        if (mask_bits && (rc = rl4rs_env_obs_mask(e, mask_bits, 4, stream))) return rc;
        return RL4RS_OK;
    }
    if ((rc = scorer_forward(s, B, 1, s->dense, s->cat, obs, nullptr, stream))) return rc;
    if ((rc = on_obs())) return rc;
    double* zero_reward = nullptr;
    if (reward) {
        if (rl4rs_env_is_reward_step(e) == 1) {
            // the state row just scored IS the last complete-state row (slate.py:205-212 vs :119-130): score n - 1 rows per env
            const int m = s->n_complete - 1;
            if (m > 0) {
                if ((rc = rl4rs_env_build_complete_rows(e, m, stream))) return rc;
                if ((rc = scorer_forward(s, B * m, m, s->c_dense, s->c_cat, nullptr, s->probs, stream))) return rc;
            }
            if ((rc = scorer_head_prob(s, B, obs, s->p_last, stream))) return rc;
            if ((rc = rl4rs_env_reward_split(e, m > 0 ? s->probs : s->p_last, m > 0 ? s->p_last : nullptr, reward, stream))) return rc;
            s->probs_rows = m;
        } else {
            zero_reward = reward;
        }
    }
    if ((done || zero_reward) && !tail_done) {      // (tail_done: the act kernel wrote both, ActTail)
        hipLaunchKernelGGL(k_step_tail, dim3((B + 255) / 256), dim3(256), 0, st, done, (uint8_t)(cur_before >= s->cfg.max_steps - 1 ? 1 : 0),
                           zero_reward, B);
        RL4RS_LAUNCH_CHECK();
    }
    if (mask_bits && (rc = rl4rs_env_obs_mask(e, mask_bits, 4, stream))) return rc;
    return RL4RS_OK;
}

// ---- record form: everything a host-returning caller needs from one transition, packed for ONE device-to-host copy

// observation row of the d3rlpy mask mode (slate.py:270-277 / seqslate.py:18-23): float64 [obs (256) | masked_actions | cur_steps]
__global__ void k_record_d3rl(const float* obs, int obs_dim, const int32_t* prev, int T, int c0, int ncols, int cur, double* out, int B) {
    const int w = obs_dim + ncols + 1;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * w) return;
    const int b = (int)(i / w), c = (int)(i - (int64_t)b * w);
    double v;
    if (c < obs_dim) v = (double)obs[(size_t)b * obs_dim + c];
    else if (c < obs_dim + ncols) v = (double)prev[(size_t)b * T + c0 + (c - obs_dim)];
    else v = (double)cur;
    out[i] = v;
}
// click probabilities of an env's complete-state rows in slate order (simulator_info_fetch, slate.py:299-301)
__global__ void k_record_click(const float* probs, const float* p_last, int m, float* out, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * (m + 1)) return;
    const int b = i / (m + 1), j = i - b * (m + 1);
    out[i] = j < m ? probs[(size_t)b * m + j] : p_last[b];
}
// status words: [0] the env's sticky bad-action flag, [1] the scorer's fp16-range flag (read AND cleared, like rl4rs_dien_status)
__global__ void k_record_status(const int32_t* env_err, int32_t* range_flag, int32_t* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        out[0] = env_err ? *env_err : 0;
        out[1] = range_flag ? atomicExch(range_flag, 0) : 0;
    }
}

// A transition on lane lp.on (step_lanes.hpp decided that, and what it waits for): the act and the observation forward of
// rl4rs_env_step_discrete, the same launches with the same arguments but for the stream, the state-row set, the active list /
// counter pair, the scorer's scratch set and the head's output pointer.  lp.reward: the folded reward step of after_act,
// launch for launch - the act, the complete rows, the forward of n_complete rows per env on the scratch set of its lane (lane 0, set 0;
// lane 1, set 1 beside a replay-ahead forward) with the observation rows into the lane's buffer, the reward into the lane's
// reward block; its AUGRU launch waits for the other lane's `done`.
int lane_transition(rl4rs_stepper* s, const LanePlan& lp, const LaneState& before, int cur, RowRefineArgs* rf, const int32_t* actions_dev, float* obs_dev,
                    double* reward_dev, void* stream) {
    hipStream_t home = (hipStream_t)stream;
    StepLane& l = s->lane[lp.on];
    const int B = s->cfg.batch_size;
    if (lp.wait_entry) {
        RL4RS_HIP_TRY(hipEventRecord(s->ev_entry, home));
        RL4RS_HIP_TRY(hipStreamWaitEvent(l.st, s->ev_entry, 0));
    }
    if (lp.wait_act) RL4RS_HIP_TRY(hipStreamWaitEvent(l.st, s->lane[lp.on ^ 1].act_done, 0));
    if (lp.wait_handout) RL4RS_HIP_TRY(hipStreamWaitEvent(l.st, l.handed, 0));
    // the act writes the other row set and the other active list / counter pair: the previous forward (other lane) reads the current
    // ones, the forward before it (this lane, stream order) has finished with those the act now writes
    if (!rf->active_src) { rf->active_src = s->part_active; rf->n_active_src = s->part_cnt; }
    rf->active = s->part_active_alt;
    rf->cnt = s->part_cnt_alt;
    env_flip_rows(s->env);             // (the act kernel takes the env's current set: flipped in front of it, back if nothing was enqueued)
    ActTail tail;
    tail.done = nullptr; tail.done_v = 0;
    tail.zero_reward = (reward_dev && !lp.reward) ? l.reward : nullptr;
    tail.next_action = s->next_off + (size_t)(cur + 1) * B;      // (cur + 1 <= T: the ring has max_steps + 1 rows)
    tail.next_cur = cur + 1;
    int rc = rl4rs::env_act_discrete_tail(s->env, actions_dev, tail, l.st, rf);
    if (rc) {
        // nothing of the transition was enqueued: the row set, the partition pairs and the lane state stand as they were
        env_flip_rows(s->env);
        env_rows_current(s->env, &s->dense, &s->cat);
        lane_undo(s->lstate, before);
        return rc;
    }
    // the act is on the lane: from here on the pairs it wrote are the current ones
    std::swap(s->part_active, s->part_active_alt);
    std::swap(s->part_cnt, s->part_cnt_alt);
    env_rows_current(s->env, &s->dense, &s->cat);
    refined(s);
    s->next_off_cur = cur + 1;
    RL4RS_HIP_TRY(hipEventRecord(l.act_done, l.st));
    if (lp.reward) {
        const int n = s->n_complete;
        if ((rc = rl4rs::env_build_complete_rows_lane(s->env, n, l.st)) ||
            (rc = rl4rs_dien_set_obs_last(s->dien, l.obs)) ||
            (rc = rl4rs_dien_set_row_partition(s->dien, s->part_rep[s->part_cur], s->part_active, s->part_cnt, B)) ||
            (rc = dien_forward_lane_full(s->dien, lane_reward_set(lp.on), B * n, n, s->c_dense, s->c_cat, s->slots, nullptr, s->probs, l.st, stream,
                                         nullptr, s->lane[lp.on ^ 1].done)) ||      // (what is in flight beside it is the other lane's)
            (rc = rl4rs::env_reward_split_lane(s->env, s->probs, nullptr, l.reward, l.st))) {
            (void)hipEventRecord(l.done, l.st);
            return rc;
        }
        s->probs_rows = n;
    } else if ((rc = rl4rs_dien_set_row_partition(s->dien, s->part_rep[s->part_cur], s->part_active, s->part_cnt, B)) ||
        (rc = dien_forward_lane(s->dien, lp.on, B, s->dense, s->cat, s->slots, l.obs, l.st, stream))) {
        // the act happened, the observation did not: the lane still gets its `done` (the state says it is in flight, a join waits
        // for that event) and the caller the error; the env is where the act left it, as after a failed forward on the caller's stream
        (void)hipEventRecord(l.done, l.st);
        return rc;
    }
    RL4RS_HIP_TRY(hipEventRecord(l.done, l.st));
    // hand-out: the caller's blocks are written on the caller's stream only
    RL4RS_HIP_TRY(hipStreamWaitEvent(home, l.done, 0));
    const int64_t n_obs = (int64_t)B * 256;
    hipLaunchKernelGGL(k_lane_handout, dim3((unsigned)((n_obs + 255) / 256)), dim3(256), 0, home, l.obs, obs_dev, n_obs, l.reward, reward_dev, B);
    RL4RS_LAUNCH_CHECK();
    RL4RS_HIP_TRY(hipEventRecord(l.handed, home));
    return RL4RS_OK;
}

// ---- replay-ahead (step_lanes.hpp)
// the buffers of the group forward, made once by the first transition that may start one (9 rows per env: the larger group)
int ensure_ahead(rl4rs_stepper* s) {
    if (s->ah_obs) return RL4RS_OK;
    const size_t R = (size_t)s->cfg.batch_size * 9, B = (size_t)s->cfg.batch_size;
    float *cat = nullptr, *part = nullptr;
    int rc;
    if ((rc = dev_alloc(&s->ah_dense, R * (size_t)s->cfg.dense_feature_num)) || (rc = dev_alloc(&cat, R * (size_t)s->cfg.category_feature_num)) ||
        (rc = dev_alloc(&part, 2 * B + 4)) || (rc = dev_alloc(&s->ah_obs, R * 256))) {
        if (s->ah_dense) (void)hipFree(s->ah_dense);
        if (cat) (void)hipFree(cat);
        if (part) (void)hipFree(part);
        s->ah_dense = nullptr;
        return rc;
    }
    s->ah_cat = reinterpret_cast<int32_t*>(cat);
    s->ah_rep = reinterpret_cast<int32_t*>(part);
    s->ah_active = s->ah_rep + B;
    s->ah_cnt = s->ah_active + B;
    return RL4RS_OK;
}
// ... and, once, the scorer's second scratch set at the reward forward's size.  No memory for it: the reward step stays
// where it was, for good; replay-ahead and every transition go on as without it
void ensure_beside(rl4rs_stepper* s) {
    // (only where the reward step is ONE forward - fold_obs: where it is not it joins, and nothing would ever run on the larger set)
    if (!s->reward_beside || s->beside_tried || !s->lanes_made || !fold_obs(s)) return;
    s->beside_tried = true;
    if (dien_reserve_lane_scratch(s->dien, s->cfg.batch_size * s->n_complete) == RL4RS_OK) s->beside_ready = true;
    else (void)hipGetLastError();
}

int ahead_handout(rl4rs_stepper* s, int k, float* obs_dev, double* reward_dev, hipStream_t home) {
    const int B = s->cfg.batch_size;
    hipLaunchKernelGGL(k_ahead_handout, dim3((unsigned)(((int64_t)B * 64 + 255) / 256)), dim3(256), 0, home, s->ah_obs, s->ah_rep, s->ahead.n, k,
                       obs_dev, reward_dev, B);
    RL4RS_LAUNCH_CHECK();
    return RL4RS_OK;
}

// The transition that starts a group forward (ahead_decide said Start; `was`: the state in front of it): its act as a lane transition
// on lane 0 runs it (or, without lanes, on the caller's stream, which has joined), the rows of the act indices cur .. T - 2 with a
// copy of the partition the act left, ONE forward of n rows per env on the scorer's first scratch set - its head output into ah_obs -
// and the hand-out of row 0 on the caller's stream.
int ahead_start(rl4rs_stepper* s, const AheadState& was, int cur, RowRefineArgs* rf, const int32_t* actions_dev, float* obs_dev, double* reward_dev,
                void* stream) {
    hipStream_t home = (hipStream_t)stream;
    const int B = s->cfg.batch_size, n = s->ahead.n;
    const bool lanes = s->ahead.lanes;
    const LaneState before = s->lstate;
    hipStream_t st = home;
    hipEvent_t before_augru = nullptr;
    if (lanes) {
        const LanePlan lp = lane_ahead_start(s->lstate);
        StepLane& l = s->lane[0];
        st = l.st;
        // (a wait that cannot be enqueued: nothing of the transition has been, the state in front of it stands again)
        hipError_t he = hipSuccess;
        if (lp.wait_entry && (he = hipEventRecord(s->ev_entry, home)) == hipSuccess) he = hipStreamWaitEvent(st, s->ev_entry, 0);
        if (he == hipSuccess && lp.wait_act) he = hipStreamWaitEvent(st, s->lane[1].act_done, 0);
        if (he != hipSuccess) {
            lane_undo(s->lstate, before);
            s->ahead = was;
            set_error("env_step_discrete: %s", hipGetErrorString(he));
            return RL4RS_EHIP;
        }
        if (lp.wait_act) before_augru = s->lane[1].done;      // the forward in flight on lane 1 leaves the chip first
        // as every lane transition: the act writes the other row set and the other active list / counter pair
        if (!rf->active_src) { rf->active_src = s->part_active; rf->n_active_src = s->part_cnt; }
        rf->active = s->part_active_alt;
        rf->cnt = s->part_cnt_alt;
        env_flip_rows(s->env);
    } else {
        const AheadState now = s->ahead;
        const int rcj = lanes_wait(s, stream, 1);      // (a join drops the rows of a forward in flight: not those of the one about to start)
        s->ahead = now;
        if (rcj) { s->ahead = was; return rcj; }
    }
    ActTail tail;
    tail.done = nullptr; tail.done_v = 0;
    tail.zero_reward = nullptr;                  // (the hand-out writes the caller's block on the caller's stream)
    tail.next_action = s->next_off + (size_t)(cur + 1) * B;
    tail.next_cur = cur + 1;
    int rc = rl4rs::env_act_discrete_tail(s->env, actions_dev, tail, st, rf);
    if (rc) {      // nothing was enqueued
        if (lanes) { env_flip_rows(s->env); lane_undo(s->lstate, before); }
        env_rows_current(s->env, &s->dense, &s->cat);
        s->ahead = was;
        return rc;
    }
    if (lanes) {
        std::swap(s->part_active, s->part_active_alt);
        std::swap(s->part_cnt, s->part_cnt_alt);
    }
    env_rows_current(s->env, &s->dense, &s->cat);
    refined(s);
    s->next_off_cur = cur + 1;
    AheadPart part = {s->part_rep[s->part_cur], s->part_active, s->part_cnt, s->ah_rep, s->ah_active, s->ah_cnt};
    rc = rl4rs::env_build_ahead_rows_lane(s->env, cur, n, s->ah_dense, s->ah_cat, &part, st);
    // (lane 1's later acts rewrite the partition the builder read: `act_done` stands behind the builder)
    if (lanes && hipEventRecord(s->lane[0].act_done, st) != hipSuccess && !rc) {
        set_error("env_step_discrete: hipEventRecord failed");
        rc = RL4RS_EHIP;
    }
    if (!rc) {
        rl4rs::dien_set_group_rows(s->dien, s->ah_obs);
        rc = rl4rs_dien_set_row_partition(s->dien, s->ah_rep, s->ah_active, s->ah_cnt, B);
    }
    if (!rc) rc = dien_forward_lane_full(s->dien, 0, B * n, n, s->ah_dense, s->ah_cat, s->slots, nullptr, nullptr, st, stream, nullptr, before_augru);
    if (lanes) (void)hipEventRecord(s->lane[0].done, st);
    if (!rc && lanes && hipStreamWaitEvent(home, s->lane[0].done, 0) != hipSuccess) {
        set_error("env_step_discrete: hipStreamWaitEvent failed");
        rc = RL4RS_EHIP;
    }
    if (rc) {      // the act happened, the forward did not: no row to hand out, the env is where the act left it
        s->ahead.active = false;
        s->ahead.handed -= 1;
        s->ahead.started -= 1;
        return rc;
    }
    return ahead_handout(s, 0, obs_dev, reward_dev, home);
}

// A later transition of the replay (ahead_decide said Next): its act alone - on lane 1 behind the row builder, or on the caller's
// stream - and row cur - c0 of the forward's output, handed out on the caller's stream behind the forward.
int ahead_next(rl4rs_stepper* s, const AheadState& was, int cur, RowRefineArgs* rf, const int32_t* actions_dev, float* obs_dev, double* reward_dev,
               void* stream) {
    hipStream_t home = (hipStream_t)stream;
    const int B = s->cfg.batch_size;
    const bool lanes = s->ahead.lanes;
    const LaneState before = s->lstate;
    hipStream_t st = home;
    if (lanes) {
        (void)lane_ahead_next(s->lstate);
        st = s->lane[1].st;
        RL4RS_HIP_TRY(hipStreamWaitEvent(st, s->lane[0].act_done, 0));
    }
    ActTail tail;
    tail.done = nullptr; tail.done_v = 0;
    tail.zero_reward = nullptr;
    tail.next_action = s->next_off + (size_t)(cur + 1) * B;      // (cur + 1 <= T - 1)
    tail.next_cur = cur + 1;
    const int rc = rl4rs::env_act_discrete_tail(s->env, actions_dev, tail, st, rf);
    if (rc) {
        if (lanes) lane_undo(s->lstate, before);
        s->ahead = was;
        return rc;
    }
    if (rf) refined(s);
    s->next_off_cur = cur + 1;
    if (lanes) {
        RL4RS_HIP_TRY(hipEventRecord(s->lane[1].act_done, st));
        RL4RS_HIP_TRY(hipEventRecord(s->lane[1].done, st));
        // the caller's stream: behind the forward (the row) and behind the act (the logged-action row the caller reads next)
        RL4RS_HIP_TRY(hipStreamWaitEvent(home, s->lane[0].done, 0));
        RL4RS_HIP_TRY(hipStreamWaitEvent(home, s->lane[1].done, 0));
    }
    return ahead_handout(s, cur - s->ahead.c0, obs_dev, reward_dev, home);
}

// the step counter in front of the act behind which the next reward is due (the rule of rl4rs_env_is_reward_step at cur + 1)
int reward_act(const rl4rs_stepper* s, int cur) {
    const int T = s->cfg.max_steps;
    if (!s->cfg.is_seq) return T - 1;
    const int d = cur / s->cfg.page_items * s->cfg.page_items + s->cfg.page_items - 1;
    return d < T - 1 ? d : T - 1;
}

int attach(rl4rs_env* env, rl4rs_dien* dien, rl4rs_simnet* simnet, const int32_t* slots_dev, int32_t seq_num, rl4rs_stepper** out) {
    RL4RS_REQUIRE(env && (dien || simnet) && slots_dev && out && seq_num >= 1 && seq_num <= 4, "env_attach_scorer: bad argument");
    rl4rs_stepper* s = new rl4rs_stepper();
    memset(s, 0, sizeof(*s));
    s->env = env; s->dien = dien; s->simnet = simnet; s->slots = slots_dev; s->seq_num = seq_num;
    int rc = rl4rs_env_get_cfg(env, &s->cfg);
    if (rc) { delete s; return rc; }
    s->n_complete = rl4rs_env_complete_rows(env);
    const size_t B = (size_t)s->cfg.batch_size;
    float* ring = nullptr;
    if ((rc = dev_alloc(&s->probs, B * (size_t)s->n_complete)) || (rc = dev_alloc(&s->p_last, B)) ||
        (rc = dev_alloc(&ring, B * (size_t)(s->cfg.max_steps + 1)))) {
        if (s->probs) (void)hipFree(s->probs);
        if (s->p_last) (void)hipFree(s->p_last);
        delete s;
        return rc;
    }
    s->next_off = reinterpret_cast<int32_t*>(ring);
    s->next_off_cur = -1;
    if (dien) {
        float* part = nullptr;          // rep x 2, active x 2, counters x 2
        if ((rc = dev_alloc(&part, 4 * B + 8))) { rl4rs_stepper_destroy(s); return rc; }
        s->part_rep[0] = reinterpret_cast<int32_t*>(part);
        s->part_rep[1] = s->part_rep[0] + B;
        s->part_active = s->part_rep[1] + B;
        s->part_active_alt = s->part_active + B;
        s->part_cnt = s->part_active_alt + B;
        s->part_cnt_alt = s->part_cnt + 4;
        if (hipMemset(s->part_cnt, 0, 32) != hipSuccess) { rl4rs_stepper_destroy(s); set_error("env_attach_scorer: hipMemset failed"); return RL4RS_EHIP; }
        s->carry = true;
    }
    // the lanes: a stepper attached earlier to this env or scorer may still have a transition in flight (the host waits, once)
    s->hook.ctx = s;
    s->hook.join = hook_join;
    s->hook.gone = hook_gone;
    lane_links_attach(s->links, LANE_LINK_ENV, env_lane_slot(env), &s->hook);
    if (dien) {
        lane_links_attach(s->links, LANE_LINK_SCORER, dien_lane_slot(dien), &s->hook);
        if (dien_takes_partition(dien) && ((rc = make_lanes(s)) || (rc = dien_reserve_lane_scratch(dien, s->cfg.batch_size)))) {
            rl4rs_stepper_destroy(s);
            return rc;
        }
        s->overlap = s->reset_lane = s->reward_lane = s->reward_beside = s->lanes_made;
    }
    s->act_tail = true;
    s->replay_ahead = dien != nullptr ? 1 : 0;
    s->obs_fold = true;
    s->distinct_hint = s->cfg.batch_size;
    void* p;
    int64_t nb;
#define BUF(which, field, type) if ((rc = rl4rs_env_buffer(env, which, &p, &nb))) { rl4rs_stepper_destroy(s); return rc; } s->field = reinterpret_cast<type>(p)
    BUF(RL4RS_BUF_DENSE, dense, const float*);
    BUF(RL4RS_BUF_CATEGORY, cat, const int32_t*);
    BUF(RL4RS_BUF_SEQ1, seq1, const int32_t*);
    BUF(RL4RS_BUF_C_DENSE, c_dense, const float*);
    BUF(RL4RS_BUF_C_CATEGORY, c_cat, const int32_t*);
#undef BUF
    *out = s;
    return RL4RS_OK;
}

}  // namespace

extern "C" {

int rl4rs_env_attach_scorer(rl4rs_env* env, rl4rs_dien* net, const int32_t* slots_dev, int32_t seq_num, rl4rs_stepper** out) {
    return attach(env, net, nullptr, slots_dev, seq_num, out);
}
int rl4rs_env_attach_simnet(rl4rs_env* env, rl4rs_simnet* net, const int32_t* slots_dev, int32_t seq_num, rl4rs_stepper** out) {
    return attach(env, nullptr, net, slots_dev, seq_num, out);
}

int rl4rs_stepper_destroy(rl4rs_stepper* s) {
    if (!s) return RL4RS_OK;
    (void)lanes_wait(s, nullptr, 0);
    lane_links_release(s->links, &s->hook);      // (neither handle is touched if it went first: hook_gone has been told)
    if (s->lanes_made || s->ev_entry) {
        if (s->ev_entry) (void)hipEventDestroy(s->ev_entry);
        for (int i = 0; i < 2; ++i) {
            StepLane& l = s->lane[i];
            if (l.st) { (void)hipStreamSynchronize(l.st); (void)hipStreamDestroy(l.st); }
            if (l.act_done) (void)hipEventDestroy(l.act_done);
            if (l.done) (void)hipEventDestroy(l.done);
            if (l.handed) (void)hipEventDestroy(l.handed);
            if (l.obs) (void)hipFree(l.obs);
            if (l.reward) (void)hipFree(l.reward);
        }
    }
    if (s->probs) (void)hipFree(s->probs);
    if (s->p_last) (void)hipFree(s->p_last);
    if (s->ah_dense) (void)hipFree(s->ah_dense);
    if (s->ah_cat) (void)hipFree(s->ah_cat);
    if (s->ah_obs) (void)hipFree(s->ah_obs);
    if (s->ah_rep) (void)hipFree(s->ah_rep);
    if (s->next_off) (void)hipFree(s->next_off);
    if (s->part_rep[0]) (void)hipFree(s->part_rep[0]);
    if (s->ev_ready) (void)hipEventDestroy(s->ev_ready);
    if (s->ev_copied) (void)hipEventDestroy(s->ev_copied);
    if (s->copy_stream) (void)hipStreamDestroy(s->copy_stream);
    delete s;
    return RL4RS_OK;
}

int rl4rs_env_step_discrete(rl4rs_stepper* s, const int32_t* actions_dev, float* obs_dev, double* reward_dev, uint8_t* done_dev,
                            uint32_t* mask_bits_dev, void* stream) {
    RL4RS_REQUIRE(s && actions_dev && obs_dev, "env_step_discrete: null argument");
    const int cur = rl4rs_env_cur_steps(s->env);
    // the caller hands back the logged-action row the previous transition's act wrote: nothing of its own stream is needed
    const bool own_row = s->next_off_cur == cur && cur >= 0 && actions_dev == s->next_off + (size_t)cur * s->cfg.batch_size;
    s->next_off_cur = -1;
    RowRefineArgs rf;
    const bool refine = plan_refine(s, cur, &rf);
    {
        const int T = s->cfg.max_steps;
        LaneCall c;
        memset(&c, 0, sizeof(c));
        c.overlap = s->overlap && s->act_tail && cur < T && lane_links_mine(s->links, LANE_LINK_ENV, &s->hook) &&
                    lane_links_mine(s->links, LANE_LINK_SCORER, &s->hook);
        c.dien_x = s->dien && dien_lane_path(s->dien, s->cfg.batch_size);
        c.carried = refine;
        c.reward_due = s->cfg.is_seq ? (cur + 1) % s->cfg.page_items == 0 : cur + 1 >= T;
        c.extra_outputs = mask_bits_dev != nullptr || done_dev != nullptr;
        c.own_row = own_row;
        c.seq_num = s->seq_num; c.distinct_hint = s->distinct_hint; c.n_cu = s->dien ? dien_n_cu(s->dien) : 0;
        // (with both halves of DESIGN 39 off the lanes alternate from where they were)
        c.to_reward = (c.reward_due || !(s->reset_lane || s->reward_lane)) ? 0 : reward_act(s, cur) - cur;
        c.no_reward_lane = !s->reward_lane;
        c.reward_fold = c.reward_due && reward_dev && c.overlap && c.dien_x && refine && fold_obs(s);
        {
            // replay-ahead: the start of a group forward, the hand-out of its next row, or a transition like any other
            AheadCall a;
            memset(&a, 0, sizeof(a));
            a.on = s->replay_ahead != 0 && s->act_tail;
            a.own_row = own_row;
            a.slate = !s->cfg.is_seq && !done_dev && !mask_bits_dev && (reinterpret_cast<uintptr_t>(obs_dev) & 15) == 0;
            a.dien_x = s->dien != nullptr;
            a.carried = refine;
            a.cur = cur; a.T = T;
            if (a.on && a.dien_x && (s->ahead.active || ahead_rows(cur, T) == 8 || ahead_rows(cur, T) == 9)) {
                // (1: only where the group forward fills the chip twice over, the regime the gain was reasoned and measured in - a
                // forward of a few workgroups is no faster than the launches it replaces and its first row arrives later)
                for (int i = 0; i < 2; ++i)
                    a.rows64[i] = s->replay_ahead == 2 ? rl4rs::dien_augru_rows64(s->dien, s->cfg.batch_size, 8 + i)
                                                       : rl4rs::dien_augru_rows64_auto(s->dien, s->cfg.batch_size, 8 + i);
            }
            a.lanes = lane_room(c);
            // (no memory for the forward's buffers: this stepper goes on without replay-ahead, every transition as it was)
            if (!s->ahead.active && ahead_trigger(a)) {
                if (ensure_ahead(s) != RL4RS_OK) {
                    (void)hipGetLastError();
                    s->replay_ahead = 0;
                    a.on = false;
                } else if (a.lanes) {
                    ensure_beside(s);
                }
            }
            const AheadState was = s->ahead;
            bool dropped = false;
            const AheadStep step = ahead_decide(s->ahead, a, &dropped);
            if (dropped) { const int rcj = lanes_wait(s, stream, 1); if (rcj) return rcj; }
            if (step == AheadStep::Start) return ahead_start(s, was, cur, &rf, actions_dev, obs_dev, reward_dev, stream);
            if (step == AheadStep::Next) return ahead_next(s, was, cur, refine ? &rf : nullptr, actions_dev, obs_dev, reward_dev, stream);
        }
        const LaneState before = s->lstate;
        // (a folded reward step behind a group forward takes lane 1 and the scorer's second set; else lane_decide alone)
        const LanePlan lp = lane_decide_beside(s->lstate, c, s->reward_beside && s->beside_ready && dien_lane_path(s->dien, s->cfg.batch_size * s->n_complete));
        if (lp.lane) return lane_transition(s, lp, before, cur, &rf, actions_dev, obs_dev, reward_dev, stream);
        // (lane_decide has joined the state; the waits go to the caller's stream)
        if (lp.join) {
            for (int i = 0; i < 2; ++i) RL4RS_HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, s->lane[i].done, 0));
        }
    }
    if (!s->act_tail) {
        int rc = rl4rs::env_act_discrete_tail(s->env, actions_dev, ActTail(), stream, refine ? &rf : nullptr);
        if (rc) return rc;
        if (refine) refined(s);
        return after_act(s, cur, obs_dev, reward_dev, done_dev, mask_bits_dev, stream, NoHook(), false, true);
    }
    // is a reward due after this act?  (rl4rs_env_is_reward_step at cur + 1; checked against it below)
    const int T = s->cfg.max_steps;
    const int due = s->cfg.is_seq ? ((cur + 1) % s->cfg.page_items == 0 ? 1 : 0) : (cur + 1 >= T ? 1 : 0);
    ActTail tail;
    tail.done = done_dev; tail.done_v = (uint8_t)(cur >= T - 1 ? 1 : 0);
    tail.zero_reward = (reward_dev && !due) ? reward_dev : nullptr;
    tail.next_action = (cur + 1 <= T) ? s->next_off + (size_t)(cur + 1) * s->cfg.batch_size : nullptr;
    tail.next_cur = cur + 1;
    int rc = rl4rs::env_act_discrete_tail(s->env, actions_dev, tail, stream, refine ? &rf : nullptr);
    if (rc) return rc;
    if (refine) refined(s);
    if (tail.next_action) s->next_off_cur = cur + 1;
    // (a different answer from the env itself: k_step_tail runs as before and has the last word)
    const bool covered = rl4rs_env_is_reward_step(s->env) == due;
    return after_act(s, cur, obs_dev, reward_dev, done_dev, mask_bits_dev, stream, NoHook(), covered, true);
}

int rl4rs_stepper_set_act_tail(rl4rs_stepper* s, int32_t on) {
    RL4RS_REQUIRE(s, "stepper_set_act_tail: null argument");
    s->act_tail = on != 0;
    s->next_off_cur = -1;
    return RL4RS_OK;
}

int rl4rs_stepper_set_obs_fold(rl4rs_stepper* s, int32_t on) {
    RL4RS_REQUIRE(s, "stepper_set_obs_fold: null argument");
    s->obs_fold = on != 0;
    return RL4RS_OK;
}

int rl4rs_stepper_set_partition_carry(rl4rs_stepper* s, int32_t on) {
    RL4RS_REQUIRE(s, "stepper_set_partition_carry: null argument");
    s->carry = on != 0 && s->part_cnt != nullptr;
    s->part_valid = s->part_now = false;
    return RL4RS_OK;
}

int rl4rs_stepper_set_step_overlap(rl4rs_stepper* s, int32_t on) {
    RL4RS_REQUIRE(s, "stepper_set_step_overlap: null argument");
    s->overlap = on != 0 && s->lanes_made;
    return RL4RS_OK;
}

int rl4rs_stepper_set_reset_lane(rl4rs_stepper* s, int32_t on) {
    RL4RS_REQUIRE(s, "stepper_set_reset_lane: null argument");
    s->reset_lane = on != 0 && s->lanes_made;
    return RL4RS_OK;
}

int rl4rs_stepper_set_reward_lane(rl4rs_stepper* s, int32_t on) {
    RL4RS_REQUIRE(s, "stepper_set_reward_lane: null argument");
    s->reward_lane = on != 0 && s->lanes_made;
    return RL4RS_OK;
}

// off - a folded reward step behind a replay-ahead forward runs on lane 0 and the first scratch set, behind that forward,
// as it did; the second set is then not grown (one that has been grown stays: a forward may be reading it)
int rl4rs_stepper_set_reward_beside(rl4rs_stepper* s, int32_t on) {
    RL4RS_REQUIRE(s, "stepper_set_reward_beside: null argument");
    s->reward_beside = on != 0 && s->lanes_made;
    return RL4RS_OK;
}

int rl4rs_stepper_reward_beside_stats(const rl4rs_stepper* s, int64_t* ran, int64_t* scratch_bytes) {
    RL4RS_REQUIRE(s, "stepper_reward_beside_stats: null argument");
    if (ran) *ran = s->lstate.ran_beside;
    if (scratch_bytes) *scratch_bytes = s->dien ? dien_lane_scratch_bytes(s->dien) : 0;
    return RL4RS_OK;
}

// Replay-ahead: 0 off - every transition issues the launches it issued without it; 1 (default) where a forward of 8 / 9
// rows per env takes the 64-row form of k_augru_x by the automatic rule; 2 also where that form is pinned (small batches: tests).
// A forward in flight keeps the rows it has (they are dropped like any others when the next transition finds the switch off).
int rl4rs_stepper_set_replay_ahead(rl4rs_stepper* s, int32_t on) {
    RL4RS_REQUIRE(s && on >= 0 && on <= 2, "stepper_set_replay_ahead: bad argument");
    s->replay_ahead = s->dien != nullptr ? on : 0;
    return RL4RS_OK;
}

int rl4rs_stepper_replay_stats(const rl4rs_stepper* s, int64_t* started, int64_t* handed, int64_t* dropped) {
    RL4RS_REQUIRE(s, "stepper_replay_stats: null argument");
    if (started) *started = s->ahead.started;
    if (handed) *handed = s->ahead.handed;
    if (dropped) *dropped = s->ahead.dropped;
    return RL4RS_OK;
}

int rl4rs_stepper_lane_stats_ex(const rl4rs_stepper* s, int64_t* reset_runs, int64_t* reward_runs) {
    RL4RS_REQUIRE(s, "stepper_lane_stats_ex: null argument");
    if (reset_runs) *reset_runs = s->lstate.ran_reset;
    if (reward_runs) *reward_runs = s->lstate.ran_reward;
    return RL4RS_OK;
}

// The observation of the state the env is in behind a reset, as a lane transition without an act: *taken = 1 and obs_dev
// is filled on the caller's stream (the hand-out of every lane transition); the logged action of step 0 is row 0 of the stepper's
// ring (rl4rs_stepper_next_offline_action), so that the first transition hands back the stepper's own row and waits for the
// partition only.  *taken = 0: the rule of step_lanes.hpp says no, nothing was enqueued or changed - the caller composes the
// observation as it did (rl4rs_dien_forward on its own stream).
int rl4rs_stepper_observe(rl4rs_stepper* s, float* obs_dev, int32_t* taken, void* stream) {
    RL4RS_REQUIRE(s && obs_dev && taken, "stepper_observe: null argument");
    *taken = 0;
    const int cur = rl4rs_env_cur_steps(s->env);
    const int B = s->cfg.batch_size;
    LaneCall c;
    memset(&c, 0, sizeof(c));
    c.overlap = s->overlap && s->act_tail && cur == 0 && lane_links_mine(s->links, LANE_LINK_ENV, &s->hook) &&
                lane_links_mine(s->links, LANE_LINK_SCORER, &s->hook);
    c.dien_x = s->dien && dien_lane_path(s->dien, B);
    c.seq_num = s->seq_num; c.distinct_hint = s->distinct_hint; c.n_cu = s->dien ? dien_n_cu(s->dien) : 0;
    c.observe = true;
    c.no_reset_lane = !s->reset_lane;
    c.to_reward = 1 + reward_act(s, cur) - cur;
    if (!lane_observe_eligible(c)) return RL4RS_OK;
    hipStream_t home = (hipStream_t)stream;
    int rc = lanes_wait(s, stream, 1);                  // (behind a reset nothing is in flight: the load has joined)
    if (rc) return rc;
    s->next_off_cur = -1;
    if ((rc = rl4rs_env_offline_action(s->env, s->next_off, nullptr, stream))) return rc;
    const LanePlan lp = lane_decide(s->lstate, c);
    StepLane& l = s->lane[lp.on];
    s->part_now = false;                                // the rows of a state nobody acted on: this forward compares them (and seeds the next act)
    env_rows_current(s->env, &s->dense, &s->cat);
    RL4RS_HIP_TRY(hipEventRecord(s->ev_entry, home));
    RL4RS_HIP_TRY(hipStreamWaitEvent(l.st, s->ev_entry, 0));
    if ((rc = dien_forward_lane_full(s->dien, lp.on, B, 1, s->dense, s->cat, s->slots, l.obs, nullptr, l.st, stream, l.act_done, nullptr))) {
        // the state says the lane is in flight: a join waits for `done`, a transition behind this one for `act_done`
        (void)hipEventRecord(l.act_done, l.st);
        (void)hipEventRecord(l.done, l.st);
        return rc;
    }
    RL4RS_HIP_TRY(hipEventRecord(l.done, l.st));
    RL4RS_HIP_TRY(hipStreamWaitEvent(home, l.done, 0));
    const int64_t n_obs = (int64_t)B * 256;
    hipLaunchKernelGGL(k_lane_handout, dim3((unsigned)((n_obs + 255) / 256)), dim3(256), 0, home, l.obs, obs_dev, n_obs, l.reward, (double*)nullptr, B);
    RL4RS_LAUNCH_CHECK();
    RL4RS_HIP_TRY(hipEventRecord(l.handed, home));
    s->next_off_cur = 0;
    *taken = 1;
    return RL4RS_OK;
}

int rl4rs_stepper_lane_stats(const rl4rs_stepper* s, int64_t* lane0, int64_t* lane1, int64_t* joins) {
    RL4RS_REQUIRE(s, "stepper_lane_stats: null argument");
    if (lane0) *lane0 = s->lstate.ran[0];
    if (lane1) *lane1 = s->lstate.ran[1];
    if (joins) *joins = s->lstate.joins;
    return RL4RS_OK;
}

int rl4rs_stepper_reward_rows(const rl4rs_stepper* s) { return s ? s->probs_rows : RL4RS_EINVAL; }

int rl4rs_stepper_click_probs(rl4rs_stepper* s, float* out_dev, void* stream) {
    RL4RS_REQUIRE(s && out_dev, "stepper_click_probs: null argument");
    { const int rcj = lanes_wait(s, stream, 1); if (rcj) return rcj; }
    RL4RS_REQUIRE(s->n_complete >= 2 && s->probs_rows > 0, "stepper_click_probs: no reward step yet");
    const int B = s->cfg.batch_size, n = s->n_complete;
    hipStream_t st = (hipStream_t)stream;
    if (s->probs_rows == n) {
        RL4RS_HIP_TRY(hipMemcpyAsync(out_dev, s->probs, (size_t)B * n * 4, hipMemcpyDeviceToDevice, st));
    } else {
        hipLaunchKernelGGL(k_record_click, dim3((B * n + 255) / 256), dim3(256), 0, st, s->probs, s->p_last, n - 1, out_dev, B);
        RL4RS_LAUNCH_CHECK();
    }
    return RL4RS_OK;
}

int rl4rs_stepper_set_distinct_hint(rl4rs_stepper* s, int32_t n_distinct) {
    RL4RS_REQUIRE(s && n_distinct >= 1, "stepper_set_distinct_hint: bad argument");
    s->distinct_hint = n_distinct < s->cfg.batch_size ? n_distinct : s->cfg.batch_size;
    if (s->dien) return rl4rs_dien_set_distinct_hint(s->dien, s->distinct_hint);     // sizes the scorer's shadow-plane order
    return RL4RS_OK;
}

int rl4rs_stepper_next_offline_action(rl4rs_stepper* s, const int32_t** ids_dev, int32_t* step) {
    RL4RS_REQUIRE(s && ids_dev && step, "stepper_next_offline_action: null argument");
    *step = s->next_off_cur;
    *ids_dev = s->next_off_cur >= 0 ? s->next_off + (size_t)s->next_off_cur * s->cfg.batch_size : nullptr;
    return RL4RS_OK;
}

int rl4rs_env_step_conti(rl4rs_stepper* s, const void* actions_dev, int is_f64, int32_t* chosen_dev, float* obs_dev,
                         double* reward_dev, uint8_t* done_dev, uint32_t* mask_bits_dev, void* stream) {
    RL4RS_REQUIRE(s && actions_dev && obs_dev, "env_step_conti: null argument");
    { const int rcj = lanes_wait(s, stream, 1); if (rcj) return rcj; }
    const int cur = rl4rs_env_cur_steps(s->env);
    s->next_off_cur = -1;
    RowRefineArgs rf;
    const bool refine = plan_refine(s, cur, &rf);
    int rc = rl4rs::env_act_conti_refine(s->env, actions_dev, is_f64, chosen_dev, stream, refine ? &rf : nullptr);
    if (rc) return rc;
    if (refine) refined(s);
    return after_act(s, cur, obs_dev, reward_dev, done_dev, mask_bits_dev, stream, NoHook(), false, true);
}

// ---- reference-shaped (host-returning) transition ---------------------------------------------------------------------
// The same transition as rl4rs_env_step_discrete / _conti with every output written into ONE device record (byte offsets from
// rl4rs_stepper_record_layout), host-visible part first: the caller brings the whole transition back with a single copy into
// pinned memory and one wait, instead of one blocking copy per returned object (obs, reward, mask, flags ...).
int rl4rs_stepper_record_layout(rl4rs_stepper* s, uint32_t want, int32_t conti, rl4rs_step_record* L) {
    RL4RS_REQUIRE(s && L, "stepper_record_layout: null argument");
    RL4RS_REQUIRE((want & ~(uint32_t)RL4RS_STEP_WANT_ALL) == 0, "stepper_record_layout: unknown want bits 0x%x", want);
    RL4RS_REQUIRE(!((want & RL4RS_STEP_WANT_CLICK_P) && s->n_complete < 2), "stepper_record_layout: click_p needs n_complete >= 2");
    const int64_t B = s->cfg.batch_size, A = s->cfg.action_size, W = (A + 31) / 32;
    int32_t od32 = 256;
    if (!s->dien) { int rc0 = rl4rs_simnet_obs_dim(s->simnet, &od32); if (rc0) return rc0; }
    const int64_t OD = od32;
    const int ncols = s->cfg.is_seq ? s->cfg.page_items : s->cfg.max_steps;
    int64_t off = 0;
    auto take = [&](int64_t bytes) { const int64_t o = off; off = (off + bytes + 63) & ~(int64_t)63; return o; };
    memset(L, 0xff, sizeof(*L));                                   // every offset -1 = absent
    L->status = take(8);
    L->reward = take(B * 8);
    L->done = take(B);
    L->chosen = take(B * 4);
    const bool d3rl = (want & RL4RS_STEP_WANT_D3RL_OBS) != 0;
    if (d3rl) L->obs_d3rl = take(B * (OD + ncols + 1) * 8); else L->obs = take(B * OD * 4);
    if (want & RL4RS_STEP_WANT_MASK_BITS) L->mask_bits = take(B * W * 4);
    if (want & RL4RS_STEP_WANT_CLICK_P) L->click_p = take(B * s->n_complete * 4);
    if (want & RL4RS_STEP_WANT_OFFLINE_ACTION) L->offline_action = take(conti ? B * s->cfg.action_emb_size * 8 : B * 4);
    // the int64 mask is by far the largest part (B * A * 8 bytes) and depends on the act alone: last of the host part, so that
    // rl4rs_env_step_record_host can send it home on its own while the scorer runs and bring the rest back as one prefix
    if (want & RL4RS_STEP_WANT_MASK_I64) L->mask_i64 = take(B * A * 8);
    L->host_bytes = off;
    if (d3rl) L->obs = take(B * OD * 4);                           // float32 activations: device-side scratch only in this mode
    L->total_bytes = off;
    L->obs_dim = (int32_t)OD;
    L->d3rl_cols = (int32_t)(OD + ncols + 1);
    return RL4RS_OK;
}

// `observe`: no transition - the record of the state the env is in (after a reset: what RecSimBase.sample returns, base.py:172-175);
// reward / done / chosen are then left alone and `actions_dev` is unused.
static int step_record(rl4rs_stepper* s, bool observe, const void* actions_dev, int32_t action_kind, uint32_t want, void* record_dev,
                       void* record_host, void* stream) {
    RL4RS_REQUIRE(s && (observe || actions_dev) && record_dev, "env_step_record: null argument");
    RL4RS_REQUIRE(action_kind >= 0 && action_kind <= 2, "env_step_record: action_kind must be 0 (int32 ids), 1 (float32) or 2 (float64 embeddings)");
    RL4RS_REQUIRE(!(observe && (want & RL4RS_STEP_WANT_CLICK_P)), "env_observe_record: click_p belongs to a reward step");
    rl4rs_step_record L;
    int rc = rl4rs_stepper_record_layout(s, want, action_kind != 0, &L);
    if (rc) return rc;
    if ((rc = lanes_wait(s, stream, 1))) return rc;
    env_rows_current(s->env, &s->dense, &s->cat);
    hipStream_t st = (hipStream_t)stream;
    char* R = reinterpret_cast<char*>(record_dev);
    const int B = s->cfg.batch_size;
    float* obs = reinterpret_cast<float*>(R + L.obs);
    int32_t* chosen = reinterpret_cast<int32_t*>(R + L.chosen);
    const int cur = rl4rs_env_cur_steps(s->env) - (observe ? 1 : 0);      // `cur + 1` below = the step counter the record describes
    RowRefineArgs rf;
    bool refine = false;
    if (observe) {
        s->part_now = false;            // the rows of a state nobody acted on: this forward compares them (and seeds the next act)
        rc = RL4RS_OK;
    } else if (action_kind == 0) {
        RL4RS_HIP_TRY(hipMemcpyAsync(chosen, actions_dev, (size_t)B * 4, hipMemcpyDeviceToDevice, st));
        s->next_off_cur = -1;
        refine = plan_refine(s, cur, &rf);
        rc = rl4rs::env_act_discrete_tail(s->env, reinterpret_cast<const int32_t*>(actions_dev), ActTail(), stream, refine ? &rf : nullptr);
    } else {
        refine = plan_refine(s, cur, &rf);
        rc = rl4rs::env_act_conti_refine(s->env, actions_dev, action_kind == 2 ? 1 : 0, chosen, stream, refine ? &rf : nullptr);
    }
    if (rc) return rc;
    if (refine) refined(s);
    const int reward_step = observe ? 0 : rl4rs_env_is_reward_step(s->env);
    // the observation-side mask is a function of the env state the act just left (slate.py:90-97); nothing below changes that state
    if (L.mask_i64 >= 0 && (rc = rl4rs_env_obs_mask(s->env, R + L.mask_i64, 2, stream))) return rc;
    char* H = reinterpret_cast<char*>(record_host);
    int64_t prefix = L.host_bytes;
    bool early = false;
    if (H && L.mask_i64 >= 0) {
        if ((rc = ensure_copy_stream(s))) return rc;
        RL4RS_HIP_TRY(hipEventRecord(s->ev_ready, st));
        RL4RS_HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev_ready, 0));
        RL4RS_HIP_TRY(hipMemcpyAsync(H + L.mask_i64, R + L.mask_i64, (size_t)(L.host_bytes - L.mask_i64), hipMemcpyDeviceToHost, s->copy_stream));
        RL4RS_HIP_TRY(hipEventRecord(s->ev_copied, s->copy_stream));
        prefix = L.mask_i64;
        early = true;
    }
    // the observation the caller gets: float32 activations, or the float64 row of the d3rlpy mode assembled from them
    const int64_t obs_off = L.obs_d3rl >= 0 ? L.obs_d3rl : L.obs;
    const int64_t obs_bytes = L.obs_d3rl >= 0 ? (int64_t)B * L.d3rl_cols * 8 : (int64_t)B * L.obs_dim * 4;
    bool obs_sent = false;
    // Steps without a reward forward (and resets): the observation is the LAST thing computed, so a device-to-host copy of its
    // 4 MB could only start when the GPU has nothing left to do (85 us at PCIe rate per step, GPU idle).  The head GEMM's epilogue
    // writes it to the pinned host block itself, tile by tile while the GEMM runs (k_gemm_h16's mirror destination): what is
    // left for the copy engine is the few KB around it.  (Reward steps overlap the copy with the reward forward instead; the
    // float64 d3rlpy rows are assembled by a kernel of their own and keep the copy.)
    bool mirror_armed = false;
    if (H && g_host_mirror && s->dien && reward_step != 1 && L.obs_d3rl < 0) {
        void* dp = nullptr;
        if (hipHostGetDevicePointer(&dp, H + L.obs, 0) == hipSuccess && dp) {
            rl4rs::dien_set_obs_mirror(s->dien, reinterpret_cast<float*>(dp));
            mirror_armed = true;
        } else {
            (void)hipGetLastError();          // not mapped for the device: the copy path below serves it
        }
    }
    auto finish_obs = [&]() -> int {
        if (mirror_armed && rl4rs::dien_obs_mirror_used(s->dien)) obs_sent = true;      // already on its way home
        if (L.obs_d3rl >= 0) {
            // masked_actions: all of prev_actions (slate.py:100-104) or the current page's columns (seqslate.py:18-23), POST-act step counter
            const int cur_after = cur + 1, T = s->cfg.max_steps, P = s->cfg.page_items;
            int c0 = 0, ncols = T;
            if (s->cfg.is_seq) {
                const int page_init = cur_after / P * P, page_end = (page_init + P - 1 < T - 1) ? page_init + P - 1 : T - 1;
                c0 = page_end + 1 - P; ncols = P;
            }
            void* pp; int64_t nb;
            int rc2 = rl4rs_env_buffer(s->env, RL4RS_BUF_PREV_ACTIONS, &pp, &nb);
            if (rc2) return rc2;
            const int64_t total = (int64_t)B * L.d3rl_cols;
            hipLaunchKernelGGL(k_record_d3rl, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, obs, L.obs_dim,
                               reinterpret_cast<const int32_t*>(pp), T, c0, ncols, cur_after, reinterpret_cast<double*>(R + L.obs_d3rl), B);
            RL4RS_LAUNCH_CHECK();
        }
        if (H && reward_step == 1) {
            // a reward step: 4 - 9 MB of observation would otherwise wait for the whole reward forward and then cross PCIe
            // with the GPU idle; it leaves now, on the copy stream, beside the reward forward
            int rc2 = ensure_copy_stream(s);
            if (rc2) return rc2;
            RL4RS_HIP_TRY(hipEventRecord(s->ev_ready, st));
            RL4RS_HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev_ready, 0));
            RL4RS_HIP_TRY(hipMemcpyAsync(H + obs_off, R + obs_off, (size_t)obs_bytes, hipMemcpyDeviceToHost, s->copy_stream));
            RL4RS_HIP_TRY(hipEventRecord(s->ev_copied, s->copy_stream));
            obs_sent = true;
            early = true;
        }
        return RL4RS_OK;
    };
    if (observe) {
        if ((rc = scorer_forward(s, B, 1, s->dense, s->cat, obs, nullptr, stream))) return rc;
        if ((rc = finish_obs())) return rc;
        if (L.mask_bits >= 0 && (rc = rl4rs_env_obs_mask(s->env, R + L.mask_bits, 4, stream))) return rc;
    } else if ((rc = after_act(s, cur, obs, reinterpret_cast<double*>(R + L.reward), reinterpret_cast<uint8_t*>(R + L.done),
                               L.mask_bits >= 0 ? reinterpret_cast<uint32_t*>(R + L.mask_bits) : nullptr, stream, finish_obs))) {
        return rc;
    }
    if (L.click_p >= 0 && reward_step == 1) {
        const int m = s->n_complete - 1;
        hipLaunchKernelGGL(k_record_click, dim3((B * (m + 1) + 255) / 256), dim3(256), 0, st, s->probs, s->p_last, m,
                           reinterpret_cast<float*>(R + L.click_p), B);
        RL4RS_LAUNCH_CHECK();
    }
    if (L.offline_action >= 0 && cur + 1 < s->cfg.max_steps) {
        // the logged action of the NEXT step (slate.py:152-161), so a replay loop needs no extra device round trip for it
        if ((rc = rl4rs_env_offline_action(s->env, action_kind == 0 ? reinterpret_cast<int32_t*>(R + L.offline_action) : nullptr,
                                           action_kind != 0 ? reinterpret_cast<double*>(R + L.offline_action) : nullptr, stream))) return rc;
    }
    {
        void* ep; int64_t nb; int32_t* rf = nullptr;
        if ((rc = rl4rs_env_buffer(s->env, RL4RS_BUF_ERROR_FLAG, &ep, &nb))) return rc;
        if (s->dien && (rc = rl4rs_dien_status_word(s->dien, &rf))) return rc;
        hipLaunchKernelGGL(k_record_status, dim3(1), dim3(64), 0, st, reinterpret_cast<const int32_t*>(ep), rf, reinterpret_cast<int32_t*>(R + L.status));
        RL4RS_LAUNCH_CHECK();
    }
    if (H) {
        if (obs_sent) {     // the prefix around the observation that is already on its way
            RL4RS_HIP_TRY(hipMemcpyAsync(H, R, (size_t)obs_off, hipMemcpyDeviceToHost, st));
            const int64_t tail = obs_off + ((obs_bytes + 63) & ~(int64_t)63);
            if (prefix > tail) RL4RS_HIP_TRY(hipMemcpyAsync(H + tail, R + tail, (size_t)(prefix - tail), hipMemcpyDeviceToHost, st));
        } else {
            RL4RS_HIP_TRY(hipMemcpyAsync(H, R, (size_t)prefix, hipMemcpyDeviceToHost, st));
        }
        if (early) RL4RS_HIP_TRY(hipStreamWaitEvent(st, s->ev_copied, 0));     // one wait on `stream` covers every copy (the copy stream is in order)
    }
    return RL4RS_OK;
}

int rl4rs_set_host_mirror(int32_t on) {
    g_host_mirror = on ? 1 : 0;
    return RL4RS_OK;
}

int rl4rs_env_step_record(rl4rs_stepper* s, const void* actions_dev, int32_t action_kind, uint32_t want, void* record_dev, void* stream) {
    return step_record(s, false, actions_dev, action_kind, want, record_dev, nullptr, stream);
}

int rl4rs_env_step_record_host(rl4rs_stepper* s, const void* actions_dev, int32_t action_kind, uint32_t want, void* record_dev,
                               void* record_host, void* stream) {
    RL4RS_REQUIRE(record_host, "env_step_record_host: null host block");
    return step_record(s, false, actions_dev, action_kind, want, record_dev, record_host, stream);
}

int rl4rs_env_observe_record_host(rl4rs_stepper* s, int32_t conti, uint32_t want, void* record_dev, void* record_host, void* stream) {
    return step_record(s, true, nullptr, conti ? 2 : 0, want, record_dev, record_host, stream);
}

}  // extern "C"
