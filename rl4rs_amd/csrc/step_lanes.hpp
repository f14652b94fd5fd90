// Which stream a transition of rl4rs_env_step_discrete runs on, and what it waits for.  The observation-sized AUGRU
// launch is bound by one workgroup's 64-step chain and fills less than half of the chip once the row dedup has run;
// in a replay loop transition k + 1 needs nothing of transition k's scorer forward - only the env state, the partition and the
// logged-action row the ACT of k left.  The stepper therefore owns two lanes (a stream and its events each) and runs consecutive
// eligible transitions on them in turn: the forward of k + 1 starts beside the forward of k.
// The two ends of an episode use the same two lanes: the reset's observation forward is a lane transition without an act
// (rl4rs_stepper_observe), and a reward step that is ONE forward of n_complete rows per env takes lane 0 beside the last observation
// transition on lane 1 (tests/test_step_lanes_episode_host.py).
// Host code only, nothing from HIP (as dien_plan.hpp): step.hip carries out what lane_decide returns, tests/test_step_lanes_host.py
// replays call sequences through it without a device.
#pragma once
#include <stdint.h>

namespace rl4rs {

// the workgroups two observation-sized k_augru_xs / k_augru_x launches bring: they co-run only where both fit the chip at once
inline int64_t lane_pair_workgroups(int seq_num, int distinct_hint) { return 2 * (int64_t)seq_num * ((distinct_hint + 31) / 32); }

// what step.hip knows about the call in front of its act
struct LaneCall {
    bool overlap;          // rl4rs_stepper_set_step_overlap (and the env / scorer handles still point at this stepper's lanes)
    bool dien_x;           // the scorer is the DIEN on the k_augru_x / k_augru_xs path (fp16x2)
    bool carried;          // plan_refine returned true: the act carries the partition (false on a SeqSlate page turn)
    bool reward_due;       // a reward is due after this act
    bool extra_outputs;    // mask_bits_dev or done_dev asked for
    bool own_row;          // actions_dev is the logged-action row the previous transition's act wrote
    int seq_num, distinct_hint, n_cu;
    // DESIGN 39 - every field below is zero in a call built the way DESIGN 38's callers build it, and lane_decide then answers as it did
    bool observe;          // rl4rs_stepper_observe: the reset's observation forward - no act, its own k_row_dedup (carried is not asked for)
    bool no_reset_lane;    // rl4rs_stepper_set_reset_lane(s, 0): that forward stays on the caller's stream
    bool reward_fold;      // the reward step is ONE forward of n_complete rows per env (fold_obs) and a reward block was given
    bool no_reward_lane;   // rl4rs_stepper_set_reward_lane(s, 0): the reward step joins
    int to_reward;         // lane transitions from this one up to the reward step, this one included, the reward step not; 0 = unknown
};

inline bool lane_room(const LaneCall& c) {
    return c.overlap && c.dien_x && !c.extra_outputs && lane_pair_workgroups(c.seq_num, c.distinct_hint) <= c.n_cu;
}
inline bool lane_eligible(const LaneCall& c) { return lane_room(c) && !c.observe && c.carried && !c.reward_due; }
// the reset's observation forward: the same rule without the act's conditions
inline bool lane_observe_eligible(const LaneCall& c) { return lane_room(c) && c.observe && !c.no_reset_lane; }

// host-side record of what is in flight
struct LaneState {
    int next;              // the lane of the next lane transition (they alternate)
    bool in_flight;        // a lane transition was issued since the last join
    bool used[2];          // ... on this lane: its `done` and hand-out events are recorded
    int last;              // the lane of the last lane transition (valid while in_flight)
    int64_t ran[2];        // lane transitions issued on each lane, joins carried out (rl4rs_stepper_lane_stats)
    int64_t joins;
    int64_t ran_reset, ran_reward;   // reset forwards and reward steps issued on a lane (rl4rs_stepper_lane_stats_ex): not part of ran[]
    // DESIGN 42 - the forward last issued on lane 0 is a replay-ahead group forward and nothing has joined since (set by
    // lane_ahead_start, dropped by lane_join and by whatever lane_decide_beside is asked next)
    bool group0;
    int64_t ran_beside;    // reward steps issued on lane 1 beside that forward (rl4rs_stepper_reward_beside_stats): part of ran_reward
};

struct LanePlan {
    bool lane;             // true: the transition runs on lane `on`; false: on the caller's stream, with today's launches
    int on;
    bool join;             // (lane == false) the caller's stream first waits for `done` of every lane in flight
    bool wait_entry;       // record the entry event on the caller's stream, the lane waits for it: a foreign action, or the
                           // first lane transition behind work on the caller's stream
    bool wait_act;         // the lane waits for `act_done` of lane `on ^ 1` (env state, partition, logged-action row of k - 1)
    bool wait_handout;     // the lane waits for the hand-out copy of its own previous transition (it rewrites the lane's
                           // observation and reward buffers); implied by wait_entry, which the caller's stream records behind it
    bool observe;          // (lane == true) the reset's observation forward: no act; `act_done` is recorded behind its k_row_dedup
    bool reward;           // (lane == true) the folded reward step: act, complete rows, the n_complete-row forward, the reward
};

// join: everything in flight is waited for by the stream the caller gave (step.hip issues the waits when this returns true)
inline bool lane_join(LaneState& s) {
    const bool any = s.in_flight;
    if (any) s.joins += 1;
    s.in_flight = false;
    s.used[0] = s.used[1] = false;
    s.group0 = false;
    return any;
}

// a transition that lane_decide placed on a lane could not be enqueued (its act failed before anything was launched): the state
// as it was in front of lane_decide (the caller kept a copy) stands again
inline void lane_undo(LaneState& s, const LaneState& before) { s = before; }

// ---- the links between a stepper and the env / scorer handles it is attached to
// The env and the scorer hold a pointer to the stepper's hook and call lanes_join through it in front of everything that touches what
// a lane may have in flight.  Any of the three may be destroyed first, and a later stepper may take a handle over: whoever goes (or
// is replaced) tells the other side, so that nobody keeps a pointer into freed memory.
//   - a handle that is destroyed: lanes_join (the host waits), then lanes_gone - the stepper forgets the handle;
//   - a stepper that is destroyed: lane_links_release - the handles that still point at its hook forget it;
//   - a stepper that attaches to a handle another stepper holds: lane_links_attach joins the old one and tells it the handle is gone.
// A stepper runs lanes only while lane_links_mine holds for its env and its scorer.
enum { LANE_LINK_ENV = 0, LANE_LINK_SCORER = 1 };
struct LaneHook {
    void* ctx;
    int (*join)(void* ctx, void* stream, int have_stream);      // 0 = ok
    void (*gone)(void* ctx, int which);                         // the handle `which` no longer points at this hook
};
inline int lanes_join(const LaneHook* h, void* stream, bool have_stream = true) {
    return h ? h->join(h->ctx, stream, have_stream ? 1 : 0) : 0;
}
inline void lanes_gone(const LaneHook* h, int which) {
    if (h && h->gone) h->gone(h->ctx, which);
}
// the stepper's side: where each handle keeps its pointer to the hook, NULL = never attached, gone or taken over
struct LaneLinks { const LaneHook** slot[2]; };
inline void lane_links_attach(LaneLinks& l, int which, const LaneHook** slot, const LaneHook* hook) {
    if (*slot && *slot != hook) {
        (void)lanes_join(*slot, nullptr, false);
        lanes_gone(*slot, which);
    }
    *slot = hook;
    l.slot[which] = slot;
}
inline void lane_links_gone(LaneLinks& l, int which) { l.slot[which] = nullptr; }
inline bool lane_links_mine(const LaneLinks& l, int which, const LaneHook* hook) { return l.slot[which] && *l.slot[which] == hook; }
inline void lane_links_release(LaneLinks& l, const LaneHook* hook) {
    for (int w = 0; w < 2; ++w) {
        if (lane_links_mine(l, w, hook)) *l.slot[w] = nullptr;
        l.slot[w] = nullptr;
    }
}

// The scorer's second scratch set holds an observation-sized forward only: the reward forward runs on lane 0 (set 0) and the
// observation transition still in flight beside it must be the one on lane 1.  Lanes alternate while something is in flight, so
// the lane is chosen where nothing is: the first of `to_reward` lane transitions in a row starts on the lane that puts the last on 1.
inline int lane_first(int to_reward) { return 1 ^ ((to_reward - 1) & 1); }

// the folded reward step takes lane 0 beside the observation transition in flight on lane 1 - and joins in every other case
inline bool lane_reward_eligible(const LaneState& s, const LaneCall& c) {
    return lane_room(c) && !c.observe && c.carried && c.reward_due && c.reward_fold && !c.no_reward_lane && s.in_flight && s.last == 1;
}

inline LanePlan lane_decide(LaneState& s, const LaneCall& c) {
    LanePlan p = {};
    if (lane_reward_eligible(s, c)) {
        p.lane = p.reward = true;
        p.on = 0;
        p.wait_act = true;
        p.wait_entry = !c.own_row;
        p.wait_handout = !p.wait_entry && s.used[0];
        s.used[0] = true;
        s.last = 0;
        s.ran_reward += 1;
        s.next = 1;
        return p;
    }
    if (lane_observe_eligible(c)) {
        // behind the load, the reset and the encode on the caller's stream: whatever is still in flight is joined first (step.hip
        // issues the waits), then the lane waits for the entry event
        p.join = lane_join(s);
        p.lane = p.observe = true;
        p.on = c.to_reward > 0 ? lane_first(c.to_reward) : s.next;
        p.wait_entry = true;
        s.in_flight = true;
        s.used[p.on] = true;
        s.last = p.on;
        s.ran_reset += 1;
        s.next = p.on ^ 1;
        return p;
    }
    if (!lane_eligible(c)) {
        p.join = lane_join(s);
        return p;
    }
    p.lane = true;
    p.on = (!s.in_flight && c.to_reward > 0) ? lane_first(c.to_reward) : s.next;
    p.wait_act = s.in_flight;                       // transition k - 1 ran on the other lane: lanes alternate
    p.wait_entry = !s.in_flight || !c.own_row;
    p.wait_handout = !p.wait_entry && s.used[p.on];
    s.in_flight = true;
    s.used[p.on] = true;
    s.last = p.on;
    s.ran[p.on] += 1;
    s.next = p.on ^ 1;
    return p;
}

// ---- replay-ahead.  In a replay loop the observation row of transition k is a function of the log line and the logged
// actions up to k, all of which the stepper knows: once the caller hands back the stepper's own logged-action row (own_row) at act
// index c0, the rows of the transitions c0 .. T - 2 are scored in ONE forward of n = T - 1 - c0 rows per env - the 64-row form of
// k_augru_x, where a row costs about two thirds of what it costs in an observation-sized launch - and every later transition runs its
// act alone and is handed its row.  A caller that deviates (a foreign action pointer, any other entry point, a reset) wastes the rows
// not handed out yet, nothing else: env state was only ever advanced by real acts.
struct AheadCall {
    bool on;               // rl4rs_stepper_set_replay_ahead
    bool own_row;          // as LaneCall::own_row
    bool slate;            // a Slate env (no SeqSlate), discrete actions, neither done_dev nor mask_bits_dev asked for
    bool dien_x;           // the scorer is the DIEN on the k_augru_x path ...
    bool carried;          // ... and the act of this transition carries the partition
    bool rows64[2];        // dien_augru_rows64(dien, B, 8) / (dien, B, 9): the forward of 8 / 9 rows per env runs the 64-row form
    bool lanes;            // the two lanes may be used (lane_room, both handles linked): the forward runs on lane 0, the later acts
                           // on lane 1; false: everything on the caller's stream
    int cur, T;            // the act index of this transition, the horizon
};
struct AheadState {
    bool active;           // rows of a forward are still to be handed out
    bool lanes;            // the forward in flight was issued on the lanes
    int c0, n;             // its first act index, its rows per env
    int next;              // the act index whose row is handed out next
    int64_t started, handed, dropped;      // forwards started; rows per env handed out / dropped (rl4rs_stepper_replay_stats)
};
enum class AheadStep { None, Start, Next };

inline int ahead_rows(int cur, int T) { return T - 1 - cur; }
inline bool ahead_trigger(const AheadCall& c) {
    const int n = ahead_rows(c.cur, c.T);
    return c.on && c.own_row && c.slate && c.dien_x && c.carried && (n == 8 || n == 9) && c.rows64[n - 8];
}
// every way out but the last hand-out: the rows not handed out yet are dropped (step.hip joins where it has to)
inline bool ahead_cancel(AheadState& s) {
    if (!s.active) return false;
    s.dropped += s.c0 + s.n - s.next;
    s.active = false;
    return true;
}
// what this transition is: the start of a forward (row 0 is handed out with it), the hand-out of the next row behind its act alone,
// or a transition like any other (*dropped: a forward was in flight and the caller deviated - join first)
inline AheadStep ahead_decide(AheadState& s, const AheadCall& c, bool* dropped) {
    *dropped = false;
    if (s.active) {
        if (c.on && c.own_row && c.slate && c.cur == s.next && c.cur < s.c0 + s.n) {
            s.next += 1;
            s.handed += 1;
            if (s.next == s.c0 + s.n) s.active = false;
            return AheadStep::Next;
        }
        *dropped = ahead_cancel(s);
    }
    if (!ahead_trigger(c)) return AheadStep::None;
    s.active = true;
    s.lanes = c.lanes;
    s.c0 = c.cur;
    s.n = ahead_rows(c.cur, c.T);
    s.next = c.cur + 1;
    s.started += 1;
    s.handed += 1;
    return AheadStep::Start;
}
// the lane side of a start on the lanes: the act of c0, the row builder and the forward take lane 0 (the scorer's full-size scratch
// set), behind `act_done` of a transition in flight on lane 1 (the reset's forward) or, on lane 0, in stream order; the lane's own
// buffers are not written, so no hand-out is waited for
inline LanePlan lane_ahead_start(LaneState& s) {
    LanePlan p = {};
    p.lane = true;
    p.on = 0;
    p.wait_entry = !s.in_flight;
    p.wait_act = s.in_flight && s.last == 1;
    s.in_flight = true;
    s.used[0] = true;
    s.last = 0;
    s.next = 1;
    s.group0 = true;
    return p;
}
// a later act: lane 1, behind lane 0's `act_done` (recorded behind the row builder: the act rewrites what it read).  It leaves the
// state a reward step looks for: the transition in flight last is lane 1's, so the folded reward step takes lane 0 behind the forward
inline LanePlan lane_ahead_next(LaneState& s) {
    LanePlan p = {};
    p.lane = true;
    p.on = 1;
    p.wait_act = true;
    s.in_flight = true;
    s.used[1] = true;
    s.last = 1;
    s.next = 0;
    return p;
}

// ---- the reward step beside the group forward.  Behind a replay-ahead forward lane 0 holds that forward until it ends,
// and a folded reward step placed there (lane_decide) starts its act, its row builder and its front kernels only then - although none
// of them needs anything of the forward.  With a second scratch set of full size (`on`: the switch, and the set was reserved) the
// reward step takes LANE 1 and SET 1 instead: in stream order behind the later acts, so no act is waited for across lanes; its AUGRU
// launch still waits for lane 0's `done` (step.hip).  Claimed only where lane_decide would have put the reward step on lane 0 AND the
// forward in flight there is a group forward nothing has joined since; every other call is answered by lane_decide alone.
// Whatever the answer, the transition asked about is either a join or the next thing issued on the lanes: the mark goes.
inline bool lane_beside_eligible(const LaneState& s, const LaneCall& c, bool on) { return on && s.group0 && lane_reward_eligible(s, c); }
inline LanePlan lane_decide_beside(LaneState& s, const LaneCall& c, bool on) {
    const bool beside = lane_beside_eligible(s, c, on);
    s.group0 = false;
    if (!beside) return lane_decide(s, c);
    LanePlan p = {};
    p.lane = p.reward = true;
    p.on = 1;
    p.wait_entry = !c.own_row;
    p.wait_handout = !p.wait_entry && s.used[1];
    s.used[1] = true;
    s.last = 1;
    s.ran_reward += 1;
    s.ran_beside += 1;
    s.next = 0;
    return p;
}
// the scratch set and the event in front of the AUGRU launch of a reward step on lane `on`: the set of its lane, the other lane's `done`
inline int lane_reward_set(int on) { return on; }

}  // namespace rl4rs
