"""The reward step beside the replay-ahead forward (rl4rs_amd/csrc/step_lanes.hpp) on the CPU: the header is compiled with
the host C++ compiler alone into stand-alone programs (address and undefined-behaviour checks where the toolchain has their runtimes, as
tests/test_step_lanes_ahead_host.py) that replay call sequences through ahead_decide / lane_ahead_start / lane_ahead_next /
lane_decide_beside / lane_join the way step.hip's rl4rs_env_step_discrete calls them.

  beside = the switch on (and the scorer's second scratch set at full size), a group forward was started on the lanes in this episode,
           nothing has joined and no caller has deviated since, and lane_decide would run the folded reward step on lane 0
           -> the reward step takes lane 1 and scratch set 1: no act of the other lane to wait for, the entry event for a foreign
           action, else lane 1's own hand-out
  else   = what lane_decide alone says, field for field

A reference simulation with the switch off runs beside every sequence: whatever is not claimed must be told what the reference is told,
and behind a reset both are in the same state but for the counters."""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'rl4rs_amd', 'csrc')

# step.hip's use of the header: sim_step is rl4rs_env_step_discrete's decision code, sim_join what lanes_wait does, sim_reset what a
# reset does (the env's load joins through the hook, then rl4rs_stepper_observe)
PRELUDE = r'''
#include <stdio.h>
#include "step_lanes.hpp"
using namespace rl4rs;
struct Sim { LaneState l; AheadState a; };
struct Knobs {
    bool on, own_row, slate, dien_x, carried, rows64_8, rows64_9;      // AheadCall
    bool overlap, no_reset_lane, no_reward_lane, room, fold;           // the lane switches; room: the distinct hint fits the chip
    bool beside;                                                       // rl4rs_stepper_set_reward_beside, and the full-size set was reserved
};
static Knobs knobs() { Knobs k = {true, true, true, true, true, true, true, true, false, false, true, true, true}; return k; }
static LaneCall lane_call(const Knobs& k, int cur, int T) {
    LaneCall c = LaneCall();
    c.overlap = k.overlap; c.dien_x = k.dien_x; c.carried = k.carried; c.own_row = k.own_row; c.extra_outputs = !k.slate;
    c.seq_num = 2; c.distinct_hint = k.room ? 1746 : 4096; c.n_cu = 256;
    c.reward_due = cur + 1 >= T;
    c.to_reward = (c.reward_due || (k.no_reset_lane && k.no_reward_lane)) ? 0 : T - 1 - cur;
    c.no_reward_lane = k.no_reward_lane;
    c.reward_fold = c.reward_due && c.overlap && c.dien_x && c.carried && k.fold;
    return c;
}
static void sim_join(Sim& s) { (void)ahead_cancel(s.a); (void)lane_join(s.l); }
static bool sim_reset(Sim& s, const Knobs& k, int T) {
    sim_join(s);
    LaneCall c = lane_call(k, -1, T);
    c.observe = true; c.carried = false; c.own_row = false; c.reward_due = false; c.no_reset_lane = k.no_reset_lane; c.to_reward = T;
    if (!lane_observe_eligible(c)) return false;
    (void)lane_decide(s.l, c);
    return true;
}
struct Told { AheadStep step; bool dropped, lanes; LanePlan p; };
static Told sim_step(Sim& s, const Knobs& k, int cur, int T) {
    Told t = Told();
    const LaneCall c = lane_call(k, cur, T);
    AheadCall a = AheadCall();
    a.on = k.on; a.own_row = k.own_row; a.slate = k.slate; a.dien_x = k.dien_x; a.carried = k.carried;
    a.rows64[0] = k.rows64_8; a.rows64[1] = k.rows64_9; a.lanes = lane_room(c); a.cur = cur; a.T = T;
    t.step = ahead_decide(s.a, a, &t.dropped);
    if (t.dropped) sim_join(s);
    t.lanes = s.a.lanes;
    if (t.step == AheadStep::Start) {
        if (t.lanes) t.p = lane_ahead_start(s.l);
        else { const AheadState now = s.a; sim_join(s); s.a = now; }
    } else if (t.step == AheadStep::Next) {
        if (t.lanes) t.p = lane_ahead_next(s.l);
    } else {
        t.p = lane_decide_beside(s.l, c, k.beside);
    }
    return t;
}
inline bool same_plan(const LanePlan& a, const LanePlan& b) {
    return a.lane == b.lane && a.on == b.on && a.join == b.join && a.wait_entry == b.wait_entry && a.wait_act == b.wait_act &&
           a.wait_handout == b.wait_handout && a.observe == b.observe && a.reward == b.reward;
}
'''


def _cxx():
    return next((x for x in ('g++', 'c++', 'clang++') if shutil.which(x)), None)


def _build_and_run(tmp_path, name, main):
    cxx = _cxx()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    src, exe = tmp_path / (name + '.cpp'), tmp_path / name
    src.write_text(PRELUDE + main)
    base = [cxx, '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I', CSRC, str(src), '-o', str(exe)]
    r = subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout, run.stderr)
    return run.stdout.splitlines()


SHOW = r'''
static void show(const Told& t) {
    const char* what = t.step == AheadStep::Start ? "start" : t.step == AheadStep::Next ? "next" : (t.p.lane ? (t.p.reward ? "reward" : "lane") : "serial");
    printf("%s lanes=%d drop=%d on=%d join=%d entry=%d act=%d handout=%d\n", what, (int)(t.step != AheadStep::None && t.lanes), (int)t.dropped,
           t.p.on, (int)t.p.join, (int)t.p.wait_entry, (int)t.p.wait_act, (int)t.p.wait_handout);
}
static void stats(const Sim& s) {
    printf("stats %lld %lld %lld | %lld %lld %lld %lld %lld %lld\n", (long long)s.a.started, (long long)s.a.handed, (long long)s.a.dropped,
           (long long)s.l.ran[0], (long long)s.l.ran[1], (long long)s.l.joins, (long long)s.l.ran_reset, (long long)s.l.ran_reward,
           (long long)s.l.ran_beside);
}
'''


def A(what, lanes=1, drop=0, on=0, join=0, entry=0, act=0, handout=0):
    return '%s lanes=%d drop=%d on=%d join=%d entry=%d act=%d handout=%d' % (what, lanes, drop, on, join, entry, act, handout)


def test_written_out_episodes(tmp_path):
    """The flagship episode (T = 9) twice in a row, a clone of the logged action at the last act, a clone at act 3, a join behind act
    1, the switch off, no_reward_lane, and T = 10 (the reward step does not fold): what every call is told, written out by hand."""
    main = SHOW + r'''
int main() {
    { printf("seq flagship twice\n"); Sim s = Sim(); Knobs k = knobs();
      for (int ep = 0; ep < 2; ++ep) { sim_reset(s, k, 9); for (int cur = 0; cur < 9; ++cur) show(sim_step(s, k, cur, 9)); }
      stats(s); }
    { printf("seq clone at the last act\n"); Sim s = Sim(); Knobs k = knobs(); sim_reset(s, k, 9);
      for (int cur = 0; cur < 9; ++cur) { k.own_row = cur != 8; show(sim_step(s, k, cur, 9)); }
      stats(s); }
    { printf("seq clone at act 3\n"); Sim s = Sim(); Knobs k = knobs(); sim_reset(s, k, 9);
      for (int cur = 0; cur < 9; ++cur) { k.own_row = cur != 3; show(sim_step(s, k, cur, 9)); }
      stats(s); }
    { printf("seq join behind act 1\n"); Sim s = Sim(); Knobs k = knobs(); sim_reset(s, k, 9);
      for (int cur = 0; cur < 9; ++cur) { show(sim_step(s, k, cur, 9)); if (cur == 1) sim_join(s); }
      stats(s); }
    { printf("seq switch off\n"); Sim s = Sim(); Knobs k = knobs(); k.beside = false; sim_reset(s, k, 9);
      for (int cur = 0; cur < 9; ++cur) show(sim_step(s, k, cur, 9));
      stats(s); }
    { printf("seq no_reward_lane\n"); Sim s = Sim(); Knobs k = knobs(); k.no_reward_lane = true; sim_reset(s, k, 9);
      for (int cur = 0; cur < 9; ++cur) show(sim_step(s, k, cur, 9));
      stats(s); }
    { printf("seq horizon 10\n"); Sim s = Sim(); Knobs k = knobs(); k.fold = false; sim_reset(s, k, 10);
      for (int cur = 0; cur < 10; ++cur) show(sim_step(s, k, cur, 10));
      stats(s); }
    return 0;
}
'''
    out = _build_and_run(tmp_path, 'beside_lines', main)
    got, name = {}, None
    for ln in out:
        if ln.startswith('seq '):
            name = ln[4:]
            got[name] = []
        else:
            got[name].append(ln)
    lane = lambda on, handout=1: A('lane', lanes=0, on=on, act=1, handout=handout)      # noqa: E731
    episode = [A('start', act=1)] + [A('next', on=1, act=1)] * 7
    want = {
        # reset on lane 1; the start on lane 0; seven acts on lane 1; the reward step on lane 1 in stream order behind the act of t7 -
        # no act to wait for, lane 1's own hand-out (the reset's observation) before its buffers are rewritten.  The same again behind
        # the next reset (which joins): two reset forwards, two reward steps, both beside
        'flagship twice': episode + [A('reward', lanes=0, on=1, handout=1)] + episode + [A('reward', lanes=0, on=1, handout=1),
                                                                                           'stats 2 16 0 | 0 0 1 2 2 2'],
        # a foreign action at the reward step: all eight rows were handed out, nothing is dropped; the lane waits for the entry event
        'clone at the last act': episode + [A('reward', lanes=0, on=1, entry=1), 'stats 1 8 0 | 0 0 0 1 1 1'],
        # the clone at act 3 drops the forward and joins: the reward step is where lane_decide puts it, lane 0 beside the act of t7
        'clone at act 3': [A('start', act=1), A('next', on=1, act=1), A('next', on=1, act=1),
                           A('lane', lanes=0, drop=1, on=1, entry=1), lane(0, handout=0), lane(1), lane(0), lane(1),
                           A('reward', lanes=0, on=0, act=1, handout=1), 'stats 1 3 5 | 2 3 1 1 1 0'],
        'join behind act 1': [A('start', act=1), A('next', on=1, act=1), A('lane', lanes=0, on=0, entry=1), lane(1, handout=0), lane(0), lane(1),
                              lane(0), lane(1), A('reward', lanes=0, on=0, act=1, handout=1), 'stats 1 2 6 | 3 3 1 1 1 0'],
        # the switch off: DESIGN 40's episode
        'switch off': episode + [A('reward', lanes=0, on=0, act=1, handout=1), 'stats 1 8 0 | 0 0 0 1 1 0'],
        # every reward step joins
        'no_reward_lane': episode + [A('serial', lanes=0, join=1), 'stats 1 8 0 | 0 0 1 1 0 0'],
        # T = 10: ten rows per env are no 64-row shape, the reward step does not fold and joins
        'horizon 10': [A('start')] + [A('next', on=1, act=1)] * 8 + [A('serial', lanes=0, join=1), 'stats 1 9 0 | 0 0 1 1 0 0'],
    }
    assert list(got) == list(want)
    wrong = [(n, i, g, w) for n in want for i, (g, w) in enumerate(zip(got[n], want[n])) if g != w]
    wrong += [(n, len(got[n]), len(want[n])) for n in want if len(got[n]) != len(want[n])]
    assert not wrong, wrong


def test_every_horizon_switch_deviation_join_and_reset(tmp_path):
    """Horizons 2 .. 12, three episodes in a row, each switch combination (reward_beside, replay-ahead, no_reset_lane, no_reward_lane,
    no_step_overlap, lane room, the reward step's fold); in the second episode a foreign action at each act together with a join at
    each point, or a reset behind each act.  The test keeps its own record of "a group forward was started on the lanes in this
    episode and nothing has joined or deviated since" and a reference simulation with the switch off.  Checked at every call:
      - the reward step is claimed (lane 1, set 1, no act waited for, the entry event exactly for a foreign action, else lane 1's
        hand-out) exactly where that record holds, the switch is on and the reference runs the reward step on lane 0;
      - every other call is told what the reference is told, field for field;
      - a full-size forward's scratch set is its lane's: the group forward set 0 on lane 0, a reward step set 0 on lane 0 (behind the
        group forward in stream order) or set 1 on lane 1 - never two of them on one set from two streams;
      - behind every reset the lane state equals the reference's but for the counters, and the counters differ by the claims alone."""
    main = r'''
int main() {
    long long bad = 0, claims = 0, declined = 0, foreign_claims = 0, rewards_ref = 0;
    for (int T = 2; T <= 12; ++T)
      for (int sw = 0; sw < 128; ++sw)
        for (int dev = -1; dev < T; ++dev)
          for (int ev = -1; ev < 2 * T; ++ev) {
            // ev < T: a join behind act ev; ev >= T: a reset behind act ev - T (then no foreign action: the episode ends there)
            const int join_at = ev < T ? ev : -1, reset_at = ev >= T ? ev - T : -1;
            if (reset_at >= 0 && dev >= 0) continue;
            Knobs k = knobs();
            k.beside = !(sw & 1); k.on = !(sw & 2); k.no_reset_lane = sw & 4; k.no_reward_lane = sw & 8; k.overlap = !(sw & 16); k.room = !(sw & 32);
            k.fold = !(sw & 64);
            Knobs k0 = k; k0.beside = false;
            Sim s = Sim(), ref = Sim();
            long long mine = 0;
            for (int ep = 0; ep < 3; ++ep) {
                const bool taken = sim_reset(s, k, T);
                if (sim_reset(ref, k0, T) != taken) ++bad;
                // behind a reset: the same lanes in flight, the same lane next; the counters differ by the claims
                if (s.l.in_flight != ref.l.in_flight || s.l.used[0] != ref.l.used[0] || s.l.used[1] != ref.l.used[1] || s.l.group0 || ref.l.group0 ||
                    (s.l.in_flight && s.l.last != ref.l.last) || s.l.ran_reset != ref.l.ran_reset || s.l.ran_reward != ref.l.ran_reward ||
                    s.l.ran[0] != ref.l.ran[0] || s.l.ran[1] != ref.l.ran[1] || s.l.joins != ref.l.joins || s.l.ran_beside != mine ||
                    ref.l.ran_beside != 0 || s.a.active || s.a.started != ref.a.started || s.a.handed != ref.a.handed || s.a.dropped != ref.a.dropped) ++bad;
                bool own_next = taken, open = false;     // open: the test's own record of the group forward on lane 0
                for (int cur = 0; cur < T; ++cur) {
                    k.own_row = k0.own_row = own_next && !(ep == 1 && cur == dev);
                    const Sim before = s;
                    const Told t = sim_step(s, k, cur, T), r = sim_step(ref, k0, cur, T);
                    if (t.step != r.step || t.dropped != r.dropped) ++bad;
                    if (t.dropped) open = false;
                    if (t.step == AheadStep::Start) {
                        if (!same_plan(t.p, r.p)) ++bad;
                        open = t.lanes;
                        if (t.lanes && t.p.on != 0) ++bad;                   // the group forward: lane 0, set 0
                    } else if (t.step == AheadStep::Next) {
                        if (!same_plan(t.p, r.p) || (t.lanes && t.p.on != 1)) ++bad;
                    } else {
                        const bool ref_on0 = r.p.lane && r.p.reward && r.p.on == 0;
                        if (r.p.lane && r.p.reward) ++rewards_ref;
                        if (k.beside && open && ref_on0) {
                            ++claims; ++mine;
                            if (!k.own_row) ++foreign_claims;
                            if (!(t.p.lane && t.p.reward && t.p.on == 1 && !t.p.join && !t.p.observe && !t.p.wait_act && t.p.wait_entry == !k.own_row &&
                                  t.p.wait_handout == (k.own_row && before.l.used[1]))) ++bad;
                            if (!(s.l.in_flight && s.l.last == 1 && s.l.used[0] && s.l.used[1])) ++bad;      // a join waits for both lanes
                        } else {
                            if (open && ref_on0) ++declined;
                            if (!same_plan(t.p, r.p)) ++bad;
                        }
                        if (t.p.lane && t.p.reward) {
                            // the reward forward's set is its lane's; on set 0 it is lane 0's, behind the group forward in stream order
                            if (lane_reward_set(t.p.on) != t.p.on) ++bad;
                            if (open && lane_reward_set(t.p.on) == 0 && t.p.on != 0) ++bad;
                        }
                        open = false;
                    }
                    if (s.l.group0 != open) ++bad;                           // the header's mark is the test's record
                    own_next = true;
                    if (ep == 1 && cur == join_at) { sim_join(s); sim_join(ref); open = false; if (s.l.group0 || s.l.in_flight) ++bad; }
                    if (ep == 1 && cur == reset_at) break;
                }
            }
            if (s.l.ran_beside != mine || ref.l.ran_beside != 0 || s.l.ran_reward != ref.l.ran_reward) ++bad;
          }
    printf("bad %lld claims %d declined %d foreign %d rewards %d\n", bad, claims > 0, declined > 0, foreign_claims > 0, rewards_ref > 0);
    return bad != 0;
}
'''
    out = _build_and_run(tmp_path, 'beside_sweep', main)
    assert out[-1] == 'bad 0 claims 1 declined 1 foreign 1 rewards 1', out[-1]
