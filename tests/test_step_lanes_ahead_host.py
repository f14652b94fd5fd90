"""Replay-ahead (rl4rs_amd/csrc/step_lanes.hpp) on the CPU: the header is compiled with the host C++ compiler alone into
stand-alone programs (address and undefined-behaviour checks where the toolchain has their runtimes, as tests/test_step_lanes_host.py)
that replay call sequences through ahead_decide / ahead_cancel / lane_ahead_start / lane_ahead_next / lane_decide / lane_join the
way step.hip's rl4rs_env_step_discrete calls them.

  start  = the switch on, the caller hands back the stepper's own row, a Slate env without mask / done outputs, the DIEN on k_augru_x
           with a carried partition, n = T - 1 - cur in {8, 9} and the 64-row form admitted for n rows per env -> ONE forward of n rows
           per env: on lane 0 (the scorer's first scratch set) behind `act_done` of lane 1 or in lane 0's stream order, or - no lane
           room - on the caller's stream
  next   = every later own-row transition up to act T - 2: its act alone (lane 1 behind lane 0's `act_done`), its row handed out
  else   = the rows not handed out yet are dropped, the lanes are joined, the transition is what it was without the switch

The plan of the group forward (dien_plan.hpp): with DienCall::rows_differ the per-row category kernel and k_augru_x_64."""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'rl4rs_amd', 'csrc')

# step.hip's use of the header, once: sim_step is rl4rs_env_step_discrete's decision code, sim_join what lanes_wait does
PRELUDE = r'''
#include <stdio.h>
#include "step_lanes.hpp"
using namespace rl4rs;
struct Sim { LaneState l; AheadState a; };
struct Knobs {
    bool on, own_row, slate, dien_x, carried, rows64_8, rows64_9;      // AheadCall
    bool overlap, no_reset_lane, no_reward_lane, room, fold;           // the lane switches; room: the distinct hint fits the chip
};
static Knobs knobs() { Knobs k = {true, true, true, true, true, true, true, true, false, false, true, true}; return k; }
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
static bool sim_observe(Sim& s, const Knobs& k, int T) {
    LaneCall c = lane_call(k, -1, T);
    c.observe = true; c.carried = false; c.own_row = false; c.reward_due = false; c.no_reset_lane = k.no_reset_lane; c.to_reward = T;
    if (!lane_observe_eligible(c)) return false;
    sim_join(s);
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
        t.p = lane_decide(s.l, c);
    }
    return t;
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
    base = [cxx, '-std=c++17', '-Wall', '-Wextra', '-Werror', '-I', CSRC, str(src), '-o', str(exe)]
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
    printf("stats %lld %lld %lld | %lld %lld %lld %lld %lld\n", (long long)s.a.started, (long long)s.a.handed, (long long)s.a.dropped,
           (long long)s.l.ran[0], (long long)s.l.ran[1], (long long)s.l.joins, (long long)s.l.ran_reset, (long long)s.l.ran_reward);
}
'''


def A(what, lanes=1, drop=0, on=0, join=0, entry=0, act=0, handout=0):
    return '%s lanes=%d drop=%d on=%d join=%d entry=%d act=%d handout=%d' % (what, lanes, drop, on, join, entry, act, handout)


def test_written_out_episodes(tmp_path):
    """The flagship episode (T = 9), the other parity (T = 10), a clone of the logged action at act 3, a join behind act 1, no lane
    room, and each switch: what every call is told, written out by hand from the rule."""
    main = SHOW + r'''
int main() {
    { printf("seq flagship\n"); Sim s = Sim(); Knobs k = knobs(); sim_observe(s, k, 9);
      for (int cur = 0; cur < 9; ++cur) show(sim_step(s, k, cur, 9));
      stats(s); }
    { printf("seq horizon 10\n"); Sim s = Sim(); Knobs k = knobs(); k.fold = false; sim_observe(s, k, 10);
      for (int cur = 0; cur < 10; ++cur) show(sim_step(s, k, cur, 10));
      stats(s); }
    { printf("seq clone at act 3\n"); Sim s = Sim(); Knobs k = knobs(); sim_observe(s, k, 9);
      for (int cur = 0; cur < 9; ++cur) { k.own_row = cur != 3; show(sim_step(s, k, cur, 9)); }
      stats(s); }
    { printf("seq join behind act 1\n"); Sim s = Sim(); Knobs k = knobs(); sim_observe(s, k, 9);
      for (int cur = 0; cur < 9; ++cur) { show(sim_step(s, k, cur, 9)); if (cur == 1) sim_join(s); }
      stats(s); }
    { printf("seq no room, horizon 10\n"); Sim s = Sim(); Knobs k = knobs(); k.room = false; const bool taken = sim_observe(s, k, 10);
      for (int cur = 0; cur < 10; ++cur) { k.own_row = cur > 0 || taken; show(sim_step(s, k, cur, 10)); }
      stats(s); }
    { printf("seq switch off\n"); Sim s = Sim(); Knobs k = knobs(); k.on = false; sim_observe(s, k, 9);
      for (int cur = 0; cur < 9; ++cur) show(sim_step(s, k, cur, 9));
      stats(s); }
    return 0;
}
'''
    out = _build_and_run(tmp_path, 'ahead_lines', main)
    got, name = {}, None
    for ln in out:
        if ln.startswith('seq '):
            name = ln[4:]
            got[name] = []
        else:
            got[name].append(ln)
    lane = lambda on, handout=1: A('lane', lanes=0, on=on, act=1, handout=handout)      # noqa: E731
    want = {
        # reset on lane 1; the start on lane 0 behind its `act_done`; seven acts on lane 1; the reward step on lane 0 behind the forward
        'flagship': [A('start', act=1)] + [A('next', on=1, act=1)] * 7 + [A('reward', lanes=0, on=0, act=1, handout=1),
                                                                            'stats 1 8 0 | 0 0 0 1 1'],
        # T = 10: the reset's forward holds lane 0, the start follows it in stream order; the reward step does not fold (10 rows per env
        # are no 64-row shape) and joins
        'horizon 10': [A('start')] + [A('next', on=1, act=1)] * 8 + [A('serial', lanes=0, join=1), 'stats 1 9 0 | 0 0 1 1 0'],
        # acts 0 .. 2 handed out; the clone drops five rows and joins, then runs as a first lane transition behind the caller's stream
        # (to_reward 5: lane 1), the rest alternate, the reward step on lane 0
        'clone at act 3': [A('start', act=1), A('next', on=1, act=1), A('next', on=1, act=1),
                           A('lane', lanes=0, drop=1, on=1, entry=1), lane(0, handout=0), lane(1), lane(0), lane(1),
                           A('reward', lanes=0, on=0, act=1, handout=1), 'stats 1 3 5 | 2 3 1 1 1'],
        # the join (a mask read) drops six rows; act 2 is the stepper's own row again but only six rows are left: six lane transitions
        # from lane 0 (to_reward 6), the reward step on lane 0 beside the last of them
        'join behind act 1': [A('start', act=1), A('next', on=1, act=1), A('lane', lanes=0, on=0, entry=1), lane(1, handout=0), lane(0), lane(1),
                              lane(0), lane(1), A('reward', lanes=0, on=0, act=1, handout=1), 'stats 1 2 6 | 3 3 1 1 1'],
        # all-distinct: no reset lane, so act 0 is a foreign row; act 1 starts 8 rows per env on the caller's stream
        'no room, horizon 10': [A('serial', lanes=0)] + [A('start', lanes=0)] + [A('next', lanes=0)] * 7 + [A('serial', lanes=0), 'stats 1 8 0 | 0 0 0 0 0'],
        # the switch off: DESIGN 39's episode
        'switch off': [lane(0, handout=0)] + [lane(1 ^ (i & 1)) for i in range(7)] + [A('reward', lanes=0, on=0, act=1, handout=1),
                                                                                       'stats 0 0 0 | 4 4 0 1 1'],
    }
    assert list(got) == list(want)
    wrong = [(n, i, g, w) for n in want for i, (g, w) in enumerate(zip(got[n], want[n])) if g != w]
    wrong += [(n, len(got[n]), len(want[n])) for n in want if len(got[n]) != len(want[n])]
    assert not wrong, wrong


def test_every_horizon_deviation_join_and_switch(tmp_path):
    """Horizons 2 .. 12, each switch combination (replay-ahead, no_reset_lane, no_reward_lane, no_step_overlap, lane room, the 64-row
    form admitted for 8 / 9 rows), a foreign action at each act and a join at each point.  Checked after every call:
      - a forward starts only on an own row of a Slate env with a carried partition, n in {8, 9} and that form admitted, never with
        the switch off;
      - every row of a started forward is handed out or dropped, and a hand-out is the act its row was built for;
      - the scorer's first scratch set: while rows are outstanding no transition takes a lane, and a reward step behind a forward issued
        on the lanes is on lane 0 (its stream) or has joined; a forward on the caller's stream leaves nothing in flight on a lane;
      - with the switch off every call is told what lane_decide alone tells it."""
    main = r'''
int main() {
    long long bad = 0, starts = 0, lane_starts = 0, home_starts = 0, drops = 0, rewards_on_lane = 0;
    for (int T = 2; T <= 12; ++T)
      for (int sw = 0; sw < 128; ++sw)
        for (int dev = -1; dev < T; ++dev)
          for (int join_at = -1; join_at < T; ++join_at) {
            Knobs k = knobs();
            k.on = !(sw & 1); k.no_reset_lane = sw & 2; k.no_reward_lane = sw & 4; k.overlap = !(sw & 8); k.room = !(sw & 16);
            k.rows64_8 = !(sw & 32); k.rows64_9 = !(sw & 64);
            Sim s = Sim(), ref = Sim();
            const bool taken = sim_observe(s, k, T);
            { Knobs k0 = k; k0.on = false; (void)sim_observe(ref, k0, T); }
            bool own_next = taken;                       // the stepper's row of act 0 exists only behind a reset forward on a lane
            for (int cur = 0; cur < T; ++cur) {
                k.own_row = own_next && cur != dev;
                const Sim before = s;
                const Told t = sim_step(s, k, cur, T);
                const int n = T - 1 - cur;
                if (t.step == AheadStep::Start) {
                    ++starts;
                    if (!(k.on && k.own_row && (n == 8 || n == 9) && (n == 8 ? k.rows64_8 : k.rows64_9))) ++bad;
                    if (before.a.active) ++bad;
                    if (s.a.c0 != cur || s.a.n != n || s.a.next != cur + 1) ++bad;
                    if (t.lanes) { ++lane_starts; if (!(k.overlap && k.room) || t.p.on != 0 || !s.l.in_flight || s.l.last != 0) ++bad; }
                    else { ++home_starts; if (s.l.in_flight) ++bad; }
                } else if (t.step == AheadStep::Next) {
                    if (!before.a.active || !k.own_row || cur != before.a.next || cur > T - 2) ++bad;
                    if (t.lanes && (t.p.on != 1 || !t.p.wait_act || s.l.last != 1)) ++bad;
                    if (!t.lanes && s.l.in_flight) ++bad;
                } else {
                    if (s.a.active) ++bad;                                   // rows outstanding and a transition of its own: never
                    if (before.a.active && !t.dropped) ++bad;
                    if (t.dropped) { ++drops; if (!t.p.lane && s.l.in_flight) ++bad; }
                    if (t.p.lane && t.p.reward) {
                        ++rewards_on_lane;
                        if (t.p.on != 0 || !t.p.wait_act) ++bad;             // lane 0: behind the group forward in stream order
                    }
                }
                if (s.a.handed + s.a.dropped + (s.a.active ? s.a.c0 + s.a.n - s.a.next : 0) != before.a.handed + before.a.dropped +
                    (before.a.active ? before.a.c0 + before.a.n - before.a.next : 0) + (t.step == AheadStep::Start ? n : 0)) ++bad;
                if (!k.on) {
                    Knobs k0 = k;
                    const Told r = sim_step(ref, k0, cur, T);
                    if (r.step != AheadStep::None || t.step != AheadStep::None || r.p.lane != t.p.lane || r.p.on != t.p.on || r.p.join != t.p.join ||
                        r.p.wait_entry != t.p.wait_entry || r.p.wait_act != t.p.wait_act || r.p.wait_handout != t.p.wait_handout) ++bad;
                }
                own_next = true;                         // every act leaves the next step's logged-action row
                if (cur == join_at) { sim_join(s); if (!k.on) sim_join(ref); if (s.a.active || s.l.in_flight) ++bad; }
            }
            if (s.a.active) ++bad;                       // the last row belongs to act T - 2: nothing is outstanding behind the reward step
            if (s.a.handed + s.a.dropped != 0 && s.a.started == 0) ++bad;
          }
    printf("bad %lld starts %d lane %d home %d drops %d rewards_on_lane %d\n", bad, starts > 0, lane_starts > 0, home_starts > 0, drops > 0,
           rewards_on_lane > 0);
    return bad != 0;
}
'''
    out = _build_and_run(tmp_path, 'ahead_sweep', main)
    assert out[-1] == 'bad 0 starts 1 lane 1 home 1 drops 1 rewards_on_lane 1', out[-1]


def test_plan_of_the_group_forward(tmp_path):
    """DienCall::rows_differ: the per-row category kernel on the active rows and the 64-row AUGRU form, every other stage what a
    reward-shaped forward of 8 / 9 rows per env selects; without the field the plans of tests/test_dien_plan_host.py stand (that
    test builds its calls without it)."""
    cxx = _cxx()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    main = r'''
#include "dien_plan.hpp"
using namespace rl4rs;
static void show(const char* name, const DienTraits& t, const DienCall& c) {
    char buf[512];
    dien_plan_str(dien_plan(t, c), buf, sizeof(buf));
    printf("%s | %s\n", name, buf);
}
int main() {
    DienTraits t{};
    t.fp16x2 = t.gemm16 = t.din16 = t.cat16 = t.augru_x = t.din_x = t.din_rows_auto = t.cat_v2 = t.cat_group = t.dense_chain = t.gemm_group = true;
    t.row_dedup = t.tier2_rows = t.augru_shadow = t.h1f = t.lazy_expand = t.ptab = t.tsum = true;
    t.E = 128; t.U = 128; t.L = 64; t.S = 2; t.Cn = 21; t.Dn = 432; t.Fld = 768; t.NH2 = 256; t.n_cu = 256; t.max_rows = 36864;
    for (int differ = 0; differ < 2; ++differ)
        for (int g = 8; g <= 9; ++g) {
            DienCall c{};
            c.R = 4096 * g; c.group = g; c.carried = true; c.part_groups = 4096; c.dense_vec = true; c.distinct_hint = 1746;
            c.rows_differ = differ != 0;
            show(differ ? (g == 8 ? "ahead g8" : "ahead g9") : (g == 8 ? "shared g8" : "shared g9"), t, c);
        }
    DienCall c{};
    c.R = 64; c.group = 8; c.carried = true; c.part_groups = 8; c.dense_vec = true; c.augru_rows = 64; c.rows_differ = true;
    show("ahead g8 pinned", t, c);
    return 0;
}
'''
    src, exe = tmp_path / 'ahead_plan.cpp', tmp_path / 'ahead_plan'
    src.write_text(main)
    r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Wextra', '-Werror', '-I', CSRC, str(src), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    got = {ln.split(' | ')[0]: dict(tok.split('=', 1) for tok in ln.split(' | ')[1].split()) for ln in out}
    rest = dict(tier2='1', shadow='0', dedup='carried', dense='pair', qside='in_pair', din='k_din_x_16', augru='k_augru_x_64', expand='lazy:768',
                head='tsum+k_gemm_h16', prob='0')
    assert got['shared g8'] == dict(rest, cat='k_cat_attn2g<8,8>')
    assert got['shared g9'] == dict(rest, cat='k_cat_attn2g<9>')
    for name in ('ahead g8', 'ahead g9', 'ahead g8 pinned'):
        assert got[name] == dict(rest, cat='k_cat_attn2<21,true>'), (name, got[name])
