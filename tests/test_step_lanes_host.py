"""The lane rule of the stepper (rl4rs_amd/csrc/step_lanes.hpp) on the CPU: the header is compiled with the host C++
compiler alone (as tests/test_dien_plan_host.py does for the launch plan) into a program that replays call sequences through
lane_decide / lane_join and prints what every call was told: lane or caller's stream, which lane, join, and the three waits.  The
expected lines are written out by hand from the rules of DESIGN 38:

  eligible  = switch on, DIEN on k_augru_x, partition carried, no reward due, no mask / done output,
              2 * seq_num * ceil(distinct / 32) <= n_cu
  lane      = lanes alternate, from one lane transition to the next
  wait_act  = a lane transition is in flight (k - 1 ran on the other lane)
  wait_entry = the action is not the stepper's own row, or nothing is in flight (the first lane transition behind a join)
  wait_handout = the lane was used since the last join and the entry event is not waited for anyway
  join      = a call that is not eligible, while something is in flight"""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'rl4rs_amd', 'csrc')

# a call: dict of the LaneCall fields that differ from an eligible own-row call of the flagship (S 2, hint 1746, 256 CUs); 'join' = an
# entry point that only joins (reset, rl4rs_dien_buffer, ...)
OK = dict(overlap=1, dien_x=1, carried=1, reward_due=0, extra_outputs=0, own_row=1, seq_num=2, distinct_hint=1746, n_cu=256)


def c(**kw):
    d = dict(OK)
    d.update(kw)
    return d


def L(on, entry=0, act=1, handout=1):
    return 'lane on=%d join=0 entry=%d act=%d handout=%d' % (on, entry, act, handout)


def S(join):
    return 'serial on=0 join=%d entry=0 act=0 handout=0' % join


FOREIGN = c(own_row=0)
REWARD = c(reward_due=1)
SEQUENCES = [
    # reset (a join, nothing in flight), 8 observation transitions (step 0 takes the k_offline_action tensor: foreign), the reward step
    ('reset then 9 steps', ['join', FOREIGN] + [c()] * 7 + [REWARD, 'join'],
     ['joined 0', L(0, entry=1, act=0, handout=0), L(1, handout=0), L(0), L(1), L(0), L(1), L(0), L(1), S(1), 'joined 0']),
    # two episodes back to back: the lanes go on alternating, the first transition behind the join waits for the entry event
    ('second episode', ['join', FOREIGN] + [c()] * 7 + [REWARD, 'join', FOREIGN, c(), c()],
     ['joined 0', L(0, entry=1, act=0, handout=0), L(1, handout=0), L(0), L(1), L(0), L(1), L(0), L(1), S(1), 'joined 0',
      L(0, entry=1, act=0, handout=0), L(1, handout=0), L(0)]),
    # a foreign action at step 3: that transition waits for the caller's stream (and still for the act before it), the rest run ahead
    ('foreign action at step 3', ['join', FOREIGN, c(), c(), FOREIGN, c(), c()],
     ['joined 0', L(0, entry=1, act=0, handout=0), L(1, handout=0), L(0), L(1, entry=1, handout=0), L(0), L(1)]),
    # own row without anything in flight (the caller's stream may hold work the lane has not seen): entry
    ('own row behind a join', ['join', c(), c()], ['joined 0', L(0, entry=1, act=0, handout=0), L(1, handout=0)]),
    # SeqSlate page turn (plan_refine false at the first act of a page): joins, the transitions behind it start over with the entry event
    ('page turn', [c(), c(), c(carried=0), c(), c()],
     [L(0, entry=1, act=0, handout=0), L(1, handout=0), S(1), L(0, entry=1, act=0, handout=0), L(1, handout=0)]),
    # a reward step with nothing in flight joins nothing
    ('reward step alone', [REWARD, REWARD], [S(0), S(0)]),
    # mask or done output, simnet / fp32 scorer
    ('extra outputs', [c(), c(extra_outputs=1), c()], [L(0, entry=1, act=0, handout=0), S(1), L(1, entry=1, act=0, handout=0)]),
    ('other scorer', [c(dien_x=0), c(dien_x=0)], [S(0), S(0)]),
    # the room rule: 2 * S * ceil(n / 32) against n_cu - just under (252), at it (256), over it (260), the all-distinct workload (512)
    ('room under', [c(distinct_hint=2016), c(distinct_hint=2016)], [L(0, entry=1, act=0, handout=0), L(1, handout=0)]),
    ('room at', [c(distinct_hint=2048), c(distinct_hint=2048)], [L(0, entry=1, act=0, handout=0), L(1, handout=0)]),
    ('room over', [c(distinct_hint=2049), c(distinct_hint=2049)], [S(0), S(0)]),
    ('room all distinct', [c(distinct_hint=4096), c(distinct_hint=4096)], [S(0), S(0)]),
    ('room small chip', [c(distinct_hint=96, n_cu=12), c(distinct_hint=97, n_cu=12)], [L(0, entry=1, act=0, handout=0), S(1)]),
    # the hint changes in mid-flight (SeqSlate gives every env its own slot from the second page on): the call joins
    ('hint grows', [c(), c(), c(distinct_hint=4096)], [L(0, entry=1, act=0, handout=0), L(1, handout=0), S(1)]),
    # the switch off: every call on the caller's stream, nothing to join
    ('switch off', ['join'] + [c(overlap=0)] * 8 + [c(overlap=0, reward_due=1)], ['joined 0'] + [S(0)] * 9),
    # the switch turned off in mid-flight joins once
    ('switch off in flight', [c(), c(), c(overlap=0), c(overlap=0)], [L(0, entry=1, act=0, handout=0), L(1, handout=0), S(1), S(0)]),
    # an entry point that only joins, in mid-flight
    ('join in flight', [c(), c(), 'join', c()], [L(0, entry=1, act=0, handout=0), L(1, handout=0), 'joined 1', L(0, entry=1, act=0, handout=0)]),
]
# lane transitions per lane and joins the state has counted at the end of each sequence
STATS = {'reset then 9 steps': (4, 4, 1), 'second episode': (6, 5, 1), 'switch off': (0, 0, 0), 'join in flight': (2, 1, 1),
         'page turn': (2, 2, 1), 'foreign action at step 3': (3, 3, 0)}
WORKGROUPS = [((2, 1746), 220), ((2, 4096), 512), ((2, 32), 4), ((2, 33), 8), ((1, 1), 2), ((4, 2048), 512)]


def _cxx():
    return next((x for x in ('g++', 'c++', 'clang++') if shutil.which(x)), None)


def _program():
    body = []
    for name, calls, _ in SEQUENCES:
        body.append('    { LaneState s = LaneState(); printf("seq %s\\n");' % name)
        for call in calls:
            if call == 'join':
                body.append('      printf("joined %d\\n", (int)lane_join(s));')
            else:
                body.append('      { LaneCall x = LaneCall(); %s show(lane_decide(s, x)); }' % ' '.join('x.%s = %d;' % kv for kv in call.items()))
        body.append('      printf("stats %lld %lld %lld\\n", (long long)s.ran[0], (long long)s.ran[1], (long long)s.joins); }')
    for args, _ in WORKGROUPS:
        body.append('    printf("wgs %%lld\\n", (long long)lane_pair_workgroups(%d, %d));' % args)
    return ('#include <stdio.h>\n#include "step_lanes.hpp"\nusing namespace rl4rs;\n'
            'static void show(const LanePlan& p) {\n'
            '    printf("%s on=%d join=%d entry=%d act=%d handout=%d\\n", p.lane ? "lane" : "serial", p.on, (int)p.join, (int)p.wait_entry,\n'
            '           (int)p.wait_act, (int)p.wait_handout);\n}\n'
            'int main() {\n' + '\n'.join(body) + '\n    return 0;\n}\n')


def test_lane_sequences(tmp_path):
    cxx = _cxx()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    src, exe = tmp_path / 'lanes_main.cpp', tmp_path / 'lanes_main'
    src.write_text(_program())
    base = [cxx, '-std=c++17', '-Wall', '-Wextra', '-Werror', '-I', CSRC, str(src), '-o', str(exe)]
    # a stand-alone program of plain C++: built with the address and undefined-behaviour checks where the toolchain has their runtimes
    r = subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    out = run.stdout.splitlines()
    got, name = {}, None
    for ln in out:
        if ln.startswith('seq '):
            name = ln[4:]
            got[name] = []
        elif not ln.startswith('wgs '):
            got[name].append(ln)
    assert list(got) == [s[0] for s in SEQUENCES]
    wrong = []
    for name, calls, want in SEQUENCES:
        lines, stats = got[name][:-1], tuple(int(v) for v in got[name][-1].split()[1:])
        assert len(want) == len(calls)
        if lines != want:
            wrong.append((name, [(i, g, w) for i, (g, w) in enumerate(zip(lines, want)) if g != w], len(lines), len(want)))
        if name in STATS and stats != STATS[name]:
            wrong.append((name, 'stats', stats, STATS[name]))
    assert not wrong, wrong
    assert [int(ln.split()[1]) for ln in out if ln.startswith('wgs ')] == [w for _, w in WORKGROUPS]


# ---- who tells whom when a handle or the stepper goes first (LaneHook / LaneLinks): heap objects freed in every order, under the
# address sanitizer where the toolchain has it - a pointer kept into a freed handle is a use-after-free the run reports
LINKS_MAIN = r'''
#include <stdio.h>
#include "step_lanes.hpp"
using namespace rl4rs;
struct Handle { const LaneHook* lanes; };
struct Stepper { LaneHook hook; LaneLinks links; int joined, told[2]; };
static int s_join(void* c, void*, int) { static_cast<Stepper*>(c)->joined++; return 0; }
static void s_gone(void* c, int w) { Stepper* s = static_cast<Stepper*>(c); lane_links_gone(s->links, w); s->told[w]++; }
static Stepper* attach(Handle* env, Handle* scorer) {                 // what step.hip's attach does
    Stepper* s = new Stepper();
    s->hook.ctx = s; s->hook.join = s_join; s->hook.gone = s_gone;
    lane_links_attach(s->links, LANE_LINK_ENV, &env->lanes, &s->hook);
    if (scorer) lane_links_attach(s->links, LANE_LINK_SCORER, &scorer->lanes, &s->hook);
    return s;
}
static void destroy(Handle* h, int which) {                           // rl4rs_env_destroy / rl4rs_dien_destroy
    (void)lanes_join(h->lanes, nullptr, false);
    lanes_gone(h->lanes, which);
    delete h;
}
static void destroy(Stepper* s) {                                     // rl4rs_stepper_destroy
    lane_links_release(s->links, &s->hook);
    delete s;
}
static void show(const char* what, const Stepper* s) {
    printf("%s mine=%d%d joined=%d told=%d%d\n", what, (int)lane_links_mine(s->links, 0, &s->hook), (int)lane_links_mine(s->links, 1, &s->hook),
           s->joined, s->told[0], s->told[1]);
}
int main() {
    {   // the scorer is closed first (new weights installed), the stepper lives on (a logged-action tensor holds it), then goes
        Handle* env = new Handle(); Handle* sc = new Handle();
        Stepper* s = attach(env, sc);
        show("A attached", s);
        destroy(sc, LANE_LINK_SCORER);
        show("A scorer gone", s);
        destroy(s);
        printf("A env hook %d\n", env->lanes != nullptr);
        destroy(env, LANE_LINK_ENV);
    }
    {   // the stepper goes first: both handles forget it and call nothing afterwards
        Handle* env = new Handle(); Handle* sc = new Handle();
        Stepper* s = attach(env, sc);
        destroy(s);
        printf("B hooks %d %d\n", env->lanes != nullptr, sc->lanes != nullptr);
        destroy(sc, LANE_LINK_SCORER); destroy(env, LANE_LINK_ENV);
    }
    {   // a second stepper takes the env over with a new scorer; the old scorer, the old stepper, the env and the new ones go in turn
        Handle* env = new Handle(); Handle* sc1 = new Handle(); Handle* sc2 = new Handle();
        Stepper* s1 = attach(env, sc1);
        Stepper* s2 = attach(env, sc2);
        show("C old", s1); show("C new", s2);
        destroy(sc1, LANE_LINK_SCORER);
        show("C old, scorer gone", s1);
        destroy(s1);
        printf("C env hook is new %d\n", env->lanes == &s2->hook);
        destroy(env, LANE_LINK_ENV);
        show("C new, env gone", s2);
        destroy(s2);
        printf("C scorer hook %d\n", sc2->lanes != nullptr);
        destroy(sc2, LANE_LINK_SCORER);
    }
    {   // the env first, then the stepper, then the scorer; a stepper without a DIEN (simnet scorer) has one link only
        Handle* env = new Handle(); Handle* sc = new Handle();
        Stepper* s = attach(env, sc);
        destroy(env, LANE_LINK_ENV);
        show("D env gone", s);
        destroy(s);
        printf("D scorer hook %d\n", sc->lanes != nullptr);
        destroy(sc, LANE_LINK_SCORER);
        Handle* env2 = new Handle();
        Stepper* s3 = attach(env2, nullptr);
        show("D simnet", s3);
        destroy(env2, LANE_LINK_ENV);
        destroy(s3);
    }
    {   // lane_undo: a transition that could not be enqueued leaves the state of before
        LaneState st = LaneState();
        LaneCall c = LaneCall();
        c.overlap = c.dien_x = c.carried = c.own_row = true; c.seq_num = 2; c.distinct_hint = 64; c.n_cu = 256;
        (void)lane_decide(st, c);
        const LaneState before = st;
        const LanePlan p = lane_decide(st, c);
        lane_undo(st, before);
        const LanePlan q = lane_decide(st, c);
        printf("E undo on=%d%d ran=%lld%lld act=%d%d\n", p.on, q.on, (long long)st.ran[0], (long long)st.ran[1], (int)p.wait_act, (int)q.wait_act);
    }
    return 0;
}
'''
LINKS_WANT = [
    'A attached mine=11 joined=0 told=00',
    'A scorer gone mine=10 joined=1 told=01',
    'A env hook 0',
    'B hooks 0 0',
    'C old mine=01 joined=1 told=10',
    'C new mine=11 joined=0 told=00',
    'C old, scorer gone mine=00 joined=2 told=11',
    'C env hook is new 1',
    'C new, env gone mine=01 joined=1 told=10',
    'C scorer hook 0',
    'D env gone mine=01 joined=1 told=10',
    'D scorer hook 0',
    'D simnet mine=10 joined=0 told=00',
    'E undo on=11 ran=11 act=11',
]


def test_links_in_every_destroy_order(tmp_path):
    cxx = _cxx()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    src, exe = tmp_path / 'links_main.cpp', tmp_path / 'links_main'
    src.write_text(LINKS_MAIN)
    base = [cxx, '-std=c++17', '-Wall', '-Wextra', '-Werror', '-g', '-I', CSRC, str(src), '-o', str(exe)]
    r = subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert run.stdout.splitlines() == LINKS_WANT
