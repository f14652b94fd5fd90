"""The two ends of an episode on the stepper's lanes (rl4rs_amd/csrc/step_lanes.hpp) on the CPU: the header is compiled
with the host C++ compiler alone into a stand-alone program (address and undefined-behaviour checks where the toolchain has their
runtimes, as tests/test_step_lanes_host.py) that replays call sequences through lane_decide / lane_join and prints what every call
was told.  The expected lines are written out by hand from the rules:

  observe   = the reset's forward: switch on, DIEN on k_augru_x, room rule, no_reset_lane clear -> a lane, entry event, no act wait
  reward    = a reward is due, the reward step folds, no_reward_lane clear, the partition is carried, room rule, AND a transition is in
              flight whose last one ran on lane 1 -> lane 0 (the scorer's set 0), waits for `act_done` (own row) - else it joins
  first lane = where nothing is in flight and the calls up to the reward step are known (to_reward), the lane that puts the last
              of them on lane 1; with to_reward = 0 the lanes go on alternating from where they were (DESIGN 38's behaviour)

Every call sequence of tests/test_step_lanes_host.py built its way - the new fields left at zero - must give that file's lines."""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'rl4rs_amd', 'csrc')

OK = dict(overlap=1, dien_x=1, carried=1, reward_due=0, extra_outputs=0, own_row=1, seq_num=2, distinct_hint=1746, n_cu=256)


def c(**kw):
    d = dict(OK)
    d.update(kw)
    return d


def obs(T=9, **kw):
    """rl4rs_stepper_observe at cur_steps 0 of a horizon of T acts: the reset and T - 1 observation transitions up to the reward step"""
    return c(observe=1, carried=0, own_row=0, to_reward=T, **kw)


def step(cur, T=9, **kw):
    return c(to_reward=T - 1 - cur, **kw)


def reward(**kw):
    return c(reward_due=1, reward_fold=1, **kw)


def L(on, entry=0, act=1, handout=1, kind='step', join=0):
    return 'lane on=%d join=%d entry=%d act=%d handout=%d kind=%s' % (on, join, entry, act, handout, kind)


def S(join):
    return 'serial on=0 join=%d entry=0 act=0 handout=0 kind=step' % join


def episode(T=9, first=1, **kw):
    """the lines of reset + T - 1 own-row transitions, the lanes alternating from `first`"""
    out = [L(first, entry=1, act=0, handout=0, kind='observe')]
    for k in range(T - 1):
        lane = first ^ ((k + 1) & 1)
        out.append(L(lane, handout=1 if k >= 1 else 0))
    return out


FLAG = [obs()] + [step(k) for k in range(8)] + [reward()]
SEQUENCES = [
    # the flagship: reset on lane 1, t1..t8 alternating from lane 0, the reward step on lane 0 behind `act_done` alone (its own
    # lane was used by t7: it waits for that hand-out)
    ('flagship episode', ['join'] + FLAG,
     ['joined 0'] + episode() + [L(0, kind='reward')]),
    # the next episode's load joins what the reward step left in flight; the same lanes again
    ('two episodes', ['join'] + FLAG + ['join'] + FLAG,
     ['joined 0'] + episode() + [L(0, kind='reward'), 'joined 1'] + episode() + [L(0, kind='reward')]),
    # a horizon of the other parity: the reset starts on lane 0, so that the last transition is again on lane 1
    ('horizon 10', ['join', obs(T=10)] + [step(k, T=10) for k in range(9)] + [reward()],
     ['joined 0'] + episode(T=10, first=0) + [L(0, kind='reward')]),
    # a join in mid-episode (rl4rs_dien_buffer behind t3): the transitions behind it start from the lane their number to the reward
    # step asks for, and the reward step lands on lane 0 beside lane 1
    ('join in mid-episode', [obs(), step(0), step(1), step(2), 'join'] + [step(k) for k in range(3, 8)] + [reward()],
     [L(1, entry=1, act=0, handout=0, kind='observe'), L(0, handout=0), L(1), L(0), 'joined 1',
      L(1, entry=1, act=0, handout=0), L(0, handout=0), L(1), L(0), L(1), L(0, kind='reward')]),
    # an unknown horizon (to_reward 0) and a join that flips the parity: the last transition is on lane 0, whose forward holds the
    # first scratch set - the reward step joins
    ('parity flipped, horizon unknown', [c(), c(), 'join', c(), reward()],
     [L(0, entry=1, act=0, handout=0), L(1, handout=0), 'joined 1', L(0, entry=1, act=0, handout=0), S(1)]),
    ('parity kept, horizon unknown', [c(), c(), reward()], [L(0, entry=1, act=0, handout=0), L(1, handout=0), L(0, kind='reward')]),
    # a reward step without the fold (a small batch without the pinned 64-row form, all-distinct, no_reward_obs_fold): it joins
    ('reward without fold', [obs()] + [step(k) for k in range(8)] + [c(reward_due=1)], episode() + [S(1)]),
    # nothing in flight in front of the reward step: the caller's stream, as before
    ('reward alone', [reward(), reward()], [S(0), S(0)]),
    # a foreign action at the reward step: lane 0, behind the caller's stream
    ('foreign action at the reward step', [obs()] + [step(k) for k in range(8)] + [reward(own_row=0)],
     episode() + [L(0, entry=1, handout=0, kind='reward')]),
    # each switch off alone
    ('no_reset_lane', ['join', obs(no_reset_lane=1), c(own_row=0, to_reward=8)] + [step(k) for k in range(1, 8)] + [reward()],
     ['joined 0', S(0), L(0, entry=1, act=0, handout=0), L(1, handout=0), L(0), L(1), L(0), L(1), L(0), L(1), L(0, kind='reward')]),
    ('no_reward_lane', [obs()] + [step(k) for k in range(8)] + [reward(no_reward_lane=1)], episode() + [S(1)]),
    ('no_step_overlap', [obs(overlap=0)] + [step(k, overlap=0) for k in range(8)] + [reward(overlap=0)], [S(0)] * 10),
    # mask / done outputs, another scorer, no room (all-distinct): the reset and the reward step stay where they were
    ('no room', [obs(distinct_hint=4096)] + [step(k, distinct_hint=4096) for k in range(8)] + [reward(distinct_hint=4096)], [S(0)] * 10),
    ('other scorer', [obs(dien_x=0), step(0, dien_x=0), reward(dien_x=0)], [S(0)] * 3),
    ('reward with extra outputs', [obs()] + [step(k) for k in range(8)] + [reward(extra_outputs=1)], episode() + [S(1)]),
    # SeqSlate, page_items 9: the reward step of the first page on lane 0, the page turn behind it joins (no carried partition), the
    # seven transitions of the second page start on lane 1 and end on lane 1
    ('seqslate two pages', [obs()] + [step(k) for k in range(8)] + [reward(), c(carried=0)] + [step(k, T=8) for k in range(7)] + [reward()],
     episode() + [L(0, kind='reward'), S(1), L(1, entry=1, act=0, handout=0), L(0, handout=0), L(1), L(0), L(1), L(0), L(1),
                  L(0, kind='reward')]),
    # a reset while a reset forward and a transition are in flight (env.reset() in mid-episode: the load joins; observe joins whatever is left)
    ('observe in flight', [obs(), step(0), obs()], [L(1, entry=1, act=0, handout=0, kind='observe'), L(0, handout=0),
                                                    L(1, entry=1, act=0, handout=0, kind='observe', join=1)]),
]
# (ran[0], ran[1], joins, reset forwards on a lane, reward steps on a lane): ran[] counts observation step transitions only
STATS = {'flagship episode': (4, 4, 0, 1, 1), 'two episodes': (8, 8, 1, 2, 2), 'horizon 10': (4, 5, 0, 1, 1),
         'join in mid-episode': (4, 4, 1, 1, 1), 'reward without fold': (4, 4, 1, 1, 0), 'no_reset_lane': (4, 4, 0, 0, 1),
         'no_reward_lane': (4, 4, 1, 1, 0), 'no_step_overlap': (0, 0, 0, 0, 0), 'no room': (0, 0, 0, 0, 0),
         'seqslate two pages': (4 + 3, 4 + 4, 1, 1, 2), 'observe in flight': (1, 0, 1, 2, 0)}

# tests/test_step_lanes_host.py's sequences, built its way (LaneCall() with its nine fields set, nothing else): its lines, without the kind
OLD = [
    ('old: reset then 9 steps', ['join', c(own_row=0)] + [c()] * 7 + [c(reward_due=1), 'join'],
     ['joined 0', L(0, entry=1, act=0, handout=0), L(1, handout=0), L(0), L(1), L(0), L(1), L(0), L(1), S(1), 'joined 0'], (4, 4, 1, 0, 0)),
    ('old: page turn', [c(), c(), c(carried=0), c(), c()],
     [L(0, entry=1, act=0, handout=0), L(1, handout=0), S(1), L(0, entry=1, act=0, handout=0), L(1, handout=0)], (2, 2, 1, 0, 0)),
    ('old: join in flight', [c(), c(), 'join', c()],
     [L(0, entry=1, act=0, handout=0), L(1, handout=0), 'joined 1', L(0, entry=1, act=0, handout=0)], (2, 1, 1, 0, 0)),
    ('old: extra outputs', [c(), c(extra_outputs=1), c()], [L(0, entry=1, act=0, handout=0), S(1), L(1, entry=1, act=0, handout=0)],
     (1, 1, 1, 0, 0)),
    ('old: room over', [c(distinct_hint=2049), c(distinct_hint=2049)], [S(0), S(0)], (0, 0, 0, 0, 0)),
]


def _cxx():
    return next((x for x in ('g++', 'c++', 'clang++') if shutil.which(x)), None)


def _program(seqs):
    body = []
    for name, calls in seqs:
        body.append('    { LaneState s = LaneState(); printf("seq %s\\n");' % name)
        for call in calls:
            if call == 'join':
                body.append('      printf("joined %d\\n", (int)lane_join(s));')
            else:
                body.append('      { LaneCall x = LaneCall(); %s show(lane_decide(s, x)); }' % ' '.join('x.%s = %d;' % kv for kv in call.items()))
        body.append('      printf("stats %lld %lld %lld %lld %lld\\n", (long long)s.ran[0], (long long)s.ran[1], (long long)s.joins,'
                    ' (long long)s.ran_reset, (long long)s.ran_reward); }')
    return ('#include <stdio.h>\n#include "step_lanes.hpp"\nusing namespace rl4rs;\n'
            'static void show(const LanePlan& p) {\n'
            '    printf("%s on=%d join=%d entry=%d act=%d handout=%d kind=%s\\n", p.lane ? "lane" : "serial", p.on, (int)p.join, (int)p.wait_entry,\n'
            '           (int)p.wait_act, (int)p.wait_handout, p.observe ? "observe" : p.reward ? "reward" : "step");\n}\n'
            'int main() {\n' + '\n'.join(body) + '\n'
            '    printf("first %d %d %d %d\\n", lane_first(9), lane_first(8), lane_first(1), lane_first(10));\n'
            '    return 0;\n}\n')


def test_episode_sequences(tmp_path):
    cxx = _cxx()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    seqs = [(n, calls, want, STATS.get(n)) for n, calls, want in SEQUENCES] + OLD
    src, exe = tmp_path / 'episode_main.cpp', tmp_path / 'episode_main'
    src.write_text(_program([(s[0], s[1]) for s in seqs]))
    base = [cxx, '-std=c++17', '-Wall', '-Wextra', '-Werror', '-I', CSRC, str(src), '-o', str(exe)]
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
        elif not ln.startswith('first '):
            got[name].append(ln)
    assert list(got) == [s[0] for s in seqs]
    wrong = []
    for name, calls, want, stats_want in seqs:
        lines, stats = got[name][:-1], tuple(int(v) for v in got[name][-1].split()[1:])
        assert len(want) == len(calls), name
        if lines != want:
            wrong.append((name, [(i, g, w) for i, (g, w) in enumerate(zip(lines, want)) if g != w], len(lines), len(want)))
        if stats_want is not None and stats != stats_want:
            wrong.append((name, 'stats', stats, stats_want))
    assert not wrong, wrong
    # flagship: 9 lane transitions up to the reward step start on lane 1; 8 (no reset lane) on lane 0: the first step stays on lane 0
    assert out[-1] == 'first 1 0 1 0'


def test_reward_never_on_set_1_beside_set_0(tmp_path):
    """Every way to reach a reward step through joins at any point and either horizon parity, with and without the horizon known:
    the program checks after every call that a reward step placed on a lane is on lane 0 and that the transition last issued
    before it ran on lane 1; anything else must have joined."""
    cxx = _cxx()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    main = r'''
#include <stdio.h>
#include "step_lanes.hpp"
using namespace rl4rs;
static LaneCall base() {
    LaneCall c = LaneCall();
    c.overlap = c.dien_x = c.carried = c.own_row = true; c.seq_num = 2; c.distinct_hint = 1746; c.n_cu = 256;
    return c;
}
int main() {
    int lanes = 0, joined = 0, bad = 0;
    for (int T = 2; T <= 12; ++T)
        for (int known = 0; known < 2; ++known)
            for (int with_reset = 0; with_reset < 2; ++with_reset)
                for (int join_at = -1; join_at < T; ++join_at)
                    for (int join2 = join_at; join2 < T; ++join2) {
                        LaneState s = LaneState();
                        if (with_reset) {
                            LaneCall c = base(); c.observe = true; c.carried = false; c.to_reward = known ? T : 0;
                            (void)lane_decide(s, c);
                        }
                        for (int cur = 0; cur < T - 1; ++cur) {
                            if (cur == join_at || cur == join2) (void)lane_join(s);
                            LaneCall c = base(); c.to_reward = known ? T - 1 - cur : 0;
                            const LanePlan p = lane_decide(s, c);
                            if (!p.lane) ++bad;
                        }
                        if (join_at == T - 1 || join2 == T - 1) (void)lane_join(s);
                        const LaneState before = s;
                        LaneCall c = base(); c.reward_due = c.reward_fold = true;
                        const LanePlan p = lane_decide(s, c);
                        if (p.lane) {
                            ++lanes;
                            if (p.on != 0 || !p.reward || !before.in_flight || before.last != 1 || !p.wait_act) ++bad;
                        } else {
                            ++joined;
                            if (s.in_flight) ++bad;
                            // a known horizon never loses the lane to parity: it joins only where nothing was in flight
                            if (known && before.in_flight) ++bad;
                        }
                    }
    printf("lanes %d joined %d bad %d\n", lanes > 0, joined > 0, bad);
    return bad != 0;
}
'''
    src, exe = tmp_path / 'parity_main.cpp', tmp_path / 'parity_main'
    src.write_text(main)
    base = [cxx, '-std=c++17', '-Wall', '-Wextra', '-Werror', '-I', CSRC, str(src), '-o', str(exe)]
    r = subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout, run.stderr)
    assert run.stdout.strip() == 'lanes 1 joined 1 bad 0'
