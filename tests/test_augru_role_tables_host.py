"""The per-role step schedule of k_augru_x (RL4RS_X_USPLIT, rl4rs_amd/csrc/augru_x.hpp: role_item / role_stretch / make_sched) replayed
on the CPU.  The tables below are transcribed as data from the constexpr functions; one test compiles the `xk` block of the header
with the host C++ compiler and compares them entry by entry, the others replay the step loop of augru_x_body.inc (boundary stretch,
rotated loop, tail) per role and check what the kernel relies on:
  * per step and role every (gate, k-block) product is issued exactly once - none for step 0 (h = 0) and none for a step past the end;
  * the k-blocks of every accumulator ascend behind its projection read (the operation order that keeps the bits);
  * no item reads a state plane before the barrier that completes it, or after the barrier behind which it is rewritten;
  * a streamed item finds its own weight fragment in its ring slot, at the loop's wrap and behind both boundary stretches, and
    a boundary stretch requests nothing for an item that is skipped."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'rl4rs_amd', 'csrc')
NI = 48
# item -> gate (0 reset, 1 update, 2 candidate) and k-block of the state it multiplies: xk::gate / xk::kb
GATE = [0] * 8 + [1] * 16 + [2] * 16 + [0] * 8
KB = list(range(8, 16)) + list(range(16)) + list(range(16)) + list(range(8))
# sequence position (counted from barrier b) -> item: xk::role_item(false, s) / xk::role_item(true, s)
ORDER_ONE = list(range(48))
ORDER_EARLY = list(range(0, 8)) + list(range(16, 40)) + list(range(40, 48)) + list(range(8, 16))
STRETCH = {False: 40, True: 32}                  # xk::role_stretch: first position behind barrier a
FORMS = [(12, 4), (4, 2)]                        # (NRES, RING) of the 32-row and the 64-row form (recur_args.hpp)
ROLES = ['one', 'early', 'late']                 # one schedule for both roles | the two roles of the split schedule


def order(split):
    return ORDER_EARLY if split else ORDER_ONE


def is_res(nres, i):
    return 40 - nres <= i < 40


def make_sched(nres, split):
    """xk::make_sched: (js_of, item_of) of the streamed sequence that starts behind barrier a"""
    o = order(split)
    k = STRETCH[split]
    while is_res(nres, o[k % NI]):
        k += 1
    js_of, item_of, js = {}, [], 0
    for c in range(NI):
        i = o[(k + c) % NI]
        js_of[i] = js
        if not is_res(nres, i):
            item_of.append(i)
            js += 1
    return js_of, item_of


def replay(role, nres, ring, T):
    """The events of one wave over T steps, in program order (augru_x_body.inc: `items`, `recur`).
    ('bar', which, t) | ('xread', gate, step) | ('mfma', item, step of its accumulator, t) | ('fetch', item, slot) | ('use', item, slot)"""
    se = role == 'early'
    o = order(se)
    sb, tail = STRETCH[se], (40 if se else NI)
    js_of, item_of = make_sched(nres, se)
    ns, la = NI - nres, ring - 1
    ev = []

    def items(t, lo, hi, light):
        for s in range(lo, hi):
            i = o[s]
            if (i == 16 and light) if se else i == 8:
                ev.append(('xread', 1, t))
            if i == 24:
                ev.append(('bar', '1', t))
                ev.append(('xread', 2, t))
            if i == 40:
                ev.append(('bar', 'a', t))
                if not light:
                    ev.append(('xread', 0, t + 1))
                    if se:
                        ev.append(('xread', 1, t + 1))
            if not is_res(nres, i):
                js = js_of[i]
                ahead = item_of[(js + la) % ns]
                skip = light and (i >= 40 or (ahead < 40 if se else i < ahead < 40))
                if not skip:
                    ev.append(('fetch', ahead, (js + la) % ring))
                if not light:
                    ev.append(('use', i, js % ring))
            if not light:
                ev.append(('mfma', i, t + 1 if s >= sb else t, t))

    ev.append(('xread', 0, 0))                                           # x_r(0), in front of step 0
    items(0, 0, sb, True)
    t = 0
    while t + 1 < T:
        items(t, sb, NI, False)
        ev.append(('bar', 'b', t))
        t += 1
        items(t, 0, sb, False)
    items(t, sb, tail, True)
    ev.append(('bar', 'b', t))
    return ev


def test_transcribed_tables_are_the_permutation_the_header_describes():
    assert sorted(ORDER_EARLY) == ORDER_ONE
    assert all(ORDER_EARLY[s] % 2 == s % 2 for s in range(NI))          # the state-fragment double buffer still alternates
    # the early role's [a, b] window: the reset-gate items of the next step, then its update-gate items on k-blocks 0..7
    win = ORDER_EARLY[STRETCH[True]:]
    assert [(GATE[i], KB[i]) for i in win] == [(0, k) for k in range(8)] + [(1, k) for k in range(8)]
    # behind barrier b it keeps the update-gate items on k-blocks 8..15 - the eight items that carry the reset gate, two elements each
    assert [(GATE[i], KB[i]) for i in ORDER_EARLY[8:16]] == [(1, k) for k in range(8, 16)]
    for nres, ring in FORMS:
        assert (NI - nres) % ring == 0
        for split in (False, True):
            js_of, item_of = make_sched(nres, split)
            assert item_of[0] == 40 and len(item_of) == NI - nres
            # the resident set stays items 40 - NRES .. 39, in front of barrier a in both orders
            assert [i for i in order(split) if is_res(nres, i)] == list(range(40 - nres, 40))


@pytest.mark.parametrize('T', [1, 2, 3, 5])
@pytest.mark.parametrize('nres,ring', FORMS)
@pytest.mark.parametrize('role', ROLES)
def test_every_product_once_and_ascending(role, nres, ring, T):
    ev = replay(role, nres, ring, T)
    per_acc = {}
    for e in ev:
        if e[0] == 'xread':
            assert (e[1], e[2]) not in per_acc, 'projection read twice'
            per_acc[(e[1], e[2])] = []
        elif e[0] == 'mfma':
            per_acc[(GATE[e[1]], e[2])].append(KB[e[1]])               # KeyError: a product in front of its accumulator's C-in read
    for (g, step), kbs in per_acc.items():
        if 1 <= step < T:
            assert kbs == list(range(16)), (g, step, kbs)
        else:
            assert kbs == [], (g, step, kbs)                           # step 0: h = 0, light; no step T
    assert all((g, step) in per_acc for g in range(3) for step in range(T))
    # both roles count the same three barriers per step, in the same order
    assert [e[1:] for e in ev if e[0] == 'bar'] == [(w, t) for t in range(T) for w in ('1', 'a', 'b')]


@pytest.mark.parametrize('nres,ring', FORMS)
@pytest.mark.parametrize('role', ROLES)
def test_no_plane_is_read_early_or_late(role, nres, ring):
    """Plane versions: the k-blocks 0..7 of h(t) are written by the early waves in front of barrier a of step t - 1 (behind barrier 1),
    the k-blocks 8..15 by the late waves between barrier a and barrier b of step t - 1; r*h of step t by every wave between barrier b
    of step t - 1 and barrier 1 of step t.  An item may read a plane only between the barrier that completes it and the barrier
    behind which its rewriting starts."""
    T = 5
    ev = replay(role, nres, ring, T)
    pos = {}
    for n, e in enumerate(ev):
        if e[0] == 'bar':
            pos[(e[1], e[2])] = n
    pos[('a', -1)] = pos[('b', -1)] = -1
    for n, e in enumerate(ev):
        if e[0] != 'mfma':
            continue
        i, step = e[1], e[2]
        if 24 <= i < 40:                                                 # candidate: r*h planes of its own step
            ready, gone = pos[('1', step)], pos[('b', step)]
        elif KB[i] < 8:                                                  # early half of h(step)
            ready, gone = pos[('a', step - 1)], pos[('1', step)]
        else:
            ready, gone = pos[('b', step - 1)], pos[('a', step)]
        assert ready < n < gone, (role, i, step)


@pytest.mark.parametrize('T', [1, 2, 3, 5])
@pytest.mark.parametrize('nres,ring', FORMS)
@pytest.mark.parametrize('role', ROLES)
def test_ring_slots_hold_the_item_that_reads_them(role, nres, ring, T):
    ev = replay(role, nres, ring, T)
    slot = [None] * ring
    pending = 0
    for e in ev:
        if e[0] == 'fetch':
            assert slot[e[2]] is None, 'a request lands on a fragment that was not used yet'
            slot[e[2]] = e[1]
            pending += 1
        elif e[0] == 'use':
            assert slot[e[2]] == e[1], (role, T, e)
            slot[e[2]] = None
            pending -= 1
    # what is still in flight at the end was requested by the last stretch in front of the tail for the tail's items 40.. (as in the
    # one-schedule loop); the tail itself and step 0's skipped items request nothing
    assert pending == ring - 1
    first = next((k for k, x in enumerate(ev) if x[0] == 'mfma'), len(ev))
    assert all(e[1] >= 40 for e in ev[:first] if e[0] == 'fetch')
    assert not [e for e in ev[ev.index(('bar', 'a', T - 1)):] if e[0] == 'fetch']


def _cxx():
    return next((c for c in ('g++', 'c++', 'clang++') if shutil.which(c)), None)


def test_tables_match_the_header(tmp_path):
    cxx = _cxx()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    text = open(os.path.join(CSRC, 'augru_x.hpp')).read()
    block = text[text.index('namespace xk {'):text.index('}  // namespace xk')] + '}\n'
    main = ['#include <stdio.h>', '#define RL4RS_X_NRES 12', block, 'using namespace xk;', 'template <int NRES> void dump(bool split) {',
            '    constexpr Sched a = make_sched<NRES>(false), b = make_sched<NRES>(true);', '    const Sched& s = split ? b : a;',
            '    printf("sched %d %d :", NRES, (int)split);', '    for (int i = 0; i < NI; ++i) printf(" %d", s.js_of[i]);', '    printf(" :");',
            '    for (int j = 0; j < NI - NRES; ++j) printf(" %d", s.item_of[j]);', '    printf("\\n");', '}', 'int main() {',
            '    for (int split = 0; split < 2; ++split) {', '        printf("order %d %d :", split, role_stretch(split));',
            '        for (int s = 0; s < NI; ++s) printf(" %d", role_item(split, s));', '        printf("\\n");', '    }',
            '    printf("gate :");', '    for (int i = 0; i < NI; ++i) printf(" %d", gate(i));', '    printf("\\nkb :");',
            '    for (int i = 0; i < NI; ++i) printf(" %d", kb(i));', '    printf("\\nres :");',
            '    for (int i = 0; i < NI; ++i) printf(" %d", (int)is_res<4>(i) + 2 * (int)is_res<12>(i));', '    printf("\\n");',
            '    dump<12>(false); dump<12>(true); dump<4>(false); dump<4>(true);', '    return 0;', '}']
    src, exe = tmp_path / 'tables.cpp', tmp_path / 'tables'
    src.write_text('\n'.join(main) + '\n')
    r = subprocess.run([cxx, '-std=c++17', str(src), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    rows = {}
    for ln in out:
        head, *rest = ln.split(' :')
        rows[head.strip()] = [[int(x) for x in part.split()] for part in rest]
    assert rows['order 0 40'][0] == ORDER_ONE and rows['order 1 32'][0] == ORDER_EARLY
    assert rows['gate'][0] == GATE and rows['kb'][0] == KB
    assert rows['res'][0] == [int(is_res(4, i)) + 2 * int(is_res(12, i)) for i in range(NI)]
    for nres, _ in FORMS:
        for split in (False, True):
            js_of, item_of = make_sched(nres, split)
            got = rows['sched %d %d' % (nres, int(split))]
            assert got[1] == item_of
            assert all(got[0][i] == js_of[i] for i in range(NI) if not is_res(nres, i))
    assert re.search(r'#define RL4RS_X_USPLIT [012]\b', text)
