"""The refinement rule of rl4rs_amd/csrc/row_refine.hpp replayed in numpy: the stepper carries the duplicate-row
partition of the env batch from one forward to the next - an env stays with its representative iff it took the representative's
action, an env that split off looks, earliest first, at the CAP - 1 positions in front of it for an env with the same previous
representative and the same action, chains are followed to their roots and the active list is rebuilt in processing order.

Random small cases (40 - 200 envs drawn from 3 - 8 log lines, one line filling more than a cap's worth of consecutive positions so
that chains occur; a look-back window of 4 and of 64; natural order and the envs sorted by line; 9 steps of random actions).
After every step, for every env g: rep[g] is a root; g and rep[g] have the same line and the same action history (= bitwise equal
rows); `active` lists the roots in processing order; and there are never more roots than a replay of k_row_dedup's own search
(row_dedup.hpp) finds on the rows just built - a carried partition merges at least what the content search merges."""
import numpy as np
import pytest

T = 9


def content_dedup(rows, slots, order, cap):
    """k_row_dedup's search: position p looks, earliest first, at the positions of its run (equal slots, consecutive) among the
    cap - 1 in front of it and takes the first equal row; chains are followed to their root.  -> (rep, active)"""
    n = len(rows)
    rep = np.arange(n)
    for p in range(n):
        g = order[p]
        back = 0
        while back < cap - 1 and p - 1 - back >= 0 and slots[order[p - 1 - back]] == slots[g]:
            back += 1
        for k in range(back, 0, -1):
            g2 = order[p - k]
            if rows[g2] == rows[g]:
                rep[g] = g2
                break
    return _compact(rep, order)


def _compact(rep, order):
    rep = rep.copy()
    for g in order:
        r = rep[g]
        while rep[r] != r:
            r = rep[r]
        rep[g] = r
    active = [g for g in order if rep[g] == g]
    return rep, active


def refine(rep_prev, key, order, cap):
    """row_refine_env + row_refine_finish -> (rep, active, envs that split off)"""
    n = len(rep_prev)
    rep = np.empty(n, dtype=np.int64)
    marked = np.zeros(n, dtype=bool)
    for g in range(n):
        r = rep_prev[g]
        if key[g] == key[r]:
            rep[g] = r
        else:
            marked[g] = True
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n)
    for g in np.nonzero(marked)[0]:
        p = pos[g]
        rep[g] = g
        for d in range(min(cap - 1, p), 0, -1):              # earliest first
            g2 = order[p - d]
            if rep_prev[g2] == rep_prev[g] and key[g2] == key[g]:
                rep[g] = g2
                break
    rep, active = _compact(rep, order)
    return rep, active, int(marked.sum())


def _case(rng, cap):
    n = int(rng.integers(40, 201))
    n_lines = int(rng.integers(3, 9))
    line = rng.integers(0, n_lines, size=n)
    # one line fills more than a cap's worth of consecutive positions (in either order below): chains
    run = min(n - 1, cap + int(rng.integers(2, 2 * cap)))
    start = int(rng.integers(0, n - run))
    line[start:start + run] = 0
    return n, line


@pytest.mark.parametrize('cap', [4, 64])
@pytest.mark.parametrize('ordered', [False, True])
def test_refined_partition_against_content_search(cap, ordered):
    rng = np.random.default_rng(1000 * cap + int(ordered))
    chains = splits_seen = merged_more = 0
    for _ in range(12):
        n, line = _case(rng, cap)
        order = np.argsort(line, kind='stable') if ordered else np.arange(n)
        hist = [() for _ in range(n)]
        rows = [(int(line[g]), hist[g]) for g in range(n)]
        rep, active = content_dedup(rows, line, order, cap)           # the reset observation: found by content
        n_items = int(rng.integers(2, 5))
        logged = rng.integers(0, n_items, size=(int(line.max()) + 1, T))
        p_follow = rng.choice([1.0, 0.9, 0.6])
        for t in range(T):
            # an env plays its line's logged item, or (sometimes) a random one
            key = np.where(rng.random(n) < p_follow, logged[line, t], rng.integers(0, n_items, size=n))
            rep_new, active, n_marked = refine(rep, key, order, cap)
            splits_seen += n_marked
            hist = [hist[g] + (int(key[g]),) for g in range(n)]
            rows = [(int(line[g]), hist[g]) for g in range(n)]
            roots = [g for g in range(n) if rep_new[g] == g]
            for g in range(n):
                r = rep_new[g]
                assert rep_new[r] == r, (t, g)
                assert rows[g] == rows[r], (t, g, r)
            assert list(active) == [g for g in order if rep_new[g] == g]
            assert sorted(active) == roots
            c_rep, c_active = content_dedup(rows, line, order, cap)
            assert len(roots) <= len(c_active), (t, len(roots), len(c_active))
            assert set(roots) <= set(int(g) for g in c_active)        # every root of the carried partition is one of the search
            merged_more += len(roots) < len(c_active)
            rep = rep_new
        # the construction really produced chains at the reset: a group whose first candidate was not a root
        first = np.arange(n)
        for p in range(n):
            g = order[p]
            back = 0
            while back < cap - 1 and p - 1 - back >= 0 and line[order[p - 1 - back]] == line[g]:
                back += 1
            if back:
                first[g] = order[p - back]
        chains += int(sum(1 for g in range(n) if first[g] != g and first[first[g]] != first[g]))
    print('cap', cap, 'ordered', ordered, 'chained groups', chains, 'split-offs', splits_seen, 'steps merged more than the search', merged_more)
    assert splits_seen > 0 and chains > 0
