"""Host replay of the shadow plane of the observation-sized AUGRU launch (augru_xs.hpp) and of the room rule that admits
it (rl4rs_dien_forward).  The grid is (ceil(R / 32), S + 1), sized for R on the host; the workgroups of plane S are the shadow
plane.  Shadow workgroup x takes positions 32 x .. 32 x + 31 of the active list: it leaves before its first barrier when 32 x lies
behind n_active; wave w (of 8) runs the category branch of positions 32 x + 4 w + 0 .. 3 and stops at the first one behind
n_active; then waves 0 - 3 run the dense tower as the 32-row mapped GEMM tile, whose positions behind the bound recompute the last
active row and store nothing."""
import numpy as np
import pytest


def replay_shadow(R, n_active, active):
    """-> (category rows written, dense rows stored, dense rows loaded, shadow workgroups that ran, grid x)"""
    bound = min(R, n_active)
    grid = (R + 31) // 32
    cat_rows, dense_stored, dense_loaded, ran = [], [], [], []
    for x in range(grid):
        p0 = 32 * x
        if p0 >= bound:
            continue                                             # leaves before its first barrier
        ran.append(x)
        for wave in range(8):
            for i in range(4):
                p = p0 + 4 * wave + i
                if p >= bound:
                    break
                cat_rows.append(int(active[p]))
        for r in range(32):                                      # gemm_h16_tile.inc, MAP, WM = 1, group 1
            pos = min(p0 + r, R - 1)
            if pos >= bound:
                pos = bound - 1
            dense_loaded.append(int(active[pos]))
            if p0 + r < bound:
                dense_stored.append(int(active[pos]))
    return cat_rows, dense_stored, dense_loaded, ran, grid


@pytest.mark.parametrize('R', [1, 31, 32, 33, 65, 257])
def test_every_active_row_in_exactly_one_shadow_tile(R):
    rs = np.random.RandomState(R)
    for n_active in sorted(set([1, max(1, R // 2), max(1, R - 1), R, min(R, 33)])):
        for perm in (np.arange(R), rs.permutation(R)):
            active = np.concatenate([perm[:n_active], np.full(R - n_active, -12345)])     # the rest of the list is stale
            cat_rows, stored, loaded, ran, grid = replay_shadow(R, n_active, active)
            want = sorted(int(a) for a in perm[:n_active])
            assert sorted(cat_rows) == want                       # every active row once, by one wave of one workgroup
            assert sorted(stored) == want
            assert all(0 <= r < R for r in cat_rows + stored + loaded)        # no stale entry is ever a row
            assert set(loaded) <= set(want)
            assert ran == list(range((n_active + 31) // 32)) and grid == (R + 31) // 32


def room(hint, R, S, n_cu):
    """rl4rs_dien_forward: the hint counts only where it is below the forward's rows"""
    g = hint if 0 < hint < R else R
    return ((g + 31) // 32) * (S + 1) <= n_cu


def test_room_rule():
    assert room(1771, 4096, 2, 256)                               # the flagship: 56 * 3 = 168 workgroups
    assert not room(0, 4096, 2, 256) and not room(4096, 4096, 2, 256)     # all distinct: 128 * 3
    assert room(0, 2720, 2, 256) and not room(0, 2721, 2, 256)    # 85 tiles fit, 86 do not
    assert room(2720, 2752, 2, 256) and not room(2721, 2752, 2, 256)
    assert room(0, 64, 2, 256) and room(9999, 64, 2, 256)
