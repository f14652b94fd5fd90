"""Host replay of the row map of the scorer's second tier: with the row dedup on, the category kernels, the dense /
q-side GEMMs and the head GEMM work on the active list as k_din_x and k_augru_x do.  Tile position p works on physical row
active[p / group] * group + p % group, the row bound is min(R, n_active * group) read on the device, the grid is sized for R on
the host, a workgroup whose first position lies behind the bound leaves before its first barrier, and the positions of a
partial last tile behind the bound recompute the last active row and store nothing.

Replayed here as the kernels compute it, for the forms used: 4 rows per workgroup (k_cat_attn2: a wave behind the bound simply
leaves, nothing is clamped), one group per workgroup (k_cat_attn2g), 32- and 64-row GEMM tiles (gemm_h16_tile.inc, MAP)."""
import numpy as np
import pytest

GROUPS = (1, 8, 9)


def replay_tile(R, group, n_active, active, tile):
    """GEMM tile of `tile` rows -> list of (workgroup, tile row, physical row loaded, stored?), workgroups that ran."""
    bound = min(R, n_active * group)
    grid = (R + tile - 1) // tile                                # sized for R on the host
    out, ran = [], []
    for wg in range(grid):
        m0 = wg * tile
        if m0 >= bound:
            continue                                             # leaves before its first barrier
        ran.append(wg)
        for r in range(tile):
            pos = min(m0 + r, bound - 1)                         # clamped: recomputes the last active row
            g = pos // group
            out.append((wg, r, int(active[g]) * group + (pos - g * group), m0 + r < bound))
    return out, ran, grid


def replay_cat_rows(R, group, n_active, active):
    """k_cat_attn2: 4 waves per workgroup, one position per wave; a wave behind the bound returns (no barrier in the kernel)."""
    bound = min(R, n_active * group)
    grid = (R + 3) // 4
    out, ran = [], []
    for wg in range(grid):
        for wave in range(4):
            pos = wg * 4 + wave
            if pos >= bound:
                continue
            if wg not in ran:
                ran.append(wg)
            g = pos // group
            out.append((wg, wave, int(active[g]) * group + (pos - g * group), True))
    return out, ran, grid


def replay_cat_groups(R, group, n_active, active):
    """k_cat_attn2g: workgroup p = group active[p], wave w = its row w; workgroups behind n_active leave."""
    grid = R // group
    out, ran = [], []
    for wg in range(grid):
        if wg >= n_active:
            continue
        ran.append(wg)
        for w in range(group):
            out.append((wg, w, int(active[wg]) * group + w, True))
    return out, ran, grid


FORMS = {'cat4': lambda R, g, na, act: replay_cat_rows(R, g, na, act),
         'catg': lambda R, g, na, act: replay_cat_groups(R, g, na, act),
         'gemm32': lambda R, g, na, act: replay_tile(R, g, na, act, 32),
         'gemm64': lambda R, g, na, act: replay_tile(R, g, na, act, 64)}
TILE = {'cat4': 4, 'catg': None, 'gemm32': 32, 'gemm64': 64}


def _n_actives(n_groups, group, tile):
    """1, a count whose n_active * group is no multiple of the tile (4-row workgroups over groups of 8 have none: half the
    groups then), and n_groups"""
    odd = next((n for n in range(n_groups - 1, 0, -1) if tile is None or (n * group) % tile != 0), n_groups // 2)
    return sorted(set([1, odd, n_groups]))


# (k_cat_attn2g is launched for groups of 8 and 9 only)
@pytest.mark.parametrize('form,group', [(f, g) for f in sorted(FORMS) for g in GROUPS if not (f == 'catg' and g == 1)])
def test_every_active_row_once_and_nothing_else(form, group):
    tile = TILE[form]
    n_groups = {1: 80, 8: 24, 9: 15}[group]                      # R = 80 / 192 / 135, the shapes of tests/test_gpu_tier2_active_rows.py
    R = n_groups * group
    rs = np.random.RandomState(group)
    for n_active in _n_actives(n_groups, group, tile):
        if tile is not None and group % tile != 0 and n_active not in (1, n_groups):
            assert (n_active * group) % tile != 0
        for perm in (np.arange(n_groups), rs.permutation(n_groups)):
            active = perm[:n_active]                             # the representatives in processing order; the rest of the list is stale
            rows, ran, grid = FORMS[form](R, group, n_active, np.concatenate([active, np.full(n_groups - n_active, -12345)]))
            want = sorted(int(a) * group + j for a in active for j in range(group))
            stored = sorted(row for (_, _, row, st) in rows if st)
            assert stored == want, (form, group, n_active)       # every active row exactly once, no row of another group
            active_rows = set(want)
            for wg, r, row, st in rows:
                assert row in active_rows                        # also what a clamped position LOADS is an active row
            bound = min(R, n_active * group)
            if tile is not None:
                # clamped positions (behind the bound, inside a tile that runs) recompute the last active row and are not stored
                last = int(active[-1]) * group + group - 1
                for wg, r, row, st in rows:
                    if wg * tile + r >= bound:
                        assert not st and row == last
                assert ran == list(range((bound + tile - 1) // tile))
                assert grid == (R + tile - 1) // tile
            else:
                assert ran == list(range(n_active)) and grid == n_groups
            # the workgroups past the bound did nothing
            assert all(wg in ran for wg, *_ in rows)


def test_group_of_the_partial_tile_shapes():
    """The GPU test's shapes: R = 80, group 1, 35 active rows = one full 32-row tile, one partial tile, one workgroup that leaves;
    group 9, R = 135, 6 active groups = 54 rows: one partial 64-row tile, two workgroups that leave."""
    rows, ran, grid = replay_tile(80, 1, 35, np.arange(80), 32)
    assert grid == 3 and ran == [0, 1] and sum(st for *_, st in rows) == 35
    rows, ran, grid = replay_tile(135, 9, 6, np.arange(15), 64)
    assert grid == 3 and ran == [0] and sum(st for *_, st in rows) == 54
    rows, ran, grid = replay_cat_rows(80, 1, 35, np.arange(80))
    assert grid == 20 and ran == list(range(9)) and len(rows) == 35
