"""Host replay of the 9-rows-per-slot 64-row form of k_augru_x (augru_x.hpp `GRP == 9`): which batch row a tile
position works on, which staged projection row it reads, and which positions store.  A workgroup's tile holds 7 whole groups
(63 positions); position 63 is a clamped position.  Every active row must be stored exactly once, no clamped position may be
stored, and every position must read the staged row that was fetched for its own group."""
import numpy as np
import pytest

GROUP, TILE_GROUPS, TILE_ROWS = 9, 7, 63
COUNTS = (1, 6, 7, 8, 13, 14, 15, 50)


def replay(n_groups, n_active=None, order=None):
    """-> list of (workgroup, tile position, batch row, group, staged row d, staged group, stored?) as the kernel computes them."""
    n_rows_host = n_groups * GROUP
    n_rows = n_rows_host if n_active is None else min(n_rows_host, n_active * GROUP)
    grid = (n_rows_host + TILE_ROWS - 1) // TILE_ROWS            # augru_x_launch: sized for the host's row count

    def phys(p):
        p = min(p, n_rows - 1)
        return (order[p // GROUP] if order is not None else p // GROUP) * GROUP + p % GROUP

    out = []
    for wg in range(grid):
        row0 = wg * TILE_ROWS
        if row0 >= n_rows:
            continue                                             # the workgroup leaves before its first barrier
        staged = [phys(row0 + GROUP * d) // GROUP for d in range(8)]          # lane group d of the one DMA instruction per gate
        for m in range(2):
            for li in range(32):
                r = 32 * m + li
                d = (r * 57) >> 9                                # the kernel's r / 9
                row = phys(row0 + r)
                stored = row0 + r < n_rows and r < TILE_ROWS
                out.append((wg, r, row, row // GROUP, d, staged[d], stored))
    return out


def test_the_multiply_shift_is_the_division():
    assert all(((r * 57) >> 9) == r // 9 for r in range(64))


@pytest.mark.parametrize('n_groups', COUNTS)
def test_every_row_once_and_no_clamped_position_stored(n_groups):
    rs = np.random.RandomState(n_groups)
    orders = [None, rs.permutation(n_groups)]
    for order in orders:
        for n_active in [None] + sorted(set([1, max(1, n_groups // 2), max(1, n_groups - 1), n_groups])):
            rows = replay(n_groups, n_active, order)
            act = n_groups if n_active is None else n_active
            ord_ = np.arange(n_groups) if order is None else order
            want = sorted(int(ord_[p]) * GROUP + j for p in range(act) for j in range(GROUP))
            stored = sorted(row for (_, r, row, _, _, _, st) in rows if st)
            assert stored == want, (n_groups, n_active)
            for wg, r, row, grp, d, staged_grp, st in rows:
                assert 0 <= row < n_groups * GROUP
                assert staged_grp == grp, (wg, r)                # reads the projections of its own group's cache slot
                if r >= TILE_ROWS:
                    assert not st                                # the clamped position of every tile
            # workgroups: ceil(active groups / 7), the rest leave
            assert len(set(w for w, *_ in rows)) == (act + TILE_GROUPS - 1) // TILE_GROUPS


def test_tile_edges_of_the_listed_counts():
    """7 and 14 groups fill their tiles exactly; 8 and 15 leave one group in a last tile; 50 = 7 full tiles + 1 group."""
    for n, tiles, last in ((1, 1, 1), (6, 1, 6), (7, 1, 7), (8, 2, 1), (13, 2, 6), (14, 2, 7), (15, 3, 1), (50, 8, 1)):
        rows = replay(n)
        wgs = sorted(set(w for w, *_ in rows))
        assert len(wgs) == tiles
        assert sum(1 for (w, *_, st) in rows if w == wgs[-1] and st) == last * GROUP
