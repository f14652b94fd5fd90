"""The store address map of k_gru_h16r (rl4rs_amd/csrc/gru_frag_map.hpp) replayed on the CPU: the header is compiled with the host C++
compiler, its tables are dumped, and numpy plays the u role's stores of every step (and the zero-tail stores of the prologue) against
the buffer descriptors the kernel builds over the valid rows of a 32-row tile:
  * every (slot, t < L, e) of the h1 cache is written exactly once;
  * every (slot, t < L, e) lands exactly once at the address k_h1_frag's formula gives (din_x.hpp), the steps L .. 32 NT - 1 of the last
    step tile are written (zeros) exactly once, and nothing else;
  * nothing is written outside the encode's slots: a piece of a row past cnt has an offset at or beyond the descriptor's size (the
    hardware drops it), every other piece lies inside;
  * the (row, column) part and the step part of an offset add up to the whole (the kernel keeps them in a VGPR and an SGPR)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'rl4rs_amd', 'csrc')

MAIN = r'''
#include <stdio.h>
#include "gru_frag_map.hpp"
using namespace gfm;
int main(int argc, char** argv) {
    const int Ls[3] = {1, 33, 64};
    for (int L : Ls) {
        const int NT = (L + 31) / 32;
        for (int row = 0; row < 32; ++row)
            for (int c4 = 0; c4 < 32; ++c4)
                for (int t = 0; t < L; ++t) {
                    if (h1_off(row, t, c4, L) != h1_lane(row, c4, L) + h1_step(t, L)) return 2;
                    if (h1f_off(row, t, c4, NT) != h1f_lane(row, c4, NT) + h1f_step(t, NT)) return 3;
                    if (h1_off(row, t, c4, L) != h1_off(0, t, c4, L) + h1_lane(row, 0, L)) return 4;        // the prefix copy's split
                    if (h1f_off(row, t, c4, NT) != h1f_off(0, t, c4, NT) + h1f_lane(row, 0, NT)) return 5;
                }
        printf("L %d %d %d %d\n", L, NT, THREADS, PIECES);
        for (int j = 0; j < THREADS; ++j)
            for (int i = 0; i < PIECES; ++i)
                printf("p %d %d %d %d\n", piece_row(j, i), piece_c4(j, i), h1_lane(piece_row(j, i), piece_c4(j, i), L),
                       h1f_lane(piece_row(j, i), piece_c4(j, i), NT));
        for (int t = 0; t < L; ++t) printf("s %d %d\n", h1_step(t, L), h1f_step(t, NT));
        for (int z = 0; z < (32 * NT - L) * 1024; ++z) printf("z %d\n", h1f_off(tail_row(z), tail_t(z, L), tail_c4(z), NT));
    }
    return 0;
}
'''


@pytest.fixture(scope='module')
def tables(tmp_path_factory):
    cxx = next((c for c in ('g++', 'c++', 'clang++') if shutil.which(c)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('gfm')
    src, exe = d / 'map.cpp', d / 'map'
    src.write_text(MAIN)
    r = subprocess.run([cxx, '-std=c++17', '-I', CSRC, str(src), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, 'an offset is not the sum of its parts (exit %d)' % r.returncode
    out, cur = {}, None
    for ln in r.stdout.splitlines():
        k, *v = ln.split()
        v = [int(x) for x in v]
        if k == 'L':
            cur = out[v[0]] = dict(NT=v[1], threads=v[2], pieces=v[3], p=[], s=[], z=[])
        else:
            cur[k].append(v if len(v) > 1 else v[0])
    return out


def frag_index(slot, t, e, NT):
    """float index of (slot, t, e) in h1f: k_h1_frag's formula (din_x.hpp)"""
    n, lane, kb = t // 32, t % 32 + 32 * ((e % 16) // 8), e // 16
    return (((slot * NT + n) * 8 + kb) * 64 + lane) * 8 + e % 8


@pytest.mark.parametrize('cnt', [1, 33])
@pytest.mark.parametrize('L', [1, 33, 64])
def test_every_state_is_stored_once_and_where_k_h1_frag_puts_it(tables, L, cnt):
    tb = tables[L]
    NT = tb['NT']
    assert NT == (L + 31) // 32 and tb['threads'] * tb['pieces'] == 32 * 32
    pieces = np.array(tb['p'])                       # [1024][row, c4, h1 lane part, h1f lane part]
    steps = np.array(tb['s']).reshape(L, 2)
    assert sorted(map(tuple, pieces[:, :2])) == [(r, c) for r in range(32) for c in range(32)]       # the tile, each piece once
    guard = 4096                                     # floats around the encode's slots that must stay untouched
    h1_cnt = np.zeros(guard + cnt * L * 128 + guard, dtype=np.int32)
    h1_val = np.full(h1_cnt.shape, -1, dtype=np.int64)
    f_cnt = np.zeros(guard + cnt * NT * 4096 + guard, dtype=np.int32)
    f_val = np.full(f_cnt.shape, -1, dtype=np.int64)
    for row0 in range(0, cnt, 32):
        rows_here = min(32, cnt - row0)
        size_h, size_f = rows_here * L * 128 * 4, rows_here * NT * 16384          # the two descriptors (bytes)
        base_h, base_f = guard + row0 * L * 128, guard + row0 * NT * 4096
        for t in range(L):
            oh, of = pieces[:, 2] + steps[t, 0], pieces[:, 3] + steps[t, 1]
            assert (oh >= 0).all() and (of >= 0).all() and (oh % 16 == 0).all() and (of % 16 == 0).all()
            valid = pieces[:, 0] < rows_here
            # a raw buffer store is dropped when it does not lie inside the descriptor - that must be exactly the rows past cnt
            assert ((oh + 16 <= size_h) == valid).all() and ((of + 16 <= size_f) == valid).all()
            for k in range(4):
                val = ((row0 + pieces[valid, 0]) * L + t) * 128 + pieces[valid, 1] * 4 + k
                np.add.at(h1_cnt, base_h + oh[valid] // 4 + k, 1)
                h1_val[base_h + oh[valid] // 4 + k] = val
                np.add.at(f_cnt, base_f + of[valid] // 4 + k, 1)
                f_val[base_f + of[valid] // 4 + k] = val
        z = np.array(tb['z'], dtype=np.int64)
        assert len(z) == (32 * NT - L) * 1024
        if len(z):
            inside = z + 16 <= size_f
            rows = z // (NT * 16384)
            assert (inside == (rows < rows_here)).all()
            for k in range(4):
                np.add.at(f_cnt, base_f + z[inside] // 4 + k, 1)
                f_val[base_f + z[inside] // 4 + k] = -2                              # a zero of the tail
    # h1: row-major, every element once, nothing around it
    assert (h1_cnt[guard:-guard] == 1).all() and (h1_cnt[:guard] == 0).all() and (h1_cnt[-guard:] == 0).all()
    assert (h1_val[guard:-guard] == np.arange(cnt * L * 128)).all()
    # h1f: every position of every slot once (state or tail zero), nothing around it, states where k_h1_frag's formula says
    assert (f_cnt[guard:-guard] == 1).all() and (f_cnt[:guard] == 0).all() and (f_cnt[-guard:] == 0).all()
    want = np.full(cnt * NT * 4096, -2, dtype=np.int64)
    slot, t, e = np.meshgrid(np.arange(cnt), np.arange(L), np.arange(128), indexing='ij')
    want[frag_index(slot, t, e, NT)] = (slot * L + t) * 128 + e
    assert (f_val[guard:-guard] == want).all()
    assert (want == -2).sum() == cnt * (32 * NT - L) * 128                           # the zero tail is covered: written, not assumed
