"""The scratch of the raw-state training handle, sized on the host: rl4rs_amd/csrc/rawtrain_scratch.hpp (what rl4rs_rawtrain_create
allocates behind cx.wt and cx.part) against what every reduction and transpose of a backward writes there, computed by the
selection code itself (rl4rs_amd/csrc/reduce_plan.hpp: tn_t128_plan and the chunk rules of st_tn / st_cs / st_back), compiled with the
host compiler as tests/test_dien_shapes_host.py does.

The handle used to size both buffers from max(F * 256, Dn * U, 256 * AE), without dense_w2's U * U.  The second test keeps that
arithmetic in the program and shows which calls it could not hold at hidden_units = 512: no device ever ran them."""
import shutil
import subprocess

import pytest

import rawdqn_ref as R
import rawstate_rows_cases as T
from test_dien_plan_host import CSRC
from test_gpu_policy_shapes import RAW_CFGS, RAW_FLOOR

ROWS = (1, 1024, 1025, 2048, 2049, 4095, 4096)
MAX_ROWS = (1, 700, 1030, 1152, 2100, 4100, 4608, 20000)
CALLS = ('head_w', 'head_b', 'ctx_w', 'ctx_b', 'dense_w2', 'dense_b2', 'dense_w1', 'dense_b1', 'back_head', 'back_ctx', 'back_dense_w2')
U512_DEFAULT = dict(RAW_FLOOR, hidden_units=512)         # E 128, S 2, Dn 432, A 284: U * U 262144 > F * 256 229376 > Dn * U 221184


def _grid():
    g = {'default': RAW_FLOOR, 'u512_default': U512_DEFAULT}
    g.update(RAW_CFGS)
    g.update((name, cfg) for name, (cfg, _) in T.CASES.items())
    for U in (256, 467, 468, 512, 1024):
        g['u%d_small_emb' % U] = dict(RAW_CFGS['R2'], hidden_units=U, emb_size=8)
        g['u%d_odd' % U] = dict(T.ODD, hidden_units=U, emb_size=4)
    return g


def _program(grid):
    names = sorted(grid)
    rows = ['    {%s},' % ', '.join(str(int(grid[n][k])) for k in ('emb_size', 'hidden_units', 'category_hash_size', 'seq_num', 'dense_feature_num',
                                                                 'category_feature_num', 'maxlen', 'action_size')) for n in names]
    return '''#include <cstdio>
#include "rawtrain_scratch.hpp"
static const long long CFG[][8] = {
%s
};
static const int ROWS[] = {%s}, MAX_ROWS[] = {%s};
// the arithmetic rl4rs_rawtrain_create had before this header existed
static void parent(const RawTrainDims& d, const RawTrainScratch& s, long long* wt, long long* part) {
    long long wmax = s.F * 256;
    if (d.Dn * d.U > wmax) wmax = d.Dn * d.U;
    if (256 * s.AE > wmax) wmax = 256 * s.AE;
    *wt = wmax;
    *part = (d.max_rows + 511) / 512 * wmax;
}
int main() {
    for (unsigned i = 0; i < sizeof(CFG) / sizeof(CFG[0]); ++i) {
        const long long* c = CFG[i];
        for (int B : MAX_ROWS) {
            const RawTrainDims d{c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], B};
            const RawTrainScratch s = rawtrain_scratch(d);
            long long pwt, ppart;
            parent(d, s, &pwt, &ppart);
            if (B == MAX_ROWS[0]) {
                printf("dims %%u %%lld %%lld %%lld |", i, (long long)s.F, (long long)s.AE, (long long)s.REC);
                for (int k = 0; k < RT_COUNT; ++k) printf(" %%lld", (long long)s.sizes[k]);
                printf("\\n");
            }
            for (int k = 0; k <= (int)(sizeof(ROWS) / sizeof(ROWS[0])); ++k) {
                const int N = k < (int)(sizeof(ROWS) / sizeof(ROWS[0])) ? ROWS[k] : B;
                if (N > B) continue;
                for (int rec = 0; rec < 2; ++rec)
                    for (int al = 0; al < 2; ++al) {
                        const RawTrainNeed n = rawtrain_need(d, N, rec ? (int)s.REC : (int)d.Dn, al != 0);
                        printf("need %%u %%d %%d %%d %%d | %%lld %%lld | %%lld %%lld |", i, B, N, rec, al, (long long)s.part_floats,
                               (long long)s.wt_floats, ppart, pwt);
                        for (size_t v : n.part) printf(" %%zu", v);
                        for (size_t v : n.wt) printf(" %%zu", v);
                        printf("\\n");
                    }
            }
        }
    }
    return 0;
}
''' % ('\n'.join(rows), ', '.join(map(str, ROWS)), ', '.join(map(str, MAX_ROWS)))


_CACHE = {}


def _table(tmp_path_factory):
    """-> (grid, dims lines, need records) of one compiled run, shared by the tests"""
    if 'out' not in _CACHE:
        cxx = next((c for c in ('g++', 'c++', 'clang++') if shutil.which(c)), None)
        if cxx is None:
            pytest.skip('no host C++ compiler')
        grid = _grid()
        d = tmp_path_factory.mktemp('rawtrain_scratch')
        src, exe = d / 'scratch_main.cpp', d / 'scratch_main'
        src.write_text(_program(grid))
        r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Wextra', '-Werror', '-I', CSRC, str(src), '-o', str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
        names = sorted(grid)
        dims, need = {}, []
        for ln in out:
            head, rest = ln.split(' | ', 1) if ln.startswith('need') else (ln, '')
            tok = head.split()
            if tok[0] == 'dims':
                a, b = ln.split(' | ')
                dims[names[int(a.split()[1])]] = (tuple(map(int, a.split()[2:])), tuple(map(int, b.split())))
            else:
                alloc, par, calls = rest.split(' | ')
                need.append(dict(name=names[int(tok[1])], max_rows=int(tok[2]), N=int(tok[3]), rec=int(tok[4]), aligned=int(tok[5]),
                                 alloc=tuple(map(int, alloc.split())), parent=tuple(map(int, par.split())),
                                 calls=dict(zip(CALLS, map(int, calls.split())))))
        _CACHE['out'] = (grid, dims, need)
    return _CACHE['out']


def _short(r, alloc):
    """the calls of record ``r`` that do not fit (part floats, wt floats) = ``alloc``"""
    return sorted(k for k, v in r['calls'].items() if v > alloc[1 if k.startswith('back_') else 0])


def test_every_call_fits_the_scratch(tmp_path_factory):
    grid, dims, need = _table(tmp_path_factory)
    pairs = sum(1 for B in MAX_ROWS for N in ROWS + (B,) if N <= B)
    assert set(dims) == set(grid) and len(need) == len(grid) * pairs * 4
    for name, cfg in grid.items():
        (F, AE, REC), sizes = dims[name]
        assert (F, AE, REC) == T.dims(cfg) and REC == R.record_fields(cfg)[0]
        H, E, U, Dn = cfg['category_hash_size'], cfg['emb_size'], cfg['hidden_units'], cfg['dense_feature_num']
        assert sizes == (H * E, H * E, Dn * U, U, U * U, U, F * 256, 256, 256 * AE, AE)
    bad = [(r['name'], r['max_rows'], r['N'], r['rec'], r['aligned'], _short(r, r['alloc'])) for r in need if _short(r, r['alloc'])]
    assert not bad, bad[:10]
    # the grid does enter what it is there for: chunked partials from 1025 rows, transposes from 2049, the 128 x 128 form from 4096
    # (fewer floats than 512-row chunks would take: its chunk count is capped by the same ceil(N / 512))
    pick = lambda **kw: [r for r in need if all(r[k] == v for k, v in kw.items())]
    for r in pick(name='base_n4100', max_rows=4100, rec=0, aligned=1):
        c, N = r['calls'], r['N']
        nz = (N + 511) // 512
        assert (c['head_w'] > 0) == (N > 1024) and (c['head_b'] > 0) == (N > 512) and (c['back_ctx'] > 0) == (N > 2048)
        if N > 1024:
            assert c['head_w'] == nz * 256 * 285 and c['dense_w2'] == nz * 128 * 128 and c['ctx_b'] == nz * 256
        if N > 2048:
            assert (c['back_head'], c['back_ctx'], c['back_dense_w2']) == (256 * 285, 320 * 256, 128 * 128)
    for cfg_name, U in (('u512_n2100', 512), ('u1024_odd', 1024)):
        r, = pick(name=cfg_name, max_rows=4100, N=4100, rec=0, aligned=0)
        assert r['calls']['dense_w2'] == 9 * U * U == r['alloc'][0] and r['calls']['back_dense_w2'] == U * U == r['alloc'][1]


def test_the_sizing_without_dense_w2_overflowed_at_hidden_512(tmp_path_factory):
    """max(F * 256, Dn * U, 256 * AE) at the default sizes with hidden_units = 512: from 1025 rows dense_w2's chunk partials pass the
    end of cx.part, from 2049 rows its transpose passes the end of cx.wt; at hidden_units = 128 the same arithmetic held."""
    grid, dims, need = _table(tmp_path_factory)
    seen = {}
    for r in need:
        if r['name'] == 'u512_default':
            # a call of fewer rows than max_rows may fit by the slack of the larger handle, never the other way round
            assert set(_short(r, r['parent'])) <= {'dense_w2', 'back_dense_w2'}
            if r['N'] == r['max_rows']:
                seen.setdefault(r['N'], set()).update(_short(r, r['parent']))
        if r['name'] == 'default':
            assert not _short(r, r['parent']), r
    for N, short in sorted(seen.items()):                   # a handle made for the rows of its one call, as every trainer makes it
        print('hidden_units 512, %5d rows: the former sizing is short for %s' % (N, sorted(short) or 'nothing'))
        want = set()
        if N > 1024:
            want.add('dense_w2')
        if N > 2048:
            want.add('back_dense_w2')
        assert short == want, (N, short)
    assert set(seen) == set(MAX_ROWS)
    r, = [r for r in need if r['name'] == 'u512_default' and r['max_rows'] == 1030 and r['N'] == 1025 and r['rec'] == 0 and r['aligned'] == 1]
    assert r['calls']['dense_w2'] == 3 * 262144 > r['parent'][0] == 3 * 229376
    # and the GPU module's own u512 cases
    for name in ('u512_n2100', 'u512d64_n2100'):
        short = set()
        for r in need:
            if r['name'] == name and r['N'] == r['max_rows'] == 2100:
                short.update(_short(r, r['parent']))
        assert short == {'dense_w2', 'back_dense_w2'}, (name, short)
