"""The DIEN scorer's off-default cases (tests/dien_shape_cases.py) on the CPU:

* rl4rs_amd/csrc/dien_plan.hpp, compiled with the host compiler as tests/test_dien_plan_host.py does, gives for every (case,
  forward shape, option, AUGRU row pin) the plan the table claims - so each case is known to enter the forms it is there for;
* the bars are attainable: OracleDien in float32 lies within a QUARTER of every bar of OracleDien in float64 on the case's own
  inputs (the figures are in dien_shape_cases.FLOAT32);
* each forward shape has the stated number of duplicate row groups, between a third and two thirds;
* teeth: a duplicate group scored from another template, or the all-feature row split at the default configuration's offsets
  512 / 640, moves the comparison far beyond the bars."""
import subprocess

import numpy as np
import pytest

import dien_shape_cases as T
from test_dien_plan_host import CSRC, _cxx, call, traits

N_CU = 256
PINS = {'f1': (0,), 'f8': (0, 32, 64), 'f9': (0, 32, 64)}
ARMS = ('', 'no_tier2_rows', 'no_row_dedup')
EXTRA_ARMS = {'A': ('no_gemm_group',), 'D': ('dense_fork',), 'G': ('dense_fork',)}


def case_traits(case, opt=None, fp32=False):
    """DienTraits as rl4rs_dien_create fills them at the case's numbers (test_dien_plan_host.traits fixes E / S / Dn / L)"""
    L, Cn, U, Dn, S, K = T.CASES[case]
    t = traits(opt or None, fp32=fp32, Cn=Cn, U=U, n_cu=N_CU)
    Kh = S * T.NH2 + U + T.E
    t.update(S=S, Dn=Dn, L=L, Fld=Kh if t['ptab'] else Kh + Cn * T.E, max_rows=128)
    t['tsum'] = t['ptab'] and Cn <= 24 and opt != 'no_head_fused'            # dien.hip: the tsum buffer exists only at Cn <= 24
    t['lazy_expand'] = t['tier2_rows']
    return t


def case_call(case, shape, pin=0, carried=False):
    group, R, _ = T.SHAPES[shape]
    Dn = T.CASES[case][3]
    c = call(R, group, hint=T.inputs(case, shape)['n_active'] if (case == 'F' and shape == 'f1') else 0, pin=pin, carried=carried)
    c.update(obs_last=shape == 'f9', dense_vec=Dn % 4 == 0)
    return c


def _table():
    rows = []
    for case in sorted(T.CASES):
        for shape in sorted(T.SHAPES):
            for arm in ARMS + EXTRA_ARMS.get(case, ()):
                for pin in PINS[shape]:
                    rows.append((case, shape, arm, pin, False, False))
            rows.append((case, shape, '', 0, True, False))                    # the exact-fp32 handle
        rows.append((case, 'f1', '', 0, False, True))                         # a carried partition
    return rows


def _program(rows):
    def init(kind, d):
        return '%s{}; %s' % (kind, ' '.join('x.%s = %s;' % (k, str(v).lower() if isinstance(v, bool) else v) for k, v in d.items()))
    body = []
    for i, (case, shape, arm, pin, fp32, carried) in enumerate(rows):
        body.append('    { DienTraits x = %s const DienTraits t = x; { DienCall x = %s show(%d, t, x); } }'
                    % (init('DienTraits', case_traits(case, arm, fp32)), init('DienCall', case_call(case, shape, pin, carried)), i))
    for case in sorted(T.CASES):
        body.append('    { DienTraits x = %s printf("one_grid %s %%d\\n", (int)x.pair_one_grid()); }' % (init('DienTraits', case_traits(case)), case))
    return ('#include "dien_plan.hpp"\nusing namespace rl4rs;\n'
            'static void show(int i, const DienTraits& t, const DienCall& c) {\n'
            '    char buf[512];\n    dien_plan_str(dien_plan(t, c), buf, sizeof(buf));\n    printf("plan %d | %s\\n", i, buf);\n}\n'
            'int main() {\n' + '\n'.join(body) + '\n    return 0;\n}\n')


def test_plans_of_every_case(tmp_path):
    cxx = _cxx()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    rows = _table()
    src, exe = tmp_path / 'shapes_main.cpp', tmp_path / 'shapes_main'
    src.write_text(_program(rows))
    r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Wextra', '-Werror', '-I', CSRC, str(src), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    plans = [ln.split(' | ')[1] for ln in out if ln.startswith('plan ')]
    assert len(plans) == len(rows)
    wrong = []
    for text, (case, shape, arm, pin, fp32, carried) in zip(plans, rows):
        got = dict(tok.split('=', 1) for tok in text.split())
        want = T.plan_tokens(case, shape, arm, pin, fp32, carried)
        if got != want:
            wrong.append((case, shape, arm, pin, fp32, carried, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}))
        if not arm and not fp32 and not carried and pin in (0, 32):
            print(case, shape, 'pin', pin, text)
    assert not wrong, wrong
    # the forms each case is in the table for, spelled out (plan_tokens is general; these are the table's claims)
    P = T.plan_tokens
    assert P('A', 'f1')['cat'] == 'k_cat_attn2<24,false>' and P('A', 'f8')['cat'] == 'k_cat_attn2g<8,8>' and P('A', 'f9')['cat'] == 'k_cat_attn2g<9>'
    assert P('A', 'f1')['dense'] == 'pair' and P('A', 'f1')['expand'] == 'lazy:992' and P('A', 'f8')['expand'] == 'behind:992'
    assert all(P('B', s)['cat'] == 'k_cat_attn2<24,false>' and P('B', s)['tier2'] == '1' for s in T.SHAPES) and P('B', 'f1')['expand'] == 'lazy:416'
    assert all(P('C', s)['cat'] == 'k_cat_attn' and P('C', s)['head'] == 'tables+k_head_finish' and P('C', s)['tier2'] == '0' and
               P('C', s)['expand'] == 'front:512' for s in T.SHAPES)
    assert all(P('D', s)['dense'] == 'two_gemms' and P('D', s)['qside'] == 'scorer_gemm' and P('D', s)['tier2'] == '0' and P('D', s)['shadow'] == '0' and
               P('D', s)['expand'] == 'front:512' for s in T.SHAPES)
    assert P('E', 'f8')['cat'] == 'k_cat_attn2g<8,8>' and P('E', 'f9')['cat'] == 'k_cat_attn2g<9>' and P('E', 'f9')['expand'] == 'behind:1216'
    assert P('F', 'f1')['shadow'] == '1' and P('F', 'f1')['augru'] == 'k_augru_xs' and P('F', 'f1')['din'] == 'k_din_xq'
    assert P('G', 'f8')['cat'] == 'k_cat_attn2g<8,8>' and P('G', 'f1')['cat'] == 'k_cat_attn2<24,false>' and P('G', 'f1', 'dense_fork')['dense'] == 'chain@side'
    assert all(P('H', s)['cat'] == 'k_cat_attn2<24,false>' and P('H', s)['dense'] == 'two_gemms' and P('H', s)['expand'] == 'front:256' for s in T.SHAPES)
    assert all(P(c, 'f8', pin=64)['augru'] == 'k_augru_x_64' and P(c, 'f9', pin=64)['augru'] == 'k_augru_x_64' and
               P(c, 'f8', pin=0)['augru'] == 'k_augru_x_32' for c in T.CASES)
    # the paired GEMM launch as one grid: what the header says equals the rule read from gemm.hip.  Case A's q-side term is
    # S * 64 = 192 columns wide: ny == 2 in gemm_h16_route, the condition of launch_gemm_h16_pair's two-launch fallback
    one = dict((ln.split()[1], int(ln.split()[2])) for ln in out if ln.startswith('one_grid '))
    assert one == dict((c, int(T.pair_one_grid(c))) for c in T.CASES), one
    S_A = T.CASES['A'][4]
    assert S_A * T.ATT_H1 == 192 and ((192 + 31) // 32 + 3) // 4 == 2
    assert one == dict(A=0, B=1, C=1, D=0, E=0, F=0, G=1, H=0)


@pytest.mark.parametrize('case', sorted(T.CASES))
def test_bars_attainable_in_float32(case):
    """float32 arithmetic can meet the bars at the case's widths: OracleDien(float32) within a quarter of each"""
    worst = {}
    for shape in sorted(T.SHAPES):
        got = T.oracle_outputs(case, shape, np.float32)
        if case != 'A':
            got.pop('h1_0')                    # the first-GRU cache is compared with the oracle in case A only
        errs = T.errors(got, T.reference(case, shape), case)
        print(T.report('%s %s float32 vs float64' % (case, shape), errs))
        assert not T.misses(errs, 0.25), T.misses(errs, 0.25)
        for k, (e, bar) in errs.items():
            key = k.rstrip('0123456789').rstrip('_')
            rel = e / (bar / T.BARS['dense']) if k == 'dense' else e
            worst[key] = max(worst.get(key, 0.0), rel)
    print('FLOAT32', case, ' '.join('%s %.1e' % kv for kv in sorted(worst.items())))
    # the figures written into the table (one machine's BLAS; another sums in another order) are themselves inside the quarter
    assert set(T.FLOAT32[case]) == set(worst)
    for k, v in T.FLOAT32[case].items():
        assert v < 0.25 * T.BARS[{'score': 'scores'}.get(k, k)], (k, v)


@pytest.mark.parametrize('shape', sorted(T.SHAPES))
def test_duplicate_counts(shape):
    ng, dup = T.DUPLICATES[shape]
    assert ng / 3.0 <= dup <= 2.0 * ng / 3.0
    for case in sorted(T.CASES):
        x = T.inputs(case, shape)
        assert x['slots'].shape == (T.CASES[case][4], ng) and x['R'] == ng * x['group']
        assert ng - x['n_active'] == dup, (case, shape, x['n_active'])
        # a duplicate's representative holds the same template of the same run, and no two representatives do
        for g, r in enumerate(x['rep']):
            assert x['who'][g] == x['who'][r]
        assert len(set(x['who'][r] for r in set(x['rep']))) == x['n_active']


def _outputs_from(ref, rows):
    """what a forward would hand back if output row i held the result of row rows[i]"""
    out = dict((k, v[rows]) for k, v in ref.items() if k not in ('scores', 'obs_last'))
    out['scores'] = ref['scores'][:, rows]
    return out


@pytest.mark.parametrize('case,shape', [('A', 'f1'), ('E', 'f8'), ('H', 'f9')])
def test_teeth_a_wrong_representative_is_seen(case, shape):
    """A wrong 'equal' of row_words_equal gives a row group another group's result.  Take every duplicate group's expected rows
    from ANOTHER template of its run instead of its representative's: the comparison moves far beyond the bars (the right
    representative leaves it at zero)."""
    x, ref = T.inputs(case, shape), T.reference(case, shape)
    g = x['group']
    rows = np.arange(x['R'])
    good = (x['rep'][rows // g] * g + rows % g)
    ok = T.errors(_outputs_from(ref, good), ref, case)
    assert all(e == 0.0 for e, _ in ok.values()), ok
    other = x['rep'].copy()
    for grp, r in enumerate(x['rep']):
        if r != grp:                                                   # a duplicate: the nearest group of its run with another template
            run = x['who'][grp][0]
            cand = [h for h in range(len(x['who'])) if x['who'][h][0] == run and x['who'][h][1] != x['who'][grp][1]]
            if cand:
                other[grp] = cand[0]
    assert (other != x['rep']).sum() >= 3
    bad = T.errors(_outputs_from(ref, other[rows // g] * g + rows % g), ref, case)
    print(T.report('%s %s wrong representative' % (case, shape), bad))
    # the histories are the run's, so the AUGRU input differs only through the query: every row-dependent quantity is off
    for k in ('dense', 'cat', 'query', 'obs', 'prob'):
        assert bad[k][0] > 20 * bad[k][1], (k, bad[k])


@pytest.mark.parametrize('case', ['A', 'B', 'D', 'E', 'F', 'H'])
def test_teeth_the_default_offsets_are_seen(case):
    """The all-feature row split at the default configuration's offsets (AUGRU columns end at 512, dense at 640) instead of the
    case's own: the dense or the category part is read from the wrong columns, far beyond the bars."""
    ref = T.reference(case, 'f1')
    nseq, U, _, _ = T.columns(case)
    assert (nseq, nseq + U) != (512, 640)
    ok = T.errors(dict(ref), ref, case)
    assert all(e == 0.0 for e, _ in ok.values())
    bad = T.errors(dict(ref), ref, case, offsets=(512, 640))
    print(T.report('%s split at 512 / 640' % case, bad))
    assert any(bad[k][0] > 20 * bad[k][1] for k in ('dense', 'cat')) and T.misses(bad)
