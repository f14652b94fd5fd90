"""The lazy form of the duplicates' expansion in the launch plan of the scorer forward (rl4rs_amd/csrc/dien_plan.hpp), on the
CPU: dien_plan.hpp alone, compiled with the host C++ compiler as tests/test_dien_plan_host.py does it.  With the trait `lazy_expand`
on, exactly the forwards that would say `expand=behind` and are observation-shaped, or reward-shaped without a caller's obs
buffer, say `expand=lazy`; every other token of every plan, and every plan of a handle or call the form does not apply to, is
what the existing table holds.  With the trait off (what zero-initialisation gives) the existing table's rows come out unchanged."""
import subprocess

import pytest

import test_dien_plan_host as base
from test_dien_plan_host import BY_OPT, FP32, G8, NO_T2, SHADOW, call, plan, traits

LAZY = dict(expand='lazy:768')
G9 = dict(cat='k_cat_attn2g<9>', din='k_din_x_16', augru='k_augru_x_64')


def lz(opt=None, **kw):
    return dict(traits(opt, **kw), lazy_expand=True)


def no_obs(c):
    return dict(c, obs=False)


CASES = [
    # (name, traits, call, expected)
    ('lazy: flagship obs hint 1771', lz(), call(4096, 1, hint=1771), plan(**SHADOW, **LAZY)),
    ('lazy: flagship obs hint 1771 carried', lz(), call(4096, 1, hint=1771, carried=True), plan(dedup='carried', **SHADOW, **LAZY)),
    ('lazy: flagship obs no hint', lz(), call(4096, 1), plan(**LAZY)),
    ('lazy: obs-shaped without a caller obs', lz(), no_obs(call(96, 1, hint=32)), plan(**SHADOW, **LAZY)),
    ('lazy: flagship reward g9 no obs', lz(), no_obs(call(36864, 9)), plan(**G9, **LAZY)),
    ('lazy: flagship reward g9 no obs carried', lz(), no_obs(call(36864, 9, carried=True)), plan(dedup='carried', **G9, **LAZY)),
    ('lazy: flagship reward g9 caller obs', lz(), call(36864, 9), plan(**G9)),
    ('lazy: flagship reward g8 no obs', lz(), no_obs(call(32768, 8)), plan(augru='k_augru_x_64', **G8, **LAZY)),
    ('lazy: flagship reward g8 caller obs', lz(), call(32768, 8), plan(augru='k_augru_x_64', **G8)),
    ('lazy: R192 g8 rows32 no obs', lz(), no_obs(call(192, 8, pin=32)), plan(**G8, **LAZY)),
    # the forms that keep exactly their launches: the tokens of the existing table
    ('lazy: mirror armed, obs given', lz(), call(96, 1, hint=32, mirror=True), plan(head='tsum+k_gemm_h16+mirror', **NO_T2)),
    ('lazy: dup_store g1', lz('dup_store'), call(96, 1, hint=32), BY_OPT['dup_store'][0]),
    ('lazy: dup_store g8 no obs', lz('dup_store'), no_obs(call(192, 8, pin=32)), BY_OPT['dup_store'][1]),
    ('lazy: no_tier2_rows g1', lz('no_tier2_rows'), call(96, 1, hint=32), BY_OPT['no_tier2_rows'][0]),
    ('lazy: no_tier2_rows g8 no obs', lz('no_tier2_rows'), no_obs(call(192, 8, pin=32)), BY_OPT['no_tier2_rows'][1]),
    ('lazy: no_row_dedup g1', lz('no_row_dedup'), call(96, 1, hint=32), BY_OPT['no_row_dedup'][0]),
    ('lazy: no_row_dedup g8 no obs', lz('no_row_dedup'), no_obs(call(192, 8, pin=32)), BY_OPT['no_row_dedup'][1]),
    ('lazy: fp32 g1', lz(fp32=True), call(96, 1, hint=32), plan(din='k_din_scores<0,0>x4', **FP32)),
    ('lazy: fp32 g9 no obs', lz(fp32=True), no_obs(call(189, 9, pin=64)), plan(cat='k_cat_attn2g<9>', din='k_din_scores<1,0>x3', **FP32)),
    ('lazy: dense_fork g1', lz('dense_fork'), call(96, 1, hint=32), BY_OPT['dense_fork'][0]),
    ('lazy: Cn 25 g1', lz(Cn=25), call(96, 1, hint=32), plan(cat='k_cat_attn', head='tables+k_head_finish', **NO_T2)),
    # other options change other stages and leave the form alone
    ('lazy: no_augru_shadow g1', lz('no_augru_shadow'), call(96, 1, hint=32), plan(**LAZY)),
    ('lazy: no_gemm_group g1', lz('no_gemm_group'), call(96, 1, hint=32), plan(dense='chain', qside='mapped_k_gemm_h16', **LAZY)),
    # the trait off: rows of the existing table, unchanged
    ('off: flagship obs hint 1771', traits(), call(4096, 1, hint=1771), plan(**SHADOW)),
    ('off: flagship reward g9', traits(), call(36864, 9), plan(**G9)),
    ('off: flagship reward g9 no obs', traits(), no_obs(call(36864, 9)), plan(**G9)),
    ('off: carried partition', traits(), call(96, 1, carried=True), plan(dedup='carried', **SHADOW)),
    ('off: no_tier2_rows g1', traits('no_tier2_rows'), call(96, 1, hint=32), BY_OPT['no_tier2_rows'][0]),
    ('off: dup_store g8', traits('dup_store'), call(192, 8, pin=32), BY_OPT['dup_store'][1]),
]


def _program():
    def init(kind, d):
        return '%s{}; %s' % (kind, ' '.join('x.%s = %s;' % (k, str(v).lower() if isinstance(v, bool) else v) for k, v in d.items()))
    body = ['    { DienTraits x = %s const DienTraits t = x; { DienCall x = %s show("%s", t, x); } }' % (init('DienTraits', t), init('DienCall', c), name)
            for name, t, c, _ in CASES]
    # the gather head's address rule: allf (768 columns) is the widest of the three matrices - 2^29 elements end behind row 699 050
    body.append('    printf("fits %d %d %d\\n", (int)g16_gather_fits(4096, 768, 768), (int)g16_gather_fits(699050, 768, 768), (int)g16_gather_fits(699051, 768, 768));')
    return ('#include "dien_plan.hpp"\nusing namespace rl4rs;\n'
            'static void show(const char* name, const DienTraits& t, const DienCall& c) {\n'
            '    char buf[512];\n    dien_plan_str(dien_plan(t, c), buf, sizeof(buf));\n    printf("plan %s | %s\\n", name, buf);\n}\n'
            'int main() {\n' + '\n'.join(body) + '\n    return 0;\n}\n')


def test_lazy_plans(tmp_path):
    cxx = base._cxx()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    src, exe = tmp_path / 'plan_lazy.cpp', tmp_path / 'plan_lazy'
    src.write_text(_program())
    r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Wextra', '-Werror', '-I', base.CSRC, str(src), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    plans = [ln[5:].split(' | ') for ln in out if ln.startswith('plan ')]
    assert [p[0] for p in plans] == [c[0] for c in CASES]
    wrong = []
    for (name, text), (_, _, _, want) in zip(plans, CASES):
        got = dict(tok.split('=', 1) for tok in text.split())
        if got != want:
            wrong.append((name, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}))
    assert not wrong, wrong
    assert [ln for ln in out if ln.startswith('fits ')] == ['fits 1 1 0']
