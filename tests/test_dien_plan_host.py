"""The launch plan of the scorer forward (rl4rs_amd/csrc/dien_plan.hpp) on the CPU: the header is compiled with the host
C++ compiler alone into a small program that prints dien_plan() for a table of handles and calls, and the printed plans are
compared with what the forward launched for these cases BEFORE the plan existed.

Where the entries come from: 'trace' = the kernel list of that arm and forward in profiles/r18_forward_launches.md (the parent
library under tools/forward_launches.py, n_cu = 256); 'code' = read from the parent's rl4rs_dien_forward, for the shapes that
listing cannot reach (full size, U = 144: hidden_units is a multiple of 32 on a real handle)."""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'rl4rs_amd', 'csrc')
OPTS = ('no_row_dedup', 'no_tier2_rows', 'no_augru_shadow', 'dup_store', 'dense_fork', 'no_gemm_group', 'no_dense_chain', 'no_gemm16',
        'din_v1', 'no_din16', 'augru_h16', 'cat_v1', 'no_cat_group', 'no_head_tables', 'no_head_fused', 'din_rows16')


def traits(opt=None, fp32=False, Cn=21, U=128, n_cu=256):
    """DienTraits as rl4rs_dien_create fills them for one option on top of the defaults (weights inside every fp16 range),
    flagship shape numbers: E 128, L 64, S 2, Dn 432"""
    E, S, NH2, Dn = 128, 2, 256, 432
    t = dict(fp16x2=not fp32, augru_x=opt != 'augru_h16', din_x=opt != 'din_v1', din_rows_auto=opt != 'din_rows16',
             cat_v2=opt != 'cat_v1', cat_group=opt != 'no_cat_group', dense_chain=opt != 'no_dense_chain',
             gemm_group=opt != 'no_gemm_group', dense_fork=opt == 'dense_fork', augru_shadow=opt != 'no_augru_shadow')
    t['gemm16'] = t['fp16x2'] and opt != 'no_gemm16'
    t['din16'] = t['fp16x2'] and opt != 'no_din16'
    t['cat16'] = t['fp16x2']
    t['h1f'] = t['din16'] and t['din_x']
    t['row_dedup'] = opt != 'no_row_dedup' and t['augru_x'] and t['h1f']
    t['dup_store'] = t['row_dedup'] and opt == 'dup_store'
    t['tier2_rows'] = t['row_dedup'] and opt != 'no_tier2_rows'
    t['ptab'] = opt != 'no_head_tables'
    t['tsum'] = t['ptab'] and Cn <= 24 and opt != 'no_head_fused'
    Kh = S * NH2 + U + E
    t.update(E=E, U=U, L=64, S=S, Cn=Cn, Dn=Dn, Fld=Kh if t['ptab'] else Kh + Cn * E, NH2=NH2, n_cu=n_cu, max_rows=36864)
    return t


def call(R, group, hint=0, pin=0, mirror=False, carried=False):
    return dict(R=R, group=group, obs=True, prob=True, mirror=mirror, obs_last=False, carried=carried, part_groups=R // group if carried else 0,
                row_order=False, augru_rows=pin, distinct_hint=hint, dense_vec=True)


def plan(**kw):
    """the default forward of a row-dedup handle without the shadow plane, with the fields a case changes"""
    p = dict(tier2='1', shadow='0', dedup='k_row_dedup', cat='k_cat_attn2<21,true>', dense='pair', qside='in_pair', din='k_din_x_auto',
             augru='k_augru_x_32', expand='behind:768', head='tsum+k_gemm_h16', prob='1')
    p.update(kw)
    return p


SHADOW = dict(shadow='1', cat='shadow', dense='shadow', qside='in_k_din_xq', din='k_din_xq', augru='k_augru_xs')
G8 = dict(cat='k_cat_attn2g<8,8>', din='k_din_x_16')
NO_T2 = dict(tier2='0', expand='front:512')
NO_DD = dict(tier2='0', dedup='none', expand='none:0')
# what one option changes on the group-1 shape (R 96, hint 32: the default handle takes the shadow plane) and on the group-8 shape
# (R 192, rows pinned 32) - 'trace'
BY_OPT = {
    'no_row_dedup': (plan(**NO_DD), plan(**NO_DD, **G8)),
    'no_tier2_rows': (plan(**NO_T2), plan(**NO_T2, **G8)),
    'no_augru_shadow': (plan(), plan(**G8)),
    'dup_store': (plan(tier2='0', dedup='k_row_dedup+dup_lists', expand='none:0'), plan(tier2='0', dedup='k_row_dedup+dup_lists', expand='none:0', **G8)),
    'dense_fork': (plan(dense='chain@side', qside='scorer_gemm', **NO_T2), plan(dense='chain@side', qside='scorer_gemm', **NO_T2, **G8)),
    'no_gemm_group': (plan(dense='chain', qside='mapped_k_gemm_h16'), plan(dense='chain', qside='mapped_k_gemm_h16', **G8)),
    'no_dense_chain': (plan(dense='two_gemms', qside='scorer_gemm', **NO_T2), plan(dense='two_gemms', qside='scorer_gemm', **NO_T2, **G8)),
    'no_gemm16': (plan(dense='two_gemms', qside='scorer_gemm', head='tsum+packed', **NO_T2),
                  plan(dense='two_gemms', qside='scorer_gemm', head='tsum+packed', **NO_T2, **G8)),
    'din_v1': (plan(din='k_din_scores<0,1>x4', **NO_DD), plan(cat='k_cat_attn2g<8,8>', din='k_din_scores<1,1>x4', **NO_DD)),
    'no_din16': (plan(din='k_din_scores<0,0>x4', **NO_DD), plan(cat='k_cat_attn2g<8,8>', din='k_din_scores<1,0>x4', **NO_DD)),
    'augru_h16': (plan(augru='k_augru_h16', **NO_DD), plan(augru='k_augru_h16', **NO_DD, **G8)),
    'cat_v1': (plan(cat='k_cat_attn', **NO_T2), plan(cat='k_cat_attn', din='k_din_x_16', **NO_T2)),
    'no_cat_group': (plan(**SHADOW), plan(din='k_din_x_16')),
    'no_head_tables': (plan(head='plain', **NO_T2), plan(head='plain', **NO_T2, **G8)),
    'no_head_fused': (plan(head='tables+k_head_finish', **NO_T2), plan(head='tables+k_head_finish', **NO_T2, **G8)),
    'din_rows16': (plan(din='k_din_x_16'), plan(**G8)),
}
FP32 = dict(dense='two_gemms', qside='scorer_gemm', augru='k_recur_fp32', head='tsum+packed', **NO_DD)
CASES = [
    # (name, traits, call, expected, source)
    ('flagship obs hint 1771', traits(), call(4096, 1, hint=1771), plan(**SHADOW), 'code'),
    ('flagship obs no hint', traits(), call(4096, 1), plan(), 'code'),
    ('flagship obs hint 4096', traits(), call(4096, 1, hint=4096), plan(), 'code'),
    ('flagship reward g8', traits(), call(32768, 8), plan(augru='k_augru_x_64', **G8), 'code'),
    ('flagship reward g9', traits(), call(36864, 9), plan(cat='k_cat_attn2g<9>', din='k_din_x_16', augru='k_augru_x_64'), 'code'),
    ('default R96 g1 hint 32', traits(), call(96, 1, hint=32), plan(**SHADOW), 'trace'),
    ('default R96 g1', traits(), call(96, 1), plan(**SHADOW), 'trace'),
    ('default R192 g8', traits(), call(192, 8), plan(**G8), 'code'),
    ('default R192 g8 rows32', traits(), call(192, 8, pin=32), plan(**G8), 'trace'),
    ('default R192 g8 rows64', traits(), call(192, 8, pin=64), plan(augru='k_augru_x_64', **G8), 'trace'),
    ('default R189 g9 rows64', traits(), call(189, 9, pin=64), plan(cat='k_cat_attn2g<9>', din='k_din_x_16', augru='k_augru_x_64'), 'trace'),
    ('default R96 g1 rows64', traits(), call(96, 1, pin=64), plan(), 'code'),       # the pin keeps the shadow plane away, the tiles stay 32 rows
    ('fp32 R96 g1', traits(fp32=True), call(96, 1, hint=32), plan(din='k_din_scores<0,0>x4', **FP32), 'trace'),
    ('fp32 R192 g8', traits(fp32=True), call(192, 8, pin=32), plan(cat='k_cat_attn2g<8,8>', din='k_din_scores<1,0>x4', **FP32), 'trace'),
    ('fp32 R189 g9', traits(fp32=True), call(189, 9, pin=64), plan(cat='k_cat_attn2g<9>', din='k_din_scores<1,0>x3', **FP32), 'trace'),
    ('mirror armed, obs given', traits(), call(96, 1, hint=32, mirror=True), plan(head='tsum+k_gemm_h16+mirror', **NO_T2), 'code'),
    ('carried partition', traits(), call(96, 1, carried=True), plan(dedup='carried', **SHADOW), 'trace'),
    ('Cn 24 g1', traits(Cn=24), call(96, 1, hint=32), plan(cat='k_cat_attn2<24,false>'), 'trace'),
    ('Cn 24 g8', traits(Cn=24), call(192, 8, pin=32), plan(**G8), 'trace'),
    ('Cn 25 g1', traits(Cn=25), call(96, 1, hint=32), plan(cat='k_cat_attn', head='tables+k_head_finish', **NO_T2), 'trace'),
    ('Cn 25 g8', traits(Cn=25), call(192, 8, pin=32), plan(cat='k_cat_attn', din='k_din_x_16', head='tables+k_head_finish', **NO_T2), 'trace'),
    ('U 144 g1', traits(U=144), call(96, 1, hint=32), plan(dense='two_gemms', qside='scorer_gemm', **NO_T2), 'code'),
    ('U 144 g8', traits(U=144), call(192, 8), plan(dense='two_gemms', qside='scorer_gemm', **NO_T2, **G8), 'code'),
    ('U 160 g1', traits(U=160), call(96, 1, hint=32), plan(dense='two_gemms', qside='scorer_gemm', **NO_T2), 'trace'),
] + [(o + ' g1', traits(o), call(96, 1, hint=32), BY_OPT[o][0], 'trace') for o in OPTS] + [
    (o + ' g8', traits(o), call(192, 8, pin=32), BY_OPT[o][1], 'trace') for o in OPTS]
# test_augru_shadow_mapping.py::test_room_rule, the same values: (hint, R, S, n_cu) -> fits
ROOM = [((1771, 4096, 2, 256), 1), ((0, 4096, 2, 256), 0), ((4096, 4096, 2, 256), 0), ((0, 2720, 2, 256), 1), ((0, 2721, 2, 256), 0),
        ((2720, 2752, 2, 256), 1), ((2721, 2752, 2, 256), 0), ((0, 64, 2, 256), 1), ((9999, 64, 2, 256), 1)]
# augru_tiles(rows64, rows, group) and augru_rows64(pin, R, group, S, n_cu): the grids augru_x_launch had and the automatic rule
TILES = [((0, 4096, 1), 128), ((0, 33, 1), 2), ((1, 32768, 8), 512), ((1, 192, 8), 3), ((1, 36864, 9), 586), ((1, 189, 9), 3), ((1, 63, 9), 1),
         ((1, 72, 9), 2), ((1, 1704, 8), 27)]
ROWS64 = [((0, 32768, 8, 2, 256), 1), ((0, 16384, 8, 2, 256), 1), ((0, 16320, 8, 2, 256), 0), ((0, 36864, 9, 2, 256), 1), ((0, 192, 8, 2, 256), 0),
          ((64, 192, 8, 2, 256), 1), ((64, 96, 8, 2, 256), 0), ((64, 189, 9, 2, 256), 1), ((32, 32768, 8, 2, 256), 0), ((64, 4096, 1, 2, 256), 0)]


def _cxx():
    return next((c for c in ('g++', 'c++', 'clang++') if shutil.which(c)), None)


def _program():
    def init(kind, d):
        return '%s{}; %s' % (kind, ' '.join('x.%s = %s;' % (k, str(v).lower() if isinstance(v, bool) else v) for k, v in d.items()))
    body = []
    for name, t, c, _, _ in CASES:
        body.append('    { DienTraits x = %s const DienTraits t = x; { DienCall x = %s show("%s", t, x); } }' % (init('DienTraits', t), init('DienCall', c), name))
    for args, _ in ROOM:
        body.append('    printf("room %%d\\n", (int)augru_shadow_room(%d, %d, %d, %d));' % args)
    for args, _ in TILES:
        body.append('    printf("tiles %%lld\\n", (long long)augru_tiles(%d, %d, %d));' % args)
    for args, _ in ROWS64:
        body.append('    printf("rows64 %%d\\n", (int)augru_rows64(%d, %d, %d, %d, %d));' % args)
    return ('#include "dien_plan.hpp"\nusing namespace rl4rs;\n'
            'static void show(const char* name, const DienTraits& t, const DienCall& c) {\n'
            '    char buf[512];\n    dien_plan_str(dien_plan(t, c), buf, sizeof(buf));\n    printf("plan %s | %s\\n", name, buf);\n}\n'
            'int main() {\n' + '\n'.join(body) + '\n    return 0;\n}\n')


def test_plan_table_room_rule_and_tiles(tmp_path):
    cxx = _cxx()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    src, exe = tmp_path / 'plan_main.cpp', tmp_path / 'plan_main'
    src.write_text(_program())
    r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Wextra', '-Werror', '-I', CSRC, str(src), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    plans = [ln[5:].split(' | ') for ln in out if ln.startswith('plan ')]
    assert [p[0] for p in plans] == [c[0] for c in CASES]
    wrong = []
    for (name, text), (_, _, _, want, source) in zip(plans, CASES):
        got = dict(tok.split('=', 1) for tok in text.split())
        if got != want:
            wrong.append((name, source, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}))
    assert not wrong, wrong
    assert [int(ln.split()[1]) for ln in out if ln.startswith('room ')] == [w for _, w in ROOM]
    assert [int(ln.split()[1]) for ln in out if ln.startswith('tiles ')] == [w for _, w in TILES]
    assert [int(ln.split()[1]) for ln in out if ln.startswith('rows64 ')] == [w for _, w in ROWS64]
