"""The DIEN scorer forward off its default configuration: the case table, the input builders and the bars shared by
tests/test_dien_shapes_host.py (CPU: plans, attainability of the bars in float32, duplicate counts, teeth) and
tests/test_gpu_dien_shapes.py (every row of every forward form against the fp64 oracle).  No GPU import here.

A case is (maxlen L, category_feature_num Cn, hidden_units U, dense_feature_num Dn, seq_num S, class_num K); what it is there to
enter is written beside it.  Every case runs three forward shapes, the smallest at which the forms differ:

    f1   group 1, R = 45    one full and one ragged 32-row tile
    f8   group 8, R = 128   16 groups: the 64-row AUGRU form is admissible (R % 64 == 0)
    f9   group 9, R = 126   14 groups = two 7-group tiles of the 64-row form, with obs_last

Duplicate row groups (runs of equal slot entries holding repeated templates, as tests/test_gpu_tier2_active_rows.py builds them):
f1 20 of 45 groups, f8 9 of 16, f9 7 of 14 - the same run patterns in every case, so the same counts (DUPLICATES below, checked
with that file's numpy rule).

The bars are the standing ones of tests/test_gpu_dien.py.  FLOAT32 below holds, per case, what OracleDien in float32 differs
from OracleDien in float64 on the case's own inputs (worst of the three shapes, measured by tests/test_dien_shapes_host.py, which
asserts a quarter of each bar): the bars can be met in float32 at every width in the table."""
import functools

import numpy as np

BASE = {"maxlen": 64, "batch_size": 8, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
        "category_feature_num": 21, "category_hash_size": 600, "seq_num": 2, "emb_size": 128,
        "page_items": 9, "hidden_units": 128, "max_steps": 9, "action_emb_size": 32}
E, NH2, OBS_DIM, ATT_H1 = 128, 256, 256, 64
NSLOTS = 16
CAP = 64                                         # ROW_DEDUP_CAP of rl4rs_amd/csrc/row_dedup.hpp

# name -> (L, Cn, U, Dn, S, K)
CASES = {
    # S = 3: the pair's two-launch fallback (q-side term 192 wide), three slot rows in the dedup.  Dn = 61: scalar row_words_equal
    # at group 1, 16-byte path at group 8 (8 * 61 words), dense k-tail without vector loads.  k_cat_attn2<24,false> at group 1,
    # k_cat_attn2g at group 8 / 9.  K = 3.
    'A': (33, 13, 96, 61, 3, 3),
    # S = 1: q-side term 64 wide.  Cn < 10: the query is the mean over all 7 ids.  Cn < 11: no group category kernel, the per-row
    # kernel runs with its group argument.  Chain at N1 = 32.
    'B': (64, 7, 32, 432, 1, 2),
    # Cn > 24: k_cat_attn, tables + k_head_finish, tier off, expand front.  Dn = 40: one k-tile.
    'C': (16, 32, 128, 40, 2, 2),
    # U > 128: two GEMMs, scorer_gemm, tier off, expand front, no shadow.  Another Fld (800).
    'D': (64, 21, 160, 432, 2, 2),
    # every upper limit at once: S = 4, Cn = 24 (the last with tsum, the tier and the group kernels), K = 8.  Chain at N1 = 64.
    'E': (64, 24, 64, 100, 4, 8),
    # the shadow plane (k_din_xq, k_augru_xs) away from U 128 / Dn 432 / L 64, its dense tile with vec off; a distinct hint is set
    'F': (8, 21, 96, 61, 2, 2),
    # Cn = 11: the smallest that takes the group kernels.  Dn % 4 == 0 but % 16 != 0: vector loads with a k-tail.
    'G': (64, 11, 128, 436, 2, 2),
    # the lower limits: one step, one category id, a 3-wide dense row; the widest tower tested
    'H': (1, 1, 256, 3, 1, 2),
}
# name -> (group, R, runs of template letters)
SHAPES = {
    'f1': (1, 45, ['ABACC'] * 5 + ['AAAA'] * 2 + ['ABCD', 'ABAAB', 'AAB']),
    'f8': (8, 128, ['ABAAB', 'AAB', 'ABBA', 'AAAA']),
    'f9': (9, 126, ['ABAAB', 'AAB', 'AAAA', 'AB']),
}
# shape -> (groups, duplicates among them): between a third and two thirds
DUPLICATES = {'f1': (45, 20), 'f8': (16, 9), 'f9': (14, 7)}

BARS = {'h2': 5e-6, 'h1': 2e-6, 'scores': 2e-6, 'cat': 2e-6, 'query': 1e-6, 'dense': 2e-5, 'obs': 5e-5, 'obs_last': 5e-5, 'prob': 5e-6}

# case -> init_dien_weights(seed, emb_scale, bias_noise) and the scale of the dense rows: the values of tests/test_gpu_dien.py
INIT = dict((name, dict(seed=5 + i, emb_scale=0.5, bias_noise=0.2, dense_scale=3.0)) for i, name in enumerate(sorted(CASES)))

# OracleDien float32 against float64, worst of f1 / f8 / f9, as tests/test_dien_shapes_host.py::test_bars_attainable_in_float32
# prints it (bar / 4 is asserted); 'dense' is relative to max(1, |ref|); h1, the first-GRU cache, is compared in case A only
FLOAT32 = {
    'A': dict(h2=3.3e-07, h1=2.6e-07, score=6.1e-08, cat=5.6e-08, query=5.4e-08, dense=4.2e-07, obs=8.8e-07, obs_last=7.2e-07, prob=1.9e-07),
    'B': dict(h2=2.6e-07, score=3.1e-08, cat=7.5e-08, query=4.9e-08, dense=5.0e-07, obs=1.6e-06, obs_last=1.6e-06, prob=2.7e-07),
    'C': dict(h2=5.1e-07, score=4.9e-08, cat=4.7e-08, query=4.2e-08, dense=5.1e-07, obs=1.0e-06, obs_last=1.0e-06, prob=2.4e-07),
    'D': dict(h2=3.2e-07, score=5.1e-08, cat=4.9e-08, query=3.9e-08, dense=5.7e-07, obs=2.5e-06, obs_last=1.9e-06, prob=4.2e-07),
    'E': dict(h2=3.8e-07, score=3.9e-08, cat=4.8e-08, query=5.1e-08, dense=3.1e-07, obs=1.3e-06, obs_last=1.2e-06, prob=8.9e-08),
    'F': dict(h2=2.6e-07, score=3.8e-08, cat=5.4e-08, query=4.3e-08, dense=3.8e-07, obs=1.5e-06, obs_last=1.3e-06, prob=2.3e-07),
    'G': dict(h2=4.4e-07, score=6.1e-08, cat=5.3e-08, query=4.6e-08, dense=7.0e-07, obs=2.9e-06, obs_last=1.9e-06, prob=2.8e-07),
    'H': dict(h2=4.0e-08, score=3.8e-08, cat=0.0, query=0.0, dense=6.2e-07, obs=1.3e-06, obs_last=1.1e-06, prob=2.4e-07),
}


def config(case, **extra):
    L, Cn, U, Dn, S, K = CASES[case]
    return dict(BASE, maxlen=L, category_feature_num=Cn, hidden_units=U, dense_feature_num=Dn, seq_num=S, class_num=K, **extra)


def columns(case):
    """-> (S * 256, U, E, Fld): the widths of the all-feature row of the table form [AUGRU finals | dense tower | pooled category]"""
    _, _, U, _, S, _ = CASES[case]
    return S * NH2, U, E, S * NH2 + U + E


@functools.lru_cache(maxsize=None)
def weights(case):
    from rl4rs_amd.nets.dien import init_dien_weights
    i = INIT[case]
    return init_dien_weights(config(case), seed=i['seed'], emb_scale=i['emb_scale'], bias_noise=i['bias_noise'])


@functools.lru_cache(maxsize=None)
def histories(case):
    """[NSLOTS, S, L] ids as test_gpu_scorer_boundary._histories takes them: leading padding (half the history, at least one step)
    on a third of input 0, every second row of input 1 all padding, no zero id elsewhere"""
    L, _, _, _, S, _ = CASES[case]
    rs = np.random.RandomState(1000 + ord(case))
    seq = rs.randint(1, 284, size=(NSLOTS, S, L)).astype(np.int32)
    seq[: NSLOTS // 3, 0, : max(1, L // 2)] = 0
    if S > 1:
        seq[::2, 1, :] = 0
    return seq


def template(case, group, rs):
    """one row group: dense [group, Dn], cat [group, Cn]; the rows of a group of complete states share every id but the last"""
    _, Cn, _, Dn, _, _ = CASES[case]
    dense = np.abs(rs.randn(group, Dn) * INIT[case]['dense_scale']).astype(np.float32)
    cat = rs.randint(0, BASE['category_hash_size'], size=(group, Cn)).astype(np.int32)
    tail = min(Cn, 11)
    cat[:, Cn - tail:] = rs.randint(0, 284, size=(group, tail))
    if group > 1:
        cat[:, :Cn - 1] = cat[0, :Cn - 1]
    return dense, cat


def groups(case, runs, group, rs):
    """tests/test_gpu_tier2_active_rows.py::_groups at (Cn, Dn, S, group): run r reads slot r % NSLOTS of input 0, slot r % 2 of
    input 1 and slot (r + 5 s) % NSLOTS of a further input s, so neighbouring runs never share their slot entries
    -> slots [S, n], dense [n * group, Dn], cat [n * group, Cn], letters [n] (run index, template letter)"""
    S = CASES[case][4]
    sl, dn, ct, who = [], [], [], []
    for r, letters in enumerate(runs):
        tpl = {}
        for ch in letters:
            if ch not in tpl:
                tpl[ch] = template(case, group, rs)
            sl.append([r % NSLOTS, r % 2] + [(r + 5 * s) % NSLOTS for s in range(2, 4)])
            dn.append(tpl[ch][0])
            ct.append(tpl[ch][1])
            who.append((r, ch))
    slots = np.ascontiguousarray(np.array(sl, dtype=np.int32).T[:S])
    return slots, np.concatenate(dn), np.concatenate(ct), who


def expected_partition(slots, cat, dense, group):
    """The duplicate rule of row_dedup.hpp in numpy (tests/test_gpu_tier2_active_rows.py::_expected, natural order, any number of
    slot rows) -> (n_active, rep[n_groups])"""
    ng = slots.shape[1]
    key = [(cat[g * group:(g + 1) * group].tobytes(), dense[g * group:(g + 1) * group].view(np.uint32).tobytes()) for g in range(ng)]
    rep = np.arange(ng)
    for g in range(ng):
        back = 0
        while back < CAP - 1 and g - 1 - back >= 0 and tuple(slots[:, g - 1 - back]) == tuple(slots[:, g]):
            back += 1
        for k in range(back, 0, -1):
            if key[g - k] == key[g]:
                rep[g] = g - k
                break
    for g in range(ng):
        r = rep[g]
        while rep[r] != r:
            r = rep[r]
        rep[g] = r
    return int((rep == np.arange(ng)).sum()), rep


@functools.lru_cache(maxsize=None)
def inputs(case, shape):
    """-> dict: group, R, slots [S, R / group], dense, cat, seq [R, S, L] (the history of every row), who, n_active, rep"""
    group, R, runs = SHAPES[shape]
    rs = np.random.RandomState(100 * ord(case) + group)
    slots, dense, cat, who = groups(case, runs, group, rs)
    assert slots.shape[1] * group == R
    hist = histories(case)
    seq_group = np.stack([hist[slots[s], s] for s in range(slots.shape[0])], axis=1)          # [n, S, L]
    n_active, rep = expected_partition(slots, cat, dense, group)
    return dict(group=group, R=R, slots=slots, dense=dense, cat=cat, seq=np.repeat(seq_group, group, axis=0), who=who,
                n_active=n_active, rep=rep)


def all_feature(parts, case):
    """the table form's all-feature row from the oracle's parts: [h2_0 .. h2_{S-1} | dense tower | pooled category part]"""
    S = CASES[case][4]
    return np.concatenate([parts['h2_%d' % s] for s in range(S)] + [parts['dense_feat'], parts['cat_feat'][:, :E]], axis=1)


def oracle_outputs(case, shape, dtype, w=None):
    """OracleDien on the case's inputs -> dict(all_feature [R, Fld], scores [S, R, L], query, h1_0 [R, L, E], obs, prob, obs_last)"""
    from oracle.dien import OracleDien, _elu, _softmax
    S = CASES[case][4]
    x = inputs(case, shape)
    orc = OracleDien(weights(case) if w is None else w, config(case), dtype)
    allf, parts = orc.features(x['seq'], x['dense'], x['cat'], return_parts=True)
    obs = _elu(allf @ orc.w['obs_w'] + orc.w['obs_b'])                      # OracleDien.obs / reward_probs on the features at hand
    prob = _softmax(obs @ orc.w['out_w'] + orc.w['out_b'])[:, 1]
    g = x['group']
    return dict(all_feature=all_feature(parts, case), scores=np.stack([parts['score_%d' % s] for s in range(S)]), query=parts['query'],
                h1_0=parts['h1_0'], obs=obs, prob=prob, obs_last=obs[g - 1::g])


@functools.lru_cache(maxsize=None)
def reference(case, shape):
    """the fp64 oracle, computed once per (case, shape) and shared; nobody writes to it"""
    out = oracle_outputs(case, shape, np.float64)
    for v in out.values():
        v.setflags(write=False)
    return out


def errors(got, ref, case, offsets=None):
    """got / ref: dicts as oracle_outputs returns them (got may lack h1_0 / obs_last) -> {quantity: (worst |got - ref|, bar)}; the
    all-feature row is split at the case's own offsets (`offsets` = (end of the AUGRU columns, end of the dense columns) overrides
    them: the teeth test splits at the default configuration's 512 / 640)"""
    nseq, U, _, Fld = columns(case)
    a, b = (nseq, nseq + U) if offsets is None else offsets
    S = CASES[case][4]
    ga, ra = np.asarray(got['all_feature'], dtype=np.float64), ref['all_feature']
    assert ga.shape == ra.shape == (ra.shape[0], Fld), (ga.shape, ra.shape, Fld)
    out = {}
    # the split under test: columns [0, a) as S AUGRU states, [a, a + U) against the oracle's dense tower, [b, b + E) against its
    # pooled category part
    gs = ga[:, :a]
    for s in range(S):
        out['h2_%d' % s] = (_worst(gs[:, s * NH2:(s + 1) * NH2], ra[:, s * NH2:(s + 1) * NH2]), BARS['h2'])
    rd, rc = ra[:, nseq:nseq + U], ra[:, nseq + U:]
    gd, gc = ga[:, a:a + U], ga[:, b:b + E]
    out['dense'] = (_worst(gd, rd), BARS['dense'] * max(1.0, np.abs(rd).max()))
    out['cat'] = (_worst(gc, rc), BARS['cat'])
    for s in range(S):
        out['score_%d' % s] = (_worst(got['scores'][s], ref['scores'][s]), BARS['scores'])
    out['query'] = (_worst(got['query'], ref['query']), BARS['query'])
    out['obs'] = (_worst(got['obs'], ref['obs']), BARS['obs'])
    out['prob'] = (_worst(got['prob'], ref['prob']), BARS['prob'])
    for name in ('h1_0', 'obs_last'):
        if got.get(name) is not None:
            out[name] = (_worst(got[name], ref[name]), BARS['h1' if name == 'h1_0' else 'obs_last'])
    return out


def _worst(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if x.shape != y.shape:                         # a split at the wrong offsets may run off the row: as wrong as can be
        return np.inf
    d = np.abs(x - y)
    return float(np.inf if not np.isfinite(d).all() else d.max())


def report(tag, errs):
    return '%s: %s' % (tag, '  '.join('%s %.3g/%.3g' % (k, e, bar) for k, (e, bar) in errs.items()))


def misses(errs, fraction=1.0):
    return dict((k, (e, bar)) for k, (e, bar) in errs.items() if not e < bar * fraction)


# ---------------------------------------------------------------------------------------------------------------- the plans
def plan_tokens(case, shape, arm='', pin=0, fp32=False, carried=False):
    """What the table claims dien_plan gives for this case, forward shape, handle option and AUGRU row pin, as the tokens of
    dien_plan_str.  Written from the case's numbers alone; tests/test_dien_shapes_host.py holds rl4rs_amd/csrc/dien_plan.hpp to it,
    tests/test_gpu_dien_shapes.py holds DeviceDien.last_plan() to it."""
    L, Cn, U, Dn, S, K = CASES[case]
    group = SHAPES[shape][0]
    tier_shape = Cn <= 24 and U <= 128                      # the second tier: k_cat_attn2 with its tsum, the chained dense tower
    p = dict(tier2='1' if tier_shape else '0', shadow='0', dedup='k_row_dedup', prob='1')
    if Cn > 24:
        p['cat'] = 'k_cat_attn'
    elif group in (8, 9) and Cn >= 11:
        p['cat'] = 'k_cat_attn2g<8,8>' if group == 8 else 'k_cat_attn2g<9>'
    else:
        p['cat'] = 'k_cat_attn2<21,true>' if Cn == 21 else 'k_cat_attn2<24,false>'
    p['dense'], p['qside'] = ('pair', 'in_pair') if U <= 128 else ('two_gemms', 'scorer_gemm')
    p['din'] = 'k_din_x_auto' if group == 1 else 'k_din_x_16'
    p['augru'] = 'k_augru_x_64' if (pin == 64 and group != 1) else 'k_augru_x_32'
    p['head'] = 'tsum+k_gemm_h16' if Cn <= 24 else 'tables+k_head_finish'
    ncol = S * NH2 + U + E
    # group 1: the head GEMM gathers from the representative's row (lazy); the observation is handed out at group 8 / 9: behind
    p['expand'] = ('%s:%d' % ('lazy' if group == 1 else 'behind', ncol)) if tier_shape else 'front:%d' % (S * NH2)
    if fp32:
        p.update(tier2='0', dedup='none', expand='none:0', dense='two_gemms', qside='scorer_gemm', augru='k_recur_fp32',
                 din='k_din_scores<%d,0>x%d' % (int(group != 1), 3 if group == 9 else 4))
        if Cn <= 24:
            p['head'] = 'tsum+packed'
        return p
    if arm == 'no_gemm_group':
        assert tier_shape
        p.update(dense='chain', qside='mapped_k_gemm_h16')
    elif arm == 'dense_fork':
        p.update(tier2='0', dense=('chain' if U <= 128 else 'two_gemms') + '@side', qside='scorer_gemm', expand='front:%d' % (S * NH2))
    elif arm == 'no_tier2_rows':
        p.update(tier2='0', expand='front:%d' % (S * NH2))
    elif arm == 'no_row_dedup':
        p.update(tier2='0', dedup='none', expand='none:0')
    else:
        assert arm == ''
        if tier_shape and group == 1 and Cn == 21 and S <= 2 and pin != 64:      # case F: the shadow plane
            p.update(shadow='1', cat='shadow', dense='shadow', qside='in_k_din_xq', din='k_din_xq', augru='k_augru_xs')
    if carried and p['dedup'] != 'none':
        p['dedup'] = 'carried'
    return p


def pair_one_grid(case):
    """launch_gemm_h16_pair issues ONE grid (k_gemm_h16_pair) only when both problems are one block of columns wide
    (gemm.hip::gemm_h16_route: ny = ((N + 31) / 32 + 3) / 4 == 1, i.e. N <= 128; the q-side term is S * 64 wide) and load their rows
    alike (the dense rows take 16-byte loads only at Dn % 4 == 0, the query rows always do)"""
    _, _, U, Dn, S, _ = CASES[case]
    ny = ((S * ATT_H1 + 31) // 32 + 3) // 4
    return U <= 128 and ny == 1 and Dn % 4 == 0
