"""Row dedup of the fp16x2 DIEN scorer: k_row_dedup finds the row groups of a forward that are bit-identical in
cache slots, category ids and dense values, k_din_x / k_augru_x score one representative per set, k_row_expand copies its
AUGRU states and attention scores to the duplicates.  Everything is pinned against scorer_kernels='no_row_dedup' BIT FOR BIT
(observation, click probability, all-feature buffer, attention scores), and the number of scored groups against the count the
duplicate rule gives in numpy - without that second check the first would pass with nothing deduplicated."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CFG = {"maxlen": 64, "batch_size": 8, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
       "category_feature_num": 21, "category_hash_size": 3000, "seq_num": 2, "emb_size": 128,
       "page_items": 9, "hidden_units": 128, "max_steps": 9, "action_emb_size": 32}
CAP = 64            # ROW_DEDUP_CAP of rl4rs_amd/csrc/row_dedup.hpp: every run built here is shorter


@functools.lru_cache(maxsize=None)
def _weights(L):
    from rl4rs_amd.nets.dien import init_dien_weights
    return init_dien_weights(dict(CFG, maxlen=L), seed=9, emb_scale=0.5, bias_noise=0.2)


def _histories(B, L, rs):
    """[B, 2, L] ids: a third of the rows of input 0 start with padding (half the history, at least one step), every second
    row of input 1 is all padding, the rest have no zero id at all."""
    seq = rs.randint(1, 284, size=(B, 2, L)).astype(np.int32)
    seq[: B // 3, 0, : max(1, L // 2)] = 0
    seq[::2, 1, :] = 0
    return seq


def _template(group, rs):
    dense = np.abs(rs.randn(group, 432) * 3).astype(np.float32)
    cat = rs.randint(0, CFG['category_hash_size'], size=(group, 21)).astype(np.int32)
    cat[:, 10:] = rs.randint(0, 284, size=(group, 11))
    return dense, cat


def _expected(slots, cat, dense, group, order=None):
    """The duplicate rule in numpy: positions in processing order, runs of consecutive positions with equal slot entries,
    inside a run the first group with the same category ids and the same dense BIT PATTERNS is the representative.
    -> (n_active, rep[n_groups])."""
    ng = slots.shape[1]
    order = np.arange(ng) if order is None else np.asarray(order)
    rep = np.arange(ng)
    seen, prev = {}, None
    for p in range(ng):
        g = int(order[p])
        key_s = tuple(slots[:, g])
        if key_s != prev:
            seen, prev, run = {}, key_s, 0
        run += 1
        assert run < CAP
        key = (cat[g * group:(g + 1) * group].tobytes(), dense[g * group:(g + 1) * group].view(np.uint32).tobytes())
        rep[g] = seen.setdefault(key, g)
    return int((rep == np.arange(ng)).sum()), rep


def _case_groups(pattern_cycles, group, rs):
    """Groups laid out run after run: `pattern_cycles` = list of runs, a run = string of template letters ('ABA': three groups,
    the third equal to the first).  Every run gets its own slot of input 0; input 1 alternates between slots 0 and 1 per run.
    -> slots [2, n], dense [n * group, 432], cat [n * group, 21]"""
    s0, s1, dn, ct = [], [], [], []
    for r, letters in enumerate(pattern_cycles):
        tpl = {}
        for ch in letters:
            if ch not in tpl:
                tpl[ch] = _template(group, rs)
            s0.append(r)
            s1.append(r % 2)
            dn.append(tpl[ch][0])
            ct.append(tpl[ch][1])
    return np.array([s0, s1], dtype=np.int32), np.concatenate(dn), np.concatenate(ct)


def _case1(rs):
    """96 single-row groups: runs of 1, 2, 3 and 5 (A B A inside), then three adjacent pairs that must NOT match - one dense
    element one ulp apart, +0 against -0, equal in everything but the slot of the second input - and a tail of short runs."""
    runs = ['A', 'AA', 'ABA', 'ABAAB', 'AAAAA'] * 5 + ['AB', 'AB', 'AB'] + ['AA', 'ABA'] * 2
    slots, dense, cat = _case_groups(runs, 1, rs)
    assert slots.shape[1] == 96
    base = 80
    dense[base + 1], cat[base + 1] = dense[base], cat[base]
    dense[base + 1, 7] = np.nextafter(dense[base, 7], np.float32(np.inf))         # one ulp
    dense[base + 3], cat[base + 3] = dense[base + 2], cat[base + 2]
    dense[base + 2, 11], dense[base + 3, 11] = 0.0, -0.0                          # equal as numbers, not as bits
    dense[base + 5], cat[base + 5] = dense[base + 4], cat[base + 4]
    slots[1, base + 5] = 1 - slots[1, base + 4]                                   # the second input's slot differs
    return slots, dense, cat


def _forward(cfg, L, seq, R, group, dense, cat, slots, kernels, order=None, rows=(0,), want_dedup=True):
    """One handle, one forward per entry of `rows` (set_augru_rows) -> list of (obs, prob, all_feature, scores, n_active, rep)
    and the handle's profile labels."""
    import torch
    from rl4rs_amd.device import DeviceDien, DIEN_ALL_FEATURE, DIEN_SCORES, DIEN_N_ACTIVE, DIEN_ROW_REP
    nslots = seq.shape[0]
    net = DeviceDien(dict(cfg, maxlen=L, scorer_kernels=kernels), _weights(L), max_rows=R, max_slots=nslots)
    for s in range(2):
        net.encode(s, torch.from_numpy(np.ascontiguousarray(seq[:, s])).cuda(), 0)
    if order is not None:
        net.set_row_order(torch.from_numpy(np.asarray(order, dtype=np.int32)).cuda())
    sl = torch.from_numpy(np.ascontiguousarray(slots)).cuda()
    d, c = torch.from_numpy(dense).cuda(), torch.from_numpy(cat).cuda()
    outs = []
    for r in rows:
        net.set_augru_rows(r)
        obs, p = net.forward(R, group, d, c, sl, True, True)
        out = [obs.clone(), p.clone(), net.snapshot(DIEN_ALL_FEATURE, R)[:R].clone(), net.snapshot(DIEN_SCORES, R)[:, :R].clone()]
        if want_dedup and 'no_row_dedup' not in kernels:
            out += [int(net.snapshot(DIEN_N_ACTIVE, 0).item()), net.snapshot(DIEN_ROW_REP, R)[:R // group].cpu().numpy()]
        outs.append(out)
    labels = sorted(net.profile())
    net.check_status()
    net.close()
    return outs, labels


def _check(got, ref, expected):
    import torch
    for name, a, b in zip(('obs', 'prob', 'all_feature', 'scores'), got, ref):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), name
    n_exp, rep_exp = expected
    print('n_active', got[4], 'expected', n_exp, 'of', len(rep_exp))
    assert got[4] == n_exp
    assert np.array_equal(got[5], rep_exp)


def _both(L, seq, R, group, dense, cat, slots, extra='', order=None, rows=(0,)):
    cfg = dict(CFG, scorer_precision='fp16x2')
    on, labels_on = _forward(cfg, L, seq, R, group, dense, cat, slots, extra, order, rows)
    off, labels_off = _forward(cfg, L, seq, R, group, dense, cat, slots, ','.join(x for x in ('no_row_dedup', extra) if x), order, rows)
    assert any('k_row_expand' in k for k in labels_on) and not any('k_row_expand' in k for k in labels_off), (labels_on, labels_off)
    return on, off


def test_runs_patterns_and_near_misses():
    """Case 1: R = 96, one row per group, 32-row form, natural order.  n_active between 33 and 64: one full tile, one partial
    tile, one workgroup that leaves at once."""
    rs = np.random.RandomState(1)
    slots, dense, cat = _case1(rs)
    seq = _histories(int(slots[0].max()) + 1, 64, rs)
    exp = _expected(slots, cat, dense, 1)
    assert 32 < exp[0] <= 64
    on, off = _both(64, seq, 96, 1, dense, cat, slots)
    _check(on[0], off[0], exp)
    # the three near misses are all kept
    rep = on[0][5]
    for g in (80, 81, 82, 83, 84, 85):
        assert rep[g] == g, g


def test_row_order_brings_the_duplicates_together():
    """Case 2: the rows of case 1 scattered over the batch, with the processing order that puts the runs back together: the
    same n_active as case 1; and with no order set: fewer hits (the rule applied to the natural order), still bit-identical."""
    rs = np.random.RandomState(1)
    slots, dense, cat = _case1(rs)
    seq = _histories(int(slots[0].max()) + 1, 64, rs)
    n_case1 = _expected(slots, cat, dense, 1)[0]
    perm = np.random.RandomState(5).permutation(96)           # physical row i holds case-1 row perm[i]
    slots, dense, cat = np.ascontiguousarray(slots[:, perm]), dense[perm], cat[perm]
    order = np.argsort(perm).astype(np.int32)                  # position p -> the physical row that holds case-1 row p
    assert not np.array_equal(order, np.arange(96))
    exp = _expected(slots, cat, dense, 1, order)
    assert exp[0] == n_case1
    on, off = _both(64, seq, 96, 1, dense, cat, slots, order=order)
    _check(on[0], off[0], exp)
    exp_nat = _expected(slots, cat, dense, 1)
    assert exp[0] < exp_nat[0] <= 96
    on, off = _both(64, seq, 96, 1, dense, cat, slots)
    _check(on[0], off[0], exp_nat)


def test_all_rows_identical():
    """Case 3: R = 33, every row the same: one group is scored, 32 are copies."""
    rs = np.random.RandomState(3)
    slots, dense, cat = _case_groups(['A' * 33], 1, rs)
    seq = _histories(2, 64, rs)
    exp = _expected(slots, cat, dense, 1)
    assert exp[0] == 1
    on, off = _both(64, seq, 33, 1, dense, cat, slots)
    _check(on[0], off[0], exp)


def test_no_two_rows_alike():
    """Case 4: R = 96, shared slots but no duplicate: n_active = 96, the expansion has nothing to do."""
    rs = np.random.RandomState(4)
    slots, dense, cat = _case_groups(['ABC'] * 32, 1, rs)
    seq = _histories(32, 64, rs)
    exp = _expected(slots, cat, dense, 1)
    assert exp[0] == 96
    on, off = _both(64, seq, 96, 1, dense, cat, slots)
    _check(on[0], off[0], exp)


def test_reward_shaped_groups_in_both_row_tile_forms():
    """Case 5: R = 192 in 24 groups of 8 rows, 9 of them distinct (72 rows): the 64-row form gets one full workgroup, one
    partial one and one that leaves; the 32-row form two full, one partial, three that leave.  Both against 'no_row_dedup' and
    against each other, bit for bit."""
    import torch
    rs = np.random.RandomState(5)
    slots, dense, cat = _case_groups(['AAAA', 'ABAB', 'AAAA', 'ABBA', 'AAAA', 'AABA'], 8, rs)
    seq = _histories(6, 64, rs)
    exp = _expected(slots, cat, dense, 8)
    assert slots.shape[1] == 24 and exp[0] == 9
    on, off = _both(64, seq, 192, 8, dense, cat, slots, rows=(64, 32))
    for i in range(2):
        _check(on[i], off[i], exp)
    for a, b in zip(on[0][:4], on[1][:4]):
        assert torch.equal(a, b)


@pytest.mark.parametrize('extra', ['', 'no_gru_pad'])
def test_short_history_with_leading_padding(extra):
    """Case 6: maxlen = 16, histories with leading padding: the pad-slot instantiation of k_augru_x (default handle) and the
    plain one ('no_gru_pad') both read the active list."""
    rs = np.random.RandomState(6)
    slots, dense, cat = _case_groups(['A', 'AA', 'ABA', 'ABAAB'] * 6, 1, rs)
    R = slots.shape[1]
    seq = _histories(24, 16, rs)
    exp = _expected(slots, cat, dense, 1)
    assert exp[0] < R
    on, off = _both(16, seq, R, 1, dense, cat, slots, extra=extra)
    _check(on[0], off[0], exp)


@pytest.mark.parametrize('precision,extra', [('fp32', ''), ('fp16x2', 'din_v1')])
def test_option_is_a_no_op_on_other_kernel_selections(precision, extra):
    """Case 7: where k_din_x and k_augru_x are not both the selected kernels the forward issues what it always did: the same
    profile labels with and without 'no_row_dedup', equal outputs."""
    import torch
    rs = np.random.RandomState(7)
    slots, dense, cat = _case_groups(['A', 'AA', 'ABA'] * 6, 1, rs)
    R = slots.shape[1]
    seq = _histories(18, 64, rs)
    cfg = dict(CFG, scorer_precision=precision)
    a, la = _forward(cfg, 64, seq, R, 1, dense, cat, slots, extra, want_dedup=False)
    b, lb = _forward(cfg, 64, seq, R, 1, dense, cat, slots, ','.join(x for x in ('no_row_dedup', extra) if x), want_dedup=False)
    assert la == lb and not any('k_row_expand' in k for k in la), (la, lb)
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)


def _episode(tmp_path, seq, distinct, kernels):
    """One episode of offline_action replay, B = 64 -> (per-step observations and rewards, n_active of the last forward)"""
    import torch
    import rl4rs_amd
    from rl4rs_amd import synth
    from rl4rs_amd.device import DIEN_N_ACTIVE
    from rl4rs_amd.env.slate import SlateRecEnv, SlateState
    from rl4rs_amd.env.seqslate import SeqSlateRecEnv, SeqSlateState
    d = str(tmp_path)
    B, T = 64, 18 if seq else 9
    # 20 log lines for 64 envs: duplicates by construction; the all-distinct variant (is_eval, cache_size = B: every env its own
    # line) needs a log of at least B lines
    n_lines = B + 5 if distinct else 20
    text = synth.make_catalog_text(seed=4)
    synth.write_text(os.path.join(d, 'c.csv'), text)
    recs = synth.make_records(n_lines, pages=2 if seq else 1, seed=3, hash_size=2000, special_ids=synth.special_ids_from_text(text))
    synth.write_records(os.path.join(d, 'log.csv'), recs)
    cfg = {"maxlen": 64, "batch_size": B, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
           "category_feature_num": 21, "category_hash_size": 2000, "seq_num": 2, "emb_size": 128, "page_items": 9,
           "hidden_units": 128, "max_steps": T, "action_emb_size": 32, "sample_file": os.path.join(d, 'log.csv'),
           "iteminfo_file": os.path.join(d, 'c.csv'), "cache_size": B if distinct else 20, "model_seed": 3,
           "return_tensors": True, "scorer_kernels": kernels}
    if distinct:
        cfg['is_eval'] = True
    if seq:
        cfg['support_rllib_mask'] = True
        env = rl4rs_amd.make('SeqSlateRecEnv-v0', recsim=SeqSlateRecEnv(cfg, state_cls=SeqSlateState))
    else:
        env = rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))
    env.seed(11)
    obs = env.reset()
    out = [(obs['obs'] if isinstance(obs, dict) else obs).clone()]
    for t in range(T):
        obs, reward, done, info = env.step(env.offline_action)
        out.append((obs['obs'] if isinstance(obs, dict) else obs).clone())
        out.append(reward.clone())
    n_active = None
    if 'no_row_dedup' not in kernels:
        n_active = int(env.sim.model.device_net.snapshot(DIEN_N_ACTIVE, 0).item())
    return out, n_active


@pytest.mark.parametrize('kind', ['slate', 'seq', 'slate_distinct'])
def test_episode_replay_is_bit_identical(tmp_path, kind):
    """SlateRecEnv / SeqSlateRecEnv, 64 envs over a 20-line log, offline_action replay: every observation and reward equal to
    the 'no_row_dedup' run; duplicates survive replay (Slate: n_active < B at the last forward); the all-distinct variant
    (is_eval, cache_size = B, a log of B + 5 lines) scores every env."""
    import torch
    seq, distinct = kind == 'seq', kind == 'slate_distinct'
    os.makedirs(str(tmp_path / 'a'))
    os.makedirs(str(tmp_path / 'b'))
    on, n_active = _episode(tmp_path / 'a', seq, distinct, '')
    off, _ = _episode(tmp_path / 'b', seq, distinct, 'no_row_dedup')
    assert len(on) == len(off)
    assert float(sum(x.abs().sum() for x in on[2::2])) > 0          # some reward was paid
    for t, (x, y) in enumerate(zip(on, off)):
        assert torch.equal(x, y), t
    print(kind, 'n_active of the last forward', n_active)
    if distinct:
        assert n_active == 64
    elif not seq:
        assert 1 <= n_active < 64
    else:
        assert 1 <= n_active <= 64
