"""Reward step: the state row is scored inside the reward forward.

  * k_augru_x's 64-row form with 9 rows per cache slot (63 positions per workgroup) against the 32-row form of the same
    forward, BIT FOR BIT: final states (all-feature buffer), attention scores, observation and probability of every row - at
    group counts that exercise the tile edges, with and without a row order, with the row dedup on and off, with duplicate
    patterns that end n_active inside a tile, and with short histories (leading padding).
  * rl4rs_dien_set_obs_last: obs[g] of the group-9 forward against the observation of a group-1 forward fed row 9g + 8 alone.
  * the 8-rows-per-slot form at the same counts still equals its 32-row form.
  * the stepper: a Slate episode and SeqSlate pages with the fold against config['no_reward_obs_fold'].
No tolerance anywhere: the change claims identical operation sequences per output element."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CFG = {"maxlen": 64, "batch_size": 8, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
       "category_feature_num": 21, "category_hash_size": 3000, "seq_num": 2, "emb_size": 128,
       "page_items": 9, "hidden_units": 128, "max_steps": 9, "action_emb_size": 32, "scorer_precision": "fp16x2"}
COUNTS = (1, 6, 7, 8, 13, 14, 15, 50)
CAP = 64            # ROW_DEDUP_CAP (row_dedup.hpp): no run built here is longer


@functools.lru_cache(maxsize=None)
def _weights(L):
    from rl4rs_amd.nets.dien import init_dien_weights
    return init_dien_weights(dict(CFG, maxlen=L), seed=9, emb_scale=0.5, bias_noise=0.2)


def _histories(n, L, rs):
    """[n, 2, L] ids: a third of the rows of input 0 start with padding, every second row of input 1 is all padding."""
    seq = rs.randint(1, 284, size=(n, 2, L)).astype(np.int32)
    seq[: n // 3, 0, : max(1, L // 2)] = 0
    seq[::2, 1, :] = 0
    return seq


def _groups(n_groups, group, pattern, rs):
    """n_groups groups of `group` rows laid out run after run (a run = consecutive groups that share their cache slots; equal
    letters inside a run = bit-identical groups).  'aba': runs with A B A inside; 'same': every group equal; 'none': shared
    slots, no two groups alike.  -> slots [2, n], dense [n * group, 432], cat [n * group, 21], number of histories"""
    runs = {'aba': ['ABA', 'AB', 'A', 'ABAAB', 'AA'], 'same': ['A' * n_groups], 'none': ['ABC']}[pattern]
    s0, s1, dn, ct = [], [], [], []
    r = 0
    while len(s0) < n_groups:
        tpl = {}
        for ch in runs[r % len(runs)]:
            if len(s0) == n_groups:
                break
            if ch not in tpl:
                dense = np.abs(rs.randn(group, 432) * 3).astype(np.float32)
                cat = rs.randint(0, CFG['category_hash_size'], size=(group, 21)).astype(np.int32)
                cat[:, 10:] = rs.randint(0, 284, size=(group, 11))
                tpl[ch] = (dense, cat)
            s0.append(r)
            s1.append(r % 2)
            dn.append(tpl[ch][0])
            ct.append(tpl[ch][1])
        r += 1
    return np.array([s0, s1], dtype=np.int32), np.concatenate(dn), np.concatenate(ct), max(r, 2)


def _n_active(slots, cat, dense, group, order=None):
    """The duplicate rule of row_dedup.hpp in numpy (processing order, runs of equal slots, first equal group represents)."""
    ng = slots.shape[1]
    order = np.arange(ng) if order is None else np.asarray(order)
    seen, prev, n = {}, None, 0
    for p in range(ng):
        g = int(order[p])
        key_s = tuple(slots[:, g])
        if key_s != prev:
            seen, prev = {}, key_s
        key = (cat[g * group:(g + 1) * group].tobytes(), dense[g * group:(g + 1) * group].view(np.uint32).tobytes())
        if key not in seen:
            seen[key] = g
            n += 1
    return n


def _run(L, seq, group, dense, cat, slots, kernels, order):
    """One handle: the forward in the 64-row and in the 32-row form (+ the observation of each group's last row), and a group-1
    forward of the last row of every group alone.  -> ({64: outs, 32: outs}, obs of the lone rows, n_active or None)"""
    import torch
    from rl4rs_amd.device import DeviceDien, DIEN_ALL_FEATURE, DIEN_SCORES, DIEN_N_ACTIVE
    ng = slots.shape[1]
    R = ng * group
    net = DeviceDien(dict(CFG, maxlen=L, scorer_kernels=kernels), _weights(L), max_rows=R, max_slots=seq.shape[0])
    for s in range(2):
        net.encode(s, torch.from_numpy(np.ascontiguousarray(seq[:, s])).cuda(), 0)
    if order is not None:
        net.set_row_order(torch.from_numpy(np.asarray(order, dtype=np.int32)).cuda())
    sl = torch.from_numpy(np.ascontiguousarray(slots)).cuda()
    d, c = torch.from_numpy(dense).cuda(), torch.from_numpy(cat).cuda()
    outs, n_active = {}, None
    for rows in (64, 32):
        net.set_augru_rows(rows)
        obs, p, last = net.forward(R, group, d, c, sl, True, True, want_obs_last=True)
        outs[rows] = dict(obs=obs.clone(), prob=p.clone(), last=last.clone(), all_feature=net.snapshot(DIEN_ALL_FEATURE, R)[:R].clone(),
                          scores=net.snapshot(DIEN_SCORES, R)[:, :R].clone())
        if 'no_row_dedup' not in kernels:
            n_active = int(net.snapshot(DIEN_N_ACTIVE, 0).item())
    net.set_augru_rows(0)
    lone, _ = net.forward(ng, 1, d[group - 1::group].contiguous(), c[group - 1::group].contiguous(), sl, True, False)
    lone = lone.clone()
    net.check_status()
    net.close()
    return outs, lone, n_active


def _check_forms(outs, lone, group):
    import torch
    a, b = outs[64], outs[32]
    for name in ('all_feature', 'scores', 'obs', 'prob', 'last'):
        assert torch.isfinite(a[name]).all(), name
        assert torch.equal(a[name], b[name]), name
    # the observation of each group's last row: the forward's own row, and the row scored on its own
    assert torch.equal(a['last'], a['obs'][group - 1::group])
    assert torch.equal(a['last'], lone)


@pytest.mark.parametrize('pattern', ['aba', 'same', 'none'])
@pytest.mark.parametrize('n_groups', COUNTS)
def test_group9_64_row_form_against_32_row_form(n_groups, pattern):
    """Groups of 9 rows: 1, 6, 7 (one exactly full tile of 63), 8 (one full tile plus one group), 13, 14 (two full tiles), 15, 50.
    Row dedup on (n_active against the rule in numpy: it ends inside a tile for most cases) and off, natural order and a
    processing order that scatters the runs."""
    rs = np.random.RandomState(100 + n_groups)
    slots, dense, cat, n_hist = _groups(n_groups, 9, pattern, rs)
    seq = _histories(n_hist, 64, rs)
    order = np.random.RandomState(7).permutation(n_groups).astype(np.int32)
    for kernels in ('', 'no_row_dedup'):
        for od in (None, order):
            outs, lone, n_active = _run(64, seq, 9, dense, cat, slots, kernels, od)
            _check_forms(outs, lone, 9)
            if not kernels:
                exp = _n_active(slots, cat, dense, 9, od)
                print(n_groups, pattern, 'order' if od is not None else 'natural', 'n_active', n_active, 'expected', exp)
                assert n_active == exp
                if pattern == 'same' and od is None:
                    assert n_active == 1
                if pattern == 'none':
                    assert n_active == n_groups


def test_group9_short_histories_with_leading_padding():
    """maxlen = 16, a third of the histories start with padding: the handle keeps a pad slot, the 64-row form reads the rows' own slots."""
    rs = np.random.RandomState(6)
    slots, dense, cat, n_hist = _groups(15, 9, 'aba', rs)
    seq = _histories(n_hist, 16, rs)
    for kernels in ('', 'no_row_dedup'):
        outs, lone, _ = _run(16, seq, 9, dense, cat, slots, kernels, None)
        _check_forms(outs, lone, 9)


@pytest.mark.parametrize('n_groups', COUNTS)
def test_group8_still_equals_its_32_row_form(n_groups):
    """The 8-rows-per-slot instantiation at the same group counts (its 64-row form is taken where R % 64 == 0: 8 groups; the
    forward falls to the 32-row form elsewhere) - and its last-row observation."""
    rs = np.random.RandomState(200 + n_groups)
    slots, dense, cat, n_hist = _groups(n_groups, 8, 'aba', rs)
    seq = _histories(n_hist, 64, rs)
    for kernels in ('', 'no_row_dedup'):
        outs, lone, _ = _run(64, seq, 8, dense, cat, slots, kernels, None)
        _check_forms(outs, lone, 8)


def test_group8_three_64_row_tiles_with_partial_activity():
    """24 groups of 8 (R = 192 = 3 x 64): the 64-row form of the existing instantiation with n_active inside a tile."""
    rs = np.random.RandomState(5)
    slots, dense, cat, n_hist = _groups(24, 8, 'aba', rs)
    seq = _histories(n_hist, 64, rs)
    outs, lone, n_active = _run(64, seq, 8, dense, cat, slots, '', None)
    _check_forms(outs, lone, 8)
    assert n_active == _n_active(slots, cat, dense, 8) and n_active * 8 % 64 != 0


# ---- the stepper ----------------------------------------------------------------------------------------------------------

def _episode(tmp_path, seq, distinct, fold, steps=None, conti=False, masked=False, pin=True):
    """Offline-action replay at B = 64 with the 64-row form pinned -> per-step observations, rewards, done flags, and the click
    probabilities of the last reward step's rows."""
    import torch
    import rl4rs_amd
    from rl4rs_amd import synth
    from rl4rs_amd.env.slate import SlateRecEnv, SlateState
    from rl4rs_amd.env.seqslate import SeqSlateRecEnv, SeqSlateState
    d = str(tmp_path)
    os.makedirs(d)
    B, T = 64, 18 if seq else 9
    n_lines = B + 5 if distinct else 20
    text = synth.make_catalog_text(seed=4)
    synth.write_text(os.path.join(d, 'c.csv'), text)
    recs = synth.make_records(n_lines, pages=2 if seq else 1, seed=3, hash_size=2000, special_ids=synth.special_ids_from_text(text))
    synth.write_records(os.path.join(d, 'log.csv'), recs)
    cfg = {"maxlen": 64, "batch_size": B, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
           "category_feature_num": 21, "category_hash_size": 2000, "seq_num": 2, "emb_size": 128, "page_items": 9,
           "hidden_units": 128, "max_steps": T, "action_emb_size": 32, "sample_file": os.path.join(d, 'log.csv'),
           "iteminfo_file": os.path.join(d, 'c.csv'), "cache_size": B if distinct else 20, "model_seed": 3,
           "return_tensors": True, "scorer_kernels": 'augru_rows64' if pin else '', "scorer_precision": "fp16x2"}
    if not fold:
        cfg['no_reward_obs_fold'] = True
    if distinct:
        cfg['is_eval'] = True
    if conti:
        cfg['support_conti_env'] = True
    if masked:
        cfg['support_rllib_mask'] = True
    if seq:
        env = rl4rs_amd.make('SeqSlateRecEnv-v0', recsim=SeqSlateRecEnv(cfg, state_cls=SeqSlateState))
    else:
        env = rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))
    env.seed(11)
    obs = env.reset()
    out = []
    for t in range(T):
        obs, reward, done, info = env.step(env.offline_action)
        o = obs['obs'] if isinstance(obs, dict) else obs
        out.append(o.clone())
        if isinstance(obs, dict):
            out.append(torch.as_tensor(obs['action_mask']).clone())
        out.append(torch.as_tensor(reward).clone())
        out.append(torch.as_tensor(np.asarray(done, dtype=np.int64)))
        if steps is not None and t + 1 >= steps:
            break
    out.append(env.sim._stepper.click_probs().clone())            # the last reward step's probabilities, every row
    assert env.sim._stepper.reward_rows() == (9 if (fold and pin) else 8)   # the path under test was the one taken
    return out


def _same(a, b):
    import torch
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.cpu(), y.cpu()), i


@pytest.mark.parametrize('kind', ['slate', 'slate_distinct', 'seq', 'seq_distinct'])
def test_episode_with_the_fold_equals_the_two_forward_order(tmp_path, kind):
    """One Slate episode (the reward on the last step) / one SeqSlate episode of two pages (a reward at each page end), B = 64 over
    20 log lines (duplicates) and all distinct: every observation, reward and done flag equal to the run with the switch off."""
    seq, distinct = kind.startswith('seq'), kind.endswith('distinct')
    on = _episode(tmp_path / 'a', seq, distinct, True)
    off = _episode(tmp_path / 'b', seq, distinct, False)
    _same(on, off)
    rewards = [x for x in on[:-1] if x.dtype.is_floating_point and x.dim() == 1]
    assert float(sum(r.double().abs().sum() for r in rewards)) > 0          # some reward was paid


@pytest.mark.parametrize('variant', ['conti', 'rllib_mask'])
def test_one_reward_step_of_the_other_step_forms(tmp_path, variant):
    """The continuous-action transition (rl4rs_env_step_conti) and the rllib-mask observation: up to and including the first
    reward step (SeqSlate: the 9th step)."""
    kw = dict(conti=True) if variant == 'conti' else dict(masked=True)
    on = _episode(tmp_path / 'a', True, False, True, steps=9, **kw)
    off = _episode(tmp_path / 'b', True, False, False, steps=9, **kw)
    _same(on, off)


def test_a_small_batch_keeps_the_two_forward_order(tmp_path):
    """B = 64 without the pin: the 9-row forward would run 32-row workgroups, so the stepper does not fold (asserted inside
    _episode through reward_rows) - and the results are those of the pinned, folded run."""
    plain = _episode(tmp_path / 'a', False, False, True, pin=False)
    folded = _episode(tmp_path / 'b', False, False, True)
    _same(plain, folded)
