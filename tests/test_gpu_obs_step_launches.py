"""Launches of an observation step: k_din_x / k_augru_x store a representative's scores and final states to its
duplicates (no k_row_expand launch), k_din_x picks 8 or 16 rows per workgroup on the device, the act kernel writes done, the
zero reward and the next step's logged action (no k_step_tail / k_offline_action launch).  Every part is pinned BIT FOR BIT
against its own switch ('dup_store' against the default 'no_dup_store' - the measurement kept the copy launch, DESIGN 20 -,
'din_rows16', config['no_act_tail']), and every case asserts that the situation it
is about really occurred (n_active, a duplicate stored across a row tile, the mapping the row count selects)."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CFG = {"maxlen": 64, "batch_size": 8, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
       "category_feature_num": 21, "category_hash_size": 3000, "seq_num": 2, "emb_size": 128,
       "page_items": 9, "hidden_units": 128, "max_steps": 9, "action_emb_size": 32, "scorer_precision": "fp16x2"}
CAP = 64            # ROW_DEDUP_CAP of rl4rs_amd/csrc/row_dedup.hpp
NEW, OLD = 'dup_store', 'no_dup_store,din_rows16'


@functools.lru_cache(maxsize=None)
def _weights(L):
    from rl4rs_amd.nets.dien import init_dien_weights
    return init_dien_weights(dict(CFG, maxlen=L), seed=9, emb_scale=0.5, bias_noise=0.2)


def _histories(n, L, rs):
    seq = rs.randint(1, 284, size=(n, 2, L)).astype(np.int32)
    seq[: n // 3, 0, : max(1, L // 2)] = 0          # leading padding on a third of input 0
    seq[::2, 1, :] = 0                              # input 1: every second history all padding
    return seq


def _template(group, rs):
    dense = np.abs(rs.randn(group, 432) * 3).astype(np.float32)
    cat = rs.randint(0, CFG['category_hash_size'], size=(group, 21)).astype(np.int32)
    cat[:, 10:] = rs.randint(0, 284, size=(group, 11))
    return dense, cat


def _groups(runs, group, rs):
    """runs = list of strings of template letters, one cache slot of input 0 per run ('ABA': three groups, the third equal to
    the first) -> slots [2, n], dense [n * group, 432], cat [n * group, 21]"""
    s0, s1, dn, ct = [], [], [], []
    for r, letters in enumerate(runs):
        tpl = {}
        for ch in letters:
            if ch not in tpl:
                tpl[ch] = _template(group, rs)
            s0.append(r)
            s1.append(r % 2)
            dn.append(tpl[ch][0])
            ct.append(tpl[ch][1])
    return np.array([s0, s1], dtype=np.int32), np.concatenate(dn), np.concatenate(ct)


def _expected(slots, cat, dense, group, order=None):
    """The duplicate rule of row_dedup.hpp in numpy, look-back window and chains included: position p takes the EARLIEST equal
    group among the positions of its run in the CAP - 1 in front of it; chains are then followed to their root.
    -> (n_active, rep[n_groups], active list in processing order)"""
    ng = slots.shape[1]
    order = np.arange(ng) if order is None else np.asarray(order)
    key = [(cat[g * group:(g + 1) * group].tobytes(), dense[g * group:(g + 1) * group].view(np.uint32).tobytes()) for g in range(ng)]
    rep = np.arange(ng)
    for p in range(ng):
        g = int(order[p])
        back = 0
        while back < CAP - 1 and p - 1 - back >= 0 and tuple(slots[:, order[p - 1 - back]]) == tuple(slots[:, g]):
            back += 1
        for k in range(back, 0, -1):
            g2 = int(order[p - k])
            if key[g2] == key[g]:
                rep[g] = g2
                break
    for g in range(ng):
        r = rep[g]
        while rep[r] != r:
            r = rep[r]
        rep[g] = r
    active = [int(order[p]) for p in range(ng) if rep[order[p]] == order[p]]
    return len(active), rep, active


def _crosses_tile(rep, active, group, tile=32):
    """Is some duplicate's row outside the row tile its representative is scored in (tile position = index in the active list)
    AND outside the representative's own block of `tile` batch rows?"""
    pos = {g: i for i, g in enumerate(active)}
    for g, r in enumerate(rep):
        if r != g and (g * group) // tile != (pos[int(r)] * group) // tile and (g * group) // tile != (int(r) * group) // tile:
            return True
    return False


class _Pair(object):
    """Two handles over the same weights and encoded histories: every new part on (`NEW` + the defaults) and `OLD` (+ `extra` on both)."""

    def __init__(self, L, seq, R, extra=''):
        import torch
        from rl4rs_amd.device import DeviceDien
        self.nets = []
        for kernels in (','.join(x for x in (NEW, extra) if x), ','.join(x for x in (OLD, extra) if x)):
            net = DeviceDien(dict(CFG, maxlen=L, scorer_kernels=kernels), _weights(L), max_rows=R, max_slots=seq.shape[0])
            for s in range(2):
                net.encode(s, torch.from_numpy(np.ascontiguousarray(seq[:, s])).cuda(), 0)
            self.nets.append(net)

    def forward(self, R, group, dense, cat, slots, order=None, rows=0):
        """-> [new, old], each (obs, prob, all_feature, scores, n_active, rep)"""
        import torch
        from rl4rs_amd.device import DIEN_ALL_FEATURE, DIEN_SCORES, DIEN_N_ACTIVE, DIEN_ROW_REP
        sl = torch.from_numpy(np.ascontiguousarray(slots)).cuda()
        d, c = torch.from_numpy(dense).cuda(), torch.from_numpy(cat).cuda()
        outs = []
        for net in self.nets:
            net.set_row_order(None if order is None else torch.from_numpy(np.asarray(order, dtype=np.int32)).cuda())
            net.set_augru_rows(rows)
            obs, p = net.forward(R, group, d, c, sl, True, True)
            outs.append((obs.clone(), p.clone(), net.snapshot(DIEN_ALL_FEATURE, R)[:R].clone(), net.snapshot(DIEN_SCORES, R)[:, :R].clone(),
                         int(net.snapshot(DIEN_N_ACTIVE, 0)[0].item()), net.snapshot(DIEN_ROW_REP, R)[:R // group].cpu().numpy()))
            net.check_status()
        return outs

    def close(self):
        for net in self.nets:
            net.close()


def _same(new, old, expected, what):
    import torch
    for name, a, b in zip(('obs', 'prob', 'all_feature', 'scores'), new, old):
        assert torch.isfinite(a).all(), (what, name)
        assert torch.equal(a, b), (what, name)
    n_exp, rep_exp, _ = expected
    print(what, 'n_active', new[4], old[4], 'expected', n_exp, 'of', len(rep_exp))
    assert new[4] == n_exp and old[4] == n_exp, what
    assert np.array_equal(new[5], rep_exp) and np.array_equal(old[5], rep_exp), what


def _cases(group):
    """name -> (runs, expected n_active or None, must a duplicate be stored across a row tile?)"""
    if group == 1:          # 96 groups of one row: three 32-row tiles
        long_run = 'A' * 40 + 'B' + 'A' * 30        # 71 positions > CAP with A B A inside: the tail's first choice is a duplicate itself
        return {'distinct': (['ABC'] * 32, 96, False),
                'equal': (['A' * 96], 1, True),                                  # one run longer than the cap; a one-row last tile
                'mixed': (['ABA', 'ABAAB', long_run, 'AA', 'A', 'ABAB', 'AAAAAAAAAA'], None, True)}
    return {'distinct': (['ABCD'] * 6, 24, False),      # 24 groups of 8 rows = 192 rows: six 32-row / three 64-row tiles
            'equal': (['A' * 24], 1, True),
            'mixed': (['AAAA', 'ABAB', 'AAAAAAAA', 'ABBA', 'AAAA'], None, True)}


@pytest.mark.parametrize('L', [16, 33])
@pytest.mark.parametrize('group,R', [(1, 96), (8, 192)])
def test_forward_is_bit_identical_to_the_old_launches(group, R, L):
    """group 1 at R = 96 and group 8 at R = 192 (both row-tile forms of k_augru_x), maxlen 16 and 33: all groups distinct, all
    equal (group 1: a run longer than ROW_DEDUP_CAP), A B A inside a run, duplicates whose representative is scored in another
    row tile, a partial last tile - each in natural order and scattered over the batch with the row order that undoes it."""
    rs = np.random.RandomState(100 * group + L)
    seq = _histories(40, L, rs)
    pair = _Pair(L, seq, R)
    try:
        for name, (runs, n_exp, cross) in sorted(_cases(group).items()):
            slots, dense, cat = _groups(runs, group, rs)
            ng = slots.shape[1]
            assert ng * group == R and int(slots[0].max()) < 40
            perm = np.random.RandomState(5).permutation(ng)           # physical group i holds group perm[i] of the layout above
            rows8 = (perm[:, None] * group + np.arange(group)[None, :]).reshape(-1)
            scattered = (np.ascontiguousarray(slots[:, perm]), dense[rows8], cat[rows8], np.argsort(perm).astype(np.int32))
            for order_name, (sl, dn, ct, order) in (('natural', (slots, dense, cat, None)), ('ordered', scattered)):
                exp = _expected(sl, ct, dn, group, order)
                if n_exp is not None:
                    assert exp[0] == n_exp, (name, order_name, exp[0])
                else:
                    assert 1 < exp[0] < ng and (exp[0] * group) % 32 != 0, (name, exp[0])        # duplicates, and a partial last tile
                if cross:
                    assert _crosses_tile(exp[1], exp[2], group), (name, order_name)
                if name == 'equal' and group == 1:
                    # the run is longer than the cap: positions >= CAP first chose a group that is a duplicate itself
                    assert ng > CAP and (exp[1] == exp[2][0]).all()
                for rows in ((0,) if group == 1 else (32, 64)):
                    new, old = pair.forward(R, group, dn, ct, sl, order, rows)
                    _same(new, old, exp, (name, order_name, rows))
    finally:
        pair.close()


def test_din_mapping_8_16_and_threshold():
    """k_din_x, group 1, all rows distinct, against the device's CU count: R at exactly the threshold ceil(R / 8) * S = 2 * n_cu
    (one row per wave), 8 rows above it (two rows per wave, as before) and far below it.  The scores of the rows the three forwards
    share are bit-identical across them, and each forward is bit-identical to the 'din_rows16' handle."""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    S, L = 2, 16
    r_thr = (2 * n_cu // S) * 8
    r_max = r_thr + 8
    assert ((r_thr + 7) // 8) * S <= 2 * n_cu < ((r_max + 7) // 8) * S and ((96 + 7) // 8) * S <= 2 * n_cu
    rs = np.random.RandomState(7)
    seq = _histories(64, L, rs)
    dense = np.abs(rs.randn(r_max, 432) * 3).astype(np.float32)
    cat = rs.randint(0, 284, size=(r_max, 21)).astype(np.int32)
    slots = np.stack([rs.randint(0, 64, size=r_max), rs.randint(0, 2, size=r_max)]).astype(np.int32)
    pair = _Pair(L, seq, r_max)
    try:
        got = {}
        for R in (r_thr, r_max, 96):
            new, old = pair.forward(R, 1, dense[:R], cat[:R], np.ascontiguousarray(slots[:, :R]))
            assert new[4] == R and old[4] == R                        # nothing deduplicated: the active row count IS R
            for name, a, b in zip(('obs', 'prob', 'all_feature', 'scores'), new, old):
                assert torch.isfinite(a).all() and torch.equal(a, b), (R, name)
            got[R] = new[3]
        assert float(got[96].abs().sum()) > 0
        assert torch.equal(got[r_thr][:, :96], got[96]) and torch.equal(got[r_max][:, :r_thr], got[r_thr])
    finally:
        pair.close()


def _episodes(tmp_path, seq, no_tail, scorer_kernels=''):
    """Two episodes back to back, B = 64 envs over a 24-line log -> (list of everything a step returned, the scorer's profile
    of the second episode).  Every third log line is shorter than the horizon; one env is handed an illegal action id at step 3."""
    import torch
    import rl4rs_amd
    from rl4rs_amd import synth
    from rl4rs_amd.env.slate import SlateRecEnv, SlateState
    from rl4rs_amd.env.seqslate import SeqSlateRecEnv, SeqSlateState
    d = str(tmp_path)
    B, T = 64, 18 if seq else 9
    text = synth.make_catalog_text(seed=4)
    synth.write_text(os.path.join(d, 'c.csv'), text)
    recs = synth.make_records(24, pages=2 if seq else 1, seed=3, hash_size=2000, special_ids=synth.special_ids_from_text(text))
    for i in range(2, 24, 3):                           # every third line: the logged slate ends two items before the horizon
        f = recs[i].split('@')
        f[3] = ','.join(f[3].split(',')[:T - 2])
        f[4] = ','.join(f[4].split(',')[:T - 2])
        recs[i] = '@'.join(f)
    synth.write_records(os.path.join(d, 'log.csv'), recs)
    cfg = {"maxlen": 64, "batch_size": B, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
           "category_feature_num": 21, "category_hash_size": 2000, "seq_num": 2, "emb_size": 128, "page_items": 9,
           "hidden_units": 128, "max_steps": T, "action_emb_size": 32, "sample_file": os.path.join(d, 'log.csv'),
           "iteminfo_file": os.path.join(d, 'c.csv'), "cache_size": 24, "model_seed": 3,
           "return_tensors": True, "scorer_kernels": scorer_kernels, "no_act_tail": no_tail}
    if seq:
        cfg['support_rllib_mask'] = True
        env = rl4rs_amd.make('SeqSlateRecEnv-v0', recsim=SeqSlateRecEnv(cfg, state_cls=SeqSlateState))
    else:
        env = rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))
    env.seed(11)
    out, raised, from_tail = [], 0, 0
    prof = None
    for ep in range(2):
        obs = env.reset()
        out.append((obs['obs'] if isinstance(obs, dict) else obs).clone())
        net = env.sim.model.device_net
        if ep == 1:
            net.set_profiling(1)
            net.profile_reset()
        for t in range(T):
            live = env.samples._live()
            logged = live.offline_action()              # k_offline_action itself: what the rule gives at this step
            try:
                a = env.offline_action
            except IndexError:                          # the short line: the logged slate has no item for this step
                raised += 1
                a = logged
            stepper = getattr(env.sim, '_stepper', None)
            nxt = stepper.next_offline_action() if (stepper is not None and t > 0) else None
            if nxt is not None:                         # the act kernel's copy of the same ids, for exactly this step
                assert nxt[0] == t and torch.equal(nxt[1], logged), t
                from_tail += 1
            assert a.dtype == torch.int32 and torch.equal(a, logged), t
            out.append(a.clone())
            if t == 3:
                a = a.clone()
                a[7] = 284 + 5                          # an illegal id: the env flags it and plays item 0
            obs, reward, done, info = env.step(a)
            out.append((obs['obs'] if isinstance(obs, dict) else obs).clone())
            out.append(reward.clone())
            out.append(torch.as_tensor(np.asarray(done, dtype=np.int64)))
        # the logged action past the horizon (0 for every env)
        out.append(env.samples._live().offline_action().clone())
        if ep == 1:
            torch.cuda.synchronize()
            prof = net.profile()
            net.set_profiling(0)
    flag = int(env.samples._live().snapshot(rl4rs_amd.device.BUF_ERROR_FLAG).item())
    return out, prof, dict(raised=raised, from_tail=from_tail, flag=flag)


@pytest.mark.parametrize('kind', ['slate', 'seq'])
def test_transition_is_bit_identical_without_the_tail_launches(tmp_path, kind):
    """SlateRecEnv (T = 9) and SeqSlateRecEnv (T = 18), 64 envs over 24 lines, two episodes: observation, reward, done and the
    action every offline_action returned, with config['no_act_tail'] off and on - ints exact, floats bit for bit."""
    import torch
    seq = kind == 'seq'
    os.makedirs(str(tmp_path / 'a'))
    os.makedirs(str(tmp_path / 'b'))
    on, _, info_on = _episodes(tmp_path / 'a', seq, False)
    off, _, info_off = _episodes(tmp_path / 'b', seq, True)
    print(kind, info_on, info_off)
    T = 18 if seq else 9
    assert info_on['from_tail'] == 2 * (T - 1) and info_off['from_tail'] == 0     # every action but an episode's first came from the act kernel
    assert info_on['raised'] == info_off['raised'] == 2 * 2                        # the short lines: the last two steps of both episodes
    assert info_on['flag'] == info_off['flag'] == 1                                # the illegal id was seen
    assert len(on) == len(off)
    assert float(sum(x.double().abs().sum() for x in on)) > 0
    for i, (x, y) in enumerate(zip(on, off)):
        assert x.dtype == y.dtype and torch.equal(x, y), i


def test_dedup_class_launch_counts(tmp_path):
    """net.profile() of one Slate episode at B = 64: the 'k_row_dedup + k_row_expand' class counts one launch per forward with the
    duplicates stored by the producers ('dup_store'), two with 'no_dup_store' and by default."""
    os.makedirs(str(tmp_path / 'a'))
    os.makedirs(str(tmp_path / 'b'))
    counts = {}
    os.makedirs(str(tmp_path / 'c'))
    for name, kernels in (('a', 'dup_store'), ('b', 'no_dup_store'), ('c', '')):
        _, prof, _ = _episodes(tmp_path / name, False, False, kernels)
        dd = [v for k, v in prof.items() if 'k_row_expand' in k]
        din = [v for k, v in prof.items() if k.startswith('k_din_x')]
        assert len(dd) == 1 and len(din) == 1, sorted(prof)
        counts[name] = (dd[0][1], din[0][1])
    print(counts)
    assert counts['a'][1] == counts['b'][1] >= 10          # forwards of the episode: nine observations and the reward forward at least
    assert counts['a'][0] == counts['a'][1]
    assert counts['b'][0] == 2 * counts['b'][1]
    assert counts['c'] == counts['b']
