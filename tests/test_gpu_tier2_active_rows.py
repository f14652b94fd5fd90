"""Second tier of the fp16x2 DIEN scorer on the active rows only: with the row dedup on, the category kernels, the
dense tower / q-side GEMMs and the head GEMM take the active list as k_din_x and k_augru_x do, and k_row_expand - behind the
head GEMM - copies a duplicate's whole all-feature row, its scores, its query row and its head output.  Everything is pinned
BIT FOR BIT against the same handle with scorer_kernels='no_tier2_rows' (the launches of before) and against 'no_row_dedup':
obs, prob, ALL_FEATURE, SCORES, QUERY, N_ACTIVE, ROW_REP and obs_last; N_ACTIVE also against the duplicate rule in numpy, so
that every case is known to have had the duplicates (or their absence) it is about."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CFG = {"maxlen": 64, "batch_size": 8, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
       "category_feature_num": 21, "category_hash_size": 3000, "seq_num": 2, "emb_size": 128,
       "page_items": 9, "hidden_units": 128, "max_steps": 9, "action_emb_size": 32, "scorer_precision": "fp16x2"}
CAP = 64            # ROW_DEDUP_CAP of rl4rs_amd/csrc/row_dedup.hpp
NSLOTS = 16
ARMS = ('', 'no_tier2_rows', 'no_row_dedup')


@functools.lru_cache(maxsize=None)
def _weights():
    from rl4rs_amd.nets.dien import init_dien_weights
    return init_dien_weights(dict(CFG), seed=9, emb_scale=0.5, bias_noise=0.2)


@functools.lru_cache(maxsize=None)
def _histories():
    rs = np.random.RandomState(77)
    seq = rs.randint(1, 284, size=(NSLOTS, 2, 64)).astype(np.int32)
    seq[: NSLOTS // 3, 0, :32] = 0                  # leading padding on a third of input 0
    seq[::2, 1, :] = 0                              # input 1: every second history all padding
    return seq


def _template(group, rs):
    dense = np.abs(rs.randn(group, 432) * 3).astype(np.float32)
    cat = rs.randint(0, CFG['category_hash_size'], size=(group, 21)).astype(np.int32)
    cat[:, 10:] = rs.randint(0, 284, size=(group, 11))
    if group > 1:                                   # complete states of one env: all ids but the last are the env's
        cat[:, :20] = cat[0, :20]
    return dense, cat


def _groups(runs, group, rs, pool=None):
    """runs = list of strings of template letters ('ABA': three groups, the third equal to the first); run r reads slot r % NSLOTS
    of input 0 and slot r % 2 of input 1, so neighbouring runs never share their slots.  `pool`: templates to draw from in turn
    (large cases) instead of fresh ones per run -> slots [2, n], dense [n * group, 432], cat [n * group, 21]"""
    s0, s1, dn, ct = [], [], [], []
    k = 0
    for r, letters in enumerate(runs):
        tpl = {}
        for ch in letters:
            if ch not in tpl:
                if pool is None:
                    tpl[ch] = _template(group, rs)
                else:
                    tpl[ch] = pool[k % len(pool)]
                    k += 1
            s0.append(r % NSLOTS)
            s1.append(r % 2)
            dn.append(tpl[ch][0])
            ct.append(tpl[ch][1])
    return np.array([s0, s1], dtype=np.int32), np.concatenate(dn), np.concatenate(ct)


def _expected(slots, cat, dense, group, order=None):
    """The duplicate rule of row_dedup.hpp in numpy (look-back window and chains included) -> (n_active, rep[n_groups])"""
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
    return int((rep == np.arange(ng)).sum()), rep


@functools.lru_cache(maxsize=None)
def _nets(R, arms=ARMS):
    """One handle per arm over the same weights and encoded histories, kept for every case of that row count."""
    import torch
    from rl4rs_amd.device import DeviceDien
    nets = []
    for kernels in arms:
        net = DeviceDien(dict(CFG, scorer_kernels=kernels), _weights(), max_rows=R, max_slots=NSLOTS)
        for s in range(2):
            net.encode(s, torch.from_numpy(np.ascontiguousarray(_histories()[:, s])).cuda(), 0)
        nets.append(net)
    return nets


NAMES = ('obs', 'prob', 'all_feature', 'scores', 'query', 'obs_last')


def _forward(net, kernels, R, group, dense, cat, slots, order=None, rows=0, obs_last=False, count=False):
    """-> ([obs, prob, all_feature, scores, query, obs_last or None], n_active, rep, launch counts per profile class)"""
    import torch
    from rl4rs_amd.device import DIEN_ALL_FEATURE, DIEN_SCORES, DIEN_QUERY, DIEN_N_ACTIVE, DIEN_ROW_REP
    sl = torch.from_numpy(np.ascontiguousarray(slots)).cuda()
    d, c = torch.from_numpy(dense).cuda(), torch.from_numpy(cat).cuda()
    net.set_row_order(None if order is None else torch.from_numpy(np.asarray(order, dtype=np.int32)).cuda())
    net.set_augru_rows(rows)
    net.set_profiling(1 if count else 0)
    net.profile_reset()
    res = net.forward(R, group, d, c, sl, True, True, want_obs_last=obs_last)
    out = [res[0].clone(), res[1].clone(), net.snapshot(DIEN_ALL_FEATURE, R)[:R].clone(), net.snapshot(DIEN_SCORES, R)[:, :R].clone(),
           net.snapshot(DIEN_QUERY, R)[:R].clone(), res[2].clone() if obs_last else None]
    n_active = rep = None
    if 'no_row_dedup' not in kernels:
        n_active = int(net.snapshot(DIEN_N_ACTIVE, 0)[0].item())
        rep = net.snapshot(DIEN_ROW_REP, R)[:R // group].cpu().numpy()
    counts = dict((k, v[1]) for k, v in net.profile().items()) if count else None
    net.set_profiling(0)
    net.check_status()
    return out, n_active, rep, counts


def _same(a, b, what):
    import torch
    for name, x, y in zip(NAMES, a, b):
        if x is None:
            assert y is None
            continue
        assert torch.isfinite(x).all(), (what, name)
        assert torch.equal(x, y), (what, name)


def _compare(R, group, dense, cat, slots, order=None, rows=0, obs_last=False, arms=ARMS, nets=None):
    exp_n, exp_rep = _expected(slots, cat, dense, group, order)
    res = [_forward(net, k, R, group, dense, cat, slots, order, rows, obs_last) for net, k in zip(nets or _nets(R, arms), arms)]
    on = res[0]
    print('R', R, 'group', group, 'rows', rows, 'n_active', on[1], 'expected', exp_n, 'of', R // group)
    assert on[1] == exp_n and np.array_equal(on[2], exp_rep)
    for other, k in zip(res[1:], arms[1:]):
        _same(on[0], other[0], k)
        if other[1] is not None:
            assert other[1] == on[1] and np.array_equal(other[2], on[2])
    return exp_n


def _scatter(slots, dense, cat, group, seed):
    """The groups scattered over the batch, and the processing order that puts the runs back together."""
    ng = slots.shape[1]
    perm = np.random.RandomState(seed).permutation(ng)            # physical group i holds group perm[i] of the run layout
    rows = (perm[:, None] * group + np.arange(group)[None, :]).reshape(-1)
    return np.ascontiguousarray(slots[:, perm]), dense[rows], cat[rows], np.argsort(perm).astype(np.int32)


OBS_PATTERNS = {'aba_cc': (['ABACC'] * 10 + ['AAAAAA'] * 5, 35),       # n_active ends inside the second 32-row tile
                'identical': (['A' * 80], 1),
                'distinct': (['ABCDE'] * 16, 80)}


@pytest.mark.parametrize('ordered', [False, True])
@pytest.mark.parametrize('pattern', sorted(OBS_PATTERNS))
def test_observation_shaped(pattern, ordered):
    """group = 1, R = 80: three 32-row GEMM tiles with the last one partial, 20 category workgroups.  With 35 active rows one tile
    is full, one partial, one leaves; with one active row two leave; with 80 nothing is copied."""
    runs, n_want = OBS_PATTERNS[pattern]
    rs = np.random.RandomState(len(pattern))
    slots, dense, cat = _groups(runs, 1, rs)
    assert slots.shape[1] == 80
    order = None
    if ordered:
        slots, dense, cat, order = _scatter(slots, dense, cat, 1, 5)
    assert _compare(80, 1, dense, cat, slots, order) == n_want


@pytest.mark.parametrize('group,R,runs,n_want', [(8, 192, ['ABAAB', 'AAB', 'ABBA', 'AAAA', 'ABAAB', 'AAA'], 10),
                                                 (9, 135, ['ABAAB', 'AAB', 'AAAA', 'ABA'], 7)])
def test_reward_shaped(group, R, runs, n_want):
    """Groups of 8 (R = 192) and of 9 (R = 135), about 40 % of them distinct, both AUGRU row-tile forms pinned, with obs_last:
    k_cat_attn2g takes group active[p], the 32-row GEMM tiles end inside a group's rows (80 / 63 active rows)."""
    rs = np.random.RandomState(group)
    slots, dense, cat = _groups(runs, group, rs)
    assert slots.shape[1] * group == R
    slots, dense, cat, order = _scatter(slots, dense, cat, group, 3)
    for rows in (32, 64):
        assert _compare(R, group, dense, cat, slots, order, rows=rows, obs_last=True) == n_want
    _compare(R, group, dense, cat, slots, None, rows=0, obs_last=True)       # the natural order: fewer hits, the same bits


def test_reward_sized_launch_takes_the_64_row_gemm_tiles():
    """The 64-row tile form of the mapped GEMMs is chosen from 512 row tiles on (gemm.hip: gemm_h16_route), which only a
    reward-sized launch reaches: R = 32 760 in groups of 9, 40 % of the groups distinct - 13 104 active rows, the last of 205
    tiles partial, 307 workgroups leave."""
    group, ng = 9, 3640
    rs = np.random.RandomState(11)
    pool = [_template(group, rs) for _ in range(24)]
    slots, dense, cat = _groups(['ABAAB'] * (ng // 5), group, rs, pool=pool)
    R = ng * group
    assert (R + 63) // 64 >= 512
    arms = ('', 'no_tier2_rows')
    nets = _nets.__wrapped__(R, arms)                            # not kept: two handles of 32 760 rows
    try:
        n = _compare(R, group, dense, cat, slots, arms=arms, obs_last=True, nets=nets)
    finally:
        for net in nets:
            net.close()
    assert n == 2 * (ng // 5) and (n * group) % 64 != 0


def test_dup_store_keeps_its_launches():
    """'dup_store': the forward issues exactly the launches it issued before - equal results and equal launch counts per profile
    class with and without 'no_tier2_rows'."""
    runs, _ = OBS_PATTERNS['aba_cc']
    rs = np.random.RandomState(2)
    slots, dense, cat = _groups(runs, 1, rs)
    arms = ('dup_store', 'dup_store,no_tier2_rows')
    a, b = [_forward(net, k, 80, 1, dense, cat, slots, count=True) for net, k in zip(_nets(80, arms), arms)]
    _same(a[0], b[0], 'dup_store')
    assert a[1] == b[1] == 35
    assert a[3] == b[3] and sum(a[3].values()) > 0, (a[3], b[3])
    # ... while the default handle does move the expansion: same classes, same counts, bit-identical as well
    c = _forward(_nets(80, ARMS)[0], '', 80, 1, dense, cat, slots, count=True)
    _same(a[0], c[0], 'default')


def _episode(tmp_path, kernels, tensors, host_mirror=False):
    """One SlateRecEnv episode of offline_action replay, B = 64, T = 9, 20 log lines and cache_size = 16 (most envs share a line)
    -> (observations of every step and rewards as float32 arrays, n_active of the last forward, launch counts per class)"""
    import torch
    import rl4rs_amd
    from rl4rs_amd import synth, _lib
    from rl4rs_amd.device import DIEN_N_ACTIVE
    from rl4rs_amd.env.slate import SlateRecEnv, SlateState
    d = str(tmp_path)
    os.makedirs(d, exist_ok=True)
    B, T = 64, 9
    text = synth.make_catalog_text(seed=4)
    synth.write_text(os.path.join(d, 'c.csv'), text)
    recs = synth.make_records(20, pages=1, seed=3, hash_size=2000, special_ids=synth.special_ids_from_text(text))
    synth.write_records(os.path.join(d, 'log.csv'), recs)
    cfg = {"maxlen": 64, "batch_size": B, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
           "category_feature_num": 21, "category_hash_size": 2000, "seq_num": 2, "emb_size": 128, "page_items": 9,
           "hidden_units": 128, "max_steps": T, "action_emb_size": 32, "sample_file": os.path.join(d, 'log.csv'),
           "iteminfo_file": os.path.join(d, 'c.csv'), "cache_size": 16, "model_seed": 3, "scorer_kernels": kernels}
    if tensors:
        cfg['return_tensors'] = True
    lib = _lib.load()
    lib.rl4rs_set_host_mirror(1 if host_mirror else 0)
    try:
        env = rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))
        env.seed(11)
        net = env.sim.model.device_net
        net.set_profiling(1)
        net.profile_reset()

        def arr(x):
            x = x['obs'] if isinstance(x, dict) else x
            return (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).astype(np.float32)
        out = [arr(env.reset())]
        for t in range(T):
            obs, reward, done, info = env.step(env.offline_action)
            out.append(arr(obs))
            out.append(arr(reward))
        torch.cuda.synchronize()
        counts = dict((k, v[1]) for k, v in net.profile().items())
        net.set_profiling(0)
        n_active = int(net.snapshot(DIEN_N_ACTIVE, 0)[0].item())
    finally:
        lib.rl4rs_set_host_mirror(0)
    return out, n_active, counts


def _equal_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_episode_replay_is_bit_identical(tmp_path):
    """One episode on device tensors: the observation of every step and the rewards equal those of the 'no_tier2_rows' run, and
    the last forward (the reward forward over the complete states) really had duplicates."""
    on, n_active, c_on = _episode(tmp_path / 'a', '', True)
    off, n_off, c_off = _episode(tmp_path / 'b', 'no_tier2_rows', True)
    assert len(on) == len(off) == 19
    assert float(sum(np.abs(x).sum() for x in on[2::2])) > 0          # some reward was paid
    for t, (x, y) in enumerate(zip(on, off)):
        assert _equal_bits(x, y), t
    print('n_active of the last forward', n_active, 'of 64')
    assert n_active == n_off and 1 <= n_active < 64
    assert c_on == c_off                                               # the expansion moved, no launch was added


def test_host_mirror_keeps_its_launches(tmp_path):
    """The record form with the head GEMM's host mirror armed (rl4rs_set_host_mirror): such a forward issues exactly the launches
    it issued before - identical observations and rewards, equal launch counts per profile class."""
    on, n_active, c_on = _episode(tmp_path / 'a', '', False, host_mirror=True)
    off, n_off, c_off = _episode(tmp_path / 'b', 'no_tier2_rows', False, host_mirror=True)
    ref, _, _ = _episode(tmp_path / 'c', 'no_tier2_rows', False, host_mirror=False)
    assert len(on) == len(off) == len(ref) == 19
    for t, (x, y, z) in enumerate(zip(on, off, ref)):
        assert _equal_bits(x, y) and _equal_bits(x, z), t
    assert n_active == n_off and 1 <= n_active < 64
    assert c_on == c_off and sum(c_on.values()) > 0, (c_on, c_off)
