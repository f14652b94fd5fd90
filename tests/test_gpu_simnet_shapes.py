"""The dnn / widedeep / lstm scorer forward (rl4rs_simnet_*) away from the one shape tests/test_gpu_simnet.py runs, against the
float64 restatement (oracle/simnets.py) of seeded weights (init_simnet_weights(emb_scale=0.5, bias_noise=0.2)); every case's
category and sequence ids hold id 0 and id H - 1 (tests/simnet_cases.py generates the cases, tests/test_simnet_shapes_host.py checks
on the CPU that they are what this file says they are).

* the shape table L1..W2 of simnet_cases.SHAPES at R = 65: GRUs of length 1 (no next-step prefetch), 13, 16, 33 and 64; 1, 3 and 4
  sequence inputs; 2, 3 and 8 classes; a 7-row embedding table; dnn / widedeep at E 8 / U 32 and E 200 / U 160
* each family at R in {1, 31, 32, 33, 65} with max_rows = R: the 4-row (gathers, head) and 32-row (k_recur) block edges, the handle
  exactly full
* keras hard_sigmoid gates on both clamps (no input of tests/test_gpu_simnet.py reaches +-2.5): the GRU matrices scaled up
* one handle over several encodes, permuted and shared slots, groups of 1 / 4 / 9 rows, a smaller R in between, prob-only calls
* ids outside the embedding table: every gather clamps them to [0, H - 1]
* one episode at maxlen 16 with histories on both sides of it

Bars: those of tests/test_gpu_simnet.py - obs 5e-5, probabilities 5e-6 absolute, rewards rtol / atol 1e-5.  A case whose float32
restatement misses the float64 one by more than a quarter of a bar on its own inputs takes 4 x that miss instead
(simnet_cases.bar); measured on the CPU: table and row sweep at most 4.4e-6 (obs, W2) and 5.4e-7 (probabilities, D2), 'kernel16' at
most 1.6e-6 / 4.9e-7 - the fixed bars hold.  'x8' (kernel and recurrent matrices times 8) is the one exception: that recurrence
amplifies rounding, L3 (16 steps) float32 misses by 4.9e-4 (obs) / 9.4e-5 (probabilities), the default configuration (64 steps) by
1.3 / 0.30 - its float32 and float64 trajectories part ways, so at 'x8' only L3 is a sharp check, and 'kernel16' is what pins the
clamps at the default configuration."""
import os

import numpy as np
import pytest

import simnet_cases as sc

pytestmark = pytest.mark.gpu

_REFS = {}


def _case(name, R, saturated=None):
    """-> algo, cfg, w, (seq, dense, cat), obs_ref, prob_ref, obs_bar, prob_bar; computed once per case"""
    key = (name, R, saturated)
    if key not in _REFS:
        algo, cfg = sc.SHAPES[name]
        w = sc.weights(name, saturated=saturated)
        x = sc.case_inputs(name, R)
        obs_ref, prob_ref, e_obs, e_prob = sc.yardstick(algo, w, cfg, *x)
        for a in x + (obs_ref, prob_ref):
            a.setflags(write=False)
        _REFS[key] = (algo, cfg, w, x, obs_ref, prob_ref, sc.bar(sc.OBS_BAR, e_obs), sc.bar(sc.PROB_BAR, e_prob))
        print('%s R=%d %s: float32 restatement off by %.3g (obs) %.3g (prob)' % (name, R, saturated, e_obs, e_prob))
    return _REFS[key]


def _t(a):
    import torch
    return torch.from_numpy(np.array(a, order='C')).cuda()          # a copy: the shared references are read-only


def _encode_rows(net, seq, slot_base=0):
    for s in range(seq.shape[1]):
        net.encode(s, _t(seq[:, s]), slot_base)


def _iota_slots(S, R):
    import torch
    return torch.arange(R, dtype=torch.int32).repeat(S, 1).contiguous().cuda()


def _check(net, R, group, dense, cat, slots, obs_ref, prob_ref, obs_bar=sc.OBS_BAR, prob_bar=sc.PROB_BAR, what=''):
    """one obs + prob forward and the head on its obs against the reference; -> obs, prob (device tensors)"""
    obs, prob = net.forward(R, group, _t(dense), _t(cat), slots, want_obs=True, want_prob=True)
    assert tuple(obs.shape) == obs_ref.shape and tuple(prob.shape) == prob_ref.shape
    e_obs = np.abs(obs.cpu().numpy() - obs_ref).max()
    e_prob = np.abs(prob.cpu().numpy() - prob_ref).max()
    e_head = np.abs(net.head_prob(obs).cpu().numpy() - prob_ref).max()
    print('%s: obs off by %.3g (bar %.3g), prob %.3g, head_prob %.3g (bar %.3g)' % (what, e_obs, obs_bar, e_prob, e_head, prob_bar))
    assert e_obs < obs_bar and e_prob < prob_bar and e_head < prob_bar, what
    return obs, prob


def _run_case(name, R, saturated=None):
    from rl4rs_amd.nets.simnets import obs_dim
    from rl4rs_amd.device import DeviceSimnet
    algo, cfg, w, (seq, dense, cat), obs_ref, prob_ref, obs_bar, prob_bar = _case(name, R, saturated)
    net = DeviceSimnet(cfg, w, max_rows=R, max_slots=R, algo=algo)
    try:
        assert net.obs_dim == obs_dim(cfg, algo)
        _encode_rows(net, seq)
        _check(net, R, 1, dense, cat, _iota_slots(cfg['seq_num'], R), obs_ref, prob_ref, obs_bar, prob_bar, '%s R=%d' % (name, R))
    finally:
        net.close()


@pytest.mark.parametrize('name', sc.TABLE)
def test_shape_table(name):
    _run_case(name, sc.TABLE_R)


@pytest.mark.parametrize('R', sc.ROW_COUNTS)
@pytest.mark.parametrize('algo', sorted(sc.ROW_SWEEP))
def test_row_counts_at_the_block_edges(algo, R):
    _run_case(sc.ROW_SWEEP[algo], R)


@pytest.mark.parametrize('variant', sorted(sc.SAT_VARIANTS))
@pytest.mark.parametrize('name', sc.SATURATED)
def test_saturated_hard_sigmoid_gates(name, variant):
    """a quarter and more of the gate pre-activations at or beyond each clamp (the forward is continuous at the kinks: no margin
    needed).  Without the clip a gate leaves [0, 1] and the state leaves (-1, 1)."""
    _run_case(name, sc.TABLE_R, saturated=variant)


def _slot_case(name):
    """39 histories in slots 0, 1, 3 .. 39 of a 40-slot handle (slot 2 is never encoded and never read)"""
    algo, cfg = sc.SHAPES[name]
    S, L, H = cfg['seq_num'], cfg['maxlen'], cfg['category_hash_size']
    hist = np.zeros((40, S, L), dtype=np.int32)
    parts = {}
    for base, cnt in ((36, 4), (3, 33), (0, 2)):
        parts[base] = sc.inputs(cfg, cnt, seed=500 + base)[0]
        hist[base:base + cnt] = parts[base]
    return algo, cfg, hist, parts


@pytest.mark.parametrize('name', ['L3', 'W2'])
def test_slots_groups_and_handle_reuse(name):
    """One handle (max_rows 70, max_slots 40).  Encodes of 4 histories at slot 36, then 33 at slot 3, then 2 at slot 0 - in this
    order a write past the last row of the ragged 33- or 2-row encode lands in a slot encoded before it and shows below.  Forwards
    with groups of 1, 4 and 9 rows over permuted slot tables (one per sequence input) in which the first two groups share a slot
    equal the restatement on the expanded rows; then R = 65, R = 5 on other inputs and R = 65 again: each within the bars, the third
    bit-identical to the first; a prob-only call equals the obs + prob call bit for bit."""
    import torch
    from rl4rs_amd.device import DeviceSimnet
    from oracle.simnets import OracleSimnet
    algo, cfg, hist, parts = _slot_case(name)
    S = cfg['seq_num']
    w = sc.weights(name, seed=4)
    orc = OracleSimnet(algo, w, cfg, np.float64)
    net = DeviceSimnet(cfg, w, max_rows=70, max_slots=40, algo=algo)
    try:
        for base in (36, 3, 0):
            _encode_rows(net, parts[base], base)
        used = np.array([0, 1] + list(range(3, 40)))

        def forward(n_groups, group, seed, tag):
            r2 = np.random.RandomState(seed)
            draw = lambda: r2.permutation(used)[:n_groups] if n_groups <= len(used) else r2.choice(used, n_groups)
            slots = np.stack([draw() for _ in range(S)]).astype(np.int32)
            if n_groups > 1:
                slots[:, 1] = slots[:, 0]
            R = n_groups * group
            _, dense, cat = sc.inputs(cfg, R, seed=seed + 1)
            seq_rows = np.stack([hist[np.repeat(slots[s], group), s] for s in range(S)], axis=1)
            obs_ref = orc.obs(seq_rows, dense, cat)
            prob_ref = orc.reward_probs(seq_rows, dense, cat)[:, 1]
            ds = _t(slots)
            obs, prob = _check(net, R, group, dense, cat, ds, obs_ref, prob_ref, what='%s %s' % (name, tag))
            none, prob_only = net.forward(R, group, _t(dense), _t(cat), ds, want_obs=False, want_prob=True)
            assert none is None and torch.equal(prob_only, prob), tag
            return obs.clone(), prob.clone()

        forward(39, 1, 10, 'group 1')
        forward(17, 4, 20, 'group 4')
        forward(7, 9, 30, 'group 9')
        first = forward(65, 1, 40, 'R 65')
        forward(5, 1, 50, 'R 5')
        again = forward(65, 1, 40, 'R 65 again')
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    finally:
        net.close()


@pytest.mark.parametrize('name', ['L3', 'D1'])
def test_ids_outside_the_table_clamp(name):
    """-1 and H (and far beyond) in a few rows of `cat` - and, lstm, of the sequence inputs: every row equals the restatement fed the
    ids clamped to [0, H - 1].  In the lstm forward the same `cat` row feeds k_emb_flatten and the category GRU (k_recur); both must
    follow the one rule."""
    from rl4rs_amd.device import DeviceSimnet
    algo, cfg, w, (seq, dense, cat), _, _, _, _ = _case(name, sc.TABLE_R)
    H, R, S = cfg['category_hash_size'], sc.TABLE_R, cfg['seq_num']
    cat, seq = cat.copy(), seq.copy()
    cat[3, 0], cat[4, -1], cat[31, 0], cat[64, -1] = -1, H, H + 100000, -7
    cat[33, :] = -1
    cat[34, :] = H
    if algo == 'lstm':
        seq[2, 0, 0], seq[5, 0, -1], seq[40, S - 1, 3], seq[64, S - 1, -1] = -1, H, -2 ** 31, 2 ** 31 - 1
    from oracle.simnets import OracleSimnet
    orc = OracleSimnet(algo, w, cfg, np.float64)
    cc, cs = np.clip(cat, 0, H - 1), np.clip(seq, 0, H - 1)
    net = DeviceSimnet(cfg, w, max_rows=R, max_slots=R, algo=algo)
    try:
        _encode_rows(net, seq)
        _check(net, R, 1, dense, cat, _iota_slots(S, R), orc.obs(cs, dense, cc), orc.reward_probs(cs, dense, cc)[:, 1],
               what='%s ids outside the table' % name)
    finally:
        net.close()


@pytest.mark.parametrize('algo', ['lstm', 'widedeep'])
def test_episode_at_maxlen_16(tmp_path, algo):
    """test_gpu_simnet.py::test_episode_with_other_simulators at maxlen 16: config['algo'] through SlateRecEnv + RecEnvBase against
    the oracle env.  Histories of up to 40 items (synth.make_records(max_hist=40); its default, 128, leaves none of the first ten
    records shorter than 16): some are truncated to their last 16, some left-padded - asserted from the records themselves."""
    import rl4rs_amd
    from rl4rs_amd import synth
    from rl4rs_amd.nets.simnets import init_simnet_weights, obs_dim
    from rl4rs.env.slate import SlateRecEnv, SlateState
    from oracle.simnets import OracleSimnet
    from oracle.env import OracleEnv
    B, T = sc.EPISODE_B, 9
    d = str(tmp_path)
    cat_path, log_path = os.path.join(d, 'item_info.csv'), os.path.join(d, 'log.csv')
    cat_text, records = sc.episode_records()
    lengths = sc.history_lengths(records[:B])
    assert max(lengths) > sc.EPISODE_MAXLEN and min(lengths) < sc.EPISODE_MAXLEN, lengths
    synth.write_text(cat_path, cat_text)
    synth.write_records(log_path, records)
    cfg = {"maxlen": sc.EPISODE_MAXLEN, "batch_size": B, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
           "category_feature_num": 21, "category_hash_size": 5000, "seq_num": 2, "emb_size": 128,
           "page_items": 9, "hidden_units": 128, "max_steps": T, "action_emb_size": 32,
           "sample_file": log_path, "iteminfo_file": cat_path, "is_eval": True, "cache_size": B, "algo": algo}
    w = init_simnet_weights(cfg, algo, seed=5, emb_scale=0.5, bias_noise=0.2)
    wpath = os.path.join(d, algo + '.npz')
    np.savez(wpath, **w)
    cfg['model_file'] = wpath
    env = rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))
    orc = OracleEnv(cfg, records[:B], OracleSimnet(algo, w, cfg, np.float64), seq=False)
    obs = env.reset(reset_file=True)
    o_obs = orc.reset()
    D = obs_dim(cfg, algo)
    assert obs.shape == (B, D) and env.observation_space.shape == (D,)
    assert np.abs(obs - o_obs['obs']).max() < 5e-5
    saw_reward = False
    for t in range(T):
        a = env.offline_action
        assert list(a) == list(orc.samples.offline_action)
        obs, reward, done, info = env.step(a)
        o_obs, o_reward, o_done, _ = orc.step(a)
        assert np.abs(obs - o_obs['obs']).max() < 5e-5
        np.testing.assert_allclose(np.asarray(reward, dtype=np.float64), np.asarray(o_reward, dtype=np.float64),
                                   rtol=1e-5, atol=1e-5)
        assert list(done) == list(o_done)
        saw_reward = saw_reward or np.abs(np.asarray(o_reward)).max() > 0
    assert saw_reward
