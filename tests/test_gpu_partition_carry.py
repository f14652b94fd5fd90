"""The duplicate-row partition carried from step to step (step.hip, row_refine.hpp, k_env_rows_refine): with the carry
on, the act kernel refines the partition of the previous forward by the action every env took and the forwards of the transition
take it through rl4rs_dien_set_row_partition instead of launching k_row_dedup.  Everything a transition returns - observation,
reward, done, the click probabilities - is compared bit for bit with config['no_partition_carry'] (the parent's launches), at every
step; the carried partition itself is read back (rl4rs_dien_buffer) and checked against the env's own dense / category rows.

Shapes: the smallest at which each path can go wrong - a run of one log line longer than ROW_DEDUP_CAP (chains, a split further
than the window from its root), a partial last 32-row tile, several envs per history slot."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = 64            # ROW_DEDUP_CAP of rl4rs_amd/csrc/row_dedup.hpp = ROW_REFINE_CAP of row_refine.hpp


def _pick(B, n_lines, big):
    """Line of every env: line 0 drawn `big` times, the others share the rest; shuffled so that the row order matters."""
    rest = np.arange(B - big) % (n_lines - 1) + 1
    pick = np.concatenate([np.zeros(big, dtype=np.int64), rest])
    return np.random.RandomState(5).permutation(pick)


def _make(tmp_path, monkeypatch, kind, B, pick, carry, fold=True, conti=False):
    import rl4rs_amd
    from rl4rs_amd import synth
    from rl4rs_amd.env.slate import SlateRecEnv, SlateState
    from rl4rs_amd.env.seqslate import SeqSlateRecEnv, SeqSlateState
    d = str(tmp_path)
    os.makedirs(d, exist_ok=True)
    seq = kind == 'seq'
    T = 18 if seq else 9
    n_lines = int(pick.max()) + 1
    text = synth.make_catalog_text(seed=4)
    synth.write_text(os.path.join(d, 'c.csv'), text)
    recs = synth.make_records(n_lines, pages=2 if seq else 1, seed=3, hash_size=2000, special_ids=synth.special_ids_from_text(text))
    synth.write_records(os.path.join(d, 'log.csv'), recs)
    cfg = {"maxlen": 64, "batch_size": B, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
           "category_feature_num": 21, "category_hash_size": 2000, "seq_num": 2, "emb_size": 128, "page_items": 9,
           "hidden_units": 128, "max_steps": T, "action_emb_size": 32, "sample_file": os.path.join(d, 'log.csv'),
           "iteminfo_file": os.path.join(d, 'c.csv'), "cache_size": n_lines, "model_seed": 3, "return_tensors": True,
           "scorer_kernels": 'augru_rows64', "scorer_precision": "fp16x2"}      # (the pin: a batch this small folds its reward step too)
    if not carry:
        cfg['no_partition_carry'] = True
    if not fold:
        cfg['no_reward_obs_fold'] = True
    if conti:
        cfg['support_conti_env'] = True
    real = np.random.choice

    def choice(a, size=None, *args, **kw):          # RecDataBase.sample draws the batch here: the scripted lines instead
        if isinstance(a, (int, np.integer)) and a == n_lines and size == B:
            return pick.copy()
        return real(a, size, *args, **kw)
    monkeypatch.setattr(np.random, 'choice', choice)
    if seq:
        env = rl4rs_amd.make('SeqSlateRecEnv-v0', recsim=SeqSlateRecEnv(cfg, state_cls=SeqSlateState))
    else:
        env = rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))
    env.seed(11)
    return env, T


def _partition(env, B):
    """What the LAST forward worked on -> (rep [B], active list, n_active) as numpy"""
    import torch
    from rl4rs_amd.device import DIEN_N_ACTIVE, DIEN_ROW_REP, DIEN_ROW_ACTIVE
    net = env.sim.model.device_net
    n_active = int(net.snapshot(DIEN_N_ACTIVE, 0)[0].item())
    rep = net.snapshot(DIEN_ROW_REP, B)[:B].cpu().numpy()
    active = net.snapshot(DIEN_ROW_ACTIVE, B)[:n_active].cpu().numpy()
    torch.cuda.synchronize()
    return rep, active, n_active


def _check_partition(env, B, rep, active, n_active):
    """rep is idempotent, active = the roots in processing order, and the env's rows of g and rep[g] are equal as bits"""
    from rl4rs_amd import device as D
    assert rep.min() >= 0 and rep.max() < B
    assert np.array_equal(rep[rep], rep)
    order = getattr(env.samples, '_row_order', None)
    order = np.arange(B) if order is None else order.cpu().numpy()
    assert list(active) == [int(g) for g in order if rep[g] == g] and len(active) == n_active
    live = env.samples._live()
    dense = live.snapshot(D.BUF_DENSE).cpu().numpy().view(np.uint32).reshape(B, -1)
    cat = live.snapshot(D.BUF_CATEGORY).cpu().numpy().reshape(B, -1)
    assert np.array_equal(dense, dense[rep]) and np.array_equal(cat, cat[rep])


def _alt(env, base, g, k):
    """The k-th legal item of env g (observation-side mask) that is not its logged one"""
    m = env.samples._obs_mask()[g]
    legal = [int(i) for i in m.nonzero().flatten().tolist() if int(i) != int(base[g])]
    assert len(legal) > k
    return legal[k]


def _drive(env, T, B, script, conti, carry, episodes=1, cut=None):
    """`episodes` episodes of offline_action replay with the deviations of `script` ({step: [(envs, k)]}: these envs take their k-th
    legal alternative).  `cut`: the first episode is abandoned after that many steps (a reset in mid-episode).
    -> (every tensor a transition returned, n_active of every forward's partition, (launched, carried) of the scorer)"""
    import torch
    out, parts = [], []
    net = None
    for ep in range(episodes):
        obs = env.reset()
        if net is None:
            net = env.sim.model.device_net
            net.profile_reset()                         # (behind the first reset observation: counted by hand below)
        out.append(obs.clone())
        rep, active, n_active = _partition(env, B)
        _check_partition(env, B, rep, active, n_active)
        parts.append(n_active)
        for t in range(T):
            a = env.offline_action
            a = a.clone() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
            if t in script:
                ids = env.samples._live().offline_action()          # the logged item ids (the continuous action is its embedding)
                emb = torch.as_tensor(np.asarray(env.samples.action_emb)).to(a.device) if conti else None
                for envs, k in script[t]:
                    item = _alt(env, ids, envs[0], k)
                    for g in envs:
                        if conti:
                            a[g] = emb[item].to(a.dtype)
                        else:
                            a[g] = item
            obs, reward, done, info = env.step(a)
            out += [obs.clone(), torch.as_tensor(reward).clone(), torch.as_tensor(np.asarray(done, dtype=np.int64))]
            rep, active, n_active = _partition(env, B)
            _check_partition(env, B, rep, active, n_active)
            parts.append(n_active)
            if cut is not None and ep == 0 and t + 1 >= cut:
                break
        if not (cut is not None and ep == 0):
            out.append(env.sim._stepper.click_probs().clone())
    return out, parts, net.dedup_counts()


def _same(a, b):
    import torch
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and x.shape == y.shape, i
        if x.dtype.is_floating_point:
            x, y = x.contiguous().view(torch.int32 if x.dtype == torch.float32 else torch.int64), y.contiguous().view(torch.int32 if y.dtype == torch.float32 else torch.int64)
        assert torch.equal(x.cpu(), y.cpu()), i


def _slate_script(pick):
    """Steps 2 and 5: envs of line 0 (70 envs, consecutive in processing order) and of line 1 take other legal items - a group of
    several envs of which some sit more than 63 positions behind their root, a singleton, a pair whose members are more than a
    window apart; at step 5 the first of those groups splits again."""
    l0 = np.flatnonzero(pick == 0)           # ascending env index = their processing order (stable sort by slot)
    l1 = np.flatnonzero(pick == 1)
    assert len(l0) > CAP + 5
    return {2: [(list(l0[10:14]) + list(l0[66:69]), 0),     # several envs; l0[66] finds l0[10] 56 positions in front, l0[67] finds it too
                ([l0[20]], 1),                               # a singleton
                ([l0[1], l0[69]], 2),                        # two envs 68 positions apart: the second finds nobody inside the window
                (list(l1[:2]), 0)],
            5: [(list(l0[11:13]) + [l0[67]], 1),             # the first group splits again
                ([l0[40]], 0),
                (list(l1[1:3]), 1)]}


@pytest.mark.parametrize('drive', ['replay', 'scripted'])
def test_slate_episode_is_bit_identical_and_the_partition_holds(tmp_path, monkeypatch, drive):
    """SlateRecEnv, B = 96 from 5 log lines, line 0 drawn 70 times, T = 9.  (replay) nothing splits: n_active equals the content
    search's at every forward, k_row_dedup runs once per episode.  (scripted) splits at steps 2 and 5: never more representatives
    than the content search."""
    B = 96
    pick = _pick(B, 5, 70)
    script = _slate_script(pick) if drive == 'scripted' else {}
    env, T = _make(tmp_path / 'on', monkeypatch, 'slate', B, pick, True)
    on, p_on, c_on = _drive(env, T, B, script, False, True)
    env, T = _make(tmp_path / 'off', monkeypatch, 'slate', B, pick, False)
    off, p_off, c_off = _drive(env, T, B, script, False, False)
    _same(on, off)
    print(drive, 'n_active per forward, carried', p_on, 'content', p_off, 'dedup launches (launched, carried)', c_on, c_off)
    assert float(on[-2].double().abs().sum()) > 0                       # the reward step paid
    assert all(a <= b for a, b in zip(p_on, p_off))
    assert 1 < p_on[0] <= 5 + 1                                          # the reset: 5 lines, line 0 in two chained windows
    # forwards behind the reset observation: 8 observation forwards and the folded reward forward
    assert c_off == (9, 0) and c_on == (0, 9)
    if drive == 'replay':
        assert p_on == p_off
    else:
        assert p_on[3] > p_on[2] and p_on[6] > p_on[5]                  # both scripted steps split something


def test_two_forward_reward_step_gets_the_partition_twice(tmp_path, monkeypatch):
    """config['no_reward_obs_fold'] with the carry: the reward step's observation forward and its 8-row reward forward both take
    the partition (10 carried forwards), results as with the carry off."""
    B = 96
    pick = _pick(B, 5, 70)
    script = _slate_script(pick)
    env, T = _make(tmp_path / 'on', monkeypatch, 'slate', B, pick, True, fold=False)
    on, p_on, c_on = _drive(env, T, B, script, False, True)
    env, T = _make(tmp_path / 'off', monkeypatch, 'slate', B, pick, False, fold=False)
    off, p_off, c_off = _drive(env, T, B, script, False, False)
    _same(on, off)
    assert c_on == (0, 10) and c_off == (10, 0)
    assert all(a <= b for a, b in zip(p_on, p_off))


def test_reset_in_mid_episode_then_a_second_episode(tmp_path, monkeypatch):
    """Four steps, a reset(), then a whole episode: the reset drops the partition, the second episode is seeded by its own reset
    observation (one k_row_dedup launch per reset)."""
    B = 96
    pick = _pick(B, 5, 70)
    script = _slate_script(pick)
    env, T = _make(tmp_path / 'on', monkeypatch, 'slate', B, pick, True)
    on, p_on, c_on = _drive(env, T, B, script, False, True, episodes=2, cut=4)
    env, T = _make(tmp_path / 'off', monkeypatch, 'slate', B, pick, False)
    off, p_off, c_off = _drive(env, T, B, script, False, False, episodes=2, cut=4)
    _same(on, off)
    assert c_on == (1, 4 + 9) and c_off == (1 + 4 + 9, 0)              # (the second reset observation is inside the counted span)
    assert all(a <= b for a, b in zip(p_on, p_off))


@pytest.mark.parametrize('drive', ['replay', 'scripted'])
def test_continuous_env(tmp_path, monkeypatch, drive):
    """The continuous-action transition, B = 64 from 4 lines: the key of the refinement is the item the K-NN resolved."""
    B = 64
    pick = _pick(B, 4, 40)
    l0 = np.flatnonzero(pick == 0)
    script = {2: [(list(l0[3:6]), 0), ([l0[20]], 1)], 5: [(list(l0[4:6]) + [l0[30]], 1)]} if drive == 'scripted' else {}
    env, T = _make(tmp_path / 'on', monkeypatch, 'slate', B, pick, True, conti=True)
    on, p_on, c_on = _drive(env, T, B, script, True, True)
    env, T = _make(tmp_path / 'off', monkeypatch, 'slate', B, pick, False, conti=True)
    off, p_off, c_off = _drive(env, T, B, script, True, False)
    _same(on, off)
    print(drive, 'n_active per forward, carried', p_on, 'content', p_off, c_on, c_off)
    assert c_on == (0, 9) and c_off == (9, 0)
    assert all(a <= b for a, b in zip(p_on, p_off))
    if drive == 'replay':
        assert p_on == p_off
    else:
        assert p_on[-1] > p_on[0]


def test_seqslate_page_turn_drops_the_partition(tmp_path, monkeypatch):
    """SeqSlateRecEnv, B = 32, T = 18: the first act of the second page re-encodes every env's second input into a slot of its own -
    the forwards of that transition compare rows again (and find every env distinct).  Bit-identical on both pages."""
    B = 32
    pick = _pick(B, 4, 20)
    l0 = np.flatnonzero(pick == 0)
    script = {3: [(list(l0[2:5]), 0)], 12: [(list(l0[6:8]), 1)]}
    env, T = _make(tmp_path / 'on', monkeypatch, 'seq', B, pick, True)
    on, p_on, c_on = _drive(env, T, B, script, False, True)
    env, T = _make(tmp_path / 'off', monkeypatch, 'seq', B, pick, False)
    off, p_off, c_off = _drive(env, T, B, script, False, False)
    _same(on, off)
    print('n_active per forward, carried', p_on, 'content', p_off, c_on, c_off)
    assert all(a <= b for a, b in zip(p_on, p_off))
    assert p_on[9] < B and p_on[10] == B                                # first page: duplicates; second page: none
    assert c_off[1] == 0 and c_on[0] >= 1 and c_on[0] + c_on[1] == c_off[0]
    assert c_on[0] < c_off[0] // 2


def test_scorer_takes_a_partition_from_its_caller(tmp_path):
    """rl4rs_dien_set_row_partition on the scorer alone: a forward that is handed the partition a content forward found launches no
    k_row_dedup and returns the same bits; the arming is one-shot; a partition for another number of groups is an error."""
    import torch
    from rl4rs_amd import _lib
    from rl4rs_amd.device import DeviceDien, DIEN_N_ACTIVE, DIEN_ROW_REP, DIEN_ROW_ACTIVE
    from rl4rs_amd.nets.dien import init_dien_weights
    cfg = {"maxlen": 16, "batch_size": 8, "action_size": 284, "class_num": 2, "dense_feature_num": 432, "category_feature_num": 21,
           "category_hash_size": 2000, "seq_num": 2, "emb_size": 128, "hidden_units": 128, "scorer_precision": "fp16x2"}
    rs = np.random.RandomState(2)
    R, nslots = 80, 6
    net = DeviceDien(cfg, init_dien_weights(cfg, seed=9, emb_scale=0.5, bias_noise=0.2), max_rows=R, max_slots=nslots)
    seq = rs.randint(1, 284, size=(nslots, 2, 16)).astype(np.int32)
    for s in range(2):
        net.encode(s, torch.from_numpy(np.ascontiguousarray(seq[:, s])).cuda(), 0)
    tpl_d = np.abs(rs.randn(7, 432) * 3).astype(np.float32)
    tpl_c = rs.randint(0, 284, size=(7, 21)).astype(np.int32)
    which = np.sort(rs.randint(0, 7, size=R))                            # rows of one template are neighbours
    dense, cat = torch.from_numpy(tpl_d[which]).cuda(), torch.from_numpy(tpl_c[which]).cuda()
    slots = torch.from_numpy(np.stack([which % nslots, which % 2]).astype(np.int32)).cuda()
    obs0, p0 = net.forward(R, 1, dense, cat, slots, True, True)
    n_active = net.snapshot(DIEN_N_ACTIVE, 0).clone()
    rep = net.snapshot(DIEN_ROW_REP, R)[:R].clone()
    active = net.snapshot(DIEN_ROW_ACTIVE, R)[:R].clone()
    assert int(n_active.item()) == 7
    net.profile_reset()
    net.set_row_partition(rep, active, n_active)
    obs1, p1 = net.forward(R, 1, dense, cat, slots, True, True)
    assert net.dedup_counts() == (0, 1)
    assert int(net.snapshot(DIEN_N_ACTIVE, 0).item()) == 7 and net.snapshot(DIEN_ROW_REP, R).numel() == R
    obs2, p2 = net.forward(R, 1, dense, cat, slots, True, True)          # one-shot: this one compares rows again
    assert net.dedup_counts() == (1, 1)
    for a, b in ((obs0, obs1), (p0, p1), (obs0, obs2), (p0, p2)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    net.set_row_partition(rep[:40].contiguous(), active, n_active)
    with pytest.raises(_lib.Rl4rsHipError):
        net.forward(R, 1, dense, cat, slots, True, True)
    obs3, _ = net.forward(R, 1, dense, cat, slots, True, True)           # the failed call disarmed it
    assert torch.equal(obs0.view(torch.int32), obs3.view(torch.int32))
    net.check_status()
    net.close()
