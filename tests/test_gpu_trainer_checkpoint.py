"""GPU: ``save`` / ``restore`` of the online trainers (``train._Checkpoint``) and ``Trainer.evaluate``.

An on-policy trainer restored into a fresh process-equivalent (fresh env over the same files, fresh trainer with the same ``seed`` and
another ``init_seed``) continues bit for bit; a replay trainer comes back with bit-equal networks, targets, Adam state and
counters and an EMPTY ring that refills from its next rollout."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _env(d, conti=False, B=64, T=9):
    """the synthetic 64 x 9 SlateRecEnv of tests/test_gpu_dqn.py::_env (``conti``: the continuous-action form of tests/test_gpu_td3.py)"""
    import rl4rs_amd
    from rl4rs_amd import synth
    from rl4rs_amd.env.slate import SlateRecEnv, SlateState
    text = synth.make_catalog_text(seed=4)
    synth.write_text(os.path.join(d, 'c.csv'), text)
    recs = synth.make_records(300, seed=2, hash_size=2000, special_ids=synth.special_ids_from_text(text))
    synth.write_records(os.path.join(d, 'log.csv'), recs)
    cfg = {"maxlen": 64, "batch_size": B, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
           "category_feature_num": 21, "category_hash_size": 2000, "seq_num": 2, "emb_size": 128, "page_items": 9,
           "hidden_units": 128, "max_steps": T, "action_emb_size": 32, "sample_file": os.path.join(d, 'log.csv'),
           "iteminfo_file": os.path.join(d, 'c.csv'), "cache_size": 256, "model_seed": 3, "return_tensors": True}
    if conti:
        cfg["support_conti_env"] = True
    return rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))


def _make(kind, env, init_seed, **kw):
    from rl4rs_amd import train as T
    if kind == 'ContiPPO':
        return T.ContiTrainer(env, 'PPO', hidden=64, seed=3, init_seed=init_seed, minibatch=256, **kw)
    if kind == 'IMPALA':
        return T.Trainer(env, 'IMPALA', seed=3, init_seed=init_seed, broadcast_interval=2, drop_last=False, **kw)
    if kind in ('A2C', 'PPO', 'PG'):
        return T.Trainer(env, kind, seed=3, init_seed=init_seed, minibatch=256, **kw)
    replay = dict(seed=3, init_seed=init_seed, learning_starts=500, train_batch_size=256, buffer_size=2000)
    if kind == 'DQN':
        return T.DQNTrainer(env, **dict(replay, **kw))
    if kind == 'RAINBOW':
        return T.RainbowTrainer(env, **dict(replay, **kw))
    return T.TD3Trainer(env, algo=kind, random_timesteps=600, **dict(replay, **kw))


def _nets(tr):
    """{name: (params, m, v, t)} of every handle a checkpoint covers, and the tensors beside them"""
    import torch
    out = {}
    for name, net, adam in tr._ckpt_nets():
        out[name] = (net.params(),) + (tuple(net.adam_state()) if adam else ())
    for name, t in tr._ckpt_tensors().items():
        out['tensor.' + name] = (t.clone(),)
    return out


def _assert_same_nets(a, b):
    import torch
    na, nb = _nets(a), _nets(b)
    assert sorted(na) == sorted(nb)
    for name in na:
        for x, y in zip(na[name], nb[name]):
            assert torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y, name


# ---- 5. on-policy continuation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['A2C', 'PPO', 'PG', 'IMPALA', 'ContiPPO'])
def test_on_policy_continuation_is_bit_identical(tmp_path, kind):
    import torch
    conti = kind == 'ContiPPO'
    path = str(tmp_path / 'trainer.npz')

    def two_more(tr, env):
        env.seed(77)
        env.reset(reset_file=True)
        return [dict(tr.train_iteration()) for _ in range(2)]

    env_x = _env(str(tmp_path), conti)
    env_x.seed(5)
    x = _make(kind, env_x, init_seed=1)
    for _ in range(3):
        x.train_iteration()
    x.save(path)
    if kind == 'IMPALA':                                   # three updates, broadcast every second: the actor trails the learner
        assert x.num_updates == 3 and not torch.equal(x.actor.params(), x.policy.params())
    if kind == 'PPO':
        assert x.B * x.T // x.minibatch == 2
    stats_x = two_more(x, env_x)
    env_y = _env(str(tmp_path), conti)
    y = _make(kind, env_y, init_seed=2)
    assert not torch.equal(y.policy.params(), x.policy.params())
    y.restore(path)
    assert y.iteration == 3 and y._rollouts == 3
    stats_y = two_more(y, env_y)
    _assert_same_nets(x, y)
    assert x.policy.adam_state()[2] == y.policy.adam_state()[2] > 0
    assert x.kl_coeff == y.kl_coeff and x.iteration == y.iteration == 5 and x._rollouts == y._rollouts and x.num_updates == y.num_updates
    assert stats_x == stats_y, (stats_x, stats_y)
    assert np.isfinite([v for s in stats_x for v in s.values()]).all()
    x.close()
    y.close()


# ---- 6. replay trainers -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['DQN', 'RAINBOW', 'TD3', 'DDPG'])
def test_replay_trainer_comes_back_with_an_empty_ring(tmp_path, kind):
    import torch
    conti = kind in ('TD3', 'DDPG')
    path = str(tmp_path / 'trainer.npz')
    env_x = _env(str(tmp_path), conti)
    env_x.seed(5)
    x = _make(kind, env_x, init_seed=1, target_network_update_freq=1000) if not conti else _make(kind, env_x, init_seed=1)
    for _ in range(3):
        st = x.train_iteration()
    assert st['num_updates'] == 3 and x.replay.rows == 3 * 576
    x.save(path)
    env_y = _env(str(tmp_path), conti)
    y = _make(kind, env_y, init_seed=2, target_network_update_freq=1000) if not conti else _make(kind, env_y, init_seed=2)
    y.restore(path)
    _assert_same_nets(x, y)
    for name in x._ckpt_host:
        assert getattr(x, name) == getattr(y, name) and type(getattr(x, name)) is type(getattr(y, name)), name
    assert y.timesteps == 3 * 576 and y.num_updates == 3
    if conti:
        assert torch.equal(x._gen.get_state(), y._gen.get_state()) and y.ou_state.abs().sum().item() > 0
    else:
        assert y.num_target_updates == x.num_target_updates == 1 and not torch.equal(y.target, y.policy.params())
    assert y.evaluate(128, seed=11) == x.evaluate(128, seed=11)
    assert y.replay.rows == 0 and y.replay in y._owned
    st = y.train_iteration()                               # pushes its one new rollout, then samples from it
    assert st['num_updates'] == 4 and st['buffer_rows'] == 576 and st['iteration'] == 4
    assert np.isfinite(list(st.values())).all()
    x.close()
    y.close()


# ---- 7. refusals and evaluate -------------------------------------------------------------------------------------------
def test_restore_refuses_another_class_algo_or_shape(tmp_path):
    import torch
    from rl4rs_amd import train as T
    env = _env(str(tmp_path))
    env.seed(5)
    a2c = _make('A2C', env, init_seed=1)
    a2c.train_iteration()
    a2c.save(str(tmp_path / 'a2c.npz'))
    dqn = _make('DQN', env, init_seed=1)
    dqn.train_iteration()
    dqn.save(str(tmp_path / 'dqn.npz'))
    for other, fname, sides in ((_make('PPO', env, init_seed=2), 'a2c.npz', ("'A2C'", "'PPO'")),
                                (T.Trainer(env, 'A2C', hidden=128, seed=3, init_seed=2), 'a2c.npz', ('["hidden", 64]', '["hidden", 128]')),
                                (_make('RAINBOW', env, init_seed=2), 'dqn.npz', ('DQNTrainer', 'RainbowTrainer'))):
        before = other.policy.params()
        with pytest.raises(ValueError) as e:
            other.restore(str(tmp_path / fname))
        assert all(s in str(e.value) for s in sides), str(e.value)
        assert torch.equal(other.policy.params(), before) and other.iteration == 0
        other.close()
    # save after a train call includes that call: its deferred statistics are settled by save
    b = _make('A2C', env, init_seed=1)
    b.train_iteration()
    assert b._pending
    b.save(str(tmp_path / 'b.npz'))
    assert not b._pending
    with np.load(str(tmp_path / 'b.npz')) as z:
        assert int(z['host.iteration']) == 1 and int(z['net.policy.adam_t']) == 1
        assert np.array_equal(z['net.policy.params'], b.policy.params().cpu().numpy())
    for tr in (a2c, dqn, b):
        tr.close()


@pytest.mark.parametrize('algo', ['A2C', 'IMPALA'])
def test_trainer_evaluate_is_greedy_legal_and_deterministic(tmp_path, algo):
    import torch
    env = _env(str(tmp_path))
    env.seed(5)
    tr = _make(algo, env, init_seed=1)
    for _ in range(2):
        tr.train_iteration()
    state = np.random.get_state()
    e0 = tr.evaluate(128, seed=11)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    assert np.isfinite(e0) and e0 == tr.evaluate(128, seed=11)
    assert env.samples.get_violation().all()               # the greedy action of the masked logits is always legal
    if algo == 'IMPALA':
        # evaluate plays the learner: a stale (here: garbage) actor changes nothing
        tr.actor.set_params(torch.randn(tr.actor.n_params, device='cuda'))
        assert tr.evaluate(128, seed=11) == e0
    tr.close()
