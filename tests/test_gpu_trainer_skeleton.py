"""GPU: what the shared trainer skeleton of rl4rs_amd/train.py (deferred statistics, replay loop, evaluate frame)
promises for every trainer: the statistics mapping of a train call has exactly the trainer's keys, every value is finite, and
deferring the read changes WHEN the numbers arrive, not WHICH numbers - the first call's mapping read after the second call was
issued equals what an identical trainer returns when its first mapping is read at once.  ``kl_coeff`` belongs to the on-policy
trainers alone.  B = 64, T = 9 on the synthetic envs of the trainers' own tests."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, T = 64, 9
ON_POLICY = ['episode_reward_mean', 'policy_loss', 'vf_loss', 'entropy', 'kl', 'kl_mean', 'kl_coeff', 'iteration']
DQN = ['episode_reward_mean', 'td_loss', 'mean_q', 'mean_td_abs', 'buffer_rows', 'num_updates', 'num_target_updates', 'iteration']
TD3 = ['episode_reward_mean', 'critic_loss', 'actor_loss', 'mean_q', 'mean_td_abs', 'buffer_rows', 'num_updates', 'iteration']
EXACTK = ['episode_reward_mean', 'reward_first_climb', 'baseline_mean', 'critic_loss', 'policy_loss', 'invalid_targets', 'skipped',
          'skipped_total', 'iteration']
REPLAY = dict(seed=3, init_seed=9, learning_starts=1000, train_batch_size=128, buffer_size=2000)      # 576 steps per call: the second call updates

# name -> (env kind, trainer class, constructor arguments, keys of the mapping, has kl_coeff)
CASES = {
    'a2c': ('discrete', 'Trainer', dict(algo='A2C', seed=3, init_seed=9), ON_POLICY, True),
    'ppo': ('discrete', 'Trainer', dict(algo='PPO', seed=3, init_seed=9, minibatch=128), ON_POLICY, True),
    'pg': ('discrete', 'Trainer', dict(algo='PG', seed=3, init_seed=9), ON_POLICY, True),
    'impala': ('discrete', 'Trainer', dict(algo='IMPALA', seed=3, init_seed=9, broadcast_interval=2, drop_last=False),
               ON_POLICY + ['rho_mean', 'rho_clipped_mean', 'vs_mean'], True),
    'dqn': ('discrete', 'DQNTrainer', REPLAY, DQN, False),
    'rainbow': ('discrete', 'RainbowTrainer', dict(REPLAY, masked=True), DQN + ['mean_target'], False),
    'td3': ('conti', 'TD3Trainer', dict(REPLAY, algo='TD3', random_timesteps=576), TD3, False),
    'ddpg': ('conti', 'TD3Trainer', dict(REPLAY, algo='DDPG', random_timesteps=576), TD3, False),
    'exactk': ('discrete', 'ExactKTrainer', dict(seed=1, init_seed=2), EXACTK, False),
    'raw_a2c': ('raw', 'RawStateTrainer', dict(algo='A2C', seed=1, lr=1e-3), ON_POLICY, True),
}


def _write_files(d, kind):
    """The catalogue and log of tests/test_gpu_dqn.py::_env (and test_gpu_td3.py), or of test_rawstate_training_loop -> config."""
    from rl4rs_amd import synth
    raw = kind == 'raw'
    text = synth.make_catalog_text(seed=21 if raw else 4)
    cpath, lpath = os.path.join(d, 'c.csv'), os.path.join(d, 'log.csv')
    synth.write_text(cpath, text)
    special = synth.special_ids_from_text(text)
    if raw:
        recs = synth.make_records(B + 3, pages=1, seed=8, illegal_frac=0.0, hash_size=5000, special_ids=special)
    else:
        recs = synth.make_records(300, seed=2, hash_size=2000, special_ids=special)
    synth.write_records(lpath, recs)
    cfg = {"maxlen": 64, "batch_size": B, "action_size": 284, "class_num": 2, "dense_feature_num": 432, "category_feature_num": 21,
           "category_hash_size": 5000 if raw else 2000, "seq_num": 2, "emb_size": 128, "page_items": 9, "hidden_units": 128,
           "max_steps": T, "action_emb_size": 32, "sample_file": lpath, "iteminfo_file": cpath, "cache_size": B if raw else 256,
           "model_seed": 3, "return_tensors": True}
    if raw:
        cfg.update({"is_eval": False, "support_rllib_mask": True, "rawstate_as_obs": True})
    if kind == 'conti':
        cfg["support_conti_env"] = True
    return cfg


def _trainer(cfg, cls, kw):
    """A fresh env and trainer from the same files and seeds (the env draws its batches with numpy's global generator)."""
    import rl4rs_amd
    from rl4rs_amd import train
    from rl4rs_amd.env.slate import SlateRecEnv, SlateState
    env = rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(dict(cfg), state_cls=SlateState))
    env.seed(7)
    np.random.seed(1000)
    return getattr(train, cls)(env, **kw)


@pytest.mark.parametrize('name', list(CASES))
def test_deferred_statistics_have_the_trainers_keys_and_the_immediate_numbers(tmp_path, name):
    kind, cls, kw, keys, has_kl = CASES[name]
    cfg = _write_files(str(tmp_path), kind)
    tr = _trainer(cfg, cls, kw)
    first = tr.train_iteration()
    second = tr.train_iteration()                           # issued before anybody looked at ``first``
    first, second = dict(first), dict(second)
    for st in (first, second):
        assert sorted(st) == sorted(keys), (name, sorted(st))
        assert all(np.isfinite(v) for v in st.values()), (name, st)
    assert (first['iteration'], second['iteration']) == (1, 2)
    if 'num_updates' in keys:
        assert first['num_updates'] == 0 and second['num_updates'] == 1          # learning_starts lies between the two calls
    assert hasattr(tr, 'kl_coeff') == has_kl
    twin = _trainer(cfg, cls, kw)
    at_once = dict(twin.train_iteration())                  # read immediately
    print(name, first)
    assert at_once == first, (name, at_once, first)
    assert hasattr(twin, 'kl_coeff') == has_kl
