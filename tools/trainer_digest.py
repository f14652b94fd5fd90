#!/usr/bin/env python
"""sha256 per trainer configuration of what 6 train calls and one evaluate(episodes=128, seed=11) leave behind at B = 64, T = 9 on the
synthetic env of the trainer tests: every network's flat parameters and Adam moments, step counters, target parameters, the filled
replay columns and every call's statistics as float64.  For bit-identity A/Bs of rl4rs_amd/train.py between two trees that share
one library (profiles/r19_trainer_digest.md):
    python tools/trainer_digest.py                                        (this tree)
    python tools/trainer_digest.py --tree tools/_ab/parent                (another tree with its own Python)
Prints one line `DIGEST <config> <sha256>` per configuration.  The raw-state trainer scatters its embedding gradients with float
atomicAdd, so two runs of one tree differ: its line is `DIGEST raw_a2c_rollout <sha256>` over the first rollout's actions and
rewards (they precede any update), and --raw-params FILE.npy saves its final flat parameters for a max-abs comparison."""
import argparse
import hashlib
import os
import sys
import tempfile

import numpy as np

CONFIGS = ('a2c', 'ppo', 'pg', 'impala', 'dqn', 'rainbow', 'td3', 'ddpg', 'exactk', 'raw_a2c')
B, T, CALLS = 64, 9, 6


def build_env(d, kind):
    """'discrete' / 'conti': the env of tests/test_gpu_dqn.py / test_gpu_td3.py; 'raw': that of test_rawstate_training_loop."""
    import rl4rs_amd
    from rl4rs_amd import synth
    from rl4rs_amd.env.slate import SlateRecEnv, SlateState
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
    env = rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))
    env.seed(7)
    return env


def build_trainer(name, env):
    from rl4rs_amd import train
    replay = dict(seed=3, init_seed=9, learning_starts=576, train_batch_size=256, buffer_size=2000)
    if name in ('a2c', 'pg'):
        return train.Trainer(env, algo=name.upper(), seed=3, init_seed=9)
    if name == 'ppo':
        return train.Trainer(env, algo='PPO', seed=3, init_seed=9, minibatch=128)
    if name == 'impala':
        return train.Trainer(env, algo='IMPALA', seed=3, init_seed=9, broadcast_interval=2, drop_last=False)
    if name == 'dqn':
        return train.DQNTrainer(env, target_network_update_freq=1500, **replay)
    if name == 'rainbow':
        return train.RainbowTrainer(env, target_network_update_freq=1500, masked=True, **replay)
    if name in ('td3', 'ddpg'):
        return train.TD3Trainer(env, algo=name.upper(), random_timesteps=576, **replay)
    if name == 'exactk':
        return train.ExactKTrainer(env, seed=1, init_seed=2)
    return train.RawStateTrainer(env, algo='A2C', seed=1, lr=1e-3)


def networks(name, tr):
    """[(label, handle)] of every network of the trainer, in a fixed order."""
    if name in ('td3', 'ddpg'):
        return list(tr.learner.named)
    nets = [('policy', tr.policy)]
    if getattr(tr, 'actor', None) is not None:
        nets.append(('actor', tr.actor))
    if name == 'exactk':
        nets.append(('critic', tr.critic))
    return nets


def run(name):
    import torch
    kind = 'conti' if name in ('td3', 'ddpg') else 'raw' if name == 'raw_a2c' else 'discrete'
    h = hashlib.sha256()
    put = lambda t: h.update(np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, 'detach') else t).tobytes())
    with tempfile.TemporaryDirectory() as d:
        env = build_env(d, kind)
        np.random.seed(1000)
        tr = build_trainer(name, env)
        if name == 'raw_a2c':
            first = tr.train_iteration()
            put(tr.buf['act'])
            put(tr.buf['rew'])
            stats = [first] + [tr.train_iteration() for _ in range(CALLS - 1)]
            assert all(np.isfinite(list(s.values())).all() for s in stats)
            return h.hexdigest(), tr.policy.params().cpu().numpy()
        stats = [tr.train_iteration() for _ in range(CALLS)]
        for s in stats:
            put(np.array([float(s[k]) for k in sorted(s.keys())], dtype=np.float64))
        if hasattr(tr, 'evaluate'):
            put(np.array([tr.evaluate(episodes=128, seed=11)], dtype=np.float64))
        for _, net in networks(name, tr):
            m, v, t = net.adam_state()
            for x in (net.params(), m, v, np.array([t], dtype=np.int64)):
                put(x)
        counters = [getattr(tr, k, -1) for k in ('iteration', 'num_updates', 'num_target_updates', 'timesteps', 'skipped_total')]
        put(np.array(counters, dtype=np.int64))
        if hasattr(tr, 'target'):
            put(tr.target)
        if hasattr(tr, 'ou_state'):
            put(tr.ou_state)
        if hasattr(tr, 'replay'):
            rows = tr.replay.rows
            for col in sorted(tr.replay._DTYPES):
                c = tr.replay.column(col)
                put(c if col == 'max_priority' else c[:rows])
        torch.cuda.synchronize()
        return h.hexdigest(), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--configs', default=','.join(CONFIGS))
    ap.add_argument('--raw-params', default=None, help='save the raw-state trainer\'s final flat parameters here (.npy)')
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    torch.cuda.set_device(0)
    for name in a.configs.split(','):
        digest, raw = run(name)
        print('DIGEST %s %s' % (name + '_rollout' if raw is not None else name, digest), flush=True)
        if raw is not None and a.raw_params:
            np.save(a.raw_params, raw)


if __name__ == '__main__':
    main()
