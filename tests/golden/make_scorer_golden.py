#!/usr/bin/env python
"""Generate the offline-scorer fixtures (tests/golden/scorer_*.npz) by running the REFERENCE's own code: the four functions of
rl4rs/utils/d3rlpy_scorer.py - ``soft_opc_scorer``, ``discrete_action_match_scorer`` and the two dynamics reward-error scorers -
over table-driven fakes.

The reference module is loaded from its file under stub ``d3rlpy.metrics.scorer`` / ``d3rlpy.dataset`` / ``rl4rs.policy.policy_model``
modules; the stubs hold this generator's own ``_make_batches`` (windows of ``window_size`` consecutive transitions of an episode)
and an ``Episode`` with ``compute_return`` = ``sum(rewards[1:])`` (d3rlpy 0.91).  Nothing of the reference is copied: the fixtures
hold inputs, thresholds and results only.  A fake ``predict_q`` / ``predict_with_mask`` reads seeded tables by the row number an
observation carries.

* ``scorer_mixed.npz``   one dataset with episodes of 1, 2, 10, 37 and 1030 rows (the last crosses the 1024-row window);
* ``scorer_tens.npz``    300 episodes of 10 rows;
each with three thresholds: some episodes succeed, none (NaN), all.

    python tests/golden/make_scorer_golden.py [--out DIR]

It ends by re-loading what it wrote and comparing."""
import argparse
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
A = 284
CASES = (('scorer_mixed.npz', (1, 2, 10, 37, 1030), 11), ('scorer_tens.npz', (10,) * 300, 12))


class Episode(object):
    """rows of one episode: ``rewards[t]`` is stored with observation t (the reward of the action before it)"""

    def __init__(self, observations, actions, rewards):
        self.observations, self.actions, self.rewards = observations, actions, rewards

    def compute_return(self):
        return np.sum(self.rewards[1:])

    def __len__(self):
        return len(self.observations)


def _make_batches(episode, window_size, n_frames):
    n = len(episode)
    next_rewards = np.concatenate([episode.rewards[1:], np.zeros(1, dtype=episode.rewards.dtype)])
    for lo in range(0, n, window_size):
        hi = min(lo + window_size, n)
        yield types.SimpleNamespace(observations=episode.observations[lo:hi], actions=episode.actions[lo:hi],
                                    next_rewards=next_rewards[lo:hi].reshape(-1, 1))


def load_reference():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    mod('d3rlpy')
    mod('d3rlpy.metrics')
    mod('d3rlpy.metrics.scorer', AlgoProtocol=object, _make_batches=_make_batches)
    mod('d3rlpy.dataset', Episode=Episode)
    mod('rl4rs')
    mod('rl4rs.policy')
    mod('rl4rs.policy.policy_model', policy_model=object)
    spec = importlib.util.spec_from_file_location('ref_d3rlpy_scorer', os.path.join(REF, 'rl4rs', 'utils', 'd3rlpy_scorer.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class Tables(object):
    """the fake ``policy_model``: every answer is a seeded table indexed by the row number in column 0 of an observation"""

    def __init__(self, lengths, seed):
        rs = np.random.RandomState(seed)
        self.lengths = np.asarray(lengths, dtype=np.int64)
        n = int(self.lengths.sum())
        self.qd = rs.normal(50.0, 20.0, n).astype(np.float32)
        self.a = rs.randint(0, A, size=n).astype(np.int32)
        self.a_mask = np.where(rs.rand(n) < 0.55, self.a, rs.randint(0, A, size=n)).astype(np.int32)
        self.rhat = rs.normal(5.0, 3.0, n).astype(np.float32)
        # next rewards: 0 on the terminal row of each episode, as the transition rule leaves it
        self.next_rewards = (rs.rand(n) * 20.0).astype(np.float32)
        self.next_rewards[np.cumsum(self.lengths) - 1] = 0.0
        self.policy = types.SimpleNamespace(n_frames=1)

    def episodes(self):
        out, lo = [], 0
        for T in self.lengths:
            rows = np.arange(lo, lo + T)
            rewards = np.concatenate([np.zeros(1, dtype=np.float32), self.next_rewards[lo:lo + T - 1]])
            out.append(Episode(rows.astype(np.float64).reshape(-1, 1), self.a[lo:lo + T].reshape(-1, 1), rewards))
            lo += T
        return out

    @staticmethod
    def _rows(obs):
        return np.asarray(obs)[:, 0].astype(np.int64)

    def predict_q(self, obs, actions):
        rows = self._rows(obs)
        assert np.array_equal(np.asarray(actions).reshape(-1), self.a[rows])
        return self.qd[rows]

    def predict_with_mask(self, obs):
        return self.a_mask[self._rows(obs)]


class DynamicsTables(object):
    def __init__(self, tables):
        self.t = tables
        self.policy = tables.policy

    def predict_q(self, obs, actions):
        return None, self.t.rhat[Tables._rows(obs)].reshape(-1, 1)


def case(ref, lengths, seed):
    t = Tables(lengths, seed)
    episodes = t.episodes()
    returns = np.asarray([float(e.compute_return()) for e in episodes])
    srt = np.sort(returns)
    mid = 0.5 * (srt[len(srt) // 2 - 1] + srt[len(srt) // 2]) if len(srt) > 1 else srt[0] - 1.0
    thresholds = np.asarray([mid, srt[-1] + 10.0, srt[0] - 10.0], dtype=np.float64)       # some succeed, none, all
    # the reference sums float32 rewards, the device float64: no return may sit within 1e-3 of a threshold
    assert (np.abs(returns[:, None] - thresholds[None, :]) > 1e-3).all(), (returns, thresholds)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        soft_opc = np.asarray([ref.soft_opc_scorer(float(th))(t, episodes) for th in thresholds], dtype=np.float64)
    n_success = np.asarray([(returns >= th).sum() for th in thresholds])
    assert 0 < n_success[0] < len(episodes) and n_success[1] == 0 and n_success[2] == len(episodes), n_success
    assert np.isfinite(soft_opc[0]) and np.isnan(soft_opc[1]) and abs(soft_opc[2]) <= 1e-9 * abs(np.mean(t.qd.astype(np.float64)))
    match = np.float64(ref.discrete_action_match_scorer(t, episodes))
    assert 0.0 < match < 1.0
    dyn = DynamicsTables(t)
    dyn_mean = np.float64(ref.dynamics_reward_prediction_mean_error_scorer(dyn, episodes))
    dyn_abs = np.float64(ref.dynamics_reward_prediction_abs_mean_error_scorer(dyn, episodes))
    assert dyn_abs > abs(dyn_mean) > 0.0
    return dict(lengths=t.lengths, qd=t.qd, a=t.a, a_mask=t.a_mask, rhat=t.rhat, next_rewards=t.next_rewards, thresholds=thresholds,
                soft_opc=soft_opc, discrete_action_match=match, dynamics_mean_error=dyn_mean, dynamics_abs_mean_error=dyn_abs)


def generate():
    ref = load_reference()
    assert ref.WINDOW_SIZE == 1024
    return {name: case(ref, lengths, seed) for name, lengths, seed in CASES}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=HERE)
    args = ap.parse_args()
    for name, arrays in generate().items():
        path = os.path.join(args.out, name)
        np.savez(path, **arrays)
        with np.load(path) as z:
            assert sorted(z.files) == sorted(arrays)
            for k, v in arrays.items():
                assert np.array_equal(z[k], np.asarray(v), equal_nan=True) and z[k].dtype == np.asarray(v).dtype, (name, k)
        print('%s: %d bytes' % (name, os.path.getsize(path)))


if __name__ == '__main__':
    main()
