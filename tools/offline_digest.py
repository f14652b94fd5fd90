#!/usr/bin/env python
"""sha256 per offline-learner configuration of what 6 ``fit`` steps, one ``predict`` and one ``predict_value`` leave behind: every
network's flat parameters, Adam moments and step counter, the learned scalars' state and step, ``total_step``, the filled rows of
the generated FIFO, every step's losses as float64 (keys sorted) and the two predictions.  For bit-identity A/Bs of
rl4rs_amd/offline_rl.py and the one-call updates of the library between two trees (profiles/r20_offline_digest.md):
    python tools/offline_digest.py                                        (this tree)
    python tools/offline_digest.py --tree tools/_ab/parent                (another tree with its own Python and library)
Prints one line `DIGEST <config> <sha256>` per configuration.  The discrete learners run at one shape; BCQ, CQL, MOPO and COMBO at
(D, A, B) = (37, 5, 33), (12, 4, 16) and the default widths (266, 32, 64), BCQ / CQL / COMBO once as one library call and once as
the per-phase calls; MOPO and COMBO with update_actor_interval = 2 and a rollout interval that fires twice."""
import argparse
import hashlib
import os
import sys

import numpy as np

STEPS = 6
SHAPES = ((37, 5, 33), (12, 4, 16), (266, 32, 64))
N_SAMPLES = {'bcq': {33: 7, 16: 7, 64: 100}, 'cql': {33: 3, 16: 3, 64: 10}}     # the default widths at the learners' default sample counts
REAL_RATIO = {33: 0.03, 16: 0.3125, 64: 0.5}                                    # COMBO: n_real = 1, 5, 32


def discrete_data(ow=40, P=3, A=65, n=80, seed=5):
    """the observation layout of tests/test_gpu_offline_rl_shapes.py: ow floats | P previous-action ids | cur_step, and its tables"""
    rs = np.random.RandomState(seed)
    special = [int(s) for s in np.sort(rs.choice(np.arange(1, A - 1), 3, replace=False))]
    loc = (rs.rand(3, A) < 0.8).astype(np.uint8)
    loc[:, special[0]] = 1
    x = np.zeros((n, ow + P + 1), np.float32)
    x[:, :ow] = rs.randn(n, ow)
    cur = rs.randint(0, 9, size=n)
    x[:, ow:ow + P] = rs.randint(1, A, size=(n, P)) * (np.arange(P)[None, :] < cur[:, None])
    x[:, -1] = cur
    data = dict(observations=x, actions=rs.randint(0, A, size=n), rewards=(rs.rand(n) * 5).astype(np.float32),
                terminals=(np.arange(n) % 10 == 9).astype(np.float32))
    return {'action_size': A, 'page_items': P, 'location_mask': loc, 'special_items': special}, data


def continuous_data(D, A, n=200, seed=7):
    rs = np.random.RandomState(seed)
    return dict(observations=rs.standard_normal((n, D)).astype(np.float32), actions=np.tanh(rs.standard_normal((n, A))).astype(np.float32),
                rewards=rs.standard_normal(n).astype(np.float32), terminals=(np.arange(n) % 10 == 9).astype(np.float32))


def small_dynamics(D, A, seed=6):
    """the dynamics model of tests/test_gpu_mopo.py"""
    from rl4rs_amd.dynamics import MinMaxScaler, ProbabilisticEnsembleDynamics
    from rl4rs_amd.offline_rl import StandardRewardScaler
    rs = np.random.RandomState(seed)
    obs = rs.standard_normal((200, D)).astype(np.float32)
    return ProbabilisticEnsembleDynamics({'action_emb_size': A}, D, hidden_units=(24, 12), n_ensembles=3, batch_size=32, predict_rows=40,
                                         scaler=MinMaxScaler(obs), reward_scaler=StandardRewardScaler(rs.standard_normal(200) * 2 + 1), seed=seed)


def configs():
    out = [('discrete_' + a, None, None) for a in ('bc', 'bcq', 'cql')]
    for shape in SHAPES:
        tag = '%dx%dx%d' % shape
        for algo, calls in (('bcq', (True, False)), ('cql', (True, False)), ('mopo', (None,)), ('combo', (True, False))):
            out += [('%s_%s%s' % (algo, tag, '' if c is None else '_onecall' if c else '_phases'), shape, c) for c in calls]
    return out


def build(name, shape):
    from rl4rs_amd import offline_rl as R
    algo = name.split('_')[0]
    if shape is None:
        cfg, data = discrete_data()
        cls = {'bc': R.DiscreteBC, 'bcq': R.DiscreteBCQ, 'cql': R.DiscreteCQL}[name.split('_')[1]]
        kw = {} if cls is R.DiscreteBC else {'target_update_interval': 4}
        return cls(cfg, data['observations'].shape[1], batch_size=16, seed=5, **kw), data, None
    D, A, B = shape
    cfg, data, dyn = {'action_emb_size': A}, continuous_data(D, A), None
    if algo == 'bcq':
        learner = R.BCQ(cfg, D, batch_size=B, n_action_samples=N_SAMPLES['bcq'][B], predict_rows=64, seed=3)
    elif algo == 'cql':
        learner = R.CQL(cfg, D, batch_size=B, n_action_samples=N_SAMPLES['cql'][B], predict_rows=64, seed=3,
                        reward_scaler=R.StandardRewardScaler(data['rewards']))
    else:
        dyn = small_dynamics(D, A)
        kw = dict(batch_size=B, update_actor_interval=2, rollout_interval=3, rollout_horizon=2, rollout_batch_size=20, generated_maxlen=70,
                  predict_rows=64, seed=3)
        if algo == 'mopo':
            learner = R.MOPO(cfg, D, dyn, real_ratio=0.25, lam=0.7, **kw)
        else:
            learner = R.COMBO(cfg, D, dyn, real_ratio=REAL_RATIO[B], n_action_samples=N_SAMPLES['cql'][B], **kw)
    return learner, data, dyn


def run(name, shape, one_call):
    import torch
    from rl4rs_amd import offline_rl as R
    h = hashlib.sha256()
    put = lambda t: h.update(np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, 'detach') else t).tobytes())
    learner, data, dyn = build(name, shape)
    if one_call is not None:
        learner.one_call = one_call
    discrete = shape is None
    tr = R.transitions_from_mdp(data['observations'], data['actions'], data['rewards'], data['terminals'], discrete_action=discrete)
    hist = learner.fit([t.cuda() for t in tr], STEPS, shuffle_seed=11)
    if discrete:
        put(np.array(hist, dtype=np.float64))
    else:
        for k in sorted(hist):
            put(np.array(hist[k], dtype=np.float64))
    for _, net in learner._io_nets():
        m, v, t = net.adam_state()
        for x in (net.flat_params(), m, v, np.array([t], dtype=np.int64)):
            put(x)
    for sp in (getattr(learner, 'log_temp', None), getattr(learner, 'log_alpha', None)):
        if sp is not None:
            put(sp.state)
            put(np.array([sp.t], dtype=np.int64))
    put(np.array([learner.total_step], dtype=np.int64))
    if getattr(learner, 'generated', None) is not None:
        for col in learner.generated.oldest_first():
            put(col)
    obs = torch.from_numpy(data['observations'][:16 if discrete else 50]).cuda()          # (a discrete net takes one minibatch of rows)
    act = learner.predict(obs)
    put(act)
    if hasattr(learner, 'predict_value'):
        put(learner.predict_value(obs, act))
    torch.cuda.synchronize()
    learner.close()
    if dyn is not None:
        dyn.close()
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--configs', default=None, help='comma-separated configuration names (default: all)')
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    torch.cuda.set_device(0)
    want = None if a.configs is None else set(a.configs.split(','))
    for name, shape, one_call in configs():
        if want is None or name in want:
            print('DIGEST %s %s' % (name, run(name, shape, one_call)), flush=True)


if __name__ == '__main__':
    main()
