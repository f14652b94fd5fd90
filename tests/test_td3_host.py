"""CPU: the float64 TD3 / DDPG restatement the GPU tests compare against (tests/td3_ref.py) is itself checked here - its hand-written
critic gradient against torch float64 autograd of the same loss, RLlib's actor squashing against tanh - together with the host
side of the learner: ``init_ddpg_params``, the two presets, the exploration-scale schedule, the refused n_step, the host
restatement of the counter RNG, and the ctypes mirror of rl4rs_td3_step."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import td3_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

@pytest.mark.parametrize('twin', [True, False])
@pytest.mark.parametrize('use_huber', [True, False])
@pytest.mark.parametrize('weighted', [True, False])
def test_hand_written_critic_gradient_equals_float64_autograd(twin, use_huber, weighted):
    N = 133
    rs = np.random.RandomState(1 + 4 * twin + 2 * use_huber + weighted)
    q1, q2, q1t, q2t = (rs.randn(N) * 2.0 for _ in range(4))
    rew, done, w = rs.randn(N), (rs.rand(N) < 0.2).astype(np.int32), rs.rand(N) + 0.1
    q1t[done != 0] = np.nan                                 # a terminal row's target Q is never used
    a = (q1, q2 if twin else None, q1t, q2t if twin else None, rew, done, w if weighted else None, 0.9, use_huber, 0.7)
    out = R.critic_loss_and_grads(*a)
    t1 = torch.tensor(q1, dtype=torch.float64, requires_grad=True)
    t2 = torch.tensor(q2, dtype=torch.float64, requires_grad=True) if twin else None
    c = R.critic_terms(t1, t2, *a[2:])
    c['loss'].backward()
    assert np.isfinite(out['dq1']).all() and np.isfinite(out['y']).all() and np.isfinite(out['stats']).all()
    if use_huber:
        assert (np.abs(out['td']) < 0.7).any() and (np.abs(out['td']) > 0.7).any()          # both sides of the knee
    assert np.allclose(out['dq1'], t1.grad.numpy(), rtol=1e-12, atol=1e-15)
    if twin:
        assert np.allclose(out['dq2'], t2.grad.numpy(), rtol=1e-12, atol=1e-15)
    else:
        assert out['dq2'] is None
    assert np.allclose(out['y'], c['y'].numpy(), rtol=0, atol=0) and abs(out['loss'] - float(c['loss'].detach())) < 1e-12
    assert np.array_equal(out['y'][done != 0], rew[done != 0])
    live = done == 0
    qn = np.minimum(q1t, q2t) if twin else q1t
    assert np.allclose(out['y'][live], rew[live] + 0.9 * qn[live], rtol=1e-15)


def test_rllib_actor_squashing_is_tanh_on_the_unit_box():
    x = torch.linspace(-12.0, 12.0, 4801, dtype=torch.float64)
    low, high = -1.0, 1.0
    squashed = torch.sigmoid(2.0 * x) * (high - low) + low
    assert (squashed - torch.tanh(x)).abs().max() < 4 * np.finfo(np.float64).eps


def test_init_ddpg_params_is_glorot_uniform_with_zero_biases():
    from rl4rs_amd.offline_rl import init_ddpg_params
    for od, e, k, h1, h2 in ((256, 0, 32, 400, 300), (256, 32, 1, 400, 300), (37, 5, 1, 48, 40)):
        p = init_ddpg_params(od, e, k, h1, h2, seed=3)
        assert sorted(p) == sorted(R.NAMES)
        for name, (fi, fo) in (('fc1', (od + e, h1)), ('fc2', (h1, h2)), ('head', (h2, k))):
            w, b = p[name + '_w'], p[name + '_b']
            assert w.shape == (fi, fo) and b.shape == (fo,) and w.dtype == np.float32 and b.dtype == np.float32
            lim = np.sqrt(6.0 / (fi + fo))
            assert np.abs(w).max() <= lim and (b == 0).all()
            if w.size >= 1000:                              # fills the interval: uniform, not a narrower law
                assert np.abs(w).max() > 0.98 * lim and abs(w.var() / (lim * lim / 3.0) - 1.0) < 0.1
    a, b = init_ddpg_params(256, 32, 1, seed=1), init_ddpg_params(256, 32, 1, seed=2)
    assert a['fc1_w'].shape == (288, 400) and a['fc2_w'].shape == (400, 300)       # the default hiddens
    assert not np.array_equal(a['fc1_w'], b['fc1_w'])
    assert np.array_equal(a['fc1_w'], init_ddpg_params(256, 32, 1, seed=1)['fc1_w'])


def test_presets_are_the_reference_configuration():
    from rl4rs_amd.train import TD3_PRESETS, TD3Trainer
    assert TD3_PRESETS['TD3'] == dict(twin_q=True, policy_delay=2, smooth_target_policy=True, target_noise=0.2, target_noise_clip=0.5,
                                      tau=5e-3, l2_reg=0.0, buffer_size=1000000, prioritized_replay=False, learning_starts=10000,
                                      random_timesteps=10000)
    d = TD3_PRESETS['DDPG']
    assert (d['twin_q'], d['policy_delay'], d['smooth_target_policy']) == (False, 1, False)
    assert (d['tau'], d['l2_reg'], d['buffer_size'], d['prioritized_replay'], d['learning_starts'], d['random_timesteps']) == \
        (2e-3, 1e-6, 50000, True, 1500, 1000)
    sig = inspect.signature(TD3Trainer.__init__).parameters
    common = dict(algo='TD3', gamma=1.0, actor_lr=1e-3, critic_lr=1e-3, use_huber=False, n_step=1, train_batch_size=None, ou_theta=0.15,
                  ou_sigma=0.2, ou_base_scale=0.1, initial_scale=1.0, final_scale=0.02, scale_timesteps=10000, updates_per_rollout=1,
                  prioritized_replay_alpha=0.6, prioritized_replay_beta=0.4, actor_hiddens=(400, 300), critic_hiddens=(400, 300))
    for k, v in common.items():
        assert sig[k].default == v, k
    for k in TD3_PRESETS['TD3']:                            # every preset value is a constructor argument, None = the preset
        assert sig[k].default is None, k


def test_exploration_scale_schedule():
    from rl4rs_amd.train import ou_scale
    assert ou_scale(0) == 1.0
    assert abs(ou_scale(5000) - 0.51) < 1e-15
    assert ou_scale(10000) == 0.02 and ou_scale(10 ** 7) == 0.02
    # RLlib's schedule starts where the random phase ends
    assert ou_scale(10000, random_timesteps=10000) == 1.0 and abs(ou_scale(15000, random_timesteps=10000) - 0.51) < 1e-15
    assert ou_scale(20000, random_timesteps=10000) == 0.02
    for t in (0, 1, 576, 4999, 9999, 10000, 12345, 19999, 20000, 50000):
        for rt in (0, 1000, 10000):
            assert abs(ou_scale(t, random_timesteps=rt) - R.ou_scale(t, random_timesteps=rt)) < 1e-15
    assert abs(ou_scale(250, 0, 2.0, 1.0, 1000) - 1.75) < 1e-15


def test_n_step_other_than_one_and_unknown_algo_are_refused():
    from rl4rs_amd.train import TD3Trainer
    with pytest.raises(ValueError):
        TD3Trainer(None, n_step=3)
    with pytest.raises(ValueError):
        TD3Trainer(None, algo='SAC')


def test_restatement_moves_every_target_and_delays_the_actor():
    """The restatement's own schedule on a tiny case: do_actor = False leaves the actor and its Adam step alone, moves its target."""
    from rl4rs_amd.offline_rl import init_ddpg_params
    rs = np.random.RandomState(0)
    od, e, h, M = 6, 3, (8, 7), 11
    prm = dict(actor=init_ddpg_params(od, 0, e, *h, seed=1), q1=init_ddpg_params(od, e, 1, *h, seed=2), q2=init_ddpg_params(od, e, 1, *h, seed=3))
    for n in ('actor', 'q1', 'q2'):
        prm[n + '_targ'] = dict((k, v + 0.05 * rs.randn(*v.shape)) for k, v in prm[n].items())
    ref = R.TD3Ref(prm, l2_reg=1e-3)
    b = (rs.randn(M, od), rs.rand(M, e) * 2 - 1, rs.randn(M), (rs.rand(M) < 0.3).astype(np.int32), rs.randn(M, od))
    a0, at0 = ref.flat('actor'), ref.flat('actor_targ')
    ref.update(*b, noise=rs.randn(M, e), do_actor=False)
    assert np.array_equal(ref.flat('actor'), a0) and ref.adam['actor']['t'] == 0 and ref.adam['q1']['t'] == 1
    assert np.allclose(ref.flat('actor_targ'), (1 - 5e-3) * at0 + 5e-3 * a0, rtol=1e-15)
    out = ref.update(*b, noise=rs.randn(M, e), do_actor=True)
    assert not np.array_equal(ref.flat('actor'), a0) and ref.adam['actor']['t'] == 1 and ref.adam['q2']['t'] == 2
    assert all((out['critic_grads'][0][k] != 0).any() for k in R.NAMES)
    # the L2 term touches weights only: with a zero data gradient a bias gradient stays zero
    g = out['actor_grads']
    assert np.isfinite(out['actor_loss']) and all(np.isfinite(v).all() for v in g.values())


def test_td3_step_mirror_has_the_header_fields_in_order():
    """tests/test_cabi.py holds header, exports and bindings together; what it cannot see is the ctypes mirror of rl4rs_td3_step."""
    from rl4rs_amd import _lib
    text = open(os.path.join(REPO, 'include', 'rl4rs_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    body = re.search(r'typedef struct rl4rs_td3_step \{(.*?)\} rl4rs_td3_step;', text, flags=re.S).group(1)
    fields = [f.strip(' *') for decl in body.split(';') for f in re.sub(r'^\s*(const\s+)?\w+\s*\**', '', decl.strip()).split(',') if f.strip()]
    assert fields == [n for n, _ in _lib.Td3Step._fields_], fields
    assert 'RL4RS_REPLAY_BUF_ACTION_F32 = 7' in text and _lib.REPLAY_BUFS['action_f32'] == 7


def test_counter_rng_restatement_is_uniform_and_normal():
    """The host restatement of the library's counter RNG (the GPU tests compare the kernels' noise with it): values strictly inside
    (0, 1) on the 2^-24 grid, moments of 65 536 draws within 5 standard errors."""
    n, e = R.explore_keys(64, 32, 64)
    u = np.concatenate([R.uniform01(5, s, n, e).reshape(-1) for s in range(32)])
    assert u.min() > 0 and u.max() < 1 and np.array_equal(u, u.astype(np.float32)) and len(np.unique(u)) > 0.99 * u.size
    assert abs(u.mean() - 0.5) < 5 / np.sqrt(12.0 * u.size) and abs(u.var() - 1 / 12.0) < 5 * np.sqrt(1 / 180.0 / u.size)
    z = np.concatenate([R.normal01(5, s, n, e).reshape(-1) for s in range(32)])
    assert abs(z.mean()) < 5 / np.sqrt(z.size) and abs(z.var() - 1.0) < 5 * np.sqrt(2.0 / z.size)
    assert np.array_equal(R.uniform01(5, 3, n, e), R.uniform01(5, 3, n, e)) and not np.array_equal(R.uniform01(5, 3, n, e), R.uniform01(5, 4, n, e))
    shared = R.normal01(5, 3, *R.explore_keys(64, 32, 1))
    assert (shared == shared[0:1]).all()
