"""COMBO (rl4rs_amd/offline_rl.py::COMBO = d3rlpy 0.91's SAC with a conservative critic term over minibatches of real rows followed
by model-generated ones; csrc/combo.hpp) against the float64 restatement in tests/combo_ref.py (PARITY UNPINNED: d3rlpy is absent):
the critic step alone - target, the six sums, the loss, both critics' full gradients after the join of the two passes - a whole
update, three updates, the one-call and the per-phase path, determinism, update_actor_interval, a rollout with the unpenalised reward,
files, and an end-to-end fit on the golden slate records followed by env.step(combo.predict(obs)).

Bars as in test_gpu_mopo.py: 4 x the float32-to-float64 difference of the restatement on the case's own inputs."""
import json
import os

import numpy as np
import pytest
import torch

import combo_ref as R
from test_gpu_dynamics import Check
from test_gpu_mopo import AMLP_KEYS, _cmp_net, _cuda, _pool, _small_dynamics, _weights

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F64, F32 = torch.float64, torch.float32
# (D, A, B, n_real, n): the default widths; nothing a multiple of a tile and a single real row; B > 256 and a single generated row;
# 3n = 69 > 64, so the lane loop of the logsumexp runs twice
CASES = [(266, 32, 64, 32, 10), (37, 5, 33, 1, 3), (40, 8, 300, 299, 2), (12, 4, 16, 5, 23)]
IDS = lambda c: 'x'.join(str(v) for v in c)
LRS = (1e-4, 3e-4, 1e-4)
GAMMA, TAU, W = 0.99, 0.005, 1.7            # a conservative weight off 1, so that a missing or doubled weight shows


class _NoDynamics(object):
    pass


def _learner(D, A, B, n, seed=3, **kw):
    from rl4rs_amd.offline_rl import COMBO
    combo = COMBO({'action_emb_size': A}, D, _NoDynamics(), batch_size=B, gamma=GAMMA, tau=TAU, seed=seed, predict_rows=64,
                  conservative_weight=W, n_action_samples=n, **kw)
    # a policy with some spread and critics / targets that disagree (fresh ones are copies of each other)
    for name, f in (('policy', 1.5), ('q2', 1.2), ('q1_targ', 0.8), ('q2_targ', 1.1)):
        net = getattr(combo, name)
        net.set_flat_params((net.flat_params() * f).contiguous())
    combo.log_temp.p.fill_(-0.3)
    return combo


def _ref(combo, dt, interval=1):
    ref = R.COMBO(_weights(combo.policy), _weights(combo.q1), _weights(combo.q2), dt, GAMMA, TAU, LRS, combo.n, W, interval, log_temp=-0.3)
    ref.P['q1t'], ref.P['q2t'] = _weights(combo.q1_targ), _weights(combo.q2_targ)
    return ref


def _batch(case, seed, steps=1):
    D, A, B, n_real, n = case
    F = B - n_real
    rs = np.random.RandomState(seed)
    f = lambda *s: rs.standard_normal(s).astype(np.float32)
    b = dict(obs=f(B, D), act=np.tanh(f(B, A)), rew=f(B), nxt=f(B, D), ter=(rs.uniform(size=B) < 0.2).astype(np.float32))
    noise = [dict(critic=(f(F * n, A), f(F * n, A), rs.uniform(-1, 1, size=(F, n, A)).astype(np.float32)), eps_actor=f(B, A), eps_temp=f(B, A))
             for _ in range(steps)]
    return b, noise


def _tn(noise):
    return dict((k, tuple(torch.from_numpy(x) for x in v) if isinstance(v, tuple) else torch.from_numpy(v)) for k, v in noise.items())


def _ref_update(r, b, n_real, noise):
    return r.update(b['obs'], b['act'], b['rew'], b['nxt'], b['ter'], n_real, noise)


def _check_critic_step(case, one_call):
    """an odd step of update_actor_interval = 2: the critics only"""
    D, A, B, n_real, n = case
    b, noise = _batch(case, 50 + D)
    ck = Check('combo critic %s %s' % (IDS(case), 'one call' if one_call else 'per phase'))
    combo = _learner(D, A, B, n, update_actor_interval=2)
    combo.one_call = one_call
    refs = [_ref(combo, dt, 2) for dt in (F64, F32)]
    combo.total_step = 1
    before = [net.flat_params().clone() for net in (combo.policy, combo.q1_targ, combo.q2_targ)]
    m = combo.update(*_cuda(b), n_real=n_real, noise=_tn(noise[0]))
    outs = []
    for r in refs:
        r.step = 1
        outs.append(_ref_update(r, b, n_real, noise[0]))
    assert sorted(m) == ['conservative_loss', 'critic_loss'] and 'actor_loss' not in outs[0]
    y, sums = combo.critic_step_outputs(B, n_real)
    sums = sums.cpu().numpy()
    ck('y', y, outs[0]['y'], outs[1]['y'])
    # the six sums as one pooled quantity per pair: a single scalar's float32 error can be zero by chance
    for name, sl in (('sums td', slice(0, 2)), ('sums lse', slice(2, 4)), ('sums data', slice(4, 6))):
        ck(name, sums[sl], outs[0]['sums'][sl], outs[1]['sums'][sl])
    # (one float32 number: at (37, 5, 33, 1, 3) the bar is 8.3e-7, below the half-ulp at 20.7; the device combines the six sums in
    # double and rounds once, 2.1e-7 there - DESIGN section 24)
    ck('critic_loss', m['critic_loss'].reshape(1), [outs[0]['critic_loss']], [outs[1]['critic_loss']])
    # the critics' FULL gradients after the join: a gradient overwritten by the second pass, not accumulated, shows here
    _cmp_net(ck, 'd q1', combo.q1.gradients(), outs[0]['g_q1'], outs[1]['g_q1'])
    _cmp_net(ck, 'd q2', combo.q2.gradients(), outs[0]['g_q2'], outs[1]['g_q2'])
    after = [net.flat_params() for net in (combo.policy, combo.q1_targ, combo.q2_targ)]
    assert all(torch.equal(p, q) for p, q in zip(before, after)) and combo.log_temp.t == 0
    combo.close()
    ck.done()


def _check_whole_update(case, one_call):
    """the actor's gradient through min(Q1, Q2) of the stepped critics, the temperature step on the stepped policy"""
    D, A, B, n_real, n = case
    b, noise = _batch(case, 50 + D)
    ck = Check('combo update %s %s' % (IDS(case), 'one call' if one_call else 'per phase'))
    combo = _learner(D, A, B, n)
    combo.one_call = one_call
    refs = [_ref(combo, dt) for dt in (F64, F32)]
    m = combo.update(*_cuda(b), n_real=n_real, noise=_tn(noise[0]))
    outs = [_ref_update(r, b, n_real, noise[0]) for r in refs]
    assert sorted(m) == ['actor_loss', 'conservative_loss', 'critic_loss', 'temp_loss']
    _cmp_net(ck, 'd policy', combo.policy.gradients(), outs[0]['g_policy'], outs[1]['g_policy'])
    ck('actor_loss', m['actor_loss'].reshape(1), [outs[0]['actor_loss']], [outs[1]['actor_loss']])
    ck('temp_loss', m['temp_loss'].reshape(1), [outs[0]['temp_loss']], [outs[1]['temp_loss']])
    ck('log_temp', combo.log_temp.p, [refs[0].log_temp], [refs[1].log_temp])
    assert combo.log_temp.t == 1 and combo.total_step == 1
    combo.close()
    ck.done()


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_critic_step_alone(case):
    _check_critic_step(case, True)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_a_whole_update(case):
    _check_whole_update(case, True)


@pytest.mark.parametrize('one_call', [True, False], ids=['one_call', 'per_phase'])
def test_both_paths_match_the_restatement(one_call):
    _check_critic_step(CASES[1], one_call)
    _check_whole_update(CASES[1], one_call)


@pytest.mark.parametrize('case', CASES[:2], ids=IDS)
def test_three_updates_track_the_restatement(case):
    D, A, B, n_real, n = case
    b, noise = _batch(case, 70 + D, steps=3)
    combo = _learner(D, A, B, n)
    refs = [_ref(combo, dt) for dt in (F64, F32)]
    for t in range(3):
        combo.update(*_cuda(b), n_real=n_real, noise=_tn(noise[t]))
        for r in refs:
            _ref_update(r, b, n_real, noise[t])
    ck = Check('combo 3 updates %s' % IDS(case))
    # ONE comparison for the parameters of the learner, for the reason test_gpu_mopo.py::test_three_updates_track_the_restatement
    # states: Adam turns the rounding noise of a gradient entry of the order of 1e-8 into a step of up to lr, on the device and in
    # the float32 restatement alike, and which array such an entry falls in is chance (each array's own figure is printed)
    nets = ((combo.policy, 'policy'), (combo.q1, 'q1'), (combo.q2, 'q2'), (combo.q1_targ, 'q1t'), (combo.q2_targ, 'q2t'))
    got = dict((key, _weights(dev)) for dev, key in nets)
    for _, key in nets:
        for k in AMLP_KEYS:
            print('%-10s %-8s device %.3e  fp32 restatement %.3e' % (key, k, R.maxdiff(got[key][k], refs[0].P[key][k]),
                                                                    R.maxdiff(refs[1].P[key][k], refs[0].P[key][k])))
    ck('parameters', np.concatenate([_pool(got[key], AMLP_KEYS) for _, key in nets]),
       np.concatenate([_pool(refs[0].P[key], AMLP_KEYS) for _, key in nets]), np.concatenate([_pool(refs[1].P[key], AMLP_KEYS) for _, key in nets]))
    ck('log_temp', combo.log_temp.p, [refs[0].log_temp], [refs[1].log_temp])
    assert abs(refs[0].log_temp + 0.3) > 1.5e-4               # three Adam steps of 1e-4 moved it
    assert abs(float(combo.log_temp.p) + 0.3) > 1.5e-4
    combo.close()
    ck.done()


def test_two_identical_updates_are_bit_identical():
    case = CASES[3]
    D, A, B, n_real, n = case
    b, noise = _batch(case, 110)
    got = []
    for _ in range(2):
        combo = _learner(D, A, B, n)
        assert combo.one_call
        m = combo.update(*_cuda(b), n_real=n_real, noise=_tn(noise[0]))
        got.append([m[k].clone() for k in sorted(m)] + [net.flat_gradient() for net in (combo.policy, combo.q1, combo.q2)] +
                   [net.flat_params() for net in combo.nets] + [combo.log_temp.state.clone()])
        combo.close()
    assert len(got[0]) == 4 + 3 + 5 + 1
    assert all(torch.equal(p, q) for p, q in zip(*got))
    assert all(bool(torch.isfinite(p).all()) for p in got[0])


def test_update_actor_interval_two_skips_exactly_the_odd_steps():
    case = CASES[1]
    D, A, B, n_real, n = case
    b, noise = _batch(case, 90, steps=4)
    combo = _learner(D, A, B, n, update_actor_interval=2)
    snap = lambda: [net.flat_params().clone() for net in (combo.policy, combo.q1_targ, combo.q2_targ)] + [combo.log_temp.state.clone()]
    crit = lambda: [net.flat_params().clone() for net in (combo.q1, combo.q2)]
    keys = []
    for t in range(4):
        before, cb = snap(), crit()
        keys.append(sorted(combo.update(*_cuda(b), n_real=n_real, noise=_tn(noise[t]))))
        after, ca = snap(), crit()
        assert all(not torch.equal(p, q) for p, q in zip(cb, ca)), t             # the critics step every time
        same = [torch.equal(p, q) for p, q in zip(before, after)]
        assert same == ([False] * 4 if t % 2 == 0 else [True] * 4), (t, same)      # actor, targets, temperature: even steps only
    assert keys == [['actor_loss', 'conservative_loss', 'critic_loss', 'temp_loss'], ['conservative_loss', 'critic_loss']] * 2
    assert combo.log_temp.t == 2 and combo.total_step == 4
    combo.close()


def test_refusals_of_update():
    D, A, B, n = 12, 4, 16, 2
    combo = _learner(D, A, B, n)
    b, _ = _batch((D, A, B, 8, n), 1)
    for n_real in (0, B):
        with pytest.raises(ValueError, match='n_real=%d' % n_real):
            combo.update(*_cuda(b), n_real=n_real)
    assert combo.total_step == 0
    combo.close()


def test_a_rollout_stores_the_unpenalised_reward_row_for_row():
    from rl4rs_amd import device as Dv
    from rl4rs_amd.offline_rl import COMBO
    D, A, N, H = 37, 5, 50, 2
    dyn, real_obs = _small_dynamics(D, A)
    combo = COMBO({'action_emb_size': A}, D, dyn, batch_size=32, n_action_samples=2, rollout_horizon=H, rollout_batch_size=N, predict_rows=32, seed=2)
    combo.policy.set_flat_params((combo.policy.flat_params() * 1.5).contiguous())
    rs = np.random.RandomState(8)
    given = dict(start=torch.from_numpy(rs.randint(0, 200, size=N)), eps=[torch.from_numpy(rs.standard_normal((N, A)).astype(np.float32)).cuda() for _ in range(H)],
                 indices=[torch.from_numpy(rs.randint(0, 3, size=N).astype(np.int32)).cuda() for _ in range(H)],
                 noise=[torch.from_numpy(rs.standard_normal((3, N, D + 1)).astype(np.float32)).cuda() for _ in range(H)])
    combo.generate_new_data(real_obs, given=given)
    assert len(combo.generated) == N * H
    obs, act, rew, nxt, ter = combo.generated.oldest_first()
    s = real_obs[given['start'].cuda()]
    for h in range(H):
        sl = slice(h * N, (h + 1) * N)
        a = torch.cat([Dv.squashed_sample(combo.policy.forward(s[lo:lo + 32].contiguous()), given['eps'][h][lo:lo + 32].contiguous())[0]
                       for lo in range(0, N, 32)])
        nx, r, var = dyn.predict(s, a, with_variance=True, indices=given['indices'][h], noise=given['noise'][h])
        _, rp, _ = dyn.predict(s, a, with_variance=True, indices=given['indices'][h], noise=given['noise'][h], lam=1.0)
        assert torch.equal(obs[sl], s) and torch.equal(act[sl], a) and torch.equal(nxt[sl], nx)
        assert torch.equal(rew[sl], r[:, 0]) and float(ter[sl].abs().max()) == 0.0         # the model's reward as it is
        assert float(var.min()) > 0 and not torch.equal(rew[sl], rp[:, 0])                   # (a penalty would have shown)
        s = nx
    combo.close()
    dyn.close()


def test_save_and_load_round_trip(tmp_path):
    case = CASES[1]
    D, A, B, n_real, n = case
    b, noise = _batch(case, 120, steps=2)
    one = _learner(D, A, B, n, seed=3)
    one.update(*_cuda(b), n_real=n_real, noise=_tn(noise[0]))
    path = str(tmp_path / 'combo.npz')
    one.save_model(path)
    two = _learner(D, A, B, n, seed=44)
    two.load_model(path)
    names = ('policy', 'q1', 'q2', 'q1_targ', 'q2_targ')
    assert all(torch.equal(getattr(one, k).flat_params(), getattr(two, k).flat_params()) for k in names)
    assert torch.equal(one.log_temp.state, two.log_temp.state) and one.log_temp.t == two.log_temp.t and two.total_step == 1
    x = torch.from_numpy(b['obs']).cuda()
    assert torch.equal(one.predict(x), two.predict(x))
    m1, m2 = [c.update(*_cuda(b), n_real=n_real, noise=_tn(noise[1])) for c in (one, two)]       # Adam state travelled too
    assert sorted(m1) == sorted(m2) and all(torch.equal(m1[k], m2[k]) for k in m1)
    assert all(torch.equal(getattr(one, k).flat_params(), getattr(two, k).flat_params()) for k in names)
    from rl4rs_amd.offline_rl import MOPO
    mopo = MOPO({'action_emb_size': A}, D, _NoDynamics(), batch_size=B, predict_rows=64)
    with pytest.raises(ValueError, match='holds a COMBO'):
        mopo.load_model(path)
    mopo.close()
    one.close()
    two.close()


def test_fit_on_the_golden_slate_records_then_step_the_env(tmp_path):
    """'dynamics' then 'COMBO' end to end as the script chains them, on the env of tests/golden/records_slate.txt with continuous
    actions; then the learned policy drives the env, directly and through the policy_model wrapper."""
    import rl4rs_amd
    from rl4rs.policy.policy_model import policy_model
    from rl4rs_amd.dynamics import ProbabilisticEnsembleDynamics
    from rl4rs_amd.env.slate import SlateRecEnv, SlateState
    from rl4rs_amd.offline import generate_offline_dataset
    from rl4rs_amd.offline_rl import COMBO
    man = json.load(open(os.path.join(HERE, 'golden', 'manifest.json')))['slate_conti']
    cfg = dict(man['config'])
    cfg.update({'iteminfo_file': os.path.join(HERE, 'golden', man['catalog']), 'sample_file': os.path.join(HERE, 'golden', man['records']),
                'cache_size': 256, 'model_seed': 3, 'return_tensors': True, 'support_d3rl_mask': True, 'support_conti_env': True})
    env = rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))
    data = generate_offline_dataset(env, epochs=12, shuffle=False)
    D, A = data['observations'].shape[1], cfg['action_emb_size']
    dyn = ProbabilisticEnsembleDynamics(cfg, D, batch_size=64, learning_rate=1e-3, predict_rows=256, seed=1)
    hist = dyn.fit_mdp(data, n_epochs=2)
    assert len(hist['loss']) >= 8 and np.isfinite(hist['loss']).all()
    combo = COMBO(cfg, D, dyn, batch_size=32, gamma=1.0, update_actor_interval=2, n_action_samples=4, rollout_interval=5, rollout_horizon=2,
                  rollout_batch_size=100, generated_maxlen=300, reward_scaler='standard', seed=1)
    out = combo.fit_mdp(data, n_epochs=1)
    n = len(out['critic_loss'])
    assert n >= 10 and len(out['conservative_loss']) == n and len(out['actor_loss']) == (n + 1) // 2 == len(out['temp_loss'])
    for k in ('critic_loss', 'conservative_loss', 'actor_loss', 'temp_loss'):
        assert np.isfinite(out[k]).all(), (k, out[k])
    assert len(combo.generated) == 300 and not isinstance(combo.reward_scaler, str)
    policy = policy_model(combo, config=cfg)
    obs = env.reset()
    total = 0.0
    for t in range(cfg['max_steps']):
        x = torch.as_tensor(obs, dtype=torch.float32)
        act = combo.predict(x)
        assert tuple(act.shape) == (cfg['batch_size'], A) and bool((act.abs() <= 1).all())
        assert torch.equal(torch.as_tensor(policy.predict_with_mask(obs)).to(act.device), act)       # the wrapper is the learner's predict
        obs, reward, done, info = env.step(act)
        reward = torch.as_tensor(reward)
        assert reward.is_floating_point() and bool(torch.isfinite(reward).all())
        total = total + reward.double().cpu()
    prev = env.samples.prev_actions
    prev = prev.cpu().numpy() if torch.is_tensor(prev) else np.asarray(prev)
    loc = np.asarray(env.samples.location_mask)
    for j in range(cfg['page_items']):
        assert (loc[j // 3][prev[:, j]] == 1).all()                       # the K-NN resolves every embedding to an item legal for its slot
    assert bool(torch.isfinite(total).all()) and bool(torch.isfinite(torch.as_tensor(obs, dtype=torch.float32)).all())
    q = policy.predict_q(x, act)
    assert bool(torch.isfinite(torch.as_tensor(q)).all())
    combo.close()
    dyn.close()
