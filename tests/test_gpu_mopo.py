"""MOPO (rl4rs_amd/offline_rl.py::MOPO = d3rlpy 0.91's SAC on minibatches of real and model-generated rows) against the float64
restatement in tests/dynamics_ref.py (PARITY UNPINNED: d3rlpy is absent): the soft target, the critic / actor / temperature
gradients, update_actor_interval, whole updates with supplied noise, a rollout reproduced row for row, files, and an end-to-end
fit on the golden slate records followed by env.step(mopo.predict(obs)).

Bars as in test_gpu_dynamics.py: 4 x the float32-to-float64 difference of the restatement on the case's own inputs."""
import json
import os

import numpy as np
import pytest
import torch

import dynamics_ref as R
from test_gpu_dynamics import Check

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F64, F32 = torch.float64, torch.float32
DIMS = [(266, 32, 64), (37, 5, 33), (40, 8, 300)]          # (D, A, B): default widths; nothing a multiple of a tile; B > 256
LRS = (3e-4, 3e-4, 3e-4)
GAMMA, TAU = 0.99, 0.005
AMLP_KEYS = ('fc1_w', 'fc1_b', 'fc2_w', 'fc2_b', 'head_w', 'head_b')


class _NoDynamics(object):
    pass


def _learner(D, A, B, seed=3, **kw):
    from rl4rs_amd.offline_rl import MOPO
    mopo = MOPO({'action_emb_size': A}, D, _NoDynamics(), batch_size=B, gamma=GAMMA, tau=TAU, seed=seed, predict_rows=64, **kw)
    # a policy with some spread and critics / targets that disagree (fresh ones are copies of each other)
    for name, f in (('policy', 1.5), ('q2', 1.2), ('q1_targ', 0.8), ('q2_targ', 1.1)):
        net = getattr(mopo, name)
        net.set_flat_params((net.flat_params() * f).contiguous())
    mopo.log_temp.p.fill_(-0.3)
    return mopo


def _weights(net):
    return dict((k, v.cpu().numpy()) for k, v in net.weights().items())


def _ref(mopo, dt, interval=1):
    sac = R.SAC(_weights(mopo.policy), _weights(mopo.q1), _weights(mopo.q2), dt, GAMMA, TAU, LRS, interval, log_temp=-0.3)
    sac.P['q1t'], sac.P['q2t'] = _weights(mopo.q1_targ), _weights(mopo.q2_targ)
    return sac


def _batch(D, A, B, seed, steps=1):
    rs = np.random.RandomState(seed)
    f = lambda *s: rs.standard_normal(s).astype(np.float32)
    b = dict(obs=f(B, D), act=np.tanh(f(B, A)), rew=f(B), nxt=f(B, D), ter=(rs.uniform(size=B) < 0.2).astype(np.float32))
    noise = [dict(eps_next=f(B, A), eps_actor=f(B, A), eps_temp=f(B, A)) for _ in range(steps)]
    return b, noise


def _cuda(b):
    return [torch.from_numpy(b[k]).cuda() for k in ('obs', 'act', 'rew', 'nxt', 'ter')]


def _tn(noise):
    return dict((k, torch.from_numpy(v)) for k, v in noise.items())


def _np(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def _pool(d, keys):
    return np.concatenate([_np(d[k]).astype(np.float64).reshape(-1) for k in keys])


# A one-element array has no "largest" float32-to-float64 difference to speak of: its single rounding error is zero or a fraction of
# an ulp by chance, and 4 x that is no measure of what another summation order does.  The head's bias gradient (one number: the
# batch sum of dq) is therefore compared together with the head's weight gradient, whose 256 entries are the same batch reduction.
GRAD_GROUPS = (('fc1_w',), ('fc1_b',), ('fc2_w',), ('fc2_b',), ('head_w', 'head_b'))


def _cmp_net(ck, what, dev_dict, r64, r32):
    for keys in GRAD_GROUPS:
        ck('%s %s' % (what, '+'.join(keys)), _pool(dev_dict, keys), _pool(r64, keys), _pool(r32, keys))


@pytest.mark.parametrize('dims', DIMS, ids=lambda d: 'x'.join(str(v) for v in d))
def test_target_and_gradients(dims):
    D, A, B = dims
    b, noise = _batch(D, A, B, 50 + D)
    ck = Check('mopo %dx%dx%d' % dims)
    # critic only (an odd step of update_actor_interval = 2): y and the critics' gradients
    mopo = _learner(D, A, B, update_actor_interval=2)
    refs = [_ref(mopo, dt, 2) for dt in (F64, F32)]
    mopo.total_step = 1
    y = mopo.soft_target(*[t for t in _cuda(b)[2:]], eps_next=torch.from_numpy(noise[0]['eps_next']))
    m = mopo.update(*_cuda(b), noise=_tn(noise[0]))
    outs = []
    for r in refs:
        r.step = 1
        outs.append(r.update(b['obs'], b['act'], b['rew'], b['nxt'], b['ter'], noise[0]))
    assert sorted(m) == ['critic_loss'] and 'actor_loss' not in outs[0]
    ck('y', y, outs[0]['y'], outs[1]['y'])
    ck('critic_loss', m['critic_loss'].reshape(1), [outs[0]['critic_loss']], [outs[1]['critic_loss']])
    _cmp_net(ck, 'd q1', mopo.q1.gradients(), outs[0]['g_q1'], outs[1]['g_q1'])
    _cmp_net(ck, 'd q2', mopo.q2.gradients(), outs[0]['g_q2'], outs[1]['g_q2'])
    mopo.close()
    # a whole update: the actor's gradient through min(Q1, Q2) of the stepped critics, the temperature loss = its gradient
    mopo = _learner(D, A, B)
    refs = [_ref(mopo, dt) for dt in (F64, F32)]
    m = mopo.update(*_cuda(b), noise=_tn(noise[0]))
    outs = [r.update(b['obs'], b['act'], b['rew'], b['nxt'], b['ter'], noise[0]) for r in refs]
    _cmp_net(ck, 'd policy', mopo.policy.gradients(), outs[0]['g_policy'], outs[1]['g_policy'])
    ck('actor_loss', m['actor_loss'].reshape(1), [outs[0]['actor_loss']], [outs[1]['actor_loss']])
    ck('temp_loss', m['temp_loss'].reshape(1), [outs[0]['temp_loss']], [outs[1]['temp_loss']])
    ck('log_temp', mopo.log_temp.p, [refs[0].log_temp], [refs[1].log_temp])
    mopo.close()
    ck.done()


@pytest.mark.parametrize('dims', DIMS[:2], ids=lambda d: 'x'.join(str(v) for v in d))
def test_three_updates_track_the_restatement(dims):
    D, A, B = dims
    b, noise = _batch(D, A, B, 70 + D, steps=3)
    mopo = _learner(D, A, B)
    refs = [_ref(mopo, dt) for dt in (F64, F32)]
    for t in range(3):
        mopo.update(*_cuda(b), noise=_tn(noise[t]))
        for r in refs:
            r.update(b['obs'], b['act'], b['rew'], b['nxt'], b['ter'], noise[t])
    ck = Check('mopo 3 updates %dx%dx%d' % dims)
    # ONE comparison for the parameters of the learner: Adam's step is lr * m / (sqrt(v) + 1e-8), so an entry whose gradient is of the
    # order of 1e-8 turns the rounding noise of that gradient into a step of up to lr = 3e-4 - on the device, and in the float32
    # restatement alike.  A handful of the ~ 10^5 entries are such, and which array they fall in is chance: the yardstick is the
    # largest float32-to-float64 difference over all the arrays (each array's own figure is printed).
    nets = ((mopo.policy, 'policy'), (mopo.q1, 'q1'), (mopo.q2, 'q2'), (mopo.q1_targ, 'q1t'), (mopo.q2_targ, 'q2t'))
    got = dict((key, _weights(dev)) for dev, key in nets)
    for _, key in nets:
        for k in AMLP_KEYS:
            print('%-10s %-8s device %.3e  fp32 restatement %.3e' % (key, k, R.maxdiff(got[key][k], refs[0].P[key][k]),
                                                                    R.maxdiff(refs[1].P[key][k], refs[0].P[key][k])))
    ck('parameters', np.concatenate([_pool(got[key], AMLP_KEYS) for _, key in nets]),
       np.concatenate([_pool(refs[0].P[key], AMLP_KEYS) for _, key in nets]), np.concatenate([_pool(refs[1].P[key], AMLP_KEYS) for _, key in nets]))
    ck('log_temp', mopo.log_temp.p, [refs[0].log_temp], [refs[1].log_temp])
    assert abs(refs[0].log_temp + 0.3) > 5e-4                # three Adam steps of 3e-4 moved it
    mopo.close()
    ck.done()


def test_update_actor_interval_two_skips_exactly_the_odd_steps():
    D, A, B = 37, 5, 33
    b, noise = _batch(D, A, B, 90, steps=4)
    mopo = _learner(D, A, B, update_actor_interval=2)
    snap = lambda: [n.flat_params().clone() for n in (mopo.policy, mopo.q1_targ, mopo.q2_targ)] + [mopo.log_temp.state.clone()]
    crit = lambda: [n.flat_params().clone() for n in (mopo.q1, mopo.q2)]
    keys = []
    for t in range(4):
        before, cb = snap(), crit()
        keys.append(sorted(mopo.update(*_cuda(b), noise=_tn(noise[t]))))
        after, ca = snap(), crit()
        assert all(not torch.equal(p, q) for p, q in zip(cb, ca)), t             # the critics step every time
        same = [torch.equal(p, q) for p, q in zip(before, after)]
        assert same == ([False] * 4 if t % 2 == 0 else [True] * 4), (t, same)      # actor, targets, temperature: even steps only
    assert keys == [['actor_loss', 'critic_loss', 'temp_loss'], ['critic_loss']] * 2
    assert mopo.log_temp.t == 2 and mopo.total_step == 4
    mopo.close()


def _small_dynamics(D, A, seed=6):
    from rl4rs_amd.dynamics import MinMaxScaler, ProbabilisticEnsembleDynamics
    from rl4rs_amd.offline_rl import StandardRewardScaler
    rs = np.random.RandomState(seed)
    obs = rs.standard_normal((200, D)).astype(np.float32)
    dyn = ProbabilisticEnsembleDynamics({'action_emb_size': A}, D, hidden_units=(24, 12), n_ensembles=3, batch_size=32, predict_rows=40,
                                        scaler=MinMaxScaler(obs), reward_scaler=StandardRewardScaler(rs.standard_normal(200) * 2 + 1),
                                        seed=seed)
    return dyn, torch.from_numpy(obs).cuda()


def test_a_rollout_of_horizon_two_is_predict_and_the_policy_sample_row_for_row():
    from rl4rs_amd import device as Dv
    from rl4rs_amd.offline_rl import MOPO
    D, A, N, H, lam = 37, 5, 50, 2, 0.7
    dyn, real_obs = _small_dynamics(D, A)
    mopo = MOPO({'action_emb_size': A}, D, dyn, batch_size=32, rollout_horizon=H, rollout_batch_size=N, lam=lam, predict_rows=32, seed=2)
    mopo.policy.set_flat_params((mopo.policy.flat_params() * 1.5).contiguous())
    rs = np.random.RandomState(8)
    given = dict(start=torch.from_numpy(rs.randint(0, 200, size=N)), eps=[torch.from_numpy(rs.standard_normal((N, A)).astype(np.float32)).cuda() for _ in range(H)],
                 indices=[torch.from_numpy(rs.randint(0, 3, size=N).astype(np.int32)).cuda() for _ in range(H)],
                 noise=[torch.from_numpy(rs.standard_normal((3, N, D + 1)).astype(np.float32)).cuda() for _ in range(H)])
    mopo.generate_new_data(real_obs, given=given)
    assert len(mopo.generated) == N * H and mopo.generated.cols[0].shape[0] == N * H         # sized to what was generated
    obs, act, rew, nxt, ter = mopo.generated.oldest_first()
    s = real_obs[given['start'].cuda()]
    for h in range(H):
        sl = slice(h * N, (h + 1) * N)
        a = torch.cat([Dv.squashed_sample(mopo.policy.forward(s[lo:lo + 32].contiguous()), given['eps'][h][lo:lo + 32].contiguous())[0]
                       for lo in range(0, N, 32)])
        nx, r, var = dyn.predict(s, a, with_variance=True, indices=given['indices'][h], noise=given['noise'][h])
        _, rp, _ = dyn.predict(s, a, with_variance=True, indices=given['indices'][h], noise=given['noise'][h], lam=lam)
        assert torch.equal(obs[sl], s) and torch.equal(act[sl], a) and torch.equal(nxt[sl], nx)
        assert torch.equal(rew[sl], rp[:, 0]) and float(ter[sl].abs().max()) == 0.0
        # r - lam * variance: one multiply and one subtraction in float32 on either side
        assert float((rew[sl] - (r - lam * var)[:, 0]).abs().max()) <= 2.0 ** -22 * float((r.abs() + lam * var).max())
        assert float(var.min()) > 0
        s = nx
    # a seeded generator draws the starts and the noise when nothing is given: two learners with one seed agree
    twins = []
    for _ in range(2):
        m2 = MOPO({'action_emb_size': A}, D, dyn, batch_size=32, rollout_horizon=H, rollout_batch_size=N, lam=lam, predict_rows=32, seed=2)
        m2.generate_new_data(real_obs)
        twins.append(m2.generated.oldest_first())
        m2.close()
    assert all(torch.equal(p, q) for p, q in zip(*twins))
    mopo.close()
    dyn.close()


def test_save_and_load_round_trip(tmp_path):
    D, A, B = 37, 5, 33
    b, noise = _batch(D, A, B, 120, steps=2)
    one = _learner(D, A, B, seed=3)
    one.update(*_cuda(b), noise=_tn(noise[0]))
    path = str(tmp_path / 'mopo.npz')
    one.save_model(path)
    two = _learner(D, A, B, seed=44)
    two.load_model(path)
    names = ('policy', 'q1', 'q2', 'q1_targ', 'q2_targ')
    assert all(torch.equal(getattr(one, n).flat_params(), getattr(two, n).flat_params()) for n in names)
    assert torch.equal(one.log_temp.state, two.log_temp.state) and one.log_temp.t == two.log_temp.t and two.total_step == 1
    x = torch.from_numpy(b['obs']).cuda()
    assert torch.equal(one.predict(x), two.predict(x))
    m1, m2 = one.update(*_cuda(b), noise=_tn(noise[1])), two.update(*_cuda(b), noise=_tn(noise[1]))       # Adam state travelled too
    assert all(torch.equal(m1[k], m2[k]) for k in m1)
    assert all(torch.equal(getattr(one, n).flat_params(), getattr(two, n).flat_params()) for n in names)
    one.close()
    two.close()


def test_fit_on_the_golden_slate_records_then_step_the_env(tmp_path):
    """'dynamics' then 'MOPO' end to end as the script chains them (batchrl_train.py: the dynamics model is trained first and handed
    to MOPO), on the env of tests/golden/records_slate.txt with continuous actions; then the learned policy drives the env."""
    import rl4rs_amd
    from rl4rs.policy.policy_model import policy_model
    from rl4rs_amd.dynamics import ProbabilisticEnsembleDynamics
    from rl4rs_amd.env.slate import SlateRecEnv, SlateState
    from rl4rs_amd.offline import generate_offline_dataset
    from rl4rs_amd.offline_rl import MOPO
    man = json.load(open(os.path.join(HERE, 'golden', 'manifest.json')))['slate_conti']
    cfg = dict(man['config'])
    cfg.update({'iteminfo_file': os.path.join(HERE, 'golden', man['catalog']), 'sample_file': os.path.join(HERE, 'golden', man['records']),
                'cache_size': 256, 'model_seed': 3, 'return_tensors': True, 'support_d3rl_mask': True, 'support_conti_env': True})
    env = rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))
    data = generate_offline_dataset(env, epochs=12, shuffle=False)
    D, A = data['observations'].shape[1], cfg['action_emb_size']
    assert D == 256 + cfg['page_items'] + 1 and data['actions'].shape[1] == A
    dyn = ProbabilisticEnsembleDynamics(cfg, D, batch_size=64, learning_rate=1e-3, predict_rows=256, seed=1)
    hist = dyn.fit_mdp(data, n_epochs=2)
    assert len(hist['loss']) >= 8 and np.isfinite(hist['loss']).all()
    mopo = MOPO(cfg, D, dyn, batch_size=32, gamma=1.0, update_actor_interval=2, rollout_interval=5, rollout_horizon=2,
                rollout_batch_size=100, generated_maxlen=300, reward_scaler='standard', seed=1)
    out = mopo.fit_mdp(data, n_epochs=1)
    n = len(out['critic_loss'])
    assert n >= 10 and np.isfinite(out['critic_loss']).all() and len(out['actor_loss']) == (n + 1) // 2
    assert np.isfinite(out['actor_loss']).all() and np.isfinite(out['temp_loss']).all()
    assert len(mopo.generated) == 300                        # rollouts of 200 rows every 5 updates through a FIFO of 300
    assert not isinstance(mopo.reward_scaler, str)
    policy = policy_model(mopo, config=cfg)
    obs = env.reset()
    for t in range(cfg['max_steps']):
        act = policy.predict_with_mask(obs)
        assert tuple(act.shape) == (cfg['batch_size'], A) and bool((act.abs() <= 1).all())
        obs, reward, done, info = env.step(act)
    assert bool(torch.isfinite(torch.as_tensor(obs, dtype=torch.float32)).all())
    mopo.close()
    dyn.close()
