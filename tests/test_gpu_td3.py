"""GPU: the on-device TD3 / DDPG (continuous replay ring, OU exploration, critic-loss kernels, rl4rs_td3_update, TD3Learner /
TD3Trainer) against the float64 restatement in tests/td3_ref.py.

Bars are those of tests/test_gpu_offline_conti.py ("forward 2e-4 abs on O(1) outputs (fp32 MFMA GEMMs over K <= 298), gradients
2e-3 relative to the largest entry of each array, parameters after k Adam steps 2e-4 abs"), its losses at 2e-3 * max(1, |loss|),
and TD errors at tests/test_gpu_dqn.py's TD_ABS (2e-5 + 1e-6) scaled by max(1, |y|).  Element-wise kernels fed their own noise
(exploration, smoothing) are held to 1e-6: a handful of fp32 roundings on values of at most a few units.  The means of the Q-valued
columns (mean q, mean y) are outputs of the forward and take its 2e-4 abs; TD errors and their mean |td| take the TD bar wherever
they appear, behind the loss kernel alone and behind the real forwards."""
import os

import numpy as np
import pytest

import dqn_ref as DR
import td3_ref as R

pytestmark = pytest.mark.gpu

TD_ABS = 2e-5 + 1e-6
FWD, GRAD, PARAM, LOSS = 2e-4, 2e-3, 2e-4, 2e-3


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---- 1. the ring of continuous actions ---------------------------------------------------------------------------------------------
def _rollout(rs, T, B, od, E):
    host = dict(obs=rs.randn(T * B, od).astype(np.float32), act=(rs.rand(T * B, E) * 2 - 1).astype(np.float32), rew=rs.randn(T * B) * 3.0)
    return host, dict((k, _cuda(v)) for k, v in host.items())


@pytest.mark.parametrize('od,E,T,B', [(256, 32, 3, 8), (10, 5, 2, 7)])
def test_conti_ring_evicts_whole_rollouts_and_gathers_exactly(od, E, T, B):
    from rl4rs_amd.device import DeviceContiReplay
    rs = np.random.RandomState(od + B)
    per = T * B
    rp = DeviceContiReplay(od, E, T, B, buffer_size=3 * per + 1, alpha=0.6)
    assert rp.counts() == (0, 3 * per, 0)
    hosts = []
    for k in range(4):
        h, d = _rollout(rs, T, B, od, E)
        rp.push(d['obs'], d['act'], d['rew'])
        hosts.append(h)
        assert rp.counts() == (min(k + 1, 3) * per, 3 * per, k + 1)
    col = dict((k, rp.column(k).cpu().numpy()) for k in ('obs', 'action', 'reward', 'done', 'priority'))
    assert col['action'].shape == (3 * per, E) and col['action'].dtype == np.float32
    for slot, h in ((0, hosts[3]), (1, hosts[1]), (2, hosts[2])):          # rollout 0 is gone: push 3 took its slot
        sl = slice(slot * per, (slot + 1) * per)
        assert np.array_equal(col['obs'][sl], h['obs']) and np.array_equal(col['action'][sl], h['act'])
        assert np.array_equal(col['reward'][sl], h['rew'].astype(np.float32))
    assert not (col['obs'] == hosts[0]['obs'][0]).all(axis=1).any()
    assert np.array_equal(col['done'], DR.row_fields(np.arange(3 * per), T, B)[3].astype(np.int32))
    assert (col['priority'] == 1.0).all() and rp.max_priority() == 1.0
    # uniform draws: idx = floor(u * n); rows, actions and successors are the ring's, bit for bit
    n, M = rp.rows, 997
    b = rp.sample(M, prioritized=False, seed=9, step=4, want_u=True)
    s = dict((k, v.cpu().numpy()) for k, v in b.items())
    idx = s['idx']
    assert np.array_equal(idx, DR.uniform_select(s['u'].astype(np.float64), n)) and (np.bincount(idx, minlength=n) > 0).all()
    _, _, _, done, nxt = DR.row_fields(idx, T, B)
    assert np.array_equal(s['obs'], col['obs'][idx]) and np.array_equal(s['action'], col['action'][idx])
    assert np.array_equal(s['reward'], col['reward'][idx]) and np.array_equal(s['done'], done.astype(np.int32))
    assert done.any() and (~done).any() and (s['weight'] == 1.0).all()
    assert np.array_equal(s['next_obs'][~done], col['obs'][nxt[~done]])
    assert np.array_equal(s['next_obs'][done], s['obs'][done])             # a terminal row's successor is the row itself


@pytest.mark.parametrize('od,E,T,B,pushes', [(256, 32, 3, 8, 4), (10, 5, 2, 7, 4), (16, 4, 9, 64, 5)])
def test_conti_ring_prioritized_draws_follow_the_float64_prefix_sums(od, E, T, B, pushes):
    """The two shapes of the ring test and one of 2880 rows (three 1024-row scan tiles, the last partial)."""
    import torch
    from rl4rs_amd.device import DeviceContiReplay
    rs = np.random.RandomState(2 + od)
    rp = DeviceContiReplay(od, E, T, B, buffer_size=(3 if pushes == 4 else 6) * T * B, alpha=0.6)
    for _ in range(pushes):
        d = _rollout(rs, T, B, od, E)[1]
        rp.push(d['obs'], d['act'], d['rew'])
    n = rp.rows
    assert n == min(pushes, 3 if pushes == 4 else 6) * T * B
    prio = rs.rand(n) * 5.0 + 0.01
    rp.set_priorities(torch.from_numpy(prio))
    M = 4096
    b = rp.sample(M, prioritized=True, beta=0.4, seed=3, step=0, want_u=True)
    u, idx, w = b['u'].cpu().numpy().astype(np.float64), b['idx'].cpu().numpy(), b['weight'].cpu().numpy()
    ref, dist, total = DR.prioritized_select(prio, u)
    near = dist < 1e-9 * total
    assert near.sum() <= 0.001 * M
    assert np.array_equal(idx[~near], ref[~near])
    assert np.allclose(w, DR.is_weights(prio, idx, 0.4), rtol=1e-6, atol=0)
    assert np.array_equal(b['action'].cpu().numpy(), rp.column('action').cpu().numpy()[idx])
    b2 = rp.sample(M, prioritized=True, beta=0.4, seed=3, step=0, want_u=True)
    assert all(torch.equal(b[k], b2[k]) for k in b)
    # the shared priority update works on this ring as on the discrete one
    td = _cuda((rs.randn(M) * 2).astype(np.float32))
    rp.update_priorities(b['idx'], td)
    new, mx = DR.update_priorities(prio, 1.0, idx, td.cpu().numpy(), alpha=0.6)
    assert np.allclose(rp.column('priority').cpu().numpy()[:n], new, rtol=1e-12, atol=0) and rp.max_priority() == mx


def test_discrete_and_continuous_calls_refuse_the_other_ring():
    import ctypes as C
    import torch
    from rl4rs_amd import _lib
    from rl4rs_amd.device import DeviceContiReplay, DeviceReplay, _ptr, _stream
    T, B, od, E, A = 2, 4, 8, 3, 40
    lib = _lib.load()
    conti, disc = DeviceContiReplay(od, E, T, B, buffer_size=T * B), DeviceReplay(od, A, T, B, buffer_size=T * B)
    f = torch.zeros(T * B * max(od, E), dtype=torch.float32, device='cuda')
    i = torch.zeros(T * B * 2, dtype=torch.int32, device='cuda')
    r = torch.zeros(T * B, dtype=torch.float64, device='cuda')
    conti.push(f[:T * B * od].view(T * B, od), f[:T * B * E].view(T * B, E), r)
    disc.push(f[:T * B * od].view(T * B, od), i.view(T * B, 2), i[:T * B], r)
    p, n = C.c_void_p(), C.c_int64()
    calls = [
        ('continuous', lambda: lib.rl4rs_replay_push(conti.h, _ptr(f), _ptr(i), _ptr(i), _ptr(r), _stream())),
        ('continuous', lambda: lib.rl4rs_replay_sample(conti.h, 4, 0, 0.4, 0, 0, _ptr(f), _ptr(f), _ptr(i), _ptr(i), _ptr(f), _ptr(i), _ptr(i),
                                                       None, None, _stream())),
        ('continuous', lambda: lib.rl4rs_replay_buffer(conti.h, _lib.REPLAY_BUFS['mask'], C.byref(p), C.byref(n))),
        ('continuous', lambda: lib.rl4rs_replay_buffer(conti.h, _lib.REPLAY_BUFS['action'], C.byref(p), C.byref(n))),
        ('discrete', lambda: lib.rl4rs_replay_push_conti(disc.h, _ptr(f), _ptr(f), _ptr(r), _stream())),
        ('discrete', lambda: lib.rl4rs_replay_sample_conti(disc.h, 4, 0, 0.4, 0, 0, _ptr(f), _ptr(f), _ptr(f), _ptr(f), _ptr(i), _ptr(i), None,
                                                           None, _stream())),
        ('discrete', lambda: lib.rl4rs_replay_buffer(disc.h, _lib.REPLAY_BUFS['action_f32'], C.byref(p), C.byref(n))),
    ]
    for word, call in calls:
        with pytest.raises(_lib.Rl4rsHipError) as e:
            _lib.check(call())
        assert word in str(e.value), str(e.value)
    assert conti.counts()[2] == 1 and disc.counts()[2] == 1               # the refused pushes left the rings alone
    assert disc.sample(4, prioritized=False)['obs'].shape == (4, od) and conti.sample(4, prioritized=False)['action'].shape == (4, E)


# ---- 2. exploration ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,E,rows', [(67, 5, 67), (64, 32, 64), (64, 32, 1)])
def test_explore_ou_follows_the_restatement_fed_its_own_noise(N, E, rows):
    import torch
    from rl4rs_amd.device import DeviceContiReplay, explore_ou
    rs = np.random.RandomState(N + E + rows)
    theta, sigma, scale, seed = 0.15, 0.2, 0.1, 77
    state = torch.zeros((rows, E), dtype=torch.float32, device='cuda')
    ref_state = np.zeros((rows, E))
    at_clip = 0
    first = None
    for step in range(4):
        det = np.where(rs.rand(N, E) < 0.5, np.sign(rs.randn(N, E)) * 0.99, rs.rand(N, E) - 0.5).astype(np.float32)
        before = state.clone()
        act, eps = explore_ou(_cuda(det), state, theta, sigma, scale, seed=seed, step=step, want_eps=True)
        eps_np, act_np = eps.cpu().numpy().astype(np.float64), act.cpu().numpy()
        if rows == 1:
            assert (eps_np == eps_np[0:1]).all()                          # every row gets the same noise
        # the noise is Box-Muller on the counter RNG keyed (seed, step, state row, column): a few fp32 roundings of logf / cosf on
        # |eps| < 6 (6 * 2^-24 * a few), held to 1e-5
        assert np.abs(eps_np - R.normal01(seed, step, *R.explore_keys(N, E, rows))).max() < 1e-5
        ref_state, ref_act = R.ou_step(ref_state, eps_np[:rows], det, theta, sigma, scale)
        assert np.abs(state.cpu().numpy() - ref_state).max() < 1e-6 and np.abs(act_np - ref_act).max() < 1e-6
        assert (np.abs(act_np) <= 1.0).all()
        at_clip += int((np.abs(act_np) == 1.0).sum())
        # same (seed, step): the same bits; another step: other bits
        st2 = before.clone()
        act2, eps2 = explore_ou(_cuda(det), st2, theta, sigma, scale, seed=seed, step=step, want_eps=True)
        assert torch.equal(act, act2) and torch.equal(eps, eps2) and torch.equal(st2, state)
        if first is not None:
            assert not torch.equal(eps, first)
        first = eps
    assert at_clip > 0
    # random phase: a = 2u - 1 with u of the counter RNG keyed (seed, step, row, column); the state does not move
    keep = state.clone()
    act = explore_ou(_cuda(det), state, theta, sigma, scale, seed=seed, step=9, random_phase=True)[0]
    a = act.cpu().numpy()
    assert torch.equal(state, keep) and (np.abs(a) < 1.0).all()
    n_, e_ = R.explore_keys(N, E, N)                                       # (the random phase is keyed by the action's own row)
    assert np.array_equal(a, (2.0 * R.uniform01(seed, 9, n_, e_) - 1.0).astype(np.float32))           # every column, bit for bit
    rp = DeviceContiReplay(4, 2, 1, 1, buffer_size=1)                      # (the ring's u_out is the same RNG keyed (seed, step, draw, 0))
    rp.push(torch.zeros((1, 4), device='cuda'), torch.zeros((1, 2), device='cuda'), torch.zeros(1, dtype=torch.float64, device='cuda'))
    u = rp.sample(N, prioritized=False, seed=seed, step=9, want_u=True)['u'].cpu().numpy()
    assert np.array_equal(u, R.uniform01(seed, 9, np.arange(N), np.zeros(N, dtype=np.int64)).astype(np.float32))
    n = a.size
    assert abs(a.mean()) < 5 / np.sqrt(3.0 * n) and len(np.unique(a)) > 0.99 * n
    assert not torch.equal(act, explore_ou(_cuda(det), state, theta, sigma, scale, seed=seed, step=10, random_phase=True)[0])


def test_explore_ou_noise_is_standard_normal():
    import torch
    from rl4rs_amd.device import explore_ou
    N, E = 64, 32
    state = torch.zeros((N, E), dtype=torch.float32, device='cuda')
    det = torch.zeros((N, E), dtype=torch.float32, device='cuda')
    eps = torch.cat([explore_ou(det, state, seed=5, step=s, want_eps=True)[1].reshape(-1) for s in range(32)]).cpu().numpy().astype(np.float64)
    n = eps.size
    assert n == 65536
    print('eps mean %.4g (bar %.4g)  var - 1 %.4g (bar %.4g)' % (eps.mean(), 5 / np.sqrt(n), eps.var() - 1, 5 * np.sqrt(2.0 / n)))
    assert abs(eps.mean()) < 5 / np.sqrt(n) and abs(eps.var() - 1.0) < 5 * np.sqrt(2.0 / n)
    assert len(np.unique(eps)) > 0.99 * n


# ---- 3. the element-wise and loss kernels --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [576, 67])
@pytest.mark.parametrize('twin', [True, False])
@pytest.mark.parametrize('use_huber', [True, False])
@pytest.mark.parametrize('weighted', [True, False])
def test_critic_loss_kernel_matches_the_restatement(N, twin, use_huber, weighted):
    import torch
    from rl4rs_amd.device import td3_critic_loss
    rs = np.random.RandomState(N + 4 * twin + 2 * use_huber + weighted)
    q1, q2, q1t, q2t = ((rs.randn(N) * 2.0).astype(np.float32) for _ in range(4))
    rew, done = rs.randn(N).astype(np.float32), (rs.rand(N) < 0.2).astype(np.int32)
    done[-1] = 1
    w = (rs.rand(N) + 0.1).astype(np.float32)
    d = dict(q1=_cuda(q1), q2=_cuda(q2) if twin else None, q1t=_cuda(q1t), q2t=_cuda(q2t) if twin else None, rew=_cuda(rew),
             done=_cuda(done), w=_cuda(w) if weighted else None)
    run = lambda a, b: td3_critic_loss(d['q1'], d['q2'], a, b, d['rew'], d['done'], weights=d['w'], gamma=0.9, use_huber=use_huber,
                                       huber_threshold=0.7)
    out = run(d['q1t'], d['q2t'])
    ref = R.critic_loss_and_grads(q1, q2 if twin else None, q1t, q2t if twin else None, rew, done, w if weighted else None, 0.9, use_huber, 0.7)
    ybar = TD_ABS * max(1.0, np.abs(ref['y']).max())
    err_y, err_td = np.abs(out['y'].cpu().numpy() - ref['y']).max(), np.abs(out['td'].cpu().numpy() - ref['td']).max()
    print('y err %.3g td err %.3g (bar %.3g)' % (err_y, err_td, ybar))
    assert err_y < ybar and err_td < ybar
    for k in ('dq1', 'dq2'):
        if ref[k] is None:
            assert out[k] is None
            continue
        assert np.abs(out[k].cpu().numpy() - ref[k]).max() < GRAD * np.abs(ref[k]).max(), k
    st = out['stats'].cpu().numpy().astype(np.float64) / N
    rs_ = ref['stats'] / N
    assert abs(st[0] - rs_[0]) < LOSS * max(1.0, abs(rs_[0]))
    assert abs(st[1] - rs_[1]) < FWD and abs(st[2] - rs_[2]) < FWD and abs(st[3] - rs_[3]) < ybar      # mean q, mean y; mean |td| at the TD bar
    if use_huber:
        assert (np.abs(ref['td']) < 0.7).any() and (np.abs(ref['td']) > 0.7).any()
    # bit-identical from run to run
    out2 = run(d['q1t'], d['q2t'])
    assert all(torch.equal(out[k], out2[k]) for k in out if out[k] is not None)
    # a terminal row's target Q values reach nothing: NaN there changes no bit and everything stays finite
    nan1 = d['q1t'].clone()
    nan1[d['done'] != 0] = float('nan')
    nan2 = None
    if twin:
        nan2 = d['q2t'].clone()
        nan2[d['done'] != 0] = float('nan')
    out3 = run(nan1, nan2)
    for k in out:
        if out[k] is not None:
            assert torch.equal(out[k], out3[k]) and bool(torch.isfinite(out3[k]).all()), k


@pytest.mark.parametrize('N,E', [(576, 32), (67, 5)])
def test_target_smoothing_tanh_head_gradient_and_l2(N, E):
    import torch
    from rl4rs_amd.device import DeviceAMLP, amlp_add_l2, tanh_head_grad, td3_smooth_action
    from rl4rs_amd.offline_rl import init_ddpg_params
    rs = np.random.RandomState(N)
    a = np.clip(rs.randn(N, E) * 0.8, -1, 1).astype(np.float32)
    eps = rs.randn(N, E).astype(np.float32)
    want, noise_bound, box_bound = R.smooth_action(a, eps, 0.4, 0.5)
    assert noise_bound.any() and box_bound.any() and (~noise_bound).any() and (~box_bound).any()      # both clips bind somewhere
    got = td3_smooth_action(_cuda(a), _cuda(eps), 0.4, 0.5)
    assert np.abs(got.cpu().numpy() - want).max() < 1e-6
    inplace = _cuda(a)
    td3_smooth_action(inplace, _cuda(eps), 0.4, 0.5, out=inplace)
    assert torch.equal(inplace, got)
    t = np.tanh(rs.randn(N, E)).astype(np.float32)
    dout = rs.randn(N, E).astype(np.float32)
    d = tanh_head_grad(_cuda(t), _cuda(dout)).cpu().numpy()
    assert np.abs(d - dout.astype(np.float64) * (1.0 - t.astype(np.float64) ** 2)).max() < 1e-6
    # L2: grad += l2 * W on the three weight matrices, the biases keep their bits
    prm = init_ddpg_params(N % 50 + 7, E, 1, 24, 20, seed=1)
    for k in ('fc1_b', 'fc2_b', 'head_b'):
        prm[k] = rs.randn(*prm[k].shape).astype(np.float32)
    net = DeviceAMLP(N % 50 + 7, E, 1, prm, hidden1=24, hidden2=20, max_rows=8)
    g0 = rs.randn(net.n_params).astype(np.float32)
    net.set_flat_gradient(_cuda(g0))
    amlp_add_l2(net, 0.0)
    assert np.array_equal(net.flat_gradient().cpu().numpy(), g0)
    amlp_add_l2(net, 0.25)
    g, w, g0d = net.gradients(), net.weights(), net._split(_cuda(g0))
    for k in R.NAMES:
        if k.endswith('_w'):
            assert np.abs(g[k].cpu().numpy() - (g0d[k].cpu().numpy().astype(np.float64) + 0.25 * w[k].cpu().numpy())).max() < 1e-6, k
        else:
            assert torch.equal(g[k], g0d[k]), k


# ---- 4. / 5. the whole update --------------------------------------------------------------------------------------------------------
def _params(rs, od, E, hid, twin):
    from rl4rs_amd.offline_rl import init_ddpg_params
    prm = dict(actor=init_ddpg_params(od, 0, E, hid[0], hid[1], seed=1), q1=init_ddpg_params(od, E, 1, hid[0], hid[1], seed=2))
    if twin:
        prm['q2'] = init_ddpg_params(od, E, 1, hid[0], hid[1], seed=3)
    for n in list(prm):
        for k in ('fc1_b', 'fc2_b', 'head_b'):                            # (zero biases would hide a bias touched by the L2 term)
            prm[n][k] = (rs.randn(*prm[n][k].shape) * 0.05).astype(np.float32)
        prm[n + '_targ'] = dict((k, (v + 0.02 * rs.randn(*v.shape)).astype(np.float32)) for k, v in prm[n].items())
    return prm


def _batches(rs, k, M, od, E):
    out = []
    for _ in range(k):
        done = (rs.rand(M) < 0.15).astype(np.int32)
        done[-1] = 1
        out.append(dict(obs=rs.randn(M, od).astype(np.float32), action=(rs.rand(M, E) * 2 - 1).astype(np.float32),
                        reward=rs.randn(M).astype(np.float32), done=done, next_obs=rs.randn(M, od).astype(np.float32),
                        noise=rs.randn(M, E).astype(np.float32), weight=(rs.rand(M) + 0.1).astype(np.float32)))
    return out


PRESETS = {'TD3': dict(twin_q=True, smooth=True, tau=5e-3, l2=1e-3, delay=2, weighted=False),         # (l2 1e-3 so that the term shows)
           'DDPG': dict(twin_q=False, smooth=False, tau=2e-3, l2=1e-6, delay=1, weighted=True)}


def _learner(prm, od, E, hid, M, ps):
    from rl4rs_amd.train import TD3Learner
    return TD3Learner(od, E, M, twin_q=ps['twin_q'], smooth_target_policy=ps['smooth'], target_noise=0.2, target_noise_clip=0.5, tau=ps['tau'],
                      l2_reg=ps['l2'], gamma=1.0, actor_hiddens=hid, critic_hiddens=hid, params=prm)


@pytest.mark.parametrize('od,E,hid,M', [(37, 5, (48, 40), 67), (256, 32, (400, 300), 576), (256, 32, (256, 256), 256)])
@pytest.mark.parametrize('preset', ['TD3', 'DDPG'])
def test_whole_update_tracks_the_restatement(od, E, hid, M, preset):
    ps = PRESETS[preset]
    rs = np.random.RandomState(M + len(preset))
    prm = _params(rs, od, E, hid, ps['twin_q'])
    L = _learner(prm, od, E, hid, M, ps)
    ref = R.TD3Ref(prm, twin_q=ps['twin_q'], smooth=ps['smooth'], tau=ps['tau'], l2_reg=ps['l2'], gamma=1.0)
    names = [n for n, _ in L.named]
    assert len(names) == (6 if ps['twin_q'] else 4)
    last_actor = None
    for it, b in enumerate(_batches(rs, 3, M, od, E)):
        do_actor = it % ps['delay'] == 0
        d = dict((k, _cuda(v)) for k, v in b.items())
        before = L.flat_params()
        m = L.update(d, noise=d['noise'] if ps['smooth'] else None, weights=d['weight'] if ps['weighted'] else None, do_actor=do_actor)
        out = ref.update(b['obs'], b['action'], b['reward'], b['done'], b['next_obs'], noise=b['noise'],
                         weights=b['weight'] if ps['weighted'] else None, do_actor=do_actor)
        m = m.cpu().numpy().astype(np.float64) / M
        want = out['stats'] / M
        assert abs(m[0] - want[0]) < LOSS * max(1.0, abs(want[0])), (it, m[0], want[0])
        ybar = TD_ABS * max(1.0, np.abs(out['y']).max())
        err_td = np.abs(L.td.cpu().numpy() - out['td']).max()
        print('update %d: mean q err %.3g, mean y err %.3g (bar %.3g)  td err %.3g, mean |td| err %.3g (bar %.3g)'
              % (it, abs(m[1] - want[1]), abs(m[2] - want[2]), FWD, err_td, abs(m[3] - want[3]), ybar))
        assert abs(m[1] - want[1]) < FWD and abs(m[2] - want[2]) < FWD, (it, m, want)
        assert err_td < ybar and abs(m[3] - want[3]) < ybar, (it, err_td, m[3], want[3], ybar)
        if do_actor:
            last_actor = out['actor_loss']
        assert abs(m[4] - last_actor) < LOSS * max(1.0, abs(last_actor)), (it, m[4], last_actor)
        after = L.flat_params()
        for n in names:
            err = np.abs(after[n].cpu().numpy() - ref.flat(n)).max()
            assert err < PARAM, (it, n, err)
        import torch
        if not do_actor:                                                   # policy_delay: the actor rests, its target still moves
            assert torch.equal(after['actor'], before['actor']) and not torch.equal(after['actor_targ'], before['actor_targ'])
        else:
            assert not torch.equal(after['actor'], before['actor'])
        assert L.actor.adam_state()[2] == ref.adam['actor']['t'] and L.q1.adam_state()[2] == it + 1
    assert ref.adam['actor']['t'] == (2 if ps['delay'] == 2 else 3)
    L.close()


@pytest.mark.parametrize('od,E,hid,M', [(256, 32, (256, 256), 256), (37, 5, (48, 40), 67), (256, 32, (400, 300), 576)])
@pytest.mark.parametrize('preset', ['TD3', 'DDPG'])
def test_update_as_one_library_call_equals_the_per_phase_calls(od, E, hid, M, preset):
    import torch
    ps = PRESETS[preset]
    rs = np.random.RandomState(7 + M)
    prm = _params(rs, od, E, hid, ps['twin_q'])
    one, phases = _learner(prm, od, E, hid, M, ps), _learner(prm, od, E, hid, M, ps)
    phases.one_call = False
    for it, b in enumerate(_batches(rs, 3, M, od, E)):
        d = dict((k, _cuda(v)) for k, v in b.items())
        kw = dict(noise=d['noise'] if ps['smooth'] else None, weights=d['weight'] if ps['weighted'] else None, do_actor=it % ps['delay'] == 0)
        m1, m2 = one.update(d, **kw).clone(), phases.update(d, **kw).clone()
        assert torch.equal(m1[:4], m2[:4]) and torch.equal(one.td, phases.td)
        assert abs(float(m1[4]) - float(m2[4])) <= 1e-5 * max(1.0, abs(float(m1[4])))       # (the per-phase path sums q with torch)
        p1, p2 = one.flat_params(), phases.flat_params()
        for n in p1:
            assert torch.equal(p1[n], p2[n]), (it, n)
    assert not torch.equal(p1['actor'], _cuda(R.TD3Ref(prm, twin_q=ps['twin_q']).flat('actor').astype(np.float32)))
    one.close()
    phases.close()


# ---- 6. the trainer ----------------------------------------------------------------------------------------------------------------------
def _cfg(d, B=64, T=9, rank=0):
    from rl4rs_amd import synth
    text = synth.make_catalog_text(seed=4)
    cpath = os.path.join(d, 'c.csv')
    if not os.path.exists(cpath):
        synth.write_text(cpath, text)
    lpath = os.path.join(d, 'log%d.csv' % rank)
    recs = synth.make_records(300, seed=2 + rank, hash_size=2000, special_ids=synth.special_ids_from_text(text))
    synth.write_records(lpath, recs)
    return {"maxlen": 64, "batch_size": B, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
            "category_feature_num": 21, "category_hash_size": 2000, "seq_num": 2, "emb_size": 128, "page_items": 9,
            "hidden_units": 128, "max_steps": T, "action_emb_size": 32, "sample_file": lpath, "iteminfo_file": cpath,
            "cache_size": 256, "model_seed": 3, "return_tensors": True, "support_conti_env": True}


def _env(d, rank=0):
    import rl4rs_amd
    from rl4rs_amd.env.slate import SlateRecEnv, SlateState
    return rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(_cfg(d, rank=rank), state_cls=SlateState))


def _param_dicts(learner):
    return dict((n, dict((k, v.cpu().numpy()) for k, v in net.weights().items())) for n, net in learner.named)


@pytest.mark.parametrize('algo', ['TD3', 'DDPG'])
def test_trainer_tracks_a_float64_host_loop(tmp_path, algo):
    """Five train calls against a host loop built from the restatement and fed the device's own sampled rows, weights and noise."""
    from rl4rs_amd.train import TD3Trainer
    env = _env(str(tmp_path))
    env.seed(7)
    tr = TD3Trainer(env, algo=algo, seed=3, init_seed=9, learning_starts=576, random_timesteps=576, train_batch_size=256, buffer_size=2000,
                    keep_last_batch=True)
    L = tr.learner
    assert L.twin_q == (algo == 'TD3') and tr.prioritized == (algo == 'DDPG') and tr.M == 256
    ref = R.TD3Ref(_param_dicts(L), twin_q=L.twin_q, smooth=L.smooth, tau=L.tau, l2_reg=L.l2_reg, gamma=1.0)
    for n, _ in L.named:                                                   # the targets start as copies of the online networks
        if n.endswith('_targ'):
            assert np.array_equal(ref.flat(n), ref.flat(n[:-5]))
    last_actor = 0.0
    for it in range(5):
        st = tr.train_iteration()
        lb = dict((k, (v.cpu().numpy() if hasattr(v, 'cpu') else v)) for k, v in tr.last_batch.items())
        assert lb['idx'].max() < min(it + 1, 3) * 576 and lb['do_actor'] == (it % tr.policy_delay == 0)
        assert (np.abs(lb['action']) <= 1.0).all()
        out = ref.update(lb['obs'], lb['action'], lb['reward'], lb['done'], lb['next_obs'], noise=lb.get('noise'),
                         weights=lb['weight'] if tr.prioritized else None, do_actor=lb['do_actor'])
        if lb['do_actor']:
            last_actor = out['actor_loss']
        got = tr.params()
        for n in got:
            err = np.abs(got[n].cpu().numpy() - ref.flat(n)).max()
            print('iteration %d %s: parameter err %.3g (bar %.3g)' % (it, n, err, PARAM))
            assert err < PARAM, (it, n, err)
        assert abs(st['critic_loss'] - out['critic_loss']) < LOSS * max(1.0, abs(out['critic_loss']))
        assert abs(st['actor_loss'] - last_actor) < LOSS * max(1.0, abs(last_actor))
        assert abs(st['mean_q'] - out['stats'][1] / 256) < FWD and abs(st['mean_td_abs'] - out['stats'][3] / 256) < TD_ABS * max(1.0, np.abs(out['y']).max())
        assert np.abs(lb['td'] - out['td']).max() < TD_ABS * max(1.0, np.abs(out['y']).max())
        assert st['buffer_rows'] == min(it + 1, 3) * 576 and st['num_updates'] == it + 1 and st['iteration'] == it + 1
        if tr.prioritized:                                                 # the priorities took this update's TD errors
            pr = tr.replay.column('priority').cpu().numpy()
            last = dict((int(r), i) for i, r in enumerate(lb['idx']))
            rows = np.array(list(last.keys()))
            want = (np.abs(lb['td'][np.array(list(last.values()))].astype(np.float64)) + 1e-6) ** 0.6
            assert np.allclose(pr[rows], want, rtol=1e-12, atol=0)
    tr.close()


def test_trainer_schedule(tmp_path):
    import torch
    from rl4rs_amd.train import TD3Trainer
    env = _env(str(tmp_path))
    env.seed(1)
    with pytest.raises(ValueError):
        TD3Trainer(env, n_step=3)
    tr = TD3Trainer(env, seed=1, init_seed=2, learning_starts=1200, random_timesteps=1152, train_batch_size=128, buffer_size=1800,
                    keep_last_batch=True)
    assert tr.M == 128 and tr.policy_delay == 2 and tr.replay.counts()[1] == 3 * 576
    p0 = tr.params()
    for it in range(2):                                    # 576, 1152 sampled steps: the random phase, below learning_starts
        st = tr.train_iteration()
        assert st['num_updates'] == 0 and st['critic_loss'] == 0.0 and st['buffer_rows'] == (it + 1) * 576
        assert not bool(tr.ou_state.any()) and (np.abs(tr.buf['act'].cpu().numpy()) < 1.0).all()
    assert all(torch.equal(v, p0[k]) for k, v in tr.params().items())
    st = tr.train_iteration()                              # 1728 steps: the OU noise drives the actor, the first update steps everything
    assert bool(tr.ou_state.any()) and st['num_updates'] == 1 and st['buffer_rows'] == 1728 and tr.last_batch['do_actor']
    p3 = tr.params()
    assert not torch.equal(p3['actor'], p0['actor']) and not torch.equal(p3['q1'], p0['q1'])
    st = tr.train_iteration()                              # update 2: the actor rests, every target moves
    assert st['num_updates'] == 2 and st['buffer_rows'] == 1728 and not tr.last_batch['do_actor']
    p4 = tr.params()
    assert torch.equal(p4['actor'], p3['actor']) and not torch.equal(p4['actor_targ'], p3['actor_targ'])
    assert not torch.equal(p4['q1'], p3['q1']) and not torch.equal(p4['q2_targ'], p3['q2_targ'])
    st = tr.train_iteration()
    assert st['num_updates'] == 3 and tr.last_batch['do_actor'] and not torch.equal(tr.params()['actor'], p4['actor'])
    assert tr.learner.actor.adam_state()[2] == 2 and tr.learner.q1.adam_state()[2] == 3
    assert abs(tr.scale_at(1152) - 0.1) < 1e-12 and abs(tr.scale_at(1152 + 5000) - 0.051) < 1e-12 and abs(tr.scale_at(10 ** 6) - 0.002) < 1e-12
    tr.close()


def test_evaluate_is_deterministic_and_every_played_action_is_legal(tmp_path):
    """No assertion that the return improved: 160 updates on a synthetic catalogue promise nothing for an actor-critic."""
    from rl4rs_amd.train import TD3Trainer
    env = _env(str(tmp_path))
    env.seed(5)
    tr = TD3Trainer(env, seed=2, init_seed=4, learning_starts=576, random_timesteps=576, train_batch_size=256, updates_per_rollout=8)
    e0 = tr.evaluate(episodes=128, seed=11)
    assert e0 == tr.evaluate(episodes=128, seed=11)
    for _ in range(20):
        st = tr.train_iteration()
        assert env.samples.get_violation().all()           # the K-NN is masked: whatever the actor says resolves to a legal item
    assert st['num_updates'] == 160 and np.isfinite(list(st.values())).all()
    e1 = tr.evaluate(episodes=128, seed=11)
    assert e1 == tr.evaluate(episodes=128, seed=11) and np.isfinite(e1)
    print('deterministic evaluate: %.4f before, %.4f after 20 iterations (160 updates)' % (e0, e1))
    tr.close()


# ---- 7. two ranks ----------------------------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, d, iters, out):
    import torch
    from test_gpu_train_dp import _init_dist
    D = _init_dist(rank, world, port)
    from rl4rs_amd.train import TD3Trainer
    env = _env(d, rank=rank)
    env.seed(100 + rank)
    tr = TD3Trainer(env, seed=1 + rank, init_seed=5, learning_starts=576, random_timesteps=576, train_batch_size=128, buffer_size=2000,
                    keep_last_batch=True)
    log = []
    for _ in range(iters):
        tr.train_iteration()
        log.append(dict(params=dict((k, v.cpu()) for k, v in tr.params().items()), obs=tr.last_batch['obs'].cpu()))
    D.barrier()
    torch.save(log, os.path.join(d, 'td3_rank%d.pt' % rank))
    out.put(rank)


def test_two_ranks_keep_identical_replicas(tmp_path):
    import torch
    from test_gpu_train_dp import _spawn
    d = str(tmp_path)
    _spawn(_dp_worker, (d, 2), deadline=240)
    r0 = torch.load(os.path.join(d, 'td3_rank0.pt'), weights_only=False)
    r1 = torch.load(os.path.join(d, 'td3_rank1.pt'), weights_only=False)
    for i in range(2):
        assert not torch.equal(r0[i]['obs'], r1[i]['obs'])                 # the ranks drew different minibatches ...
        for n in r0[i]['params']:                                          # ... and still hold the same parameters, bit for bit
            assert torch.equal(r0[i]['params'][n], r1[i]['params'][n]), (i, n)
    assert not torch.equal(r0[0]['params']['q1'], r0[1]['params']['q1'])
