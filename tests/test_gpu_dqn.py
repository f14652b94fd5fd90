"""GPU: the on-device DQN (replay memory, double-Q loss kernels, greedy action, per-variable-clipped Adam, DQNTrainer) against
the float64 restatement in tests/dqn_ref.py.

Bars are those of tests/test_gpu_policy.py: Q values 1e-5 abs, gradients within 2e-4 of the reference gradient's max-norm.  A TD
error is the difference of two Q-valued terms, so it is held to 2e-5 plus the fp32 rounding of r + gamma * Q (|r| < 16: 1e-6).
An integer a* / greedy action is compared on every row whose float64 top-two masked Q gap is >= 1e-4 (ten times the Q bar); at
most 1 % of the rows may fall under that gap."""
import os

import numpy as np
import pytest

import dqn_ref as R

pytestmark = pytest.mark.gpu

Q_ABS = 1e-5
TD_ABS = 2e-5 + 1e-6
GAP = 1e-4


def _pack(mask):
    N, A = mask.shape
    W = (A + 31) // 32
    bits = np.zeros((N, W), dtype=np.uint32)
    for k in range(A):
        bits[:, k >> 5] |= (mask[:, k].astype(np.uint32) << np.uint32(k & 31))
    return bits.view(np.int32)


def _case(rs, N, od, hid, A):
    from rl4rs_amd.nets.policy import init_policy_params, param_count
    n = param_count(od, hid, A)
    flat = init_policy_params(od, hid, A, seed=1) + (rs.randn(n) * 0.05).astype(np.float32)
    tflat = flat + (rs.randn(n) * 0.02).astype(np.float32)
    obs, nobs = rs.randn(N, od).astype(np.float32), rs.randn(N, od).astype(np.float32)
    mask = (rs.rand(N, A) < 0.4).astype(np.int64)
    mask[np.arange(N), rs.randint(0, A, size=N)] = 1
    done = (rs.rand(N) < 0.15).astype(np.int32)
    done[-1] = 1
    k = int(np.nonzero(done == 0)[0][0])
    mask[k] = 0                                             # ONE non-terminal successor row that allows nothing
    act = rs.randint(0, A, size=N).astype(np.int32)
    rew = (rs.randn(N) * 2.0).astype(np.float32)
    w = (rs.rand(N) + 0.1).astype(np.float32)
    return dict(flat=flat, tflat=tflat, obs=obs, nobs=nobs, mask=mask, bits=_pack(mask), done=done, act=act, rew=rew, w=w, k=k)


def _dev(c):
    import torch
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return dict((k, t(c[k])) for k in ('tflat', 'obs', 'nobs', 'bits', 'done', 'act', 'rew', 'w'))


@pytest.mark.parametrize('od,hid,A,N,double_q,tile,weighted', [
    (256, 64, 284, 1024, True, 1, True),          # the default shape
    (256, 64, 284, 1003, True, 1, True),          # N not a multiple of 8
    (256, 64, 50, 517, True, 1, False),           # action_size not a multiple of 32
    (256, 128, 284, 1024, True, 1, True),         # hidden 128
    (100, 48, 75, 333, True, 0, True),            # the one-wave-per-row path, at a shape no tiled kernel takes
    (256, 64, 284, 1024, False, 1, True),         # double_q off: the target net picks a*
    (256, 64, 284, 601, False, 0, False),
    (10, 48, 40, 16500, True, 0, True),           # 33 chunks of the sample-axis reductions (the handle's chunk is 512 rows)
    (256, 64, 284, 16500, True, 1, True),
    (10, 48, 40, 32800, True, 0, True),           # ceil(N / 512) = 65 > 64: the reductions re-chunk to 576 rows
])
def test_loss_and_gradient_match_the_restatement(od, hid, A, N, double_q, tile, weighted):
    import torch
    from rl4rs_amd.device import DevicePolicy
    rs = np.random.RandomState(N + hid + A)
    c = _case(rs, N, od, hid, A)
    d = _dev(c)
    pol = DevicePolicy(od, hid, A, max_rows=N, params=c['flat'])
    pol.set_option('tile', tile)
    w_dev, w_np = (d['w'], c['w']) if weighted else (None, None)
    run = lambda nobs, bits: pol.dqn_loss_grad(d['tflat'], d['obs'], d['act'], d['rew'], d['done'], nobs, bits, weights=w_dev,
                                               gamma=0.9, double_q=double_q, want_next_action=True)
    g, td, stats, astar = run(d['nobs'], d['bits'])
    g_np, td_np, a_np = g.cpu().numpy(), td.cpu().numpy(), astar.cpu().numpy()
    kw = dict(gamma=0.9, double_q=double_q, od=od, hid=hid, A=A)
    ref0 = R.dqn_loss_and_grad(c['flat'], c['tflat'], c['obs'], c['act'], c['rew'], c['done'], c['nobs'], c['mask'], w_np, **kw)
    boot, gap = ref0['boot'], ref0['gap']
    assert (~boot & (c['done'] == 0)).sum() == 1 and not boot[c['k']]
    # the integer a*: equal wherever the float64 decision is not a near-tie; terminal rows report -1
    firm = boot & (gap >= GAP)
    left_out = int((boot & ~firm).sum())
    print('a*: %d of %d bootstrapping rows under the %.0e gap' % (left_out, int(boot.sum()), GAP))
    assert left_out <= 0.01 * N
    assert np.array_equal(a_np[firm], ref0['astar_ref'][firm])
    assert (a_np[c['done'] != 0] == -1).all()
    assert ((a_np[boot] >= 0) & (a_np[boot] < A)).all() and c['mask'][np.nonzero(boot)[0], a_np[boot]].all()
    # loss and gradient of the restatement with the device's a* on the bootstrapping rows
    ref = R.dqn_loss_and_grad(c['flat'], c['tflat'], c['obs'], c['act'], c['rew'], c['done'], c['nobs'], c['mask'], w_np, astar=a_np, **kw)
    err_td = np.abs(td_np - ref['td']).max()
    err_g, g_max = np.abs(g_np - ref['grad']).max(), np.abs(ref['grad']).max()
    print('td err %.3g (bar %.3g)  grad err %.3g (bar %.3g)' % (err_td, TD_ABS, err_g, 2e-4 * g_max))
    assert err_td < TD_ABS
    assert err_g < 2e-4 * g_max
    assert np.allclose(stats.cpu().numpy(), ref['stats'], rtol=2e-4, atol=1e-3)
    # the all-masked non-terminal successor bootstraps nothing: y = r, everything finite
    assert np.isfinite(g_np).all() and np.isfinite(td_np).all()
    assert abs(td_np[c['k']] - (ref['qsa'][c['k']] - c['rew'][c['k']])) < TD_ABS
    # value head: exactly zero
    gW2 = g_np[od * hid + hid:od * hid + hid + hid * (A + 1)].reshape(hid, A + 1)
    assert (gW2[:, A] == 0).all() and g_np[-1] == 0
    # bit-identical from run to run
    g2, td2, stats2, astar2 = run(d['nobs'], d['bits'])
    assert torch.equal(g, g2) and torch.equal(td, td2) and torch.equal(stats, stats2) and torch.equal(astar, astar2)
    # nothing of a terminal row's successor is used: NaN there changes nothing
    nobs_nan = d['nobs'].clone()
    nobs_nan[d['done'] != 0] = float('nan')
    bits_junk = d['bits'].clone()
    bits_junk[d['done'] != 0] = -1
    g3, td3, stats3, astar3 = run(nobs_nan, bits_junk)
    assert torch.equal(g, g3) and torch.equal(td, td3) and torch.equal(stats, stats3) and torch.equal(astar, astar3)


@pytest.mark.parametrize('od,hid,A,N,tile', [(256, 64, 284, 1003, 1), (256, 128, 284, 512, 1), (100, 48, 75, 333, 0), (256, 64, 284, 77, 0)])
def test_greedy_action_is_the_first_maximum_of_the_masked_q(od, hid, A, N, tile):
    import torch
    from rl4rs_amd.device import DevicePolicy
    from oracle import policy as OP
    rs = np.random.RandomState(N + A)
    c = _case(rs, N, od, hid, A)
    pol = DevicePolicy(od, hid, A, max_rows=N, params=c['flat'])
    pol.set_option('tile', tile)
    o, b = torch.from_numpy(c['obs']).cuda(), torch.from_numpy(c['bits']).cuda()
    a, q = pol.greedy(o, b, want_q=True)
    a_np, q_np = a.cpu().numpy(), q.cpu().numpy()
    q_ref = OP.forward(c['flat'], c['obs'], c['mask'], od, hid, A)[0]
    ok = c['mask'] > 0
    print('Q err %.3g (bar %.3g)' % (np.abs(q_np[ok] - q_ref[ok]).max(), Q_ABS))
    assert np.abs(q_np[ok] - q_ref[ok]).max() < Q_ABS
    assert (q_np[~ok] < -1e37).all()
    top = np.sort(q_ref, axis=1)[:, -2:]
    legal = ok.any(axis=1)
    firm = legal & (top[:, 1] - top[:, 0] >= GAP)
    assert (legal & ~firm).sum() <= 0.01 * N
    assert np.array_equal(a_np[firm], q_ref.argmax(axis=1)[firm])
    assert c['mask'][np.nonzero(legal)[0], a_np[legal]].all()             # never a masked action
    assert a_np[c['k']] == 0                                              # a row that allows nothing: action 0
    assert torch.equal(pol.greedy(o, b)[0], a)
    # no mask: plain argmax
    a_nm = pol.greedy(o, None)[0].cpu().numpy()
    q_nm = OP.forward(c['flat'], c['obs'], None, od, hid, A)[0]
    t2 = np.sort(q_nm, axis=1)[:, -2:]
    f2 = t2[:, 1] - t2[:, 0] >= GAP
    assert np.array_equal(a_nm[f2], q_nm.argmax(axis=1)[f2])


def test_adam_step_clips_each_variable_by_its_own_norm():
    import torch
    from rl4rs_amd.device import DevicePolicy
    from rl4rs_amd.nets.policy import init_policy_params
    od, hid, A = 256, 64, 284
    rs = np.random.RandomState(5)
    flat = init_policy_params(od, hid, A, seed=2)
    pol = DevicePolicy(od, hid, A, max_rows=8, params=flat)
    ends = np.cumsum([od * hid, hid, hid * (A + 1), A + 1])
    state = (flat.astype(np.float64), np.zeros(len(flat)), np.zeros(len(flat)), 0)
    for step, scales in enumerate([(1.0, 0.01, 0.5, 0.02), (0.001, 2.0, 0.3, 0.001)]):
        g = rs.randn(len(flat)).astype(np.float32)
        lo = 0
        norms = []
        for hi, s in zip(ends, scales):
            g[lo:hi] *= s
            norms.append(float(np.sqrt((g[lo:hi].astype(np.float64) ** 2).sum())))
            lo = hi
        clip = 4.0
        active = [n > clip for n in norms]
        assert any(active) and not all(active), norms       # the clip bites some variables and leaves others alone
        before = pol.params().cpu().numpy().astype(np.float64)
        pol.adam_step_clip_by_var(torch.from_numpy(g).cuda(), lr=1e-3, eps=1e-8, var_clip=clip)
        after = pol.params().cpu().numpy().astype(np.float64)
        state = R.adam_clip_by_var(state[0], state[1], state[2], state[3], g, 1e-3, clip, od, hid, A)
        # rtol 1e-3 on the step (the existing Adam comparison's), atol = fp32 spacing of parameters below 1 (1.2e-7)
        assert np.allclose(after - before, state[0] - before, rtol=1e-3, atol=1.2e-7)
        assert np.abs(after - state[0]).max() < 1e-6
    m, v, t = pol.adam_state()
    assert t == 2 and np.allclose(m.cpu().numpy(), state[1], rtol=1e-3, atol=1e-9)


# ---- replay memory ---------------------------------------------------------------------------------------------------
def _rollout(rs, T, B, od, A):
    import torch
    R_ = T * B
    obs = rs.randn(R_, od).astype(np.float32)
    mask = (rs.rand(R_, A) < 0.5).astype(np.int64)
    act = rs.randint(0, A, size=R_).astype(np.int32)
    rew = rs.randn(R_) * 3.0
    host = dict(obs=obs, mask=_pack(mask), act=act, rew=rew)
    return host, dict((k, torch.from_numpy(v).cuda()) for k, v in host.items())


def test_ring_holds_whole_rollouts_and_evicts_the_oldest():
    from rl4rs_amd.device import DeviceReplay
    T, B, od, A = 3, 4, 8, 40
    rs = np.random.RandomState(0)
    rp = DeviceReplay(od, A, T, B, buffer_size=25, alpha=0.6)
    assert rp.counts() == (0, 24, 0)
    hosts = []
    for k in range(3):
        h, d = _rollout(rs, T, B, od, A)
        rp.push(d['obs'], d['mask'], d['act'], d['rew'])
        hosts.append(h)
        assert rp.counts() == (R.filled_rows(k + 1, 25, T, B), 24, k + 1)
    col = dict((k, rp.column(k).cpu().numpy()) for k in ('obs', 'mask', 'action', 'reward', 'done', 'priority'))
    for slot, h in ((0, hosts[2]), (1, hosts[1])):         # rollout 0 is gone: push 2 took its slot
        sl = slice(slot * T * B, (slot + 1) * T * B)
        assert np.array_equal(col['obs'][sl], h['obs']) and np.array_equal(col['mask'][sl], h['mask'])
        assert np.array_equal(col['action'][sl], h['act'])
        assert np.array_equal(col['reward'][sl], h['rew'].astype(np.float32))
    assert not (col['obs'] == hosts[0]['obs'][0]).all(axis=1).any()
    assert np.array_equal(col['done'], R.row_fields(np.arange(24), T, B)[3].astype(np.int32))
    assert (col['priority'] == 1.0).all() and rp.max_priority() == 1.0


@pytest.mark.parametrize('od', [256, 10])
def test_uniform_sampling_gathers_rows_and_successors_exactly(od):
    from rl4rs_amd.device import DeviceReplay
    T, B, A = 5, 8, 70
    rs = np.random.RandomState(1)
    rp = DeviceReplay(od, A, T, B, buffer_size=3 * T * B, alpha=0.6)
    for _ in range(2):
        d = _rollout(rs, T, B, od, A)[1]
        rp.push(d['obs'], d['mask'], d['act'], d['rew'])
    n = rp.rows
    assert n == 80 and rp.counts()[1] == 120
    M = 4001
    b = rp.sample(M, prioritized=False, seed=9, step=4, want_u=True)
    s = dict((k, v.cpu().numpy()) for k, v in b.items())
    assert ((s['u'] > 0) & (s['u'] < 1)).all()
    idx = s['idx']
    assert np.array_equal(idx, R.uniform_select(s['u'].astype(np.float64), n))
    assert (np.bincount(idx, minlength=n) > 0).all()
    col = dict((k, rp.column(k).cpu().numpy()) for k in ('obs', 'mask', 'action', 'reward', 'done'))
    _, _, _, done, nxt = R.row_fields(idx, T, B)
    assert np.array_equal(s['obs'], col['obs'][idx]) and np.array_equal(s['action'], col['action'][idx])
    assert np.array_equal(s['reward'], col['reward'][idx]) and np.array_equal(s['done'], done.astype(np.int32))
    live = ~done
    assert live.any() and done.any()
    assert np.array_equal(s['next_obs'][live], col['obs'][nxt[live]]) and np.array_equal(s['next_mask'][live], col['mask'][nxt[live]])
    assert np.isfinite(s['next_obs']).all()                # terminal rows: anything finite
    assert (s['weight'] == 1.0).all()


def test_prioritized_sampling_follows_the_float64_prefix_sums():
    import torch
    from rl4rs_amd.device import DeviceReplay
    T, B, od, A = 9, 64, 16, 40
    rs = np.random.RandomState(2)
    rp = DeviceReplay(od, A, T, B, buffer_size=6 * T * B, alpha=0.6)
    for _ in range(5):
        d = _rollout(rs, T, B, od, A)[1]
        rp.push(d['obs'], d['mask'], d['act'], d['rew'])
    n = rp.rows
    assert n == 2880                                       # three 1024-row scan tiles, the last one partial
    prio = rs.rand(n) * 5.0 + 0.01
    rp.set_priorities(torch.from_numpy(prio))
    M = 8192
    b = rp.sample(M, prioritized=True, beta=0.4, seed=3, step=0, want_u=True)
    u, idx, w = b['u'].cpu().numpy().astype(np.float64), b['idx'].cpu().numpy(), b['weight'].cpu().numpy()
    ref, dist, total = R.prioritized_select(prio, u)
    near = dist < 1e-9 * total
    print('prioritized: %d of %d draws within 1e-9 * total of a boundary' % (near.sum(), M))
    assert near.sum() <= 0.001 * M
    assert np.array_equal(idx[~near], ref[~near])
    assert np.allclose(w, R.is_weights(prio, idx, 0.4), rtol=1e-6, atol=0)
    # the gather is the uniform mode's
    col_obs = rp.column('obs').cpu().numpy()
    assert np.array_equal(b['obs'].cpu().numpy(), col_obs[idx])
    # same (seed, step): the same batch; another step: another batch
    b2 = rp.sample(M, prioritized=True, beta=0.4, seed=3, step=0, want_u=True)
    assert all(torch.equal(b[k], b2[k]) for k in b)
    b3 = rp.sample(M, prioritized=True, beta=0.4, seed=3, step=1)
    assert not torch.equal(b['idx'], b3['idx'])


def test_prioritized_frequencies_follow_the_priorities():
    import torch
    from rl4rs_amd.device import DeviceReplay
    T, B, od, A = 2, 32, 8, 40
    rs = np.random.RandomState(3)
    rp = DeviceReplay(od, A, T, B, buffer_size=T * B, alpha=0.6)
    d = _rollout(rs, T, B, od, A)[1]
    rp.push(d['obs'], d['mask'], d['act'], d['rew'])
    prio = rs.rand(64) ** 2 * 4.0 + 0.05
    rp.set_priorities(torch.from_numpy(prio))
    M = 200000
    idx = rp.sample(M, prioritized=True, beta=0.4, seed=1, step=0)['idx'].cpu().numpy()
    freq = np.bincount(idx, minlength=64) / float(M)
    print('frequency err %.4f (bar 0.01)' % np.abs(freq - prio / prio.sum()).max())
    assert np.abs(freq - prio / prio.sum()).max() < 0.01


def test_priority_update_with_repeated_indices():
    import torch
    from rl4rs_amd.device import DeviceReplay
    T, B, od, A = 4, 16, 8, 40
    rs = np.random.RandomState(4)
    rp = DeviceReplay(od, A, T, B, buffer_size=2 * T * B, alpha=0.6)
    d = _rollout(rs, T, B, od, A)[1]
    rp.push(d['obs'], d['mask'], d['act'], d['rew'])
    M = 300                                                # 300 draws over 64 rows: every row repeats
    idx = rs.randint(0, 64, size=M).astype(np.int32)
    td = (rs.randn(M) * 3.0).astype(np.float32)
    rp.update_priorities(torch.from_numpy(idx).cuda(), torch.from_numpy(td).cuda())
    new, mx = R.update_priorities(np.ones(64), 1.0, idx, td, alpha=0.6)
    got = rp.column('priority').cpu().numpy()[:64]
    assert np.allclose(got, new, rtol=1e-12, atol=0)       # (device pow against numpy's)
    last = dict((int(r), i) for i, r in enumerate(idx))    # the highest batch position of every row
    assert all(np.isclose(got[r], (abs(float(td[i])) + 1e-6) ** 0.6, rtol=1e-12) for r, i in last.items())
    assert rp.max_priority() == mx and mx > 1.0
    # a smaller batch afterwards does not lower max_priority; new rows enter at max_priority ^ alpha
    rp.update_priorities(torch.from_numpy(idx[:4]).cuda(), torch.zeros(4, device='cuda'))
    assert rp.max_priority() == mx
    rp.push(d['obs'], d['mask'], d['act'], d['rew'])
    assert np.allclose(rp.column('priority').cpu().numpy()[64:], mx ** 0.6, rtol=1e-12, atol=0)
    # twice the same update: the same bits
    a = rp.column('priority').clone()
    rp.update_priorities(torch.from_numpy(idx).cuda(), torch.from_numpy(td).cuda())
    b = rp.column('priority').clone()
    rp.update_priorities(torch.from_numpy(idx).cuda(), torch.from_numpy(td).cuda())
    assert torch.equal(b, rp.column('priority')) and not torch.equal(a, b)


# ---- trainer ---------------------------------------------------------------------------------------------------------
def _env(d, B=64, T=9):
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
    return rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))


def test_trainer_tracks_a_float64_host_loop(tmp_path):
    """Five train calls against a host loop built from the restatement and fed the device's own sampled rows, weights and a*:
    parameters to the 2e-5 of test_trainer_tracks_fp64_ppo_restatement."""
    from rl4rs_amd.train import DQNTrainer
    env = _env(str(tmp_path))
    env.seed(7)
    tr = DQNTrainer(env, seed=3, init_seed=9, lr=1e-3, learning_starts=576, train_batch_size=256, buffer_size=2000,
                    target_network_update_freq=1500, keep_last_batch=True)
    flat = tr.params().cpu().numpy().astype(np.float64)
    state = (flat, np.zeros_like(flat), np.zeros_like(flat), 0)
    target = flat.copy()
    syncs = 0
    for it in range(5):
        st = tr.train_iteration()
        lb = dict((k, v.cpu().numpy()) for k, v in tr.last_batch.items())
        assert lb['idx'].max() < min(it + 1, 3) * 576
        out = R.dqn_loss_and_grad(state[0], target, lb['obs'], lb['action'], lb['reward'], lb['done'], lb['next_obs'],
                                  R.unpack_bits(lb['next_mask'], 284), lb['weight'], gamma=1.0, double_q=True, astar=lb['next_action'])
        state = R.adam_clip_by_var(state[0], state[1], state[2], state[3], out['grad'], 1e-3, 40.0, 256, 64, 284)
        got = tr.params().cpu().numpy()
        err = np.abs(got - state[0]).max()
        print('iteration %d: parameter err %.3g (bar 2e-5)' % (it, err))
        assert err < 2e-5, (it, err)
        assert abs(st['td_loss'] - out['loss']) < 1e-5 + 2e-3 * abs(out['loss'])
        assert abs(st['mean_q'] - out['qsa'].mean()) < 1e-4 and st['buffer_rows'] == min(it + 1, 3) * 576
        assert st['num_updates'] == it + 1 and st['iteration'] == it + 1
        if st['num_target_updates'] != syncs:                               # the device copied online -> target after this update
            syncs = st['num_target_updates']
            target = state[0].copy()
    assert syncs == 1


def test_trainer_learning_starts_and_target_schedule(tmp_path):
    import torch
    from rl4rs_amd.train import DQNTrainer
    env = _env(str(tmp_path))
    env.seed(1)
    with pytest.raises(ValueError):
        DQNTrainer(env, n_step=3)
    tr = DQNTrainer(env, seed=1, init_seed=2, lr=1e-3, learning_starts=1200, target_network_update_freq=1500, train_batch_size=128)
    assert tr.M == 128 and DQNTrainer(env).M == 576
    p0 = tr.params().clone()
    assert torch.equal(tr.target, p0)
    for it in range(2):                                    # 576, 1152 sampled steps: below learning_starts
        st = tr.train_iteration()
        assert st['num_updates'] == 0 and st['td_loss'] == 0.0 and st['buffer_rows'] == (it + 1) * 576
        assert torch.equal(tr.params(), p0)
    st = tr.train_iteration()                              # 1728 steps: trains, and 1728 - 0 >= 1500: the target is copied AFTER the update
    assert st['num_updates'] == 1 and st['num_target_updates'] == 1 and st['td_loss'] > 0
    p3 = tr.params().clone()
    assert not torch.equal(p3, p0) and torch.equal(tr.target, p3)
    st = tr.train_iteration()                              # 2304 - 1728 < 1500: no copy, the nets differ
    assert st['num_updates'] == 2 and st['num_target_updates'] == 1
    assert torch.equal(tr.target, p3) and not torch.equal(tr.params(), p3)
    tr.train_iteration()                                   # 2880 - 1728 < 1500
    st = tr.train_iteration()                              # 3456 - 1728 >= 1500
    assert st['num_target_updates'] == 2 and torch.equal(tr.target, tr.params())
    assert np.isfinite(list(st.values())).all()
    assert env.samples.get_violation().all()               # SoftQ over the masked Q only ever plays legal actions


def test_evaluate_is_deterministic_and_training_does_not_hurt(tmp_path):
    from rl4rs_amd.train import DQNTrainer
    env = _env(str(tmp_path))
    env.seed(5)
    tr = DQNTrainer(env, seed=2, init_seed=4, learning_starts=576, updates_per_rollout=16)
    e0 = tr.evaluate(episodes=128, seed=11)
    assert e0 == tr.evaluate(episodes=128, seed=11)
    for _ in range(20):
        st = tr.train_iteration()
    assert st['num_updates'] == 320 and np.isfinite(list(st.values())).all()
    e1 = tr.evaluate(episodes=128, seed=11)
    assert e1 == tr.evaluate(episodes=128, seed=11)
    print('greedy evaluate: %.4f before, %.4f after 20 iterations (320 updates)' % (e0, e1))
    assert e1 >= e0
