"""GPU: one OPE step of a score-matrix policy (rl4rs_ope_greedy_rows, rl4rs_policy_ope_step), ``policy_model`` over the online
trainers and ``ope_eval`` with a trainer (the ope stage of script/modelfree_train.py:498-514).

Bars.  The row kernel is held to its own masked row read back: the action is numpy's first maximum of those float32 values (no gap
rule), the row is the host's float32 application of the mask rule bit for bit, pi is within rtol 1e-12 of numpy's float64 softmax
(the bar of test_fused_softmax_propensity), q is exact.  The handle form is held to ``oracle.policy.forward`` in float64 with the
bars tests/test_gpu_dqn.py takes from tests/test_gpu_policy.py (logits and value 1e-5 abs); pi = exp(l_a - logsumexp(l)) carries the
logit bar twice, so rtol 2e-5.  Measured errors: DESIGN 37."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Q_ABS = 1e-5
PI_RTOL = 2e-5
NEG = np.float32(-3.4028235e38)


def _pack(mask):
    N, A = mask.shape
    W = (A + 31) // 32
    bits = np.zeros((N, W), dtype=np.uint32)
    for k in range(A):
        bits[:, k >> 5] |= (mask[:, k].astype(np.uint32) << np.uint32(k & 31))
    return bits.view(np.int32)


def _unpack(bits, A):
    b = bits.view(np.uint32)
    return np.stack([(b[:, k >> 5] >> np.uint32(k & 31)) & 1 for k in range(A)], axis=1).astype(bool)


def _softmax64(m):
    z = m.astype(np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _rel(got, want):
    return float((np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).max()) if got.size else 0.0


def _bits_equal(a, b):
    import torch
    return torch.equal(a.view(torch.int64), b.view(torch.int64))          # (NaN == NaN)


# ---- 1. the row kernel ------------------------------------------------------------------------------------------------
ROW_NOTHING, ROW_FORBIDDEN_LOGGED, ROW_LOGGED_A, ROW_LOGGED_NEG, ROW_TIES, ROW_FORBIDDEN_MAX = 0, 1, 2, 3, (4, 5, 6), 7


def _row_case(A, pad, N):
    rs = np.random.RandomState(A + pad + N)
    full = (rs.randn(N, A + pad) * 4).astype(np.float32)
    mask = rs.rand(N, A) < 0.4
    mask[np.arange(N), rs.randint(0, A, size=N)] = True
    logged = rs.randint(0, A, size=N).astype(np.int32)
    mask[ROW_NOTHING] = False
    mask[ROW_FORBIDDEN_LOGGED, [0, 3]] = [True, False]
    logged[ROW_FORBIDDEN_LOGGED] = 3
    logged[ROW_LOGGED_A], logged[ROW_LOGGED_NEG] = A, -1
    for r in ROW_TIES:                                      # the maximum copied into a LATER allowed column: the first wins
        mask[r, [1, 4]] = True
        full[r, [1, 4]] = np.abs(full[r, :A]).max() + np.float32(1.0)
    mask[ROW_FORBIDDEN_MAX, [2, 5]] = [False, True]
    full[ROW_FORBIDDEN_MAX, 2] = 100.0
    return full, mask, logged, (rs.randn(N) * 3).astype(np.float32), (rs.randn(N, A + 1) * 3).astype(np.float32)


# (4500, 0, 9): a row beyond the wave's share of LDS - the path that reads the row from memory a second time
@pytest.mark.parametrize('A,pad,N', [(284, 1, 333), (284, 0, 77), (75, 0, 333), (7, 1, 77), (1000, 0, 130), (4500, 0, 9)])
def test_row_kernel_against_its_own_masked_row(A, pad, N):
    import torch
    from rl4rs_amd.device import ope_greedy_rows
    full, mask, logged, value, value_wide = _row_case(A, pad, N)
    scores = torch.from_numpy(full).cuda()[:, :A]
    assert scores.stride(0) == A + pad
    s = full[:, :A]
    bits, lg = torch.from_numpy(_pack(mask)).cuda(), torch.from_numpy(logged).cuda()
    v1, vw = torch.from_numpy(value).cuda(), torch.from_numpy(value_wide).cuda()[:, A]
    assert vw.stride(0) == A + 1
    valid = (logged >= 0) & (logged < A)
    rows = np.arange(N)
    worst = 0.0
    for mask_set, m_dev, allowed in ((0, bits, mask), (1, bits, mask), (0, None, np.ones_like(mask))):
        with np.errstate(over='ignore'):
            want_row = np.where(allowed, s, (s + NEG).astype(np.float32) if mask_set == 0 else NEG).astype(np.float32)
        for val, val_np in ((None, None), (v1, value), (vw, value_wide[:, A])):
            out = torch.empty((N, A), dtype=torch.float32, device='cuda')
            a, pi, q = ope_greedy_rows(scores, lg, mask_bits=m_dev, mask_set=mask_set, value=val, masked_out=out)
            m = out.cpu().numpy()
            a_np, pi_np, q_np = a.cpu().numpy(), pi.cpu().numpy(), q.cpu().numpy()
            assert np.array_equal(m.view(np.int32), want_row.view(np.int32))
            assert np.array_equal(a_np, m.argmax(axis=1))
            ref = _softmax64(m)[rows[valid], logged[valid]]
            err = _rel(pi_np[valid], ref)
            worst = max(worst, err)
            assert err <= 1e-12, err
            assert np.isnan(pi_np[ROW_LOGGED_A]) and np.isnan(pi_np[ROW_LOGGED_NEG]) and not np.isnan(pi_np[valid]).any()
            assert q_np.dtype == np.float64
            assert np.array_equal(q_np, (m[rows, a_np] if val is None else val_np).astype(np.float64))
            if m_dev is not None:
                assert a_np[ROW_NOTHING] == 0 and pi_np[ROW_NOTHING] == 1.0 / A
                assert pi_np[ROW_FORBIDDEN_LOGGED] == 0.0
                assert a_np[ROW_FORBIDDEN_MAX] != 2 and allowed[rows[1:], a_np[1:]].all()
            else:
                assert a_np[ROW_FORBIDDEN_MAX] == 2
            assert all(a_np[r] == 1 for r in ROW_TIES)
            a2, pi2, q2 = ope_greedy_rows(scores, lg, mask_bits=m_dev, mask_set=mask_set, value=val)
            assert torch.equal(a, a2) and _bits_equal(pi, pi2) and _bits_equal(q, q2)
    print('A %d ld %d N %d: pi rel err %.3g (bar 1e-12)' % (A, A + pad, N, worst))


# ---- 2. the mask-model handle -------------------------------------------------------------------------------------------
def _policy_case(rs, N, od, hid, A):
    """parameters perturbed off their initialisation, a 40 % mask with one row that allows nothing (tests/test_gpu_dqn.py::_case)"""
    from rl4rs_amd.nets.policy import init_policy_params, param_count
    flat = init_policy_params(od, hid, A, seed=1) + (rs.randn(param_count(od, hid, A)) * 0.05).astype(np.float32)
    obs = rs.randn(N, od).astype(np.float32)
    mask = (rs.rand(N, A) < 0.4).astype(np.int64)
    mask[np.arange(N), rs.randint(0, A, size=N)] = 1
    mask[3] = 0
    logged = rs.randint(0, A, size=N).astype(np.int32)
    logged[5] = int(np.nonzero(mask[5] == 0)[0][0])         # a forbidden logged action
    return flat, obs, mask, logged


@pytest.mark.parametrize('q_mode', [0, 1])
@pytest.mark.parametrize('od,hid,A,N', [(256, 64, 284, 333), (256, 128, 284, 77), (100, 48, 75, 130)])
def test_policy_ope_step_against_the_float64_forward(od, hid, A, N, q_mode):
    import torch
    from oracle import policy as OP
    from rl4rs_amd._lib import Rl4rsHipError
    from rl4rs_amd.device import DevicePolicy
    flat, obs, mask, logged = _policy_case(np.random.RandomState(N + hid + A), N, od, hid, A)
    pol = DevicePolicy(od, hid, A, max_rows=N, params=flat)
    o, b, lg = torch.from_numpy(obs).cuda(), torch.from_numpy(_pack(mask)).cuda(), torch.from_numpy(logged).cuda()
    out = torch.empty((N, A), dtype=torch.float32, device='cuda')
    a, pi, q = pol.ope_step(o, b, lg, q_mode, masked_out=out)
    m, a_np, pi_np, q_np = out.cpu().numpy(), a.cpu().numpy(), pi.cpu().numpy(), q.cpu().numpy()
    logits, value = OP.forward(flat, obs, mask, od, hid, A)
    ok = mask > 0
    err_l = np.abs(m[ok] - logits[ok]).max()
    assert err_l < Q_ABS and (m[~ok] < -1e37).all()
    rows = np.arange(N)
    if q_mode == 0:
        err_q = np.abs(q_np - value).max()
        assert err_q < Q_ABS
    else:
        # the same forward as rl4rs_policy_greedy's GEMM path: the same bits
        a_g, row_g = pol.greedy(o, b, want_q=True)
        assert torch.equal(a, a_g) and torch.equal(out, row_g)
        err_q = 0.0
        assert np.array_equal(q_np, m[rows, a_np].astype(np.float64))
    assert np.array_equal(a_np, m.argmax(axis=1)) and a_np[3] == 0
    pi_ref = np.exp(OP.log_softmax(logits))[rows, logged]
    legal = ok[rows, logged]
    legal[3] = True                                          # the row that allows nothing is uniform in both
    err_pi = _rel(pi_np[legal], pi_ref[legal])
    err_own = _rel(pi_np, _softmax64(m)[rows, logged])
    print('od %d hid %d A %d N %d q_mode %d: logit err %.3g (bar %.0e)  q err %.3g (bar %.0e)  pi rel err %.3g (bar %.0e)  '
          'pi vs its own row %.3g (bar 1e-12)' % (od, hid, A, N, q_mode, err_l, Q_ABS, err_q, Q_ABS, err_pi, PI_RTOL, err_own))
    assert err_pi <= PI_RTOL
    assert (pi_np[~legal] == 0.0).all() and pi_np[5] == 0.0
    assert err_own <= 1e-12
    with pytest.raises(Rl4rsHipError, match='max_rows'):
        pol.ope_step(torch.cat([o, o[:1]]), torch.cat([b, b[:1]]), torch.cat([lg, lg[:1]]), q_mode)
    pol.close()


# ---- 3. policy_model over the online trainers --------------------------------------------------------------------------
def _cfg(d, B=64, T=9, **extra):
    from rl4rs_amd import synth
    text = synth.make_catalog_text(seed=4)
    synth.write_text(os.path.join(d, 'c.csv'), text)
    recs = synth.make_records(300, seed=2, hash_size=2000, special_ids=synth.special_ids_from_text(text))
    synth.write_records(os.path.join(d, 'log.csv'), recs)
    cfg = {"maxlen": 64, "batch_size": B, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
           "category_feature_num": 21, "category_hash_size": 2000, "seq_num": 2, "emb_size": 128, "page_items": 9,
           "hidden_units": 128, "max_steps": T, "action_emb_size": 32, "sample_file": os.path.join(d, 'log.csv'),
           "iteminfo_file": os.path.join(d, 'c.csv'), "cache_size": 256, "model_seed": 3, "return_tensors": True}
    cfg.update(extra)
    return cfg


def _env(cfg):
    """the synthetic 64 x 9 SlateRecEnv of tests/test_gpu_dqn.py::_env"""
    import rl4rs_amd
    from rl4rs_amd.env.slate import SlateRecEnv, SlateState
    return rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))


def _trainer(kind, env):
    from rl4rs_amd import train as T
    if kind in ('A2C', 'PPO'):
        return T.Trainer(env, kind, seed=3, init_seed=9)
    if kind == 'DQN':
        return T.DQNTrainer(env, seed=3, init_seed=9, learning_starts=env.config['batch_size'] * 9, train_batch_size=256)
    return T.RainbowTrainer(env, seed=3, init_seed=9, learning_starts=576, train_batch_size=256, masked=kind == 'RAINBOW-masked')


@pytest.mark.parametrize('kind', ['A2C', 'DQN', 'RAINBOW', 'RAINBOW-masked'])
def test_policy_model_over_a_trainer(tmp_path, kind):
    import torch
    from rl4rs_amd.policy.policy_model import policy_model
    cfg = _cfg(str(tmp_path))
    env = _env(cfg)
    env.seed(7)
    tr = _trainer(kind, env)
    for _ in range(2):
        tr.train_iteration()
    tr.params()
    masked, has_q = kind != 'RAINBOW', kind != 'A2C'
    obs = env.reset().clone()
    B, A = obs.shape[0], 284
    bits = env.samples._live().obs_mask_bits().clone()
    allowed = torch.from_numpy(_unpack(bits.cpu().numpy(), A)).cuda()
    assert 0 < int(allowed.sum()) < B * A
    a_ref, row = tr.policy.greedy(obs, bits if masked else None, want_q=True)
    pm = policy_model(tr, cfg, env=env)
    a = pm.predict_with_mask(obs)
    assert a.is_cuda and a.dtype == torch.int64 and torch.equal(a, a_ref.long()) and torch.equal(pm.predict(obs), a)
    if masked:
        assert allowed[torch.arange(B), a].all()
    p = pm.action_probs(obs)
    assert p.is_cuda and p.dtype == torch.float32 and tuple(p.shape) == (B, A)
    assert (p.sum(dim=1) - 1).abs().max().item() < 1e-5
    assert torch.equal(p, torch.softmax(row, dim=1))
    if masked:
        assert (p[~allowed] == 0).all()
    q = pm.predict_q(obs, a)
    assert q.is_cuda and q.dtype == torch.float32 and tuple(q.shape) == (B,)
    if has_q:
        assert torch.equal(q, row[torch.arange(B), a])
        other = torch.randint(0, A, (B,), device='cuda')
        assert torch.equal(pm.predict_q(obs, other), row[torch.arange(B), other])
    else:
        # the value head: the handle's own number, and rl4rs_policy_evaluate's within twice the 1e-5 each forward is held to
        assert torch.equal(q.double(), tr.policy.ope_step(obs, bits, None, 0)[2])
        assert (q - tr.policy.evaluate(obs, a.int(), bits)[1]).abs().max().item() < 2 * Q_ABS
    # numpy in, numpy out
    obs_h = obs.cpu().numpy()
    for got, want in ((pm.predict_with_mask(obs_h), a), (pm.action_probs(obs_h), p), (pm.predict_q(obs_h, a.cpu().numpy()), q)):
        assert isinstance(got, np.ndarray) and np.array_equal(got, want.cpu().numpy())
    # the support_rllib_mask dict observation carries the mask itself: the same results without an env
    pm_d = policy_model(tr, cfg)
    d = {'obs': obs, 'action_mask': allowed.long()}
    assert torch.equal(pm_d.predict_with_mask(d), a) and torch.equal(pm_d.action_probs(d), p) and torch.equal(pm_d.predict_q(d, a), q)
    d_h = [{'obs': o, 'action_mask': m} for o, m in zip(obs_h, allowed.long().cpu().numpy())]
    assert np.array_equal(pm_d.predict_with_mask(d_h), a.cpu().numpy())
    if masked:
        with pytest.raises(ValueError, match='action mask'):
            pm_d.predict_with_mask(obs)
    else:
        assert torch.equal(pm_d.predict_with_mask(obs), a)
    # more rows than the handle takes at once: chunked
    reps = tr.policy.max_rows // B + 1
    big = {'obs': obs.repeat(reps, 1), 'action_mask': allowed.long().repeat(reps, 1)}
    assert big['obs'].shape[0] > tr.policy.max_rows
    assert torch.equal(pm_d.predict_with_mask(big), a.repeat(reps)) and torch.equal(pm_d.action_probs(big), p.repeat(reps, 1))
    assert torch.equal(pm_d.predict_q(big, a.repeat(reps)), q.repeat(reps))
    tr.close()


# ---- 4. ope_eval with a trainer ----------------------------------------------------------------------------------------
class _Behaviour(object):
    """a seeded callable: positive [B, 284] scores from the observation (host or device)"""

    def __init__(self, seed):
        import torch
        self.w = torch.from_numpy((np.random.RandomState(seed).randn(256, 284) * 0.05).astype(np.float32)).cuda()

    def __call__(self, obs):
        import torch
        x = obs if isinstance(obs, torch.Tensor) else torch.from_numpy(np.asarray(obs, dtype=np.float32))
        return torch.exp(x.to(device='cuda', dtype=torch.float32) @ self.w)


def _collect(columns):
    def on_epoch(epoch, log, actions, offline_actions):
        import torch
        host = lambda v: v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        cols = dict((name, log.column(name).cpu().numpy()) for name in ('pi', 'mu', 'q', 'reward', 'logged_reward'))
        cols['action'] = np.stack([host(a) for a in actions])
        cols['offline_action'] = np.stack([host(a).astype(np.int64) for a in offline_actions])
        assert epoch == len(columns)
        columns.append(cols)
    return on_epoch


@pytest.mark.parametrize('kind', ['PPO', 'DQN'])
def test_ope_eval_with_a_trainer_end_to_end(tmp_path, kind):
    import torch
    from test_gpu_ope import _array_path, _close
    from rl4rs_amd.ope import ope_eval
    from rl4rs_amd.policy.behavior_model import behavior_model
    from rl4rs_amd.policy.policy_model import policy_model
    cfg = _cfg(str(tmp_path), B=96, epoch=2, is_eval=True, cache_size=96)
    B, T = 96, 9
    train_env = _env(dict(cfg, is_eval=False))
    train_env.seed(7)
    tr = _trainer(kind, train_env)
    tr.train_iteration()
    tr.params()
    sample_model = behavior_model(cfg, _Behaviour(5))
    sample_model.takes_observation = True                   # it reads the observation the policy reads, not the raw records
    assert not sample_model.logits
    columns = []
    out = ope_eval(cfg, _env(cfg), tr, sample_model=sample_model, on_epoch=_collect(columns))
    assert out['metrics'].shape == (2, 4, 2) and len(columns) == 2
    assert np.isfinite(out['metrics']).all(), out['metrics']
    # (a) the metrics are the array functions on the log's columns, bit for bit
    for e in range(2):
        s = _array_path(columns[e], 1.0)
        want = np.array([(s['cips'], s['cips_c']), (s['dr'], s['dr_se']), (s['wips'], s['wips_2']), (s['seqdr'], s['seqdr_2'])])
        assert out['metrics'][e].tobytes() == want.tobytes(), (e, out['metrics'][e], want)
        assert out['stats'][e]['sim_reward'] == s['sim_reward']
    # (b) the columns are what the three policy_model methods return, called the reference's way on the same episodes
    env = _env(cfg)
    pm = policy_model(tr, cfg, env=env)
    for e in range(2):
        cols = columns[e]
        obs = env.reset()
        for j in range(T):
            action = pm.predict_with_mask(obs)
            off = env.offline_action
            pi = pm.action_probs(obs)[torch.arange(B), off.long()].cpu().numpy()
            q = pm.predict_q(obs, action).cpu().numpy()
            obs, reward, done, info = env.step(action)
            logged = env.offline_reward
            logged = logged.cpu().numpy() if isinstance(logged, torch.Tensor) else np.asarray(logged, dtype=np.float64)
            assert np.array_equal(cols['action'][j], action.cpu().numpy()), (e, j)
            assert np.array_equal(cols['offline_action'][j], off.cpu().numpy().astype(np.int64)), (e, j)
            assert np.array_equal(cols['reward'][j], reward.cpu().numpy().astype(np.float64)), (e, j)
            assert np.array_equal(cols['logged_reward'][j], logged), (e, j)
            _close(cols['pi'][j], pi, 1e-5, 'pi epoch %d step %d' % (e, j))
            _close(cols['q'][j], q, 1e-5, 'q epoch %d step %d' % (e, j))
    # (c) host observations (return_tensors off): the three methods fill the same columns
    host_columns = []
    out_h = ope_eval(cfg, _env(dict(cfg, return_tensors=False)), tr, sample_model=sample_model, on_epoch=_collect(host_columns))
    assert np.isfinite(out_h['metrics']).all()
    for e in range(2):
        assert np.array_equal(host_columns[e]['action'], columns[e]['action'])
        for name in ('pi', 'mu', 'q', 'reward', 'logged_reward'):
            _close(host_columns[e][name], columns[e][name], 1e-5, '%s epoch %d (host observations)' % (name, e))
    tr.close()
