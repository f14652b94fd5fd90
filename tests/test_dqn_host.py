"""CPU: the float64 DQN restatement the GPU tests compare against (tests/dqn_ref.py) is itself checked here - its hand-written
gradient against torch float64 autograd of the same loss, the prioritized sampler, weight formula and duplicate-index rule on
hand-made cases, the ring's successor / eviction arithmetic - and the C ABI declares, exports and binds the new entry points."""
import os
import re

import numpy as np
import pytest

import dqn_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DQN_SYMBOLS = ('rl4rs_replay_create', 'rl4rs_replay_destroy', 'rl4rs_replay_rows', 'rl4rs_replay_buffer', 'rl4rs_replay_push',
               'rl4rs_replay_sample', 'rl4rs_replay_update_priorities', 'rl4rs_policy_dqn_loss_grad', 'rl4rs_policy_greedy',
               'rl4rs_policy_adam_step_clip_by_var')


def _case(rs, N, od, hid, A, all_masked_row=True):
    from rl4rs_amd.nets.policy import init_policy_params, param_count
    n = param_count(od, hid, A)
    flat = init_policy_params(od, hid, A, seed=1).astype(np.float64) + rs.randn(n) * 0.05
    tflat = flat + rs.randn(n) * 0.02
    obs, nobs = rs.randn(N, od), rs.randn(N, od)
    mask = (rs.rand(N, A) < 0.4).astype(np.float64)
    mask[np.arange(N), rs.randint(0, A, size=N)] = 1
    done = rs.rand(N) < 0.15
    if all_masked_row:
        k = int(np.nonzero(~done)[0][0])
        mask[k] = 0                         # a non-terminal successor that allows nothing
    act = rs.randint(0, A, size=N)
    rew = rs.randn(N) * 2.0                 # |td| on both sides of the Huber knee
    w = rs.rand(N) + 0.1
    return flat, tflat, obs, act, rew, done, nobs, mask, w


@pytest.mark.parametrize('double_q', [True, False])
@pytest.mark.parametrize('weighted', [True, False])
def test_restatement_gradient_equals_float64_autograd(double_q, weighted):
    od, hid, A, N = 24, 16, 37, 200
    rs = np.random.RandomState(3 + 2 * double_q + weighted)
    flat, tflat, obs, act, rew, done, nobs, mask, w = _case(rs, N, od, hid, A)
    nobs[done] = np.nan                     # a terminal row's successor is never read
    ww = w if weighted else None
    out = R.dqn_loss_and_grad(flat, tflat, obs, act, rew, done, nobs, mask, ww, gamma=0.9, double_q=double_q, od=od, hid=hid, A=A)
    assert done.any() and (~out['boot'] & ~done).sum() == 1
    assert np.isfinite(out['grad']).all() and np.isfinite(out['loss'])
    assert (np.abs(out['td']) < 1).any() and (np.abs(out['td']) > 1).any()
    # targets by hand: r on terminal and no-legal-action rows, r + gamma * Q_target(s')[a*] elsewhere
    from oracle import policy as OP
    q_sel = OP.forward(flat if double_q else tflat, np.nan_to_num(nobs), mask, od, hid, A)[0]
    q_t = OP.forward(tflat, np.nan_to_num(nobs), None, od, hid, A)[0]
    a = q_sel.argmax(1)
    y = np.where(out['boot'], rew + 0.9 * q_t[np.arange(N), a], rew)
    assert np.array_equal(a[out['boot']], out['astar'][out['boot']])
    assert np.allclose(out['y'], y, rtol=0, atol=1e-13)
    loss, grad = R.dqn_loss_autograd(flat, out['y'], obs, act, ww, od, hid, A)
    assert abs(loss - out['loss']) <= 1e-10 * abs(loss)
    assert np.abs(grad - out['grad']).max() <= 1e-10 * np.abs(grad).max()
    # the value head's column gets exactly nothing
    gW2 = out['grad'][od * hid + hid:od * hid + hid + hid * (A + 1)].reshape(hid, A + 1)
    assert (gW2[:, A] == 0).all() and out['grad'][-1] == 0


def test_teacher_forced_next_action_only_touches_bootstrapping_rows():
    od, hid, A, N = 24, 16, 37, 64
    rs = np.random.RandomState(11)
    flat, tflat, obs, act, rew, done, nobs, mask, w = _case(rs, N, od, hid, A)
    base = R.dqn_loss_and_grad(flat, tflat, obs, act, rew, done, nobs, mask, w, od=od, hid=hid, A=A)
    forced = np.full(N, -1)
    forced[base['boot']] = base['astar'][base['boot']]
    again = R.dqn_loss_and_grad(flat, tflat, obs, act, rew, done, nobs, mask, w, od=od, hid=hid, A=A, astar=forced)
    assert np.array_equal(base['grad'], again['grad'])
    other = forced.copy()
    k = int(np.nonzero(base['boot'])[0][0])
    other[k] = (other[k] + 1) % A
    assert R.dqn_loss_and_grad(flat, tflat, obs, act, rew, done, nobs, mask, w, od=od, hid=hid, A=A, astar=other)['y'][k] != base['y'][k]


def test_prioritized_selection_on_hand_made_priorities():
    prio = np.array([1.0, 3.0, 0.5, 0.5, 5.0])           # prefix 1, 4, 4.5, 5, 10
    u = np.array([0.0, 0.05, 0.1, 0.25, 0.3999, 0.4, 0.449, 0.45, 0.5, 0.75, 0.999999])
    idx, dist, total = R.prioritized_select(prio, u)
    assert total == 10.0
    # mass 1.0 (u = 0.1) is NOT below prefix[0] = 1: "exceeds" is strict, so it belongs to row 1
    assert idx.tolist() == [0, 0, 1, 1, 1, 2, 2, 3, 4, 4, 4]
    assert dist[2] == 0.0 and abs(dist[1] - 0.5) < 1e-15
    # explicit definition
    c = np.cumsum(prio)
    for ui, i in zip(u, idx):
        assert i == next(k for k in range(5) if c[k] > ui * 10.0)
    assert R.uniform_select(np.array([0.0, 0.1999, 0.2, 0.999999]), 5).tolist() == [0, 0, 1, 4]


def test_importance_weights_formula():
    prio = np.array([1.0, 3.0, 0.5, 0.5, 5.0])
    w = R.is_weights(prio, np.array([0, 1, 2, 4]), beta=0.4)
    # (p_i / p_min)^-beta: the smallest priority has weight 1, larger ones less
    assert np.allclose(w, (np.array([1.0, 3.0, 0.5, 5.0]) / 0.5) ** -0.4, rtol=1e-14)
    assert w[2] == 1.0 and (w <= 1.0).all()
    assert np.allclose(R.is_weights(prio, np.arange(5), beta=0.0), 1.0)


def test_duplicate_indices_keep_the_highest_batch_position():
    prio = np.ones(6)
    idx = np.array([2, 4, 2, 5, 2, 4])
    td = np.array([0.5, -3.0, 7.0, 0.0, -0.25, 1.0])
    new, mx = R.update_priorities(prio, 1.0, idx, td, alpha=0.6)
    assert new[2] == (0.25 + 1e-6) ** 0.6 and new[4] == (1.0 + 1e-6) ** 0.6 and new[5] == 1e-6 ** 0.6
    assert new[0] == new[1] == new[3] == 1.0
    assert mx == 7.0 + 1e-6                                # a losing duplicate still raises max_priority
    assert R.update_priorities(prio, 9.0, idx, td, alpha=0.6)[1] == 9.0


def test_ring_successor_and_eviction_arithmetic():
    T, B = 3, 4
    assert R.capacity_rollouts(100000, 9, 64) == 173 and R.capacity_rollouts(10, T, B) == 1 and R.capacity_rollouts(25, T, B) == 2
    assert [R.slot_of_push(k, 25, T, B) for k in range(5)] == [0, 1, 0, 1, 0]          # push 2 evicts rollout 0 whole
    assert [R.filled_rows(k, 25, T, B) for k in range(4)] == [0, 12, 24, 24]
    slot, t, b, done, nxt = R.row_fields(np.arange(24), T, B)
    assert slot.tolist() == [0] * 12 + [1] * 12
    assert t[:12].tolist() == [0] * 4 + [1] * 4 + [2] * 4 and b[:8].tolist() == [0, 1, 2, 3] * 2
    assert done.tolist() == ([False] * 8 + [True] * 4) * 2
    live = ~done
    assert (nxt[live] == np.arange(24)[live] + B).all() and (nxt[done] == -1).all()
    # a successor never leaves its rollout
    assert (R.row_fields(nxt[live], T, B)[0] == slot[live]).all() and (R.row_fields(nxt[live], T, B)[2] == b[live]).all()


def test_adam_clip_by_var_clips_each_variable_by_its_own_norm():
    od, hid, A = 4, 3, 5
    n = od * hid + hid + hid * (A + 1) + (A + 1)
    g = np.concatenate([np.full(od * hid, 10.0), np.full(hid, 0.1), np.full(hid * (A + 1), -20.0), np.full(A + 1, 0.01)])
    flat, m, v, t = R.adam_clip_by_var(np.zeros(n), np.zeros(n), np.zeros(n), 0, g, lr=1e-3, var_clip=2.0, od=od, hid=hid, A=A)
    assert t == 1
    # m = 0.1 * clipped gradient: W1 and W2e clipped to norm 2, the biases untouched
    assert np.isclose(np.sqrt(((m[:12] / 0.1) ** 2).sum()), 2.0) and np.allclose(m[12:15] / 0.1, 0.1)
    assert np.isclose(np.sqrt(((m[15:33] / 0.1) ** 2).sum()), 2.0) and np.allclose(m[33:] / 0.1, 0.01)


def test_dqn_symbols_are_declared_exported_and_bound():
    """FAILS on a tree without the feature: the header, the built library and the ctypes table all carry the new entry points."""
    from rl4rs_amd.build import build_lib
    build_lib()
    from rl4rs_amd import _lib
    lib = _lib.load()
    text = open(os.path.join(REPO, 'include', 'rl4rs_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(rl4rs_[a-z0-9_]+)\s*\(', text))
    for name in DQN_SYMBOLS:
        assert name in declared, 'include/rl4rs_hip.h does not declare %s' % name
        assert hasattr(lib, name), 'the library does not export %s' % name
        assert name in _lib.SIGNATURES, '_lib.SIGNATURES does not bind %s' % name
    assert lib.rl4rs_abi_version() == 1
    from rl4rs_amd.train import DQNTrainer, Trainer          # exported like Trainer
    assert DQNTrainer is not Trainer
