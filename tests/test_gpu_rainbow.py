"""GPU: the on-device Rainbow (rl4rs_distq_*: fused dueling / distributional head, categorical loss kernels, n-step replay draw,
RainbowTrainer) against the float64 restatement in tests/rainbow_ref.py.

Error bars.  The net is four layers deep and Q is scaled by up to v_max = 1000, so the two-layer policy's 1e-5 does not carry over.
The yardstick is an fp32 eager-torch CPU forward / backward of the restatement against the float64 restatement on these very
inputs (rainbow_ref.fp32_yardstick, a reference implementation, not the code under test); every bar is 4 x the measured value (the
accumulation order differs between implementations).  Measured max errors and bars per shape (od, A, atoms, N, dueling, double_q,
masked), the gradient relative to the reference gradient's max-norm:

    shape                            Q measured / bar      td measured / bar     gradient measured / bar
    (256, 284,  8, 1024, 1, 1, 0)    2.84e-4 / 1.14e-3     1.10e-6 / 4.40e-6     8.29e-8 / 3.32e-7
    (256, 284,  8, 1003, 1, 1, 1)    3.17e-4 / 1.27e-3     8.91e-7 / 3.56e-6     7.33e-8 / 2.93e-7
    (256,  50,  5,  517, 1, 0, 0)    2.68e-6 / 1.07e-5     9.95e-7 / 3.98e-6     2.05e-7 / 8.20e-7
    (100,  75, 51,  333, 0, 1, 1)    5.92e-7 / 2.37e-6     9.88e-7 / 3.95e-6     1.13e-6 / 4.52e-6
    (256, 284,  2,   77, 1, 1, 0)    3.78e-4 / 1.51e-3     4.30e-7 / 1.72e-6     4.25e-7 / 1.70e-6

(rainbow_ref.MEASURED holds the same numbers.)  The first, second and last shape use the reference's support [0, 1000], the other
two [-2, 6]; gamma^n is 1 except 0.5 on the 51-atom shape.  An integer a* / greedy action is compared on every row whose float64
top-two Q gap is at least ten times the Q bar; at most 1 % of the rows may fall under it, which tests/test_rainbow_host.py confirms
on the CPU with the restatement alone.  A SoftQ draw is compared on every row whose u is farther from a CDF edge than
rainbow_ref.softq_edge_bar (derived there from the Q bar).  The loss is not differentiable where a relu unit's pre-activation is 0
and fp32 may put a value within its rounding of 0 on either side, so the inputs keep every stream pre-activation of s at least
rainbow_ref.RELU_MARGIN = 1e-5 away from 0 (more than 4 x the 1.9e-6 fp32 error of those pre-activations; checked on the CPU)."""
import functools
import os

import numpy as np
import pytest

import rainbow_gpu as G
import rainbow_ref as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(i):
    """(inputs, float64 reference without teacher forcing) of shape i: computed once, shared, never modified."""
    c = R.make_case(R.GPU_SHAPES[i], R.CASE_SEEDS[i])
    return c, G.reference(c)


def _bars(i):
    return G.bars_of(R.MEASURED[i])


@pytest.mark.parametrize('i', range(len(R.GPU_SHAPES)))
def test_loss_and_gradient_match_the_restatement(i):
    c, ref0 = _case(i)
    G.check_loss_and_gradient(c, ref0, _bars(i))


@pytest.mark.parametrize('i', [1, 2])
def test_dueling_gradient_sums_to_zero_over_the_actions(i):
    """tests/rainbow_gpu.py, check_dueling_gradient_sums_to_zero: the advantage head's gradients sum to zero over the actions."""
    c, ref0 = _case(i)
    G.check_dueling_gradient_sums_to_zero(c, ref0)


@pytest.mark.parametrize('i,temperature', [(1, 1.0), (2, 1.0), (3, 2.0)])
def test_acting_softq_draw_and_greedy(i, temperature):
    c, _ = _case(i)
    G.check_acting(c, _bars(i)[0], temperature)


# ---- n-step sampling --------------------------------------------------------------------------------------------------------
def _rollout(rs, T, B, od, A):
    import torch
    n = T * B
    obs = rs.randn(n, od).astype(np.float32)
    mask = (rs.rand(n, A) < 0.5).astype(np.int64)
    mask[:, 0] = 1
    act = rs.randint(0, A, size=n).astype(np.int32)
    rew = rs.randint(-3, 8, size=n).astype(np.float64)                          # small integers: every float sum is exact
    host = dict(obs=obs, mask=R.pack_bits(mask), act=act, rew=rew)
    return host, dict((k, torch.from_numpy(v).cuda()) for k, v in host.items())


@pytest.mark.parametrize('T,B,n_step,gamma', [(9, 8, 3, 1.0), (9, 8, 3, 0.5), (2, 8, 3, 1.0)])
def test_nstep_sample_matches_the_row_rule(T, B, n_step, gamma):
    from rl4rs_amd.device import DeviceReplay
    od, A, M = 12, 40, 300
    rs = np.random.RandomState(T + n_step)
    rp = DeviceReplay(od, A, T, B, buffer_size=2 * T * B, alpha=0.6)
    hosts = []
    for _ in range(2):
        h, d = _rollout(rs, T, B, od, A)
        rp.push(d['obs'], d['mask'], d['act'], d['rew'])
        hosts.append(h)
    ring = dict((k, np.concatenate([h[k] for h in hosts])) for k in hosts[0])
    for prioritized in (False, True):
        b = rp.sample(M, prioritized=prioritized, beta=0.4, seed=3, step=1, n_step=n_step, gamma=gamma)
        b = dict((k, v.cpu().numpy()) for k, v in b.items() if v is not None)
        idx = b['idx'].astype(np.int64)
        assert len(set(idx.tolist())) > 30
        Rn, done, succ, k = R.nstep_row(idx, ring['rew'], T, B, n_step, gamma)
        assert np.array_equal(b['reward'], Rn.astype(np.float32)) and np.array_equal(b['done'] != 0, done)
        assert np.array_equal(b['obs'], ring['obs'][idx]) and np.array_equal(b['action'], ring['act'][idx])
        nd = ~done
        assert np.array_equal(b['next_obs'][nd], ring['obs'][succ[nd]]) and np.array_equal(b['next_mask'][nd], ring['mask'][succ[nd]])
        assert np.isfinite(b['next_obs']).all()
        if T == 2:
            assert done.all()


@pytest.mark.parametrize('prioritized', [False, True])
def test_nstep_one_is_the_plain_sample(prioritized):
    import torch
    from rl4rs_amd.device import DeviceReplay, check, _ptr, _stream
    T, B, od, A, M = 9, 8, 12, 40, 257
    rs = np.random.RandomState(8)
    rp = DeviceReplay(od, A, T, B, buffer_size=2 * T * B, alpha=0.6)
    for _ in range(2):
        d = _rollout(rs, T, B, od, A)[1]
        rp.push(d['obs'], d['mask'], d['act'], d['rew'])
    rp.set_priorities(torch.from_numpy(rs.rand(2 * T * B) * 3.0 + 0.01))
    plain = rp.sample(M, prioritized=prioritized, beta=0.4, seed=5, step=2, want_u=True)
    b = rp.new_batch(M, want_u=True)
    for v in b.values():
        v.fill_(7)
    check(rp.lib.rl4rs_replay_sample_nstep(rp.h, M, 1, 0.9, 1 if prioritized else 0, 0.4, 5, 2, _ptr(b['obs']), _ptr(b['next_obs']),
                                           _ptr(b['next_mask']), _ptr(b['action']), _ptr(b['reward']), _ptr(b['done']), _ptr(b['idx']),
                                           _ptr(b['weight']), _ptr(b['u']), _stream()))
    for k in plain:
        assert torch.equal(plain[k], b[k]), k


# ---- trainer ----------------------------------------------------------------------------------------------------------------
def _env(d, B=8, T=9):
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
    """Three train calls of two updates each against a host loop built from the restatement and fed the device's own sampled rows,
    weights and a*: parameters to the 2e-5 of tests/test_gpu_dqn.py's Adam bar; the target copy happens on schedule."""
    import torch
    from rl4rs_amd.train import RainbowTrainer
    env = _env(str(tmp_path))
    env.seed(7)
    with pytest.raises(ValueError):
        RainbowTrainer(env, noisy=True)
    tr = RainbowTrainer(env, seed=3, init_seed=9, learning_starts=0, updates_per_rollout=2, buffer_size=144,
                        target_network_update_freq=144, keep_last_batch=True)
    assert tr.M == 72 and tr.n_step == 3 and tr.gamma_n == 1.0 and not tr.masked
    dm = R.Dims()
    flat = tr.params().cpu().numpy().astype(np.float64)
    assert len(flat) == dm.n_params()
    state = (flat, np.zeros_like(flat), np.zeros_like(flat), 0)
    target = flat.copy()
    seen = []
    inner = tr.update

    def recording_update():
        stats = inner()
        seen.append((dict((k, v.cpu().numpy()) for k, v in tr.last_batch.items()), tr.policy.params().cpu().numpy()))
        return stats

    tr.update = recording_update
    syncs = 0
    for it in range(3):
        st = tr.train_iteration()
        assert len(seen) == 2 * (it + 1)
        rew_ring = tr.replay.column('reward').cpu().numpy()
        for lb, got in seen[-2:]:
            assert lb['idx'].max() < min(it + 1, 2) * 72
            Rn, done, succ, _ = R.nstep_row(lb['idx'], rew_ring, 9, 8, 3, 1.0)
            assert np.array_equal(lb['reward'], Rn.astype(np.float32)) and np.array_equal(lb['done'] != 0, done)
            out = R.loss_and_grad(state[0], target, lb['obs'], lb['action'], lb['reward'], lb['done'], lb['next_obs'], None, lb['weight'],
                                  1.0, True, dm, astar=lb['next_action'])
            state = R.adam_clip_by_var(state[0], state[1], state[2], state[3], out['grad'], 5e-4, 40.0, dm)
            err = np.abs(got - state[0]).max()
            print('iteration %d: parameter err %.3g (bar 2e-5)' % (it, err))
            assert err < 2e-5, (it, err)
        assert abs(st['td_loss'] - out['loss']) < 1e-5 + 2e-3 * abs(out['loss'])
        assert abs(st['mean_q'] - out['qsa'].mean()) < 4.0 * R.MEASURED[0]['q'] + 1e-6 * abs(out['qsa'].mean())
        assert st['num_updates'] == 2 * (it + 1) and st['iteration'] == it + 1 and st['buffer_rows'] == min(it + 1, 2) * 72
        if st['num_target_updates'] != syncs:                               # the device copied online -> target after these updates
            syncs = st['num_target_updates']
            target = state[0].copy()
            assert torch.equal(tr.target, tr.policy.params())
        else:
            assert not torch.equal(tr.target, tr.policy.params())
    assert syncs == 1                                                       # 72, 144 (copy), 216 sampled steps at a frequency of 144


def test_trainer_evaluate_is_deterministic_and_the_mask_knob_plays_legal_actions(tmp_path):
    from rl4rs_amd.train import RainbowTrainer
    env = _env(str(tmp_path))
    env.seed(5)
    tr = RainbowTrainer(env, seed=2, init_seed=4, learning_starts=0, masked=True, num_atoms=5, v_min=-2.0, v_max=6.0, dueling=False,
                        n_step=2, gamma=0.9, train_batch_size=64)
    e0 = tr.evaluate(episodes=16, seed=11)
    assert e0 == tr.evaluate(episodes=16, seed=11)
    for _ in range(2):
        st = tr.train_iteration()
    assert st['num_updates'] == 2 and np.isfinite(list(st.values())).all() and st['td_loss'] > 0
    assert env.samples.get_violation().all()               # SoftQ over the masked Q only ever plays legal actions
    e1 = tr.evaluate(episodes=16, seed=11)
    assert e1 == tr.evaluate(episodes=16, seed=11)
