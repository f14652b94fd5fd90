"""CPU: the float64 restatement of the on-device Rainbow (tests/rainbow_ref.py) against torch float64 autograd, the categorical
projection on a hand-made case, the n-step row rule, the inputs of the GPU tests (how many rows their near-tie bars leave out), and
the new symbols of the C ABI."""
import os
import re

import numpy as np
import pytest

import rainbow_ref as R
import td3_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('dueling,weighted,double_q', [(True, True, True), (True, False, False), (False, True, True), (False, False, True)])
def test_hand_written_gradient_equals_float64_autograd(dueling, weighted, double_q):
    rs = np.random.RandomState(5 + 2 * dueling + weighted)
    dm = R.Dims(od=24, A=13, atoms=6, trunk=32, sh=32, dueling=dueling, v_min=-1.0, v_max=4.0)
    N = 41
    flat, tflat = rs.randn(dm.n_params()) * 0.2, rs.randn(dm.n_params()) * 0.2
    obs, nobs = rs.randn(N, 24), rs.randn(N, 24)
    mask = (rs.rand(N, 13) < 0.5).astype(np.int64)
    mask[:, 3] = 1
    done = (rs.rand(N) < 0.2).astype(np.int32)
    act = rs.randint(0, 13, size=N)
    rew = rs.randn(N) * 2.0
    rew[:6] = [0.0, 1.0, 9.0, -7.0, 2.0, 0.5]
    w = rs.rand(N) + 0.1 if weighted else None
    out = R.loss_and_grad(flat, tflat, obs, act, rew, done, nobs, mask, w, 0.9 ** 3, double_q, dm)
    assert np.abs(out['m'].sum(axis=1) - 1.0).max() < 1e-12 and (out['m'] >= 0).all()
    loss, grad, td, qsa = R.loss_autograd(flat, out['m'], obs, act, w, dm)
    assert abs(loss - out['loss']) < 1e-12
    assert np.abs(td - out['td']).max() < 1e-12 and np.abs(qsa - out['qsa']).max() < 1e-12
    assert np.abs(grad - out['grad']).max() < 1e-12 * max(1.0, np.abs(grad).max())
    assert np.abs(grad).max() > 1e-4
    if dueling:       # the dueling head's structural zero: the advantage gradients of every atom sum to zero over the actions
        gWa2 = R.split(out['grad'], dm)['Wa2'].reshape(dm.sh, dm.A, dm.atoms)
        assert np.abs(gWa2.sum(axis=1)).max() < 1e-14


def test_projection_on_a_hand_made_case():
    dm = R.Dims(od=4, A=3, atoms=5, trunk=32, sh=32, v_min=0.0, v_max=8.0)           # z = 0, 2, 4, 6, 8
    p = np.array([[0.1, 0.2, 0.3, 0.25, 0.15]] * 6)
    R_ = np.array([2.0, 1.0, 100.0, -50.0, 3.0, 3.0])
    boot = np.array([True, True, True, True, False, True])
    p[4] = np.nan                                                                      # the done row's successor is not read
    m = R.project(R_, boot, p, 1.0, dm)
    assert np.abs(m.sum(axis=1) - 1.0).max() < 1e-12
    # row 0: b_j = j + 1 exactly (the eq branch): every atom moves one up, the top two pile up on the last
    assert np.allclose(m[0], [0.0, 0.1, 0.2, 0.3, 0.4], atol=1e-15)
    # row 1: b_j = j + 0.5: halves to the neighbours; j = 4 clips to b = 4 (eq)
    assert np.allclose(m[1], [0.05, 0.05 + 0.1, 0.1 + 0.15, 0.15 + 0.125, 0.125 + 0.15], atol=1e-15)
    assert np.allclose(m[2], [0, 0, 0, 0, 1.0], atol=1e-15)                           # clips at v_max
    assert np.allclose(m[3], [1.0, 0, 0, 0, 0], atol=1e-15)                           # clips at v_min
    assert np.allclose(m[4], [0, 0.5, 0.5, 0, 0], atol=1e-15)                         # done: the point R = 3 between z_1 and z_2
    # without the eq term the integer rows lose their whole mass
    assert m[0].sum() > 0.99
    # the fp32 form of the same arithmetic agrees
    assert np.abs(R.project(R_, boot, p, 1.0, dm, dtype=np.float32) - m).max() < 1e-6


def test_nstep_arithmetic():
    T, B, n = 9, 4, 3
    rew = np.arange(2 * T * B, dtype=np.float64) % 7
    idx = np.arange(2 * T * B)
    Rn, done, succ, k = R.nstep_row(idx, rew, T, B, n, 0.5)
    t = (idx % (T * B)) // B
    assert np.array_equal(k, np.minimum(3, 9 - t)) and np.array_equal(done, t >= 6)
    assert np.array_equal(succ[~done], idx[~done] + 3 * B) and (succ[done] == -1).all()
    i = 5 * B + 2                                           # t = 5: three terms
    assert Rn[i] == rew[i] + 0.5 * rew[i + B] + 0.25 * rew[i + 2 * B]
    i = T * B + 8 * B + 1                                   # second rollout, t = 8: one term
    assert Rn[i] == rew[i] and done[i]
    # T = 2, n = 3: every row is done; t = 0 sums two rewards, t = 1 one
    T, B = 2, 3
    rew = np.array([1.0, 2.0, 3.0, 10.0, 20.0, 30.0])
    Rn, done, succ, k = R.nstep_row(np.arange(6), rew, T, B, 3, 1.0)
    assert done.all() and (succ == -1).all() and np.array_equal(k, [2, 2, 2, 1, 1, 1])
    assert np.array_equal(Rn, [11.0, 22.0, 33.0, 10.0, 20.0, 30.0])


@pytest.mark.parametrize('i', range(len(R.GPU_SHAPES)))
def test_gpu_cases_leave_at_most_one_percent_of_rows_to_near_ties(i):
    """The inputs of tests/test_gpu_rainbow.py, with the restatement alone: integer b on a tenth of the rows at least, rewards past
    both ends of the support, and at most 1 % of the bootstrapping rows under the a* gap bar."""
    c = R.make_case(R.GPU_SHAPES[i], R.CASE_SEEDS[i])
    dm = c['dm']
    ref = R.loss_and_grad(c['flat'], c['tflat'], c['obs'], c['act'], c['rew'], c['done'], c['nobs'], c['mask'], c['w'], c['gamma_n'],
                          c['double_q'], dm)
    gap_bar = 10.0 * R.BAR_FACTOR * R.MEASURED[i]['q']
    boot = ref['boot']
    left = int((boot & (ref['gap'] < gap_bar)).sum())
    print('%d of %d bootstrapping rows under the gap bar %.3g' % (left, int(boot.sum()), gap_bar))
    assert left <= 0.01 * boot.sum()
    b0 = (np.clip(c['rew'].astype(np.float64) + c['gamma_n'] * dm.z[0], dm.v_min, dm.v_max) - dm.v_min) / dm.dz
    b2 = (np.clip(c['rew'].astype(np.float64) + c['gamma_n'] * dm.z[2 % dm.atoms], dm.v_min, dm.v_max) - dm.v_min) / dm.dz
    integer = (np.abs(b0 - np.round(b0)) < 1e-9) & (np.abs(b2 - np.round(b2)) < 1e-9)
    assert integer.mean() >= 0.1 and (c['rew'] > dm.v_max).any() and (c['rew'] < dm.v_min).any()
    assert np.abs(ref['m'].sum(axis=1) - 1.0).max() < 1e-12 and (ref['td'] >= 0).all()
    assert R.relu_margin(c['flat'], c['obs'], dm).min() >= R.RELU_MARGIN           # no stream unit of s sits on the relu's kink
    if c['masked']:
        assert (~boot & (c['done'] == 0)).sum() == 1 and not boot[c['k']]


@pytest.mark.parametrize('i,temperature', [(1, 1.0), (2, 1.0), (3, 2.0)])
def test_gpu_acting_cases_leave_at_most_one_percent_of_rows_to_cdf_edges(i, temperature):
    c = R.make_case(R.GPU_SHAPES[i], R.CASE_SEEDS[i])
    q = R.forward(c['flat'], c['obs'], c['dm'])[2]
    cdf = R.softq_cdf(q, c['mask'], temperature)
    u = td3_ref.uniform01(11, 5, np.arange(c['N']), 0)
    a, dist = R.softq_draw(cdf, u)
    bar = R.softq_edge_bar(R.BAR_FACTOR * R.MEASURED[i]['q'], temperature)
    print('%d of %d rows within %.3g of a CDF edge; %d distinct actions' % ((dist < bar).sum(), c['N'], bar, len(set(a))))
    assert (dist < bar).sum() <= 0.01 * c['N']
    if c['mask'] is not None:
        ok = c['mask'].any(axis=1)
        assert c['mask'][np.nonzero(ok)[0], a[ok]].all()


def test_new_symbols_are_declared_exported_and_bound():
    from rl4rs_amd.build import build_lib
    build_lib()
    from rl4rs_amd import _lib
    lib = _lib.load()
    text = open(os.path.join(REPO, 'include', 'rl4rs_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    names = ['rl4rs_distq_param_count', 'rl4rs_distq_create', 'rl4rs_distq_destroy', 'rl4rs_distq_params', 'rl4rs_distq_copy_params',
             'rl4rs_distq_adam_state', 'rl4rs_distq_set_adam_step', 'rl4rs_distq_act', 'rl4rs_distq_greedy', 'rl4rs_distq_loss_grad',
             'rl4rs_distq_adam_step_clip_by_var', 'rl4rs_replay_sample_nstep']
    for name in names:
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    # the layout the header states, and the configs it refuses
    from rl4rs_amd.nets.distq import param_count, init_distq_params
    import ctypes as C
    cfg = _lib.DistqCfg(256, 284, 8, 256, 128, 1, 0.0, 1000.0, 64)
    assert lib.rl4rs_distq_param_count(C.byref(cfg)) == param_count(256, 284, 8) == R.Dims().n_params() == len(init_distq_params())
    cfg = _lib.DistqCfg(256, 284, 8, 256, 128, 0, 0.0, 1000.0, 64)
    assert lib.rl4rs_distq_param_count(C.byref(cfg)) == param_count(256, 284, 8, dueling=False)
    for bad in (_lib.DistqCfg(256, 284, 1, 256, 128, 1, 0.0, 1000.0, 64), _lib.DistqCfg(256, 284, 65, 256, 128, 1, 0.0, 1000.0, 64),
                _lib.DistqCfg(256, 284, 8, 250, 128, 1, 0.0, 1000.0, 64), _lib.DistqCfg(256, 284, 8, 256, 128, 1, 5.0, 5.0, 64)):
        assert lib.rl4rs_distq_param_count(C.byref(bad)) == -1


def test_trainer_refuses_what_it_does_not_implement():
    from rl4rs_amd.train import RainbowTrainer

    class _Env(object):
        config = {'return_tensors': True, 'batch_size': 4, 'max_steps': 9, 'action_size': 284}

    with pytest.raises(ValueError, match='noisy'):
        RainbowTrainer(_Env(), noisy=True)
    with pytest.raises(ValueError, match='DQNTrainer'):
        RainbowTrainer(_Env(), num_atoms=1)
