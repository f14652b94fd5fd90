"""CPU: the float64 restatement of the on-device Rainbow (tests/rainbow_ref.py) against torch float64 autograd, the categorical
projection on a hand-made case, the n-step row rule, the inputs of the GPU tests (how many rows their near-tie bars leave out), and
the new symbols of the C ABI."""
import hashlib
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


def _cases(indices, shape_indices):
    """('base', i): shape i of GPU_SHAPES (ids as before the second list existed); ('shape', i): case i of SHAPE_CASES"""
    return [pytest.param(('base',) + ((i,) if not isinstance(i, tuple) else i), id='-'.join(str(x) for x in (i if isinstance(i, tuple) else (i,))))
            for i in indices] + \
           [pytest.param(('shape',) + ((i,) if not isinstance(i, tuple) else i), id='shape' + '-'.join(str(x) for x in (i if isinstance(i, tuple) else (i,))))
            for i in shape_indices]


def _load(kind, i):
    """-> (inputs, yardstick figures, relu margin) of a case of either list"""
    if kind == 'base':
        return R.make_case(R.GPU_SHAPES[i], R.CASE_SEEDS[i]), R.MEASURED[i], R.RELU_MARGIN
    return R.shape_case(i), R.MEASURED_SHAPES[i], R.shape_margin(i)


def _digest(c):
    h = hashlib.sha256()
    for k in ('flat', 'tflat', 'obs', 'nobs', 'mask', 'done', 'act', 'rew', 'w'):
        h.update(np.ascontiguousarray(c[k]).tobytes())
    h.update(repr((c['k'], c['gamma_n'], c['double_q'], c['masked'], c['N'])).encode())
    return h.hexdigest()


def test_make_case_defaults_reproduce_the_inputs_of_the_reference_width():
    """make_case grew trunk / sh / support / margin arguments: with the defaults, the second shape's inputs are bit for bit what
    they were before (the digest was taken with the function as it stood then), and naming the defaults changes nothing."""
    shape = R.GPU_SHAPES[1]
    c = R.make_case(shape, R.CASE_SEEDS[1])
    assert _digest(c) == '4d24ff10e79b7bc27781cc1f9bda8baa3fd15bf47a6ba8fbfab77b04f53237ab'
    assert (c['dm'].trunk, c['dm'].sh, c['margin']) == (256, 128, R.RELU_MARGIN)
    assert _digest(R.make_case(shape, R.CASE_SEEDS[1], trunk=256, sh=128, support=R.SUPPORT[shape[2]], margin=R.RELU_MARGIN)) == _digest(c)
    assert _digest(R.make_case(shape, R.CASE_SEEDS[1] + 1)) != _digest(c)


def test_shape_cases_are_the_ends_of_what_the_handle_admits():
    assert len(R.SHAPE_CASES) == len(R.SHAPE_SEEDS) == len(R.MEASURED_SHAPES) == 5
    for i, (shape, support) in enumerate(R.SHAPE_CASES):
        c = R.shape_case(i)
        dm = c['dm']
        assert (dm.od, dm.A, dm.atoms, c['N'], int(dm.dueling), int(c['double_q']), int(c['masked']), dm.trunk, dm.sh) == shape
        assert (dm.v_min, dm.v_max, c['gamma_n']) == support[:3]
        assert c['margin'] == max(R.RELU_MARGIN, 4.0 * R.MEASURED_SHAPES[i]['pre'])
        assert len(c['flat']) == dm.n_params()
    assert R.shape_margin(2) > R.RELU_MARGIN                                # the 1024-wide trunk: the margin is its own
    one = R.shape_case(3)                                                   # the one row is set by hand
    assert one['N'] == 1 and one['done'][0] == 0 and one['rew'][0] == np.float32(support[3] + one['dm'].dz)


@pytest.mark.parametrize('case', _cases(range(len(R.GPU_SHAPES)), range(len(R.SHAPE_CASES))))
def test_gpu_cases_leave_at_most_one_percent_of_rows_to_near_ties(case):
    """The inputs of tests/test_gpu_rainbow.py and tests/test_gpu_rainbow_shapes.py, with the restatement alone: integer b on a tenth
    of the rows at least, rewards past both ends of the support, and at most 1 % of the bootstrapping rows under the a* gap bar
    (a condition: with the 24 to 60 bootstrapping rows of the small cases it means none)."""
    c, measured, margin = _load(*case)
    dm = c['dm']
    ref = R.loss_and_grad(c['flat'], c['tflat'], c['obs'], c['act'], c['rew'], c['done'], c['nobs'], c['mask'], c['w'], c['gamma_n'],
                          c['double_q'], dm)
    gap_bar = 10.0 * R.BAR_FACTOR * measured['q']
    boot = ref['boot']
    left = int((boot & (ref['gap'] < gap_bar)).sum())
    print('%d of %d bootstrapping rows under the gap bar %.3g' % (left, int(boot.sum()), gap_bar))
    assert left <= 0.01 * boot.sum()
    b0 = (np.clip(c['rew'].astype(np.float64) + c['gamma_n'] * dm.z[0], dm.v_min, dm.v_max) - dm.v_min) / dm.dz
    b2 = (np.clip(c['rew'].astype(np.float64) + c['gamma_n'] * dm.z[2 % dm.atoms], dm.v_min, dm.v_max) - dm.v_min) / dm.dz
    integer = (np.abs(b0 - np.round(b0)) < 1e-9) & (np.abs(b2 - np.round(b2)) < 1e-9)
    if c['N'] >= 31:
        assert integer.mean() >= 0.1
        assert (c['rew'] > dm.v_max).any() and (c['rew'] < dm.v_min).any() and (c['done'] != 0).any()
    else:
        # the one row bootstraps on R0 + dz: b_j = j + 1 up to the float32 rounding of the reward (dz = 1000 / 15 is no float32
        # number), so every source atom sits within a rounding of the lo == up branch, on either side of it
        assert c['N'] == 1 and boot.all()
        assert np.abs(b0 - 1.0).max() <= 2.0 ** -24 and np.abs(b2 - 3.0).max() <= 3.0 * 2.0 ** -24
    assert boot.any()
    assert np.abs(ref['m'].sum(axis=1) - 1.0).max() < 1e-12 and (ref['td'] >= 0).all()
    assert R.relu_margin(c['flat'], c['obs'], dm).min() >= margin                  # no stream unit of s sits on the relu's kink
    if c['masked']:
        assert (~boot & (c['done'] == 0)).sum() == 1 and not boot[c['k']]


@pytest.mark.parametrize('case', _cases([(1, 1.0), (2, 1.0), (3, 2.0)], [(0, 1.0), (1, 1.0), (2, 2.0)]))
def test_gpu_acting_cases_leave_at_most_one_percent_of_rows_to_cdf_edges(case):
    kind, i, temperature = case
    c, measured, _ = _load(kind, i)
    q = R.forward(c['flat'], c['obs'], c['dm'])[2]
    cdf = R.softq_cdf(q, c['mask'], temperature)
    u = td3_ref.uniform01(11, 5, np.arange(c['N']), 0)
    a, dist = R.softq_draw(cdf, u)
    bar = R.softq_edge_bar(R.BAR_FACTOR * measured['q'], temperature)
    print('%d of %d rows within %.3g of a CDF edge; %d distinct actions' % ((dist < bar).sum(), c['N'], bar, len(set(a))))
    assert (dist < bar).sum() <= 0.01 * c['N']
    assert len(set(a)) >= 2                                                        # the draw is a draw
    if c['mask'] is not None:
        ok = c['mask'].any(axis=1)
        assert c['mask'][np.nonzero(ok)[0], a[ok]].all()
    # greedy on the same rows: at most 1 % near-ties (+ the one row that allows nothing)
    top = np.sort(R.masked_q(q, c['mask']), axis=1)[:, -2:]
    near = (top[:, 1] - top[:, 0]) < 10.0 * R.BAR_FACTOR * measured['q']
    assert near.sum() <= 0.01 * c['N'] + (0 if c['mask'] is None else 1)


@pytest.mark.parametrize('i', [3, 4])
def test_greedy_only_cases_leave_at_most_one_percent_of_rows_to_near_ties(i):
    c = R.shape_case(i)
    top = np.sort(R.forward(c['flat'], c['obs'], c['dm'])[2], axis=1)[:, -2:]
    near = (top[:, 1] - top[:, 0]) < 10.0 * R.BAR_FACTOR * R.MEASURED_SHAPES[i]['q']
    print('%d of %d rows under the greedy gap bar' % (near.sum(), c['N']))
    assert near.sum() <= 0.01 * c['N']


def test_dropping_the_last_of_33_atoms_would_show():
    """An AP = 32 lane mapping would see 32 of the third case's 33 atoms.  The same loss with the last atom dropped (softmax over
    32 logits, the projected mass of atom 32 lost) misses td by more than ten times the td bar."""
    c = R.shape_case(2)
    dm = c['dm']
    assert dm.atoms == 33
    ref = R.loss_and_grad(c['flat'], c['tflat'], c['obs'], c['act'], c['rew'], c['done'], c['nobs'], c['mask'], c['w'], c['gamma_n'],
                          c['double_q'], dm)
    logit = R.forward(c['flat'], c['obs'], dm)[0][np.arange(c['N']), c['act']][:, :32]
    sh = logit - logit.max(axis=1, keepdims=True)
    lsm = sh - np.log(np.exp(sh).sum(axis=1, keepdims=True))
    td_bad = -(ref['m'][:, :32] * lsm).sum(axis=1)
    miss = np.abs(td_bad - ref['td']).max()
    print('td without atom 32 misses by %.3g (bar %.3g)' % (miss, R.BAR_FACTOR * R.MEASURED_SHAPES[2]['td']))
    assert miss > 10.0 * R.BAR_FACTOR * R.MEASURED_SHAPES[2]['td']


def test_a_dueling_mean_over_256_of_512_actions_would_show():
    """A head that centres the second case's advantages on the mean of its first 256 actions misses Q by more than ten times the Q bar."""
    c = R.shape_case(1)
    dm = c['dm']
    assert dm.A == 512 and dm.dueling
    p = R.split(c['flat'].astype(np.float64), dm)
    _, _, ha, hv = R.hidden(p, c['obs'].astype(np.float64), dm)
    adv = (ha @ p['Wa2'] + p['ba2']).reshape(c['N'], dm.A, dm.atoms)
    v = hv @ p['Wv2'] + p['bv2']

    def q_of(mean):
        logits = v[:, None, :] + adv - mean
        e = np.exp(logits - logits.max(axis=2, keepdims=True))
        return ((e / e.sum(axis=2, keepdims=True)) * dm.z).sum(axis=2)

    q = q_of(adv.mean(axis=1, keepdims=True))
    assert np.abs(q - R.forward(c['flat'], c['obs'], dm)[2]).max() < 1e-12
    miss = np.abs(q_of(adv[:, :256].mean(axis=1, keepdims=True)) - q).max()
    print('Q with the mean of 256 actions misses by %.3g (bar %.3g)' % (miss, R.BAR_FACTOR * R.MEASURED_SHAPES[1]['q']))
    assert miss > 10.0 * R.BAR_FACTOR * R.MEASURED_SHAPES[1]['q']


def test_param_count_refuses_what_lies_past_the_ends():
    import ctypes as C
    from rl4rs_amd.build import build_lib
    build_lib()
    from rl4rs_amd import _lib
    lib = _lib.load()
    cfg = lambda od=256, A=284, atoms=8, trunk=256, sh=128: _lib.DistqCfg(od, A, atoms, trunk, sh, 1, 0.0, 1000.0, 64)
    for shape, _ in R.SHAPE_CASES:                                          # every case lies inside
        od, A, atoms, N, dueling, _, _, trunk, sh = shape
        c = _lib.DistqCfg(od, A, atoms, trunk, sh, dueling, 0.0, 1000.0, N)
        assert lib.rl4rs_distq_param_count(C.byref(c)) == R.Dims(od, A, atoms, trunk, sh, bool(dueling)).n_params()
    for bad in (cfg(A=1), cfg(A=513), cfg(trunk=1056), cfg(sh=288), cfg(sh=48), cfg(od=2049)):
        assert lib.rl4rs_distq_param_count(C.byref(bad)) == -1
    for good in (cfg(A=2), cfg(A=512), cfg(trunk=1024), cfg(sh=256), cfg(sh=32), cfg(od=2048), cfg(atoms=64)):
        assert lib.rl4rs_distq_param_count(C.byref(good)) > 0


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
