"""CPU: the off-policy-evaluation surface that needs no GPU - the reference's module names, the library's Student-t quantile
against scipy's recorded values, the argument checks of the C entry points, and (where the reference checkout and scipy exist)
that the fixture generator reproduces the committed fixtures."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden')
OPE_FIXTURES = ('ope_estimators.npz', 'ope_tquantile.npz', 'ope_behavior.npz', 'ope_loop.npz')


@pytest.fixture(scope='module')
def lib():
    from rl4rs_amd.build import build_lib
    build_lib()
    from rl4rs_amd import _lib
    return _lib.load()


def test_alias_modules_expose_the_reference_names():
    import rl4rs.utils.offline_policy_metrics as OPE
    from rl4rs.policy.behavior_model import behavior_model
    from rl4rs_amd.ope import ope_eval
    for name in ('eval_IPS', 'eval_CIPS', 'eval_SNIPS', 'eval_WIPS', 'eval_doubly_robust', 'eval_seq_doubly_robust', 'eval_DM'):
        assert callable(getattr(OPE, name)), name
    import inspect
    assert list(inspect.signature(OPE.eval_WIPS).parameters) == ['step_rewards', 'policy_prob', 'behavior_prob', 'gamma']
    assert inspect.signature(OPE.eval_WIPS).parameters['gamma'].default == 1.0
    assert list(inspect.signature(OPE.eval_doubly_robust).parameters) == ['action_rhat_rewards', 'state_rewards', 'rewards', 'policy_prob',
                                                                          'behavior_prob']
    assert list(inspect.signature(behavior_model.action_probs).parameters) == ['self', 'record', 'action', 'layer', 'page']
    assert list(inspect.signature(ope_eval).parameters) == ['config', 'eval_env', 'algo', 'sample_model', 'on_epoch']


def test_the_product_does_not_import_scipy():
    code = ("import sys; import rl4rs.utils.offline_policy_metrics, rl4rs.policy.behavior_model, rl4rs_amd.ope; "
            "sys.exit(1 if any(m == 'scipy' or m.startswith('scipy.') for m in sys.modules) else 0)")
    assert subprocess.run([sys.executable, '-c', code], cwd=REPO).returncode == 0


def test_layer_rule_of_the_behaviour_model():
    """behavior_model.py:49-57: layer 1 -> [1, 40), 2 -> [40, 148), anything else -> [148, A_b)"""
    from rl4rs_amd.policy.behavior_model import layer_range
    assert layer_range(1, 382) == (1, 40) and layer_range(2, 382) == (40, 148)
    for layer in (3, 4, 12, 0):
        assert layer_range(layer, 382) == (148, 382)


def test_student_t_quantile_against_scipy(lib):
    """rl4rs_student_t_ppf against scipy.stats.t.ppf(0.99875, df) as recorded: rtol 1e-9 (the estimators' bar - the quantile enters
    the confidence width linearly), NaN where scipy has NaN (df <= 0)."""
    with np.load(os.path.join(GOLDEN, 'ope_tquantile.npz')) as z:
        df, p, want = z['df'], float(z['p']), z['expected']
    assert len(df) == 12 and p == 0.99875
    for d, w in zip(df, want):
        got = lib.rl4rs_student_t_ppf(p, float(d))
        print('df %g: got %.17g want %.17g rel %.3g' % (d, got, w, abs(got - w) / abs(w) if w == w else float('nan')))
        if np.isnan(w):
            assert np.isnan(got), d
        else:
            assert abs(got - w) <= 1e-9 * abs(w), (d, got, w)
    # symmetry and the ends
    assert lib.rl4rs_student_t_ppf(0.5, 9.0) == 0.0
    assert lib.rl4rs_student_t_ppf(0.25, 30.0) == -lib.rl4rs_student_t_ppf(0.75, 30.0)
    # (1 - 0.99875 is not the double 0.00125: equal up to that rounding of the tail mass, 1e-13 relative)
    assert abs(lib.rl4rs_student_t_ppf(0.00125, 30.0) + lib.rl4rs_student_t_ppf(0.99875, 30.0)) < 1e-11
    assert lib.rl4rs_student_t_ppf(1.0, 3.0) == np.inf and lib.rl4rs_student_t_ppf(0.0, 3.0) == -np.inf
    assert np.isnan(lib.rl4rs_student_t_ppf(1.5, 3.0)) and np.isnan(lib.rl4rs_student_t_ppf(float('nan'), 3.0))


def test_ope_entry_points_refuse_bad_shapes_before_looking_for_a_device(lib):
    """RL4RS_EINVAL for T > 256, B < 1 and null arrays, from the size checks alone (no device needed, no pointer read)."""
    h = C.c_void_p()
    out = (C.c_double * 17)()
    dummy = C.c_void_p(16)              # never dereferenced: refused shapes only

    def msg():
        return lib.rl4rs_last_error().decode()

    for B, T, words in ((8, 257, ('257', '256')), (8, 1000, ('256',)), (0, 9, ('batch size', '< 1')), (-3, 9, ('< 1',)),
                        (8, 0, ('steps', '< 1'))):
        assert lib.rl4rs_ope_create(B, T, C.byref(h)) == -1 and not h.value, (B, T)
        for w in words:
            assert w in msg(), (B, T, msg())
        assert lib.rl4rs_ope_step_stats(B, T, dummy, dummy, dummy, None, None, 1.0, out, None) == -1, (B, T)
        for w in words:
            assert w in msg(), (B, T, msg())
    assert lib.rl4rs_ope_episode_stats(0, dummy, dummy, dummy, None, None, out, None) == -1 and '< 1' in msg()
    assert lib.rl4rs_ope_episode_stats(8, None, dummy, dummy, None, None, out, None) == -1 and 'null' in msg()
    assert lib.rl4rs_ope_step_stats(8, 9, dummy, None, dummy, None, None, 1.0, out, None) == -1 and 'null' in msg()
    assert lib.rl4rs_ope_begin(None, 8, 9) == -1 and lib.rl4rs_ope_estimate(None, 1.0, out, None) == -1
    if lib.rl4rs_device_count() <= 0:
        # admitted shapes get as far as the device check
        assert lib.rl4rs_ope_create(8, 256, C.byref(h)) == -2 and 'no HIP device' in msg() and not h.value
        assert lib.rl4rs_ope_episode_stats(8, dummy, dummy, dummy, None, None, out, None) == -2 and 'no HIP device' in msg()


def test_python_surface_refuses_mismatched_shapes_and_unsupported_policies():
    """mismatched shapes are a ValueError from the shape comparison alone, before a device is looked for (so also without one);
    with agreeing shapes and no GPU the call fails loudly (no CPU fallback)"""
    import torch
    import rl4rs.utils.offline_policy_metrics as OPE
    from rl4rs_amd.ope import ope_eval
    B, T = 6, 9
    one, two = np.ones(B), np.ones((B, T))
    with pytest.raises(ValueError, match='mismatched shapes'):
        OPE.eval_CIPS(one, one, np.ones(B + 1))
    with pytest.raises(ValueError, match='mismatched shapes'):
        OPE.eval_IPS(one, np.ones(B + 1), one)
    with pytest.raises(ValueError, match='mismatched shapes'):
        OPE.eval_doubly_robust(one, np.ones(B + 1), one, one, one)
    with pytest.raises(ValueError, match='mismatched shapes'):
        OPE.eval_WIPS(two, two, np.ones((B, T + 1)))
    with pytest.raises(ValueError, match='mismatched shapes'):
        OPE.eval_seq_doubly_robust(np.ones((B + 1, T)), two, two, two, two)
    with pytest.raises(ValueError, match='2-d array'):
        OPE.eval_WIPS(one, one, one)
    with pytest.raises(ValueError, match='1-d array'):
        OPE.eval_SNIPS(two, two, two)
    with pytest.raises(ValueError, match='non-empty'):
        OPE.eval_CIPS(np.ones(0), np.ones(0), np.ones(0))
    with pytest.raises(ValueError, match='mismatched shapes'):          # tensors are compared the same way
        OPE.eval_CIPS(torch.ones(B), torch.ones(B), torch.ones(B + 1))
    with pytest.raises(ValueError, match='support_conti_env'):
        ope_eval(dict(support_conti_env=True, epoch=1, batch_size=4, max_steps=9), None, object())
    if not torch.cuda.is_available():
        from rl4rs_amd._lib import Rl4rsHipError
        with pytest.raises(Rl4rsHipError):
            OPE.eval_CIPS(one, one, one)
        with pytest.raises(Rl4rsHipError):
            OPE.eval_WIPS(two, two, two)


def test_fixture_inputs_meet_their_conditions():
    """what the generator asserts about fixture 1, re-checked on the committed file: finite and < 1e6 for B >= 64, a case with
    WIPS away from 1, a case on the int(n_e) - 1 <= 0 (NaN) path; every required (B, T) is present."""
    import ope_inputs as I
    with np.load(os.path.join(GOLDEN, 'ope_estimators.npz')) as z:
        cases, exp = z['cases'], z['expected']
    assert [tuple(c) for c in cases] == I.ESTIMATOR_CASES and exp.shape == (len(cases), 7, 2)
    assert {(1, 9), (7, 9), (64, 9), (300, 36), (4096, 9), (4096, 32), (16384, 9)} <= set((int(b), int(t)) for b, t, _ in cases)
    big = cases[:, 0] >= 64
    assert np.isfinite(exp[big][:, [1, 2, 3, 4, 5, 6]]).all() and (np.abs(exp[big][:, [1, 2, 3, 4, 5, 6]]) < 1e6).all()
    assert (np.abs(exp[:, 4, 0] - 1) > 1e-3).any() and np.isnan(exp[:, 1, 1]).any()
    with np.load(os.path.join(GOLDEN, 'ope_loop.npz')) as z:
        assert (z['std'][z['cases'][:, 2] == 1][:, :, 0] > 0).all()          # the epochs differ


@pytest.mark.skipif(not os.path.isdir('/root/reference'), reason='the reference checkout is not on this machine')
def test_generator_reproduces_the_committed_fixtures(tmp_path):
    pytest.importorskip('scipy')
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, 'make_ope_golden.py'), '--out', str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in OPE_FIXTURES:
        with np.load(os.path.join(GOLDEN, name)) as a, np.load(os.path.join(str(tmp_path), name)) as b:
            assert sorted(a.files) == sorted(b.files), name
            for k in a.files:
                assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (name, k)
