"""CPU: the offline scorers' host side - the float64 restatement (tests/scorer_ref.py) against hand-computed cases and against the
fixtures recorded from the reference's own rl4rs/utils/d3rlpy_scorer.py, ``episodes_from_mdp`` against ``transitions_from_mdp``,
and (where the reference checkout exists) the fixtures regenerated."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scorer_ref as SR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden')
FIXTURES = ('scorer_mixed.npz', 'scorer_tens.npz')


def test_restatement_on_hand_computed_episodes():
    # two episodes: rows 0-2 and 3-4
    starts = [0, 3, 5]
    cols = dict(qd=[1.0, 2.0, 4.0, 0.5, 3.0], qp=[2.0, 2.0, 3.0, 1.5, 1.0], qn=[1.0, 0.0, 9.0, 2.0, 7.0],
                r_td=[0.5, 1.0, 0.0, 2.0, 0.0], r_raw=[5.0, 10.0, 0.0, 20.0, 0.0], ter=[0, 0, 1, 0, 1],
                a=[1, 2, 3, 4, 5], a_pi=[1, 0, 3, 0, 5], a_mask=[1, 2, 0, 4, 5], diff=[1.0, 0.0, 2.0, 3.0, 4.0])
    g = 0.5
    r = SR.scores(starts, cols, g, return_threshold=16.0)
    # td: (1 - (0.5 + 0.5))^2, (2 - 1)^2, (4 - 0)^2, (0.5 - (2 + 1))^2, (3 - 0)^2
    assert r['td_error'] == pytest.approx((0.0 + 1.0 + 16.0 + 6.25 + 9.0) / 5, rel=1e-15)
    # adv = -1, 0, 1 | -1, 2;  S = (-1 + .5 * (0 + .5 * 1), 0.5, 1) | (-1 + .5 * 2, 2)
    assert r['discounted_sum_of_advantage'] == pytest.approx((-0.75 + 0.5 + 1.0 + 0.0 + 2.0) / 5, rel=1e-15)
    assert r['average_value_estimation'] == pytest.approx(9.5 / 5, rel=1e-15)
    assert r['initial_state_value_estimation'] == pytest.approx((2.0 + 1.5) / 2, rel=1e-15)
    # returns 15 and 20: only the second episode reaches 16
    assert r['soft_opc'] == pytest.approx(3.5 / 2 - 10.5 / 5, rel=1e-15)
    assert r['discrete_action_match'] == pytest.approx(3 / 5) and r['discrete_action_match_mask'] == pytest.approx(4 / 5)
    assert r['continuous_action_diff'] == pytest.approx(2.0)
    assert np.isnan(SR.scores(starts, cols, g, return_threshold=21.0)['soft_opc'])
    assert SR.scores(starts, cols, g, return_threshold=15.0)['soft_opc'] == 0.0
    assert SR.scores(starts, cols, 1.0)['discounted_sum_of_advantage'] == pytest.approx((0.0 + 1.0 + 1.0 + 1.0 + 2.0) / 5, rel=1e-15)
    # a missing column leaves exactly the scores that need it NaN
    part = SR.scores(starts, {k: v for k, v in cols.items() if k != 'qn'}, g, 16.0)
    assert np.isnan(part['td_error']) and not any(np.isnan(part[k]) for k in SR.NAMES if k != 'td_error')


def test_restatement_restarts_the_scan_every_1024_rows():
    n = 1030
    cols = dict(qd=np.ones(n), qp=np.zeros(n))
    r = SR.scores([0, n], cols, 1.0)
    # gamma 1: S counts the rows left in the window: 1024 .. 1, then 6 .. 1
    assert r['discounted_sum_of_advantage'] == pytest.approx((1024 * 1025 / 2 + 6 * 7 / 2) / n, rel=1e-15)


@pytest.mark.parametrize('name', FIXTURES)
def test_restatement_matches_the_reference_fixtures(name):
    with np.load(os.path.join(GOLDEN, name)) as z:
        starts = SR.starts_of(z['lengths'])
        cols = dict(qd=z['qd'], r_raw=z['next_rewards'], a=z['a'], a_mask=z['a_mask'])
        for th, want in zip(z['thresholds'], z['soft_opc']):
            got = SR.scores(starts, cols, 1.0, float(th))['soft_opc']
            assert (np.isnan(got) and np.isnan(want)) or got == pytest.approx(want, rel=1e-12, abs=1e-12), (th, got, want)
        assert SR.scores(starts, cols)['discrete_action_match_mask'] == pytest.approx(float(z['discrete_action_match']), rel=1e-14)
        err = z['next_rewards'] - z['rhat']                                  # float32, as the reference subtracts
        assert SR.scores(starts, dict(qp=err))['average_value_estimation'] == pytest.approx(float(z['dynamics_mean_error']), rel=1e-12)
        assert SR.scores(starts, dict(qp=np.abs(err)))['average_value_estimation'] == pytest.approx(float(z['dynamics_abs_mean_error']), rel=1e-12)
        assert 1030 in z['lengths'] or len(z['lengths']) == 300


def _mdp(lengths, trailing=0, seed=0, D=5, conti=False):
    rs = np.random.RandomState(seed)
    n = int(np.sum(lengths)) + trailing
    ter = np.zeros(n, dtype=np.float32)
    if len(lengths):
        ter[np.cumsum(lengths) - 1] = 1.0
    actions = rs.normal(size=(n, 3)).astype(np.float32) if conti else rs.randint(0, 7, size=n)
    return dict(observations=rs.normal(size=(n, D)).astype(np.float32), actions=actions,
                rewards=rs.rand(n).astype(np.float32), terminals=ter)


@pytest.mark.parametrize('lengths,trailing,want', [((3, 1, 4), 0, (3, 1, 4)), ((3, 2), 3, (3, 2, 2)), ((2,), 1, (2,)), ((), 4, (3,))])
def test_episodes_from_mdp_are_the_transitions_of_transitions_from_mdp(lengths, trailing, want):
    from rl4rs_amd.offline_rl import transitions_from_mdp
    from rl4rs_amd.scorers import episodes_from_mdp
    data = _mdp(lengths, trailing)
    ep = episodes_from_mdp(data, device='cpu')
    tr = transitions_from_mdp(data['observations'], data['actions'], data['rewards'], data['terminals'])
    for got, ref in zip(ep.columns(), tr):
        assert got.dtype == ref.dtype and torch.equal(got, ref)
    # a trailing run without terminal flag loses its last row; left with no transition, it is no episode
    assert len(ep) == len(want) and ep.starts.dtype == torch.int64
    assert np.array_equal(ep.starts.numpy(), SR.starts_of(want))
    assert ep.discrete_action
    ret = ep.returns()
    assert ret.dtype == torch.float64 and ret.shape == (len(want),)
    for e in range(len(want)):
        lo, hi = int(ep.starts[e]), int(ep.starts[e + 1])
        assert float(ret[e]) == pytest.approx(float(tr[2][lo:hi].double().sum()), rel=1e-15)
    # d3rlpy's Episode.compute_return, sum(rewards[1:]) of the episode's rows: a terminated episode's own rewards but its first
    if lengths:
        assert float(ret[0]) == pytest.approx(float(np.sum(data['rewards'][1:lengths[0]].astype(np.float64))), rel=1e-15)


def test_episode_slices_are_views_and_other_keys_are_refused():
    from rl4rs_amd.scorers import episodes_from_mdp
    lengths = (3, 1, 4, 2, 5)
    ep = episodes_from_mdp(_mdp(lengths, conti=True), device='cpu')
    assert not ep.discrete_action and ep.actions.dtype == torch.float32 and ep.actions.shape == (15, 3)
    st = SR.starts_of(lengths)
    for key, (a, b) in ((slice(1, 4), (1, 4)), (slice(-2, None), (3, 5)), (slice(None, 2), (0, 2)), (slice(-3000, None), (0, 5)),
                        (slice(2, 3, 1), (2, 3))):
        sub = ep[key]
        assert len(sub) == b - a and np.array_equal(sub.starts.numpy(), st[a:b + 1] - st[a])
        assert sub.observations.data_ptr() == ep.observations[st[a]:].data_ptr()             # a view, not a copy
        for got, whole in zip(sub.columns(), ep.columns()):
            assert torch.equal(got, whole[st[a]:st[b]])
        assert torch.equal(sub.returns(), ep.returns()[a:b])
    assert len(ep[3:3]) == 0 and len(ep[4:2]) == 0
    for bad in (0, -1, slice(0, 4, 2), slice(None, None, -1), [0, 1], (slice(0, 1), 0)):
        with pytest.raises(TypeError):
            ep[bad]


def test_alias_module_exposes_the_reference_names():
    import rl4rs.utils.d3rlpy_scorer as alias
    import rl4rs_amd.utils.d3rlpy_scorer as own
    for name in ('soft_opc_scorer', 'discrete_action_match_scorer', 'dynamics_reward_prediction_mean_error_scorer',
                 'dynamics_reward_prediction_abs_mean_error_scorer'):
        assert getattr(alias, name) is getattr(own, name)
    assert alias.WINDOW_SIZE == 1024
    from rl4rs_amd import scorers as S
    assert S.soft_opc_scorer(90)._rl4rs_score == ('soft_opc', 90.0, False) and own.soft_opc_scorer(90)._rl4rs_score == ('soft_opc', 90.0, True)
    assert own.discrete_action_match_scorer._rl4rs_score == ('discrete_action_match_mask', None, True)


def test_unknown_names_and_a_missing_threshold_are_refused_before_any_device_work():
    from rl4rs_amd import scorers as S
    ep = S.episodes_from_mdp(_mdp((3, 2)), device='cpu')
    with pytest.raises(ValueError):
        S.evaluate_scorers(object(), ep, ['value_estimation_std'])
    with pytest.raises(ValueError):
        S.evaluate_scorers(object(), ep, ['soft_opc'])
    with pytest.raises(TypeError):
        S.evaluate_scorers(object(), ep, ['td_error'])


@pytest.mark.skipif(not os.path.isdir('/root/reference'), reason='the reference checkout is not on this machine')
def test_fixtures_regenerate_from_the_reference(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, 'make_scorer_golden.py'), '--out', str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for name in FIXTURES:
        with np.load(os.path.join(GOLDEN, name)) as a, np.load(os.path.join(str(tmp_path), name)) as b:
            assert sorted(a.files) == sorted(b.files)
            for k in a.files:
                assert np.array_equal(a[k], b[k], equal_nan=True) and a[k].dtype == b[k].dtype, (name, k)
