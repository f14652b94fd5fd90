"""CPU: the float64 restatement of Exact-K's beam search (tests/exactk_beam_ref.py) against exactk_ref's own greedy decode, the
properties every beam search has, the hand-built case in which greedy is not the best slate, the recorded score yardstick, and the
share of rows whose selections are firm (the GPU test compares whole paths on those; its per-step checks exclude no row).  The
last test is the interface's: DeviceExactK.decode_beam and the trainer's eval_mode exist and refuse what they do not run."""
import functools

import numpy as np
import pytest

import exactk_beam_ref as BR
import exactk_ref as R


@functools.lru_cache(maxsize=None)
def _measured(i, B):
    """(float32 error of the selected scores, the float64 search's (paths, scores, trace)): computed once, shared, never modified"""
    return BR.score_yardstick(i, B)


@pytest.mark.parametrize('i', (1, 3))
def test_one_beam_is_the_greedy_decode(i):
    c = R.case(i, 0.1)
    seed, step = R.DECODE_STREAMS[i]
    paths, scores, tr = BR.beam_search(c['flat'], c['obs'], c['dm'], c['loc'], c['special'], 1, seed, step)
    greedy = R.decode(c['flat'], c['obs'], c['dm'], c['loc'], c['special'], True, seed=seed, step=step)
    assert np.array_equal(paths[:, 0], greedy)
    assert (tr['parent'] == 0).all()
    # and its score is the sum of the greedy path's 9 log-probabilities
    lg = R.logits_of(c['flat'], c['obs'], greedy, c['dm'], c['loc'], c['special'], seed=seed, step=step, pas=1)
    lp = lg - (lg.max(axis=2, keepdims=True) + np.log(np.exp(lg - lg.max(axis=2, keepdims=True)).sum(axis=2, keepdims=True)))
    want = np.take_along_axis(lp, greedy[:, :, None].astype(np.int64), axis=2)[:, :, 0].sum(axis=1)
    assert np.abs(scores[:, 0] - want).max() < 1e-11


@pytest.mark.parametrize('i,B', BR.CASES)
def test_beams_are_valid_distinct_and_ordered(i, B):
    c = R.case(i, 0.1)
    _, (paths, scores, tr) = _measured(i, B)
    N, A = c['N'], c['dm'].A
    assert paths.shape == (N, B, R.T) and scores.shape == (N, B)
    for b in range(B):
        p = paths[:, b]
        assert ((p >= 0) & (p < A)).all()
        assert all(len(set(row.tolist())) == R.T for row in p)                          # 9 distinct picks
        allowed = R.allowed_sets(p, c['loc'], c['special'])
        assert allowed[np.arange(N)[:, None], np.arange(R.T)[None, :], p].all()          # each in its allowed set
    for n in range(N):
        assert len(set(tuple(paths[n, b].tolist()) for b in range(B))) == B              # the beams of a row are pairwise different
        assert len(set(tr['token'][n, 0].tolist())) == B                                 # B distinct first picks at step 0
    assert (tr['parent'][:, 0] == 0).all()
    assert (np.diff(scores, axis=1) <= 0).all() and (np.diff(tr['score'], axis=2) <= 0).all()
    assert np.array_equal(BR.replay(tr['parent'], tr['token'])[1], paths) and np.array_equal(tr['score'][:, -1], scores)


def test_beam_search_beats_greedy_on_the_hand_built_case():
    """exactk_beam_ref.tiny_case (A = 11): on its row the greedy first pick leads to a worse total than the second-best first pick."""
    c, n = BR.tiny_case(), BR.TINY['row']
    ctx = BR.Beam(c['flat'], c['obs'], c['dm'], c['loc'], c['special'])
    paths, scores, tr = BR.search(ctx, 3)
    greedy = R.decode(c['flat'], c['obs'], c['dm'], c['loc'], c['special'], True)
    first = ctx.candidate_scores(np.zeros((c['N'], 1, R.T), dtype=np.int32), 0)[n, 0]
    order = np.argsort(-first, kind='stable')
    assert greedy[n, 0] == order[0] and paths[n, 0, 0] == order[1]
    assert not np.array_equal(paths[n, 0], greedy[n])
    g_score = BR.scores_along(ctx, np.zeros((c['N'], R.T, 1), dtype=np.int32), greedy[:, :, None])[1][n, -1, 0]
    print('greedy %s %.6f   beam 0 %s %.6f' % (greedy[n], g_score, paths[n, 0], scores[n, 0]))
    assert scores[n, 0] - g_score > BR.TINY['margin']


@pytest.mark.parametrize('i,B', BR.CASES)
def test_recorded_score_yardstick_is_reproduced_and_enough_rows_are_firm(i, B):
    err, (_, _, tr) = _measured(i, B)
    rec = BR.MEASURED_SCORE[(i, B)]
    print('case %s: float32 score error %.3g (recorded %.3g)' % ((i, B), err, rec))
    assert 0.5 * rec <= err <= 2.0 * rec
    firm = BR.firm_rows(tr['gap'], BR.score_bar(i, B))
    print('case %s: %d of %d rows firm (every gap among the top %d candidates above %.3g at every step)'
          % ((i, B), int(firm.sum()), len(firm), B + 1, 2.0 * BR.score_bar(i, B)))
    assert firm.sum() >= 0.25 * len(firm)


def test_interface_exists_and_the_trainer_refuses_other_eval_modes():
    import inspect
    from rl4rs_amd import _lib
    from rl4rs_amd.device import DeviceExactK
    from rl4rs_amd.train import ExactKTrainer
    assert 'rl4rs_exactk_decode_beam' in _lib.SIGNATURES
    sig = inspect.signature(DeviceExactK.decode_beam)
    assert sig.parameters['beam_size'].default == 3 and sig.parameters['want_trace'].default is False
    sig = inspect.signature(ExactKTrainer.__init__)
    assert sig.parameters['eval_mode'].default == 'greedy' and sig.parameters['beam_size'].default == 3

    class _Env(object):
        config = {'max_steps': 9, 'batch_size': 4, 'action_size': 284}
    for bad in ('sample', None, 'BEAM'):
        with pytest.raises(ValueError, match='eval_mode'):
            ExactKTrainer(_Env(), eval_mode=bad)
    with pytest.raises(ValueError, match='beam_size'):
        ExactKTrainer(_Env(), eval_mode='beam', beam_size=9)
