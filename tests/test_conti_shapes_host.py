"""What tests/test_gpu_conti_shapes.py relies on, settled without a GPU from the references alone (tests/conti_ref.py): the crafted
BCQ-target inputs are exact in fp32 and hold every tie pattern, the overflow rows of the CQL case do tell the stabilised
logsumexp from the plain one, every yardstick is a usable number (the table prints under -s), and a backward through stale
transposed weights cannot hide inside the gradient bar."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conti_ref as R          # noqa: E402


@pytest.mark.parametrize('case', R.BCQ_TARGET_CASES, ids=lambda c: 'B%d-n%d-lam%g-%s' % (c[0], c[1], c[2], 'twin' if c[3] else 'single'))
def test_bcq_target_inputs_are_exact_and_hold_every_tie_pattern(case):
    B, n, lam, twin = case
    c = R.bcq_target_inputs(*case)
    v32, best32, y32 = R.bcq_target(c, np.float32)
    v64, best64, y64 = R.bcq_target(c, np.float64)
    assert v32.dtype == np.float32 and y32.dtype == np.float32
    assert np.array_equal(v32.astype(np.float64), v64) and np.array_equal(y32.astype(np.float64), y64)      # the mix and y are exact in fp32
    assert np.array_equal(best32, best64)
    if n >= 65:
        assert set(c['pattern']) == {'trip', 'lane', 'last'}
    for b, (kind, js) in enumerate(zip(c['pattern'], c['where'])):
        row = v64[b]
        assert best64[b] == js[0] == min(js)                                     # the expected pick is the smaller planted index
        assert (row[list(js)] == row.max()).all() and (row == row.max()).sum() == len(js)       # planted = all the maxima of the row
        if kind == 'trip':
            assert js[1] == js[0] + 64
        elif kind == 'lane':
            assert js[0] < js[1] and js[1] % 64 < js[0] % 64
        elif kind == 'near':
            assert js[0] < js[1] < 64
        else:
            assert js == (n - 1,)
    if twin and n > 1:
        tie = [js for js in c['where'] if len(js) == 2][0]
        q1, q2 = c['q1'].reshape(B, n), c['q2'].reshape(B, n)
        b = [i for i, js in enumerate(c['where']) if js == tie][0]
        assert (q1[b, tie[0]], q2[b, tie[0]]) != (q1[b, tie[1]], q2[b, tie[1]])    # equal mixes of different pairs


def test_overflow_rows_tell_the_stabilised_logsumexp_from_the_plain_one():
    case = [c for c in R.CQL_CASES if c[2]][0]
    B, m, _ = case
    c = R.cql_inputs(*case)
    ref = R.cql_critic(c['q1'], c['q2'], c['offs'], m, c['y'], c['aw'], np.float64)
    for k in ('td', 'lse', 'q0', 'dq1', 'dq2'):
        assert np.isfinite(ref[k]).all(), k
    f32 = R.cql_critic(c['q1'], c['q2'], c['offs'], m, c['y'], c['aw'], np.float32)
    assert np.isfinite(f32['lse']).all() and np.isfinite(f32['dq1']).all()      # the stabilised form in fp32 is fine
    tiny = np.finfo(np.float32).tiny
    for q in (c['q1'], c['q2']):
        naive = R.naive_lse32(q, c['offs'], B, m)
        x = (q.reshape(B, m) - c['offs'].reshape(B, m))[:, 1:]
        for row, level in R.CQL_OVERFLOW_ROWS:
            if level > 0:
                assert not np.isfinite(naive[row]), (row, naive[row])         # exp overflows: inf
            else:
                # exp underflows the normal range (5e-42: a dozen significand bits left, or zero where denormals are flushed)
                assert (np.exp(x[row].astype(np.float64)) < tiny).all()
        plain = [r for r in range(B) if r not in [row for row, _ in R.CQL_OVERFLOW_ROWS]]
        assert np.isfinite(naive[plain]).all()


def test_every_yardstick_is_a_finite_nonzero_number():
    """the float32 evaluation of each reference on the very inputs of its case: the table the GPU bars are BAR_FACTOR x of"""
    rows = []
    for name, table in (('leaf kernels', R.leaf_yardsticks()), ('networks', R.amlp_yardsticks())):
        for key, outs in table.items():
            worst = max(e for e, _ in outs.values())
            assert np.isfinite(worst) and worst > 0, (key, outs)
            for k, (e, s) in outs.items():
                assert np.isfinite(e) and np.isfinite(s) and s > 0, (key, k, e, s)
            rows.append('%-28s %s' % (key, '  '.join('%s %.2e/%.2e' % (k, e, s) for k, (e, s) in outs.items())))
    print('\nyardstick = max |float32 - float64| / scale = max |float64| per output (bar: %g x yardstick, floor %.2e x scale)' % (R.BAR_FACTOR, R.FLOOR))
    print('\n'.join(rows))
    assert len(rows) == len(R.CVAE_CASES) + len(R.CRITIC_MSE_N) + 3 * len(R.SQUASHED_A) + len(R.SAC_CASES) + 2 * len(R.CQL_CASES) + len(R.AMLP_CASES)


def test_exact_leaf_references_are_decided_by_their_inputs():
    """twin_min on tied rows, the clamp masks: the piecewise outcomes the GPU test compares exactly"""
    for B in (1, 257):
        q1, q2, tied = R.twin_min_inputs(B)
        assert tied.sum() >= 1 and (q1[tied] == q2[tied]).all() and (q1[~tied] != q2[~tied]).all()
        qmin, d1, d2 = R.twin_min(q1, q2)
        assert (d1[tied] != 0).all() and (d2[tied] == 0).all() and ((d1 != 0) ^ (d2 != 0)).all()
        assert qmin.dtype == np.float32 and d1.dtype == np.float32
    for case in R.CVAE_CASES[::2]:
        c = R.cvae_inputs(*case)
        inside = R.cvae(c['enc'], c['eps'], c['y'], c['a'], c['dz'], c['beta'], np.float64)[1]
        L = case[2]
        raw = c['enc'][:, L:]
        assert ((raw < R.LO).any() and (raw > R.HI).any()) or raw.size < 20
        if raw.size >= 100:
            assert 0.1 < (~inside).mean() < 0.3                                  # about a fifth is clamped
        assert not np.isin(raw, (np.float32(R.LO), np.float32(R.HI))).any()      # nothing sits on a bound: fp32 and fp64 agree on the mask


def test_stale_transposes_cannot_hide_inside_the_gradient_bar():
    """A3: the float64 action gradient under P0 and under P1 differ by far more than 100 x the 2e-3 gradient bar"""
    import torch
    P0, P1 = R.stale_pair()
    x, a, w = R.amlp_inputs(266, 32, 1, 36, 78)
    d0 = R.amlp_eval(P0, 'none', x, a, w, torch.float64)['dact']
    d1 = R.amlp_eval(P1, 'none', x, a, w, torch.float64)['dact']
    assert np.abs(d0 - d1).max() > 100 * 2e-3 * np.abs(d1).max(), (np.abs(d0 - d1).max(), np.abs(d1).max())
