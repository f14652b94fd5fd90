"""GPU: the on-device Rainbow at the ends of what rl4rs_distq_create admits (tests/test_gpu_rainbow.py runs one net width, atoms in
{2, 5, 8, 51}, A in {50, 75, 284} and N >= 77), against the float64 restatement in tests/rainbow_ref.py.  The bodies of the checks
are tests/rainbow_gpu.py's, the ones tests/test_gpu_rainbow.py runs.

Cases (od, A, atoms, N, dueling, double_q, masked, trunk, sh) of rainbow_ref.SHAPE_CASES and what each enters:
    0  (  24,   2, 64,    33, 1, 1, 0,   32,  32)   A = 2 (min(ac, A) binds in the head's LDS stride), atoms = 64 (AP = 64, no idle lane),
                                                    narrowest trunk and streams (two trips of the head's 16-wide k loop, a half-idle wave in
                                                    k_distq_wa2_grad), one row in a second 32-row head tile
    1  ( 100, 512,  3,    65, 1, 1, 1,   64, 256)   A = 512 (the 8-trip SoftQ prefix, the largest sQ), SH = 256 (the largest sHa), AP = 4
                                                    with one idle lane per group, masked
    2  (2048,  65, 33,    31, 0, 0, 1, 1024,  64)   widest obs and trunk, atoms = 33 (AP = 64 with 31 idle lanes), A = 65 (one action in the
                                                    second wave trip), no value stream, the target net picks a*, 31 rows
    3  (  40, 130, 16,     1, 1, 1, 0,   96,  96)   one row, AT == AP, widths that are no power of two (a ragged second trip of
                                                    k_distq_wa2_grad)
    4  (   8,   4,  2, 16500, 1, 1, 0,   32,  32)   ceil(N / 256) = 65 > chunk_cap = 64: the re-chunked sample-axis reductions

Error bars: rainbow_ref.shape_yardstick - the worst of the fp32 eager-torch CPU run against float64 over seeds 0, 1, 2 of each case,
no figure counted for less than one fp32 rounding of the quantity's scale - times BAR_FACTOR = 4; the a* / greedy gap bar is ten
times the Q bar.  Measured max errors (yardstick / bar / the device's, MI355X):

    case    Q yardstick / bar / device       td yardstick / bar / device      gradient yardstick / bar / device
    0       9.25e-5 / 3.70e-4 / 1.39e-4      1.54e-6 / 6.16e-6 / 7.34e-7      9.19e-7 / 3.68e-6 / 2.47e-7
    1       1.17e-6 / 4.68e-6 / 9.99e-7      4.18e-7 / 1.67e-6 / 2.56e-7      3.02e-7 / 1.21e-6 / 1.95e-7
    2       5.98e-7 / 2.39e-6 / 7.68e-7      9.58e-7 / 3.83e-6 / 5.63e-7      1.25e-6 / 5.00e-6 / 6.02e-7
    3       1.25e-4 / 5.00e-4 / 1.15e-4      1.90e-7 / 7.60e-7 / 1.26e-7      1.54e-6 / 6.16e-6 / 1.05e-6
    4       2.12e-4 / 8.48e-4 / 1.60e-4      4.46e-7 / 1.78e-6 / 3.72e-7      5.96e-8 / 2.38e-7 / 2.35e-7

(rainbow_ref.MEASURED_SHAPES holds the yardsticks.  The device's Q error is that of the Q rows rl4rs_distq_act / rl4rs_distq_greedy
return; the loss has no Q output of its own.)  The last case's gradient sits at 0.99 of its bar: its yardstick is the 2^-24 floor, and
k_distq_wa2_grad adds the ~4100 rows that took an action in row order, one fp32 chain, which is where the 2.35e-7 comes from (dWa2;
dba2 2.0e-7, every other block under 1e-7).  The sum is bit-identical from run to run.

The inputs keep every stream pre-activation of s rainbow_ref.shape_margin away from 0: RELU_MARGIN, or 4 x the case's own measured
pre-activation error where that is more (the 1024-wide trunk: 1.3e-5).  tests/test_rainbow_host.py confirms on the CPU, with the
restatement alone, that every case stays inside the near-tie and CDF-edge caps."""
import functools

import numpy as np
import pytest

import rainbow_gpu as G
import rainbow_ref as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(i):
    """(inputs, float64 reference without teacher forcing) of case i: computed once, shared, never modified."""
    c = R.shape_case(i)
    return c, G.reference(c)


def _bars(i):
    return G.bars_of(R.MEASURED_SHAPES[i])


@pytest.mark.parametrize('i', range(len(R.SHAPE_CASES)))
def test_loss_and_gradient_match_the_restatement(i):
    c, ref0 = _case(i)
    G.check_loss_and_gradient(c, ref0, _bars(i))


@pytest.mark.parametrize('i', [0, 1])
def test_dueling_gradient_sums_to_zero_over_the_actions(i):
    """A = 2 (half of every column's gradient is the -1 / A term) and A = 512"""
    c, ref0 = _case(i)
    assert c['dm'].A in (2, 512)
    G.check_dueling_gradient_sums_to_zero(c, ref0)


@pytest.mark.parametrize('i,temperature', [(0, 1.0), (1, 1.0), (2, 2.0)])
def test_acting_softq_draw_and_greedy(i, temperature):
    c, _ = _case(i)
    G.check_acting(c, _bars(i)[0], temperature)


@pytest.mark.parametrize('i', [3, 4])
def test_q_rows_match_the_restatement(i):
    """The head's Q rows of the two cases that take no SoftQ test (one row; 16500 rows of four actions), greedy only."""
    c, _ = _case(i)
    dm, q_bar = c['dm'], _bars(i)[0]
    dq = G.net(c, c['N'])
    a, q = dq.greedy(G.to_device(c['obs']), None, want_q=True)
    q_ref = R.forward(c['flat'], c['obs'], dm)[2]
    err = np.abs(q.cpu().numpy().astype(np.float64) - q_ref).max()
    print('Q err %.3g (bar %.3g)' % (err, q_bar))
    assert err < q_bar
    top = np.sort(q_ref, axis=1)[:, -2:]
    firm = (top[:, 1] - top[:, 0]) >= 10.0 * q_bar
    assert (~firm).sum() <= 0.01 * c['N']
    assert np.array_equal(a.cpu().numpy()[firm], q_ref.argmax(axis=1)[firm])


def test_row_count_beyond_max_rows_is_refused():
    """a handle made for 33 rows refuses 34 in act, greedy and loss_grad, before anything is launched"""
    from rl4rs_amd._lib import Rl4rsHipError
    c, _ = _case(0)
    assert c['N'] == 33
    dq = G.net(c, 33)
    more = lambda x: G.to_device(np.concatenate([x, x[:1]]))
    d = dict((k, more(c[k])) for k in ('obs', 'nobs', 'done', 'act', 'rew', 'w'))
    tflat = G.to_device(c['tflat'])
    for call in (lambda: dq.act(d['obs']), lambda: dq.greedy(d['obs']),
                 lambda: dq.loss_grad(tflat, d['obs'], d['act'], d['rew'], d['done'], d['nobs'], None, weights=d['w'])):
        with pytest.raises(Rl4rsHipError, match='max_rows'):
            call()
    dq.act(d['obs'][:33])                                                       # the handle's own row count still runs
