"""float64 numpy restatement of the offline scores (rl4rs_amd/scorers.py): d3rlpy 0.91's metrics/scorer.py
formulas over per-transition columns, one episode and one window of 1024 transitions at a time.  Test infrastructure only."""
import numpy as np

WINDOW_SIZE = 1024
NAMES = ('td_error', 'discounted_sum_of_advantage', 'average_value_estimation', 'initial_state_value_estimation', 'soft_opc',
         'discrete_action_match', 'discrete_action_match_mask', 'continuous_action_diff')


def _f64(cols, name):
    v = cols.get(name)
    return None if v is None else np.asarray(v, dtype=np.float64).reshape(-1)


def scores(starts, cols, gamma=1.0, return_threshold=None):
    """``starts`` int [E + 1]; ``cols``: dict of per-transition arrays (qd, qp, qn, r_td, r_raw, ter, a, a_pi, a_mask, diff; any may
    be missing) -> dict of the eight scores; a score whose columns are missing is NaN."""
    starts = np.asarray(starts, dtype=np.int64)
    E = len(starts) - 1
    n = int(starts[-1] - starts[0])
    qd, qp, qn, r_td, r_raw, ter, diff = [_f64(cols, k) for k in ('qd', 'qp', 'qn', 'r_td', 'r_raw', 'ter', 'diff')]
    a, a_pi, a_mask = [None if cols.get(k) is None else np.asarray(cols[k]).reshape(-1).astype(np.int64) for k in ('a', 'a_pi', 'a_mask')]
    out = {k: float('nan') for k in NAMES}
    if qd is not None and qn is not None and r_td is not None and ter is not None:
        out['td_error'] = float(np.sum((qd - (r_td + gamma * qn * (1.0 - ter))) ** 2) / n)
    if qd is not None and qp is not None:
        total = 0.0
        for e in range(E):
            for lo in range(int(starts[e]), int(starts[e + 1]), WINDOW_SIZE):
                hi = min(lo + WINDOW_SIZE, int(starts[e + 1]))
                adv = qd[lo:hi] - qp[lo:hi]
                S = 0.0
                for j in range(hi - lo - 1, -1, -1):
                    S = adv[j] if j == hi - lo - 1 else adv[j] + gamma * S
                    total += S
        out['discounted_sum_of_advantage'] = total / n
    if qp is not None:
        out['average_value_estimation'] = float(np.sum(qp) / n)
        out['initial_state_value_estimation'] = float(np.sum(qp[starts[:-1]]) / E)
    if qd is not None and r_raw is not None and return_threshold is not None:
        ok = np.zeros(len(qd), dtype=bool)
        for e in range(E):
            ok[starts[e]:starts[e + 1]] = np.sum(r_raw[starts[e]:starts[e + 1]]) >= return_threshold
        out['soft_opc'] = float(np.sum(qd[ok]) / ok.sum() - np.sum(qd) / n) if ok.any() else float('nan')
    if a is not None and a_pi is not None:
        out['discrete_action_match'] = float(np.sum(a == a_pi) / n)
    if a is not None and a_mask is not None:
        out['discrete_action_match_mask'] = float(np.sum(a == a_mask) / n)
    if diff is not None:
        out['continuous_action_diff'] = float(np.sum(diff) / n)
    return out


def starts_of(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])


def random_columns(lengths, seed, A=284):
    """seeded columns for episodes of the given lengths: every column of ``scores``"""
    rs = np.random.RandomState(seed)
    n = int(np.sum(lengths))
    ter = np.zeros(n, dtype=np.float32)
    ter[starts_of(lengths)[1:] - 1] = 1.0
    a = rs.randint(0, A, size=n).astype(np.int32)
    a_pi = np.where(rs.rand(n) < 0.4, a, rs.randint(0, A, size=n)).astype(np.int32)
    a_mask = np.where(rs.rand(n) < 0.6, a, rs.randint(0, A, size=n)).astype(np.int32)
    return dict(qd=rs.normal(3.0, 2.0, n).astype(np.float32), qp=rs.normal(3.5, 2.0, n).astype(np.float32),
                qn=rs.normal(3.2, 2.0, n).astype(np.float32), r_td=rs.normal(0.0, 1.0, n).astype(np.float32),
                r_raw=(rs.rand(n) * 20.0).astype(np.float32), ter=ter, a=a, a_pi=a_pi, a_mask=a_mask,
                diff=rs.rand(n) * 4.0)
