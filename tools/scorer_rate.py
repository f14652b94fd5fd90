#!/usr/bin/env python
"""Time the one-pass offline scorers (rl4rs_amd/scorers.py) against the same scores composed from what existed
before them.

  a  ``scorers.evaluate_scorers`` with every discrete name: each network once per row, ``rl4rs_score_rows``, ``rl4rs_score_episodes``
     (``--chunk-rows N``: with evaluation-sized copies of the networks, timed as a third side)
  b  the scorers one after another the way d3rlpy calls them, from ``predict`` / ``predict_value`` (chunks of the learner's 256 rows),
     ``policy_model.predict_with_mask`` and eager torch float64 reductions: every scorer pushes the rows through the networks again

DiscreteBCQ at its initial parameters, 8192 episodes x 10 rows (the reference's eval stage on SlateRecEnv), A = 284.  Both sides
must agree on every score before anything is timed; then alternating pairs a, b, a, b, ... and the median of each side.

    python tools/scorer_rate.py [--episodes 8192] [--pairs 5] [--chunk-rows 4096] [--out profiles/scorer_rate.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

A, P, OBS, T = 284, 9, 256, 10
D = OBS + P + 1
NAMES = ['td_error', 'discounted_sum_of_advantage', 'average_value_estimation', 'initial_state_value_estimation', 'soft_opc',
         'discrete_action_match', 'discrete_action_match_mask']


def dataset(tab, n_ep, seed=3):
    rs = np.random.RandomState(seed)
    n = n_ep * T
    x = np.zeros((n, D), np.float32)
    x[:, :OBS] = rs.randn(n, OBS)
    loc = np.asarray(tab.location_mask)
    cur = np.arange(n) % T
    for j in range(P):
        ids = rs.choice(np.nonzero(loc[j // 3])[0], size=n)
        x[:, OBS + j] = np.where(cur > j, ids, 0)
    x[:, -1] = cur
    return dict(observations=x, actions=rs.randint(1, A, size=(n, 1)).astype(np.float32), rewards=(rs.rand(n) * 20).astype(np.float32),
                terminals=(cur == T - 1).astype(np.float32))


def chunks(fn, *cols, rows=256):
    return torch.cat([fn(*[c[lo:lo + rows].contiguous() for c in cols]) for lo in range(0, cols[0].shape[0], rows)])


def composed(model, pm, ep, th):
    """the scorers one after another, each from the public calls (d3rlpy's metrics/scorer.py restated on [E, 10] episodes)"""
    obs, act, rew, nxt, ter = ep.columns()
    E = len(ep)
    f64 = torch.float64
    out = {}
    # td_error_scorer
    qd = chunks(model.predict_value, obs, act).to(f64)
    qn = chunks(model.predict_value, nxt, chunks(model.predict, nxt)).to(f64)
    out['td_error'] = float(((qd - (rew.to(f64) + model.gamma * qn * (1.0 - ter.to(f64)))) ** 2).mean())
    # discounted_sum_of_advantage_scorer
    qd = chunks(model.predict_value, obs, act).to(f64)
    qp = chunks(model.predict_value, obs, chunks(model.predict, obs)).to(f64)
    adv = (qd - qp).view(E, T)
    S = torch.zeros_like(adv)
    S[:, T - 1] = adv[:, T - 1]
    for j in range(T - 2, -1, -1):
        S[:, j] = adv[:, j] + model.gamma * S[:, j + 1]
    out['discounted_sum_of_advantage'] = float(S.mean())
    # average_value_estimation_scorer, initial_state_value_estimation_scorer
    qp = chunks(model.predict_value, obs, chunks(model.predict, obs)).to(f64)
    out['average_value_estimation'] = float(qp.mean())
    first = obs.view(E, T, D)[:, 0].contiguous()
    out['initial_state_value_estimation'] = float(chunks(model.predict_value, first, chunks(model.predict, first)).to(f64).mean())
    # soft_opc_scorer
    qd = chunks(model.predict_value, obs, act).to(f64).view(E, T)
    ok = rew.to(f64).view(E, T).sum(dim=1) >= th
    out['soft_opc'] = float(qd[ok].mean() - qd.mean())
    # discrete_action_match_scorer: d3rlpy's, then the reference's
    out['discrete_action_match'] = float((chunks(model.predict, obs) == act).to(f64).mean())
    out['discrete_action_match_mask'] = float((pm.predict_with_mask(obs).to(torch.int32) == act).to(f64).mean())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--episodes', type=int, default=8192)
    ap.add_argument('--pairs', type=int, default=5)
    ap.add_argument('--chunk-rows', type=int, default=4096)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from rl4rs_amd import synth, offline_rl as R, scorers as S
    from rl4rs_amd.data import CatalogTables
    from rl4rs_amd.policy.policy_model import policy_model
    d = tempfile.mkdtemp(prefix='scorer_rate_')
    path = os.path.join(d, 'item_info.csv')
    synth.write_text(path, synth.make_catalog_text(seed=21))
    tab = CatalogTables(path, A, 32)
    cfg = {"maxlen": 64, "batch_size": 2048, "action_size": A, "dense_feature_num": 432, "category_feature_num": 21, "max_steps": 9,
           "page_items": P, "action_emb_size": 32, "iteminfo_file": path, "location_mask": tab.location_mask,
           "special_items": tab.special_items}
    model = R.DiscreteBCQ(cfg, D, batch_size=256, seed=5)
    pm = policy_model(model, cfg)
    ep = S.episodes_from_mdp(dataset(tab, args.episodes))
    ret = np.sort(ep.returns().cpu().numpy())
    th = float(0.5 * (ret[len(ret) // 2 - 1] + ret[len(ret) // 2]))

    sides = {'one_pass': lambda: S.evaluate_scorers(model, ep, NAMES, return_threshold=th, policy=None),
             'composed': lambda: composed(model, pm, ep, th)}
    if args.chunk_rows > model.batch_size:
        sides['one_pass_eval_nets'] = lambda: S.evaluate_scorers(model, ep, NAMES, return_threshold=th, chunk_rows=args.chunk_rows)
    first = {k: f() for k, f in sides.items()}                       # (also the warm-up of every side)
    for k in NAMES:
        a, b = first['one_pass'][k], first['composed'][k]
        # the same float32 network values both ways; the mask rule here runs on the raw Q row, predict_with_mask on its softmax
        tol = 1e-3 if k == 'discrete_action_match_mask' else 1e-9 * abs(b)
        assert abs(a - b) <= tol, 'the two sides disagree on %s: %r vs %r' % (k, a, b)
    times = {k: [] for k in sides}
    for _ in range(args.pairs):
        for k, f in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    res = {'tool': 'scorer_rate', 'episodes': args.episodes, 'rows': ep.n_rows, 'action_size': A, 'pairs': args.pairs,
           'chunk_rows': args.chunk_rows, 'scores': first['one_pass'],
           'seconds_median': {k: float(np.median(v)) for k, v in times.items()}, 'seconds_all': times}
    res['composed_over_one_pass'] = res['seconds_median']['composed'] / res['seconds_median']['one_pass']
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    model.close()


if __name__ == '__main__':
    main()
