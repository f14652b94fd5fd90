#!/usr/bin/env python
"""Cost of off-policy evaluation next to the plain evaluation loop (one GPU; B = 4096 episodes x 9 steps, DiscreteCQL policy,
SlateRecEnv with support_d3rl_mask + return_tensors, synthetic catalogue and records).

  a  the loop ``predict_with_mask -> step`` alone (batchrl_trainer.evaluate).  Uses only API older than rl4rs_amd/ope.py, so the
     same file times a checkout from before it:  PYTHONPATH=<that checkout> python tools/ope_rate.py --legs a
  b  the same loop inside ``ope_eval`` with ``sample_model=None`` (rewards only)
  c  full ``ope_eval`` with a DiscreteBC behaviour model (pi, mu, q columns and the estimate)
  d  ``OpeLog.estimate`` alone on a filled log

Every figure is host wall time per epoch (reset + 9 steps), each epoch ending in a device synchronise (the estimate's read-back,
or an explicit one).  Leg a times each epoch by itself (n = rounds x epochs samples).  Legs b and c time one whole ``ope_eval`` call
of ``--epochs`` epochs and divide by the epoch count: ONE sample per round (n = rounds), which includes the call's set-up - the
``OpeLog`` handle's create / destroy (two device allocations) and the final prints - spread over its epochs.  Legs a / b / c alternate
round by round in one process, after one warm-up round each; median and p10 / p90 over the samples.  One JSON line on stdout (and
--out FILE)."""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # after PYTHONPATH: another checkout given there wins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='abcd')
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--rounds', type=int, default=12)
    ap.add_argument('--epochs', type=int, default=4, help='epochs per round and leg')
    ap.add_argument('--commit', default='', help='recorded as given (the measured tree need not be a git checkout)')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'ope_rate.py measures on the GPU only'
    import rl4rs_amd
    from rl4rs_amd import offline_rl as R
    from rl4rs_amd import synth
    from rl4rs_amd.env.slate import SlateRecEnv, SlateState
    from rl4rs_amd.policy.policy_model import policy_model
    B, T = args.batch, 9
    d = tempfile.mkdtemp(prefix='ope_rate_')
    text = synth.make_catalog_text(seed=4)
    synth.write_text(os.path.join(d, 'item_info.csv'), text)
    synth.write_records(os.path.join(d, 'log.csv'), synth.make_records(2 * B, pages=1, seed=2, hash_size=2000,
                                                                       special_ids=synth.special_ids_from_text(text)))
    cfg = {"epoch": args.epochs, "maxlen": 64, "batch_size": B, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
           "category_feature_num": 21, "category_hash_size": 2000, "seq_num": 2, "emb_size": 128, "hidden_units": 128, "max_steps": T,
           "sample_file": os.path.join(d, 'log.csv'), "page_items": 9, "action_emb_size": 32,
           "iteminfo_file": os.path.join(d, 'item_info.csv'), "support_d3rl_mask": True, "is_eval": True, "cache_size": B,
           "model_seed": 3, "return_tensors": True}
    env = rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))
    obs_dim = int(env.reset().shape[1])
    cql = R.DiscreteCQL(cfg, obs_dim, batch_size=B, seed=2)
    policy = policy_model(cql, config=cfg)

    def leg_a():
        out = []
        for _ in range(args.epochs):
            t0 = time.perf_counter()
            obs = env.reset()
            total = None
            for _j in range(T):
                action = policy.predict_with_mask(obs)
                obs, reward, done, info = env.step(action)
                total = reward if total is None else total + reward
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
        return out

    legs = {'a': leg_a}
    if set(args.legs) & set('bcd'):
        from rl4rs_amd.ope import OpeLog, ope_eval
        from rl4rs_amd.policy.behavior_model import behavior_model
        bc = R.DiscreteBC(cfg, obs_dim, batch_size=B, seed=1)
        sample_model = behavior_model(cfg, bc)

        def timed_eval(model):
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                ope_eval(cfg, env, policy, sample_model=model)
            torch.cuda.synchronize()
            return [(time.perf_counter() - t0) / args.epochs]

        legs['b'] = lambda: timed_eval(None)
        legs['c'] = lambda: timed_eval(sample_model)

        def leg_d():
            log = OpeLog(B, T)
            log.begin(B, T)
            rs = np.random.RandomState(0)
            for t in range(T):
                pi = rs.uniform(0.02, 0.9, size=B)
                for name, col in (('pi', pi), ('mu', pi * rs.uniform(0.6, 1.6, size=B)), ('q', rs.uniform(0, 10, size=B)),
                                  ('reward', rs.uniform(0, 3, size=B)), ('logged_reward', rs.uniform(0, 3, size=B))):
                    log.record_column(t, name, col)
            log.estimate()
            torch.cuda.synchronize()
            out = []
            for _ in range(args.epochs * 25):
                t0 = time.perf_counter()
                log.estimate()
                out.append(time.perf_counter() - t0)
            log.close()
            return out
        legs['d'] = leg_d

    order = [k for k in 'abcd' if k in args.legs]
    for k in order:
        legs[k]()                                        # warm-up round: code objects, allocator, caches
    times = dict((k, []) for k in order)
    for _ in range(args.rounds):
        for k in order:
            times[k].extend(legs[k]())
    result = dict(tool='ope_rate', batch=B, steps=T, rounds=args.rounds, epochs_per_round=args.epochs, commit=args.commit,
                  device=torch.cuda.get_device_name(0), torch=torch.__version__, unit='ms per epoch (d: ms per estimate call)')
    for k in order:
        v = np.asarray(times[k]) * 1e3
        result[k] = dict(median=round(float(np.median(v)), 4), p10=round(float(np.percentile(v, 10)), 4),
                         p90=round(float(np.percentile(v, 90)), 4), n=int(v.size))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
