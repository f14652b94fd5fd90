#!/usr/bin/env python
"""One arm of the same-box A/B protocol of profiles/r16_ab.md / r17_ab.md: a fresh process builds the env with bench.py's own
make_config / build_env and times, between two synchronisations (bench.timed_episodes),
    default   3 + 20 episode-batches of the default workload (B = 4096, T = 9, offline_action replay, 2048 cached lines),
    distinct  2 + 10 episode-batches of the all-distinct workload (is_eval, cache_size = B),
    random    3 + 20 episode-batches under a uniformly random LEGAL discrete policy (seeded; the observation-side mask decides what
              is legal): every class of duplicate envs splits within a few steps, so the carried partition's resolve pass runs at
              full size - a workload bench.py does not have.
Prints one line `ARM <name> <workload> <ms per episode-batch>` per workload.
    python tools/ab_carry.py --name branch
    python tools/ab_carry.py --name off --no-carry                      (r19: --name off --kernels no_lazy_expand)
    python tools/ab_carry.py --name serial --no-step-overlap            (r26: consecutive transitions on the caller's stream)
    python tools/ab_carry.py --name noreset --no-reset-lane             (r27: each half of DESIGN 39 off alone; --no-reward-lane)
    python tools/ab_carry.py --name noahead --no-replay-ahead           (r28: every replay transition scores its own row)
    python tools/ab_carry.py --name nobeside --no-reward-beside         (r29: the reward step behind the group forward, on lane 0)
    python tools/ab_carry.py --name parent --tree tools/_ab/parent      (another tree with its own library and Python)"""
import argparse
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--name', default='branch')
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--workloads', default='default,distinct,random')
    ap.add_argument('--no-carry', action='store_true', help="config['no_partition_carry']")
    ap.add_argument('--no-step-overlap', action='store_true', help="config['no_step_overlap'] (profiles/r26_ab.md)")
    ap.add_argument('--no-reset-lane', action='store_true', help="config['no_reset_lane'] (profiles/r27_ab.md)")
    ap.add_argument('--no-reward-lane', action='store_true', help="config['no_reward_lane'] (profiles/r27_ab.md)")
    ap.add_argument('--no-replay-ahead', action='store_true', help="config['no_replay_ahead'] (profiles/r28_ab.md)")
    ap.add_argument('--no-reward-beside', action='store_true', help="config['no_reward_beside'] (profiles/r29_ab.md)")
    ap.add_argument('--kernels', default=None, help="config['scorer_kernels'] (e.g. no_lazy_expand: the `off` arm of profiles/r19_lazy_ab.md)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import tempfile
    import torch
    import bench
    torch.cuda.set_device(0)
    args = argparse.Namespace(env='slate', log_records=8193, batch=4096, horizon=9, scorer='auto')
    for w in a.workloads.split(','):
        workdir = tempfile.mkdtemp(prefix='rl4rs_ab_')
        cfg, _ = bench.make_config(args, workdir, 0)
        if w == 'distinct':
            cfg.update({'is_eval': True, 'cache_size': args.batch})
        if a.no_carry:
            cfg['no_partition_carry'] = True
        if a.no_step_overlap:
            cfg['no_step_overlap'] = True
        if a.no_reset_lane:
            cfg['no_reset_lane'] = True
        if a.no_reward_lane:
            cfg['no_reward_lane'] = True
        if a.no_replay_ahead:
            cfg['no_replay_ahead'] = True
        if a.no_reward_beside:
            cfg['no_reward_beside'] = True
        if a.kernels is not None:
            cfg['scorer_kernels'] = a.kernels
        env = bench.build_env(cfg, False)
        env.seed(1000)
        env.sim._recData.store.preload(torch.device('cuda', 0))
        T = args.horizon
        fn = None
        if w == 'random':
            gen = torch.Generator(device='cuda')
            gen.manual_seed(17)

            def fn(env, T):
                env.reset()
                for _ in range(T):
                    legal = env.samples._obs_mask().to(torch.float32)
                    act = torch.multinomial(legal, 1, generator=gen).flatten().to(torch.int32)
                    obs, reward, done, info = env.step(act)
                return obs, reward
        warm, steps = (2, 10) if w == 'distinct' else (3, 20)
        dt = bench.timed_episodes(env, T, steps, warmup=warm, fn=fn)
        print('ARM %s %s %.3f' % (a.name, w, dt / steps * 1e3), flush=True)
        del env


if __name__ == '__main__':
    main()
