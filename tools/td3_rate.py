#!/usr/bin/env python
"""Speed of the on-device TD3 learner (one GPU).

  update   one TD3 update at M = 576 (the reference's train_batch_size at B = 64, T = 9) as ONE library call (rl4rs_td3_update:
           target actor + smoothing, twin target critics, twin critics forward / loss / backward, actor step through the critic,
           one Adam + soft-update launch) against the SAME update written in eager torch on the GPU (matmul autograd,
           torch.optim.Adam eps 1e-7, torch._foreach soft updates), for hiddens [400, 300] (RLlib's default: per-layer GEMMs) and
           [256, 256] (the fused minibatch launches of amlp_fused.hpp).  The two alternate in one process, ``--pairs`` pairs, every
           sample = ``--updates`` updates between two synchronisations; do_actor alternates as policy_delay 2 makes it.  Before anything is
           timed the two sides run three updates from the same parameters and must agree to 2e-4 on every parameter.
  loop     SlateRecEnv-v0 B = 4096, T = 9 (SeqSlate-free) env-steps/s with TD3Trainer in the loop (actor forward + OU exploration +
           masked K-NN step, push, ``updates_per_rollout`` updates at M = 1024) next to the same rollout driven by the logged
           actions without a learner (context for the `conti` replay rate of the README; not a bar).

One JSON line on stdout (and --out FILE).  Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OD, E = 256, 32


class TorchTD3(object):
    """The yardstick: the same update in eager torch."""

    def __init__(self, prm, tau=5e-3, target_noise=0.2, noise_clip=0.5, lr=1e-3):
        import torch
        self.t = torch
        names = ('fc1_w', 'fc1_b', 'fc2_w', 'fc2_b', 'head_w', 'head_b')
        mk = lambda n, grad: [torch.from_numpy(np.ascontiguousarray(prm[n][k])).cuda().requires_grad_(grad) for k in names]
        self.actor, self.q1, self.q2 = mk('actor', True), mk('q1', True), mk('q2', True)
        self.actor_t, self.q1_t, self.q2_t = mk('actor_targ', False), mk('q1_targ', False), mk('q2_targ', False)
        self.copt = torch.optim.Adam(self.q1 + self.q2, lr=lr, eps=1e-7)
        self.aopt = torch.optim.Adam(self.actor, lr=lr, eps=1e-7)
        self.tau, self.tn, self.nc = tau, target_noise, noise_clip

    def mlp(self, p, x, tanh=False):
        t = self.t
        h = t.relu(t.addmm(p[1], x, p[0]))
        h = t.relu(t.addmm(p[3], h, p[2]))
        o = t.addmm(p[5], h, p[4])
        return t.tanh(o) if tanh else o

    def update(self, b, noise, do_actor):
        t = self.t
        with t.no_grad():
            a2 = (self.mlp(self.actor_t, b['next_obs'], True) + (self.tn * noise).clamp_(-self.nc, self.nc)).clamp_(-1.0, 1.0)
            x2 = t.cat([b['next_obs'], a2], dim=1)
            qn = t.minimum(self.mlp(self.q1_t, x2), self.mlp(self.q2_t, x2))[:, 0]
            y = t.where(b['done'] != 0, b['reward'], b['reward'] + qn)
        x = t.cat([b['obs'], b['action']], dim=1)
        closs = (0.5 * (self.mlp(self.q1, x)[:, 0] - y) ** 2 + 0.5 * (self.mlp(self.q2, x)[:, 0] - y) ** 2).mean()
        self.copt.zero_grad(set_to_none=True)
        if do_actor:
            # both gradients from the parameters before the step: the actor's through q1 WITHOUT touching q1's gradient
            a_pi = self.mlp(self.actor, b['obs'], True)
            aloss = -self.mlp([p.detach() for p in self.q1], t.cat([b['obs'], a_pi], dim=1)).mean()
            self.aopt.zero_grad(set_to_none=True)
            aloss.backward()
        closs.backward()
        self.copt.step()
        if do_actor:
            self.aopt.step()
        with t.no_grad():
            for tg, src in ((self.q1_t, self.q1), (self.q2_t, self.q2), (self.actor_t, self.actor)):
                t._foreach_mul_(tg, 1.0 - self.tau)
                t._foreach_add_(tg, [s.detach() for s in src], alpha=self.tau)


def timed(fn, updates):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(updates):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / updates


def update_leg(args, hid):
    import torch
    from rl4rs_amd.offline_rl import init_ddpg_params
    from rl4rs_amd.train import TD3Learner
    M = args.rows
    rs = np.random.RandomState(0)
    prm = dict(actor=init_ddpg_params(OD, 0, E, hid[0], hid[1], seed=1), q1=init_ddpg_params(OD, E, 1, hid[0], hid[1], seed=2),
               q2=init_ddpg_params(OD, E, 1, hid[0], hid[1], seed=3))
    for n in ('actor', 'q1', 'q2'):
        prm[n + '_targ'] = dict((k, v.copy()) for k, v in prm[n].items())
    L = TD3Learner(OD, E, M, actor_hiddens=hid, critic_hiddens=hid, params=prm)
    ref = TorchTD3(prm)
    c = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    done = (rs.rand(M) < 1.0 / 9).astype(np.int32)
    b = dict(obs=c(rs.randn(M, OD).astype(np.float32)), action=c((rs.rand(M, E) * 2 - 1).astype(np.float32)),
             reward=c(rs.rand(M).astype(np.float32)), done=c(done), next_obs=c(rs.randn(M, OD).astype(np.float32)))
    noise = c(rs.randn(M, E).astype(np.float32))
    k = [0, 0]

    def hip_update():
        k[0] += 1
        L.update(b, noise=noise, do_actor=k[0] % 2 == 0)

    def torch_update():
        k[1] += 1
        ref.update(b, noise, k[1] % 2 == 0)

    # faster and different is not faster: three updates on either side from the same parameters, at the size that is timed, must leave
    # every online and target network within the suite's bar for parameters after k Adam steps (2e-4 abs) of the torch update's
    for _ in range(3):
        hip_update()
        torch_update()
    names = ('fc1_w', 'fc1_b', 'fc2_w', 'fc2_b', 'head_w', 'head_b')
    drift = 0.0
    for net, tp in ((L.actor, ref.actor), (L.q1, ref.q1), (L.q2, ref.q2), (L.actor_targ, ref.actor_t), (L.q1_targ, ref.q1_t), (L.q2_targ, ref.q2_t)):
        w = net.weights()
        drift = max([drift] + [float((w[k] - tp[i].detach()).abs().max()) for i, k in enumerate(names)])
    assert drift < 2e-4, 'the HIP update and the torch yardstick disagree after 3 updates: max abs parameter difference %g' % drift
    for _ in range(20):                                   # warm-up: code objects, allocator, autograd graph caches
        hip_update()
        torch_update()
    pairs = []
    for _ in range(args.pairs):
        h = timed(hip_update, args.updates)
        t = timed(torch_update, args.updates)
        pairs.append((h * 1e6, t * 1e6))
    hip = np.array([p[0] for p in pairs])
    tor = np.array([p[1] for p in pairs])
    L.close()
    return dict(hiddens=list(hid), rows=M, updates_per_sample=args.updates, unit='us per update',
                pairs=[[round(a, 2), round(b_, 2)] for a, b_ in pairs], hip_median=round(float(np.median(hip)), 2),
                torch_median=round(float(np.median(tor)), 2), ratio_torch_over_hip=round(float(np.median(tor) / np.median(hip)), 2),
                hip_faster_in_every_pair=bool((hip < tor).all()), max_abs_param_diff_after_3_updates=drift)


def _env(B, T):
    import torch
    import rl4rs_amd
    from rl4rs_amd import synth
    from rl4rs_amd.env.slate import SlateRecEnv, SlateState
    d = tempfile.mkdtemp(prefix='td3_rate_')
    text = synth.make_catalog_text(seed=1234)
    synth.write_text(os.path.join(d, 'item_info.csv'), text)
    synth.write_records(os.path.join(d, 'log.csv'), synth.make_records(8193, seed=1000, special_ids=synth.special_ids_from_text(text)))
    cfg = {"maxlen": 64, "batch_size": B, "action_size": 284, "class_num": 2, "dense_feature_num": 432, "category_feature_num": 21,
           "category_hash_size": 100000, "seq_num": 2, "emb_size": 128, "page_items": 9, "hidden_units": 128, "max_steps": T,
           "action_emb_size": 32, "sample_file": os.path.join(d, 'log.csv'), "iteminfo_file": os.path.join(d, 'item_info.csv'),
           "is_eval": False, "cache_size": 2048, "model_seed": 7, "return_tensors": True, "support_conti_env": True}
    env = rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))
    env.seed(1000)
    env.sim._recData.store.preload(torch.device('cuda', torch.cuda.current_device()))
    return env


def loop_leg(args, updates_per_rollout):
    import torch
    from rl4rs_amd.train import TD3Trainer
    B, T = args.batch, 9
    env = _env(B, T)
    tr = TD3Trainer(env, seed=1000, updates_per_rollout=updates_per_rollout, buffer_size=4 * B * T, random_timesteps=B * T)
    tr.train_iteration()                                  # the random phase, the first updates
    tr.train_iteration()                                  # the actor drives the env from here on
    steps = args.iterations
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.train_iteration()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    tr.close()
    return dict(value=round(B * T * steps / dt, 1), unit='env-steps/s', ms_per_iteration=round(dt / steps * 1e3, 3),
                updates_per_rollout=updates_per_rollout, train_batch_size=tr.M,
                workload='SlateRecEnv-v0 conti B=%d T=%d, actor + OU rollout + push + updates' % (B, T))


def replay_leg(args):
    """The same env driven by its logged continuous actions, no learner: the rollout the learner's loop is measured against."""
    import torch
    B, T = args.batch, 9
    env = _env(B, T)

    def episode():
        env.reset()
        for _ in range(T):
            env.step(env.offline_action)

    episode()
    episode()
    steps = args.iterations
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        episode()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dict(value=round(B * T * steps / dt, 1), unit='env-steps/s', ms_per_iteration=round(dt / steps * 1e3, 3),
                workload='SlateRecEnv-v0 conti B=%d T=%d, logged actions, no learner' % (B, T))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='update,loop')
    ap.add_argument('--rows', type=int, default=576)
    ap.add_argument('--pairs', type=int, default=7)
    ap.add_argument('--updates', type=int, default=2000, help='updates per timed sample (a sample should last a good fraction of a second)')
    ap.add_argument('--iterations', type=int, default=100, help='train iterations / episodes in the timed window of the loop legs')
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'td3_rate.py measures on the GPU only'
    result = dict(tool='td3_rate', device=torch.cuda.get_device_name(0), torch=torch.__version__,
                  command='python tools/td3_rate.py ' + ' '.join(sys.argv[1:]))
    legs = args.legs.split(',')
    if 'update' in legs:
        result['update'] = [update_leg(args, hid) for hid in ((400, 300), (256, 256))]
    if 'loop' in legs:
        result['replay'] = replay_leg(args)
        result['loop'] = [loop_leg(args, k) for k in (1, 8)]
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
