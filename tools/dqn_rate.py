#!/usr/bin/env python
"""Speed of the on-device DQN learner (one GPU).

  update   the steady-state update at N = 1024, default net (256 -> 64 -> 284), prioritized replay over a filled 73 728-row memory
           (two rollouts of B = 4096 x T = 9): sample + gather -> loss / gradient -> per-variable-clipped Adam -> priority update.
           HIP (rl4rs_replay_* / rl4rs_policy_dqn_loss_grad / ..._adam_step_clip_by_var) against the SAME update written in eager
           torch from API older than the DQN entry points (float64 cumsum + searchsorted, index_select, matmul autograd,
           clip_grad_norm_ per variable, torch.optim.Adam, index_put).  The two alternate in one process, ``--pairs`` pairs, every
           sample = ``--updates`` updates between two synchronisations.
  parts    the HIP update's parts timed alone the same way (sample / loss_grad / adam / priorities) and the bytes the gather moves.
  loop     SeqSlateRecEnv-v0 B = 4096, T = 32 env-steps/s with DQNTrainer in the loop at updates_per_rollout 1 and 32 (context for
           the replay rate of the README; not a bar).

One JSON line on stdout (and --out FILE).  Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OD, HID, A = 256, 64, 284


def fill(replay, rs, pushes):
    import torch
    R = replay.T * replay.B
    W = replay.W
    for _ in range(pushes):
        obs = torch.from_numpy(rs.randn(R, OD).astype(np.float32)).cuda()
        mask = torch.from_numpy(rs.randint(-2 ** 31, 2 ** 31, size=(R, W), dtype=np.int64).astype(np.int32)).cuda()
        mask[:, 0] |= 1
        act = torch.from_numpy(rs.randint(0, A, size=R).astype(np.int32)).cuda()
        rew = torch.from_numpy(rs.rand(R) * 2.0).cuda()
        replay.push(obs, mask, act, rew)


class TorchDQN(object):
    """The yardstick: the same update in eager torch on the same memory contents."""

    def __init__(self, replay, flat, B, alpha=0.6, beta=0.4, lr=5e-4, clip=40.0, gamma=1.0):
        import torch
        self.t = torch
        n = replay.rows
        self.n, self.B, self.alpha, self.beta, self.clip, self.gamma = n, B, alpha, beta, clip, gamma
        self.obs = replay.column('obs')[:n].clone()
        bits = replay.column('mask')[:n]
        sh = torch.arange(32, device='cuda', dtype=torch.int32)
        self.maskadd = torch.where(((bits[:, :, None] >> sh) & 1).reshape(n, -1)[:, :A] > 0, 0.0, -3.4028235e38).to(torch.float32)
        self.act = replay.column('action')[:n].to(torch.int64)
        self.rew = replay.column('reward')[:n].clone()
        self.done = replay.column('done')[:n] != 0
        self.prio = replay.column('priority')[:n].clone()
        from rl4rs_amd.nets.policy import split
        f = torch.from_numpy(flat).cuda()
        self.params = [p.clone().requires_grad_(True) for p in split(f, OD, HID, A)]
        self.target = [p.detach().clone() for p in self.params]
        self.opt = torch.optim.Adam(self.params, lr=lr, eps=1e-8)
        self.gen = torch.Generator(device='cuda')
        self.gen.manual_seed(0)

    def q(self, prm, x):
        W1, b1, W2, b2 = prm
        return (self.t.tanh(x @ W1 + b1) @ W2 + b2)[:, :A]

    def update(self, M):
        t = self.t
        c = t.cumsum(self.prio, 0)
        total = c[-1]
        u = t.rand(M, device='cuda', generator=self.gen, dtype=t.float64)
        idx = t.searchsorted(c, u * total, right=True).clamp_(max=self.n - 1)
        p = self.prio.index_select(0, idx)
        w = ((self.n * p / total) ** -self.beta / (self.n * self.prio.min() / total) ** -self.beta).to(t.float32)
        done = self.done.index_select(0, idx)
        nxt = t.where(done, idx, (idx + self.B).clamp_(max=self.n - 1))
        obs, nobs = self.obs.index_select(0, idx), self.obs.index_select(0, nxt)
        madd = self.maskadd.index_select(0, nxt)
        with t.no_grad():
            astar = (self.q(self.params, nobs) + madd).argmax(dim=1, keepdim=True)
            qt = self.q(self.target, nobs).gather(1, astar)[:, 0]
            y = t.where(done, self.rew.index_select(0, idx), self.rew.index_select(0, idx) + self.gamma * qt)
        qsa = self.q(self.params, obs).gather(1, self.act.index_select(0, idx)[:, None])[:, 0]
        td = qsa - y
        loss = (w * t.nn.functional.huber_loss(qsa, y, reduction='none', delta=1.0)).mean()
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        for prm in self.params:
            t.nn.utils.clip_grad_norm_([prm], self.clip)
        self.opt.step()
        self.prio.index_put_((idx,), (td.detach().abs().to(t.float64) + 1e-6) ** self.alpha)


def timed(fn, updates):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(updates):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / updates


def update_legs(args):
    import torch
    from rl4rs_amd.device import DevicePolicy, DeviceReplay
    from rl4rs_amd.nets.policy import init_policy_params
    B, T, M = 4096, 9, args.rows
    rs = np.random.RandomState(0)
    replay = DeviceReplay(OD, A, T, B, buffer_size=100000, alpha=0.6)
    fill(replay, rs, 2)
    assert replay.rows == 73728
    flat = init_policy_params(OD, HID, A, seed=1) + (rs.randn(34973) * 0.05).astype(np.float32)
    replay.set_priorities(torch.from_numpy(rs.rand(replay.rows) * 2.0 + 0.01))
    ref = TorchDQN(replay, flat, B)
    pol = DevicePolicy(OD, HID, A, max_rows=M, params=flat)
    target = pol.params()
    batch = replay.new_batch(M)
    grad = torch.empty(pol.n_params, dtype=torch.float32, device='cuda')
    td = torch.empty(M, dtype=torch.float32, device='cuda')
    step = [0]

    def sample():
        step[0] += 1
        return replay.sample(M, prioritized=True, beta=0.4, seed=1, step=step[0], out=batch)

    def loss_grad():
        b = batch
        return pol.dqn_loss_grad(target, b['obs'], b['action'], b['reward'], b['done'], b['next_obs'], b['next_mask'], weights=b['weight'],
                                 gamma=1.0, double_q=True, grad_out=grad, td_out=td)

    adam = lambda: pol.adam_step_clip_by_var(grad, lr=5e-4, var_clip=40.0)
    prios = lambda: replay.update_priorities(batch['idx'], td)

    def hip_update():
        sample()
        loss_grad()
        adam()
        prios()

    torch_update = lambda: ref.update(M)
    for _ in range(20):                                   # warm-up: code objects, allocator, autograd graph caches
        hip_update()
        torch_update()
    pairs = []
    for _ in range(args.pairs):
        h = timed(hip_update, args.updates)
        t = timed(torch_update, args.updates)
        pairs.append((h * 1e6, t * 1e6))
    parts = dict((k, round(float(np.median([timed(f, args.updates) for _ in range(args.pairs)])) * 1e6, 2))
                 for k, f in (('sample', sample), ('loss_grad', loss_grad), ('adam', adam), ('priorities', prios)))
    gather_bytes = M * (2 * 2 * OD * 4 + 2 * replay.W * 4 + 6 * 4)      # obs + next obs rows, mask words, scalars: read + write
    hip = np.array([p[0] for p in pairs])
    tor = np.array([p[1] for p in pairs])
    return dict(rows=M, memory_rows=replay.rows, updates_per_sample=args.updates, unit='us per update',
                pairs=[[round(a, 2), round(b, 2)] for a, b in pairs], hip_median=round(float(np.median(hip)), 2),
                torch_median=round(float(np.median(tor)), 2), ratio_torch_over_hip=round(float(np.median(tor) / np.median(hip)), 2),
                hip_faster_in_every_pair=bool((hip < tor).all()), parts=parts, gather_bytes_per_sample_call=gather_bytes,
                note='parts.sample = two scan launches + k_replay_sample; its gather share is in the rocprofv3 kernel table')


def loop_leg(args, updates_per_rollout, steps=3):
    import torch
    import rl4rs_amd
    from rl4rs_amd import synth
    from rl4rs_amd.env.seqslate import SeqSlateRecEnv, SeqSlateState
    from rl4rs_amd.train import DQNTrainer
    B, T = args.batch, 32
    d = tempfile.mkdtemp(prefix='dqn_rate_')
    text = synth.make_catalog_text(seed=1234)
    synth.write_text(os.path.join(d, 'item_info.csv'), text)
    synth.write_records(os.path.join(d, 'log.csv'), synth.make_records(8193, pages=4, seed=1000, illegal_frac=0.05,
                                                                       special_ids=synth.special_ids_from_text(text)))
    cfg = {"maxlen": 64, "batch_size": B, "action_size": 284, "class_num": 2, "dense_feature_num": 432, "category_feature_num": 21,
           "category_hash_size": 100000, "seq_num": 2, "emb_size": 128, "page_items": 9, "hidden_units": 128, "max_steps": T,
           "action_emb_size": 32, "sample_file": os.path.join(d, 'log.csv'), "iteminfo_file": os.path.join(d, 'item_info.csv'),
           "is_eval": False, "cache_size": 2048, "model_seed": 7, "return_tensors": True}
    env = rl4rs_amd.make('SeqSlateRecEnv-v0', recsim=SeqSlateRecEnv(cfg, state_cls=SeqSlateState))
    env.seed(1000)
    env.sim._recData.store.preload(torch.device('cuda', torch.cuda.current_device()))
    tr = DQNTrainer(env, seed=1000, updates_per_rollout=updates_per_rollout, buffer_size=2 * B * T)
    tr.train_iteration()
    tr.train_iteration()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.train_iteration()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    tr.close()
    return dict(value=round(B * T * steps / dt, 1), unit='env-steps/s', ms_per_iteration=round(dt / steps * 1e3, 3),
                updates_per_rollout=updates_per_rollout, workload='SeqSlateRecEnv-v0 B=%d T=%d, SoftQ rollout + push + updates' % (B, T))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='update,loop')
    ap.add_argument('--rows', type=int, default=1024)
    ap.add_argument('--pairs', type=int, default=7)
    ap.add_argument('--updates', type=int, default=200)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'dqn_rate.py measures on the GPU only'
    result = dict(tool='dqn_rate', device=torch.cuda.get_device_name(0), torch=torch.__version__,
                  command='python tools/dqn_rate.py ' + ' '.join(sys.argv[1:]))
    legs = args.legs.split(',')
    if 'update' in legs:
        result['update'] = update_legs(args)
    if 'loop' in legs:
        result['loop'] = [loop_leg(args, k) for k in (1, 32)]
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
