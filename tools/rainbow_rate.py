#!/usr/bin/env python
"""Speed of the on-device Rainbow learner (one GPU).

  update   the steady-state update at N = 1024, the reference's net (256 -> 256 -> 256 -> 128 | 128 -> 284 x 8 | 8, dueling), n_step 3,
           prioritized replay over a filled 73 728-row memory (two rollouts of B = 4096 x T = 9): n-step sample + gather -> loss /
           gradient -> per-variable-clipped Adam -> priority update.  HIP (rl4rs_replay_sample_nstep / rl4rs_distq_loss_grad /
           rl4rs_distq_adam_step_clip_by_var) against the SAME update written in eager torch on the GPU (float64 cumsum +
           searchsorted, index_select, matmul autograd over the full [N, 284, 8] logits, index_add for the projection,
           clip_grad_norm_ per variable, torch.optim.Adam, index_put).  The two alternate in one process, ``--pairs`` pairs, every
           sample = ``--updates`` updates between two synchronisations.
  parts    the HIP update's parts timed alone the same way (sample / loss_grad / adam / priorities).
  loop     SeqSlateRecEnv-v0 B = 4096, T = 32 env-steps/s with RainbowTrainer in the loop at updates_per_rollout 1 and 32.

One JSON line on stdout (and --out FILE).  Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OD, A, ATOMS, VMIN, VMAX, NSTEP = 256, 284, 8, 0.0, 1000.0, 3


def fill(replay, rs, pushes):
    import torch
    R = replay.T * replay.B
    for _ in range(pushes):
        obs = torch.from_numpy(rs.randn(R, OD).astype(np.float32)).cuda()
        mask = torch.full((R, replay.W), -1, dtype=torch.int32, device='cuda')
        act = torch.from_numpy(rs.randint(0, A, size=R).astype(np.int32)).cuda()
        rew = torch.from_numpy(np.where(rs.rand(R) < 0.7, 0.0, rs.rand(R) * 200.0)).cuda()        # many zero rewards, like the env
        replay.push(obs, mask, act, rew)


class TorchRainbow(object):
    """The yardstick: the same update in eager torch on the same memory contents."""

    def __init__(self, replay, flat, B, T, alpha=0.6, beta=0.4, lr=5e-4, clip=40.0, gamma=1.0):
        import torch
        from rl4rs_amd.nets.distq import split, NAMES
        self.t = torch
        n = replay.rows
        self.n, self.B, self.T, self.alpha, self.beta, self.clip, self.gamma = n, B, T, alpha, beta, clip, gamma
        self.obs = replay.column('obs')[:n].clone()
        self.act = replay.column('action')[:n].to(torch.int64)
        self.rew = replay.column('reward')[:n].clone()
        self.prio = replay.column('priority')[:n].clone()
        f = torch.from_numpy(flat).cuda()
        parts = split(f, OD, A, ATOMS)
        self.params = [parts[k].clone().requires_grad_(True) for k in NAMES]
        self.target = [p.detach().clone() for p in self.params]
        self.opt = torch.optim.Adam(self.params, lr=lr, eps=1e-8)
        self.gen = torch.Generator(device='cuda')
        self.gen.manual_seed(0)
        self.z = torch.linspace(VMIN, VMAX, ATOMS, device='cuda')
        self.dz = (VMAX - VMIN) / (ATOMS - 1)

    def dist(self, prm, x):
        t = self.t
        W1, b1, W2, b2, Wa1, ba1, Wa2, ba2, Wv1, bv1, Wv2, bv2 = prm
        h = t.tanh(t.tanh(x @ W1 + b1) @ W2 + b2)
        adv = (t.relu(h @ Wa1 + ba1) @ Wa2 + ba2).reshape(-1, A, ATOMS)
        v = t.relu(h @ Wv1 + bv1) @ Wv2 + bv2
        return v[:, None, :] + adv - adv.mean(dim=1, keepdim=True)

    def update(self, M):
        t = self.t
        c = t.cumsum(self.prio, 0)
        total = c[-1]
        u = t.rand(M, device='cuda', generator=self.gen, dtype=t.float64)
        idx = t.searchsorted(c, u * total, right=True).clamp_(max=self.n - 1)
        p = self.prio.index_select(0, idx)
        w = ((self.n * p / total) ** -self.beta / (self.n * self.prio.min() / total) ** -self.beta).to(t.float32)
        step = (idx % (self.T * self.B)) // self.B
        k = (self.T - step).clamp(max=NSTEP)
        done = step + NSTEP >= self.T
        R = t.zeros(M, dtype=t.float64, device='cuda')
        for j in range(NSTEP):
            R = R + t.where(j < k, self.rew.index_select(0, (idx + j * self.B).clamp_(max=self.n - 1)).to(t.float64) * self.gamma ** j, 0.0)
        R = R.to(t.float32)
        nxt = t.where(done, idx, (idx + k * self.B).clamp_(max=self.n - 1))
        obs, nobs = self.obs.index_select(0, idx), self.obs.index_select(0, nxt)
        rows = t.arange(M, device='cuda')
        with t.no_grad():
            astar = (t.softmax(self.dist(self.params, nobs), dim=2) * self.z).sum(dim=2).argmax(dim=1)
            pn = t.softmax(self.dist(self.target, nobs)[rows, astar], dim=1)
            r_tau = t.where(done[:, None], R[:, None].expand(M, ATOMS), R[:, None] + self.gamma ** NSTEP * self.z[None, :]).clamp(VMIN, VMAX)
            b = (r_tau - VMIN) / self.dz
            lo, up = b.floor(), b.ceil()
            eq = (up - lo < 0.5).to(t.float32)
            m = t.zeros(M, ATOMS, device='cuda')
            m.scatter_add_(1, lo.long(), pn * (up - b + eq))
            m.scatter_add_(1, up.long(), pn * (b - lo))
        la = self.dist(self.params, obs)[rows, self.act.index_select(0, idx)]
        td = -(m * t.log_softmax(la, dim=1)).sum(dim=1)
        loss = (w * td).mean()
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
    from rl4rs_amd.device import DeviceDistQ, DeviceReplay
    from rl4rs_amd.nets.distq import init_distq_params
    B, T, M = 4096, 9, args.rows
    rs = np.random.RandomState(0)
    replay = DeviceReplay(OD, A, T, B, buffer_size=100000, alpha=0.6)
    fill(replay, rs, 2)
    assert replay.rows == 73728
    flat = init_distq_params(OD, A, ATOMS, seed=1)
    flat = flat + (rs.randn(len(flat)) * 0.03).astype(np.float32)
    replay.set_priorities(torch.from_numpy(rs.rand(replay.rows) * 2.0 + 0.01))
    ref = TorchRainbow(replay, flat, B, T)
    net = DeviceDistQ(OD, A, max_rows=M, num_atoms=ATOMS, v_min=VMIN, v_max=VMAX, params=flat)
    target = net.params()
    batch = replay.new_batch(M)
    grad = torch.empty(net.n_params, dtype=torch.float32, device='cuda')
    td = torch.empty(M, dtype=torch.float32, device='cuda')
    step = [0]

    def sample():
        step[0] += 1
        return replay.sample(M, prioritized=True, beta=0.4, seed=1, step=step[0], out=batch, n_step=NSTEP, gamma=1.0)

    def loss_grad():
        b = batch
        return net.loss_grad(target, b['obs'], b['action'], b['reward'], b['done'], b['next_obs'], None, weights=b['weight'], gamma_n=1.0,
                             double_q=True, grad_out=grad, td_out=td)

    adam = lambda: net.adam_step_clip_by_var(grad, lr=5e-4, var_clip=40.0)
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
    hip = np.array([p[0] for p in pairs])
    tor = np.array([p[1] for p in pairs])
    return dict(rows=M, memory_rows=replay.rows, updates_per_sample=args.updates, unit='us per update',
                pairs=[[round(a, 2), round(b, 2)] for a, b in pairs], hip_median=round(float(np.median(hip)), 2),
                torch_median=round(float(np.median(tor)), 2), ratio_torch_over_hip=round(float(np.median(tor) / np.median(hip)), 2),
                hip_faster_in_every_pair=bool((hip < tor).all()), parts=parts)


def loop_leg(args, updates_per_rollout, steps=3):
    import torch
    import rl4rs_amd
    from rl4rs_amd import synth
    from rl4rs_amd.env.seqslate import SeqSlateRecEnv, SeqSlateState
    from rl4rs_amd.train import RainbowTrainer
    B, T = args.batch, 32
    d = tempfile.mkdtemp(prefix='rainbow_rate_')
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
    tr = RainbowTrainer(env, seed=1000, updates_per_rollout=updates_per_rollout, buffer_size=2 * B * T)
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
    ap.add_argument('--updates', type=int, default=100)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'rainbow_rate.py measures on the GPU only'
    result = dict(tool='rainbow_rate', device=torch.cuda.get_device_name(0), torch=torch.__version__,
                  command='python tools/rainbow_rate.py ' + ' '.join(sys.argv[1:]))
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
