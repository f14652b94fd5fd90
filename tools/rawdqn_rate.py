#!/usr/bin/env python
"""Speed of one raw-state DQN update (one GPU), in the manner of tools/dqn_rate.py.

  update   one learner step at M = 1024 rows and the default configuration (two 100 000 x 128 tables, 25.9 M parameters) on a fixed
           minibatch of packed records drawn from a filled ring: loss and gradient (rl4rs_rawtrain_dqn_loss_grad) ->
           per-variable-clipped Adam (rl4rs_rawtrain_adam_step_clip_by_var) -> priorities (rl4rs_replay_update_priorities),
           against the SAME update in eager torch on the GPU (embedding gathers, matmul autograd, clip_grad_norm_ per variable,
           torch.optim.Adam over dense gradients, index_put).  Before anything is timed both sides must agree on td and on the
           gradients of the eight dense variables from equal parameters.  The two alternate in one process, ``--pairs`` pairs, every
           sample = ``--updates`` updates between two synchronisations.
  split    event times of one HIP update by stage (rl4rs_rawtrain_profile): the three forwards, the row kernel, the backward, the
           sums of squares, the Adam kernel; the median over ``--pairs`` updates.

One JSON line on stdout (and --out FILE, default profiles/rawdqn_rate.json).  Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(REPO)

CFG = {"maxlen": 64, "action_size": 284, "dense_feature_num": 432, "category_feature_num": 21, "category_hash_size": 100000,
       "seq_num": 2, "emb_size": 128, "hidden_units": 128}
ORDER = ('cat_emb', 'seq_emb', 'dense_w1', 'dense_b1', 'dense_w2', 'dense_b2', 'ctx_w', 'ctx_b', 'head_w', 'head_b')


class TorchRawDQN(object):
    """The yardstick: the same update in eager torch on the same minibatch."""

    def __init__(self, weights, target, prio, lr=5e-4, clip=40.0, gamma=1.0, alpha=0.6):
        import torch
        self.t = torch
        self.params = [weights[k].clone().requires_grad_(True) for k in ORDER]
        self.target = [target[k].clone() for k in ORDER]
        self.opt = torch.optim.Adam(self.params, lr=lr, eps=1e-8)
        self.clip, self.gamma, self.alpha = clip, gamma, alpha
        self.prio = prio.clone()

    def set_batch(self, cfg, b):
        t = self.t
        Dn, Cn, L, S, H, A = (cfg['dense_feature_num'], cfg['category_feature_num'], cfg['maxlen'], cfg['seq_num'],
                              cfg['category_hash_size'], cfg['action_size'])

        def unpack(rec):
            ids = rec.view(t.int32)
            dense = rec[:, :Dn].contiguous()
            cat = ids[:, Dn:Dn + Cn].to(t.int64).clamp_(0, H - 1)
            seqs = [ids[:, Dn + Cn + s * L:Dn + Cn + (s + 1) * L].to(t.int64).clamp_(0, H - 1) for s in range(S)]
            return cat, dense, seqs
        self.s, self.sn = unpack(b['obs']), unpack(b['next_obs'])
        sh = t.arange(32, device=b['obs'].device, dtype=t.int32)
        legal = ((b['next_mask'][:, :, None] >> sh) & 1).reshape(b['next_mask'].shape[0], -1)[:, :A] > 0
        self.maskadd = t.zeros(legal.shape, dtype=t.float32, device=legal.device).masked_fill_(~legal, float(np.finfo(np.float32).min))
        self.act = b['action'].to(t.int64)[:, None]
        self.rew, self.done, self.w, self.idx = b['reward'], b['done'] != 0, b['weight'], b['idx'].to(t.int64)
        self.A = A

    def q(self, prm, x):
        t = self.t
        cat_emb, seq_emb, w1, b1, w2, b2, cw, cb, hw, hb = prm
        cat, dense, seqs = x
        elu = t.nn.functional.elu
        feat = [seq_emb[s].mean(dim=1) for s in seqs]
        d = elu(elu(dense @ w1 + b1) @ w2 + b2)
        ctx = elu(t.cat(feat + [d, cat_emb[cat].mean(dim=1)], dim=1) @ cw + cb)
        return (ctx @ hw + hb)[:, :self.A]

    def loss_grad(self):
        t = self.t
        with t.no_grad():
            astar = (self.q(self.params, self.sn) + self.maskadd).argmax(dim=1, keepdim=True)
            qt = self.q(self.target, self.sn).gather(1, astar)[:, 0]
            y = t.where(self.done, self.rew, self.rew + self.gamma * qt)
        qsa = self.q(self.params, self.s).gather(1, self.act)[:, 0]
        td = qsa - y
        loss = (self.w * t.nn.functional.huber_loss(qsa, y, reduction='none', delta=1.0)).mean()
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        return td.detach()

    def update(self):
        t = self.t
        td = self.loss_grad()
        for prm in self.params:
            t.nn.utils.clip_grad_norm_([prm], self.clip)
        self.opt.step()
        self.prio.index_put_((self.idx,), (td.abs().to(t.float64) + 1e-6) ** self.alpha)


def timed(fn, updates):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(updates):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / updates


def run(args):
    import torch
    from rl4rs_amd.device import DeviceRawTrainer, DeviceReplay
    from rl4rs_amd.nets.rawpolicy import init_rawpolicy_weights
    cfg, M = CFG, args.rows
    H, A, T, B = cfg['category_hash_size'], cfg['action_size'], 9, 1024
    rs = np.random.RandomState(0)
    w = init_rawpolicy_weights(cfg, seed=1, emb_scale=0.5, head_std=1.0, bias_noise=0.2)
    pol = DeviceRawTrainer(cfg, w, max_rows=max(M, B))
    REC = pol.record_words
    # a filled ring of one rollout of packed records
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    R = T * B
    rec = pol.pack_records(t(rs.randint(0, H, size=(R, cfg['category_feature_num'])).astype(np.int32)),
                           t(np.abs(rs.randn(R, cfg['dense_feature_num']) * 2).astype(np.float32)),
                           [t(rs.randint(0, H, size=(R, cfg['maxlen'])).astype(np.int32)) for _ in range(cfg['seq_num'])])
    replay = DeviceReplay(REC, A, T, B, buffer_size=R, alpha=0.6)
    mask = t(rs.randint(-2 ** 31, 2 ** 31, size=(R, replay.W), dtype=np.int64).astype(np.int32))
    mask[:, 0] |= 1
    replay.push(rec, mask, t(rs.randint(0, A, size=R).astype(np.int32)), t(rs.rand(R) * 2.0))
    replay.set_priorities(torch.from_numpy(rs.rand(R) * 2.0 + 0.01))
    batch = replay.sample(M, prioritized=True, beta=0.4, seed=1, step=1)
    target = pol.params() + 0.01 * torch.randn(pol.n_params, device='cuda', generator=torch.Generator(device='cuda').manual_seed(3))
    td = torch.empty(M, dtype=torch.float32, device='cuda')

    ref = TorchRawDQN(pol.weights(), pol._split(target), replay.column('priority')[:R])
    ref.set_batch(cfg, batch)

    def loss_grad():
        b = batch
        return pol.dqn_loss_grad(target, b['obs'], b['action'], b['reward'], b['done'], b['next_obs'], b['next_mask'], weights=b['weight'],
                                 gamma=1.0, double_q=True, td_out=td)

    adam = lambda: pol.adam_step_clip_by_var(lr=5e-4, var_clip=40.0)
    prios = lambda: replay.update_priorities(batch['idx'], td)

    def hip_update():
        loss_grad()
        adam()
        prios()

    # agreement from equal parameters, before anything is timed
    loss_grad()
    g_hip = pol.gradients()
    td_ref = ref.loss_grad()
    agree = {'td': float((td - td_ref).abs().max() / td_ref.abs().max().clamp_min(1.0))}
    for k, prm in zip(ORDER, ref.params):
        if not k.endswith('_emb'):
            agree[k] = float((g_hip[k] - prm.grad).abs().max() / prm.grad.abs().max().clamp_min(1e-8))
    assert max(agree.values()) < 1e-4, agree
    del g_hip

    for _ in range(5):
        hip_update()
        ref.update()
    pairs = []
    for _ in range(args.pairs):
        h = timed(hip_update, args.updates)
        o = timed(ref.update, args.updates)
        pairs.append((h * 1e6, o * 1e6))
    parts = dict((k, round(float(np.median([timed(f, args.updates) for _ in range(args.pairs)])) * 1e6, 2))
                 for k, f in (('loss_grad', loss_grad), ('adam', adam), ('priorities', prios), ('torch_loss_grad', ref.loss_grad)))
    pol.set_profiling(True)
    splits = []
    for _ in range(max(args.pairs, 5)):
        hip_update()
        splits.append(pol.profile())
    pol.set_profiling(False)
    split = dict((k, round(float(np.median([s[k] for s in splits])), 2)) for k in splits[0])
    hip = np.array([p[0] for p in pairs])
    tor = np.array([p[1] for p in pairs])
    ratio = tor / hip
    return dict(rows=M, record_words=REC, parameters=pol.n_params, updates_per_sample=args.updates, unit='us per update',
                agreement_relative=dict((k, float('%.3g' % v)) for k, v in agree.items()),
                pairs=[[round(a, 2), round(b, 2)] for a, b in pairs], hip_median=round(float(np.median(hip)), 2),
                torch_median=round(float(np.median(tor)), 2), ratio_torch_over_hip=round(float(np.median(ratio)), 3),
                ratio_spread=[round(float(ratio.min()), 3), round(float(ratio.max()), 3)],
                hip_faster_in_every_pair=bool((hip < tor).all()), parts=parts, split_event_us=split,
                adam_bytes_per_step=int(pol.n_params) * 4 * 7)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1024)
    ap.add_argument('--pairs', type=int, default=7)
    ap.add_argument('--updates', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'rawdqn_rate.json'))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'rawdqn_rate.py measures on the GPU only'
    result = dict(tool='rawdqn_rate', device=torch.cuda.get_device_name(0), torch=torch.__version__,
                  command='python tools/rawdqn_rate.py ' + ' '.join(sys.argv[1:]), update=run(args))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
