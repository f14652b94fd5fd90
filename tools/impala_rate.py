#!/usr/bin/env python
"""Speed of the on-device IMPALA learner (one GPU).

  update   one learner update on a rollout batch of R x T x B rows (default 1 x 9 x 4096), default net (256 -> 64 -> 284):
           rl4rs_policy_vtrace_loss_grad (forward, V-trace scan, loss, gradient) + Adam with global-norm clip 10, against the SAME
           update written in eager torch on the GPU (matmul forward, a python loop over T for the float64 scan, autograd,
           clip_grad_norm_, torch.optim.Adam).  The two alternate in one process, ``--pairs`` pairs, every sample = ``--updates``
           updates between two synchronisations.
  parts    the HIP update's parts timed alone the same way (evaluate / rl4rs_vtrace / loss_grad on the kept rows / adam).
  loop     SeqSlateRecEnv-v0 B = 4096, T = 32 env-steps/s with the IMPALA learner in the loop and with the A2C learner in the loop,
           alternating trainers over the same env (``--pairs`` pairs of ``--iters`` train calls each).

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
KW = dict(gamma=1.0, clip_rho=1.0, clip_pg_rho=1.0, vf_coeff=0.5, ent_coeff=0.01)


class TorchImpala(object):
    """The yardstick: the same update in eager torch on the same batch."""

    def __init__(self, flat, R, T, B, obs, mask_bits, act, blp, rew, drop_last, lr=1e-4, clip=10.0):
        import torch
        from rl4rs_amd.nets.policy import split
        self.t = torch
        self.R, self.T, self.B, self.drop_last, self.clip = R, T, B, drop_last, clip
        sh = torch.arange(32, device='cuda', dtype=torch.int32)
        n = obs.shape[0]
        self.maskadd = torch.where(((mask_bits[:, :, None] >> sh) & 1).reshape(n, -1)[:, :A] > 0, 0.0, -3.4028235e38).to(torch.float32)
        self.obs, self.act, self.blp, self.rew = obs, act.to(torch.int64), blp, rew
        self.params = [p.clone().requires_grad_(True) for p in split(torch.from_numpy(flat).cuda(), OD, HID, A)]
        self.opt = torch.optim.Adam(self.params, lr=lr, eps=1e-8)

    def update(self):
        t = self.t
        R, T, B = self.R, self.T, self.B
        W1, b1, W2, b2 = self.params
        out = t.tanh(self.obs @ W1 + b1) @ W2 + b2
        lsm = t.log_softmax(out[:, :A] + self.maskadd, dim=1)
        lp = lsm.gather(1, self.act[:, None])[:, 0].view(R, T, B)
        v = out[:, A].view(R, T, B)
        Te = T - 1 if self.drop_last else T
        with t.no_grad():
            tl, V, r = lp[:, :Te].double(), v[:, :Te].double(), self.rew.view(R, T, B)[:, :Te]
            rho = t.exp(tl - self.blp.view(R, T, B)[:, :Te].double())
            boot = v[:, T - 1].double() if self.drop_last else t.zeros((R, B), dtype=t.float64, device='cuda')
            cr, cc, cp = rho.clamp(max=KW['clip_rho']), rho.clamp(max=1.0), rho.clamp(max=KW['clip_pg_rho'])
            v_next = t.cat([V[:, 1:], boot[:, None]], dim=1)
            delta = cr * (r + KW['gamma'] * v_next - V)
            acc = t.zeros((R, B), dtype=t.float64, device='cuda')
            vs = t.empty_like(V)
            for k in range(Te - 1, -1, -1):
                acc = delta[:, k] + KW['gamma'] * cc[:, k] * acc
                vs[:, k] = V[:, k] + acc
            vs_next = t.cat([vs[:, 1:], boot[:, None]], dim=1)
            pg = (cp * (r + KW['gamma'] * vs_next - V)).float()
            vs = vs.float()
        pr = t.exp(lsm)
        ent = -t.where(pr > 0, pr * lsm, t.zeros_like(pr)).sum(1).view(R, T, B)[:, :Te]
        loss = -(lp[:, :Te] * pg).sum() + KW['vf_coeff'] * 0.5 * ((v[:, :Te] - vs) ** 2).sum() - KW['ent_coeff'] * ent.sum()
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        t.nn.utils.clip_grad_norm_(self.params, self.clip)
        self.opt.step()


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
    from rl4rs_amd import device as D
    from rl4rs_amd.nets.policy import init_policy_params
    R, T, B, drop_last = args.rollouts, args.steps, args.batch, not args.keep_last
    N = R * T * B
    Te = T - 1 if drop_last else T
    rs = np.random.RandomState(0)
    flat = init_policy_params(OD, HID, A, seed=1) + (rs.randn(34973) * 0.05).astype(np.float32)
    pol = D.DevicePolicy(OD, HID, A, max_rows=N, params=flat)
    obs = torch.from_numpy(rs.randn(N, OD).astype(np.float32)).cuda()
    mask = torch.from_numpy(rs.randint(-2 ** 31, 2 ** 31, size=(N, pol.W), dtype=np.int64).astype(np.int32)).cuda()
    mask[:, 0] |= 1
    act, lp = pol.act(obs, mask, seed=3, step=0)[:2]
    blp = (lp + torch.from_numpy(rs.uniform(-0.5, 0.5, N).astype(np.float32)).cuda()).contiguous()
    rew = torch.from_numpy(rs.rand(N) * 100.0).cuda()
    ref = TorchImpala(flat, R, T, B, obs, mask, act, blp, rew, drop_last)
    grad = torch.empty(pol.n_params, dtype=torch.float32, device='cuda')
    stats = torch.empty(4, dtype=torch.float32, device='cuda')
    vstats = torch.empty(4, dtype=torch.float64, device='cuda')

    def loss_grad():
        return pol.vtrace_loss_grad(R, T, B, obs, act, blp, rew, mask_bits=mask, drop_last=drop_last, grad_out=grad, stats_out=stats,
                                    vtrace_stats_out=vstats, **KW)

    adam = lambda: pol.adam_step(grad, lr=1e-4, grad_clip=10.0)

    def hip_update():
        loss_grad()
        adam()

    # the parts, on one rollout's worth of inputs
    tl, v = pol.evaluate(obs, act, mask)[:2]
    sh = lambda x: x.view(R, T, B)[0, :Te].contiguous()
    vin = (sh(blp), sh(tl), sh(v), sh(rew))
    vboot = v.view(R, T, B)[0, T - 1].contiguous() if drop_last else None
    vs, pg, _ = D.vtrace(*vin, bootstrap_value=vboot, gamma=1.0)
    kept = Te * B
    parts_fn = (('evaluate', lambda: pol.evaluate(obs, act, mask)),
                ('vtrace_one_rollout', lambda: D.vtrace(*vin, bootstrap_value=vboot, gamma=1.0)),
                ('loss_grad_one_rollout', lambda: pol.loss_grad(0, obs[:kept], act[:kept], pg.reshape(-1), vs.reshape(-1),
                                                                mask_bits=mask[:kept], grad_out=grad)),
                ('adam', adam))
    for _ in range(10):                                   # warm-up: code objects, allocator, autograd graph caches
        hip_update()
        ref.update()
    pairs = []
    for _ in range(args.pairs):
        h = timed(hip_update, args.updates)
        t = timed(ref.update, args.updates)
        pairs.append((h * 1e6, t * 1e6))
    parts = dict((k, round(float(np.median([timed(f, args.updates) for _ in range(args.pairs)])) * 1e6, 2)) for k, f in parts_fn)
    hip = np.array([p[0] for p in pairs])
    tor = np.array([p[1] for p in pairs])
    return dict(rollouts=R, steps=T, batch=B, drop_last=drop_last, updates_per_sample=args.updates, unit='us per update',
                pairs=[[round(a, 2), round(b, 2)] for a, b in pairs], hip_median=round(float(np.median(hip)), 2),
                torch_median=round(float(np.median(tor)), 2), ratio_torch_over_hip=round(float(np.median(tor) / np.median(hip)), 2),
                hip_faster_in_every_pair=bool((hip < tor).all()), parts=parts)


def loop_leg(args):
    import torch
    import rl4rs_amd
    from rl4rs_amd import synth
    from rl4rs_amd.env.seqslate import SeqSlateRecEnv, SeqSlateState
    from rl4rs_amd.train import Trainer
    B, T = args.batch, 32
    d = tempfile.mkdtemp(prefix='impala_rate_')
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
    trainers = dict((algo, Trainer(env, algo=algo, seed=1000)) for algo in ('IMPALA', 'A2C'))
    for tr in trainers.values():
        tr.train_iteration()
        tr.train_iteration()
    pairs = []
    for _ in range(args.pairs):
        row = []
        for algo in ('IMPALA', 'A2C'):
            tr = trainers[algo]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                tr.train_iteration()
            torch.cuda.synchronize()
            row.append(B * T * args.iters / (time.perf_counter() - t0))
        pairs.append(row)
    for tr in trainers.values():
        tr.close()
    imp, a2c = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    return dict(unit='env-steps/s', pairs=[[round(a, 1), round(b, 1)] for a, b in pairs], impala_median=round(float(np.median(imp)), 1),
                a2c_median=round(float(np.median(a2c)), 1), ratio_impala_over_a2c=round(float(np.median(imp) / np.median(a2c)), 4),
                train_calls_per_sample=args.iters, workload='SeqSlateRecEnv-v0 B=%d T=%d, rollout + learner update' % (B, T))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='update,loop')
    ap.add_argument('--rollouts', type=int, default=1)
    ap.add_argument('--steps', type=int, default=9)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--keep-last', action='store_true', help='drop_last = False')
    ap.add_argument('--pairs', type=int, default=7)
    ap.add_argument('--updates', type=int, default=50)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'impala_rate.py measures on the GPU only'
    result = dict(tool='impala_rate', device=torch.cuda.get_device_name(0), torch=torch.__version__,
                  command='python tools/impala_rate.py ' + ' '.join(sys.argv[1:]))
    legs = args.legs.split(',')
    if 'update' in legs:
        result['update'] = update_legs(args)
    if 'loop' in legs:
        result['loop'] = loop_leg(args)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
