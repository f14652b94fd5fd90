#!/usr/bin/env python
"""Speed of the Gaussian actor-critic of the continuous on-policy learners (one GPU).

  update   (a) the A2C update at N = 36 864 rows (B = 4096, T = 9: loss, gradient, global-norm clip, Adam) and (b) one PPO minibatch
           step at 256 rows (loss with KL and value clipping, gradient, Adam), each as the library runs it (rl4rs_gpolicy_loss_grad +
           rl4rs_gpolicy_adam_step) against the SAME pass written in eager torch on the GPU (matmul autograd, Adam in TF's form via
           torch._foreach).  The two alternate in one process, ``--pairs`` pairs, every sample = ``--updates`` updates between two
           synchronisations.  Before anything is timed both sides compute the gradient from equal parameters and must agree to 2e-4 of
           each block's max-norm.
  loop     SlateRecEnv-v0 B = 4096, T = 9 continuous env-steps/s with ContiTrainer (A2C, then PPO) in the loop, beside the same
           process's replay rate (the env driven by its logged ``offline_action`` embeddings, no learner).

One JSON line on stdout (and --out FILE).  Needs a GPU: there is no CPU path."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OD, H, E = 256, 256, 32
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


class TorchGauss(object):
    """The yardstick: the same loss, backward and TF-form Adam in eager torch."""

    def __init__(self, flat, lr=1e-4):
        import torch
        from rl4rs_amd.nets import gausspolicy as G
        self.t = torch
        self.p = [torch.from_numpy(np.ascontiguousarray(v)).cuda().requires_grad_(True) for v in G.split(flat, OD, E, H).values()]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.step, self.lr = 0, lr

    def forward(self, x):
        t, p = self.t, self.p
        h = t.tanh(t.addmm(p[3], t.tanh(t.addmm(p[1], x, p[0])), p[2]))
        c = t.tanh(t.addmm(p[9], t.tanh(t.addmm(p[7], x, p[6])), p[8]))
        return t.addmm(p[5], h, p[4]), t.addmm(p[11], c, p[10])[:, 0]

    def loss(self, algo, b, kl_coeff=0.2):
        t = self.t
        head, v = self.forward(b['obs'])
        mean, ls = head[:, :E], head[:, E:]
        z = (b['act'] - mean) * t.exp(-ls)
        lp = (-0.5 * z * z - ls).sum(dim=1) - E * HALF_LOG_2PI
        ent = (ls + (HALF_LOG_2PI + 0.5)).sum(dim=1)
        if algo == 0:
            return (-lp * b['adv'] + 0.25 * (v - b['ret']) ** 2 - 0.01 * ent).sum()
        ratio = t.exp(lp - b['logp'])
        pi = -t.minimum(b['adv'] * ratio, b['adv'] * ratio.clamp(0.7, 1.3))
        vc = b['val'] + (v - b['val']).clamp(-500.0, 500.0)
        vf = t.maximum((v - b['ret']) ** 2, (vc - b['ret']) ** 2)
        mo, lo = b['head'][:, :E], b['head'][:, E:]
        kl = (ls - lo + (t.exp(2.0 * lo) + (mo - mean) ** 2) / (2.0 * t.exp(2.0 * ls)) - 0.5).sum(dim=1)
        return (pi + 0.5 * vf + kl_coeff * kl).mean()

    def grad(self, algo, b):
        for p in self.p:
            p.grad = None
        self.loss(algo, b).backward()
        return [p.grad for p in self.p]

    def update(self, algo, b, grad_clip):
        t = self.t
        g = self.grad(algo, b)
        if grad_clip > 0.0:
            norm = t.sqrt(sum((x * x).sum() for x in g))
            t._foreach_mul_(g, t.clamp(grad_clip / norm, max=1.0))
        self.step += 1
        lr_t = self.lr * math.sqrt(1.0 - 0.999 ** self.step) / (1.0 - 0.9 ** self.step)
        with t.no_grad():
            t._foreach_mul_(self.m, 0.9)
            t._foreach_add_(self.m, g, alpha=0.1)
            t._foreach_mul_(self.v, 0.999)
            t._foreach_addcmul_(self.v, g, g, value=0.001)
            den = t._foreach_sqrt(self.v)
            t._foreach_add_(den, 1e-8)
            t._foreach_addcdiv_(self.p, self.m, den, value=-lr_t)


def timed(fn, updates):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(updates):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / updates


def update_leg(args, algo, N, updates):
    import torch
    from rl4rs_amd.device import DeviceGaussPolicy
    from rl4rs_amd.nets import gausspolicy as G
    rs = np.random.RandomState(N)
    flat = G.init_gausspolicy_params(OD, E, H, seed=1)
    pol = DeviceGaussPolicy(OD, E, max_rows=N, hidden=H, params=flat)
    ref = TorchGauss(flat)
    c = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    obs = c(rs.randn(N, OD))
    act, _, logp, val, _, head, _ = pol.act(obs, seed=3, step=0, want_head=True)
    b = dict(obs=obs, act=act, logp=logp + c(0.1 * rs.randn(N)), val=val, head=head + c(0.05 * rs.randn(N, 2 * E)),
             adv=c(rs.randn(N)), ret=c(rs.randn(N)))
    grad = torch.empty(pol.n_params, dtype=torch.float32, device='cuda')
    grad_clip = 10.0 if algo == 0 else 0.0

    def hip_grad():
        if algo == 0:
            return pol.loss_grad(0, b['obs'], b['act'], b['adv'], b['ret'], vf_coeff=0.5, ent_coeff=0.01, grad_out=grad)[0]
        return pol.loss_grad(1, b['obs'], b['act'], b['adv'], b['ret'], old_logp=b['logp'], old_value=b['val'], old_head=b['head'],
                             vf_coeff=0.5, ent_coeff=0.0, clip=0.3, vf_clip=500.0, kl_coeff=0.2, grad_out=grad)[0]

    def hip_update():
        pol.adam_step(hip_grad(), lr=1e-4, grad_clip=grad_clip)

    def torch_update():
        ref.update(algo, b, grad_clip)

    # faster and different is not faster: the two gradients from equal parameters, per block relative to the block's max-norm
    gh = G.split(hip_grad().clone(), OD, E, H)
    gt = ref.grad(algo, b)
    drift = max(float((gh[k] - gt[i].reshape(gh[k].shape)).abs().max() / gt[i].abs().max().clamp_min(1e-30)) for i, k in enumerate(G.NAMES))
    assert drift < 2e-4, 'the HIP gradient and the torch yardstick disagree: %g of a block max-norm' % drift
    for _ in range(10):                                   # warm-up: code objects, allocator, autograd graph caches
        hip_update()
        torch_update()
    pairs = []
    for _ in range(args.pairs):
        h = timed(hip_update, updates)
        t = timed(torch_update, updates)
        pairs.append((h * 1e6, t * 1e6))
    hip = np.array([p[0] for p in pairs])
    tor = np.array([p[1] for p in pairs])
    pol.close()
    return dict(name='A2C update' if algo == 0 else 'PPO minibatch step', rows=N, updates_per_sample=updates, unit='us per update',
                pairs=[[round(a, 2), round(b_, 2)] for a, b_ in pairs], hip_median=round(float(np.median(hip)), 2),
                torch_median=round(float(np.median(tor)), 2), ratio_torch_over_hip=round(float(np.median(tor) / np.median(hip)), 2),
                hip_faster_in_every_pair=bool((hip < tor).all()), max_rel_gradient_diff=drift)


def loop_leg(args, algo):
    import torch
    from td3_rate import _env
    from rl4rs_amd.train import ContiTrainer
    B, T = args.batch, 9
    env = _env(B, T)
    tr = ContiTrainer(env, algo=algo, seed=1000)
    tr.train_iteration()
    tr.train_iteration()
    steps = args.iterations
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.train_iteration()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    tr.close()
    return dict(algo=algo, value=round(B * T * steps / dt, 1), unit='env-steps/s', ms_per_iteration=round(dt / steps * 1e3, 3),
                workload='SlateRecEnv-v0 conti B=%d T=%d, Gaussian rollout + %s update' % (B, T, algo))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='update,loop')
    ap.add_argument('--pairs', type=int, default=7)
    ap.add_argument('--updates', type=int, default=1000, help='PPO minibatch steps per timed sample (the A2C update takes a tenth)')
    ap.add_argument('--iterations', type=int, default=50, help='train iterations / episodes in the timed window of the loop legs')
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'gauss_rate.py measures on the GPU only'
    # the measurement's own arguments; where the line is also written to is not one of them
    shown = [a for i, a in enumerate(sys.argv[1:]) if a != '--out' and not a.startswith('--out=') and (i == 0 or sys.argv[i] != '--out')]
    result = dict(tool='gauss_rate', device=torch.cuda.get_device_name(0), torch=torch.__version__,
                  command=' '.join(['python tools/gauss_rate.py'] + shown))
    legs = args.legs.split(',')
    if 'update' in legs:
        result['update'] = [update_leg(args, 0, 36864, max(1, args.updates // 10)), update_leg(args, 1, 256, args.updates)]
    if 'loop' in legs:
        from td3_rate import replay_leg
        result['replay'] = replay_leg(args)
        result['loop'] = [loop_leg(args, a) for a in ('A2C', 'PPO')]
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
