#!/usr/bin/env python
"""Speed of the on-device ensemble dynamics model and of MOPO (one GPU), each against the SAME pass written in eager torch on the
GPU, in alternating pairs inside one process.

  update    one dynamics update (training forward, loss, backward, Adam) at B = 512, M = 5 members, the real widths
            (D = 266, E = 32, hidden [256, 128]); the torch side runs the five members as batched matmuls (torch.bmm), its own
            batch norm, spectral norm and dropout, torch.optim.Adam.
  rollout   one MOPO rollout: 50 000 start rows x horizon 5, policy sampling included (policy forward, squashed sample, eval
            forward of the ensemble, one member's sample per row, max-variance penalty), in chunks of ``--predict-rows`` rows.
  mopo      MOPO updates per second at 256 rows (critic step every update, actor / temperature / targets every second one).

Before a leg is timed both sides run from equal parameters and must agree: the update leg with dropout off (the two sides draw
different masks): the loss of three successive updates within 1e-4 relative and the first update's gradient within 1e-4 of each array's
largest entry; the rollout leg with given member indices and noise, one step, within 1e-4 of
each output's largest value; the mopo leg with given noise, three updates, every parameter within 2e-4.  A ratio is reported, not required.

One JSON line on stdout (and --out FILE).  Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D, E, H1, H2, M = 266, 32, 256, 128, 5
O = D + 1


def timed(fn, n):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def pairs_of(hip, tor, pairs, n, unit_scale=1e6):
    out = []
    for _ in range(pairs):
        out.append((timed(hip, n) * unit_scale, timed(tor, n) * unit_scale))
    h, t = np.array([p[0] for p in out]), np.array([p[1] for p in out])
    return dict(pairs=[[round(a, 2), round(b, 2)] for a, b in out], hip_median=round(float(np.median(h)), 2),
                torch_median=round(float(np.median(t)), 2), ratio_torch_over_hip=round(float(np.median(t) / np.median(h)), 3),
                hip_faster_in_every_pair=bool((h < t).all()))


class TorchEnsemble(object):
    """The yardstick: the ensemble in eager torch, members batched ([M, in, out] weights, torch.bmm)."""

    def __init__(self, flat_params, flat_state, rate, lr=1e-4):
        import torch
        from rl4rs_amd import dynamics as dyn
        self.t = torch
        P = dyn.unflatten(flat_params, dyn.param_shapes(D, E, H1, H2), M)
        S = dyn.unflatten(flat_state, dyn.state_shapes(D, E, H1, H2), M)
        st = lambda dicts, k, grad: torch.from_numpy(np.stack([d[k] for d in dicts])).cuda().requires_grad_(grad)
        self.p = dict((k, st(P, k, True)) for k in P[0])
        self.s = dict((k, st(S, k, False)) for k in S[0])
        self.rate = rate
        self.opt = torch.optim.Adam(list(self.p.values()), lr=lr)

    def names(self):
        return list(self.p)

    def _sigma(self, W, uk, vk, train):
        t = self.t
        with t.no_grad():
            u, v = self.s[uk], self.s[vk]
            if train:
                v = t.nn.functional.normalize(t.bmm(W, u[:, :, None])[:, :, 0], dim=1, eps=1e-12)
                u = t.nn.functional.normalize(t.bmm(W.transpose(1, 2), v[:, :, None])[:, :, 0], dim=1, eps=1e-12)
                self.s[uk], self.s[vk] = u, v
        return (u * t.bmm(W.transpose(1, 2), v[:, :, None])[:, :, 0]).sum(dim=1)

    def _bn(self, z, g, b, rmk, rvk, train):
        t = self.t
        if train:
            mean, var = z.mean(dim=1), z.var(dim=1, unbiased=False)
            with t.no_grad():
                n = z.shape[1]
                self.s[rmk] = 0.9 * self.s[rmk] + 0.1 * mean
                self.s[rvk] = 0.9 * self.s[rvk] + 0.1 * var * (n / (n - 1.0))
        else:
            mean, var = self.s[rmk], self.s[rvk]
        return (z - mean[:, None]) * t.rsqrt(var[:, None] + 1e-5) * g[:, None] + b[:, None]

    def forward(self, xa, train):
        t, p = self.t, self.p
        X = xa[None].expand(M, -1, -1)
        drop = (lambda h: t.nn.functional.dropout(h, self.rate, True)) if (train and self.rate > 0) else (lambda h: h)
        s1 = self._sigma(p['w1'], 'u1', 'v1', train)
        h1 = drop(self._bn(t.relu(t.bmm(X, p['w1']) / s1[:, None, None] + p['b1'][:, None]), p['bn1_w'], p['bn1_b'], 'rm1', 'rv1', train))
        s2 = self._sigma(p['w2'], 'u2', 'v2', train)
        z2 = t.relu(t.bmm(t.cat([h1, X], dim=2), p['w2']) / s2[:, None, None] + p['b2'][:, None])
        h2 = drop(self._bn(z2, p['bn2_w'], p['bn2_b'], 'rm2', 'rv2', train))
        s3 = self._sigma(p['wh'][:, :, :O], 'u3', 'v3', train)
        mu = t.bmm(h2, p['wh'][:, :, :O]) / s3[:, None, None] + p['bh'][:, None, :O]
        l = t.bmm(h2, p['wh'][:, :, O:]) + p['bh'][:, None, O:]
        mx, mn = p['max_ls'][:, None], p['min_ls'][:, None]
        ls = mx - t.nn.functional.softplus(mx - l)
        return mu, mn + t.nn.functional.softplus(ls - mn)

    def update(self, x, a, nxt, rew, mask):
        t = self.t
        xa = t.cat([x, a], dim=1)
        mu, ls = self.forward(xa, True)
        like = ((xa[None, :, :D] + mu[:, :, :D] - nxt[None]) ** 2 * t.exp(-ls[:, :, :D])).mean(dim=2) + \
            (mu[:, :, D] - rew[None]) ** 2 * t.exp(-ls[:, :, D])
        pen = 0.01 * (self.p['max_ls'].sum(dim=1) - self.p['min_ls'].sum(dim=1))
        loss = (mask * (like + ls.sum(dim=2) + pen[:, None])).mean(dim=1).sum()
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        self.opt.step()
        return loss

    def predict(self, x, a, idx, noise, lam):
        t = self.t
        with t.no_grad():
            xa = t.cat([x, a], dim=1)
            mu, ls = self.forward(xa, False)
            pred = mu + t.exp(ls) * noise
            var = t.exp(2.0 * ls).sum(dim=2).max(dim=0).values
            pick = pred[idx, t.arange(x.shape[0], device=x.device)]
            return x + pick[:, :D], pick[:, D] - lam * var, var


def _mlp(t, p, x):
    h = t.relu(t.addmm(p[1], x, p[0]))
    h = t.relu(t.addmm(p[3], h, p[2]))
    return t.addmm(p[5], h, p[4])


def _squashed(t, head, eps, A):
    mu, logstd = head[:, :A], head[:, A:].clamp(-20.0, 2.0)
    u = mu + logstd.exp() * eps
    logp = (-0.5 * eps * eps - logstd - 0.5 * np.log(2 * np.pi) - 2.0 * (np.log(2.0) - u - t.nn.functional.softplus(-2.0 * u))).sum(dim=1)
    return t.tanh(u), logp


AMLP_NAMES = ('fc1_w', 'fc1_b', 'fc2_w', 'fc2_b', 'head_w', 'head_b')


def _tensors(net, grad):
    w = net.weights()
    return [w[k].clone().requires_grad_(grad) for k in AMLP_NAMES]


def _new_dynamics(rate, rows, grad_rows, seed=0):
    from rl4rs_amd import dynamics as dyn
    from rl4rs_amd.device import DeviceDynamics
    p, s = dyn.init_dynamics(D, E, H1, H2, M, True, seed)
    # u / v a few power iterations in, as in a model that has trained (an eval forward does not iterate: sigma = u^T W v of two random
    # directions would be near zero)
    P, S = dyn.unflatten(p, dyn.param_shapes(D, E, H1, H2), M), dyn.unflatten(s, dyn.state_shapes(D, E, H1, H2), M)
    for pm, sm in zip(P, S):
        for wk, uk, vk in (('w1', 'u1', 'v1'), ('w2', 'u2', 'v2'), ('wh', 'u3', 'v3')):
            W = pm[wk][:, :O].astype(np.float64) if wk == 'wh' else pm[wk].astype(np.float64)
            u = sm[uk].astype(np.float64)
            for _ in range(3):
                v = W @ u
                v /= np.linalg.norm(v)
                u = W.T @ v
                u /= np.linalg.norm(u)
            sm[uk][...], sm[vk][...] = u, v
    s = np.concatenate([s, np.zeros(D, np.float32), np.ones(D, np.float32), np.array([0.0, 1.0], np.float32)])      # no scaler
    return DeviceDynamics(D, E, p, s, (H1, H2), M, max_rows=rows, max_grad_rows=grad_rows, dropout_rate=rate), p, s[:-(2 * D + 2)]


def update_leg(args):
    import torch
    from rl4rs_amd import dynamics as dyn
    B = args.rows
    rs = np.random.RandomState(0)
    c = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    # centred observations: with inputs in [0, 1] a hidden column is active on every row or on none, the bias ahead of a batch norm
    # then has a gradient that is zero but for rounding, and the two sides' Adam steps on it are a comparison of rounding noise
    x, a = c(rs.standard_normal((B, D))), c(np.tanh(rs.standard_normal((B, E))))
    nxt, rew = c(x.cpu().numpy() + 0.1 * rs.standard_normal((B, D))), c(rs.standard_normal(B))
    mask = c(rs.uniform(size=(M, B)) < 0.5)
    # agreement, dropout off on both sides: the loss of three successive updates and the first update's gradient
    net, p, s = _new_dynamics(0.0, B, B)
    ref = TorchEnsemble(p, s, 0.0)
    loss_gap, grad_gap = 0.0, 0.0
    for k in range(3):
        lh = float(net.loss_grad(x, a, nxt, rew, mask, seed=1, step=k).sum())
        if k == 0:
            got = dyn.unflatten(net.grad().cpu().numpy(), dyn.param_shapes(D, E, H1, H2), M)
        net.adam_step(1e-4)
        lt = float(ref.update(x, a, nxt, rew, mask))
        loss_gap = max(loss_gap, abs(lh - lt) / abs(lt))
        if k == 0:
            for name in ref.names():
                g = ref.p[name].grad.cpu().numpy()
                grad_gap = max(grad_gap, float(np.abs(np.stack([d[name] for d in got]) - g).max() / np.abs(g).max()))
    assert loss_gap < 1e-4 and grad_gap < 1e-4, ('the HIP update and the torch yardstick disagree: relative loss difference %g over 3 '
                                                'updates, gradient difference %g of an array\'s largest entry' % (loss_gap, grad_gap))
    net.close()
    # timed with dropout 0.2 on both sides
    net, p, s = _new_dynamics(0.2, B, B)
    ref = TorchEnsemble(p, s, 0.2)
    k = [0]

    def hip():
        k[0] += 1
        net.loss_grad(x, a, nxt, rew, mask, seed=1, step=k[0])
        net.adam_step(1e-4)

    tor = lambda: ref.update(x, a, nxt, rew, mask)
    for _ in range(10):
        hip()
        tor()
    out = pairs_of(hip, tor, args.pairs, args.updates)
    out.update(rows=B, members=M, unit='us per update', updates_per_sample=args.updates, max_rel_loss_diff_over_3_updates=loss_gap,
               max_grad_diff_rel_to_array_max=grad_gap)
    net.close()
    return out


def rollout_leg(args):
    import torch
    from rl4rs_amd import device as Dv
    from rl4rs_amd.offline_rl import init_amlp_params
    N, H, R, lam = args.rollout_rows, args.horizon, args.predict_rows, 1.0
    rs = np.random.RandomState(1)
    c = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    net, p, s = _new_dynamics(0.2, R, 0)
    ref = TorchEnsemble(p, s, 0.2)
    policy = Dv.DeviceAMLP(D, 0, 2 * E, init_amlp_params(D, 0, 2 * E, seed=3, heads=2), max_rows=R, max_grad_rows=0)
    pt = _tensors(policy, False)
    start = c(rs.uniform(size=(N, D)))
    # agreement on one chunk with given indices and noise
    xs = start[:R].contiguous()
    eps = c(rs.standard_normal((R, E)))
    idx = torch.from_numpy(rs.randint(0, M, size=R).astype(np.int32)).cuda()
    noise = c(rs.standard_normal((M, R, O)))
    a_h, _ = Dv.squashed_sample(policy.forward(xs), eps)
    a_t, _ = _squashed(torch, _mlp(torch, pt, xs), eps, E)
    got = net.predict(xs, a_h, indices=idx, noise=noise, lam=lam)
    want = ref.predict(xs, a_t, idx.long(), noise, lam)
    diff = max(float((a_h - a_t).abs().max()), *[float((g.reshape(w.shape) - w).abs().max() / max(1.0, float(w.abs().max())))
                                                 for g, w in zip(got[:3], want)])
    assert diff < 1e-4, 'the HIP rollout step and the torch yardstick disagree: difference %g of the largest value' % diff
    gen = torch.Generator(device='cuda').manual_seed(0)
    k = [0]

    def hip():
        k[0] += 1
        st = start
        for h in range(H):
            nxt = torch.empty_like(st)
            for lo in range(0, N, R):
                xs = st[lo:lo + R].contiguous()
                e = torch.randn((xs.shape[0], E), generator=gen, device='cuda')
                act, _ = Dv.squashed_sample(policy.forward(xs), e)
                nx, r, var, _ = net.predict(xs, act, seed=k[0], step=h * 1024 + lo // R, lam=lam)
                nxt[lo:lo + R] = nx
            st = nxt

    def tor():
        st = start
        with torch.no_grad():
            for h in range(H):
                nxt = torch.empty_like(st)
                for lo in range(0, N, R):
                    xs = st[lo:lo + R]
                    n = xs.shape[0]
                    act, _ = _squashed(torch, _mlp(torch, pt, xs), torch.randn((n, E), generator=gen, device='cuda'), E)
                    ix = torch.randint(0, M, (n,), generator=gen, device='cuda')
                    nx, r, var = ref.predict(xs, act, ix, torch.randn((M, n, O), generator=gen, device='cuda'), lam)
                    nxt[lo:lo + R] = nx
                st = nxt

    hip()
    tor()
    out = pairs_of(hip, tor, args.pairs, args.rollouts, unit_scale=1e3)
    out.update(rows=N, horizon=H, chunk_rows=R, unit='ms per rollout', rollouts_per_sample=args.rollouts, max_diff_one_step_rel_to_largest_value=diff)
    net.close()
    policy.close()
    return out


class TorchSAC(object):
    def __init__(self, mopo, lr=3e-4):
        import torch
        self.t = torch
        self.policy, self.q1, self.q2 = _tensors(mopo.policy, True), _tensors(mopo.q1, True), _tensors(mopo.q2, True)
        self.q1t, self.q2t = _tensors(mopo.q1_targ, False), _tensors(mopo.q2_targ, False)
        self.log_temp = mopo.log_temp.p.clone().requires_grad_(True)
        self.copt = torch.optim.Adam(self.q1 + self.q2, lr=lr)
        self.aopt = torch.optim.Adam(self.policy, lr=lr)
        self.topt = torch.optim.Adam([self.log_temp], lr=lr)
        self.gamma, self.tau, self.A = mopo.gamma, mopo.tau, mopo.A

    def update(self, obs, act, rew, nxt, ter, noise, do_actor):
        t, A = self.t, self.A
        with t.no_grad():
            a2, lp = _squashed(t, _mlp(t, self.policy, nxt), noise['eps_next'], A)
            x2 = t.cat([nxt, a2], dim=1)
            v = t.minimum(_mlp(t, self.q1t, x2), _mlp(t, self.q2t, x2))[:, 0] - self.log_temp.exp() * lp
            y = rew + self.gamma * (1.0 - ter) * v
        x = t.cat([obs, act], dim=1)
        closs = ((_mlp(t, self.q1, x)[:, 0] - y) ** 2).mean() + ((_mlp(t, self.q2, x)[:, 0] - y) ** 2).mean()
        self.copt.zero_grad(set_to_none=True)
        closs.backward()
        self.copt.step()
        if not do_actor:
            return
        a_pi, lp = _squashed(t, _mlp(t, self.policy, obs), noise['eps_actor'], A)
        xp = t.cat([obs, a_pi], dim=1)
        q = t.minimum(_mlp(t, [p.detach() for p in self.q1], xp), _mlp(t, [p.detach() for p in self.q2], xp))[:, 0]
        aloss = (self.log_temp.detach().exp() * lp - q).mean()
        self.aopt.zero_grad(set_to_none=True)
        aloss.backward()
        self.aopt.step()
        with t.no_grad():
            _, lp = _squashed(t, _mlp(t, self.policy, obs), noise['eps_temp'], A)
            targ = (lp - A).mean()
        tloss = -(self.log_temp.exp() * targ).sum()
        self.topt.zero_grad(set_to_none=True)
        tloss.backward()
        self.topt.step()
        with t.no_grad():
            for tg, src in ((self.q1t, self.q1), (self.q2t, self.q2)):
                t._foreach_mul_(tg, 1.0 - self.tau)
                t._foreach_add_(tg, [s_.detach() for s_ in src], alpha=self.tau)


def mopo_leg(args):
    import torch
    from rl4rs_amd.offline_rl import MOPO
    B = args.mopo_rows
    rs = np.random.RandomState(2)
    c = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    mopo = MOPO({'action_emb_size': E}, D, None, batch_size=B, gamma=1.0, update_actor_interval=2, seed=5)
    ref = TorchSAC(mopo)
    b = [c(rs.standard_normal((B, D))), c(np.tanh(rs.standard_normal((B, E)))), c(rs.standard_normal(B)), c(rs.standard_normal((B, D))),
         c(rs.uniform(size=B) < 0.1)]
    noise = dict((k, c(rs.standard_normal((B, E)))) for k in ('eps_next', 'eps_actor', 'eps_temp'))
    k = [0]

    def hip():
        mopo.update(*b, noise=noise)

    def tor():
        ref.update(*b, noise=noise, do_actor=k[0] % 2 == 0)
        k[0] += 1

    for _ in range(3):
        hip()
        tor()
    drift = float((mopo.log_temp.p - ref.log_temp.detach()).abs().max())
    for net, tp in ((mopo.policy, ref.policy), (mopo.q1, ref.q1), (mopo.q2, ref.q2), (mopo.q1_targ, ref.q1t), (mopo.q2_targ, ref.q2t)):
        w = net.weights()
        drift = max([drift] + [float((w[n] - tp[i].detach()).abs().max()) for i, n in enumerate(AMLP_NAMES)])
    assert drift < 2e-4, 'the HIP update and the torch yardstick disagree after 3 updates: max abs parameter difference %g' % drift
    for _ in range(21):
        hip()
        tor()
    out = pairs_of(hip, tor, args.pairs, args.updates)
    out.update(rows=B, unit='us per update', update_actor_interval=2, updates_per_sample=args.updates,
               hip_updates_per_s=round(1e6 / out['hip_median'], 1), torch_updates_per_s=round(1e6 / out['torch_median'], 1),
               max_abs_param_diff_after_3_updates=drift)
    mopo.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='update,rollout,mopo')
    ap.add_argument('--rows', type=int, default=512)
    ap.add_argument('--mopo-rows', type=int, default=256)
    ap.add_argument('--rollout-rows', type=int, default=50000)
    ap.add_argument('--horizon', type=int, default=5)
    ap.add_argument('--predict-rows', type=int, default=8192)
    ap.add_argument('--pairs', type=int, default=7)
    ap.add_argument('--updates', type=int, default=300, help='updates per timed sample')
    ap.add_argument('--rollouts', type=int, default=3, help='rollouts per timed sample')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'dynamics_rate.py measures on the GPU only'
    result = dict(tool='dynamics_rate', device=torch.cuda.get_device_name(0), torch=torch.__version__,
                  command='python tools/dynamics_rate.py ' + ' '.join(sys.argv[1:]))
    legs = args.legs.split(',')
    for name, fn in (('update', update_leg), ('rollout', rollout_leg), ('mopo', mopo_leg)):
        if name in legs:
            result[name] = fn(args)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
