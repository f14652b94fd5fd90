"""Torch restatement of the ensemble dynamics model and of MOPO's SAC update ("Ensemble dynamics model and MOPO"), with
the arithmetic type as a parameter: float64 is the reference the device is compared with, the SAME code in float32 on the very
inputs of a test is that test's yardstick.  A comparison's bar is BAR_FACTOR x the largest float32-to-float64 difference of the
compared quantity - measured on the restatement, never on the kernels.

d3rlpy 0.91 is absent (parity unpinned): this file states what is built.  It uses torch.nn.functional.batch_norm / softplus; the
spectral norm is written out so that u and v can be given; the dropout keep mask is the library's counter hash, restated in numpy.
Parameters and state are lists (one dict per member) in the layouts of rl4rs_amd/dynamics.py, matrices [in, out]."""
import numpy as np
import torch
import torch.nn.functional as F

BAR_FACTOR = 4.0
M32 = np.uint64(0xffffffff)
SITE_INDEX, SITE_NOISE = 1000, 1001


# ---------------------------------------------------------------------------------------------------------------- the counter hash
def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & M32
    x ^= x >> np.uint64(16)
    return x


def uniform01(seed, step, row, a):
    """csrc/common.hpp uniform01: 23 bits + 0.5, exactly representable in float32"""
    row, a = np.asarray(row, dtype=np.uint64), np.asarray(a, dtype=np.uint64)
    s = mix32((np.uint64(step & 0xffffffff) * np.uint64(0x9E3779B9) + np.uint64(0x85EBCA6B)) & M32)
    r = mix32((row * np.uint64(0xC2B2AE35) + a * np.uint64(0x27D4EB2F) + np.uint64(1)) & M32)
    h = mix32((np.uint64(seed & 0xffffffff) ^ s ^ r) & M32)
    h = mix32((h + a) & M32)
    return ((h >> np.uint64(9)).astype(np.float64) + 0.5) / 8388608.0


def keep_mask(seed, step, member, layer, rows, cols, rate):
    """[rows, cols] of 0 / 1: kept where uniform01(seed, step, row, (2 member + layer) * 65536 + col) >= float32(rate)"""
    r = np.arange(rows)[:, None]
    c = np.arange(cols)[None, :]
    return (uniform01(seed, step, r, (2 * member + layer) * 65536 + c) >= float(np.float32(rate))).astype(np.float64)


def member_index(seed, step, rows, members):
    u = uniform01(seed, step, np.arange(rows), SITE_INDEX * 65536).astype(np.float32)
    return np.minimum((u * np.float32(members)).astype(np.int64), members - 1)


# ---------------------------------------------------------------------------------------------------------------- the network
def default_cfg(**kw):
    cfg = dict(use_bn=True, rate=0.2, use_dense=True, spectral=True, power_iter=True, seed=0, step=0)
    cfg.update(kw)
    return cfg


def _t(x, dt):
    return torch.as_tensor(np.asarray(x), dtype=dt)


def scale_obs(x, sc, dt):
    if sc is None:
        return _t(x, dt)
    mn, rg = _t(sc['obs_min'], dt), _t(sc['obs_range'], dt)
    return torch.where(rg > 0, (_t(x, dt) - mn) / torch.where(rg > 0, rg, torch.ones_like(rg)), torch.zeros_like(_t(x, dt)))


def scale_rew(r, sc, dt):
    return _t(r, dt) if sc is None else (_t(r, dt) - float(sc['rew'][0])) / float(sc['rew'][1])


def spectral(W, u, v, train, power_iter=True):
    """torch.nn.utils.spectral_norm on W [in, out] (torch holds W^T [out, in]; u [out], v [in]): -> (sigma, u, v); u and v are
    constants of the backward.  One power iteration in training."""
    with torch.no_grad():
        if train and power_iter:
            v = F.normalize(W @ u, dim=0, eps=1e-12)
            u = F.normalize(W.t() @ v, dim=0, eps=1e-12)
    return u @ (W.t() @ v), u, v


def member_forward(p, s, xa, m, train, cfg, dt):
    """-> dict(mu, ls, sigma [3], new state, batch statistics); p: dict of tensors (requires_grad where wanted), s: dict of arrays"""
    out = {'state': {}, 'sigma': []}
    O = p['max_ls'].shape[0]

    def lin(x, W, b, uk, vk):
        if cfg['spectral'] and uk is not None:
            sigma, u, v = spectral(W, _t(s[uk], dt), _t(s[vk], dt), train, cfg['power_iter'])
            out['state'][uk], out['state'][vk] = u, v
            out['sigma'].append(sigma.detach())
            return (x @ W) / sigma + b
        if uk is not None:
            out['sigma'].append(torch.ones((), dtype=dt))
        return x @ W + b

    def layer(x, W, b, g, be, uk, vk, rmk, rvk, l):
        z = torch.relu(lin(x, W, b, uk, vk))
        h = z
        if cfg['use_bn']:
            rm, rv = _t(s[rmk], dt).clone(), _t(s[rvk], dt).clone()
            if train:
                out['mean%d' % (l + 1)] = z.detach().mean(dim=0)
                out['var%d' % (l + 1)] = z.detach().var(dim=0, unbiased=False)
            h = F.batch_norm(z, rm, rv, g, be, training=train, momentum=0.1, eps=1e-5)
            out['state'][rmk], out['state'][rvk] = rm, rv
        if train and cfg['rate'] > 0:
            keep = _t(keep_mask(cfg['seed'], cfg['step'], m, l, x.shape[0], W.shape[1], cfg['rate']), dt)
            h = h * keep * (1.0 / (1.0 - float(np.float32(cfg['rate']))))
        return h

    h1 = layer(xa, p['w1'], p['b1'], p['bn1_w'], p['bn1_b'], 'u1', 'v1', 'rm1', 'rv1', 0)
    in2 = torch.cat([h1, xa], dim=1) if cfg['use_dense'] else h1
    h2 = layer(in2, p['w2'], p['b2'], p['bn2_w'], p['bn2_b'], 'u2', 'v2', 'rm2', 'rv2', 1)
    mu = lin(h2, p['wh'][:, :O], p['bh'][:O], 'u3', 'v3')
    l = h2 @ p['wh'][:, O:] + p['bh'][O:]
    ls = p['max_ls'] - F.softplus(p['max_ls'] - l)
    ls = p['min_ls'] + F.softplus(ls - p['min_ls'])
    out['mu'], out['ls'] = mu, ls
    out['sigma'] = torch.stack(out['sigma'])
    return out


def tensors(P, dt, grad=False):
    return [dict((k, torch.tensor(np.asarray(v), dtype=dt, requires_grad=grad)) for k, v in p.items()) for p in P]


def forward(P, S, x, a, train, cfg, dt, sc=None, grad=False):
    """every member's member_forward on xa = [scaled x | a] -> (list of outputs, parameter tensors, xa)"""
    Pt = tensors(P, dt, grad)
    xa = torch.cat([scale_obs(x, sc, dt), _t(a, dt)], dim=1)
    return [member_forward(p, s, xa, m, train, cfg, dt) for m, (p, s) in enumerate(zip(Pt, S))], Pt, xa


def member_loss(o, xa, nxt_s, rew_s, mask_m, p):
    D = nxt_s.shape[1]
    mu, ls = o['mu'], o['ls']
    mu_x, mu_r = xa[:, :D] + mu[:, :D], mu[:, D]
    like = ((mu_x - nxt_s) ** 2 * torch.exp(-ls[:, :D])).mean(dim=1) + (mu_r - rew_s) ** 2 * torch.exp(-ls[:, D])
    loss_b = like + ls.sum(dim=1) + 0.01 * (p['max_ls'].sum() - p['min_ls'].sum())
    return (mask_m * loss_b).mean()


def loss_grad(P, S, x, a, nxt, rew, mask, cfg, dt, sc=None):
    """-> dict(loss [M], grads (list of dicts of float64 arrays), outs (member_forward results))"""
    outs, Pt, xa = forward(P, S, x, a, True, cfg, dt, sc, grad=True)
    nxt_s, rew_s, mask = scale_obs(nxt, sc, dt), scale_rew(rew, sc, dt), _t(mask, dt)
    losses = [member_loss(o, xa, nxt_s, rew_s, mask[m], p) for m, (o, p) in enumerate(zip(outs, Pt))]
    torch.stack(losses).sum().backward()
    grads = [dict((k, (v.grad.numpy().astype(np.float64) if v.grad is not None else np.zeros(tuple(v.shape)))) for k, v in p.items())
             for p in Pt]
    return dict(loss=np.array([float(v.detach()) for v in losses]), grads=grads, outs=outs)


def new_state(S, outs):
    """the state after a training forward"""
    return [dict((k, (o['state'][k].numpy().astype(np.float64) if k in o['state'] else np.asarray(v, np.float64))) for k, v in s.items())
            for s, o in zip(S, outs)]


def adam(P, G, Mo, Vo, t, lr, dt, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's step t (1-based) in ``dt`` -> (P, Mo, Vo) as lists of dicts of arrays"""
    outP, outM, outV = [], [], []
    for p, g, m, v in zip(P, G, Mo, Vo):
        np_, nm, nv = {}, {}, {}
        for k in p:
            pk, gk, mk, vk = [_t(z[k], dt) for z in (p, g, m, v)]
            mk = b1 * mk + (1 - b1) * gk
            vk = b2 * vk + (1 - b2) * gk * gk
            denom = vk.sqrt() / np.sqrt(1 - b2 ** t) + eps
            np_[k], nm[k], nv[k] = (pk - (lr / (1 - b1 ** t)) * (mk / denom)).numpy(), mk.numpy(), vk.numpy()
        outP.append(np_); outM.append(nm); outV.append(nv)
    return outP, outM, outV


def predict(P, S, x, a, indices, noise, cfg, dt, sc=None, variance_type='max', deterministic=False, lam=None):
    """predict_with_variance in eval mode -> (next_x [N, D], reward [N], variance [N]) as float64 arrays.  noise [M, N, O]."""
    outs, _, xa = forward(P, S, x, a, False, cfg, dt, sc)
    D = np.asarray(x).shape[1]
    mu = torch.stack([o['mu'] for o in outs])
    ls = torch.stack([o['ls'] for o in outs])
    eps = torch.zeros_like(mu) if deterministic else _t(noise, dt)
    pred = mu + torch.exp(ls) * eps
    data = torch.cat([xa[None, :, :D] + pred[:, :, :D], pred[:, :, D:]], dim=2)               # [M, N, O] in scaled units
    if variance_type == 'max':
        var = torch.exp(2.0 * ls).sum(dim=2).max(dim=0).values
    else:
        var = (data.std(dim=0) ** 2).sum(dim=1)
    idx = torch.as_tensor(np.asarray(indices), dtype=torch.int64)
    pick = data[idx, torch.arange(data.shape[1])]
    nx, r = pick[:, :D], pick[:, D]
    if sc is not None:
        nx = nx * _t(sc['obs_range'], dt) + _t(sc['obs_min'], dt)
        r = r * float(sc['rew'][1]) + float(sc['rew'][0])
    if lam is not None:
        r = r - lam * var
    return nx.numpy().astype(np.float64), r.numpy().astype(np.float64), var.numpy().astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- SAC (MOPO)
class MLP(object):
    """d3rlpy's default encoder + one Linear head on the library's amlp parameter dict"""

    def __init__(self, params, dt):
        self.p = dict((k, torch.tensor(np.asarray(v), dtype=dt, requires_grad=True)) for k, v in params.items())
        self.dt = dt

    def __call__(self, x, a=None):
        x = torch.as_tensor(x, dtype=self.dt)
        if a is not None:
            x = torch.cat([x, torch.as_tensor(a, dtype=self.dt)], dim=1)
        h = torch.relu(x @ self.p['fc1_w'] + self.p['fc1_b'])
        h = torch.relu(h @ self.p['fc2_w'] + self.p['fc2_b'])
        return h @ self.p['head_w'] + self.p['head_b']

    def grads(self):
        return dict((k, (v.grad.numpy().astype(np.float64) if v.grad is not None else np.zeros(tuple(v.shape)))) for k, v in self.p.items())

    def zero_grad(self):
        for v in self.p.values():
            v.grad = None

    def arrays(self):
        return dict((k, v.detach().numpy().copy()) for k, v in self.p.items())


def squashed_sample(policy, obs, eps):
    head = policy(obs)
    A = head.shape[1] // 2
    eps = torch.as_tensor(np.asarray(eps), dtype=policy.dt)
    mu, logstd = head[:, :A], head[:, A:].clamp(-20.0, 2.0)
    u = mu + logstd.exp() * eps
    jacob = 2.0 * (np.log(2.0) - u - F.softplus(-2.0 * u))
    return torch.tanh(u), (torch.distributions.Normal(mu, logstd.exp()).log_prob(u) - jacob).sum(dim=1)


def sac_target(policy, q_targs, log_temp, rew, nxt, ter, eps_next, gamma):
    dt = policy.dt
    with torch.no_grad():
        a, logp = squashed_sample(policy, nxt, eps_next)
        v = torch.stack([q(nxt, a)[:, 0] for q in q_targs]).min(dim=0).values
        soft = v - torch.as_tensor(log_temp, dtype=dt).exp() * logp
        return _t(rew, dt) + gamma * (1.0 - _t(ter, dt)) * soft


def sac_critic_loss(qs, obs, act, y):
    return sum(((q(obs, act)[:, 0] - y) ** 2).mean() for q in qs)


def sac_actor_loss(policy, qs, log_temp, obs, eps):
    a, logp = squashed_sample(policy, obs, eps)
    qmin = torch.stack([q(obs, a)[:, 0] for q in qs]).min(dim=0).values
    return (torch.as_tensor(log_temp, dtype=policy.dt).exp() * logp - qmin).mean()


def sac_temp_grad(policy, log_temp, obs, eps):
    """(loss, d loss / d log_temp) of -(exp(log_temp) * (logp - A)).mean()"""
    with torch.no_grad():
        _, logp = squashed_sample(policy, obs, eps)
        targ = (logp - np.asarray(eps).shape[1]).mean()
        v = -(torch.as_tensor(log_temp, dtype=policy.dt).exp() * targ)
    return float(v), float(v)


class Adam(object):
    """torch.optim.Adam on a dict of arrays (or a scalar under the key 'x')"""

    def __init__(self, like, dt):
        self.m = dict((k, torch.zeros(np.shape(v), dtype=dt)) for k, v in like.items())
        self.v = dict((k, torch.zeros(np.shape(v), dtype=dt)) for k, v in like.items())
        self.t, self.dt = 0, dt

    def step(self, p, g, lr, b1=0.9, b2=0.999, eps=1e-8):
        self.t += 1
        out = {}
        for k in p:
            pk, gk = _t(p[k], self.dt), _t(g[k], self.dt)
            self.m[k] = b1 * self.m[k] + (1 - b1) * gk
            self.v[k] = b2 * self.v[k] + (1 - b2) * gk * gk
            denom = self.v[k].sqrt() / np.sqrt(1 - b2 ** self.t) + eps
            out[k] = (pk - (lr / (1 - b1 ** self.t)) * (self.m[k] / denom)).numpy()
        return out


class SAC(object):
    """MOPO's update (rl4rs_amd/offline_rl.py::MOPO.update) in ``dt`` on the CPU"""

    def __init__(self, policy, q1, q2, dt, gamma, tau, lrs, update_actor_interval=1, log_temp=0.0):
        self.dt = dt
        self.P = dict(policy=dict(policy), q1=dict(q1), q2=dict(q2), q1t=dict(q1), q2t=dict(q2))
        self.opt = dict((k, Adam(self.P[k], dt)) for k in ('policy', 'q1', 'q2'))
        self.opt['temp'] = Adam({'x': np.zeros(())}, dt)
        self.log_temp = float(log_temp)
        self.gamma, self.tau, self.lrs, self.interval = gamma, tau, lrs, update_actor_interval
        self.step = 0

    def nets(self):
        return dict((k, MLP(v, self.dt)) for k, v in self.P.items())

    def update(self, obs, act, rew, nxt, ter, noise):
        n = self.nets()
        out = {}
        y = sac_target(n['policy'], [n['q1t'], n['q2t']], self.log_temp, rew, nxt, ter, noise['eps_next'], self.gamma)
        out['y'] = y.numpy().astype(np.float64)
        loss = sac_critic_loss([n['q1'], n['q2']], obs, act, y)
        loss.backward()
        out['critic_loss'] = float(loss.detach())
        out['g_q1'], out['g_q2'] = n['q1'].grads(), n['q2'].grads()
        self.P['q1'] = self.opt['q1'].step(self.P['q1'], out['g_q1'], self.lrs[1])
        self.P['q2'] = self.opt['q2'].step(self.P['q2'], out['g_q2'], self.lrs[1])
        if self.step % self.interval == 0:
            n = self.nets()
            loss = sac_actor_loss(n['policy'], [n['q1'], n['q2']], self.log_temp, obs, noise['eps_actor'])
            loss.backward()
            out['actor_loss'] = float(loss.detach())
            out['g_policy'] = n['policy'].grads()
            self.P['policy'] = self.opt['policy'].step(self.P['policy'], out['g_policy'], self.lrs[0])
            n = self.nets()
            out['temp_loss'], g = sac_temp_grad(n['policy'], self.log_temp, obs, noise['eps_temp'])
            out['g_temp'] = g
            self.log_temp = float(self.opt['temp'].step({'x': np.asarray(self.log_temp)}, {'x': np.asarray(g)}, self.lrs[2])['x'])
            for s, t in (('q1', 'q1t'), ('q2', 'q2t')):
                self.P[t] = dict((k, ((1.0 - self.tau) * _t(self.P[t][k], self.dt) + self.tau * _t(self.P[s][k], self.dt)).numpy())
                                 for k in self.P[t])
        self.step += 1
        return out


# ---------------------------------------------------------------------------------------------------------------- test inputs
def make_case(D, E, H1, H2, M, B, seed, use_dense=True, scalers=True, bias_shift=(1.0, 0.5)):
    """Parameters off their initial values (biases, batch-norm weights and the ls bounds moved, so that a wrong index shows),
    inputs of unit scale, masks, indices and noise - everything a test hands to both sides."""
    from rl4rs_amd import dynamics as dyn
    rs = np.random.RandomState(seed)
    flat_p, flat_s = dyn.init_dynamics(D, E, H1, H2, M, use_dense, seed)
    P = [dict((k, v.copy()) for k, v in d.items()) for d in dyn.unflatten(flat_p, dyn.param_shapes(D, E, H1, H2, use_dense), M)]
    S = [dict((k, v.copy()) for k, v in d.items()) for d in dyn.unflatten(flat_s, dyn.state_shapes(D, E, H1, H2, use_dense), M)]
    for p in P:
        for k in ('b1', 'b2', 'bh', 'bn1_b', 'bn2_b'):
            p[k] += (0.1 * rs.standard_normal(p[k].shape)).astype(np.float32)
        p['b1'] += np.float32(bias_shift[0])    # most units active on most rows: no batch-norm column without variance
        p['b2'] += np.float32(bias_shift[1])
        for k in ('bn1_w', 'bn2_w'):
            p[k] += (0.2 * rs.standard_normal(p[k].shape)).astype(np.float32)
        p['max_ls'] = (0.5 + 0.3 * rs.standard_normal(p['max_ls'].shape)).astype(np.float32)
        p['min_ls'] = (-1.5 + 0.3 * rs.standard_normal(p['min_ls'].shape)).astype(np.float32)
    O = D + 1
    for p, s in zip(P, S):
        # u / v a few power iterations in, as in a model that has trained: sigma = u^T W v is then near the spectral norm, not the
        # near-zero product of two random directions
        for wk, uk, vk in (('w1', 'u1', 'v1'), ('w2', 'u2', 'v2'), ('wh', 'u3', 'v3')):
            W = np.asarray(p[wk], np.float64)[:, :O] if wk == 'wh' else np.asarray(p[wk], np.float64)
            u = np.asarray(s[uk], np.float64)
            for _ in range(3):
                v = W @ u
                v /= np.linalg.norm(v)
                u = W.T @ v
                u /= np.linalg.norm(u)
            s[uk], s[vk] = u.astype(np.float32), v.astype(np.float32)
    for s in S:
        for k in ('rm1', 'rm2'):
            s[k] = (0.1 + 0.05 * rs.standard_normal(s[k].shape)).astype(np.float32)
        for k in ('rv1', 'rv2'):
            s[k] = (0.5 + 0.2 * rs.uniform(size=s[k].shape)).astype(np.float32)
    x = rs.standard_normal((B, D)).astype(np.float32)
    sc = None
    if scalers:
        mn = (x.min(axis=0) - 0.1).astype(np.float32)
        sc = dict(obs_min=mn, obs_range=((x.max(axis=0) + 0.1).astype(np.float32) - mn).astype(np.float32),
                  rew=np.array([0.3, 1.7], np.float32))
    a = np.tanh(rs.standard_normal((B, E))).astype(np.float32)
    nxt = (x + 0.1 * rs.standard_normal((B, D))).astype(np.float32)
    rew = rs.standard_normal(B).astype(np.float32)
    mask = (rs.uniform(size=(M, B)) < 0.5).astype(np.float32)
    indices = rs.randint(0, M, size=B).astype(np.int32)
    noise = rs.standard_normal((M, B, D + 1)).astype(np.float32)
    return dict(P=P, S=S, x=x, a=a, nxt=nxt, rew=rew, mask=mask, indices=indices, noise=noise, sc=sc,
                shape=(D, E, H1, H2, M, B), use_dense=use_dense)


def flat_state(case, S=None):
    from rl4rs_amd import dynamics as dyn
    D, E, H1, H2, M, B = case['shape']
    S = case['S'] if S is None else S
    sc = case['sc'] or dict(obs_min=np.zeros(D, np.float32), obs_range=np.ones(D, np.float32), rew=np.array([0.0, 1.0], np.float32))
    return np.concatenate([dyn.flatten(S, dyn.state_shapes(D, E, H1, H2, case['use_dense'])), dyn.flatten([sc], dyn.scaler_shapes(D))])


def flat_params(case, P=None):
    from rl4rs_amd import dynamics as dyn
    D, E, H1, H2, M, B = case['shape']
    return dyn.flatten(case['P'] if P is None else P, dyn.param_shapes(D, E, H1, H2, case['use_dense']))


def check_conditions(outs):
    """the issue's condition on the inputs, asserted on the float64 restatement: batch variance of every batch-norm column above
    1e-3, |u^T W v| above 0.1 for every normalised matrix"""
    for o in outs:
        for k in ('var1', 'var2'):
            if k in o:
                assert float(o[k].min()) > 1e-3, (k, float(o[k].min()))
        assert float(o['sigma'].abs().min()) > 0.1, o['sigma']


def maxdiff(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())
