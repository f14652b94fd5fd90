"""Torch restatement of COMBO's update (rl4rs_amd/offline_rl.py::COMBO, DESIGN.md "COMBO") with the arithmetic type as a parameter,
in the manner of tests/dynamics_ref.py: float64 is the reference the device is compared with, the SAME code in float32 on a test's
own inputs is that test's yardstick.  d3rlpy 0.91 is absent (parity unpinned): this file states what is built.

    critic loss  = sum_c mean_{b < B} (Q_c(s_b, a_b) - y_b)^2
                   + w [ sum_c mean_{f >= n_real} logsumexp_j (Q_c(s_f, a_fj) - off_fj) - sum_c mean_{b < n_real} Q_c(s_b, a_b) ]
    y_b          = r_b + gamma (1 - ter_b) min_c Qtarg_c(s'_b, tanh(mu(s'_b)))
    a_f.         = n samples of pi(.|s_f) | n of pi(.|s'_f) | n uniform;  off = the sample's log-prob | A log 0.5

The critic loss is differentiated by autograd as ONE expression over the whole minibatch - nothing here knows of the two passes the
library runs.  Rows 0 .. n_real - 1 of a minibatch are real, the rest generated."""
import numpy as np
import torch

from dynamics_ref import MLP, Adam, maxdiff, sac_actor_loss, sac_temp_grad, squashed_sample       # noqa: F401  (maxdiff: for the tests)


def _t(x, dt):
    return torch.as_tensor(np.asarray(x), dtype=dt)


def deterministic_target(policy, q_targs, rew, nxt, ter, gamma):
    dt = policy.dt
    with torch.no_grad():
        head = policy(nxt)
        a = torch.tanh(head[:, :head.shape[1] // 2])
        v = torch.stack([q(nxt, a)[:, 0] for q in q_targs]).min(dim=0).values
        return _t(rew, dt) + gamma * (1.0 - _t(ter, dt)) * v


def conservative_rows(policy, obs_f, nxt_f, n, critic_noise):
    """-> (actions [F, 3n, A], offsets [F, 3n]) of the generated rows; constants of the critic loss"""
    dt = policy.dt
    eps_t, eps_tp1, uni = critic_noise
    uni = _t(uni, dt)
    F, _, A = uni.shape
    with torch.no_grad():
        rep = lambda x: _t(x, dt).repeat_interleave(n, dim=0)
        a_t, lp_t = squashed_sample(policy, rep(obs_f), np.asarray(eps_t).reshape(F * n, A))
        a_n, lp_n = squashed_sample(policy, rep(nxt_f), np.asarray(eps_tp1).reshape(F * n, A))
        acts = torch.cat([a_t.view(F, n, A), a_n.view(F, n, A), uni], dim=1)
        offs = torch.cat([lp_t.view(F, n), lp_n.view(F, n), torch.full((F, n), float(A * np.log(0.5)), dtype=dt)], dim=1)
    return acts, offs


def critic_terms(qs, obs, act, y, n_real, acts, offs, w):
    """-> dict(td, conservative, loss: tensors; sums: the six sums as tensors in the library's order)"""
    dt = qs[0].dt
    obs, act = _t(obs, dt), _t(act, dt)
    B, (F, k, A) = obs.shape[0], acts.shape
    obs_rep = obs[n_real:].repeat_interleave(k, dim=0)
    td, lse, data = [], [], []
    for q in qs:
        qt = q(obs, act)[:, 0]
        qc = q(obs_rep, acts.reshape(F * k, A))[:, 0].view(F, k)
        td.append(((qt - y) ** 2).sum())
        lse.append(torch.logsumexp(qc - offs, dim=1).sum())
        data.append(qt[:n_real].sum())
    out = {'td': (td[0] + td[1]) / B, 'conservative': w * ((lse[0] + lse[1]) / F - (data[0] + data[1]) / n_real)}
    out['loss'] = out['td'] + out['conservative']
    out['sums'] = td + lse + data
    return out


class COMBO(object):
    """COMBO's update in ``dt`` on the CPU.  lrs = (actor, critic, temperature)."""

    def __init__(self, policy, q1, q2, dt, gamma, tau, lrs, n_action_samples, conservative_weight, update_actor_interval=1, log_temp=0.0):
        self.dt = dt
        self.P = dict(policy=dict(policy), q1=dict(q1), q2=dict(q2), q1t=dict(q1), q2t=dict(q2))
        self.opt = dict((k, Adam(self.P[k], dt)) for k in ('policy', 'q1', 'q2'))
        self.opt['temp'] = Adam({'x': np.zeros(())}, dt)
        self.log_temp = float(log_temp)
        self.gamma, self.tau, self.lrs, self.interval = gamma, tau, lrs, update_actor_interval
        self.n, self.w = int(n_action_samples), float(conservative_weight)
        self.step = 0

    def nets(self):
        return dict((k, MLP(v, self.dt)) for k, v in self.P.items())

    def update(self, obs, act, rew, nxt, ter, n_real, noise):
        """noise: dict(critic=(eps_t [F n, A], eps_tp1 [F n, A], uniform [F, n, A]), eps_actor [B, A], eps_temp [B, A])"""
        assert 0 < n_real < np.asarray(obs).shape[0]
        n = self.nets()
        out = {}
        y = deterministic_target(n['policy'], [n['q1t'], n['q2t']], rew, nxt, ter, self.gamma)
        out['y'] = y.numpy().astype(np.float64)
        acts, offs = conservative_rows(n['policy'], np.asarray(obs)[n_real:], np.asarray(nxt)[n_real:], self.n, noise['critic'])
        terms = critic_terms([n['q1'], n['q2']], obs, act, y, n_real, acts, offs, self.w)
        terms['loss'].backward()
        out['sums'] = np.array([float(v.detach()) for v in terms['sums']])
        out['critic_loss'], out['conservative_loss'] = float(terms['loss'].detach()), float(terms['conservative'].detach())
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
        out['log_temp'] = self.log_temp
        out['params'] = dict((k, dict((kk, np.array(vv)) for kk, vv in v.items())) for k, v in self.P.items())
        return out
