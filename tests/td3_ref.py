"""TEST INFRASTRUCTURE ONLY - float64 restatement (torch autograd on oracle.offline_conti.OracleAMLP) of the on-device TD3 / DDPG
(rl4rs_amd/csrc/td3.hpp, rl4rs_amd.train.TD3Learner / TD3Trainer): RLlib 1.5.1's ddpg_tf_policy / ddpg_tf_model /
OrnsteinUhlenbeckNoise as the reference's script/modelfree_train.py:46-48,79-105 configures them.

PARITY UNPINNED: ray is absent from this image and the reference holds no vector for these learners; what follows restates the
published form -
  ddpg_tf_model     actor Dense(relu) x 2 -> Dense(E) -> sigmoid(2x) * (high - low) + low  (= tanh(x) on Box(-1, 1));
                    critics Dense(relu) x 2 on cat([obs, action]) -> 1
  ddpg_tf_policy    a' = target actor(s') (+ clip(N(0, target_noise), +-noise_clip), clipped to the box, when smooth_target_policy);
                    q' = min of the target critics (twin_q);  y = r + gamma^n (1 - done) q';  errors = huber(td) or 0.5 td^2, summed over
                    the critics;  critic_loss = mean(w * errors), actor_loss = -mean(q1(s, pi(s)));  l2_reg * tf.nn.l2_loss(var) on every
                    non-bias variable of the respective loss;  BOTH gradients are taken from the parameters before the step (one
                    session run), Adam (tf.keras epsilon 1e-7) on each, then update_target: targ = tau * online + (1 - tau) * targ
  OrnsteinUhlenbeckNoise   state += theta * (-state) + sigma * N(0, 1);  action = clip(det + scale * base_scale * state * (high - low))
Adam is oracle.offline_rl.torch_adam (the form rl4rs_amlp_adam_step implements) with eps 1e-7."""
import numpy as np
import torch

from oracle.offline_conti import OracleAMLP
from oracle.offline_rl import torch_adam

NAMES = ('fc1_w', 'fc1_b', 'fc2_w', 'fc2_b', 'head_w', 'head_b')
WEIGHTS = ('fc1_w', 'fc2_w', 'head_w')


def _t(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float64)


M32 = np.uint64(0xffffffff)


def mix32(x):
    """The library's 32-bit mixer (policy.hip), on uint64 arrays holding 32-bit values."""
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & M32
    x ^= x >> np.uint64(16)
    return x


def uniform01(seed, step, row, col):
    """The library's counter RNG: a pure function of (seed, step, row, column), 23 bits + 0.5, exactly representable in float32."""
    row, col = np.asarray(row, dtype=np.uint64), np.asarray(col, dtype=np.uint64)
    s = mix32((np.uint64(step) * np.uint64(0x9E3779B9) + np.uint64(0x85EBCA6B)) & M32)
    r = mix32((row * np.uint64(0xC2B2AE35) + col * np.uint64(0x27D4EB2F) + np.uint64(1)) & M32)
    h = mix32((np.uint64(seed & 0xffffffff) ^ s ^ r) & M32)
    h = mix32((h + col) & M32)
    return ((h >> np.uint64(9)).astype(np.float64) + 0.5) / 8388608.0


def normal01(seed, step, row, col):
    """Box-Muller on uniform01(.., 2 col) and uniform01(.., 2 col + 1); the angle is formed in float32 as the kernel forms it."""
    col = np.asarray(col, dtype=np.uint64)
    u1, u2 = uniform01(seed, step, row, 2 * col), uniform01(seed, step, row, 2 * col + np.uint64(1))
    ang = (np.float32(6.28318530717958647692) * u2.astype(np.float32)).astype(np.float64)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(ang)


def explore_keys(N, E, rows):
    """(row key, column key) [N, E] of rl4rs_explore_ou's noise: the state row (0 for a shared state) and the column."""
    n, e = np.meshgrid(np.arange(N), np.arange(E), indexing='ij')
    return (np.zeros_like(n) if rows == 1 else n), e


def ou_step(state, eps, det, theta, sigma, scale):
    """One exploration step.  state / eps: [rows, E] with rows = N or 1 (shared by all rows); det [N, E].  -> (new state, action)."""
    state = np.asarray(state, dtype=np.float64)
    state = state + theta * (-state) + sigma * np.asarray(eps, dtype=np.float64)
    action = np.clip(np.asarray(det, dtype=np.float64) + scale * state * 2.0, -1.0, 1.0)
    return state, action


def smooth_action(a, eps, target_noise, noise_clip):
    """-> (smoothed action, mask of the elements where the noise clip binds, mask where the box clip binds)."""
    a, z = np.asarray(a, dtype=np.float64), target_noise * np.asarray(eps, dtype=np.float64)
    zc = np.clip(z, -noise_clip, noise_clip)
    out = np.clip(a + zc, -1.0, 1.0)
    return out, np.abs(z) > noise_clip, np.abs(a + zc) > 1.0


def huber(x, delta):
    ax = x.abs()
    return torch.where(ax < delta, 0.5 * x * x, delta * (ax - 0.5 * delta))


def critic_terms(q1, q2, q1t, q2t, rew, done, w, gamma, use_huber, delta):
    """torch float64, differentiable in q1 / q2 (q2 / q2t None: the single critic).  -> dict y, td1, err [N], loss."""
    rew, done = _t(rew), torch.as_tensor(np.asarray(done) != 0)
    qn = _t(q1t) if q2t is None else torch.minimum(_t(q1t), _t(q2t))
    y = torch.where(done, rew, rew + gamma * qn)            # a select: a NaN target Q of a terminal row reaches nothing
    f = (lambda x: huber(x, delta)) if use_huber else (lambda x: 0.5 * x * x)
    td1 = q1 - y
    err = f(td1)
    if q2 is not None:
        err = err + f(q2 - y)
    wt = _t(w) if w is not None else torch.ones_like(y)
    return dict(y=y, td1=td1, err=err, w=wt, loss=(wt * err).mean())


def critic_loss_and_grads(q1, q2, q1t, q2t, rew, done, w, gamma, use_huber, delta):
    """The HAND-WRITTEN form of what rl4rs_td3_critic_loss computes (numpy float64): y, td, dq1, dq2, stats4."""
    q1 = np.asarray(q1, dtype=np.float64)
    N = q1.shape[0]
    rew = np.asarray(rew, dtype=np.float64)
    qn = np.asarray(q1t, dtype=np.float64) if q2t is None else np.minimum(np.asarray(q1t, dtype=np.float64), np.asarray(q2t, dtype=np.float64))
    y = np.where(np.asarray(done) != 0, rew, rew + gamma * qn)
    wt = np.asarray(w, dtype=np.float64) if w is not None else np.ones(N)

    def f(td):
        if not use_huber:
            return 0.5 * td * td, td
        return np.where(np.abs(td) < delta, 0.5 * td * td, delta * (np.abs(td) - 0.5 * delta)), np.clip(td, -delta, delta)

    td1 = q1 - y
    e1, d1 = f(td1)
    out = dict(y=y, td=td1, dq1=wt * d1 / N, dq2=None)
    err = e1
    if q2 is not None:
        e2, d2 = f(np.asarray(q2, dtype=np.float64) - y)
        err = err + e2
        out['dq2'] = wt * d2 / N
    out['stats'] = np.array([(wt * err).sum(), q1.sum(), y.sum(), np.abs(td1).sum()])
    out['loss'] = (wt * err).mean()
    return out


def l2_term(net, l2):
    """l2_reg * sum over the non-bias variables of tf.nn.l2_loss(var) = l2 / 2 * sum W^2."""
    return l2 * sum(0.5 * (net.p[k] ** 2).sum() for k in WEIGHTS)


class TD3Ref(object):
    """Six (four for DDPG) parameter dicts in float64 + Adam state; ``update`` follows the both-gradients-before-the-step order."""

    def __init__(self, params, twin_q=True, smooth=True, target_noise=0.2, noise_clip=0.5, tau=5e-3, l2_reg=0.0, gamma=1.0,
                 actor_lr=1e-3, critic_lr=1e-3, use_huber=False, huber_threshold=1.0):
        self.twin_q, self.smooth = twin_q, smooth
        self.target_noise, self.noise_clip, self.tau, self.l2, self.gamma = target_noise, noise_clip, tau, l2_reg, gamma
        self.actor_lr, self.critic_lr, self.use_huber, self.delta = actor_lr, critic_lr, use_huber, huber_threshold
        names = ['actor', 'actor_targ', 'q1', 'q1_targ'] + (['q2', 'q2_targ'] if twin_q else [])
        self.p = dict((n, dict((k, np.asarray(params[n][k], dtype=np.float64).copy()) for k in NAMES)) for n in names)
        self.adam = dict((n, dict(m=dict((k, np.zeros_like(self.p[n][k])) for k in NAMES),
                                  v=dict((k, np.zeros_like(self.p[n][k])) for k in NAMES), t=0))
                         for n in names if not n.endswith('_targ'))

    def flat(self, name):
        return np.concatenate([self.p[name][k].reshape(-1) for k in NAMES])

    def _adam(self, name, grads, lr):
        a = self.adam[name]
        a['t'] += 1
        self.p[name] = torch_adam(self.p[name], grads, a['m'], a['v'], a['t'], lr, eps=1e-7)

    def update(self, obs, act, rew, done, nxt, noise=None, weights=None, do_actor=True):
        critics = ['q1', 'q2'] if self.twin_q else ['q1']
        actor, actor_t = OracleAMLP(self.p['actor'], 'tanh'), OracleAMLP(self.p['actor_targ'], 'tanh')
        qs = [OracleAMLP(self.p[n]) for n in critics]
        qts = [OracleAMLP(self.p[n + '_targ']) for n in critics]
        obs, act, nxt = _t(obs), _t(act), _t(nxt)
        with torch.no_grad():
            a_next = actor_t(nxt)
            if self.smooth:
                a_next = _t(smooth_action(a_next.numpy(), noise, self.target_noise, self.noise_clip)[0])
            qn = [q(nxt, a_next)[:, 0] for q in qts]
        qv = [q(obs, act)[:, 0] for q in qs]
        c = critic_terms(qv[0], qv[1] if self.twin_q else None, qn[0], qn[1] if self.twin_q else None, rew, done, weights, self.gamma,
                         self.use_huber, self.delta)
        closs = c['loss'] + sum(l2_term(q, self.l2) for q in qs)
        cparams = [q.p[k] for q in qs for k in NAMES]
        cg = torch.autograd.grad(closs, cparams)
        cgrads = [dict((k, cg[i * len(NAMES) + j].numpy()) for j, k in enumerate(NAMES)) for i in range(len(qs))]
        d = lambda t: t.detach()
        out = dict(critic_loss=float(d(c['loss'])), y=c['y'].numpy(), td=d(c['td1']).numpy(),
                   stats=np.array([float(d(c['w'] * c['err']).sum()), float(d(qv[0]).sum()), float(c['y'].sum()), float(d(c['td1']).abs().sum())]))
        agrads = None
        if do_actor:
            q_pi = qs[0](obs, actor(obs))[:, 0]                    # (the critic's parameters BEFORE its step)
            aloss = -q_pi.mean() + l2_term(actor, self.l2)
            ag = torch.autograd.grad(aloss, [actor.p[k] for k in NAMES])
            agrads = dict((k, ag[j].numpy()) for j, k in enumerate(NAMES))
            out.update(actor_loss=float(-q_pi.detach().mean()), actor_sum=float(-q_pi.detach().sum()))
        out.update(critic_grads=cgrads, actor_grads=agrads)
        for n, g in zip(critics, cgrads):
            self._adam(n, g, self.critic_lr)
        if do_actor:
            self._adam('actor', agrads, self.actor_lr)
        for n in critics + ['actor']:                              # update_target: ALL targets, from the stepped parameters
            self.p[n + '_targ'] = dict((k, (1.0 - self.tau) * self.p[n + '_targ'][k] + self.tau * self.p[n][k]) for k in NAMES)
        return out


def ou_scale(t, random_timesteps=0, initial_scale=1.0, final_scale=0.02, scale_timesteps=10000):
    """PiecewiseSchedule [(random_timesteps, initial), (random_timesteps + scale_timesteps, final)], outside value final."""
    lo, hi = random_timesteps, random_timesteps + scale_timesteps
    if t < lo or t >= hi:
        return final_scale
    return initial_scale + (final_scale - initial_scale) * (t - lo) / float(hi - lo)
