"""Inputs of the off-policy-evaluation fixtures (tests/golden/ope_*.npz), regenerated from seeds: shared by the generator
(tests/golden/make_ope_golden.py, which feeds them to the REFERENCE's functions) and the tests (which feed them to this package's).
Only outputs and small inputs are stored in the fixtures."""
import numpy as np

# (B, T, seed) of the estimator cases
ESTIMATOR_CASES = [(1, 9, 101), (7, 9, 102), (64, 9, 103), (300, 36, 104), (4096, 9, 105), (4096, 32, 106), (16384, 9, 107),
                   (100, 9, 108), (1000, 36, 109)]
# order of the recorded pairs
ESTIMATOR_NAMES = ['IPS', 'CIPS', 'SNIPS', 'DR', 'WIPS', 'WIPS_gamma0.9', 'SeqDR']
T_QUANTILE_DF = [-1, 0, 1, 2, 3, 5, 10, 30, 100, 1758, 4095, 10 ** 6]
T_QUANTILE_P = 0.99875
BEHAVIOR = dict(seed=301, B=48, A_b=382, layers=[1, 2, 3, 4])
# (B, T, with sample model, seed); three epochs each
LOOP_CASES = [(B, T, s, 400 + 10 * i + s) for i, (B, T) in enumerate([(8, 9), (64, 9), (8, 36), (64, 36)]) for s in (1, 0)]
LOOP_EPOCHS = 3
LOOP_ACTIONS = 20


def estimator_inputs(B, T, seed):
    """float64 per-step arrays [B, T] and the per-episode ones assembled like script/offline_evaluation.py:41-57.
    mu = pi * u: u near 1 for long episodes (independent draws send SeqDR to 1e19 at T >= 32), wide for short ones so that both
    clips of the ratio are exercised."""
    rs = np.random.RandomState(seed)
    pi = rs.uniform(0.02, 0.9, size=(B, T))
    u = rs.uniform(0.97, 1.03, size=(B, T)) if T >= 32 else rs.uniform(0.6, 1.6, size=(B, T))
    mu = pi * u
    step_rewards = rs.uniform(0.0, 3.0, size=(B, T)) * (rs.uniform(size=(B, T)) < 0.4)
    step_rewards[:, -1] += rs.uniform(0.5, 2.0, size=B)                  # every episode pays something
    rhat = rs.uniform(0.0, 3.0, size=(B, T))
    q = rs.uniform(0.0, 10.0, size=(B, T))
    return dict(pi=pi, mu=mu, step_rewards=step_rewards, rhat=rhat, q=q, **episode_inputs(pi, mu, step_rewards, rhat, q))


def episode_inputs(pi, mu, step_rewards, rhat, q):
    """offline_evaluation.py:38-57 on [B, T] arrays"""
    return dict(rewards=np.sum(step_rewards, axis=1), pi_mul=np.multiply.reduce(pi * 100, axis=1),
                mu_mul=np.multiply.reduce(mu * 100, axis=1), episode_reward=np.sum(rhat, axis=1), q_mean=np.average(q, 1))


def behavior_inputs():
    """y [B, 382] float64 holding float32-representable positive scores, actions [B] with 0, range ends and out-of-range ids"""
    c = BEHAVIOR
    rs = np.random.RandomState(c['seed'])
    y = rs.uniform(0.001, 1.0, size=(c['B'], c['A_b'])).astype(np.float32).astype(np.float64)
    actions = rs.randint(0, c['A_b'], size=c['B']).astype(np.int64)
    actions[:12] = [0, 1, 39, 40, 147, 148, 381, 382, 500, 38, 149, 283]
    return y, actions


class _Samples(object):
    records = None


class LoopTables(object):
    """Table-driven fake env + policy + sample model for ope_eval: per epoch and step, arrays drawn from a seed.  Probabilities
    are float32-representable float64 (the device path takes float32 score matrices)."""

    def __init__(self, B, T, seed):
        rs = np.random.RandomState(seed)
        E, A = LOOP_EPOCHS, LOOP_ACTIONS
        self.B, self.T = B, T
        p = rs.uniform(0.05, 1.0, size=(E, T, B, A))
        self.probs = (p / p.sum(axis=3, keepdims=True)).astype(np.float32).astype(np.float64)
        self.off_action = rs.randint(0, A, size=(E, T, B))
        self.action = rs.randint(0, A, size=(E, T, B))
        u = rs.uniform(0.97, 1.03, size=(E, T, B)) if T >= 32 else rs.uniform(0.6, 1.6, size=(E, T, B))
        sel = np.take_along_axis(self.probs, self.off_action[..., None], axis=3)[..., 0]
        self.mu = sel * u
        self.q = rs.uniform(0.0, 10.0, size=(E, T, B))
        self.reward = rs.uniform(0.0, 3.0, size=(E, T, B))
        self.off_reward = np.zeros((E, T, B))
        self.off_reward[:, -1] = rs.uniform(0.5, 20.0, size=(E, B))
        self.epoch, self.j = -1, 0
        self.samples = _Samples()

    # env
    def reset(self):
        self.epoch += 1
        self.j = 0
        return np.zeros((self.B, 4), np.float32)

    @property
    def offline_action(self):
        return self.off_action[self.epoch, self.j]

    @property
    def offline_reward(self):
        return list(self.off_reward[self.epoch, self.j - 1])

    def step(self, action):
        r = list(self.reward[self.epoch, self.j])
        self.j += 1
        return np.zeros((self.B, 4), np.float32), r, [int(self.j >= self.T)] * self.B, [{}] * self.B

    # policy
    def predict_with_mask(self, obs):
        return self.action[self.epoch, self.j]

    def action_probs(self, *args, **kw):
        if len(args) == 1:                                  # policy.action_probs(obs)
            return self.probs[self.epoch, self.j]
        return self.mu[self.epoch, self.j]                  # sample_model.action_probs(records, action, layer, page=)

    def predict_q(self, obs, action):
        return self.q[self.epoch, self.j]
