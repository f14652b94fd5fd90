"""Probabilistic ensemble dynamics model on the device - the ``dynamics`` stage of the reference's batch-RL driver
(script/batchrl_trainer.py:15-33, ``d3rlpy.dynamics.ProbabilisticEnsembleDynamics``) and what ``offline_rl.MOPO`` rolls out.

d3rlpy is absent here (PARITY UNPINNED): the network, the loss and the prediction rule are d3rlpy 0.91's published form as restated
in DESIGN.md ("Ensemble dynamics model and MOPO"); ``tests/dynamics_ref.py`` is the float64 torch restatement every kernel is
checked against.  All arithmetic runs through ``librl4rs_hip`` (``rl4rs_dyn_*``, csrc/dynamics.hip); this module holds the flat
layouts, the initialisers, the scalers and the loop.
"""
import numpy as np
import torch

from . import device as D_
from .offline_rl import StandardRewardScaler, transitions_from_mdp


def param_shapes(D, E, H1, H2, use_dense=True):
    """One member's parameters in flat order (matrices [in, out])."""
    O, K1 = D + 1, D + E
    K2 = H1 + K1 if use_dense else H1
    return [('w1', (K1, H1)), ('b1', (H1,)), ('bn1_w', (H1,)), ('bn1_b', (H1,)), ('w2', (K2, H2)), ('b2', (H2,)), ('bn2_w', (H2,)),
            ('bn2_b', (H2,)), ('wh', (H2, 2 * O)), ('bh', (2 * O,)), ('max_ls', (O,)), ('min_ls', (O,))]


def state_shapes(D, E, H1, H2, use_dense=True):
    """One member's non-trained state in flat order; the scaler constants (``scaler_shapes``) follow the last member."""
    O, K1 = D + 1, D + E
    K2 = H1 + K1 if use_dense else H1
    return [('u1', (H1,)), ('v1', (K1,)), ('u2', (H2,)), ('v2', (K2,)), ('u3', (O,)), ('v3', (H2,)), ('rm1', (H1,)), ('rv1', (H1,)),
            ('rm2', (H2,)), ('rv2', (H2,))]


def scaler_shapes(D):
    return [('obs_min', (D,)), ('obs_range', (D,)), ('rew', (2,))]


def stats_shapes(H1, H2):
    return [('sigma', (3,)), ('mean1', (H1,)), ('var1', (H1,)), ('mean2', (H2,)), ('var2', (H2,))]


def unflatten(flat, shapes, members=1):
    """List (one dict per member) of views into ``flat`` (numpy array or tensor)."""
    out, o = [], 0
    for _ in range(members):
        d = {}
        for name, shape in shapes:
            n = int(np.prod(shape))
            d[name] = flat[o:o + n].reshape(shape)
            o += n
        out.append(d)
    return out


def flatten(dicts, shapes):
    return np.ascontiguousarray(np.concatenate([np.asarray(d[name], dtype=np.float32).reshape(-1) for d in dicts for name, _ in shapes]))


def init_dynamics(D, E, H1, H2, members, use_dense=True, seed=0):
    """(flat params, flat state without scalers): torch's default Linear initialiser, batch-norm weight 1 / bias 0, max_ls 2,
    min_ls -10, u / v normalised Gaussian draws, running mean 0 / variance 1 - what d3rlpy builds before ``fit``."""
    rs = np.random.RandomState(seed)
    O = D + 1

    def linear(fan_in, fan_out):
        k = 1.0 / np.sqrt(fan_in)
        return rs.uniform(-k, k, size=(fan_in, fan_out)).astype(np.float32), rs.uniform(-k, k, size=(fan_out,)).astype(np.float32)

    def unit(n):
        v = rs.standard_normal(n)
        return (v / max(np.linalg.norm(v), 1e-12)).astype(np.float32)

    ps, ss = [], []
    for _ in range(members):
        p, s = {}, {}
        p['w1'], p['b1'] = linear(D + E, H1)
        p['w2'], p['b2'] = linear(H1 + D + E if use_dense else H1, H2)
        wmu, bmu = linear(H2, O)
        wls, bls = linear(H2, O)
        p['wh'], p['bh'] = np.concatenate([wmu, wls], axis=1), np.concatenate([bmu, bls])
        p['bn1_w'], p['bn1_b'] = np.ones(H1, np.float32), np.zeros(H1, np.float32)
        p['bn2_w'], p['bn2_b'] = np.ones(H2, np.float32), np.zeros(H2, np.float32)
        p['max_ls'], p['min_ls'] = np.full(O, 2.0, np.float32), np.full(O, -10.0, np.float32)
        for k, (name, shape) in enumerate(state_shapes(D, E, H1, H2, use_dense)):
            s[name] = unit(shape[0]) if k < 6 else (np.ones(shape, np.float32) if name.startswith('rv') else np.zeros(shape, np.float32))
        ps.append(p)
        ss.append(s)
    return flatten(ps, param_shapes(D, E, H1, H2, use_dense)), flatten(ss, state_shapes(D, E, H1, H2, use_dense))


class MinMaxScaler(object):
    """d3rlpy ``scaler='min_max'``: (x - min) / (max - min) per column, fitted on the dataset's observations.  A column with
    max == min maps to 0 (stated deviation: d3rlpy divides by zero) and reverses to its constant."""

    def __init__(self, observations=None, minimum=None, maximum=None):
        if observations is not None:
            x = torch.as_tensor(observations, dtype=torch.float32)
            minimum, maximum = x.min(dim=0).values, x.max(dim=0).values
        self.min = torch.as_tensor(minimum, dtype=torch.float32).cpu()
        self.range = (torch.as_tensor(maximum, dtype=torch.float32).cpu() - self.min)

    def transform(self, x):
        mn, rg = self.min.to(x.device), self.range.to(x.device)
        return torch.where(rg > 0, (x - mn) / torch.where(rg > 0, rg, torch.ones_like(rg)), torch.zeros_like(x))

    def reverse_transform(self, y):
        return y * self.range.to(y.device) + self.min.to(y.device)


class ProbabilisticEnsembleDynamics(object):
    """``d3rlpy.dynamics.ProbabilisticEnsembleDynamics`` as script/batchrl_trainer.py builds it (``learning_rate=1e-4``, ``use_gpu``;
    every other default is d3rlpy 0.91's).  ``scaler`` / ``reward_scaler``: a name ('min_max' / 'standard', fitted by ``fit_mdp`` on
    the dataset), a fitted ``MinMaxScaler`` / ``StandardRewardScaler``, or None.  Observations and rewards go in and come out in
    raw units; the variance stays in scaled units, as in d3rlpy."""

    def __init__(self, config, obs_dim, action_size=None, n_ensembles=5, hidden_units=(256, 128), use_batch_norm=True, dropout_rate=0.2,
                 use_dense=True, spectral_norm=True, batch_size=512, learning_rate=1e-4, variance_type='max', scaler='min_max',
                 reward_scaler='standard', discrete_action=False, predict_rows=8192, seed=0, device=None):
        if discrete_action:
            raise ValueError('ProbabilisticEnsembleDynamics here models continuous actions only (the reference reaches the dynamics '
                             'model with support_conti_env); discrete_action=True is not built')
        if variance_type not in D_.DeviceDynamics.VARIANCE_TYPES:
            raise ValueError("variance_type must be 'max' or 'data'")
        self.config = config
        self.D = int(obs_dim)
        self.E = int(action_size if action_size is not None else config['action_emb_size'])
        self.M, self.hidden_units = int(n_ensembles), (int(hidden_units[0]), int(hidden_units[1]))
        self.batch_size, self.lr = int(batch_size), float(learning_rate)
        self.variance_type = variance_type
        self.scaler, self.reward_scaler = scaler, reward_scaler
        self.seed = int(seed)
        self.total_step = 0
        self.use_dense = bool(use_dense)
        params, state = init_dynamics(self.D, self.E, self.hidden_units[0], self.hidden_units[1], self.M, self.use_dense, seed)
        state = np.concatenate([state, self._scaler_constants()])
        self.net = D_.DeviceDynamics(self.D, self.E, params, state, self.hidden_units, self.M, max_rows=max(int(predict_rows), self.batch_size),
                                     max_grad_rows=self.batch_size, use_batch_norm=use_batch_norm, dropout_rate=dropout_rate,
                                     use_dense=use_dense, spectral_norm=spectral_norm, device=device)
        self.device = self.net.device
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(self.seed)

    # ------------------------------------------------------------------ scalers
    def _scaler_constants(self):
        """obs min [D], obs range [D], reward mean, reward scale - identity for a scaler that is absent or not fitted yet"""
        mn, rg = np.zeros(self.D, np.float32), np.ones(self.D, np.float32)
        if isinstance(self.scaler, MinMaxScaler):
            mn, rg = self.scaler.min.numpy().astype(np.float32), self.scaler.range.numpy().astype(np.float32)
        rw = np.array([0.0, 1.0], np.float32)
        if isinstance(self.reward_scaler, StandardRewardScaler):
            rw = np.array([self.reward_scaler.mean, self.reward_scaler.std + self.reward_scaler.eps], np.float32)
        return np.concatenate([mn, rg, rw]).astype(np.float32)

    def _push_scalers(self):
        st = self.net.state()
        c = torch.from_numpy(self._scaler_constants()).to(self.device)
        st[-c.numel():] = c
        self.net.set_state(st)

    def _require_fitted(self):
        if isinstance(self.scaler, str) or isinstance(self.reward_scaler, str):
            raise ValueError('a scaler given by name is fitted by fit_mdp(dataset); pass a fitted MinMaxScaler / StandardRewardScaler '
                             '(or None) to use update / fit / predict directly')

    # ------------------------------------------------------------------ training
    def update(self, obs, act, rew, nxt, ter=None, mask=None, seed=None):
        """One Adam step on a minibatch; ``mask`` float [members, B] (default: Bernoulli(1/2) from the seeded generator).
        Returns the per-member loss [members] (device tensor)."""
        self._require_fitted()
        B = obs.shape[0]
        if mask is None:
            mask = (torch.rand((self.M, B), generator=self._gen, device=self.device) < 0.5).to(torch.float32)
        loss = self.net.loss_grad(obs.contiguous(), act.contiguous(), nxt.contiguous(), rew.reshape(-1).contiguous(),
                                  mask.to(device=self.device, dtype=torch.float32).contiguous(),
                                  seed=self.seed if seed is None else seed, step=self.total_step)
        self.net.adam_step(self.lr)
        self.total_step += 1
        return loss

    def fit(self, transitions, n_steps, shuffle_seed=None, eval_transitions=None, n_steps_per_epoch=None, to_host=True):
        """``n_steps`` updates, epoch-wise random permutation.  Returns {'loss': per-step ensemble loss, and - with
        ``eval_transitions`` - 'observation_error' / 'reward_error' / 'variance': one value per epoch of ``n_steps_per_epoch``
        updates (default: one pass over the transitions)}."""
        self._require_fitted()
        obs, act, rew, nxt, ter = [t.to(self.device) for t in transitions]
        n = obs.shape[0]
        assert n >= self.batch_size, 'dataset smaller than one minibatch'
        assert act.dim() == 2 and act.shape[1] == self.E and act.dtype == torch.float32, 'continuous actions [N, %d] needed' % self.E
        per_epoch = int(n_steps_per_epoch) if n_steps_per_epoch else max(n // self.batch_size, 1)
        rs = np.random.RandomState(self.seed if shuffle_seed is None else shuffle_seed)
        losses, scores, ep, pos = [], {'observation_error': [], 'reward_error': [], 'variance': []}, None, n
        for k in range(n_steps):
            if pos + self.batch_size > n:
                perm = torch.from_numpy(rs.permutation(n)).to(self.device)
                ep = [t[perm] for t in (obs, act, rew, nxt)]
                pos = 0
            lo, hi = pos, pos + self.batch_size
            pos = hi
            losses.append(self.update(*[t[lo:hi] for t in ep]).sum())
            if eval_transitions is not None and (k + 1) % per_epoch == 0:
                for name, v in self.score(eval_transitions, epoch=(k + 1) // per_epoch).items():
                    scores[name].append(v)
        out = {'loss': torch.stack(losses) if losses else torch.zeros(0, device=self.device)}
        out.update(dict((k, torch.stack(v)) for k, v in scores.items() if v))
        if to_host:
            out = dict((k, [float(x) for x in v.cpu()]) for k, v in out.items())
        return out

    def fit_mdp(self, data, n_epochs=1, eval_data=None, **kw):
        """``fit`` on MDPDataset-style arrays for ``n_epochs`` passes; scalers given by name are fitted on ``data`` first."""
        tr = transitions_from_mdp(data['observations'], data['actions'], data['rewards'], data['terminals'], discrete_action=False)
        if self.scaler == 'min_max':
            self.scaler = MinMaxScaler(data['observations'])
        if self.reward_scaler == 'standard':
            self.reward_scaler = StandardRewardScaler(tr[2])
        self._push_scalers()
        ev = None
        if eval_data is not None:
            ev = transitions_from_mdp(eval_data['observations'], eval_data['actions'], eval_data['rewards'], eval_data['terminals'],
                                      discrete_action=False)
        per = tr[0].shape[0] // self.batch_size
        return self.fit(tr, int(n_epochs) * per, eval_transitions=ev, n_steps_per_epoch=per, **kw)

    # ------------------------------------------------------------------ prediction
    def predict(self, x, action, with_variance=False, indices=None, noise=None, deterministic=False, seed=None, step=0, lam=None):
        """(next observation [N, D], reward [N, 1]) (+ variance [N, 1]) of one ensemble member per row: ``indices`` int [N] (default:
        uniform over members from the counter hash of (seed, step, row)); ``noise`` [members, N, D + 1] (default: the counter
        hash's Gaussian); ``lam``: the reward is returned as r - lam * variance (MOPO)."""
        self._require_fitted()
        x = D_._dev_tensor(x, torch.float32, self.device)
        action = D_._dev_tensor(action, torch.float32, self.device)
        N = x.shape[0]
        if indices is not None:
            indices = D_._dev_tensor(indices, torch.int32, self.device)
        if noise is not None:
            noise = D_._dev_tensor(noise, torch.float32, self.device)
        nx = torch.empty((N, self.D), dtype=torch.float32, device=self.device)
        r = torch.empty((N, 1), dtype=torch.float32, device=self.device)
        var = torch.empty((N, 1), dtype=torch.float32, device=self.device)
        rows = self.net.max_rows
        seed = self.seed if seed is None else seed
        for k, lo in enumerate(range(0, N, rows)):
            hi = min(lo + rows, N)
            o = self.net.predict(x[lo:hi].contiguous(), action[lo:hi].contiguous(),
                                 indices=None if indices is None else indices[lo:hi].contiguous(),
                                 noise=None if noise is None else noise[:, lo:hi].contiguous(), seed=seed, step=step * 65537 + k,
                                 deterministic=deterministic, variance_type=self.variance_type, lam=lam)
            nx[lo:hi], r[lo:hi, 0], var[lo:hi, 0] = o[:3]
        return (nx, r, var) if with_variance else (nx, r)

    def score(self, transitions, epoch=0):
        """The three scorers the script passes to ``fit``: means over the transitions of the squared observation error summed over
        columns, the squared reward error and the predicted variance (device scalars); the prediction is ``predict``'s sample
        at (seed, step = epoch)."""
        obs, act, rew, nxt = [t.to(self.device) for t in transitions[:4]]
        nx, r, var = self.predict(obs, act, with_variance=True, step=epoch)
        return {'observation_error': ((nx - nxt) ** 2).sum(dim=1).mean(), 'reward_error': ((r[:, 0] - rew.reshape(-1)) ** 2).mean(),
                'variance': var.mean()}

    # ------------------------------------------------------------------ files
    def save_model(self, fname):
        self._require_fitted()
        m, v, t = self.net.adam_state()
        blob = {'__class__': np.array(type(self).__name__), 'total_step': np.array(self.total_step, dtype=np.int64),
                'shape': np.array([self.D, self.E, self.hidden_units[0], self.hidden_units[1], self.M, int(self.use_dense)], dtype=np.int64),
                'params': self.net.flat_params().cpu().numpy(), 'state': self.net.state().cpu().numpy(),
                'adam_m': m.cpu().numpy(), 'adam_v': v.cpu().numpy(), 'adam_t': np.array(t, dtype=np.int64),
                'has_scaler': np.array([self.scaler is not None, self.reward_scaler is not None])}
        if self.reward_scaler is not None:
            blob['reward_scaler'] = np.array([self.reward_scaler.mean, self.reward_scaler.std, self.reward_scaler.eps], dtype=np.float64)
        with open(fname, 'wb') as f:
            np.savez(f, **blob)

    def load_model(self, fname):
        with np.load(fname) as z:
            if str(z['__class__']) != type(self).__name__:
                raise ValueError('%s holds a %s, this is a %s' % (fname, str(z['__class__']), type(self).__name__))
            shape = [self.D, self.E, self.hidden_units[0], self.hidden_units[1], self.M, int(self.use_dense)]
            if list(z['shape']) != shape:
                raise ValueError('%s: model shape %s in the file, %s here' % (fname, list(z['shape']), shape))
            self.total_step = int(z['total_step'])
            state = torch.from_numpy(np.ascontiguousarray(z['state'], dtype=np.float32))
            self.net.set_flat_params(torch.from_numpy(np.ascontiguousarray(z['params'], dtype=np.float32)).to(self.device))
            self.net.set_state(state)
            self.net.set_adam_state(torch.from_numpy(z['adam_m']), torch.from_numpy(z['adam_v']), int(z['adam_t']))
            has = z['has_scaler']
            sc = unflatten(state[-(2 * self.D + 2):], scaler_shapes(self.D))[0]
            self.scaler = None
            if has[0]:
                self.scaler = MinMaxScaler(minimum=sc['obs_min'], maximum=sc['obs_min'] + sc['obs_range'])
                self.scaler.range = sc['obs_range'].clone()          # the stored range itself, not (min + range) - min
            self.reward_scaler = StandardRewardScaler.from_stats(*[float(x) for x in z['reward_scaler']]) if has[1] else None

    def close(self):
        self.net.close()
