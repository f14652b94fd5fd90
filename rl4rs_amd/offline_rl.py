"""Offline (batch) RL learners on the device - SURVEY section 8 row f1, BASELINE configs[4].

The reference trains d3rlpy's ``DiscreteBC`` / ``DiscreteBCQ`` / ``DiscreteCQL`` on the logged-policy ``MDPDataset``
(script/batchrl_trainer.py:34-90, :395-...), the first two with its own ``CustomVectorEncoder`` that re-derives the action
mask from the observation tail (rl4rs/nets/cql/encoder.py:9-67).  Here the same networks, losses and update rules run
through ``librl4rs_hip`` (``rl4rs_qnet_*``, ``rl4rs_qloss_*``); this module is the thin loop around them:

* ``transitions_from_mdp`` - d3rlpy 0.91's episode -> transition rule (the reward of an action is stored with the NEXT
  observation, script/batchrl_trainer.py:186-197; the terminal row yields a transition into a zero observation).
* ``DiscreteBC``  - imitator only, ``nll + beta * mean(logits^2)`` (the script passes beta = 0), Adam lr 1e-3.
* ``DiscreteBCQ`` - Q network + target + imitator; next action by the BCQ rule (action_flexibility 0.3), imitator penalty
  beta 0.5, Adam lr 6.25e-5, hard target sync every ``target_update_interval`` (8000) updates.
* ``DiscreteCQL`` - DoubleDQN + ``alpha * (logsumexp Q - Q[a])`` (alpha 1.0) on d3rlpy's default two-layer encoder, as the
  script leaves the custom factory commented out for CQL.
* ``BCQ`` - the CONTINUOUS-action learner of ``'BCQ-conti'`` (script/batchrl_trainer.py:61-73, ``d3rlpy.algos.BCQ(batch_size=256)``
  on default encoders): what BASELINE configs[4] is quoted on.  Trains on the dataset ``generate_offline_dataset`` emits for
  ``support_conti_env`` (actions = 32-d item embeddings, :220-270): conditional-VAE imitator, residual perturbation actor, twin
  critics with the lam-weighted min/max target over 100 sampled actions, soft target updates; ``predict`` returns the embedding
  the env's K-NN resolves (``env.step(policy.predict(obs))``, batchrl_trainer.py:398-399 with ``predict_with_mask`` ->
  ``predict`` for continuous envs, rl4rs/policy/policy_model.py:17-19).
* ``CQL`` - the continuous-action learner of ``'CQL-conti'`` (script/batchrl_trainer.py:91-107, ``d3rlpy.algos.CQL(batch_size=256,
  gamma=1.0, reward_scaler='standard')``; the ``alpha=`` keyword the script passes is not a parameter of the continuous CQL and
  is swallowed by d3rlpy's ``**kwargs``): SAC (squashed-Gaussian actor, learned temperature) with the conservative critic term
  over 10 policy samples at s, 10 at s' and 10 uniform actions per row, learned log-alpha with threshold 10, weight 5.

d3rlpy is absent from this image (parity unpinned): the hyper-parameter defaults above are d3rlpy 0.91's as published;
every gradient is checked against torch autograd of the restated model in ``tests/test_gpu_offline_rl.py``.  With
``torch.distributed`` initialised each rank trains on its own minibatches and the flat gradient is mean-all-reduced
before Adam (data parallel, one collective per network per update).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from . import device as D
from . import device as D_
from . import dist as rdist


def transitions_from_mdp(observations, actions, rewards, terminals, discrete_action=True):
    """(obs, act, next_reward, next_obs, terminal) tensors from MDPDataset-style arrays (rows in time order, an episode
    ends at ``terminals == 1``).  Row t of an episode gives the transition (o_t, a_t, r_{t+1}, o_{t+1}, 0); the terminal
    row gives (o_T, a_T, 0, zeros, 1); a trailing episode without terminal flag drops its last row.
    ``discrete_action=False`` (``MDPDataset(..., discrete_action=False)``, batchrl_trainer.py:266): actions stay float [N, E]."""
    obs = torch.as_tensor(observations, dtype=torch.float32)
    if discrete_action:
        act = torch.as_tensor(actions).reshape(obs.shape[0], -1)[:, 0].to(torch.int32)
    else:
        act = torch.as_tensor(actions, dtype=torch.float32).reshape(obs.shape[0], -1)
    rew = torch.as_tensor(rewards, dtype=torch.float32).reshape(-1)
    ter = torch.as_tensor(terminals, dtype=torch.float32).reshape(-1)
    n = obs.shape[0]
    is_end = ter > 0.5
    nxt = torch.roll(obs, -1, dims=0)
    nrew = torch.roll(rew, -1, dims=0)
    nxt = torch.where(is_end[:, None], torch.zeros_like(nxt), nxt)
    nrew = torch.where(is_end, torch.zeros_like(nrew), nrew)
    keep = torch.ones(n, dtype=torch.bool, device=obs.device)
    if n and not bool(is_end[-1]):
        keep[-1] = False                     # the last row has no successor and is not terminal
    return obs[keep], act[keep], nrew[keep], nxt[keep], ter[keep]


def init_qnet_params(obs_dim, action_size, mask_size=0, emb_size=32, hidden1=256, hidden2=256, seed=0):
    """torch's default initialisers (Linear: U(+-1/sqrt(fan_in)) for weight and bias; Embedding: N(0, 1)), stored [in, out]."""
    rs = np.random.RandomState(seed)

    def linear(fan_in, fan_out):
        k = 1.0 / np.sqrt(fan_in)
        return (rs.uniform(-k, k, size=(fan_in, fan_out)).astype(np.float32), rs.uniform(-k, k, size=(fan_out,)).astype(np.float32))

    p = {}
    p['fc1_w'], p['fc1_b'] = linear(obs_dim, hidden1)
    if mask_size > 0:
        p['emb'] = rs.normal(size=(action_size, emb_size)).astype(np.float32)
        p['fc2_w'], p['fc2_b'] = linear(hidden1 + mask_size * emb_size, action_size)
        p['head_w'], p['head_b'] = linear(action_size, action_size)
    else:
        p['fc2_w'], p['fc2_b'] = linear(hidden1, hidden2)
        p['head_w'], p['head_b'] = linear(hidden2, action_size)
    return p


def _epoch_minibatches(columns, batch_size, n_steps, seed, epoch_hook=None):
    """``n_steps`` minibatches over the rows of ``columns`` with an epoch-wise random permutation like d3rlpy's ``fit``.  The epoch's
    permutation is applied to the columns ONCE: minibatches are then contiguous row ranges (views), not one gather per column
    and update.  ``epoch_hook`` = (steps per epoch, f): f(epoch) runs once the consumer has used the last minibatch of an epoch
    (1-based) - the minibatches themselves are the same with and without it."""
    n = columns[0].shape[0]
    assert n >= batch_size, 'dataset smaller than one minibatch'

    def batches():
        rs = np.random.RandomState(seed)
        ep, pos = None, n
        for k in range(n_steps):
            if pos + batch_size > n:
                perm = torch.from_numpy(rs.permutation(n)).to(columns[0].device)
                ep = [t[perm] for t in columns]
                pos = 0
            yield [t[pos:pos + batch_size] for t in ep]
            pos += batch_size
            if epoch_hook is not None and (k + 1) % epoch_hook[0] == 0:
                epoch_hook[1]((k + 1) // epoch_hook[0])
    return batches()


def _score_hook(algo, per_epoch, eval_episodes, scorers):
    """(``epoch_hook`` of a ``fit``, the dict it fills): the scorer pass after every epoch (d3rlpy's ``fit(eval_episodes=, scorers=)``)"""
    if (eval_episodes is None) != (scorers is None):
        raise ValueError('fit_mdp: eval_episodes and scorers go together')
    if scorers is None:
        return None, None
    from . import scorers as S
    scores = {name: [] for name in scorers}

    def hook(epoch):
        for name, value in S.run_scorers(algo, eval_episodes, scorers).items():
            scores[name].append(value)
    return (max(int(per_epoch), 1), hook), scores


class _ModelIO(object):
    """``save_model`` / ``load_model`` / ``fit_mdp`` shared by every learner of this module: what ``script/batchrl_train.py`` calls
    on a d3rlpy algo (``model.fit(dataset, n_epochs=...)`` then ``model.save_model(path)``, :127-132; ``model.load_model(path)``
    in the eval / ope stages, :140-142).  The file is this package's own (``numpy.savez``: every network's flat parameter vector,
    Adam moments and step count, the learned scalars, the update counter) - d3rlpy's torch ``state_dict`` pickles need d3rlpy."""

    def _io_nets(self):
        seen, out = set(), []
        for name, v in sorted(vars(self).items()):
            if hasattr(v, 'flat_params') and hasattr(v, 'set_flat_params') and id(v) not in seen:
                seen.add(id(v))
                out.append((name, v))
        return out

    def check_status(self):
        """Raise what a ``fit`` so far left pending (nothing here: the learners that keep a flag on the device override it)."""

    def save_model(self, fname):
        self.check_status()
        blob = {'__class__': np.array(type(self).__name__), 'total_step': np.array(self.total_step, dtype=np.int64)}
        for name, net in self._io_nets():
            blob['net.' + name] = net.flat_params().cpu().numpy()
            m, v, t = net.adam_state()
            blob['adam_m.' + name], blob['adam_v.' + name] = m.cpu().numpy(), v.cpu().numpy()
            blob['adam_t.' + name] = np.array(t, dtype=np.int64)
        for name in ('log_temp', 'log_alpha'):
            sp = getattr(self, name, None)
            if sp is not None:
                blob['scalar.' + name] = np.concatenate([sp.p.cpu().numpy(), sp.m.cpu().numpy(), sp.v.cpu().numpy(), [float(sp.t)]])
        rs = getattr(self, 'reward_scaler', None)
        if isinstance(rs, str):
            # a scaler given by name ('standard', as batchrl_trainer builds CQL-conti) has no statistics until fit_mdp fits it on the
            # dataset: nothing to save - a learner that never trained on scaled rewards is saved as one without a scaler
            rs = None
        if rs is not None:
            blob['reward_scaler'] = np.array([rs.mean, rs.std, rs.eps], dtype=np.float64)
        with open(fname, 'wb') as f:
            np.savez(f, **blob)

    def load_model(self, fname, legacy=True):
        with np.load(fname) as z:
            cls = str(z['__class__'])
            if cls != type(self).__name__:
                raise ValueError('%s holds a %s, this learner is a %s' % (fname, cls, type(self).__name__))
            self.total_step = int(z['total_step'])
            for name, net in self._io_nets():
                flat = z['net.' + name]
                if flat.size != net.n_params:
                    raise ValueError('%s: network %r has %d parameters in the file, %d here' % (fname, name, flat.size, net.n_params))
                dev = net.device
                net.set_flat_params(torch.from_numpy(np.ascontiguousarray(flat, dtype=np.float32)).to(dev))
                net.set_adam_state(torch.from_numpy(z['adam_m.' + name]).to(dev), torch.from_numpy(z['adam_v.' + name]).to(dev),
                                   int(z['adam_t.' + name]))
            for name in ('log_temp', 'log_alpha'):
                sp = getattr(self, name, None)
                if sp is not None:
                    a = z['scalar.' + name]
                    sp.p.fill_(float(a[0])); sp.m.fill_(float(a[1])); sp.v.fill_(float(a[2])); sp.t = int(a[3])
            # the reward scale the critics were trained on travels with them (d3rlpy keeps it in params.json): a learner restored
            # onto a different scale would keep training / report predict_value in other units without any error
            if 'reward_scaler' in z.files:
                if not hasattr(self, 'reward_scaler'):
                    raise ValueError('%s carries a reward scaler, %s has none' % (fname, type(self).__name__))
                self.reward_scaler = StandardRewardScaler.from_stats(*[float(x) for x in z['reward_scaler']])
            elif getattr(self, 'reward_scaler', None) is not None and not isinstance(self.reward_scaler, str):
                # files written before the scaler travelled with the model (or by a learner whose named scaler was never fitted): the
                # learner keeps ITS scaler - loud, not fatal (legacy=False turns it back into an error)
                if not legacy:
                    raise ValueError('%s was saved without a reward scaler, this learner has one' % fname)
                import warnings
                warnings.warn('%s was saved without a reward scaler; keeping this learner\'s (mean %.6g, std %.6g) - make sure it is the '
                              'scale the file was trained on' % (fname, self.reward_scaler.mean, self.reward_scaler.std))

    def fit_mdp(self, data, n_epochs=1, discrete_action=None, eval_episodes=None, scorers=None, **kw):
        """``fit`` on MDPDataset-style arrays (the dict ``offline.generate_offline_dataset`` returns) for ``n_epochs`` passes over its
        transitions - d3rlpy's ``fit(dataset, n_epochs=...)``.  With ``eval_episodes`` (a ``scorers.EvalEpisodes``) and ``scorers``
        (``{name: callable}``, see ``scorers.run_scorers``) the scorers run after every epoch and the call returns
        ``(history, {name: [value per epoch]})``."""
        if discrete_action is None:
            discrete_action = isinstance(self, _Learner)
        tr = transitions_from_mdp(data['observations'], data['actions'], data['rewards'], data['terminals'], discrete_action=discrete_action)
        if getattr(self, 'reward_scaler', None) == 'standard':
            # d3rlpy: a scaler given by name is fitted on the dataset when fit() builds the algorithm
            self.reward_scaler = StandardRewardScaler(tr[2])
        per_epoch = tr[0].shape[0] // self.batch_size
        steps = int(n_epochs) * per_epoch
        hook, scores = _score_hook(self, per_epoch, eval_episodes, scorers)
        if hook is None:
            return self.fit(tr, steps, **kw)
        return self.fit(tr, steps, epoch_hook=hook, **kw), scores


class _Learner(_ModelIO):
    def __init__(self, config, obs_dim, batch_size, lr, seed, custom_encoder, device=None):
        self.config = config
        self.A = int(config['action_size'])
        self.D = int(obs_dim)
        self.batch_size = int(batch_size)
        self.lr = float(lr)
        self.seed = int(seed)
        self.custom = bool(custom_encoder)
        self.device = device
        self.total_step = 0

    def _net(self, seed, max_rows=None):
        kw = {}
        M = 0
        if self.custom:                                   # batchrl_trainer.py:35-41: mask_size = page_items + 1
            from .data import CatalogTables
            M = int(self.config['page_items']) + 1
            if 'location_mask' in self.config and 'special_items' in self.config:
                loc, special = self.config['location_mask'], self.config['special_items']
            else:
                tab = CatalogTables(self.config['iteminfo_file'], self.A, int(self.config.get('action_emb_size', 32)))
                loc, special = tab.location_mask, tab.special_items
            kw = dict(location_mask=loc, special_items=special)
        params = init_qnet_params(self.D, self.A, M, seed=seed)
        return D.DeviceQNet(self.D, self.A, params, mask_size=M, max_rows=max_rows or self.batch_size, device=self.device, **kw)

    def _apply(self, net):
        if rdist.collectives_active():
            g = net.flat_gradient()
            rdist.allreduce_mean_(g)                      # data parallel: the one collective of an update (per network)
            net.set_flat_gradient(g)
        net.adam_step(self.lr)

    def fit(self, transitions, n_steps, shuffle_seed=None, epoch_hook=None):
        """``n_steps`` minibatch updates over ``transitions`` (tuple of tensors from ``transitions_from_mdp``), epoch-wise
        random permutation like d3rlpy's ``fit``; returns the list of losses.  ``epoch_hook``: see ``_epoch_minibatches``."""
        columns = [t.to(self.nets[0].device) for t in transitions]
        seed = self.seed if shuffle_seed is None else shuffle_seed
        losses = [self.update(*batch) for batch in _epoch_minibatches(columns, self.batch_size, n_steps, seed, epoch_hook)]
        out = [float(x) for x in torch.stack(losses).cpu()]
        for net in self.nets:
            net.check_status()
        return out

    def close(self):
        for net in self.nets:
            net.close()


class DiscreteBC(_Learner):
    """d3rlpy.algos.DiscreteBC(batch_size=256, beta=0, encoder_factory=CustomVectorEncoderFactory(with_q=True))
    (batchrl_trainer.py:34-47)."""

    def __init__(self, config, obs_dim, batch_size=256, learning_rate=1e-3, beta=0.0, seed=0, device=None):
        super(DiscreteBC, self).__init__(config, obs_dim, batch_size, learning_rate, seed, True, device)
        self.beta = float(beta)
        self.imitator = self._net(seed)
        self.nets = [self.imitator]

    def update(self, obs, act, rew=None, nxt=None, ter=None):
        logits = self.imitator.forward(obs)
        loss2, d = self.imitator.imitation_loss(logits, act, self.beta)
        self.imitator.backward(obs, d)
        self._apply(self.imitator)
        self.total_step += 1
        return loss2[0] + self.beta * loss2[1] / self.A

    def predict(self, obs):
        return self.imitator.best_action(self.imitator.forward(obs))


class _QLearner(_Learner):
    def __init__(self, config, obs_dim, batch_size, lr, seed, custom, gamma, target_update_interval, device):
        super(_QLearner, self).__init__(config, obs_dim, batch_size, lr, seed, custom, device)
        self.gamma = float(gamma)
        self.target_update_interval = int(target_update_interval)
        self.q = self._net(seed)
        self.q_target = self._net(seed)
        self.q_target.copy_from(self.q)

    def predict_value(self, obs, actions):
        q = self.q.forward(obs)
        return q.gather(1, torch.as_tensor(actions, device=q.device).long().reshape(-1, 1))[:, 0]

    def _sync_target(self):
        self.total_step += 1
        if self.total_step % self.target_update_interval == 0:
            self.q_target.copy_from(self.q)


class DiscreteBCQ(_QLearner):
    """d3rlpy.algos.DiscreteBCQ(batch_size=256, encoder_factory=CustomVectorEncoderFactory(with_q=True))
    (batchrl_trainer.py:48-60)."""

    def __init__(self, config, obs_dim, batch_size=256, learning_rate=6.25e-5, gamma=0.99, action_flexibility=0.3, beta=0.5,
                 target_update_interval=8000, seed=0, device=None):
        super(DiscreteBCQ, self).__init__(config, obs_dim, batch_size, learning_rate, seed, True, gamma, target_update_interval, device)
        self.action_flexibility, self.beta = float(action_flexibility), float(beta)
        self.imitator = self._net(seed + 1)
        self.nets = [self.q, self.q_target, self.imitator]

    def update(self, obs, act, rew, nxt, ter):
        # the no-gradient forwards first: a handle keeps the activations of its LAST forward for the backward
        imit_next = self.imitator.forward(nxt)
        q_next = self.q.forward(nxt)
        q_next_t = self.q_target.forward(nxt)
        q_t = self.q.forward(obs)
        td2, dq, _ = self.q.dqn_loss(q_t, act, rew, ter, q_next, q_next_t, imitator_next=imit_next,
                                     action_flexibility=self.action_flexibility, gamma=self.gamma)
        self.q.backward(obs, dq)
        logits = self.imitator.forward(obs)
        im2, dl = self.imitator.imitation_loss(logits, act, self.beta)
        self.imitator.backward(obs, dl)
        self._apply(self.q)
        self._apply(self.imitator)
        self._sync_target()
        return td2[0] + im2[0] + self.beta * im2[1] / self.A

    def predict(self, obs):
        return self.q.best_action(self.q.forward(obs), self.imitator.forward(obs), self.action_flexibility)


class DiscreteCQL(_QLearner):
    """d3rlpy.algos.DiscreteCQL(batch_size=256) on d3rlpy's default encoder (batchrl_trainer.py:74-90)."""

    def __init__(self, config, obs_dim, batch_size=256, learning_rate=6.25e-5, gamma=0.99, alpha=1.0, target_update_interval=8000,
                 seed=0, device=None):
        super(DiscreteCQL, self).__init__(config, obs_dim, batch_size, learning_rate, seed, False, gamma, target_update_interval, device)
        self.alpha = float(alpha)
        self.nets = [self.q, self.q_target]

    def update(self, obs, act, rew, nxt, ter):
        q_next = self.q.forward(nxt)
        q_next_t = self.q_target.forward(nxt)
        q_t = self.q.forward(obs)
        l2, dq, _ = self.q.dqn_loss(q_t, act, rew, ter, q_next, q_next_t, gamma=self.gamma, cql_alpha=self.alpha)
        self.q.backward(obs, dq)
        self._apply(self.q)
        self._sync_target()
        return l2[0] + self.alpha * l2[1]

    def predict(self, obs):
        return self.q.best_action(self.q.forward(obs))


def init_amlp_params(obs_dim, act_dim, out_dim, hidden1=256, hidden2=256, seed=0, heads=1):
    """torch's default Linear initialiser (U(+-1/sqrt(fan_in)) for weight and bias), stored [in, out]; ``heads`` Linear layers
    of ``out_dim // heads`` outputs side by side (the mu / logstd pair of a ConditionalVAE or a SquashedNormalPolicy)."""
    rs = np.random.RandomState(seed)

    def linear(fan_in, fan_out):
        k = 1.0 / np.sqrt(fan_in)
        return (rs.uniform(-k, k, size=(fan_in, fan_out)).astype(np.float32), rs.uniform(-k, k, size=(fan_out,)).astype(np.float32))

    p = {}
    p['fc1_w'], p['fc1_b'] = linear(obs_dim + act_dim, hidden1)
    p['fc2_w'], p['fc2_b'] = linear(hidden1, hidden2)
    hw = [linear(hidden2, out_dim // heads) for _ in range(heads)]
    p['head_w'] = np.ascontiguousarray(np.concatenate([w for w, _ in hw], axis=1))
    p['head_b'] = np.ascontiguousarray(np.concatenate([b for _, b in hw]))
    return p


def init_ddpg_params(obs_dim, act_dim, out_dim, hidden1=400, hidden2=300, seed=0):
    """Keras Dense defaults, what RLlib's ddpg_tf_model builds its actor and critics from: ``glorot_uniform`` kernels
    (U(+-sqrt(6 / (fan_in + fan_out)))) and zero biases, stored [in, out] in ``DeviceAMLP``'s layout."""
    rs = np.random.RandomState(seed)

    def dense(fan_in, fan_out):
        k = np.sqrt(6.0 / (fan_in + fan_out))
        return rs.uniform(-k, k, size=(fan_in, fan_out)).astype(np.float32), np.zeros(fan_out, dtype=np.float32)

    p = {}
    p['fc1_w'], p['fc1_b'] = dense(obs_dim + act_dim, hidden1)
    p['fc2_w'], p['fc2_b'] = dense(hidden1, hidden2)
    p['head_w'], p['head_b'] = dense(hidden2, out_dim)
    return p


def _check_transitions(device, D, E, obs, act, rew, nxt, ter):
    """The one-call updates hand raw pointers to the library (which only knows the row count): everything DeviceAMLP._rows asserts
    on the per-phase path is asserted here - device, float32, shapes [B, D] / [B, E] / [B] - before any data_ptr() is taken."""
    B = obs.shape[0]
    for name, t, shape in (('observations', obs, (B, D)), ('actions', act, (B, E)), ('rewards', rew, (B,)),
                           ('next observations', nxt, (B, D)), ('terminals', ter, (B,))):
        assert isinstance(t, torch.Tensor) and t.is_cuda and (device.index is None or t.device.index == device.index), \
            '%s must be a tensor on %s' % (name, device)
        assert t.dtype == torch.float32, '%s must be float32 (got %s)' % (name, t.dtype)
        assert tuple(t.shape) == shape or (len(shape) == 1 and tuple(t.shape) == (B, 1)), \
            '%s must have shape %s (got %s)' % (name, shape, tuple(t.shape))
    return [t if t.is_contiguous() else t.contiguous() for t in (obs, act, rew, nxt, ter)]


def _allreduce_group(nets):
    """Data parallel: ONE mean all-reduce for the flat gradients of a group of networks that are stepped together."""
    if not rdist.collectives_active():
        return
    flats = [net.flat_gradient() for net in nets]
    g = torch.cat(flats)
    rdist.allreduce_mean_(g)
    o = 0
    for net, f in zip(nets, flats):
        net.set_flat_gradient(g[o:o + f.numel()].contiguous())
        o += f.numel()


class _ContinuousLearner(_ModelIO):
    """What the four continuous-action learners share: the size bookkeeping (``A`` is the action width ``fit``
    checks), the ``DeviceAMLP`` factory, the seeded generator and ``_randn``, the workspace cache of the one-call updates, the
    epoch-wise ``fit`` and the collection of its history.  A learner states its networks, its ``update`` and ``_LOSS_KEYS``."""

    def __init__(self, config, obs_dim, action_size, batch_size, predict_rows, seed, device):
        self.config = config
        self.D = int(obs_dim)
        self.A = int(action_size if action_size is not None else config['action_emb_size'])
        self.batch_size = int(batch_size)
        self.predict_rows = max(int(predict_rows), 1)
        self.seed = int(seed)
        self.total_step = 0
        self.device = device
        self.nets = []
        self.one_call = True             # update() as one library call on a single rank (False: the per-phase calls; tests compare the two)
        self._ws = {}                    # minibatch shape -> workspace of the learner's one-call update

    def _net(self, act_dim, out_dim, seed_off, max_rows, grad_rows, head_act='none', heads=1):
        params = init_amlp_params(self.D, act_dim, out_dim, seed=self.seed + seed_off, heads=heads)
        net = D_.DeviceAMLP(self.D, act_dim, out_dim, params, head_act=head_act, max_rows=max_rows, max_grad_rows=grad_rows, device=self.device)
        self.device = net.device
        self.nets.append(net)
        return net

    def _seed_generator(self):
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(self.seed + 1000003 * rdist.rank())

    def _randn(self, shape, given):
        """N(0, 1) of ``shape`` from the learner's generator, or the caller's tensor (tests) on the device"""
        if given is not None:
            return given.to(device=self.device, dtype=torch.float32).contiguous()
        return torch.randn(shape, generator=self._gen, device=self.device, dtype=torch.float32)

    def _workspace(self, key, size_fn, *dims):
        ws = self._ws.get(key)
        if ws is None:
            ws = self._ws[key] = torch.empty(int(size_fn(*dims)), dtype=torch.float32, device=self.device)
        return ws

    def _single_call(self):
        return self.one_call and not rdist.collectives_active()

    def _watch_losses(self, stacked):
        """(hook of ``_history``: the learners with an fp16x2 no-grad path keep a non-finite flag)"""

    def _history(self, hist, to_host):
        """dict of per-step loss lists from the per-update dicts (``to_host=False``: of stacked device tensors, nothing waits for the GPU)"""
        out = {}
        for k in self._LOSS_KEYS:
            vals = [h[k] for h in hist if k in h]
            if not vals:
                out[k] = []
                continue
            st = torch.stack(vals)
            self._watch_losses(st)
            out[k] = [float(x) for x in st.cpu()] if to_host else st
        return out

    def fit(self, transitions, n_steps, shuffle_seed=None, to_host=True, epoch_hook=None):
        """``n_steps`` updates over ``transitions`` (``transitions_from_mdp(..., discrete_action=False)``), epoch-wise random
        permutation like d3rlpy's ``fit``; returns dict of per-step loss lists (``to_host=False``: of stacked device tensors,
        nothing waits for the GPU).  ``epoch_hook``: see ``_epoch_minibatches``."""
        columns = [t.to(self.device) for t in transitions]
        batches = _epoch_minibatches(columns, self.batch_size, n_steps, self.seed if shuffle_seed is None else shuffle_seed, epoch_hook)
        act = columns[1]
        assert act.dim() == 2 and act.shape[1] == self.A and act.dtype == torch.float32, 'continuous actions [N, %d] needed' % self.A
        out = self._history([self.update(*batch) for batch in batches], to_host)
        if to_host:
            self.check_status()
        return out

    def close(self):
        for net in self.nets:
            net.close()


class _NonFiniteFlag(object):
    """For the learners with an fp16x2 no-grad path (BCQ, CQL): a non-finite loss poisons Adam for good (the fused fp16x2 forward
    turns a row whose hidden activation leaves the fp16 range into NaN).  The flag stays on the device; ``check_status`` reads it."""

    NONFINITE_MESSAGE = ("a training loss of this learner became non-finite; with nograd_precision='fp16x2' a hidden activation that "
                         "leaves the fp16 range does that - rebuild the learner with nograd_precision='fp32'")
    _nonfinite = None

    def _watch_losses(self, stacked):
        bad = ~torch.isfinite(stacked).all()
        self._nonfinite = bad if self._nonfinite is None else (self._nonfinite | bad)

    def check_status(self):
        """Raise if any loss of a ``fit`` so far was NaN / inf (one host read; ``fit(to_host=True)`` and ``save_model`` call it)."""
        flag = self._nonfinite
        if flag is not None and bool(flag.item()):
            self._nonfinite = None
            raise RuntimeError(self.NONFINITE_MESSAGE)


class BCQ(_NonFiniteFlag, _ContinuousLearner):
    """d3rlpy.algos.BCQ(batch_size=256) as 'BCQ-conti' instantiates it (script/batchrl_trainer.py:61-73): default
    ``VectorEncoderWithAction([256, 256])`` everywhere, Adam 1e-3 for actor / critic / imitator, gamma 0.99, tau 0.005, two
    critics, lam 0.75, 100 sampled actions, action_flexibility 0.05, latent_size 32, beta 0.5, update_actor_interval 1,
    rl_start_step 0 (d3rlpy 0.91 defaults; d3rlpy is absent here - PARITY UNPINNED).

    One ``update`` = d3rlpy's ``BCQ._update``: imitator step, critic step, actor step, soft target updates.  All network
    arithmetic runs through ``librl4rs_hip`` (``rl4rs_amlp_*`` and the cvae / residual / bcq_target / critic_mse entry points);
    torch supplies device memory and the Gaussian noise.  ``noise`` (tests): dict with ``eps`` [B, L], ``z_target`` [B * n, L]
    and ``z_actor`` [B, L] replacing the three ``torch.randn`` draws (the latter two before clamping to +-0.5).
    With ``torch.distributed`` initialised each rank trains on its own minibatches; the flat gradients of the networks of a
    phase are mean-all-reduced together before Adam (3 collectives per update; the phases depend on each other)."""

    def __init__(self, config, obs_dim, action_size=None, batch_size=256, actor_learning_rate=1e-3, critic_learning_rate=1e-3,
                 imitator_learning_rate=1e-3, gamma=0.99, tau=0.005, update_actor_interval=1, lam=0.75, n_action_samples=100,
                 action_flexibility=0.05, rl_start_step=0, latent_size=32, beta=0.5, predict_rows=512, seed=0, device=None,
                 nograd_precision='fp16x2'):
        super(BCQ, self).__init__(config, obs_dim, action_size, batch_size, predict_rows, seed, device)
        self.E = self.A                  # (d3rlpy's BCQ code calls the action width E)
        self.L = int(latent_size)
        self.n = int(n_action_samples)
        self.actor_lr, self.critic_lr, self.imitator_lr = float(actor_learning_rate), float(critic_learning_rate), float(imitator_learning_rate)
        self.gamma, self.tau, self.lam = float(gamma), float(tau), float(lam)
        self.update_actor_interval, self.rl_start_step = int(update_actor_interval), int(rl_start_step)
        self.scale, self.beta = float(action_flexibility), float(beta)
        # arithmetic of the forwards that never see a backward (the batch x n_action_samples rows of compute_target and of
        # _predict_best_action): 'fp16x2' = the scorer's split form, one fused launch per network (DeviceAMLP.forward), or 'fp32'
        assert nograd_precision in ('fp16x2', 'fp32')
        self.nograd = nograd_precision
        B, n, E, L = self.batch_size, self.n, self.E, self.L
        big = max(B, self.predict_rows) * n
        self.imit_enc = self._net(E, 2 * L, 0, B, B, heads=2)                 # ConditionalVAE._encoder_encoder + _mu | _logstd
        self.imit_dec = self._net(L, E, 1, big, B, head_act='tanh')           # ConditionalVAE._decoder_encoder + _fc, tanh
        self.policy = self._net(E, E, 2, big, B, head_act='tanh')             # DeterministicResidualPolicy
        self.policy_targ = self._net(E, E, 2, B * n, 0, head_act='tanh')
        self.q1 = self._net(E, 1, 3, big, B)                                  # ContinuousMeanQFunction x 2
        self.q2 = self._net(E, 1, 4, big, B)
        self.q1_targ = self._net(E, 1, 3, B * n, 0)
        self.q2_targ = self._net(E, 1, 4, B * n, 0)
        self.policy_targ.copy_from(self.policy)
        self.q1_targ.copy_from(self.q1)
        self.q2_targ.copy_from(self.q2)
        self._seed_generator()
        self._minus_inv_b = None
        self._imit_w = torch.tensor([1.0 / self.E, self.beta / self.L], dtype=torch.float32, device=self.device)

    def _latent(self, rows, noise, key):
        return self._randn((rows, self.L), None if noise is None else noise.get(key))

    def _clipped_latent(self, rows, noise, key):
        """clamp(randn, -0.5, 0.5) (BCQImpl: the decoder's latent is clipped when actions are sampled); a caller-supplied noise
        tensor is never modified"""
        own = noise is None or key not in noise
        z = self._latent(rows, noise, key)
        return z.clamp_(-0.5, 0.5) if own else z.clamp(-0.5, 0.5)

    def _sample_actions(self, obs, z, policy, rep, nograd=False):
        """imitator.decode(x, clip(z)) -> policy residual: [rows, E] actions for ``rep`` latents per observation."""
        sampled = self.imit_dec.forward(obs, z, rep=rep, nograd=nograd)
        t = policy.forward(obs, sampled, rep=rep, nograd=nograd)
        return sampled, t, D_.residual_action(sampled, t, self.scale)

    def _update_one_call(self, obs, act, rew, nxt, ter, noise):
        """The whole update as ONE library call (rl4rs_bcq_update: the same launches with the same arguments as ``update`` below
        issues one by one - after the fused kernels the update was bound by its ~55 Python -> C calls, not by the GPU)."""
        B, n, E, L = obs.shape[0], self.n, self.E, self.L
        lib = _lib.load()
        ws = self._workspace(B, lib.rl4rs_bcq_workspace_floats, B, n, E, L)
        total = (B + B * n + B) * L
        if noise is None:
            nz = torch.randn(total, generator=self._gen, device=self.device, dtype=torch.float32)      # eps | z_target | z_actor: one draw
        else:
            parts = [self._latent(B, noise, 'eps'), self._latent(B * n, noise, 'z_target'), self._latent(B, noise, 'z_actor')]
            nz = torch.cat([p.reshape(-1) for p in parts])                                           # (a copy: the caller's noise is never modified)
        metrics = torch.zeros(3, dtype=torch.float32, device=self.device)
        do_rl = self.total_step >= self.rl_start_step
        do_actor = do_rl and self.total_step % self.update_actor_interval == 0
        cont = _check_transitions(self.device, self.D, self.E, obs, act, rew, nxt, ter)
        st = _lib.BcqStep(*[net.h.value for net in (self.imit_enc, self.imit_dec, self.policy, self.policy_targ, self.q1, self.q2, self.q1_targ, self.q2_targ)],
                          B, n, E, L, self.beta, self.scale, self.lam, self.gamma, self.tau, self.imitator_lr, self.critic_lr, self.actor_lr,
                          1 if do_rl else 0, 1 if do_actor else 0, 1 if self.nograd == 'fp16x2' else 0, int(self.q1.H16_MIN_ROWS),
                          *[t.data_ptr() for t in cont], nz.data_ptr(), ws.data_ptr(), metrics.data_ptr())
        _lib.check(lib.rl4rs_bcq_update(C.byref(st), D_._stream()))
        self.total_step += 1
        out = {'imitator_loss': metrics[0]}
        if do_rl:
            out['critic_loss'] = metrics[1]
        if do_actor:
            out['actor_loss'] = metrics[2]
        return out

    def update(self, obs, act, rew, nxt, ter, noise=None):
        if self._single_call():
            return self._update_one_call(obs, act, rew, nxt, ter, noise)
        B, n = obs.shape[0], self.n
        metrics = {}
        # --- imitator (BCQImpl.update_imitator: ConditionalVAE.compute_error) ---
        eps = self._latent(B, noise, 'eps')
        enc_out = self.imit_enc.forward(obs, act)
        z = D_.cvae_sample(enc_out, eps)
        y = self.imit_dec.forward(obs, z)
        loss2, d_dec = D_.cvae_loss(y, act, enc_out)
        dz = self.imit_dec.backward(obs, z, d_dec, want_dact=True)
        d_enc = D_.cvae_encoder_grad(enc_out, eps, dz, self.beta)
        self.imit_enc.backward(obs, act, d_enc)
        _allreduce_group([self.imit_enc, self.imit_dec])
        D_.amlp_adam_multi([self.imit_enc, self.imit_dec], [self.imitator_lr] * 2)            # one optimiser launch per phase
        metrics['imitator_loss'] = torch.dot(loss2, self._imit_w)          # mse / E + beta * kl / L as ONE launch
        if self.total_step >= self.rl_start_step:
            # --- critic (DDPGBaseImpl.update_critic with BCQImpl.compute_target) ---
            zt = self._clipped_latent(B * n, noise, 'z_target')
            _, _, a_next = self._sample_actions(nxt, zt, self.policy_targ, n, nograd=self.nograd)
            q1n = self.q1_targ.forward(nxt, a_next, rep=n, nograd=self.nograd)
            q2n = self.q2_targ.forward(nxt, a_next, rep=n, nograd=self.nograd)
            yq, _ = D_.bcq_target(q1n, q2n, n, self.lam, rew, ter, self.gamma)
            q1v, q2v = D_.amlp_forward_multi([self.q1, self.q2], obs, act)              # the twin critics as one launch each way
            closs2, dq1, dq2 = D_.critic_mse(q1v, q2v, yq)
            D_.amlp_backward_multi([self.q1, self.q2], obs, act, [dq1, dq2])
            _allreduce_group([self.q1, self.q2])
            D_.amlp_adam_multi([self.q1, self.q2], [self.critic_lr] * 2)
            metrics['critic_loss'] = closs2.sum()
            if self.total_step % self.update_actor_interval == 0:
                # --- actor (BCQImpl.compute_actor_loss: -Q_1(s, pi(s, decode(s, z))).mean()) ---
                za = self._clipped_latent(B, noise, 'z_actor')
                sampled, t, a_pi = self._sample_actions(obs, za, self.policy, 1)
                qv = self.q1.forward(obs, a_pi)
                if self._minus_inv_b is None or self._minus_inv_b.numel() != B:
                    self._minus_inv_b = torch.full((B, 1), -1.0 / B, dtype=torch.float32, device=self.device)
                da = self.q1.backward(obs, a_pi, self._minus_inv_b, want_dact=True, want_param_grad=False)
                d_pre = D_.residual_grad(sampled, t, self.scale, da)
                self.policy.backward(obs, sampled, d_pre)
                _allreduce_group([self.policy])
                # Adam of the actor + the three soft target updates (the critics were stepped in their own phase): one launch
                D_.amlp_adam_multi([self.policy, self.q1, self.q2], [self.actor_lr, 0.0, 0.0], targets=[self.policy_targ, self.q1_targ, self.q2_targ],
                                   tau=self.tau, step=[True, False, False])
                metrics['actor_loss'] = torch.dot(qv.view(-1), self._minus_inv_b.view(-1))       # -mean(q) as ONE launch
        self.total_step += 1
        return metrics

    _LOSS_KEYS = ('imitator_loss', 'critic_loss', 'actor_loss')

    def predict(self, obs, noise=None):
        """BCQImpl._predict_best_action: 100 sampled actions per observation, the one the FIRST critic values highest.
        obs [B, D] (device tensor or array) -> actions [B, E] on the device: the embedding the env's K-NN resolves."""
        obs = D_._dev_tensor(obs, torch.float32, self.device)
        out = torch.empty((obs.shape[0], self.E), dtype=torch.float32, device=self.device)
        n = self.n
        for lo in range(0, obs.shape[0], self.predict_rows):
            x = obs[lo:lo + self.predict_rows].contiguous()
            b = x.shape[0]
            if noise is not None:
                z = noise[lo * n:(lo + b) * n].to(device=self.device, dtype=torch.float32)
            else:
                z = torch.randn((b * n, self.L), generator=self._gen, device=self.device, dtype=torch.float32)
            _, _, a = self._sample_actions(x, z.clamp(-0.5, 0.5).contiguous(), self.policy, n, nograd=self.nograd)
            q = self.q1.forward(x, a, rep=n, nograd=self.nograd)
            _, best = D_.bcq_target(q, None, n, 0.0, want_best=True)
            out[lo:lo + b] = D_.pick_rows(a, best, n)
        return out

    def predict_value(self, obs, actions):
        """AlgoBase.predict_value: the mean of the critics' values of (obs, action)."""
        obs = D_._dev_tensor(obs, torch.float32, self.device)
        actions = D_._dev_tensor(actions, torch.float32, self.device)
        out = torch.empty(obs.shape[0], dtype=torch.float32, device=self.device)
        rows = max(self.batch_size, self.predict_rows) * self.n
        for lo in range(0, obs.shape[0], rows):
            x, a = obs[lo:lo + rows].contiguous(), actions[lo:lo + rows].contiguous()
            out[lo:lo + x.shape[0]] = 0.5 * (self.q1.forward(x, a, nograd=self.nograd)[:, 0] + self.q2.forward(x, a, nograd=self.nograd)[:, 0])
        return out


class StandardRewardScaler(object):
    """d3rlpy 0.91 ``reward_scaler='standard'``: (r - mean) / (std + 1e-3) with the statistics of the dataset's rewards."""

    def __init__(self, rewards, eps=1e-3):
        r = torch.as_tensor(rewards, dtype=torch.float64)
        self.mean, self.std, self.eps = float(r.mean()), float(r.std(unbiased=False)), float(eps)

    def transform(self, r):
        return ((r - self.mean) / (self.std + self.eps)).to(torch.float32)

    def reverse_transform(self, q):
        """d3rlpy ``StandardRewardScaler.reverse_transform``: q * (std + eps) + mean (policy_model.predict_q, policy_model.py:55-61)"""
        return q * (self.std + self.eps) + self.mean

    @classmethod
    def from_stats(cls, mean, std, eps=1e-3):
        s = cls.__new__(cls)
        s.mean, s.std, s.eps = float(mean), float(std), float(eps)
        return s


class _ScalarParam(object):
    """One learned scalar (SAC's log-temperature, CQL's log-alpha) with torch-style Adam, kept on the device: a handful of
    one-element tensor ops per update (plumbing; no network arithmetic)."""

    def __init__(self, value, device):
        self.state = torch.zeros(4, dtype=torch.float32, device=device)         # {value, Adam m, Adam v, pad}: what rl4rs_cql_update steps in place
        self.p, self.m, self.v = self.state[0:1], self.state[1:2], self.state[2:3]
        self.p.fill_(float(value))
        self.t = 0

    def adam_step(self, grad, lr, beta1=0.9, beta2=0.999, eps=1e-8):
        if rdist.collectives_active():
            grad = rdist.allreduce_mean_(grad.clone())
        self.t += 1
        self.m.mul_(beta1).add_(grad, alpha=1.0 - beta1)
        self.v.mul_(beta2).addcmul_(grad, grad, value=1.0 - beta2)
        denom = (self.v / (1.0 - beta2 ** self.t)).sqrt_().add_(eps)
        self.p.addcdiv_(self.m, denom, value=-lr / (1.0 - beta1 ** self.t))


class _SAC(_ContinuousLearner):
    """The SAC half of CQL, MOPO and COMBO: the squashed-Gaussian ``policy``, the twin critics and their targets,
    ``log_temp``, the reward scaler, and the steps every one of them composes its ``update`` from.  A learner states the rows its
    critics see (``_critic_rows``) and the order of the steps; each step issues the same library calls wherever it is used."""

    def __init__(self, config, obs_dim, action_size, batch_size, actor_lr, critic_lr, temp_lr, gamma, tau, initial_temperature, reward_scaler,
                 predict_rows, seed, device):
        super(_SAC, self).__init__(config, obs_dim, action_size, batch_size, predict_rows, seed, device)
        self.actor_lr, self.critic_lr, self.temp_lr = float(actor_lr), float(critic_lr), float(temp_lr)
        self.gamma, self.tau = float(gamma), float(tau)
        self.reward_scaler = reward_scaler
        B, A = self.batch_size, self.A
        rows, grad_rows = self._critic_rows()
        self.policy = self._net(0, 2 * A, 0, max(B, self.predict_rows), B, heads=2)        # SquashedNormalPolicy: encoder + _mu | _logstd
        self.q1 = self._net(A, 1, 1, rows, grad_rows)
        self.q2 = self._net(A, 1, 2, rows, grad_rows)
        self.q1_targ = self._net(A, 1, 1, B, 0)
        self.q2_targ = self._net(A, 1, 2, B, 0)
        self.q1_targ.copy_from(self.q1)
        self.q2_targ.copy_from(self.q2)
        self.log_temp = _ScalarParam(np.log(initial_temperature), self.device)
        self._seed_generator()

    def _critic_rows(self):
        """(the most rows a critic sees in one forward, in one backward)"""
        return self.batch_size, self.batch_size

    def _scaled(self, rew):
        if self.reward_scaler is None:
            return rew
        if isinstance(self.reward_scaler, str):
            raise ValueError("reward_scaler=%r is fitted by fit_mdp(dataset); pass StandardRewardScaler(rewards) to use update / fit "
                             "directly" % self.reward_scaler)
        return self.reward_scaler.transform(rew)

    def _normal_part(self, rows, given):
        """[rows, A] of N(0, 1) for a one-call update: the caller's tensor (tests), else drawn"""
        assert given is None or given.numel() == rows * self.A, 'noise of %d values where %d x %d are needed' % (given.numel(), rows, self.A)
        return self._randn((rows, self.A), given)

    def _uniform_part(self, shape, given):
        if given is None:
            return torch.empty(shape, dtype=torch.float32, device=self.device).uniform_(-1.0, 1.0, generator=self._gen)
        assert given.numel() == int(np.prod(shape)), 'uniform noise of %d values where %s are needed' % (given.numel(), shape)
        return given.to(device=self.device, dtype=torch.float32).reshape(shape).contiguous()

    def _temp_step(self, head, eps):
        """SACImpl.update_temp: -(exp(log_temp) * (logp - A)).mean() and its Adam step on log_temp; returns the loss"""
        _, logp = D_.squashed_sample(head, eps)
        targ = (logp - self.A).mean()
        temp = self.log_temp.p.exp()
        loss = -(temp * targ)[0]
        self.log_temp.adam_step(-(temp * targ), self.temp_lr)
        return loss

    def _deterministic_target(self, head_nxt, rew, nxt, ter, one_launch):
        """y = r + gamma (1 - ter) min_c Qtarg_c(s', tanh(mu(s'))).  ``one_launch``: the twin targets through ``amlp_forward_multi``
        (COMBO) or one forward each (CQL) - what each learner's per-phase path has always issued"""
        a_next, _ = D_.squashed_sample(head_nxt, None)
        if one_launch:
            q1n, q2n = D_.amlp_forward_multi([self.q1_targ, self.q2_targ], nxt, a_next)
        else:
            q1n, q2n = self.q1_targ.forward(nxt, a_next), self.q2_targ.forward(nxt, a_next)
        return D_.bcq_target(q1n, q2n, 1, 1.0, rew.reshape(-1), ter.reshape(-1), self.gamma)[0]

    def _sampled_rows(self, head_obs, head_nxt, given, acts, offs, first):
        """Columns ``first`` .. ``first + 3n`` of ``acts`` [R, k, A] and the first 2n of them of ``offs`` [R, k]: n samples of pi(. | s)
        and n of pi(. | s') with their log-probabilities, n uniform on [-1, 1]^A (CQLImpl._compute_policy_is_values /
        _compute_random_is_values).  ``given`` = (eps_t, eps_tp1, uniform), each a tensor or None (drawn).  -> the two as flat rows"""
        R, k, A = acts.shape
        n = self.n
        e_t, e_tp1, uni = given if given is not None else (None, None, None)
        flat_a, flat_o = acts.view(R * k, A), offs.view(R * k)
        D_.squashed_sample(head_obs, self._randn((R * n, A), e_t), rep=n, act_out=flat_a, logp_out=flat_o, out_rep=k, out_off=first)
        D_.squashed_sample(head_nxt, self._randn((R * n, A), e_tp1), rep=n, act_out=flat_a, logp_out=flat_o, out_rep=k, out_off=first + n)
        if uni is not None:
            acts[:, first + 2 * n:] = uni.to(device=self.device, dtype=torch.float32)
        else:
            acts[:, first + 2 * n:].uniform_(-1.0, 1.0, generator=self._gen)
        return flat_a, flat_o

    def _actor_step(self, obs, head_obs, eps):
        """SACImpl.compute_actor_loss, (exp(log_temp) * logp - min_c Q_c(s, a)).mean(): its gradient into the policy handle (all-reduced);
        returns the loss.  The policy's Adam is the learner's (CQL fuses it with the soft target update)."""
        B, twin = obs.shape[0], [self.q1, self.q2]
        a_pi, logp = D_.squashed_sample(head_obs, eps)
        q1p, q2p = D_.amlp_forward_multi(twin, obs, a_pi)
        qmin, dq1, dq2 = D_.twin_min(q1p, q2p, want_grad=True)
        g1, g2 = D_.amlp_backward_multi(twin, obs, a_pi, [dq1.view(B, 1), dq2.view(B, 1)], want_dact=True, want_param_grad=False)
        d_head = D_.sac_actor_grad(head_obs, eps, a_pi, g1.add_(g2), self.log_temp.p)
        self.policy.backward(obs, None, d_head)
        _allreduce_group([self.policy])
        return (self.log_temp.p.exp() * logp - qmin).mean()

    def sample_action(self, obs, eps=None):
        """a ~ pi(. | obs) for any number of rows"""
        out = torch.empty((obs.shape[0], self.A), dtype=torch.float32, device=self.device)
        rows = self.policy.max_rows
        for lo in range(0, obs.shape[0], rows):
            x = obs[lo:lo + rows].contiguous()
            e = self._randn((x.shape[0], self.A), None if eps is None else eps[lo:lo + rows])
            D_.squashed_sample(self.policy.forward(x), e, act_out=out[lo:lo + x.shape[0]])
        return out

    def predict(self, obs):
        """SquashedNormalPolicy.best_action: tanh(mu(s)) - the embedding the env's K-NN resolves."""
        obs = D_._dev_tensor(obs, torch.float32, self.device)
        out = torch.empty((obs.shape[0], self.A), dtype=torch.float32, device=self.device)
        rows = self.policy.max_rows
        for lo in range(0, obs.shape[0], rows):
            x = obs[lo:lo + rows].contiguous()
            D_.squashed_sample(self.policy.forward(x), None, act_out=out[lo:lo + x.shape[0]])
        return out

    def predict_value(self, obs, actions):
        """AlgoBase.predict_value: the mean of the critics' values of (obs, action)."""
        obs = D_._dev_tensor(obs, torch.float32, self.device)
        actions = D_._dev_tensor(actions, torch.float32, self.device)
        out = torch.empty(obs.shape[0], dtype=torch.float32, device=self.device)
        rows = self.q1.max_rows
        for lo in range(0, obs.shape[0], rows):
            x, a = obs[lo:lo + rows].contiguous(), actions[lo:lo + rows].contiguous()
            out[lo:lo + x.shape[0]] = 0.5 * (self.q1.forward(x, a)[:, 0] + self.q2.forward(x, a)[:, 0])
        return out


class CQL(_NonFiniteFlag, _SAC):
    """d3rlpy.algos.CQL (continuous) as 'CQL-conti' instantiates it (script/batchrl_trainer.py:91-107): default encoders,
    actor lr 1e-4, critic lr 3e-4, temperature / alpha lr 1e-4, tau 0.005, two critics, initial temperature 1, initial alpha 1,
    alpha threshold 10, conservative weight 5, 10 action samples, deterministic (non-soft) backup; the script sets gamma = 1 and
    ``reward_scaler='standard'`` (pass ``gamma=1.0`` and ``reward_scaler=StandardRewardScaler(dataset rewards)``).
    d3rlpy 0.91 defaults as published; PARITY UNPINNED.

    One ``update`` = d3rlpy's ``CQL._update``: temperature step, alpha step, critic step (TD on the min of the target critics at
    tanh(mu(s')) + the conservative term), actor step, soft critic-target update.  Network arithmetic through ``librl4rs_hip``
    (``rl4rs_amlp_*``, ``rl4rs_squashed_sample``, ``rl4rs_cql_critic_loss``, ``rl4rs_sac_actor_grad``, ``rl4rs_twin_min``); torch
    supplies device memory, the noise and the two learned scalars' Adam.  The 1 + 3n rows of an observation (dataset action | n
    samples of pi(s) | n of pi(s') | n uniform) go through each critic as ONE forward / backward with the observation side of
    the first layer computed once per observation (rep = 31).  ``noise`` (tests): dict with ``eps_temp`` [B, A], ``alpha`` and
    ``critic`` = (eps_t [B*n, A], eps_tp1 [B*n, A], uniform [B, n, A]), ``eps_actor`` [B, A]."""

    def __init__(self, config, obs_dim, action_size=None, batch_size=256, actor_learning_rate=1e-4, critic_learning_rate=3e-4,
                 temp_learning_rate=1e-4, alpha_learning_rate=1e-4, gamma=0.99, tau=0.005, initial_temperature=1.0, initial_alpha=1.0,
                 alpha_threshold=10.0, conservative_weight=5.0, n_action_samples=10, reward_scaler=None, predict_rows=4096, seed=0,
                 device=None, nograd_precision='fp16x2'):
        assert nograd_precision in ('fp16x2', 'fp32')
        self.nograd = nograd_precision               # the alpha step's critic forwards (never differentiated): see BCQ
        self.n = int(n_action_samples)
        self.m = 1 + 3 * self.n
        super(CQL, self).__init__(config, obs_dim, action_size, batch_size, actor_learning_rate, critic_learning_rate, temp_learning_rate, gamma,
                                  tau, initial_temperature, reward_scaler, predict_rows, seed, device)
        self.alpha_lr = float(alpha_learning_rate)
        self.alpha_threshold, self.conservative_weight = float(alpha_threshold), float(conservative_weight)
        B, A, m = self.batch_size, self.A, self.m
        self.log_alpha = _ScalarParam(np.log(initial_alpha), self.device)
        self._acts = torch.zeros((B, m, A), dtype=torch.float32, device=self.device)
        self._offs = torch.zeros((B, m), dtype=torch.float32, device=self.device)
        self._offs[:, 1 + 2 * self.n:] = float(A * np.log(0.5))                       # log of the uniform density on [-1, 1]^A

    def _critic_rows(self):
        return max(self.batch_size * self.m, self.predict_rows), self.batch_size * self.m

    def _conservative_rows(self, head_obs, head_nxt, act, given):
        """[B, m, A] actions and [B, m] importance offsets of the conservative term: column 0 the dataset action, then the 3n
        columns of ``_sampled_rows``"""
        B = act.shape[0]
        acts, offs = self._acts[:B], self._offs[:B]
        acts[:, 0] = act
        return self._sampled_rows(head_obs, head_nxt, given, acts, offs, 1)

    def _conservative_value(self, sums, B):
        """conservative_weight * (mean_c mean_b logsumexp - mean_c mean_b Q(s, a))"""
        return self.conservative_weight * ((sums[2] + sums[3]) - (sums[4] + sums[5])) / (2.0 * B)

    def _update_one_call(self, obs, act, rew, nxt, ter, noise):
        """The whole update as ONE library call (rl4rs_cql_update: the launches of ``update`` below, the two learned scalars' Adam on
        the device)."""
        B, n, A = obs.shape[0], self.n, self.A
        lib = _lib.load()
        ws = self._workspace(B, lib.rl4rs_cql_workspace_floats, B, n, A)
        if noise:
            # any subset of the keys, like the per-phase path's noise.get(...): what is not given is drawn from the generator
            a_t, a_tp1, a_u = noise.get('alpha') or (None, None, None)
            c_t, c_tp1, c_u = noise.get('critic') or (None, None, None)
            rows = ((noise.get('eps_temp'), B), (a_t, B * n), (a_tp1, B * n), (c_t, B * n), (c_tp1, B * n), (noise.get('eps_actor'), B))
            normal = torch.cat([self._normal_part(r, x).reshape(-1) for x, r in rows])
            uniform = torch.cat([self._uniform_part((B * n * A,), x) for x in (a_u, c_u)])
        else:
            normal = torch.randn((2 * B + 4 * B * n) * A, generator=self._gen, device=self.device, dtype=torch.float32)
            uniform = torch.empty(2 * B * n * A, dtype=torch.float32, device=self.device).uniform_(-1.0, 1.0, generator=self._gen)
        metrics = torch.zeros(4, dtype=torch.float32, device=self.device)
        cont = _check_transitions(self.device, self.D, self.A, obs, act, rew, nxt, ter)
        st = _lib.CqlStep(*[net.h.value for net in (self.policy, self.q1, self.q2, self.q1_targ, self.q2_targ)], B, n, A,
                          self.gamma, self.tau, self.actor_lr, self.critic_lr, self.temp_lr, self.alpha_lr, self.alpha_threshold, self.conservative_weight,
                          1 if self.nograd == 'fp16x2' else 0, int(self.q1.H16_MIN_ROWS), self.log_temp.t, self.log_alpha.t,
                          self.log_temp.state.data_ptr(), self.log_alpha.state.data_ptr(), *[t.data_ptr() for t in cont],
                          normal.data_ptr(), uniform.data_ptr(), ws.data_ptr(), metrics.data_ptr())
        _lib.check(lib.rl4rs_cql_update(C.byref(st), D_._stream()))
        out = {'critic_loss': metrics[0], 'actor_loss': metrics[1]}
        if self.temp_lr > 0:
            self.log_temp.t += 1
            out['temp_loss'] = metrics[2]
        if self.alpha_lr > 0:
            self.log_alpha.t += 1
            out['alpha_loss'] = metrics[3]
        self.total_step += 1
        return out

    def update(self, obs, act, rew, nxt, ter, noise=None):
        noise = noise or {}
        B, A, m = obs.shape[0], self.A, self.m
        rew = self._scaled(rew)
        if self._single_call():
            return self._update_one_call(obs, act, rew, nxt, ter, noise)
        metrics = {}
        # the policy does not change until the actor step: its heads on s' and s are computed once (s last: the handle keeps the
        # activations of s for the actor's backward)
        head_nxt = self.policy.forward(nxt)
        head_obs = self.policy.forward(obs)
        # --- temperature (SACImpl.update_temp), before the critic and on the un-stepped policy
        if self.temp_lr > 0:
            metrics['temp_loss'] = self._temp_step(head_obs, self._randn((B, A), noise.get('eps_temp')))
        # --- alpha (CQLImpl.update_alpha): -conservative loss, gradient wrt log_alpha
        if self.alpha_lr > 0:
            fa, fo = self._conservative_rows(head_obs, head_nxt, act, noise.get('alpha'))
            sums, _, _ = D_.cql_critic_loss(self.q1.forward(obs, fa, rep=m, nograd=self.nograd), self.q2.forward(obs, fa, rep=m, nograd=self.nograd), fo, m)
            gap = self._conservative_value(sums, B) - self.alpha_threshold
            ea = self.log_alpha.p.exp()
            metrics['alpha_loss'] = -(ea.clamp(0.0, 1e6) * gap)[0]
            self.log_alpha.adam_step(torch.where(ea <= 1e6, -(ea * gap), torch.zeros_like(ea)), self.alpha_lr)
        # --- critic (DDPGBaseImpl.update_critic with CQLImpl.compute_critic_loss / _compute_deterministic_target)
        yq = self._deterministic_target(head_nxt, rew, nxt, ter, one_launch=False)
        fa, fo = self._conservative_rows(head_obs, head_nxt, act, noise.get('critic'))
        clipped_alpha = self.log_alpha.p.exp().clamp(0.0, 1e6)
        aw = (clipped_alpha * self.conservative_weight).contiguous()
        q1v = self.q1.forward(obs, fa, rep=m)
        q2v = self.q2.forward(obs, fa, rep=m)
        sums, dq1, dq2 = D_.cql_critic_loss(q1v, q2v, fo, m, y=yq, alpha_w=aw)
        self.q1.backward(obs, fa, dq1, rep=m)
        self.q2.backward(obs, fa, dq2, rep=m)
        _allreduce_group([self.q1, self.q2])
        D_.amlp_adam_multi([self.q1, self.q2], [self.critic_lr] * 2)
        metrics['critic_loss'] = (sums[0] + sums[1]) / B + (clipped_alpha * (self._conservative_value(sums, B) - self.alpha_threshold))[0]
        # --- actor; its Adam and the soft critic-target update are one launch
        metrics['actor_loss'] = self._actor_step(obs, head_obs, self._randn((B, A), noise.get('eps_actor')))
        D_.amlp_adam_multi([self.policy, self.q1, self.q2], [self.actor_lr, 0.0, 0.0], targets=[None, self.q1_targ, self.q2_targ], tau=self.tau,
                           step=[True, False, False])
        self.total_step += 1
        return metrics

    _LOSS_KEYS = ('critic_loss', 'actor_loss', 'temp_loss', 'alpha_loss')


class GeneratedFIFO(object):
    """MOPO's buffer of model-generated transitions: (s, a, r, s', terminal) rows in tensors on one device, first in first out at
    ``maxlen`` rows.  Storage grows with what is actually generated (doubling, never past ``maxlen``); once full the oldest rows
    are overwritten in place."""

    def __init__(self, maxlen, device=None):
        self.maxlen = int(maxlen)
        assert self.maxlen >= 1
        self.device = device
        self.size, self.pos = 0, 0          # rows held; where the next row goes (== size until the buffer is full)
        self.cols = None

    def __len__(self):
        return self.size

    def _reserve(self, rows):
        cap = 0 if self.cols is None else self.cols[0].shape[0]
        if rows <= cap:
            return
        new_cap = min(self.maxlen, max(rows, 2 * cap))
        self.cols = [torch.cat([c, torch.empty((new_cap - cap,) + tuple(c.shape[1:]), dtype=c.dtype, device=c.device)]) for c in self.cols]

    def append(self, obs, act, rew, nxt, ter):
        rows = [t if t.dim() > 1 else t.reshape(-1) for t in (obs, act, rew, nxt, ter)]
        b = rows[0].shape[0]
        if b > self.maxlen:                  # only the newest maxlen rows can survive
            rows = [t[b - self.maxlen:] for t in rows]
            b = self.maxlen
        if self.cols is None:
            self.cols = [torch.empty((0,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device) for t in rows]
        self._reserve(min(self.maxlen, self.size + b))
        cap = self.cols[0].shape[0]
        first = min(b, cap - self.pos)
        for c, t in zip(self.cols, rows):
            c[self.pos:self.pos + first] = t[:first]
            if first < b:                    # wraps: cap == maxlen here
                c[:b - first] = t[first:]
        self.size = min(self.maxlen, self.size + b)
        self.pos = (self.pos + b) % self.maxlen if self.size == self.maxlen else self.pos + b

    def rows(self, idx):
        return [c[idx] for c in self.cols]

    def oldest_first(self):
        """Every held row in insertion order (tests)."""
        if self.size < self.maxlen:
            return [c[:self.size] for c in self.cols]
        return [torch.cat([c[self.pos:self.size], c[:self.pos]]) for c in self.cols]


def mixed_minibatch(real, fifo, batch_size, real_ratio, gen):
    """round(real_ratio * batch_size) rows of the real transitions and the rest from the generated ones, both drawn with replacement
    from ``gen`` (real rows first).  Without generated rows the whole minibatch is real.  -> ([obs, act, rew, nxt, ter], n_real)"""
    n_real = int(round(real_ratio * batch_size)) if len(fifo) else batch_size
    dev = real[0].device
    out = [[] for _ in range(5)]
    if n_real:
        idx = torch.randint(0, real[0].shape[0], (n_real,), generator=gen, device=dev)
        for o, t in zip(out, real):
            o.append(t[idx])
    if batch_size - n_real:
        idx = torch.randint(0, len(fifo), (batch_size - n_real,), generator=gen, device=dev)
        for o, t in zip(out, fifo.rows(idx)):
            o.append(t)
    return [torch.cat(o).contiguous() for o in out], n_real


def model_rollout(sample_action, dynamics, start_obs, horizon, lam, fifo, step0=0, given=None):
    """MOPO's ``generate_new_data`` from ``start_obs`` [N, D]: ``horizon`` times a = sample_action(s, h), (s', r, var) =
    dynamics.predict(s, a, with_variance=True) with r - lam * var as the reward, (s, a, r, s', 0) appended to ``fifo``, s <- s'.
    ``given`` (tests): dict of per-step lists ``indices`` / ``noise`` handed to ``dynamics.predict``."""
    s = start_obs
    for h in range(int(horizon)):
        a = sample_action(s, h)
        kw = {}
        if given is not None:
            kw = {'indices': given['indices'][h], 'noise': given['noise'][h]}
        nx, r, _ = dynamics.predict(s, a, with_variance=True, lam=lam, step=step0 + h, **kw)
        fifo.append(s, a, r.reshape(-1), nx, torch.zeros(s.shape[0], dtype=torch.float32, device=s.device))
        s = nx
    return s


class MOPO(_SAC):
    """d3rlpy.algos.MOPO as 'MOPO' instantiates it (script/batchrl_trainer.py:108-129; the script passes batch_size=256, gamma=1.0,
    update_actor_interval=2000): SAC on default ``[256, 256]`` encoders - actor / critic / temperature lr 3e-4, tau 0.005, two
    critics, initial temperature 1 - trained on minibatches of ``real_ratio`` real and 1 - ``real_ratio`` model-generated rows.
    Every ``rollout_interval`` updates ``rollout_batch_size`` real observations are rolled ``rollout_horizon`` steps through
    ``dynamics`` under the current policy with the reward r - ``lam`` * variance.  d3rlpy 0.91 defaults as published; PARITY UNPINNED.

    One ``update``: critic step on y = r + gamma (1 - terminal) (min_c Q_targ_c(s', a') - exp(log_temp) log pi(a' | s')), a' sampled;
    then on every ``update_actor_interval``-th update (counted from 0) the actor step through min(Q1, Q2), the temperature step
    (target entropy -A) and the soft target update.  Composed of the library's entry points (``rl4rs_amlp_*``,
    ``rl4rs_squashed_sample``, ``rl4rs_sac_target``, ``rl4rs_critic_mse``, ``rl4rs_twin_min``, ``rl4rs_sac_actor_grad``); no one-call
    form.  ``noise`` (tests): dict with ``eps_next``, ``eps_actor``, ``eps_temp``, each [B, A]."""

    def __init__(self, config, obs_dim, dynamics, action_size=None, batch_size=100, actor_learning_rate=3e-4, critic_learning_rate=3e-4,
                 temp_learning_rate=3e-4, gamma=0.99, tau=0.005, initial_temperature=1.0, update_actor_interval=1, rollout_interval=1000,
                 rollout_horizon=5, rollout_batch_size=50000, lam=1.0, real_ratio=0.05, generated_maxlen=50000 * 5 * 5,
                 reward_scaler=None, predict_rows=4096, seed=0, device=None):
        super(MOPO, self).__init__(config, obs_dim, action_size, batch_size, actor_learning_rate, critic_learning_rate, temp_learning_rate, gamma,
                                   tau, initial_temperature, reward_scaler, predict_rows, seed, device)
        self.dynamics = dynamics
        self.update_actor_interval = max(int(update_actor_interval), 1)
        self.rollout_interval, self.rollout_horizon = max(int(rollout_interval), 1), int(rollout_horizon)
        self.rollout_batch_size, self.lam, self.real_ratio = int(rollout_batch_size), float(lam), float(real_ratio)
        self.generated = GeneratedFIFO(generated_maxlen, self.device)

    def _rollout_due(self):
        return self.total_step % self.rollout_interval == 0

    def _update_minibatch(self, batch, n_real):
        return self.update(*batch)

    def soft_target(self, rew, nxt, ter, eps_next=None):
        """y [B] of the critic step"""
        B, A = nxt.shape[0], self.A
        a_next, logp = D_.squashed_sample(self.policy.forward(nxt), self._randn((B, A), eps_next))
        q1t, q2t = self.q1_targ.forward(nxt, a_next), self.q2_targ.forward(nxt, a_next)
        return D_.sac_target(q1t, q2t, logp, self.log_temp.p, rew.reshape(-1).contiguous(), ter.reshape(-1).contiguous(), self.gamma)

    def update(self, obs, act, rew, nxt, ter, noise=None):
        noise = noise or {}
        obs, act, rew, nxt, ter = _check_transitions(self.device, self.D, self.A, obs, act, self._scaled(rew), nxt, ter)
        metrics = {}
        # --- critic (SACImpl.compute_target / DDPGBaseImpl.update_critic)
        y = self.soft_target(rew, nxt, ter, noise.get('eps_next'))
        q1v, q2v = D_.amlp_forward_multi([self.q1, self.q2], obs, act)
        loss2, dq1, dq2 = D_.critic_mse(q1v, q2v, y)
        D_.amlp_backward_multi([self.q1, self.q2], obs, act, [dq1, dq2])
        _allreduce_group([self.q1, self.q2])
        D_.amlp_adam_multi([self.q1, self.q2], [self.critic_lr] * 2)
        metrics['critic_loss'] = loss2[0] + loss2[1]
        if self.total_step % self.update_actor_interval == 0:
            self._actor_phase(obs, self.policy.forward(obs), noise, metrics)
        self.total_step += 1
        return metrics

    def _actor_phase(self, obs, head_obs, noise, metrics):
        """the actor step and its Adam, the temperature step on the STEPPED policy (a fresh forward), the soft target update"""
        B, A = obs.shape[0], self.A
        metrics['actor_loss'] = self._actor_step(obs, head_obs, self._randn((B, A), noise.get('eps_actor')))
        D_.amlp_adam_multi([self.policy], [self.actor_lr])
        if self.temp_lr > 0:
            metrics['temp_loss'] = self._temp_step(self.policy.forward(obs), self._randn((B, A), noise.get('eps_temp')))
        D_.amlp_adam_multi([self.q1, self.q2], [0.0, 0.0], targets=[self.q1_targ, self.q2_targ], tau=self.tau, step=[False, False])

    def generate_new_data(self, real_obs, given=None):
        """One rollout of ``rollout_batch_size`` start observations drawn with replacement from ``real_obs`` into ``self.generated``.
        ``given`` (tests): dict with ``start`` (row indices), ``eps`` [H][N, A], ``indices`` [H][N], ``noise`` [H][members, N, D + 1]."""
        if given is not None:
            idx = given['start'].to(self.device)
        else:
            idx = torch.randint(0, real_obs.shape[0], (self.rollout_batch_size,), generator=self._gen, device=self.device)
        start = real_obs.to(self.device)[idx].contiguous()
        sample = (lambda s, h: self.sample_action(s, None if given is None else given['eps'][h]))
        return model_rollout(sample, self.dynamics, start, self.rollout_horizon, self.lam, self.generated,
                             step0=self.total_step * 64, given=given)

    def fit(self, transitions, n_steps, shuffle_seed=None, to_host=True, epoch_hook=None):
        """``n_steps`` updates on mixed minibatches; a rollout before every ``rollout_interval``-th update (the first included).
        ``epoch_hook`` = (steps per epoch, f): f(epoch) after the last update of an epoch."""
        real = [t.to(self.device) for t in transitions]
        assert real[1].dim() == 2 and real[1].shape[1] == self.A and real[1].dtype == torch.float32, 'continuous actions [N, %d] needed' % self.A
        hist = []
        for k in range(n_steps):
            if self._rollout_due():
                self.generate_new_data(real[0])
            batch, n_real = mixed_minibatch(real, self.generated, self.batch_size, self.real_ratio, self._gen)
            hist.append(self._update_minibatch(batch, n_real))
            if epoch_hook is not None and (k + 1) % epoch_hook[0] == 0:
                epoch_hook[1]((k + 1) // epoch_hook[0])
        return self._history(hist, to_host)

    _LOSS_KEYS = ('critic_loss', 'actor_loss', 'temp_loss')

    def fit_mdp(self, data, n_epochs=1, eval_episodes=None, scorers=None, **kw):
        tr = transitions_from_mdp(data['observations'], data['actions'], data['rewards'], data['terminals'], discrete_action=False)
        if self.reward_scaler == 'standard':
            self.reward_scaler = StandardRewardScaler(tr[2])
        per_epoch = max(tr[0].shape[0] // self.batch_size, 1)
        hook, scores = _score_hook(self, per_epoch, eval_episodes, scorers)
        if hook is None:
            return self.fit(tr, int(n_epochs) * per_epoch, **kw)
        return self.fit(tr, int(n_epochs) * per_epoch, epoch_hook=hook, **kw), scores


class COMBO(MOPO):
    """d3rlpy.algos.COMBO as 'COMBO' instantiates it (script/batchrl_trainer.py:130-151; the script passes batch_size=256, gamma=1.0,
    update_actor_interval=2000, reward_scaler='standard'): SAC on default ``[256, 256]`` encoders - actor lr 1e-4, critic lr 3e-4,
    temperature lr 1e-4, tau 0.005, two critics, initial temperature 1 - whose critic loss is TD + a conservative term, trained on
    minibatches of ``n_real`` real rows followed by F = B - n_real rows generated by MOPO's rollouts with the reward NOT penalised:

        TD            = sum_c mean_{b < B} (Q_c(s_b, a_b) - y_b)^2,  y_b = r_b + gamma (1 - ter_b) min_c Qtarg_c(s'_b, tanh(mu(s'_b)))
        conservative  = w [ sum_c mean_{f generated} logsumexp_j (Q_c(s_f, a_fj) - off_fj) - sum_c mean_{b real} Q_c(s_b, a_b) ]

    with CQL's 3n sampled actions per generated row (n of pi(.|s_f), n of pi(.|s'_f), n uniform; offsets: the sample's log-prob, or
    A log 0.5) and no learned alpha (d3rlpy fixes it at 1 and never steps it).  After the critic step, on every
    ``update_actor_interval``-th update counted from 0: the SAC actor step, the temperature step on the STEPPED policy, the soft
    critic-target update (``MOPO.update``'s order).  d3rlpy 0.91 defaults as published; PARITY UNPINNED.

    The critic step is two passes through the twin critics joined by ``rl4rs_amlp_grad_stash`` (csrc/combo.hpp): pass T over the B
    rows (s, a), pass C over the F * 3n sample rows with the observation side of the first layer once per generated observation.
    ``update`` is one library call (``rl4rs_combo_update``) on a single rank, or the per-phase calls with ``_allreduce_group`` around
    each Adam when collectives are active or ``one_call`` is False.  ``noise`` (tests): dict with any of ``critic`` = (eps_t [F n, A],
    eps_tp1 [F n, A], uniform [F, n, A]), ``eps_actor`` [B, A], ``eps_temp`` [B, A]; the rest is drawn.

    Stated deviations and unpinned points: (a) d3rlpy splits the batch at int(B * real_ratio); here the split is the ``n_real`` the
    minibatch was built with (``mixed_minibatch``: round), so the two cannot disagree.  (b) Whether 0.91's COMBOImpl multiplies its
    conservative loss by ``conservative_weight`` cannot be verified here; it is applied (at the default 1.0 both readings
    coincide).  (c) As for MOPO (points 2, 4, 6): both parts of a minibatch are drawn with replacement, the
    learner's own observation scaler is not applied, the noise comes from this library's sources.  A half without rows (d3rlpy: NaN)
    is an error here."""

    def __init__(self, config, obs_dim, dynamics, action_size=None, batch_size=256, actor_learning_rate=1e-4, critic_learning_rate=3e-4,
                 temp_learning_rate=1e-4, gamma=0.99, tau=0.005, initial_temperature=1.0, update_actor_interval=1, conservative_weight=1.0,
                 n_action_samples=10, soft_q_backup=False, rollout_interval=1000, rollout_horizon=5, rollout_batch_size=50000, lam=0.0,
                 real_ratio=0.5, generated_maxlen=50000 * 5 * 5, reward_scaler=None, discrete_action=False, predict_rows=4096, seed=0,
                 device=None):
        # (the refusals come first: none of them needs a device)
        if soft_q_backup:
            raise NotImplementedError('COMBO(soft_q_backup=True) is not built: the backup is the deterministic one, min_c Qtarg_c(s\', tanh(mu(s\')))')
        if float(lam) != 0.0:
            raise ValueError('COMBO does not penalise the generated reward: lam must be 0 (got %r); MOPO is the learner with r - lam * variance' % (lam,))
        if discrete_action:
            raise ValueError('COMBO here learns continuous actions only (the reference reaches it with support_conti_env); discrete_action=True is not built')
        self.n = int(n_action_samples)
        self.conservative_weight = float(conservative_weight)
        n_real = int(round(float(real_ratio) * int(batch_size)))
        if self.n < 1 or not 0 < n_real < int(batch_size):
            raise ValueError('COMBO needs n_action_samples >= 1 and both real and generated rows in a minibatch: n_action_samples=%d, '
                             'round(real_ratio * batch_size) = %d of %d' % (self.n, n_real, int(batch_size)))
        MOPO.__init__(self, config, obs_dim, dynamics, action_size=action_size, batch_size=batch_size, actor_learning_rate=actor_learning_rate,
                      critic_learning_rate=critic_learning_rate, temp_learning_rate=temp_learning_rate, gamma=gamma, tau=tau,
                      initial_temperature=initial_temperature, update_actor_interval=update_actor_interval, rollout_interval=rollout_interval,
                      rollout_horizon=rollout_horizon, rollout_batch_size=rollout_batch_size, lam=0.0, real_ratio=real_ratio,
                      generated_maxlen=generated_maxlen, reward_scaler=reward_scaler, predict_rows=predict_rows, seed=seed, device=device)
        self.lam = None                  # model_rollout: dynamics.predict's reward as it is, no variance penalty
        self._w = torch.full((1,), self.conservative_weight, dtype=torch.float32, device=self.device)
        self._log_uniform = float(self.A * np.log(0.5))          # log of the uniform density on [-1, 1]^A
        self._stash_n = (self.q1.n_params + 3) // 4 * 4
        self._stash = torch.empty(2 * self._stash_n, dtype=torch.float32, device=self.device)

    def _critic_rows(self):
        # pass C: at most batch_size - 1 generated rows with 3n samples each
        rows = max(self.batch_size, (self.batch_size - 1) * 3 * self.n)
        return rows, rows

    def _rollout_due(self):
        # (a learner restored in the middle of an interval has no generated rows yet: the generated half is never empty in fit)
        return MOPO._rollout_due(self) or len(self.generated) == 0

    def _update_minibatch(self, batch, n_real):
        return self.update(*batch, n_real=n_real)

    def _noise(self, noise, B, F):
        """(eps_t, eps_tp1, uniform) of the critic step: what ``noise['critic']`` gives, the rest drawn"""
        e_t, e_tp1, uni = noise.get('critic') or (None, None, None)
        return self._normal_part(F * self.n, e_t), self._normal_part(F * self.n, e_tp1), self._uniform_part((F, self.n, self.A), uni)

    def _update_one_call(self, obs, act, rew, nxt, ter, n_real, noise, do_actor):
        B, n, A, F = obs.shape[0], self.n, self.A, obs.shape[0] - n_real
        lib = _lib.load()
        ws = self._workspace((B, n_real), lib.rl4rs_combo_workspace_floats, B, n_real, n, A)
        if noise:
            e_t, e_tp1, uniform = self._noise(noise, B, F)
            parts = [e_t.reshape(-1), e_tp1.reshape(-1)]
            if do_actor:
                parts += [self._normal_part(B, noise.get(key)).reshape(-1) for key in ('eps_actor', 'eps_temp')]
            normal = torch.cat(parts)
        else:
            normal = torch.randn((2 * F * n + (2 * B if do_actor else 0)) * A, generator=self._gen, device=self.device, dtype=torch.float32)
            uniform = torch.empty(F * n * A, dtype=torch.float32, device=self.device).uniform_(-1.0, 1.0, generator=self._gen)
        metrics = torch.zeros(4, dtype=torch.float32, device=self.device)
        st = _lib.ComboStep(*[net.h.value for net in (self.policy, self.q1, self.q2, self.q1_targ, self.q2_targ)], B, n_real, n, A,
                            self.gamma, self.tau, self.actor_lr, self.critic_lr, self.temp_lr, self.conservative_weight,
                            1 if do_actor else 0, 0, self.log_temp.t, self.log_temp.state.data_ptr(), *[t.data_ptr() for t in (obs, act, rew, nxt, ter)],
                            normal.data_ptr(), uniform.data_ptr(), self._stash.data_ptr(), ws.data_ptr(), metrics.data_ptr())
        _lib.check(lib.rl4rs_combo_update(C.byref(st), D_._stream()))
        out = {'critic_loss': metrics[0], 'conservative_loss': metrics[3]}
        if do_actor:
            out['actor_loss'] = metrics[1]
            if self.temp_lr > 0:
                self.log_temp.t += 1
                out['temp_loss'] = metrics[2]
        self.total_step += 1
        return out

    def update(self, obs, act, rew, nxt, ter, n_real, noise=None):
        noise = noise or {}
        B, A, n = obs.shape[0], self.A, self.n
        n_real = int(n_real)
        F, k = B - n_real, 3 * n
        if not 0 < n_real < B:
            raise ValueError('COMBO.update: n_real=%d of %d rows: the data term needs real rows and the logsumexp term generated ones' % (n_real, B))
        if max(B, F * k) > self.q1.max_rows:
            raise ValueError('COMBO.update: a minibatch of %d rows (%d generated) where the learner was built for batch_size=%d' % (B, F, self.batch_size))
        obs, act, rew, nxt, ter = _check_transitions(self.device, self.D, self.A, obs, act, self._scaled(rew), nxt, ter)
        do_actor = self.total_step % self.update_actor_interval == 0
        if self._single_call():
            return self._update_one_call(obs, act, rew, nxt, ter, n_real, noise, do_actor)
        metrics = {}
        twin = [self.q1, self.q2]
        # the policy does not change until the actor step: its heads on s' and s are computed once (s last: the handle keeps the
        # activations of s for the actor's backward); the generated rows' heads are rows n_real .. of these
        head_nxt = self.policy.forward(nxt)
        head_obs = self.policy.forward(obs)
        yq = self._deterministic_target(head_nxt, rew, nxt, ter, one_launch=True)
        # --- the F * 3n rows of pass C: [pi(s_f) | pi(s'_f) | uniform] and their importance offsets
        given = self._noise(noise, B, F)
        acts = torch.empty((F, k, A), dtype=torch.float32, device=self.device)
        offs = torch.empty((F, k), dtype=torch.float32, device=self.device)
        flat_a, flat_o = self._sampled_rows(head_obs[n_real:], head_nxt[n_real:], given, acts, offs, 0)
        offs[:, 2 * n:] = self._log_uniform
        # --- critic: forward T, backward T, stash, forward C, backward C, add (a backward WRITES the handle's gradient)
        rows = torch.empty(4 * B + 2 * F, dtype=torch.float32, device=self.device)
        stash = [self._stash[:self._stash_n], self._stash[self._stash_n:]]
        q1t, q2t = D_.amlp_forward_multi(twin, obs, act)
        dq1t, dq2t = D_.combo_critic_loss(B, n_real, k, self._w, rows, t=(q1t, q2t, yq))
        D_.amlp_backward_multi(twin, obs, act, [dq1t, dq2t])
        D_.amlp_grad_stash(twin, stash)
        obs_f = obs[n_real:]
        q1c, q2c = self.q1.forward(obs_f, flat_a, rep=k), self.q2.forward(obs_f, flat_a, rep=k)
        sums, dq1c, dq2c = D_.combo_critic_loss(B, n_real, k, self._w, rows, c=(q1c, q2c, flat_o))
        self.q1.backward(obs_f, flat_a, dq1c, rep=k)
        self.q2.backward(obs_f, flat_a, dq2c, rep=k)
        D_.amlp_grad_stash(twin, stash, add=True)
        _allreduce_group(twin)
        D_.amlp_adam_multi(twin, [self.critic_lr] * 2)
        self.last_sums, self.last_y = sums, yq
        s64 = sums.double()              # (combined in double and rounded once, as k_combo_metrics does)
        cons = self.conservative_weight * ((s64[2] + s64[3]) / F - (s64[4] + s64[5]) / n_real)
        metrics['conservative_loss'] = cons.float()
        metrics['critic_loss'] = ((s64[0] + s64[1]) / B + cons).float()
        if do_actor:
            self._actor_phase(obs, head_obs, noise, metrics)
        self.total_step += 1
        return metrics

    def critic_step_outputs(self, B, n_real):
        """(y [B], sums6) of the LAST update's critic step (tests; the one-call path leaves them in its workspace)"""
        if not self._single_call():
            return self.last_y, self.last_sums
        lib, ws = _lib.load(), self._ws[(B, n_real)]
        y0, s0 = [int(lib.rl4rs_combo_workspace_offset(B, n_real, self.n, self.A, what)) for what in (0, 1)]
        return ws[y0:y0 + B], ws[s0:s0 + 6]

    _LOSS_KEYS = ('critic_loss', 'conservative_loss', 'actor_loss', 'temp_loss')
