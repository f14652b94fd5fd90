"""On-device policy training loops over the GPU env (A2C / PPO with the reference's RLlib hyper-parameters,
script/modelfree_train.py:179-304: gamma = 1, GAE lambda = 1, lr 1e-4, vf_loss_coeff 0.5; A2C entropy 0.01 and
grad_clip 10; PPO clip 0.3, kl_coeff 0.2 adapted towards kl_target 0.01, vf_clip 500, one SGD pass over minibatches of 256;
train_batch_size = min(B * T, 1024) timesteps per train call, :409).  The same ``Trainer`` runs that driver's PG (:306-343: lr 4e-4,
the plain policy gradient on the return-to-go) and IMPALA (:345-390: V-trace, rl4rs_policy_vtrace_loss_grad, with an actor copy of
the policy that trails the learner by a fixed number of updates).

Rollout, policy forward/backward and Adam run through librl4rs_hip.so; torch is used for buffers, the reversed
cumulative sum of rewards and (data-parallel) the RCCL all-reduce of the flat gradient buffer.

``ContiTrainer`` is the same loop on the continuous-action env (that driver's ``is_conti`` branches, :219-234,271-286,315-330,362-377):
the Gaussian actor-critic of ``DeviceGaussPolicy`` (rl4rs_gpolicy_*) in place of the masked policy, a float action column, the env
stepped with the clipped draw.

``DQNTrainer`` is the value-based learner of the same driver (script/modelfree_train.py:106-133: RLlib DQN with double_q, n_step 1,
target_network_update_freq 200, buffer_size 100000 on the mask model): replay memory, TD loss, per-variable-clipped Adam and
the target copy all stay on the device (rl4rs_replay_*, rl4rs_policy_dqn_loss_grad).

``RawDQNTrainer`` is that driver's ``DQN_rawstate`` (script/modelfree_train.py:55-56,63-66): ``DQNTrainer``'s loop on the raw-state
model (``DeviceRawTrainer``), the observations kept in the ring as packed records (rl4rs_rawstate_pack, rl4rs_rawtrain_dqn_loss_grad).

``RainbowTrainer`` is that driver's RAINBOW (script/modelfree_train.py:50-53,146-178: RLlib DQN with num_atoms 8, dueling, double_q,
n_step 3 on RLlib's default model): the distributional network has a handle of its own (rl4rs_distq_*), the ring's n-step draw is
rl4rs_replay_sample_nstep, everything else is ``DQNTrainer``'s loop.

``TD3Trainer`` is the continuous actor-critic learner of that driver (script/modelfree_train.py:46-48,79-105: RLlib TD3 / DDPG on
support_conti_env): OU exploration, a replay ring of float actions and the whole update (rl4rs_td3_update) stay on the device.

All of them hang on one skeleton: ``_DeferredStats`` (a train call's statistics are copied asynchronously and
settled one call later), ``_OnPolicy`` (PPO's KL rule, for ``Trainer`` and ``RawStateTrainer`` only), ``_Evaluated`` (the evaluation
frame) and ``_ReplayTrainer`` (rollout, push, updates of DQN / Rainbow / TD3); a trainer states what differs.  ``_Checkpoint`` gives
``Trainer``, ``ContiTrainer``, ``DQNTrainer``, ``RainbowTrainer`` and ``TD3Trainer`` ``save(path)`` / ``restore(path)``.

Data parallelism: every rank owns its own env batch and sampling stream (``seed`` differs per rank) and a replica
of the policy that is IDENTICAL on all ranks: initialised from the shared ``init_seed``, rank 0's parameters / Adam state are
broadcast at construction, and every optimiser step applies the rank-mean gradient.  A2C: one all-reduce per iteration.
PPO: one per minibatch (synchronous SGD over the global minibatch of world_size x 256 samples): phase A + the gradient
tiles of the persistent pass run as ONE launch per minibatch (rl4rs_policy_ppo_minibatch_grad), then all-reduce, then Adam.
"""
import json
import math

import numpy as np
import torch

from . import dist as rdist
from . import device as D


def update_kl_coeff(kl_coeff, sampled_kl, kl_target):
    """RLlib's adaptive KL penalty (ray 1.5.1 ``KLCoeffMixin.update_kl``, configured by modelfree_train.py:189 kl_coeff 0.2 and
    :216 kl_target 0.01): x1.5 when the pass-mean KL exceeds 2 x target, x0.5 when it is below target / 2."""
    if sampled_kl > 2.0 * kl_target:
        return kl_coeff * 1.5
    if sampled_kl < 0.5 * kl_target:
        return kl_coeff * 0.5
    return kl_coeff


def rollouts_per_train_call(batch_size, max_steps, train_batch_size=None):
    """modelfree_train.py:403-409: rollout_fragment_length = max_steps, batch_mode complete_episodes, train_batch_size =
    min(B * T, 1024).  One vector-env rollout yields B * T timesteps, RLlib keeps sampling until it holds at least
    train_batch_size, so the reference's value always means exactly ONE rollout per train call; a larger explicit value asks
    for ceil(train_batch_size / (B * T)) rollouts."""
    per = int(batch_size) * int(max_steps)
    if train_batch_size is None:
        train_batch_size = min(per, 1024)
    return max(1, int(math.ceil(float(train_batch_size) / per)))


def _returns(rew, R, T, B):
    """gamma = 1, lambda = 1: reward-to-go within each rollout ([R, T, B] layout of the flat buffers)."""
    r = rew.view(R, T, B)
    return torch.flip(torch.cumsum(torch.flip(r, dims=[1]), dim=1), dims=[1]).reshape(-1).to(torch.float32)


DISCRETE_ENV_MESSAGE = "%s needs the zero-copy discrete-action env (config['return_tensors'] = True)"


def _require_env(cfg, message, conti=False, error=AssertionError):
    """Every trainer here runs the zero-copy env, discrete-action unless ``conti``; raises ``error(message)`` otherwise."""
    if not cfg.get('return_tensors', False) or bool(cfg.get('support_conti_env', False)) != conti:
        raise error(message)


def _obs_width(env):
    """The observation width the env reports (base.py:206-213): 256 for the DIEN / dnn / lstm simulators, 3072 for widedeep."""
    space = env.observation_space
    space = space.spaces['obs'] if hasattr(space, 'spaces') else space
    return int(space.shape[0])


def _default_minibatch(batch_size, max_steps, train_batch_size=None):
    """modelfree_train.py:409: train_batch_size = min(B * T, 1024) sampled rows per update unless one is given."""
    return int(train_batch_size) if train_batch_size is not None else min(batch_size * max_steps, 1024)


def sync_policy_replicas(policy, src=0):
    """Make every rank's parameters, Adam moments and step counter of ``policy`` those of rank ``src``."""
    p = policy.params()
    m, v, t = policy.adam_state()
    rdist.broadcast_(p, src)
    rdist.broadcast_(m, src)
    rdist.broadcast_(v, src)
    step = torch.tensor([t], dtype=torch.int64)
    if rdist.collectives_active():
        import torch.distributed as dist
        if dist.get_backend() != 'gloo':
            step = step.to(p.device)
        dist.broadcast(step, src=src)
    policy.set_params(p)
    policy.set_adam_state(m, v, int(step.item()))


class LazyStats(object):
    """Mapping over the statistics of one train call.  The numbers live on the device until somebody looks: the train call
    only enqueues an asynchronous copy into pinned memory + an event, so a loop that does not read its statistics never
    drains the GPU queue (the next rollout's host work - sampling, de-duplication, launches - overlaps the update pass).
    Any access (``stats['kl']``, ``dict(stats)``, ``repr``) waits for that one event."""

    def __init__(self, trainer, token):
        self._trainer, self._token, self._values = trainer, token, None

    def _resolve(self):
        if self._values is None:
            self._values = self._trainer._resolve(self._token)
        return self._values

    def __getitem__(self, k):
        return self._resolve()[k]

    def __iter__(self):
        return iter(self._resolve())

    def __len__(self):
        return len(self._resolve())

    def __contains__(self, k):
        return k in self._resolve()

    def keys(self):
        return self._resolve().keys()

    def items(self):
        return self._resolve().items()

    def values(self):
        return self._resolve().values()

    def get(self, k, default=None):
        return self._resolve().get(k, default)

    def __repr__(self):
        return repr(self._resolve())

    def __eq__(self, other):
        return dict(self._resolve()) == (dict(other._resolve()) if isinstance(other, LazyStats) else other)

    def __reduce__(self):                   # pickles / torch.save as the plain dict of numbers
        return (dict, (dict(self._resolve()),))


class _DeferredStats(object):
    """The skeleton every trainer hangs on: the statistics of a train call are copied asynchronously (``_submit``) and settled one
    call later (``_settle``, ``LazyStats``).  A trainer keeps ``_pending`` (a list) and ``iteration``, and fills ``_values``; one
    whose networks run a persistent pass is recognised by its ``policy`` handle's status words."""

    def _status_word(self, dev):
        """float64 [1]: non-zero when a persistent pass of this call timed out.  Reads the policy handle's status words; a trainer
        whose networks have none reports zero."""
        policy = getattr(self, 'policy', None)
        if hasattr(policy, 'status_words'):
            return policy.status_words()[1:2].to(torch.float64)
        return torch.zeros(1, dtype=torch.float64, device=dev)

    def _submit(self, mean_reward, stats, **extra):
        """Enqueue the device -> pinned copy of one train call's numbers [mean_reward, stats..., status word] and an event.
        ``extra``: host values of this call that ``_values`` wants back."""
        dev = stats.device
        status = self._status_word(dev)
        overflow = rdist.take_row_overflow(dev)
        if overflow is not None:
            status = status + 1000.0 * overflow.to(torch.float64)
        vec = torch.cat([mean_reward.reshape(1).to(torch.float64), stats.reshape(-1).to(torch.float64), status])
        pin = torch.empty(vec.shape, dtype=torch.float64, pin_memory=True)
        pin.copy_(vec, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        token = dict(pin=pin, ev=ev, values=None, iteration=self.iteration, **extra)
        self._pending.append(token)
        return LazyStats(self, token)

    def _settle(self):
        """Finish every outstanding train call in order: wait for its numbers, validate the pass, build its mapping."""
        while self._pending:
            tok = self._pending.pop(0)
            tok['ev'].synchronize()
            v = tok['pin'].numpy().copy()
            if v[-1] >= 1000.0:
                raise RuntimeError(rdist.ROW_OVERFLOW_MESSAGE)
            if v[-1] != 0.0:
                self.policy.check_status()                  # clears the flag and raises
                raise RuntimeError(D.DevicePolicy.PASS_TIMEOUT_MESSAGE)
            tok['values'] = dict(self._values(tok, float(v[0]), v[1:-1]), iteration=tok['iteration'])

    def _values(self, tok, mean_reward, s):
        """The trainer's hook: one settled call's token, mean episode reward and float64 statistics ``s`` -> its mapping."""
        raise NotImplementedError

    def _resolve(self, token):
        if token['values'] is None:
            self._settle()
        return token['values']


class _Evaluated(_DeferredStats):
    """A trainer with an evaluation pass (``_eval_batch``) and device handles of its own to close (``_owned``, ``device``)."""

    def close(self):
        try:
            self._settle()
        finally:
            for handle in self._owned:
                handle.close()

    def evaluate(self, episodes=None, seed=0):
        """Mean episode reward of ceil(episodes / B) evaluation batches (``_eval_batch``: no exploration) from the start of the record
        file with the env's record sampling seeded by ``seed``, so two calls on the same parameters give the same number.  Leaves
        the global numpy RNG as it found it; the env's record cursor restarts."""
        self._settle()
        n = 1 if episodes is None else max(1, int(math.ceil(float(episodes) / self.B)))
        state = np.random.get_state()
        try:
            np.random.seed(seed)
            total = torch.zeros((), dtype=torch.float64, device=self.device)
            for k in range(n):
                total += self._eval_batch(k)
        finally:
            np.random.set_state(state)
        return float(total.item()) / n


def _host_array(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _like(dst, arr):
    """``arr`` as what ``dst`` takes: a tensor on ``dst``'s device for a device handle / tensor, the array itself for a host stand-in."""
    dev = getattr(dst, 'device', None)
    return torch.from_numpy(np.ascontiguousarray(arr)).to(dev) if isinstance(dev, torch.device) else arr


class _Checkpoint(object):
    """``save`` / ``restore`` of the online trainers - what ``trainer.save(...)`` and the ``trainer.restore(...)`` at the head of the
    eval / eval_v2 / ope stages of script/modelfree_train.py (:434, :437-514) are to an RLlib trainer - in the style of
    ``offline_rl._ModelIO``.  The file is one ``numpy.savez``:

        class, algo_name, seed      the trainer's class name, ``algo_name`` ('' where a class has one algorithm), the constructor's seed
                                    (recorded, NOT restored: ranks differ in it)
        shapes                      json: handle name -> its shape tuple (``_HANDLE_DIMS`` and the parameter count)
        net.<name>.params           flat float32 parameters of every handle (``_ckpt_nets``)
        net.<name>.adam_m/_v/_t     Adam moments and step counter of the handles that are stepped (not of IMPALA's actor, not of a target)
        tensor.<name>               device tensors restored in place (``_ckpt_tensors``: DQN / Rainbow's target, TD3's OU state)
        host.<name>                 the host state that decides what the next call does (``_ckpt_host``)
        extra.<name>                what a trainer adds (``_ckpt_extra``: TD3's noise generator)

    A trainer states ``_ckpt_nets`` and ``_ckpt_host`` (and the optional hooks).  ``restore`` reads and checks the WHOLE file before it
    touches the trainer: a class, algo or shape mismatch raises ``ValueError`` naming both sides, a truncated file raises what numpy /
    zipfile raise, and in both cases nothing has changed.  Deviation from RLlib's checkpoint: none for the on-policy learners (their
    continuation is bit-identical); the replay ring is not saved (RLlib 1.5.1 does not save it either) - it is EMPTY after
    ``restore`` and refills from the next rollout, which ``train_iteration`` pushes before it samples."""

    _HANDLE_DIMS = ('obs_dim', 'hidden', 'action_size', 'act_dim', 'out_dim', 'hidden1', 'hidden2', 'num_atoms', 'trunk', 'stream_hidden',
                    'dueling', 'v_min', 'v_max', 'D', 'E', 'K', 'H1', 'H2', 'n_params')        # (D .. H2: DeviceAMLP's names)
    _ckpt_host = ()

    def _ckpt_nets(self):
        """[(name, handle, has Adam state)]"""
        raise NotImplementedError

    def _ckpt_tensors(self):
        return {}

    def _ckpt_extra(self):
        return {}

    def _ckpt_set_extra(self, extra):
        pass

    def _ckpt_after_restore(self):
        pass

    def _ckpt_meta(self):
        shapes = dict((name, [[d, getattr(net, d)] for d in self._HANDLE_DIMS if hasattr(net, d)]) for name, net, _ in self._ckpt_nets())
        return {'class': type(self).__name__, 'algo_name': str(getattr(self, 'algo_name', getattr(self, 'algo', '')) or ''),
                'shapes': json.dumps(shapes, sort_keys=True)}

    def save(self, path):
        """Write the checkpoint; every finished train call is in it (the deferred statistics are settled and the passes validated first)."""
        self._settle()
        for _, net, _ in self._ckpt_nets():
            if hasattr(net, 'check_status'):
                net.check_status()
        blob = dict((k, np.array(v)) for k, v in self._ckpt_meta().items())
        blob['seed'] = np.array(int(getattr(self, 'seed', 0)), dtype=np.int64)
        for name, net, adam in self._ckpt_nets():
            blob['net.%s.params' % name] = _host_array(net.params())
            if adam:
                m, v, t = net.adam_state()
                blob['net.%s.adam_m' % name], blob['net.%s.adam_v' % name] = _host_array(m), _host_array(v)
                blob['net.%s.adam_t' % name] = np.array(int(t), dtype=np.int64)
        for name, t in self._ckpt_tensors().items():
            blob['tensor.' + name] = _host_array(t)
        for name in self._ckpt_host:
            blob['host.' + name] = np.array(getattr(self, name))
        for name, v in self._ckpt_extra().items():
            blob['extra.' + name] = _host_array(v)
        with open(path, 'wb') as f:
            np.savez(f, **blob)

    def restore(self, path):
        """Load a checkpoint written by ``save`` of the same class, algorithm and shapes; under ``torch.distributed`` every rank's
        replica is then made rank 0's (``sync_replicas``)."""
        self._settle()
        with np.load(path) as z:
            blob = dict((k, z[k]) for k in z.files)                 # the whole file, before anything is touched
        here = self._ckpt_meta()
        for key, what in (('class', 'a %s'), ('algo_name', 'algo %r'), ('shapes', 'handles %s')):
            there = str(blob[key])
            if there != here[key]:
                raise ValueError('%s holds %s, this trainer is %s' % (path, what % there, what % here[key]))
        want = ['net.%s.%s' % (name, part) for name, _, adam in self._ckpt_nets()
                for part in (('params', 'adam_m', 'adam_v', 'adam_t') if adam else ('params',))]
        want += (['tensor.' + k for k in self._ckpt_tensors()] + ['host.' + k for k in self._ckpt_host] +
                 ['extra.' + k for k in self._ckpt_extra()])
        missing = [k for k in want if k not in blob]
        if missing:
            raise ValueError('%s lacks %s' % (path, ', '.join(missing)))
        for name, net, _ in self._ckpt_nets():
            n = _host_array(net.params()).size
            if blob['net.%s.params' % name].size != n:
                raise ValueError('%s: handle %r has %d parameters in the file, %d here' % (path, name, blob['net.%s.params' % name].size, n))
        for name, t in self._ckpt_tensors().items():
            if tuple(blob['tensor.' + name].shape) != tuple(t.shape):
                raise ValueError('%s: %r is %r in the file, %r here' % (path, name, tuple(blob['tensor.' + name].shape), tuple(t.shape)))
        for name, net, adam in self._ckpt_nets():
            net.set_params(_like(net, blob['net.%s.params' % name]))
            if adam:
                net.set_adam_state(_like(net, blob['net.%s.adam_m' % name]), _like(net, blob['net.%s.adam_v' % name]),
                                   int(blob['net.%s.adam_t' % name]))
        for name, t in self._ckpt_tensors().items():
            if isinstance(t, torch.Tensor):
                t.copy_(torch.from_numpy(blob['tensor.' + name]))
            else:
                t[...] = blob['tensor.' + name]
        for name in self._ckpt_host:
            setattr(self, name, type(getattr(self, name))(blob['host.' + name].item()))
        self._ckpt_set_extra(dict((k, blob['extra.' + k]) for k in self._ckpt_extra()))
        self._ckpt_after_restore()
        if rdist.collectives_active():
            self.sync_replicas()


class _OnPolicy(_DeferredStats):
    """What ``Trainer`` and ``RawStateTrainer`` share: the A2C / PPO statistics, PPO's adaptive KL coefficient and the statistics
    vector of a data-parallel PPO pass."""

    @property
    def kl_coeff(self):
        """PPO's adaptive KL coefficient AFTER every finished train call (waits for the last call's statistics)."""
        self._settle()
        return self._kl_coeff

    @kl_coeff.setter
    def kl_coeff(self, v):
        self._settle()
        self._kl_coeff = float(v)

    def _values(self, tok, mean_reward, s):
        """A token with ``kl_div`` is a PPO call: s[7] / kl_div is the pass-mean KL that RLlib's rule sees."""
        kl_mean = 0.0
        if tok.get('kl_div'):
            kl_mean = float(s[7]) / tok['kl_div']
            self._kl_coeff = update_kl_coeff(self._kl_coeff, kl_mean, self.kl_target)
        values = {'episode_reward_mean': mean_reward, 'policy_loss': float(s[0]), 'vf_loss': float(s[1]), 'entropy': float(s[2]),
                  'kl': float(s[3]), 'kl_mean': kl_mean, 'kl_coeff': self._kl_coeff}
        if tok.get('vtrace_rows'):                      # IMPALA: s[4:8] = sums of {rho, min(rho, clip_rho), vs, pg_adv} over the kept rows
            n = float(tok['vtrace_rows'])
            values.update(rho_mean=float(s[4]) / n, rho_clipped_mean=float(s[5]) / n, vs_mean=float(s[6]) / n)
        return values

    def _submit_ppo_minibatches(self, mean_reward, stats, kl_sum, rows):
        """Data-parallel PPO (one gradient / all-reduce / Adam per minibatch): the last minibatch's statistics and the KL sum over
        this rank's ``rows`` samples, laid out like the single-launch pass's eight.  Every rank must take the same kl_coeff
        decision: the rule sees the mean over ALL ranks' samples.  The sum is all-reduced ON THE DEVICE and travels with the
        deferred statistics: no rank reads a device scalar in a train call."""
        stats8 = torch.cat([stats.reshape(-1)[:4].to(torch.float32), torch.zeros(3, dtype=torch.float32, device=kl_sum.device),
                            kl_sum.reshape(1)])
        rdist.allreduce_sum_(stats8[7:8])
        return self._submit(mean_reward, stats8, kl_div=rows * rdist.world_size())


class RawStateTrainer(_OnPolicy):
    """The same loop for an env with config['rawstate_as_obs'] (+ support_rllib_mask, return_tensors): the policy is the
    raw-state encoder (rllib_rawstate_model.py; modelfree_train.py 'rawstate' variants) acting on the device tensors of the
    raw features; loss, backward and Adam run through rl4rs_rawtrain_*.

    Data-parallel: the gradient lives in the handle's flat buffer [cat_emb | seq_emb | dense layers]; the dense tail
    (~280 K floats) is mean-all-reduced in place, the two 100000 x 128 embedding tables exchange only the rows the minibatch
    touched (``dist.allreduce_rows_mean_``).

    No ``save`` / ``restore`` and no ``evaluate``: ``_Checkpoint`` covers the trainers of the flat policy networks only (this one's two
    100000 x 128 tables are 100 MB of parameters, three times that with Adam's moments)."""

    def __init__(self, env, algo='A2C', seed=0, lr=1e-4, minibatch=256, weights=None, init_seed=0, kl_coeff=0.2, kl_target=0.01):
        from .nets.rawpolicy import init_rawpolicy_weights
        cfg = env.config
        assert cfg.get('return_tensors', False) and cfg.get('rawstate_as_obs', False) and cfg.get('support_rllib_mask', False), \
            "RawStateTrainer needs config rawstate_as_obs + support_rllib_mask + return_tensors"
        self.env = env
        self.algo = {'A2C': D.DeviceRawTrainer.A2C, 'PPO': D.DeviceRawTrainer.PPO}[algo]
        self.B, self.T, self.A = cfg['batch_size'], cfg['max_steps'], cfg['action_size']
        self.S, self.L = cfg['seq_num'], cfg['maxlen']
        self.seed, self.lr, self.minibatch = seed, lr, minibatch
        self._kl_coeff, self.kl_target = float(kl_coeff), float(kl_target)
        self._pending = []
        if weights is None:
            weights = init_rawpolicy_weights(cfg, seed=init_seed)
        N = self.B * self.T
        if algo == 'PPO' and N < minibatch:
            raise ValueError("PPO needs at least one full minibatch per train call: batch_size * max_steps = %d < minibatch = %d"
                             % (N, minibatch))
        self.policy = D.DeviceRawTrainer(cfg, weights, max_rows=max(N, self.B))
        self.iteration = 0
        dev = self.policy.device
        W = self.policy.W
        self.buf = dict(cat=torch.empty((N, cfg['category_feature_num']), dtype=torch.int32, device=dev),
                        dense=torch.empty((N, cfg['dense_feature_num']), dtype=torch.float32, device=dev),
                        seqs=[torch.empty((N, self.L), dtype=torch.int32, device=dev) for _ in range(self.S)],
                        mask=torch.empty((N, W), dtype=torch.int32, device=dev),
                        act=torch.empty(N, dtype=torch.int32, device=dev), logp=torch.empty(N, dtype=torch.float32, device=dev),
                        val=torch.empty(N, dtype=torch.float32, device=dev), rew=torch.empty(N, dtype=torch.float64, device=dev),
                        logits=torch.empty((N, self.A), dtype=torch.float32, device=dev))
        self._grad = None
        self._row_caps = None            # static distinct-row bounds of the sparse table exchange (dist.calibrate_row_cap)
        if rdist.collectives_active():
            rdist.broadcast_(self.policy.flat_view('params'), src=0)      # replicas start identical (Adam state is zero)
            self._grad = self.policy.flat_view('grad')

    def _mask_bits(self, mask):
        W = self.policy.W
        m = mask.to(torch.int32)
        pad = W * 32 - self.A
        if pad:
            m = torch.nn.functional.pad(m, (0, pad))
        w = (m.view(self.B, W, 32) << torch.arange(32, device=m.device, dtype=torch.int32)).sum(dim=2, dtype=torch.int64)
        return (w & 0xffffffff).to(torch.int32).contiguous()

    def rollout(self):
        B, T = self.B, self.T
        obs = self.env.reset()
        b = self.buf
        for t in range(T):
            sl = slice(t * B, (t + 1) * B)
            bits = self._mask_bits(obs['action_mask'])
            seqs = [q.contiguous() for q in obs['sequence_feature']]
            a, lp, v, ent, lg = self.policy.act(obs['category_feature'], obs['dense_feature'], seqs, bits, seed=self.seed,
                                                step=self.iteration * T + t, want_logits=self.algo == D.DeviceRawTrainer.PPO)
            b['cat'][sl] = obs['category_feature']
            b['dense'][sl] = obs['dense_feature']
            for s in range(self.S):
                b['seqs'][s][sl] = seqs[s]
            b['mask'][sl] = bits
            b['act'][sl] = a
            b['logp'][sl] = lp
            b['val'][sl] = v
            if lg is not None:
                b['logits'][sl] = lg
            obs, reward, done, info = self.env.step(a)
            b['rew'][sl] = reward
        ret = _returns(b['rew'], 1, T, B)
        return ret, ret - b['val'], b['rew'].view(T, B).sum(dim=0).mean()         # stays on the device (LazyStats)

    def _allreduce_gradient(self, cat, seqs):
        """Mean over ranks of the gradient the last loss_grad left in the handle (no-op on one rank)."""
        if self._grad is None:
            return
        g = self._grad
        tables = self.policy.table_rows()
        # ids clamped the way the kernels clamp them; allreduce_rows_mean_ finds the distinct rows itself with fixed-shape
        # device ops (torch.unique would drain the queue once per minibatch)
        flat = [cat.reshape(-1).to(torch.int64), torch.cat([q.reshape(-1) for q in seqs]).to(torch.int64)]
        if self._row_caps is None:
            # static distinct-row bounds, measured on the first minibatch and agreed across the ranks (start-up only)
            self._row_caps = [rdist.calibrate_row_cap(i.clamp(0, H - 1), H) for (off, H, E), i in zip(tables, flat)]
        for (off, H, E), i, cap in zip(tables, flat, self._row_caps):
            rdist.allreduce_rows_mean_(g[off:off + H * E].view(H, E), i.clamp(0, H - 1), cap=cap)
        tail = tables[-1][0] + tables[-1][1] * tables[-1][2]
        rdist.allreduce_mean_(g[tail:])

    def train_iteration(self):
        """One train call; returns a ``LazyStats`` mapping (see Trainer.train_iteration)."""
        ret, adv, mean_reward = self.rollout()
        self._settle()
        b = self.buf
        N = self.B * self.T
        self.iteration += 1
        if self.algo == D.DeviceRawTrainer.A2C:
            stats = self.policy.loss_grad(self.algo, b['cat'], b['dense'], b['seqs'], b['act'], adv, ret, mask_bits=b['mask'],
                                          vf_coeff=0.5, ent_coeff=0.01)
            self._allreduce_gradient(b['cat'], b['seqs'])
            self.policy.adam_step(lr=self.lr, grad_clip=10.0)
            return self._submit(mean_reward, stats[:4])
        adv_n = (adv - adv.mean()) / adv.std().clamp_min(1e-4)
        perm = torch.from_numpy(np.random.RandomState(self.seed + self.iteration - 1).permutation(N)).to(b['cat'].device)
        sh = dict((k, b[k][perm]) for k in ('cat', 'dense', 'mask', 'act', 'logp', 'val', 'logits'))
        shs = [q[perm] for q in b['seqs']]
        adv_s, ret_s = adv_n[perm], ret[perm]
        kl_sum = torch.zeros((), dtype=torch.float32, device=b['cat'].device)
        nmb = 0
        for lo in range(0, N - self.minibatch + 1, self.minibatch):
            hi = lo + self.minibatch
            seq_mb = [q[lo:hi] for q in shs]
            stats = self.policy.loss_grad(self.algo, sh['cat'][lo:hi], sh['dense'][lo:hi], seq_mb, sh['act'][lo:hi],
                                          adv_s[lo:hi], ret_s[lo:hi], mask_bits=sh['mask'][lo:hi], old_logp=sh['logp'][lo:hi],
                                          old_value=sh['val'][lo:hi], old_logits=sh['logits'][lo:hi], vf_coeff=0.5,
                                          ent_coeff=0.0, clip=0.3, vf_clip=500.0, kl_coeff=self._kl_coeff)
            self._allreduce_gradient(sh['cat'][lo:hi], seq_mb)
            self.policy.adam_step(lr=self.lr)
            kl_sum += stats[3]
            nmb += 1
        return self._submit_ppo_minibatches(mean_reward, stats, kl_sum, nmb * self.minibatch)


class Trainer(_OnPolicy, _Evaluated, _Checkpoint):
    """A2C / PPO / PG / IMPALA on the action-masked FC policy (rllib_mask_model.py:7-64) over the zero-copy discrete-action env.

    seed       sampling stream of this rank (Gumbel noise, PPO shuffle): pass a different value per rank
    init_seed  parameter initialisation, shared by all ranks (and rank 0's parameters are broadcast anyway)
    lr         None = the driver's value for ``algo`` (DRIVER_LR: 1e-4 for A2C / PPO / IMPALA, 4e-4 for PG); a number is used as given
    kl_coeff / kl_target   PPO's adaptive KL penalty (update_kl_coeff above)
    train_batch_size       timesteps per train call (rollouts_per_train_call above; the reference's value = one rollout)
    keep_last_batch        keep the shuffled tensors of the last iteration in ``last_batch`` (tests)

    algo='PG' (RLlib pg_tf_policy, parity unpinned): loss = -mean(logp * return-to-go) with gamma 1 (``_returns``), Adam, no critic, no
    entropy term, no gradient clip.  It is the A2C loss with vf_coeff = ent_coeff = 0 and advantages = returns / N, so the value head
    receives an exactly zero gradient and keeps its initial bits; ``vf_loss`` / ``entropy`` are still reported (sums, as for A2C),
    ``policy_loss`` is the mean.

    algo='IMPALA' (RLlib impala with vtrace, parity unpinned): the rollout samples from a second handle, the ACTOR, and the learner's
    update is rl4rs_policy_vtrace_loss_grad on the whole rollout batch (no minibatches, no replay slots), the rank-mean gradient,
    Adam with global-norm clip 10.  After every ``broadcast_interval``-th update the learner's parameters are copied into the actor on
    the device: with 1 the run is on-policy up to kernel rounding (every importance weight is 1), with k the actor is stale in k - 1
    of every k train calls - a deterministic stand-in for RLlib's asynchronous workers.  ``vtrace_clip_rho`` /
    ``vtrace_clip_pg_rho`` / ``vf_coeff`` / ``ent_coeff`` are RLlib's vtrace_clip_rho_threshold / vtrace_clip_pg_rho_threshold /
    vf_loss_coeff / entropy_coeff.  ``drop_last=True`` is RLlib's behaviour: the last step of every rollout only supplies the
    bootstrap value.  On SlateRecEnv-v0 the only reward arrives at that last step, so with drop_last=True THE LEARNER SEES NO REWARD
    (what the reference's IMPALA branch does as written); pass drop_last=False (all T steps, zero bootstrap) to train on it.
    ``train_iteration`` adds rho_mean, rho_clipped_mean and vs_mean (means over the kept rows) to the A2C statistics.

    ``evaluate(episodes, seed)`` (the driver's eval stage) plays the learner's greedy action under the env's mask; ``save(path)`` /
    ``restore(path)`` are ``_Checkpoint``'s: a restored trainer with the same ``seed`` continues bit for bit."""

    DRIVER_LR = {'A2C': 1e-4, 'PPO': 1e-4, 'IMPALA': 1e-4, 'PG': 4e-4}          # script/modelfree_train.py:204,261,354,309

    def __init__(self, env, algo='A2C', hidden=64, seed=0, lr=None, minibatch=256, init_seed=0, kl_coeff=0.2, kl_target=0.01,
                 train_batch_size=None, keep_last_batch=False, broadcast_interval=1, vtrace_clip_rho=1.0, vtrace_clip_pg_rho=1.0,
                 drop_last=True, vf_coeff=0.5, ent_coeff=0.01, grad_clip=10.0):
        cfg = env.config
        self._check_env(cfg)
        self.env = env
        if algo not in self.DRIVER_LR:
            raise ValueError("%s runs A2C, PPO, PG or IMPALA; got algo = %r" % (type(self).__name__, algo))
        # PG and IMPALA run on the A2C form of the loss kernels
        self.algo = {'A2C': D.DevicePolicy.A2C, 'PPO': D.DevicePolicy.PPO, 'PG': D.DevicePolicy.A2C, 'IMPALA': D.DevicePolicy.A2C}[algo]
        self.algo_name = algo
        self.B, self.T, self.A = cfg['batch_size'], cfg['max_steps'], cfg['action_size']
        self.hidden = int(hidden)
        self.R = rollouts_per_train_call(self.B, self.T, train_batch_size)
        if lr is None:
            lr = self.DRIVER_LR[algo]
        self.seed, self.lr, self.minibatch = seed, lr, minibatch
        self.broadcast_interval, self.drop_last = int(broadcast_interval), bool(drop_last)
        self.vtrace_clip_rho, self.vtrace_clip_pg_rho = float(vtrace_clip_rho), float(vtrace_clip_pg_rho)
        self.vf_coeff, self.ent_coeff, self.grad_clip = float(vf_coeff), float(ent_coeff), float(grad_clip)
        if algo == 'IMPALA':
            if self.broadcast_interval < 1:
                raise ValueError("IMPALA: broadcast_interval must be >= 1 (got %r)" % (broadcast_interval,))
            if self.drop_last and self.T < 2:
                raise ValueError("IMPALA: drop_last needs max_steps >= 2 (the dropped step's value is the bootstrap)")
        self._kl_coeff, self.kl_target = float(kl_coeff), float(kl_target)
        self._pending = []          # train calls whose statistics have not been looked at yet (oldest first)
        self.keep_last_batch = keep_last_batch
        self.last_batch = None
        N = self.R * self.B * self.T
        if algo == 'PPO' and N < minibatch:
            # (N // minibatch == 0 would leave the data-parallel pass without a single step: undefined statistics, a division
            # by zero, ranks failing at different points around a collective)
            raise ValueError("PPO needs at least one full minibatch per train call: %d rollouts x batch_size x max_steps = %d < "
                             "minibatch = %d" % (self.R, N, minibatch))
        self.OD = _obs_width(env)
        self.policy = self._new_policy(N, init_seed)
        share = rdist.ranks_sharing_device()
        if share > 1 and hasattr(self.policy, 'set_option'):
            # several ranks on ONE GPU (gloo dry runs only): the persistent PPO pass may use its grid barrier only while the grids of
            # all the processes on the device fit together, one workgroup per CU; beyond that the per-minibatch kernels run
            n_cu = torch.cuda.get_device_properties(self.policy.device).multi_processor_count
            self.policy.set_option('resident_wgs', n_cu // share)
        self.iteration = 0
        self._rollouts = 0
        dev = self.policy.device
        self.buf = self._new_buffers(N, dev)
        self.grad = torch.empty(self.policy.n_params, dtype=torch.float32, device=dev)
        self._mb_stats = torch.empty(4, dtype=torch.float32, device=dev)
        self.actor = None
        self.num_updates = 0
        if rdist.collectives_active():
            self.sync_replicas()
        if algo == 'IMPALA':
            # the actor: the handle rollouts sample from; it only ever sees one env batch per call
            self.actor = self._new_policy(self.B, init_seed)
            self.actor.copy_params_from(self.policy)
            self._vt_stats = torch.empty(4, dtype=torch.float64, device=dev)
        self.device = dev
        self._owned = (self.policy,) + ((self.actor,) if self.actor is not None else ())
        self._eval_act = torch.empty(self.B, dtype=torch.int32, device=dev)

    _ckpt_host = ('iteration', '_rollouts', 'num_updates', '_kl_coeff')

    def _ckpt_nets(self):
        return [('policy', self.policy, True)] + ([('actor', self.actor, False)] if self.actor is not None else [])

    # ---- what ContiTrainer states differently: the env it takes, the policy handle, the rollout columns (and ``rollout``)
    _old = 'logits'                     # the rollout column PPO's KL term reads: the old distribution's parameters
    _masked = True                      # the policy calls take the packed action mask of the rollout

    def _check_env(self, cfg):
        _require_env(cfg, DISCRETE_ENV_MESSAGE % 'Trainer' + "; the continuous-action env (support_conti_env) is ContiTrainer's")

    def _new_policy(self, max_rows, init_seed):
        return D.DevicePolicy(self.OD, self.hidden, self.A, max_rows=max_rows, seed=init_seed)

    def _new_buffers(self, N, dev):
        return dict(obs=torch.empty((N, self.OD), dtype=torch.float32, device=dev),
                    mask=torch.empty((N, self.policy.W), dtype=torch.int32, device=dev),
                    act=torch.empty(N, dtype=torch.int32, device=dev),
                    logp=torch.empty(N, dtype=torch.float32, device=dev),
                    val=torch.empty(N, dtype=torch.float32, device=dev),
                    rew=torch.empty(N, dtype=torch.float64, device=dev),
                    logits=torch.empty((N, self.A), dtype=torch.float32, device=dev))

    def _mask_kw(self, b):
        return dict(mask_bits=b['mask']) if self._masked else {}

    def sync_replicas(self, src=0):
        """Make every rank's parameters, Adam moments and step counter those of rank ``src``."""
        sync_policy_replicas(self.policy, src)

    def params(self):
        """Flat parameters (validated: raises if a persistent pass was cut short)."""
        self._settle()
        self.policy.check_status()
        return self.policy.params()

    def close(self):
        try:
            self._settle()
            self.policy.check_status()
        finally:
            self.policy.close()
            if self.actor is not None:
                self.actor.close()

    def _mask_bits(self):
        """Packed obs-side action mask (action_mask & location_mask[layer] & special_mask, slate.py:92-97)."""
        return self.env.samples._live().obs_mask_bits()          # packed on the device: no dense [B, A] round trip

    def _eval_batch(self, k):
        """One episode batch on the LEARNER's greedy action (the first maximum of its masked logits; IMPALA's actor only samples
        rollouts) under the env's mask -> mean episode reward (device scalar)."""
        obs = self.env.reset(reset_file=True) if k == 0 else self.env.reset()
        total = torch.zeros(self.B, dtype=torch.float64, device=self.device)
        for t in range(self.T):
            obs_t = (obs['obs'] if isinstance(obs, dict) else obs).contiguous()
            a = self.policy.greedy(obs_t, self._mask_bits(), out=self._eval_act)[0]
            obs, reward, done, info = self.env.step(a)
            total += reward
        return total.mean()

    def rollout(self):
        B, T, R = self.B, self.T, self.R
        b = self.buf
        ppo = self.algo == D.DevicePolicy.PPO
        actor = self.actor if self.actor is not None else self.policy          # IMPALA samples from the (possibly stale) actor
        for r in range(R):
            obs = self.env.reset()
            for t in range(T):
                obs_t = obs['obs'] if isinstance(obs, dict) else obs
                sl = slice((r * T + t) * B, (r * T + t + 1) * B)
                # mask, sampled actions, log-probs, values (and PPO's logits) are written straight into the rollout buffers
                mask = self.env.samples._live().obs_mask_bits(out=b['mask'][sl])
                b['obs'][sl] = obs_t
                a = actor.act(b['obs'][sl], mask, seed=self.seed, step=self._rollouts * T + t, want_logits=ppo,
                              out=(b['act'][sl], b['logp'][sl], b['val'][sl], b['logits'][sl] if ppo else None))[0]
                obs, reward, done, info = self.env.step(a)
                b['rew'][sl] = reward
            self._rollouts += 1
        # gamma = 1, lambda = 1: advantage = (sum of future rewards) - V
        ret = _returns(b['rew'], R, T, B)
        adv = ret - b['val']
        return ret, adv, b['rew'].view(R, T, B).sum(dim=1).mean()        # mean episode reward stays on the device

    def train_iteration(self):
        """One train call.  Returns a ``LazyStats`` mapping (episode_reward_mean, policy_loss, vf_loss, entropy, kl, kl_mean,
        kl_coeff, iteration): nothing in here waits for the GPU on one rank - the previous call's numbers (needed for PPO's KL
        rule and to validate its pass) are collected after this call's rollout has been enqueued, when they are long there."""
        ret, adv, mean_reward = self.rollout()
        self._settle()                       # previous call: statistics, pass status, kl_coeff (the GPU is busy with the rollout)
        b = self.buf
        N = self.R * self.B * self.T
        self.iteration += 1
        if self.algo_name == 'IMPALA':
            # V-trace needs neither the returns nor the actor's values: the learner re-evaluates every row
            g, stats, vstats = self.policy.vtrace_loss_grad(self.R, self.T, self.B, b['obs'], b['act'], b['logp'], b['rew'],
                                                            gamma=1.0, clip_rho=self.vtrace_clip_rho,
                                                            clip_pg_rho=self.vtrace_clip_pg_rho, drop_last=self.drop_last,
                                                            vf_coeff=self.vf_coeff, ent_coeff=self.ent_coeff, grad_out=self.grad,
                                                            stats_out=self._mb_stats, vtrace_stats_out=self._vt_stats,
                                                            **self._mask_kw(b))[:3]
            if self.keep_last_batch:
                self.last_batch = dict((k, b[k].clone()) for k in ('obs', 'act', 'mask', 'logp', 'rew') if k in b)
            rdist.allreduce_mean_(g)
            self.policy.adam_step(g, lr=self.lr, grad_clip=self.grad_clip)
            self.num_updates += 1
            if self.num_updates % self.broadcast_interval == 0:
                self.actor.copy_params_from(self.policy)            # device to device, in stream order behind the Adam step
            kept = self.R * (self.T - 1 if self.drop_last else self.T) * self.B
            return self._submit(mean_reward, torch.cat([stats.to(torch.float64), vstats]), vtrace_rows=kept)
        if self.algo == D.DevicePolicy.A2C:
            if self.algo_name == 'PG':
                # -mean(logp * return): the A2C kernels with the critic and the entropy term off and the 1 / N folded into the advantages
                adv, vf_coeff, ent_coeff, grad_clip = ret * (1.0 / N), 0.0, 0.0, 0.0
            else:
                vf_coeff, ent_coeff, grad_clip = 0.5, 0.01, 10.0
            g, stats = self.policy.loss_grad(self.algo, b['obs'], b['act'], adv, ret, vf_coeff=vf_coeff, ent_coeff=ent_coeff,
                                             grad_out=self.grad, **self._mask_kw(b))
            if self.keep_last_batch:
                self.last_batch = dict(((k, b[k].clone()) for k in ('obs', 'act', 'mask') if k in b), adv=adv.clone(), ret=ret.clone())
            rdist.allreduce_mean_(g)                         # the ONE collective: flat policy gradient over RCCL
            self.policy.adam_step(g, lr=self.lr, grad_clip=grad_clip)
            return self._submit(mean_reward, stats[:4])
        adv_n = (adv - adv.mean()) / adv.std().clamp_min(1e-4)      # RLlib standardises PPO advantages
        perm = torch.from_numpy(np.random.RandomState(self.seed + self.iteration - 1).permutation(N)).to(b['obs'].device)
        # shuffle every buffer ONCE (7 gathers per iteration instead of 7 per minibatch): minibatches are then
        # contiguous row ranges that go to the library as plain pointers
        sh = dict((k, b[k][perm]) for k in ('obs', 'act', 'mask', 'logp', 'val', self._old) if k in b)
        adv_s, ret_s = adv_n[perm].contiguous(), ret[perm].contiguous()
        if self.keep_last_batch:
            self.last_batch = dict(sh, adv=adv_s, ret=ret_s, kl_coeff=self._kl_coeff)
        MB = self.minibatch
        nmb = N // MB
        old = ((sh['mask'],) if self._masked else ()) + (sh['logp'], sh['val'], sh[self._old])
        if not rdist.collectives_active():
            # single GPU: the whole pass is one library call (no per-minibatch collective to interleave)
            stats = self.policy.ppo_epoch(sh['obs'], sh['act'], adv_s, ret_s, *old, minibatch=MB, vf_coeff=0.5, ent_coeff=0.0,
                                          clip=0.3, vf_clip=500.0, kl_coeff=self._kl_coeff, lr=self.lr, grad_out=self.grad)
            return self._submit(mean_reward, stats, kl_div=nmb * MB)
        # data parallel: per minibatch ONE fused gradient launch, ONE all-reduce, ONE Adam launch
        kl_sum = torch.zeros((), dtype=torch.float32, device=b['obs'].device)
        for mb in range(nmb):
            g, stats = self.policy.ppo_minibatch_grad(mb, sh['obs'], sh['act'], adv_s, ret_s, *old, minibatch=MB, vf_coeff=0.5, ent_coeff=0.0,
                                                      clip=0.3, vf_clip=500.0, kl_coeff=self._kl_coeff,
                                                      grad_out=self.grad, stats_out=self._mb_stats)
            rdist.allreduce_mean_(g)
            self.policy.adam_step(g, lr=self.lr)
            kl_sum += stats[3]
        # (the KL sum settles with the deferred statistics like the single-GPU path; ADVICE / VERDICT r3: this path used to read
        # kl_sum on the host - one queue drain per train call and rank)
        return self._submit_ppo_minibatches(mean_reward, stats, kl_sum, nmb * MB)


class ContiTrainer(Trainer, _Evaluated):
    """A2C / PPO / PG / IMPALA on the Gaussian actor-critic (``DeviceGaussPolicy``: RLlib's default FullyConnectedNetwork and its
    DiagGaussian, restated, parity unpinned) over the zero-copy continuous-action env - the ``is_conti`` branches of
    script/modelfree_train.py:219-234,271-286,315-330,362-377.  Constructor arguments, defaults, ``DRIVER_LR`` and ``train_iteration``
    are ``Trainer``'s, branch for branch; what differs is the policy handle and the action column: the rollout stores the unclipped
    action [N, E] (the log-probability and every loss use it) and steps the env with ``clip(a, -1, 1)``, which the env's masked K-NN
    turns into an item; PPO keeps the old head [N, 2E] where ``Trainer`` keeps the old logits.  ``hidden`` is the width of both
    hidden layers of both towers (64, 128 or 256).

    Deviations, as in ``Trainer``: IMPALA's actor lag is the deterministic ``broadcast_interval``, and a train call consumes whole
    rollouts.  ``support_onehot_action`` (a 284-wide action) and ``rawstate_as_obs`` are refused.

    ``evaluate(episodes, seed)`` plays the deterministic action (the mean)."""

    _old = 'head'
    _masked = False

    def __init__(self, env, algo='A2C', hidden=256, seed=0, lr=None, minibatch=256, init_seed=0, kl_coeff=0.2, kl_target=0.01,
                 train_batch_size=None, keep_last_batch=False, broadcast_interval=1, vtrace_clip_rho=1.0, vtrace_clip_pg_rho=1.0,
                 drop_last=True, vf_coeff=0.5, ent_coeff=0.01, grad_clip=10.0):
        Trainer.__init__(self, env, algo=algo, hidden=hidden, seed=seed, lr=lr, minibatch=minibatch, init_seed=init_seed, kl_coeff=kl_coeff,
                         kl_target=kl_target, train_batch_size=train_batch_size, keep_last_batch=keep_last_batch,
                         broadcast_interval=broadcast_interval, vtrace_clip_rho=vtrace_clip_rho, vtrace_clip_pg_rho=vtrace_clip_pg_rho,
                         drop_last=drop_last, vf_coeff=vf_coeff, ent_coeff=ent_coeff, grad_clip=grad_clip)
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)
        self._env_act = f(self.B, self.E)                   # the clipped draw of the current step: what the env receives
        self._eval = (f(self.B, self.E), f(self.B, self.E), f(self.B), f(self.B), None)

    def _check_env(self, cfg):
        _require_env(cfg, "ContiTrainer needs the zero-copy continuous-action env (config['return_tensors'] and ['support_conti_env'] = True)",
                     conti=True)
        if cfg.get('support_onehot_action', False):
            raise ValueError("ContiTrainer: support_onehot_action (an action as wide as the catalogue) is out of scope: the Gaussian "
                             "policy takes act_dim <= 64")
        if cfg.get('rawstate_as_obs', False):
            raise ValueError("ContiTrainer: rawstate_as_obs is out of scope (the *_rawstate variants of the continuous learners)")
        self.E = int(cfg.get('action_emb_size', 32))

    def _new_policy(self, max_rows, init_seed):
        return D.DeviceGaussPolicy(self.OD, self.E, max_rows=max_rows, hidden=self.hidden, seed=init_seed)

    def _new_buffers(self, N, dev):
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        b = dict(obs=f(N, self.OD), act=f(N, self.E), logp=f(N), val=f(N), rew=torch.empty(N, dtype=torch.float64, device=dev))
        if self.algo == D.DeviceGaussPolicy.PPO:
            b['head'] = f(N, 2 * self.E)
        return b

    def params(self):
        self._settle()
        return self.policy.params()

    def close(self):
        _Evaluated.close(self)

    def rollout(self):
        B, T, R = self.B, self.T, self.R
        b = self.buf
        actor = self.actor if self.actor is not None else self.policy          # IMPALA samples from the (possibly stale) actor
        for r in range(R):
            obs = self.env.reset()
            for t in range(T):
                obs_t = obs['obs'] if isinstance(obs, dict) else obs
                sl = slice((r * T + t) * B, (r * T + t + 1) * B)
                b['obs'][sl] = obs_t
                # the draw, its log-prob, the value (and PPO's head) go straight into the rollout buffers; the env gets the clipped draw
                actor.act(b['obs'][sl], seed=self.seed, step=self._rollouts * T + t,
                          out=(b['act'][sl], self._env_act, b['logp'][sl], b['val'][sl], b['head'][sl] if 'head' in b else None))
                obs, reward, done, info = self.env.step(self._env_act)
                b['rew'][sl] = reward
            self._rollouts += 1
        ret = _returns(b['rew'], R, T, B)
        return ret, ret - b['val'], b['rew'].view(R, T, B).sum(dim=1).mean()

    def _eval_batch(self, k):
        """One episode batch on the mean action -> mean episode reward (device scalar)."""
        obs = self.env.reset(reset_file=True) if k == 0 else self.env.reset()
        total = torch.zeros(self.B, dtype=torch.float64, device=self.device)
        for t in range(self.T):
            obs_t = (obs['obs'] if isinstance(obs, dict) else obs).contiguous()
            self.policy.act(obs_t, deterministic=True, out=self._eval)
            obs, reward, done, info = self.env.step(self._eval[1])
            total += reward
        return total.mean()


class _ReplayTrainer(_Evaluated, _Checkpoint):
    """The loop of the replay learners (DQN, Rainbow, TD3 / DDPG): one complete-episode rollout into ``buf``, the push of its
    ``_columns`` into the replay ring, ``updates_per_rollout`` updates once ``learning_starts`` sampled steps are reached.  A trainer
    fills ``_act`` (and ``_step_mask``), ``update``, ``_stats0``, ``_after_updates``, ``_extras`` and ``_values``, and ``_new_replay``
    (a fresh, empty ring: what ``restore`` leaves, see ``_Checkpoint``)."""

    _ckpt_host = ('iteration', '_rollouts', 'timesteps', 'num_updates')

    def _ckpt_after_restore(self):
        old, self.replay = self.replay, self._new_replay()
        self._owned = tuple(self.replay if h is old else h for h in self._owned)
        old.close()

    def _init_loop(self, env, seed, train_batch_size, learning_starts, updates_per_rollout, prioritized_replay, beta, keep_last_batch):
        cfg = env.config
        self.env, self.seed = env, seed
        self.B, self.T = cfg['batch_size'], cfg['max_steps']
        self.M = _default_minibatch(self.B, self.T, train_batch_size)
        self.OD = self._obs_dim(env)
        self.learning_starts, self.updates_per_rollout = int(learning_starts), int(updates_per_rollout)
        self.prioritized, self.beta = bool(prioritized_replay), float(beta)
        self.keep_last_batch, self.last_batch = keep_last_batch, None
        self._pending = []
        self.iteration = 0
        self._rollouts = 0
        self.timesteps = 0                  # sampled env steps (RLlib's num_steps_sampled)
        self.num_updates = 0

    def _obs_dim(self, env):
        """Floats of one row of the rollout buffer's and the ring's observation column."""
        return _obs_width(env)

    def _step_mask(self, sl):
        """The packed action mask of the current observation, written into rows ``sl`` of the rollout buffer (None: no mask)."""
        return None

    def _episode(self, explore, step0, reset_file=False):
        """One complete-episode rollout into the rollout buffers -> mean episode reward (device scalar)."""
        B, T = self.B, self.T
        b = self.buf
        obs = self.env.reset(reset_file=True) if reset_file else self.env.reset()
        for t in range(T):
            obs_t = obs['obs'] if isinstance(obs, dict) else obs
            sl = slice(t * B, (t + 1) * B)
            mask = self._step_mask(sl)
            b['obs'][sl] = obs_t
            a = self._act(explore, sl, mask, t, step0 + t)
            obs, reward, done, info = self.env.step(a)
            b['rew'][sl] = reward
        return b['rew'].view(T, B).sum(dim=0).mean()

    def _eval_batch(self, k):
        return self._episode(False, 0, reset_file=k == 0)

    def _sample(self, **kw):
        # (the replay draws share the counter RNG of the action noise: a seed of their own keeps them apart from the noise of row = draw)
        return self.replay.sample(self.M, prioritized=self.prioritized, beta=self.beta, seed=self.seed + 0x5bd1e995, step=self.num_updates,
                                  out=self._batch, **kw)

    def _keep(self, b):
        self.last_batch = dict((k, v.clone()) for k, v in b.items() if v is not None)

    def _after_updates(self):
        pass

    def train_iteration(self):
        """One rollout, one push, ``updates_per_rollout`` updates once ``learning_starts`` sampled steps are reached, then
        ``_after_updates``.  Returns a ``LazyStats`` mapping (``_values``); nothing here waits for the GPU."""
        mean_reward = self._episode(True, self._rollouts * self.T)
        self._rollouts += 1
        self._settle()
        self.replay.push(*[self.buf[k] for k in self._columns])
        self.timesteps += self.B * self.T
        self.iteration += 1
        stats = self._stats0()
        trained = self.timesteps >= self.learning_starts
        if trained:
            for _ in range(self.updates_per_rollout):
                stats = self.update()
        self._after_updates()
        return self._submit(mean_reward, stats, buffer_rows=self.replay.rows, num_updates=self.num_updates, **self._extras(trained))


class DQNTrainer(_ReplayTrainer):
    """Online DQN on the action-masked FC net (rllib_mask_model.py:7-64) over the zero-copy discrete-action env, with the
    reference's merged RLlib 1.5.1 configuration (script/modelfree_train.py:106-133 over the DQN defaults) as defaults: gamma 1,
    lr 5e-4, Adam eps 1e-8, grad_clip 40 per variable, double_q, n_step 1, buffer_size 100000, target_network_update_freq 200
    sampled timesteps, learning_starts 1000, train_batch_size min(B * T, 1024), prioritized replay alpha 0.6 / beta 0.4 (constant),
    SoftQ exploration at temperature 1 (= the net's own categorical draw, ``DevicePolicy.act``).  RLlib parity is unpinned (ray is
    absent), as for A2C and PPO.

    seed / init_seed        as in ``Trainer`` (this rank's sampling streams / the shared parameter initialisation)
    updates_per_rollout     updates after every rollout once learning_starts is reached.  1 is RLlib's round-robin (one train op per
                            sample op); at B = 4096, T = 9 that is one update per 36 864 env steps, which starves the learner, so this
                            is a knob
    The replay ring holds whole rollouts: max(1, buffer_size // (B * T)) of them (the one deviation from RLlib's per-timestep
    ring)."""

    _columns = ('obs', 'mask', 'act', 'rew')

    def __init__(self, env, hidden=64, seed=0, init_seed=0, lr=5e-4, gamma=1.0, adam_eps=1e-8, grad_clip=40.0, double_q=True, n_step=1,
                 buffer_size=100000, target_network_update_freq=200, learning_starts=1000, train_batch_size=None,
                 prioritized_replay=True, prioritized_replay_alpha=0.6, prioritized_replay_beta=0.4, softq_temperature=1.0,
                 updates_per_rollout=1, keep_last_batch=False):
        _require_env(env.config, DISCRETE_ENV_MESSAGE % 'DQNTrainer')
        if n_step != 1:
            raise ValueError("DQNTrainer implements n_step = 1 (the reference's setting, modelfree_train.py:117); got %r" % (n_step,))
        if softq_temperature != 1.0:
            raise ValueError("DQNTrainer explores with SoftQ at temperature 1.0 (RLlib's default); got %r" % (softq_temperature,))
        self._init_loop(env, seed, train_batch_size, learning_starts, updates_per_rollout, prioritized_replay, prioritized_replay_beta,
                        keep_last_batch)
        self.A, self.n_step = env.config['action_size'], 1
        self.lr, self.gamma, self.adam_eps, self.grad_clip = float(lr), float(gamma), float(adam_eps), float(grad_clip)
        self.double_q, self.target_network_update_freq = bool(double_q), int(target_network_update_freq)
        self._make_net(hidden, init_seed)
        dev = self.device = self.policy.device
        self._new_replay = lambda: D.DeviceReplay(self.OD, self.A, self.T, self.B, buffer_size=buffer_size, alpha=prioritized_replay_alpha,
                                                  device=dev)
        self.replay = self._new_replay()
        self._owned = (self.policy, self.replay)
        N = self.B * self.T
        self.buf = dict(obs=torch.empty((N, self.OD), dtype=torch.float32, device=dev),
                        mask=torch.empty((N, self.policy.W), dtype=torch.int32, device=dev),
                        act=torch.empty(N, dtype=torch.int32, device=dev),
                        rew=torch.empty(N, dtype=torch.float64, device=dev))
        self._batch = self.replay.new_batch(self.M)
        self._td = torch.empty(self.M, dtype=torch.float32, device=dev)
        self.grad = self._new_grad()
        self.num_target_updates = 0
        self._last_target_sync = 0
        if rdist.collectives_active():
            sync_policy_replicas(self.policy)
        self.target = self.policy.params()                  # the target net starts as a copy of the online one

    _ckpt_host = _ReplayTrainer._ckpt_host + ('_last_target_sync', 'num_target_updates')

    def _ckpt_nets(self):
        return [('policy', self.policy, True)]

    def _ckpt_tensors(self):
        return {'target': self.target}

    def sync_replicas(self, src=0):
        """Make every rank's online parameters, Adam state and target those of rank ``src``."""
        sync_policy_replicas(self.policy, src)
        rdist.broadcast_(self.target, src)

    def _make_net(self, hidden, init_seed):
        """The online network ``policy`` and what its act call writes besides the action."""
        self.policy = D.DevicePolicy(self.OD, hidden, self.A, max_rows=max(self.M, self.B), seed=init_seed)
        self._logp = torch.empty(self.B, dtype=torch.float32, device=self.policy.device)
        self._val = torch.empty(self.B, dtype=torch.float32, device=self.policy.device)

    def _new_grad(self):
        """The flat gradient buffer the loss calls fill (None: the network's handle keeps its own)."""
        return torch.empty(self.policy.n_params, dtype=torch.float32, device=self.device)

    def _adam_step(self, g):
        self.policy.adam_step_clip_by_var(g, lr=self.lr, eps=self.adam_eps, var_clip=self.grad_clip)

    def params(self):
        self._settle()
        return self.policy.params()

    def _step_mask(self, sl):
        return self.env.samples._live().obs_mask_bits(out=self.buf['mask'][sl])

    def _act(self, explore, sl, mask, t, step):
        """SoftQ at temperature 1 (= the net's own categorical draw), or the greedy action."""
        b = self.buf
        if explore:
            return self.policy.act(b['obs'][sl], mask, seed=self.seed, step=step, out=(b['act'][sl], self._logp, self._val, None))[0]
        return self.policy.greedy(b['obs'][sl], mask, out=b['act'][sl])[0]

    def sync_target(self):
        """target <- online, a device-to-device copy."""
        self.policy.params(out=self.target)
        self._last_target_sync = self.timesteps
        self.num_target_updates += 1

    def _loss_grad(self, b, w):
        """-> (grad, td, stats[4] device sums of {w * huber, Q(s)[a], y, |td|} over the minibatch, a* or None)."""
        return self.policy.dqn_loss_grad(self.target, b['obs'], b['action'], b['reward'], b['done'], b['next_obs'], b['next_mask'],
                                         weights=w, gamma=self.gamma, double_q=self.double_q, grad_out=self.grad, td_out=self._td,
                                         want_next_action=self.keep_last_batch)

    def update(self):
        """One learner step: (n-step) sample -> loss / gradient (``_loss_grad``) -> all-reduce (data parallel) -> per-variable-clipped
        Adam -> priorities.  -> the loss call's stats[4]."""
        b = self._sample(n_step=self.n_step, gamma=self.gamma)
        g, td, stats, astar = self._loss_grad(b, b['weight'] if self.prioritized else None)
        if self.keep_last_batch:
            self._keep(b)
            self.last_batch.update(td=td.clone(), next_action=astar)
        if rdist.collectives_active():
            rdist.allreduce_mean_(g)
        self._adam_step(g)
        if self.prioritized:
            self.replay.update_priorities(b['idx'], td)
        self.num_updates += 1
        return stats

    def _stats0(self):
        return torch.zeros(4, dtype=torch.float32, device=self.device)

    def _after_updates(self):
        """The target copy when due."""
        if self.timesteps - self._last_target_sync >= self.target_network_update_freq:
            self.sync_target()

    def _extras(self, trained):
        return dict(rows=self.M if trained and self.updates_per_rollout > 0 else 0, num_target_updates=self.num_target_updates)

    def _values(self, tok, mean_reward, s):
        """episode_reward_mean, td_loss, mean_q, mean_td_abs of the last update - 0 before the first -, buffer_rows, num_updates,
        num_target_updates (and iteration)."""
        n = max(tok['rows'], 1)
        return {'episode_reward_mean': mean_reward, 'td_loss': float(s[0]) / n, 'mean_q': float(s[1]) / n, 'mean_td_abs': float(s[3]) / n,
                'buffer_rows': tok['buffer_rows'], 'num_updates': tok['num_updates'], 'num_target_updates': tok['num_target_updates']}


class RainbowTrainer(DQNTrainer):
    """Online Rainbow - distributional (C51), dueling, double-Q, n-step DQN - over the zero-copy discrete-action env, with what the
    reference's driver makes of RLlib 1.5.1's DQN defaults (script/modelfree_train.py:50-53,146-178) as defaults: num_atoms 8 over
    [v_min 0, v_max 1000], dueling, double_q, n_step 3, gamma 1, lr 5e-4, Adam eps 1e-8, grad_clip 40 per variable,
    target_network_update_freq 500 sampled timesteps, learning_starts 1000, buffer_size 100000, train_batch_size min(B * T, 1024),
    prioritized replay alpha 0.6 / beta 0.4, SoftQ exploration at temperature 1 over Q, noisy False.  The network is RLlib's
    default model (``DeviceDistQ``), initialised by ``init_distq_params(seed=init_seed)``.  RLlib parity is unpinned (ray is
    absent), as for DQN / A2C / PPO.

    The env may be the plain-observation one (the reference's setting: it forces support_rllib_mask False, because its
    distributional model "will make action masking not work") or the support_rllib_mask one.
    masked      False: the reference's unmasked behaviour.  True: the env's packed action mask goes to act / greedy / a*, where it
                sets a disallowed action's Q to -3.4e38 (the logits are untouched) - the second deviation from the reference
    The replay ring holds whole rollouts (``DQNTrainer``); without ``masked`` its mask words are all ones.
    Structure, statistics and the data-parallel all-reduce of the flat gradient are ``DQNTrainer``'s; ``train_iteration`` reports
    td_loss (the mean weighted cross-entropy), mean_q, mean_target (the mean of the projected target distribution) and
    mean_td_abs (the mean cross-entropy = the new priorities) of the last update."""

    def __init__(self, env, seed=0, init_seed=0, lr=5e-4, gamma=1.0, adam_eps=1e-8, grad_clip=40.0, double_q=True, n_step=3, num_atoms=8,
                 v_min=0.0, v_max=1000.0, dueling=True, noisy=False, masked=False, trunk=256, stream_hidden=128, buffer_size=100000,
                 target_network_update_freq=500, learning_starts=1000, train_batch_size=None, prioritized_replay=True,
                 prioritized_replay_alpha=0.6, prioritized_replay_beta=0.4, softq_temperature=1.0, updates_per_rollout=1,
                 keep_last_batch=False):
        _require_env(env.config, DISCRETE_ENV_MESSAGE % 'RainbowTrainer')
        if noisy:
            raise ValueError("RainbowTrainer: noisy layers are not implemented (the reference leaves RLlib's noisy = False)")
        if int(num_atoms) < 2:
            raise ValueError("RainbowTrainer is the distributional learner (num_atoms >= 2); num_atoms = 1 is DQNTrainer")
        if int(n_step) < 1 or float(softq_temperature) <= 0.0:
            raise ValueError("RainbowTrainer: n_step >= 1 and softq_temperature > 0 (got %r, %r)" % (n_step, softq_temperature))
        self._net_kw = dict(num_atoms=num_atoms, v_min=v_min, v_max=v_max, dueling=dueling, trunk=trunk, stream_hidden=stream_hidden)
        DQNTrainer.__init__(self, env, seed=seed, init_seed=init_seed, lr=lr, gamma=gamma, adam_eps=adam_eps, grad_clip=grad_clip,
                            double_q=double_q, buffer_size=buffer_size, target_network_update_freq=target_network_update_freq,
                            learning_starts=learning_starts, train_batch_size=train_batch_size, prioritized_replay=prioritized_replay,
                            prioritized_replay_alpha=prioritized_replay_alpha, prioritized_replay_beta=prioritized_replay_beta,
                            updates_per_rollout=updates_per_rollout, keep_last_batch=keep_last_batch)
        self.n_step, self.masked, self.temperature = int(n_step), bool(masked), float(softq_temperature)
        self.gamma_n = float(np.float32(self.gamma ** self.n_step))
        self.buf['mask'].fill_(-1)                          # all ones unless ``masked``

    def _make_net(self, hidden, init_seed):
        self.policy = D.DeviceDistQ(self.OD, self.A, max_rows=max(self.M, self.B), seed=init_seed, **self._net_kw)

    def _step_mask(self, sl):
        return DQNTrainer._step_mask(self, sl) if self.masked else None

    def _act(self, explore, sl, mask, t, step):
        """SoftQ over Q at ``temperature``, or the greedy action."""
        if not explore:
            return DQNTrainer._act(self, False, sl, mask, t, step)
        b = self.buf
        return self.policy.act(b['obs'][sl], mask, temperature=self.temperature, seed=self.seed, step=step, out=b['act'][sl])[0]

    def _loss_grad(self, b, w):
        """-> (grad, td, stats[4] device sums of {w * td, Q(s)[a], sum_i z_i m_i, td} over the minibatch, a* or None)."""
        return self.policy.loss_grad(self.target, b['obs'], b['action'], b['reward'], b['done'], b['next_obs'],
                                     b['next_mask'] if self.masked else None, weights=w, gamma_n=self.gamma_n, double_q=self.double_q,
                                     grad_out=self.grad, td_out=self._td, want_next_action=self.keep_last_batch)

    def _values(self, tok, mean_reward, s):
        """``DQNTrainer``'s and mean_target, the mean of the projected target distribution."""
        return dict(DQNTrainer._values(self, tok, mean_reward, s), mean_target=float(s[2]) / max(tok['rows'], 1))


class RawDQNTrainer(DQNTrainer):
    """``DQNTrainer`` on the raw features - the driver's ``DQN_rawstate`` (script/modelfree_train.py:55-56,63-66,106-133: the DQN
    settings on mask_model_rawstate) - for an env with config['rawstate_as_obs'] (+ support_rllib_mask, return_tensors), beside
    ``RawStateTrainer``.  The network is the raw-state encoder of ``DeviceRawTrainer``; its Q values are the masked logits.

    Every step's observation is packed into one record of ``policy.record_words`` 32-bit words ([dense | cat ids | sequence ids],
    ``rl4rs_rawstate_pack``), so the rollout buffer and the replay ring are ``DQNTrainer``'s with obs_dim = REC; the loss reads the
    sampled records in place (``rl4rs_rawtrain_dqn_loss_grad``), the gradient stays in the handle, Adam clips each of the ten
    variables by its own norm, and the target is a torch copy of the flat parameters (both 100000 x 128 tables included: 104 MB at
    the default configuration).  Arguments and defaults are ``DQNTrainer``'s without ``hidden``; ``weights`` defaults to
    ``init_rawpolicy_weights(cfg, seed=init_seed)``.  Schedule and statistics are ``DQNTrainer``'s.

    Not here: data-parallel training (the sparse table exchange of ``RawStateTrainer`` is not wired to this learner) and
    ``save`` / ``restore`` (``_Checkpoint`` covers the flat policy networks only, see ``RawStateTrainer``)."""

    def __init__(self, env, seed=0, init_seed=0, lr=5e-4, gamma=1.0, adam_eps=1e-8, grad_clip=40.0, double_q=True, n_step=1,
                 buffer_size=100000, target_network_update_freq=200, learning_starts=1000, train_batch_size=None,
                 prioritized_replay=True, prioritized_replay_alpha=0.6, prioritized_replay_beta=0.4, softq_temperature=1.0,
                 updates_per_rollout=1, keep_last_batch=False, weights=None):
        from .nets.rawpolicy import init_rawpolicy_weights
        cfg = env.config
        assert cfg.get('return_tensors', False) and cfg.get('rawstate_as_obs', False) and cfg.get('support_rllib_mask', False), \
            "RawDQNTrainer needs config rawstate_as_obs + support_rllib_mask + return_tensors"
        if rdist.collectives_active():
            raise NotImplementedError("RawDQNTrainer is single-process: the sparse exchange of the two embedding tables' gradients "
                                      "(RawStateTrainer's) is not wired to this learner, and a dense all-reduce of 25.9 M floats per "
                                      "update is not offered in its place")
        self._weights = weights if weights is not None else init_rawpolicy_weights(cfg, seed=init_seed)
        self.S = cfg['seq_num']
        DQNTrainer.__init__(self, env, seed=seed, init_seed=init_seed, lr=lr, gamma=gamma, adam_eps=adam_eps, grad_clip=grad_clip,
                            double_q=double_q, n_step=n_step, buffer_size=buffer_size, target_network_update_freq=target_network_update_freq,
                            learning_starts=learning_starts, train_batch_size=train_batch_size, prioritized_replay=prioritized_replay,
                            prioritized_replay_alpha=prioritized_replay_alpha, prioritized_replay_beta=prioritized_replay_beta,
                            softq_temperature=softq_temperature, updates_per_rollout=updates_per_rollout, keep_last_batch=keep_last_batch)
        del self._weights
        self._raw = None

    def _obs_dim(self, env):
        c = env.config
        return (c['dense_feature_num'] + c['category_feature_num'] + c['seq_num'] * c['maxlen'] + 3) // 4 * 4

    def _make_net(self, hidden, init_seed):
        self.policy = D.DeviceRawTrainer(self.env.config, self._weights, max_rows=max(self.M, self.B))
        assert self.policy.record_words == self.OD

    def _new_grad(self):
        return None                                         # the handle's own flat gradient buffer

    def save(self, path):
        raise NotImplementedError("RawDQNTrainer has no checkpoints: _Checkpoint covers the trainers of the flat policy networks only "
                                  "(this one's two embedding tables are 100 MB of parameters, three times that with Adam's moments)")

    restore = save

    def sync_replicas(self, src=0):
        raise NotImplementedError("RawDQNTrainer is single-process")

    def _episode(self, explore, step0, reset_file=False):
        """``_ReplayTrainer._episode`` with every step's raw features packed into the observation rows of the rollout buffer."""
        B, T = self.B, self.T
        b = self.buf
        obs = self.env.reset(reset_file=True) if reset_file else self.env.reset()
        for t in range(T):
            sl = slice(t * B, (t + 1) * B)
            mask = self._step_mask(sl)
            self._raw = (obs['category_feature'], obs['dense_feature'], [q.contiguous() for q in obs['sequence_feature']])
            self.policy.pack_records(*self._raw, out=b['obs'][sl])
            a = self._act(explore, sl, mask, t, step0 + t)
            obs, reward, done, info = self.env.step(a)
            b['rew'][sl] = reward
        self._raw = None
        return b['rew'].view(T, B).sum(dim=0).mean()

    def _act(self, explore, sl, mask, t, step):
        """SoftQ at temperature 1 (the net's own categorical draw over the masked logits), or the greedy action."""
        cat, dense, seqs = self._raw
        if not explore:
            return self.policy.greedy(cat, dense, seqs, mask, out=self.buf['act'][sl])[0]
        a = self.policy.act(cat, dense, seqs, mask, seed=self.seed, step=step)[0]
        self.buf['act'][sl] = a
        return a

    def _loss_grad(self, b, w):
        td, stats, astar = self.policy.dqn_loss_grad(self.target, b['obs'], b['action'], b['reward'], b['done'], b['next_obs'], b['next_mask'],
                                                     weights=w, gamma=self.gamma, double_q=self.double_q, td_out=self._td,
                                                     want_next_action=self.keep_last_batch)
        return None, td, stats, astar

    def _adam_step(self, g):
        self.policy.adam_step_clip_by_var(lr=self.lr, eps=self.adam_eps, var_clip=self.grad_clip)


# ---- TD3 / DDPG -----------------------------------------------------------------------------------------------------------------
# What the reference's merged config makes of RLlib 1.5.1's TD3 / DDPG defaults (script/modelfree_train.py:79-105): every value is a
# constructor argument of TD3Trainer, None = the preset of its ``algo``.
TD3_PRESETS = {
    'TD3': dict(twin_q=True, policy_delay=2, smooth_target_policy=True, target_noise=0.2, target_noise_clip=0.5, tau=5e-3, l2_reg=0.0,
                buffer_size=1000000, prioritized_replay=False, learning_starts=10000, random_timesteps=10000),
    'DDPG': dict(twin_q=False, policy_delay=1, smooth_target_policy=False, target_noise=0.2, target_noise_clip=0.5, tau=2e-3, l2_reg=1e-6,
                 buffer_size=50000, prioritized_replay=True, learning_starts=1500, random_timesteps=1000),
}


def ou_scale(timestep, random_timesteps=0, initial_scale=1.0, final_scale=0.02, scale_timesteps=10000):
    """RLlib's exploration scale (GaussianNoise / OrnsteinUhlenbeckNoise: PiecewiseSchedule from (random_timesteps, initial_scale) to
    (random_timesteps + scale_timesteps, final_scale), final_scale outside): linear in the sampled timestep."""
    t = float(timestep) - float(random_timesteps)
    if t < 0.0 or t >= scale_timesteps:
        return float(final_scale)
    return float(initial_scale) + (float(final_scale) - float(initial_scale)) * t / float(scale_timesteps)


class TD3Learner(object):
    """The networks and one update of TD3 / DDPG on minibatches the caller supplies (``TD3Trainer`` feeds it from its replay ring):
    actor / critics as ``DeviceAMLP`` with RLlib's ddpg_tf_model shapes, their targets, and ``update`` = rl4rs_td3_update on a single
    process (``one_call``) or the same sequence as per-phase calls with the data-parallel all-reduce in front of the one Adam launch.
    ``params``: optional dict name -> DeviceAMLP parameter dict for actor, actor_targ, q1, q1_targ (and q2, q2_targ), replacing
    ``init_ddpg_params(seed=init_seed ...)`` and the target = online copy (tests)."""

    def __init__(self, obs_dim, act_dim, batch_size, twin_q=True, smooth_target_policy=True, target_noise=0.2, target_noise_clip=0.5,
                 tau=5e-3, l2_reg=0.0, gamma=1.0, actor_lr=1e-3, critic_lr=1e-3, use_huber=False, huber_threshold=1.0,
                 actor_hiddens=(400, 300), critic_hiddens=(400, 300), init_seed=0, max_act_rows=0, params=None, device=None):
        from .offline_rl import init_ddpg_params
        if len(actor_hiddens) != 2 or len(critic_hiddens) != 2:
            raise ValueError('TD3Learner: actor_hiddens / critic_hiddens are two layers each')
        self.OD, self.E, self.M = int(obs_dim), int(act_dim), int(batch_size)
        self.twin_q, self.smooth = bool(twin_q), bool(smooth_target_policy)
        self.target_noise, self.target_noise_clip = float(target_noise), float(target_noise_clip)
        self.tau, self.l2_reg, self.gamma = float(tau), float(l2_reg), float(gamma)
        self.actor_lr, self.critic_lr = float(actor_lr), float(critic_lr)
        self.use_huber, self.huber_threshold = bool(use_huber), float(huber_threshold)
        OD, E, M = self.OD, self.E, self.M
        ah, ch = [int(x) for x in actor_hiddens], [int(x) for x in critic_hiddens]
        params = params or {}

        def actor(name, grad_rows):
            prm = params.get(name) or init_ddpg_params(OD, 0, E, ah[0], ah[1], seed=init_seed)
            return D.DeviceAMLP(OD, 0, E, prm, hidden1=ah[0], hidden2=ah[1], head_act='tanh', max_rows=max(M, int(max_act_rows)),
                                max_grad_rows=grad_rows, device=device)

        def critic(name, k, grad_rows):
            prm = params.get(name) or init_ddpg_params(OD, E, 1, ch[0], ch[1], seed=init_seed + 1 + k)
            return D.DeviceAMLP(OD, E, 1, prm, hidden1=ch[0], hidden2=ch[1], max_rows=M, max_grad_rows=grad_rows, device=device)

        self.actor, self.actor_targ = actor('actor', M), actor('actor_targ', 0)
        self.q1, self.q1_targ = critic('q1', 0, M), critic('q1_targ', 0, 0)
        self.q2, self.q2_targ = (critic('q2', 1, M), critic('q2_targ', 1, 0)) if self.twin_q else (None, None)
        self.critics = [self.q1, self.q2] if self.twin_q else [self.q1]
        self.critic_targs = [self.q1_targ, self.q2_targ] if self.twin_q else [self.q1_targ]
        self.named = [('actor', self.actor), ('actor_targ', self.actor_targ), ('q1', self.q1), ('q1_targ', self.q1_targ)]
        if self.twin_q:
            self.named += [('q2', self.q2), ('q2_targ', self.q2_targ)]
        dev = self.device = self.actor.device
        self.td = torch.empty(M, dtype=torch.float32, device=dev)
        self.metrics = torch.zeros(6, dtype=torch.float32, device=dev)
        self._ws = torch.empty(int(self.actor.lib.rl4rs_td3_workspace_floats(M, E)), dtype=torch.float32, device=dev)
        self._minus_inv_m = torch.full((M, 1), float(np.float32(-1.0) / np.float32(M)), dtype=torch.float32, device=dev)
        self.one_call = True             # update() as one library call on a single rank (False: the per-phase calls; tests compare the two)

    def sync_replicas(self, src=0):
        """Data parallel: every rank's online parameters become those of rank ``src`` (the Adam state is still zero)."""
        for net in [self.actor] + self.critics:
            p = net.flat_params()
            rdist.broadcast_(p, src)
            net.set_flat_params(p)

    def sync_targets(self):
        self.actor_targ.copy_from(self.actor)
        for t, s in zip(self.critic_targs, self.critics):
            t.copy_from(s)

    def flat_params(self):
        """dict name -> flat float32 parameters of every network (actor, actor_targ, q1, q1_targ and, with twin_q, q2, q2_targ)."""
        return dict((name, net.flat_params()) for name, net in self.named)

    def close(self):
        for _, net in self.named:
            net.close()

    def _update_one_call(self, b, noise, weights, do_actor):
        from . import _lib
        import ctypes as C
        h = lambda net: (net.h.value if net is not None else None)
        p = lambda t: (t.data_ptr() if t is not None else None)
        st = _lib.Td3Step(h(self.actor), h(self.actor_targ), h(self.q1), h(self.q2), h(self.q1_targ), h(self.q2_targ), self.M, self.E,
                          self.gamma, self.tau, self.actor_lr, self.critic_lr, self.target_noise, self.target_noise_clip, self.l2_reg,
                          self.huber_threshold, 1 if self.smooth else 0, 1 if self.use_huber else 0, 1 if do_actor else 0, 0,
                          p(b['obs']), p(b['action']), p(b['reward']), p(b['done']), p(b['next_obs']), p(weights), p(noise), p(self._ws),
                          p(self.td), p(self.metrics))
        _lib.check(self.actor.lib.rl4rs_td3_update(C.byref(st), D._stream()))

    def _update_phases(self, b, noise, weights, do_actor):
        """The sequence of rl4rs_td3_update as per-phase calls, with the all-reduce of the data-parallel learner in front of Adam."""
        from .offline_rl import _allreduce_group
        obs, act, nxt = b['obs'], b['action'], b['next_obs']
        a_next = self.actor_targ.forward(nxt)
        if self.smooth:
            D.td3_smooth_action(a_next, noise, self.target_noise, self.target_noise_clip, out=a_next)
        qn = D.amlp_forward_multi(self.critic_targs, nxt, a_next)
        qv = D.amlp_forward_multi(self.critics, obs, act)
        twin = self.twin_q
        r = D.td3_critic_loss(qv[0], qv[1] if twin else None, qn[0], qn[1] if twin else None, b['reward'], b['done'], weights=weights,
                              gamma=self.gamma, use_huber=self.use_huber, huber_threshold=self.huber_threshold, td_out=self.td,
                              stats_out=self.metrics[:4])
        D.amlp_backward_multi(self.critics, obs, act, [r['dq1'], r['dq2']] if twin else [r['dq1']])
        for q in self.critics:
            D.amlp_add_l2(q, self.l2_reg)
        if do_actor:
            a_pi = self.actor.forward(obs)
            q_pi = self.q1.forward(obs, a_pi)
            da = self.q1.backward(obs, a_pi, self._minus_inv_m, want_dact=True, want_param_grad=False)
            self.actor.backward(obs, None, D.tanh_head_grad(a_pi, da))
            D.amlp_add_l2(self.actor, self.l2_reg)
            self.metrics[4] = -q_pi.sum()
        _allreduce_group(self.critics + ([self.actor] if do_actor else []))
        D.amlp_adam_multi(self.critics + [self.actor], [self.critic_lr] * len(self.critics) + [self.actor_lr],
                          targets=self.critic_targs + [self.actor_targ], tau=self.tau, step=[True] * len(self.critics) + [do_actor],
                          eps=1e-7)

    def update(self, batch, noise=None, weights=None, do_actor=True):
        """One update on ``batch`` (dict obs, action, reward, done int32, next_obs: float32 device tensors of ``batch_size`` rows),
        ``noise`` [M, E] N(0, 1) for the target smoothing, ``weights`` [M] or None.  -> the metrics buffer float[6] = sums of
        {w * error, q1, y, |td1|}, -sum q1(s, pi(s)) of the last actor step, spare; ``self.td`` holds the first critic's TD errors."""
        M, E = self.M, self.E
        for k, shape, dt in (('obs', (M, self.OD), torch.float32), ('next_obs', (M, self.OD), torch.float32), ('action', (M, E), torch.float32),
                             ('reward', (M,), torch.float32), ('done', (M,), torch.int32)):
            t = batch[k]
            assert t.is_cuda and t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous(), (k, t.dtype, tuple(t.shape))
        if self.smooth:
            assert noise is not None and noise.is_cuda and noise.dtype == torch.float32 and tuple(noise.shape) == (M, E) and noise.is_contiguous()
        if weights is not None:
            assert weights.is_cuda and weights.dtype == torch.float32 and tuple(weights.shape) == (M,) and weights.is_contiguous()
        if self.one_call and not rdist.collectives_active():
            self._update_one_call(batch, noise, weights, do_actor)
        else:
            self._update_phases(batch, noise, weights, do_actor)
        return self.metrics


class TD3Trainer(_ReplayTrainer):
    """Online TD3 / DDPG over the zero-copy continuous-action env (``support_conti_env``, plain 256-wide observations): the third
    learner family of script/modelfree_train.py (:46-48, :79-105; modelfree_trainer.py:25-28).  The action is the 32-d vector in
    Box(-1, 1) that the env resolves with its masked K-NN.  Defaults are the reference's merged RLlib 1.5.1 configuration
    (``TD3_PRESETS`` by ``algo``; common: gamma 1, actor_lr = critic_lr = 1e-3, use_huber False, n_step 1, train_batch_size
    min(B * T, 1024), OU theta 0.15 / sigma 0.2 / ou_base_scale 0.1, scale 1.0 -> 0.02 over 10 000 sampled steps, Adam eps 1e-7).
    The reference driver's own DDPG branch raises (an ``if`` in front of a separate if / elif / else chain); ``algo='DDPG'`` here is
    TD3 with twin_q, policy_delay and smooth_target_policy off.  RLlib parity is unpinned (ray is absent), as for A2C / PPO / DQN.

    One rollout is actor forward -> OU exploration -> env.step for T steps; then the push; then ``updates_per_rollout`` updates once
    ``learning_starts`` sampled steps are reached, ``do_actor = num_updates % policy_delay == 0``.  All three targets move on every
    update (target_network_update_freq 0).  Networks and update are ``TD3Learner``'s (``self.learner``): ONE library call
    (rl4rs_td3_update) on a single process; with ``torch.distributed`` initialised the same sequence as per-phase calls, the
    gradients of the critics and the actor mean-all-reduced together before the one Adam launch.

    Deviations from RLlib: the replay ring holds whole rollouts (max(1, buffer_size // (B * T)) of them); the OU state is one [E]
    vector PER ENV (RLlib: one variable shaped like a single action), never reset between episodes."""

    _columns = ('obs', 'act', 'rew')

    def __init__(self, env, algo='TD3', actor_hiddens=(400, 300), critic_hiddens=(400, 300), seed=0, init_seed=0, actor_lr=1e-3,
                 critic_lr=1e-3, gamma=1.0, twin_q=None, policy_delay=None, smooth_target_policy=None, target_noise=None,
                 target_noise_clip=None, tau=None, l2_reg=None, use_huber=False, huber_threshold=1.0, n_step=1, buffer_size=None,
                 prioritized_replay=None, prioritized_replay_alpha=0.6, prioritized_replay_beta=0.4, learning_starts=None,
                 random_timesteps=None, train_batch_size=None, ou_theta=0.15, ou_sigma=0.2, ou_base_scale=0.1, initial_scale=1.0,
                 final_scale=0.02, scale_timesteps=10000, updates_per_rollout=1, keep_last_batch=False):
        if algo not in TD3_PRESETS:
            raise ValueError("TD3Trainer: algo must be 'TD3' or 'DDPG'; got %r" % (algo,))
        if n_step != 1:
            raise ValueError("TD3Trainer implements n_step = 1 (the reference's setting); got %r" % (n_step,))
        cfg = env.config
        _require_env(cfg, "TD3Trainer needs the zero-copy continuous-action env (config['return_tensors'] and ['support_conti_env'] = True)",
                     conti=True)
        pre = dict(TD3_PRESETS[algo])
        given = dict(twin_q=twin_q, policy_delay=policy_delay, smooth_target_policy=smooth_target_policy, target_noise=target_noise,
                     target_noise_clip=target_noise_clip, tau=tau, l2_reg=l2_reg, buffer_size=buffer_size,
                     prioritized_replay=prioritized_replay, learning_starts=learning_starts, random_timesteps=random_timesteps)
        pre.update((k, v) for k, v in given.items() if v is not None)
        self._init_loop(env, seed, train_batch_size, pre['learning_starts'], updates_per_rollout, pre['prioritized_replay'],
                        prioritized_replay_beta, keep_last_batch)
        self.algo, self.E = algo, cfg['action_emb_size']
        self.policy_delay, self.buffer_size, self.random_timesteps = int(pre['policy_delay']), int(pre['buffer_size']), int(pre['random_timesteps'])
        self.ou_theta, self.ou_sigma, self.ou_base_scale = float(ou_theta), float(ou_sigma), float(ou_base_scale)
        self.initial_scale, self.final_scale, self.scale_timesteps = float(initial_scale), float(final_scale), int(scale_timesteps)
        OD, E, M = self.OD, self.E, self.M
        self.learner = TD3Learner(OD, E, M, twin_q=pre['twin_q'], smooth_target_policy=pre['smooth_target_policy'],
                                  target_noise=pre['target_noise'], target_noise_clip=pre['target_noise_clip'], tau=pre['tau'],
                                  l2_reg=pre['l2_reg'], gamma=gamma, actor_lr=actor_lr, critic_lr=critic_lr, use_huber=use_huber,
                                  huber_threshold=huber_threshold, actor_hiddens=actor_hiddens, critic_hiddens=critic_hiddens,
                                  init_seed=init_seed, max_act_rows=self.B)
        self.actor = self.learner.actor
        dev = self.device = self.actor.device
        self._new_replay = lambda: D.DeviceContiReplay(OD, E, self.T, self.B, buffer_size=self.buffer_size, alpha=prioritized_replay_alpha,
                                                       device=dev)
        self.replay = self._new_replay()
        self._owned = (self.learner, self.replay)
        N = self.B * self.T
        self.buf = dict(obs=torch.empty((N, OD), dtype=torch.float32, device=dev), act=torch.empty((N, E), dtype=torch.float32, device=dev),
                        rew=torch.empty(N, dtype=torch.float64, device=dev))
        self._det = torch.empty((self.B, E), dtype=torch.float32, device=dev)
        self.ou_state = torch.zeros((self.B, E), dtype=torch.float32, device=dev)
        self._batch = self.replay.new_batch(M)
        self._gen = torch.Generator(device=dev)
        self._gen.manual_seed(int(seed) * 7919 + 17)
        if rdist.collectives_active():
            self.learner.sync_replicas(0)                   # replicas start identical (shared init_seed; the Adam state is zero)
        self.learner.sync_targets()

    def params(self):
        """dict name -> flat float32 parameters of every network (``TD3Learner.flat_params``)."""
        self._settle()
        return self.learner.flat_params()

    def _ckpt_nets(self):
        """actor, critics (with their Adam state) and the targets (parameters only)"""
        return [(name, net, not name.endswith('_targ')) for name, net in self.learner.named]

    def _ckpt_tensors(self):
        return {'ou_state': self.ou_state}              # the annealed scale reads ``timesteps``, which is host state

    def _ckpt_extra(self):
        return {'noise_generator': self._gen.get_state()}           # the target-smoothing noise stream

    def _ckpt_set_extra(self, extra):
        self._gen.set_state(torch.from_numpy(extra['noise_generator']))

    def sync_replicas(self, src=0):
        self.learner.sync_replicas(src)

    def scale_at(self, timestep):
        """ou_base_scale x the annealed scale at a sampled timestep: the ``scale`` of rl4rs_explore_ou, computed on the host."""
        return self.ou_base_scale * ou_scale(timestep, self.random_timesteps, self.initial_scale, self.final_scale, self.scale_timesteps)

    def _act(self, explore, sl, mask, t, step):
        """The actor's own action; exploring: plus OU noise, or uniformly random during the first ``random_timesteps``."""
        b = self.buf
        a = b['act'][sl]
        if explore:
            ts = self.timesteps + t * self.B
            random_phase = ts < self.random_timesteps
            if not random_phase:
                self.actor.forward(b['obs'][sl], out=self._det)
            D.explore_ou(self._det, self.ou_state, self.ou_theta, self.ou_sigma, self.scale_at(ts), seed=self.seed, step=step,
                         random_phase=random_phase, out=a)
        else:
            self.actor.forward(b['obs'][sl], out=a)
        return a

    def update(self):
        """One learner step: sample -> ``TD3Learner.update`` -> priorities.  -> the learner's metrics buffer."""
        M, L = self.M, self.learner
        b = self._sample()
        noise = torch.randn((M, self.E), generator=self._gen, device=self.device, dtype=torch.float32) if L.smooth else None
        do_actor = self.num_updates % self.policy_delay == 0
        if self.keep_last_batch:
            self._keep(b)
            self.last_batch.update(noise=noise.clone() if noise is not None else None, do_actor=do_actor)
        L.update(b, noise=noise, weights=b['weight'] if self.prioritized else None, do_actor=do_actor)
        if self.prioritized:
            self.replay.update_priorities(b['idx'], L.td)
        if self.keep_last_batch:
            self.last_batch['td'] = L.td.clone()
        self.num_updates += 1
        return L.metrics

    def _stats0(self):
        return self.learner.metrics

    def _extras(self, trained):
        return dict(rows=self.M)

    def _values(self, tok, mean_reward, s):
        """episode_reward_mean; critic_loss, mean_q, mean_td_abs of the last update and actor_loss of the last actor step, without the
        L2 terms, 0 before the first; buffer_rows, num_updates (and iteration)."""
        n = float(tok['rows'])
        return {'episode_reward_mean': mean_reward, 'critic_loss': float(s[0]) / n, 'actor_loss': float(s[4]) / n, 'mean_q': float(s[1]) / n,
                'mean_td_abs': float(s[3]) / n, 'buffer_rows': tok['buffer_rows'], 'num_updates': tok['num_updates']}


class ExactKTrainer(_Evaluated):
    """Exact-K (script/exact_k_train.py, rl4rs/nets/exact_k) over the zero-copy discrete ``SlateRecEnv-v0`` (T = 9): the pointer-network
    generator emits the whole 9-item slate from the first observation, REINFORCE with the critic's prediction of the batch reward as
    baseline and a hill climb over ``samples`` sampled slates per user.  Defaults are the reference's: hidden_units 64, 4 heads,
    2 blocks, dropout 0.1 (on in every pass, greedy evaluation included: the reference builds its generator with is_training=True
    for its eval stage too), Adam lr 1e-3 (generator) / 5e-3 (critic) with beta2 0.98.  TF parity is unpinned (TensorFlow 1.15 is
    absent).

    One ``train_iteration`` is the reference's episode (exact_k_train.py:72-114): reset and keep obs0; per climb decode a sampled
    slate from obs0, play its 9 actions and keep the last step's reward (the episode reward on this env); per row keep the climb with
    the larger reward (ties: the first); baseline = critic(obs0) BEFORE the critic's update toward the kept reward; advantage =
    (reward - baseline) / its population std; generator update with w = advantage on the kept paths.

    Deviations: (1) ``same_users=True`` (default) replays the SAME batch of users for every climb (the record cursor and the global
    numpy RNG state are saved before the first reset and restored before the later ones).  The reference calls env.reset() between
    its two climbs and keeps the old observation, so its second slate is scored on different users than it was generated for;
    ``same_users=False`` is the reference as written.  (2) A batch whose advantage has zero or non-finite std skips the generator
    update (the reference would divide by zero); the decision is a device flag that gates the Adam step, counted in the statistics
    (``skipped``, ``skipped_total``).

    ``eval_mode='beam'`` evaluates beam 0 of ``DeviceExactK.decode_beam(beam_size=...)`` in place of the greedy slate, at the same
    (seed, step); training is the same in both modes.

    No ``save`` / ``restore`` yet: ``_Checkpoint`` covers the learners of script/modelfree_train.py.  The reference's Exact-K script
    does checkpoint (a tf.train.Saver, exact_k_train.py:118-132); here the generator's and the critic's parameters and Adam state are
    read with ``policy.params()`` / ``adam_state()``."""

    def __init__(self, env, seed=0, init_seed=0, lr=1e-3, critic_lr=5e-3, dropout_rate=0.1, samples=2, same_users=True, hidden_units=64,
                 num_heads=4, num_blocks=2, vocab=500, critic_hidden=128, temperature=1, num_glimpse=1, num_layers=1, use_mha=True,
                 eval_mode='greedy', beam_size=3):
        cfg = env.config
        if eval_mode not in ('greedy', 'beam'):
            raise ValueError("eval_mode must be 'greedy' or 'beam'; got %r" % (eval_mode,))
        if not 1 <= int(beam_size) <= D.DeviceExactK.BEAM_MAX:
            raise ValueError('beam_size must be in [1, %d]; got %r' % (D.DeviceExactK.BEAM_MAX, beam_size))
        self.eval_mode, self.beam_size = eval_mode, int(beam_size)
        if getattr(getattr(env, 'samples', None), 'is_seq', False) or cfg['max_steps'] != D.DeviceExactK.SLATE:
            raise ValueError("ExactKTrainer runs SlateRecEnv-v0 (max_steps 9) only: on SeqSlateRecEnv-v0 the reference script indexes its "
                             "9-wide slate with 36 steps and cannot run either")
        _require_env(cfg, "ExactKTrainer needs the zero-copy discrete-action env (config['return_tensors'] = True, no conti env)",
                     error=ValueError)
        for name, val, want in (('temperature', temperature, 1), ('num_glimpse', num_glimpse, 1), ('num_layers', num_layers, 1),
                                ('use_mha', bool(use_mha), True)):
            if val != want:
                raise ValueError('ExactKTrainer implements %s = %r (the reference default); got %r' % (name, want, val))
        if int(samples) < 1:
            raise ValueError('samples must be >= 1')
        if rdist.collectives_active():
            raise RuntimeError('ExactKTrainer is single-process: data-parallel training is out of scope')
        self.env = env
        self.B, self.T, self.A = cfg['batch_size'], cfg['max_steps'], cfg['action_size']
        self.seed, self.lr, self.critic_lr = seed, float(lr), float(critic_lr)
        self.samples, self.same_users = int(samples), bool(same_users)
        self._pending = []
        self.OD = _obs_width(env)
        catalog = env.samples._catalog
        self.policy = D.DeviceExactK(catalog.location_mask[:3], catalog.is_special, max_rows=self.B, obs_dim=self.OD, action_size=self.A,
                                     hidden_units=hidden_units, num_heads=num_heads, num_blocks=num_blocks, vocab=max(vocab, self.A),
                                     dropout_rate=dropout_rate, seed=init_seed)
        self.device = self.policy.device
        self.critic = D.DeviceExactKCritic(self.B, obs_dim=self.OD, hidden=critic_hidden, seed=init_seed + 1, device=self.device)
        self._owned = (self.policy, self.critic)
        self.iteration = 0
        self._decodes = 0
        self.skipped_total = 0
        self.last = None                   # the last iteration (tests): rewards [samples, B], paths, the kept ones, every climb's env state

    def params(self):
        self._settle()
        return self.policy.params()

    def _obs(self, obs):
        obs = obs['obs'] if isinstance(obs, dict) else obs
        return obs.to(torch.float32).contiguous()

    def _play(self, path):
        """The 9 actions of every row's slate -> the last step's reward [B] float32."""
        cols = path.t().contiguous()
        reward = None
        for t in range(self.T):
            _, reward, _, _ = self.env.step(cols[t])
        return reward.to(torch.float32).reshape(-1)

    @staticmethod
    def select_best(rewards, paths):
        """Per row the climb with the larger reward, ties to the first: rewards [S, B], paths [S, B, 9] -> (reward [B], path [B, 9])."""
        best_r, best_p = rewards[0], paths[0]
        for s in range(1, rewards.shape[0]):
            better = rewards[s] > best_r
            best_r = torch.where(better, rewards[s], best_r)
            best_p = torch.where(better[:, None], paths[s], best_p)
        return best_r.contiguous(), best_p.contiguous()

    @staticmethod
    def normalise_advantage(reward, baseline):
        """(reward - baseline) / its population std -> (w [B] float32, skip int32 [1]): skip = 1 (and w = 0) when the std is 0 or not
        finite.  Device tensors in, device tensors out, nothing waits."""
        adv = reward - baseline
        sd = adv.std(unbiased=False)
        bad = ~torch.isfinite(sd) | (sd == 0)
        w = torch.where(bad, torch.zeros_like(adv), adv / torch.where(bad, torch.ones_like(sd), sd))
        return w.to(torch.float32).contiguous(), bad.to(torch.int32).reshape(1)

    def train_iteration(self):
        """One episode of the reference's loop.  Returns a ``LazyStats`` mapping (episode_reward_mean of the kept slates,
        reward_first_climb, baseline_mean, critic_loss, policy_loss, invalid_targets, skipped, skipped_total, iteration); nothing here
        waits for the GPU."""
        data = self.env.sim._recData
        saved = (data._cursor, np.random.get_state()) if self.same_users else None
        obs0 = self._obs(self.env.reset()).clone()
        rewards, paths, states = [], [], []
        for s in range(self.samples):
            if s > 0 and self.same_users:
                data._cursor = saved[0]
                np.random.set_state(saved[1])
                self.env.reset()
            path, _ = self.policy.decode(obs0, greedy=False, seed=self.seed, step=self._decodes)
            self._decodes += 1
            states.append(self.env.samples)        # (its .user is read lazily on the host: tests only)
            rewards.append(self._play(path))
            paths.append(path)
            if not self.same_users:
                self.env.reset()                   # exact_k_train.py:85: the next climb (and nothing else) sees this batch
        self._settle()
        rewards, paths = torch.stack(rewards), torch.stack(paths)
        reward, path = self.select_best(rewards, paths)
        baseline, err = self.critic.loss_grad(obs0, reward)
        self.critic.adam_step(lr=self.critic_lr)
        w, skip = self.normalise_advantage(reward, baseline)
        stats, _ = self.policy.loss_grad(obs0, path, w, seed=self.seed, step=self.iteration)
        self.policy.adam_step(lr=self.lr, skip=skip)
        self.iteration += 1
        self.last = dict(rewards=rewards, paths=paths, reward=reward, path=path, baseline=baseline, weights=w, states=states, obs0=obs0)
        vec = torch.stack([rewards[0].mean(), baseline.mean(), err.mean(), stats[0], stats[1], skip[0].to(torch.float32)])
        return self._submit(reward.mean(), vec)

    def _values(self, tok, mean_reward, s):
        self.skipped_total += int(s[5] != 0)
        return {'episode_reward_mean': mean_reward, 'reward_first_climb': float(s[0]), 'baseline_mean': float(s[1]),
                'critic_loss': float(s[2]), 'policy_loss': float(s[3]), 'invalid_targets': int(s[4]), 'skipped': int(s[5] != 0),
                'skipped_total': self.skipped_total}

    def _eval_batch(self, k):
        """One batch of greedy slates (``eval_mode='beam'``: the best of ``beam_size`` beams); dropout stays on (as in the reference's
        eval stage) with a fixed mask stream."""
        obs0 = self._obs(self.env.reset(reset_file=True) if k == 0 else self.env.reset())
        if self.eval_mode == 'beam':
            path = self.policy.decode_beam(obs0, beam_size=self.beam_size, seed=self.seed, step=k)[0][:, 0].contiguous()
        else:
            path, _ = self.policy.decode(obs0, greedy=True, seed=self.seed, step=k)
        return self._play(path).to(torch.float64).mean()
