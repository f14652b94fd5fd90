"""Off-policy evaluation of a trained policy against the logs: ``ope_eval`` of the reference
(script/offline_evaluation.py:9-73, called from batchrl_train.py:132-147 and modelfree_train.py:500-514) on the device.

    from rl4rs_amd.ope import ope_eval
    from rl4rs.policy.behavior_model import behavior_model
    result = ope_eval(config, eval_env, algo, sample_model=behavior_model(config, bc))

The loop is the reference's: per epoch ``reset``, then ``max_steps`` times ``predict_with_mask`` -> (``action_probs`` of the
logged action, ``predict_q`` of the chosen one, the behaviour model's probability of the logged action) -> ``step``, collecting
the simulator's reward and ``offline_reward``.  What differs is where the numbers live: every per-step column goes into the
``[T, B]`` float64 log of an ``OpeLog`` (``rl4rs_ope_*``) - the propensities straight from the score matrices by the gather
kernels - and one epoch's four estimators are one ``rl4rs_ope_estimate``: with a device env (``return_tensors``) and a device
learner nothing is copied to the host inside an epoch but that call's vector of statistics.

Reproduced quirks: the simulator's summed reward is DR's ``action_rhat_rewards`` and the per-episode mean Q its
``state_rewards``; the per-episode propensities are products of ``probs * 100``; ``layer = j // 3 + 1`` and
``page = j // page_items`` go to the behaviour model; ``sample_model=None`` collects rewards only (the metrics are empty)."""
import ctypes as C
import warnings

import numpy as np
import torch

from . import _lib
from . import device as D
from . import offline_rl as R
from ._lib import OPE_COLS, OPE_STATS, check
from .policy.policy_model import policy_model


class OpeLog(object):
    """``rl4rs_ope`` handle: the per-step log of one epoch (``[T, B]`` float64 columns pi, mu, q, reward, logged_reward) and
    its estimators."""

    def __init__(self, max_batch, max_steps, device=None):
        self.lib = _lib.load()
        self.h = C.c_void_p()
        _lib.require_device()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        with torch.cuda.device(self.device):
            check(self.lib.rl4rs_ope_create(int(max_batch), int(max_steps), C.byref(self.h)))
        self.B = self.T = 0
        self._zeros = None

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def begin(self, B, T):
        check(self.lib.rl4rs_ope_begin(self.h, int(B), int(T)))
        self.B, self.T = int(B), int(T)

    def _scores(self, scores, action):
        if isinstance(scores, torch.Tensor) and scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 2 and scores.stride(1) == 1:
            s = scores.to(self.device)                    # rows of a wider matrix are read in place (row stride = ld)
        else:
            s = D._dev_tensor(scores, torch.float32, self.device)
        a = D.to_device_async(action, torch.int32, self.device).reshape(-1)
        if s.dim() != 2 or s.shape[0] != self.B or a.shape[0] != self.B:
            raise ValueError('scores %r / actions %r do not fit the epoch\'s batch size %d' % (tuple(s.shape), tuple(a.shape), self.B))
        return s, a

    def record_policy(self, t, scores, action, logits):
        s, a = self._scores(scores, action)
        check(self.lib.rl4rs_ope_record_policy(self.h, int(t), D._ptr(s), s.shape[1], s.stride(0), D._ptr(a), int(bool(logits)), self._stream()))

    def record_behavior(self, t, scores, lo, hi, action, logits):
        s, a = self._scores(scores, action)
        check(self.lib.rl4rs_ope_record_behavior(self.h, int(t), D._ptr(s), s.shape[1], s.stride(0), int(lo), int(hi), D._ptr(a),
                                                 int(bool(logits)), self._stream()))

    def record_q(self, t, scores, action):
        s, a = self._scores(scores, action)
        check(self.lib.rl4rs_ope_record_q(self.h, int(t), D._ptr(s), s.shape[1], s.stride(0), D._ptr(a), self._stream()))

    def _step_address(self, t, col):
        """device address of step ``t`` of one column (rl4rs_ope_log + t * B)"""
        if not 0 <= int(t) < self.T:
            raise ValueError('step %d outside the epoch\'s [0, %d)' % (t, self.T))
        p, n = C.c_void_p(), C.c_int64()
        check(self.lib.rl4rs_ope_log(self.h, OPE_COLS[col], C.byref(p), C.byref(n)))
        return int(p.value) + int(t) * self.B * 8

    def _mark(self, t):
        for col in ('pi', 'q'):
            check(self.lib.rl4rs_ope_mark_recorded(self.h, int(t), OPE_COLS[col]))

    def record_step(self, t, policy_handle, obs, mask_bits, logged_action, q_mode, actions_out=None, masked_out=None):
        """One OPE step of a mask-model handle (``DevicePolicy.ope_step``: two GEMMs and one row launch): writes pi[t] =
        softmax(masked logits)[logged_action] and q[t] (``q_mode`` 1: the masked Q of the greedy action, 0: the value head) in place
        and returns the greedy actions (int32 [B] device tensor)."""
        a = D.to_device_async(logged_action, torch.int32, self.device).reshape(-1)
        if obs.shape[0] != self.B or a.shape[0] != self.B:
            raise ValueError('observations %r / actions %r do not fit the epoch\'s batch size %d' % (tuple(obs.shape), tuple(a.shape), self.B))
        out = policy_handle.ope_step(obs, mask_bits, a, q_mode, pi=self._step_address(t, 'pi'), q=self._step_address(t, 'q'),
                                     actions_out=actions_out, masked_out=masked_out)[0]
        self._mark(t)
        return out

    def record_scores_step(self, t, scores, logged_action, mask_bits=None, mask_set=0, value=None, actions_out=None, masked_out=None):
        """The same step from a score matrix (``device.ope_greedy_rows``): ``scores`` float32 [B, A] (rows of a wider device matrix are
        read in place), ``value`` float32 [B] or None (q[t] is then the masked score of the greedy action)."""
        s, a = self._scores(scores, logged_action)
        out = D.ope_greedy_rows(s, a, mask_bits=mask_bits, mask_set=mask_set, value=value, pi=self._step_address(t, 'pi'),
                                q=self._step_address(t, 'q'), actions_out=actions_out, masked_out=masked_out)[0]
        self._mark(t)
        return out

    def record_column(self, t, col, values):
        """one [B] column of step ``t`` from a device tensor (float32 / float64 as they are) or host data"""
        if _is_zero_list(values, self.B):
            if self._zeros is None or self._zeros.shape[0] < self.B:
                self._zeros = torch.zeros(self.B, dtype=torch.float64, device=self.device)
            v = self._zeros[:self.B]
        elif isinstance(values, torch.Tensor) and values.is_cuda and values.dtype in (torch.float32, torch.float64):
            v = values.to(self.device).reshape(-1).contiguous()
        elif isinstance(values, torch.Tensor) and values.is_cuda:
            v = values.to(device=self.device, dtype=torch.float64).reshape(-1).contiguous()
        else:
            v = D.to_device_async(values, torch.float64, self.device).reshape(-1)
        if v.shape[0] != self.B:
            raise ValueError('column of %d values, the epoch has %d episodes' % (v.shape[0], self.B))
        check(self.lib.rl4rs_ope_record_column(self.h, int(t), OPE_COLS[col], D._ptr(v), int(v.dtype == torch.float64), self._stream()))

    def column(self, col):
        """a copy of one column's log, float64 [T, B] device tensor"""
        p, n = C.c_void_p(), C.c_int64()
        check(self.lib.rl4rs_ope_log(self.h, OPE_COLS[col], C.byref(p), C.byref(n)))
        out = torch.empty((self.T, self.B), dtype=torch.float64, device=self.device)
        check(self.lib.rl4rs_copy_d2d(D._ptr(out), p, n.value * 8, self._stream()))
        return out

    def estimate(self, gamma=1.0):
        """dict of the statistics vector (``_lib.OPE_STATS``): the one read-back of an epoch"""
        out = (C.c_double * len(OPE_STATS))()
        check(self.lib.rl4rs_ope_estimate(self.h, float(gamma), out, self._stream()))
        return dict(zip(OPE_STATS, [float(v) for v in out]))

    def close(self):
        if self.h:
            self.lib.rl4rs_ope_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _is_zero_list(values, n):
    """the python list ``[0] * B`` the envs hand out as ``offline_reward`` before the last step (slate.py:164-166): it is not
    converted and uploaded, a device column of zeros stands in (not timed on its own)"""
    return type(values) is list and len(values) == n and values.count(0) == n


def _q_learner(policy):
    """the learner behind a ``policy_model`` of this package when its scores are the Q values of one device network"""
    m = getattr(policy, 'policy', None)
    if isinstance(policy, policy_model) and isinstance(m, R._QLearner) and getattr(m, 'reward_scaler', None) is None:
        return m
    return None


def ope_eval(config, eval_env, algo, sample_model=None, on_epoch=None):
    """script/offline_evaluation.py:9-73.  ``eval_env``: anything with ``reset`` / ``step`` / ``offline_action`` /
    ``offline_reward`` / ``samples.records``; ``algo``: a learner of ``offline_rl``, an online trainer of ``train`` (``Trainer``,
    ``DQNTrainer``, ``RainbowTrainer`` - the ope stage of modelfree_train.py:498-514; wrapped in ``policy_model(algo, config,
    env=eval_env)``, and with a device observation every step is one ``OpeLog.record_step``) or a ``policy_model`` (anything with
    ``predict_with_mask`` / ``action_probs`` / ``predict_q``); ``sample_model``: a ``behavior_model`` (anything with
    ``action_probs(record, action, layer, page=)``; one whose ``takes_observation`` is true is handed the observation the policy's network
    receives (``obs['obs']`` of a mask-mode dict) instead of ``eval_env.samples.records``) or None.

    Prints the reference's lines and returns what it only prints: ``dict(metrics [epoch, 4, 2] (IS, DR, WIPS, SeqDR) x (value,
    second), mean, std (over the epochs), episode_reward (mean simulated episode reward), stats (per epoch, every statistic))``.
    ``on_epoch(epoch, log, actions, offline_actions)``, when given, is called after each epoch's estimate with the ``OpeLog`` (its
    columns still hold the epoch: ``log.column(name)``) and the per-step chosen / logged actions as the loop held them."""
    if config.get('support_conti_env', False):
        raise ValueError("ope_eval: config['support_conti_env'] - a continuous-action policy has no probability of the logged item "
                         "(action_probs indexes a [B, action_size] matrix with offline_action, offline_evaluation.py:27-28)")
    learner = getattr(algo, 'policy', algo)
    if sample_model is not None and isinstance(learner, R.DiscreteBC):
        raise ValueError("ope_eval: DiscreteBC has no predict_value, so the evaluated policy's Q values (DR / SeqDR state rewards, "
                         "offline_evaluation.py:29) do not exist; evaluate a DiscreteBCQ / DiscreteCQL, or pass sample_model=None")
    from . import train as T
    if hasattr(algo, 'predict_with_mask'):
        policy = algo
    elif isinstance(algo, (T.Trainer, T.DQNTrainer)):
        # the model-free driver's ope stage (modelfree_train.py:498-514): the trainer's greedy policy under the env's own mask
        policy = policy_model(algo, config, env=eval_env)
    else:
        env_ok = hasattr(getattr(eval_env, 'samples', None), '_live')
        policy = policy_model(algo, config, env=eval_env if env_ok and 'iteminfo_file' not in config else None)
    epoch, batch_size, max_steps = int(config['epoch']), int(config['batch_size']), int(config['max_steps'])
    page_items = config.get('page_items', 9)
    qlearner = _q_learner(policy)
    scores = getattr(policy, '_scores', None) if isinstance(policy, policy_model) else None      # an online trainer's
    log = OpeLog(batch_size, max_steps)
    metrics, stats = [], []
    try:
        for i in range(epoch):
            obs = eval_env.reset()
            log.begin(batch_size, max_steps)
            print('test batch at ', i)
            actions, off_actions = [], []
            for j in range(max_steps):
                fused = qlearner is not None and sample_model is not None and isinstance(obs, torch.Tensor) and obs.is_cuda
                obs_2d = obs['obs'] if isinstance(obs, dict) else obs           # what the policy's network receives
                step = (scores is not None and sample_model is not None and isinstance(obs_2d, torch.Tensor) and obs_2d.is_cuda
                        and obs_2d.shape[0] <= scores.handle.max_rows)
                if step:
                    # an online trainer: its forward, the masked arg-max, pi and q of this step are one record_step
                    off_action = eval_env.offline_action
                    action = scores.record_step(log, j, *scores.split(obs), off_action).to(torch.int64)
                elif fused:
                    # one forward of the Q network serves the masked arg-max, pi (fused softmax gather) and Q(s, a)
                    x = policy._obs(obs)
                    qmat = policy._chunks(qlearner.q, x)
                    action = policy._handle().predict_with_mask(torch.softmax(qmat, dim=1), x[:, -policy.mask_size:]).to(torch.int64)
                else:
                    action = policy.predict_with_mask(obs)
                if not step:
                    off_action = eval_env.offline_action
                if sample_model is not None:
                    if fused:
                        log.record_policy(j, qmat, off_action, logits=True)
                        log.record_q(j, qmat, action)
                    elif not step:
                        log.record_policy(j, policy.action_probs(obs), off_action, logits=False)
                        log.record_column(j, 'q', policy.predict_q(obs, action))
                    layer, page = j // 3 + 1, j // page_items
                    record = obs_2d if getattr(sample_model, 'takes_observation', False) else eval_env.samples.records
                    if hasattr(sample_model, 'record_into'):
                        sample_model.record_into(log, j, record, off_action, layer)
                    else:
                        log.record_column(j, 'mu', sample_model.action_probs(record, off_action, layer, page=page))
                if on_epoch is not None:
                    actions.append(action)
                    off_actions.append(off_action)
                obs, reward, done, info = eval_env.step(action)
                log.record_column(j, 'logged_reward', eval_env.offline_reward)
                log.record_column(j, 'reward', reward)
            s = log.estimate()
            stats.append(s)
            if on_epoch is not None:
                on_epoch(i, log, actions, off_actions)
            if sample_model is not None:
                metrics.append(((s['cips'], s['cips_c']), (s['dr'], s['dr_se']), (s['wips'], s['wips_2']), (s['seqdr'], s['seqdr_2'])))
    finally:
        log.close()
    m = np.array(metrics, dtype=np.float64).reshape(len(metrics), 4, 2)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                 # sample_model=None: the mean of no epochs is NaN, as the reference prints
        mean = np.average(m, axis=0) if len(m) else np.full((4, 2), np.nan)
        std = np.std(m, axis=0) if len(m) else np.full((4, 2), np.nan)
    print('IS', 'DR', 'WIPS', 'SeqDR', sep=' ')
    print(mean)
    print(std)
    return dict(metrics=m, mean=mean, std=std, episode_reward=float(np.mean([s['sim_reward'] for s in stats])), stats=stats)
