"""Offline scorers on the device: d3rlpy 0.91's ``metrics/scorer.py`` and the reference's ``rl4rs/utils/d3rlpy_scorer.py`` over
evaluation episodes, as ONE pass.

    episodes = episodes_from_mdp(dataset)                         # offline.generate_offline_dataset's dict
    evaluate_scorers(algo, episodes[-3000:], ['td_error', 'soft_opc', 'discrete_action_match'], return_threshold=90)

Every network runs once per transition row; ``rl4rs_score_rows`` reads each score row once and writes the few scalars every
scorer needs (the columns below); ``rl4rs_score_episodes`` - one lane per episode, then a fixed-order float64 reduction - produces
all requested scores together, bit-identical from run to run.  Per transition i the columns are float32

    qd = Q(o_i, a_i)        qp = Q(o_i, pi(o_i))        qn = Q(o'_i, pi(o'_i))        r_raw = the next reward        ter
    r_td = r_raw through ``reward_scaler.transform`` when the learner has a fitted scaler

the integer actions ``a``, ``a_pi = predict(o)``, ``a_mask = predict_with_mask(o)`` and, for continuous actions, the float64
``diff = sum_k (a_k - predict(o)_k)^2``.  The scores (float64 arithmetic on those columns; gamma = the learner's):

    td_error                          mean (qd - (r_td + gamma qn (1 - ter)))^2
    discounted_sum_of_advantage       mean S; inside each episode and each window of 1024 consecutive transitions of it
                                      (d3rlpy's _make_batches, WINDOW_SIZE) S_last = adv_last, S_j = adv_j + gamma S_{j+1}, adv = qd - qp
    average_value_estimation          mean qp
    initial_state_value_estimation    mean over episodes of qp at the episode's first row
    soft_opc                          mean qd over rows of episodes with return >= threshold, minus mean qd; NaN when none succeeds
    discrete_action_match             mean [a_pi == a]                  (d3rlpy's)
    discrete_action_match_mask        mean [a_mask == a]                (the reference's: it asks policy_model.predict_with_mask)
    continuous_action_diff            mean diff

d3rlpy's ``value_estimation_std_scorer`` stays out: these learners keep no ensemble of Q functions whose std it reports.
The reference's ``soft_opc_scorer`` takes ``policy_model.predict_q``: given ``policy=``, qd goes through the scaler's
``reverse_transform`` in float32 exactly as ``predict_q`` does, before it enters the pass (the kernels carry no scaler arithmetic).
The mask rule runs on the learner's raw score row (Q values; the imitator's logits for ``DiscreteBC``) where ``predict_with_mask``
masks ``softmax`` of it: the same arg-max unless a Q value lies below the fill value -2^15 or float32 softmax merges two scores.
d3rlpy is absent here: the formulas are restated from the published 0.91 sources, parity unpinned."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from . import device as D
from . import offline_rl as R

NAMES = _lib.SCORE_STATS[:8]
_SLOT = {n: i for i, n in enumerate(_lib.SCORE_STATS)}
_NEEDS_Q = ('td_error', 'discounted_sum_of_advantage', 'average_value_estimation', 'initial_state_value_estimation', 'soft_opc')
WINDOW_SIZE = 1024


class EvalEpisodes(object):
    """Evaluation episodes as five transition columns on the device (``offline_rl.transitions_from_mdp``'s) and ``starts``: int64
    [E + 1] offsets, episode e = rows [starts[e], starts[e + 1]).  ``len()`` = E; ``episodes[a:b]`` is a view of a contiguous
    range of episodes (step 1 only)."""

    def __init__(self, obs, act, rew, nxt, ter, starts, discrete_action):
        self.observations, self.actions, self.next_rewards, self.next_observations, self.terminals = obs, act, rew, nxt, ter
        self._starts_host = np.ascontiguousarray(starts, dtype=np.int64)
        assert self._starts_host.ndim == 1 and self._starts_host.size >= 1 and self._starts_host[0] == 0
        assert int(self._starts_host[-1]) == obs.shape[0] and (np.diff(self._starts_host) > 0).all()
        self.starts = torch.from_numpy(self._starts_host).to(obs.device)
        self.discrete_action = bool(discrete_action)

    @property
    def device(self):
        return self.observations.device

    @property
    def n_rows(self):
        return int(self.observations.shape[0])

    def columns(self):
        return self.observations, self.actions, self.next_rewards, self.next_observations, self.terminals

    def __len__(self):
        return int(self._starts_host.size - 1)

    def __getitem__(self, key):
        if not isinstance(key, slice) or key.step not in (None, 1):
            raise TypeError('EvalEpisodes takes a contiguous slice of episodes (step 1), got %r' % (key,))
        a, b, _ = key.indices(len(self))
        b = max(a, b)
        lo, hi = int(self._starts_host[a]), int(self._starts_host[b])
        return EvalEpisodes(*[t[lo:hi] for t in self.columns()], self._starts_host[a:b + 1] - lo, self.discrete_action)

    def returns(self):
        """float64 [E]: the sum of each episode's next-rewards - d3rlpy 0.91's ``Episode.compute_return``, ``sum(rewards[1:])``."""
        lengths = torch.from_numpy(np.diff(self._starts_host)).to(self.device)
        if not len(self):
            return torch.zeros(0, dtype=torch.float64, device=self.device)
        return torch.segment_reduce(self.next_rewards.to(torch.float64), 'sum', lengths=lengths)


def episodes_from_mdp(data, discrete_action=None, device=None):
    """``EvalEpisodes`` of MDPDataset-style arrays (dict with 'observations', 'actions', 'rewards', 'terminals').  Transitions are
    exactly ``transitions_from_mdp``'s; an episode is a maximal run of them ending at ``terminal == 1``, or the trailing run; an
    episode left with no transition (a trailing single row) is dropped.  ``discrete_action`` None: integer actions, and a single
    action column, are discrete."""
    if discrete_action is None:
        a = data['actions']
        a = a if isinstance(a, torch.Tensor) else np.asarray(a)
        floating = a.dtype.is_floating_point if isinstance(a, torch.Tensor) else np.issubdtype(a.dtype, np.floating)
        discrete_action = not floating or a.ndim == 1 or a.shape[1] == 1      # ([N, 1] is how generate_offline_dataset stores item ids)
    tr = R.transitions_from_mdp(data['observations'], data['actions'], data['rewards'], data['terminals'], discrete_action=discrete_action)
    if device is None:
        device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')
    ter = tr[4].cpu().numpy()
    n = ter.shape[0]
    ends = (np.nonzero(ter > 0.5)[0] + 1).tolist()
    if n and (not ends or ends[-1] != n):
        ends.append(n)                                       # the trailing run without a terminal flag
    return EvalEpisodes(*[t.to(device).contiguous() for t in tr], np.asarray([0] + ends, dtype=np.int64), discrete_action)


# ---------------------------------------------------------------------------------------------------------------- device calls
def score_rows(scores, imitator=None, action_flexibility=0.3, logged=None, env=None, obs=None, want=('qd', 'a_pi', 'qp', 'a_mask'), out=None):
    """``rl4rs_score_rows`` on a float32 score matrix [N, A] (rows may be a view of a wider matrix): dict of the columns in ``want``
    - qd / qp float32 [N], a_pi / a_mask int32 [N].  ``imitator`` [N, A]: the BCQ rule; ``logged`` int32 [N] for qd; ``env`` (a
    ``DeviceEnv``) and ``obs`` [N, D] for a_mask.  ``out``: dict of contiguous [N] tensors to write into."""
    assert scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 2 and scores.stride(1) == 1
    N, A = scores.shape
    dev = scores.device
    res = {}
    for name in want:
        t = None if out is None else out.get(name)
        if t is None:
            t = torch.empty(N, dtype=torch.float32 if name in ('qd', 'qp') else torch.int32, device=dev)
        assert t.shape == (N,) and t.is_contiguous() and t.is_cuda and t.dtype == (torch.float32 if name in ('qd', 'qp') else torch.int32)
        res[name] = t
    if imitator is not None:
        assert imitator.is_cuda and imitator.dtype == torch.float32 and tuple(imitator.shape) == (N, A) and imitator.stride(1) == 1
    if 'qd' in res:
        assert logged is not None and logged.dtype == torch.int32 and logged.shape == (N,) and logged.is_contiguous() and logged.is_cuda
    if 'a_mask' in res:
        assert env is not None and obs is not None and obs.is_cuda and obs.dtype == torch.float32 and obs.dim() == 2 and obs.stride(1) == 1 \
            and obs.shape[0] == N
    with torch.cuda.device(dev):
        _lib.check(_lib.load().rl4rs_score_rows(
            N, D._ptr(scores), A, scores.stride(0) if N > 1 else A, D._ptr(imitator), (imitator.stride(0) if N > 1 else A) if imitator is not None else 0,
            float(action_flexibility), D._ptr(logged if 'qd' in res else None), env.h if 'a_mask' in res else None,
            D._ptr(obs if 'a_mask' in res else None), obs.shape[1] if 'a_mask' in res else 0,
            (obs.stride(0) if N > 1 else obs.shape[1]) if 'a_mask' in res else 0,
            D._ptr(res.get('qd')), D._ptr(res.get('a_pi')), D._ptr(res.get('qp')), D._ptr(res.get('a_mask')), D._stream()))
    return res


def action_diff(actions, predicted):
    """float64 [N]: sum_k (actions - predicted)^2 of two float32 [N, E] device tensors (``rl4rs_score_action_diff``)."""
    actions, predicted = actions.contiguous(), predicted.contiguous()
    assert actions.is_cuda and actions.dtype == torch.float32 and predicted.dtype == torch.float32 and actions.shape == predicted.shape
    out = torch.empty(actions.shape[0], dtype=torch.float64, device=actions.device)
    with torch.cuda.device(actions.device):
        _lib.check(_lib.load().rl4rs_score_action_diff(actions.shape[0], actions.shape[1], D._ptr(actions), D._ptr(predicted), D._ptr(out), D._stream()))
    return out


def score_episodes(starts, cols, gamma=1.0, return_threshold=None):
    """``rl4rs_score_episodes``: ``starts`` int64 [E + 1] device tensor, ``cols`` dict of device columns by the names of
    ``_lib.ScoreCols`` (float32; a / a_pi / a_mask int32; diff float64; missing = not supplied) -> dict of the eleven host floats
    of ``_lib.SCORE_STATS``.  A slot whose columns were not supplied is NaN."""
    assert starts.is_cuda and starts.dtype == torch.int64 and starts.dim() == 1 and starts.is_contiguous() and starts.numel() >= 2
    E = starts.numel() - 1
    rows = None
    c = _lib.ScoreCols()
    keep = []
    for name in _lib.ScoreCols.SCORE_COLS:
        t = cols.get(name)
        if t is None:
            continue
        want = torch.int32 if name in ('a', 'a_pi', 'a_mask') else (torch.float64 if name == 'diff' else torch.float32)
        t = t.reshape(-1).to(device=starts.device, dtype=want).contiguous()
        rows = t.numel() if rows is None else rows
        assert t.numel() == rows, 'column %r has %d rows, the others %d' % (name, t.numel(), rows)
        keep.append(t)
        setattr(c, name, t.data_ptr())
    assert rows, 'no column supplied'
    stats = (C.c_double * len(_lib.SCORE_STATS))()
    with torch.cuda.device(starts.device):
        _lib.check(_lib.load().rl4rs_score_episodes(E, D._ptr(starts), rows, C.byref(c), float(gamma), 0 if return_threshold is None else 1,
                                                    0.0 if return_threshold is None else float(return_threshold), stats, D._stream()))
    return dict(zip(_lib.SCORE_STATS, [float(x) for x in stats]))


# ---------------------------------------------------------------------------------------------------------------- the pass
def _scaler(algo):
    s = getattr(algo, 'reward_scaler', None)
    if isinstance(s, str):
        raise ValueError("reward_scaler=%r has not been fitted (fit_mdp fits a scaler given by name on its dataset)" % s)
    return s


def _eval_nets(algo, rows):
    """Evaluation-sized copies of a discrete learner's networks (a learner's own handles take ``batch_size`` rows per call), kept on
    the learner; their parameters are copied from the learner's at the start of every pass."""
    cache = algo.__dict__.setdefault('_scorer_nets', {})
    if cache.get('rows', 0) < rows:
        for net in cache.get('nets', {}).values():
            net.close()
        cache['rows'] = rows
        cache['nets'] = {name: algo._net(0, max_rows=rows) for name in ('q', 'imitator') if hasattr(algo, name)}
    for name, net in cache['nets'].items():
        net.copy_from(getattr(algo, name))
    return cache['nets']


def _discrete_columns(algo, ep, need, env, chunk_rows):
    obs, act, _, nxt, _ = ep.columns()
    n, dev = ep.n_rows, ep.device
    is_bc = isinstance(algo, R.DiscreteBC)
    if chunk_rows is None or chunk_rows <= algo.batch_size:
        nets = {name: getattr(algo, name) for name in ('q', 'imitator') if hasattr(algo, name)}
    else:
        nets = _eval_nets(algo, min(n, int(chunk_rows)))
    main = nets['imitator'] if is_bc else nets['q']
    imit = nets.get('imitator') if not is_bc else None                  # the BCQ rule
    flex = getattr(algo, 'action_flexibility', 0.3)
    cols = {'a': act.to(torch.int32).contiguous()}
    want = ['a_pi'] + (['qd', 'qp'] if not is_bc else []) + (['a_mask'] if 'a_mask' in need else [])
    for name in want + (['qn'] if 'qn' in need else []):
        cols[name] = torch.empty(n, dtype=torch.float32 if name in ('qd', 'qp', 'qn') else torch.int32, device=dev)
    R_ = main.max_rows
    for lo in range(0, n, R_):
        x = obs[lo:lo + R_].contiguous()
        hi = lo + x.shape[0]
        score_rows(main.forward(x), imit.forward(x) if imit is not None else None, flex, cols['a'][lo:hi], env, x, want,
                   out={k: cols[k][lo:hi] for k in want})
        if 'qn' in need:
            y = nxt[lo:lo + R_].contiguous()
            score_rows(main.forward(y), imit.forward(y) if imit is not None else None, flex, want=('qp',), out={'qp': cols['qn'][lo:hi]})
    for net in nets.values():
        net.check_status()
    return cols


def _continuous_columns(algo, ep, need, noise, noise_next):
    obs, act, _, nxt, _ = ep.columns()
    kw = (lambda z: {'noise': z} if z is not None else {}) if isinstance(algo, R.BCQ) else (lambda z: {})
    cols = {}
    if 'qd' in need:
        cols['qd'] = algo.predict_value(obs, act)
    if 'qp' in need or 'diff' in need:
        a_pred = algo.predict(obs, **kw(noise))
        if 'diff' in need:
            cols['diff'] = action_diff(act, a_pred)
        if 'qp' in need:
            cols['qp'] = algo.predict_value(obs, a_pred)
    if 'qn' in need:
        cols['qn'] = algo.predict_value(nxt, algo.predict(nxt, **kw(noise_next)))
    return cols


def _columns(algo, episodes, names, policy=None, noise=None, noise_next=None, chunk_rows=None):
    """The columns the names need, each network run once per row -> (dict for ``score_episodes``, qd reverse-transformed or None)"""
    names = set(names)
    discrete = isinstance(algo, R._Learner)
    if not discrete and not isinstance(algo, R._ContinuousLearner):
        raise TypeError('evaluate_scorers: %r is not one of this package\'s offline learners' % type(algo).__name__)
    if isinstance(algo, R.DiscreteBC) and names & set(_NEEDS_Q):
        raise TypeError('DiscreteBC has no Q function: %s cannot be scored' % ', '.join(sorted(names & set(_NEEDS_Q))))
    if discrete and 'continuous_action_diff' in names:
        raise TypeError('continuous_action_diff needs a continuous-action learner')
    if not discrete and names & {'discrete_action_match', 'discrete_action_match_mask'}:
        raise TypeError('discrete_action_match needs a discrete-action learner')
    if discrete != episodes.discrete_action:
        raise TypeError('the episodes hold %s actions, the learner takes the other kind' % ('discrete' if episodes.discrete_action else 'continuous'))
    need = set()
    if 'td_error' in names:
        need.add('qn')
    if names & {'td_error', 'discounted_sum_of_advantage', 'soft_opc'}:
        need.add('qd')
    if names & {'discounted_sum_of_advantage', 'average_value_estimation', 'initial_state_value_estimation'}:
        need.add('qp')
    if 'continuous_action_diff' in names:
        need.add('diff')
    env = None
    if 'discrete_action_match_mask' in names:
        need.add('a_mask')
        if policy is None:
            from .policy.policy_model import policy_model
            policy = algo.__dict__.get('_scorer_policy') or algo.__dict__.setdefault('_scorer_policy', policy_model(algo, algo.config))
        env = policy._handle()
    cols = _discrete_columns(algo, episodes, need, env, chunk_rows) if discrete else _continuous_columns(algo, episodes, need, noise, noise_next)
    scaler = _scaler(algo)
    cols['r_raw'] = episodes.next_rewards
    cols['r_td'] = scaler.transform(episodes.next_rewards) if scaler is not None else episodes.next_rewards
    cols['ter'] = episodes.terminals
    qd_rev = None
    if policy is not None and scaler is not None and 'qd' in cols:
        qd_rev = scaler.reverse_transform(cols['qd'])                  # float32, as policy_model.predict_q does it
    return cols, qd_rev


def _stats(episodes, cols, qd_rev, gamma, names, return_threshold):
    stats = score_episodes(episodes.starts, cols, gamma, return_threshold)
    if qd_rev is not None and 'soft_opc' in names:
        stats['soft_opc'] = score_episodes(episodes.starts, {'qd': qd_rev, 'r_raw': cols['r_raw']}, gamma, return_threshold)['soft_opc']
    return stats


def evaluate_scorers(algo, episodes, names, return_threshold=None, policy=None, noise=None, noise_next=None, chunk_rows=None):
    """Every score in ``names`` (``NAMES``) of ``algo`` on ``episodes`` from one pass -> dict of host floats.  Only the forwards the
    names need are run (Q(o', pi(o')) for ``td_error`` only, the mask rule for ``discrete_action_match_mask`` only).
    ``return_threshold``: soft_opc's.  ``policy``: the ``policy_model`` around ``algo`` - the reference's call convention: soft_opc then
    scores ``policy.predict_q``'s values (reverse-transformed where the learner has a reward scaler) and the mask rule uses the
    policy's env handle.  ``noise`` / ``noise_next``: ``BCQ.predict(obs, noise=)``'s draws for o and o'.  A name that needs Q on a
    ``DiscreteBC`` raises ``TypeError``.  ``chunk_rows`` (discrete learners): None = the learner's own handles, ``batch_size`` rows
    per forward - the values ``predict`` / ``predict_value`` give, bit for bit; a larger number = evaluation-sized copies of the
    networks kept on the learner (fewer, larger forwards; the GEMM picks its tiling by the row count, so last bits may differ)."""
    names = list(names)
    for n in names:
        if n not in NAMES:
            raise ValueError('unknown scorer %r (known: %s)' % (n, ', '.join(NAMES)))
    if 'soft_opc' in names and return_threshold is None:
        raise ValueError('soft_opc needs return_threshold')
    if not len(episodes):
        raise ValueError('no evaluation episodes')
    cols, qd_rev = _columns(algo, episodes, names, policy, noise, noise_next, chunk_rows)
    stats = _stats(episodes, cols, qd_rev, getattr(algo, 'gamma', 1.0), names, return_threshold)
    return {n: stats[n] for n in names}


# ---------------------------------------------------------------------------------------------------------------- callables
def _scorer(name, threshold=None, reference=False):
    def scorer(algo, episodes):
        if reference:                                        # (policy_model, episodes)
            return evaluate_scorers(algo.policy, episodes, [name], return_threshold=threshold, policy=algo)[name]
        return evaluate_scorers(algo, episodes, [name], return_threshold=threshold)[name]
    scorer._rl4rs_score = (name, threshold, bool(reference))
    scorer.__name__ = name + '_scorer'
    return scorer


td_error_scorer = _scorer('td_error')
discounted_sum_of_advantage_scorer = _scorer('discounted_sum_of_advantage')
average_value_estimation_scorer = _scorer('average_value_estimation')
initial_state_value_estimation_scorer = _scorer('initial_state_value_estimation')
discrete_action_match_scorer = _scorer('discrete_action_match')
continuous_action_diff_scorer = _scorer('continuous_action_diff')


def soft_opc_scorer(return_threshold):
    """d3rlpy's ``soft_opc_scorer(return_threshold)`` -> ``(algo, episodes) -> float``"""
    return _scorer('soft_opc', float(return_threshold))


def run_scorers(algo, episodes, scorers):
    """``{name: callable}`` as d3rlpy's ``fit(scorers=)`` takes it -> ``{name: float}``.  Callables of this module and of
    ``rl4rs_amd.utils.d3rlpy_scorer`` are recognised and evaluated together from ONE pass over the episodes; any other callable is
    called as ``f(algo, episodes)``."""
    out, known = {}, {}
    for key, f in scorers.items():
        tag = getattr(f, '_rl4rs_score', None)
        if tag is None or tag[0] not in NAMES:
            out[key] = float(f(algo, episodes))
        else:
            known[key] = tag
    if known:
        policy = None
        if any(ref for _, _, ref in known.values()):
            from .policy.policy_model import policy_model
            policy = algo.__dict__.get('_scorer_policy') or algo.__dict__.setdefault('_scorer_policy', policy_model(algo, algo.config))
        names = sorted({n for n, _, _ in known.values()})
        cols, qd_rev = _columns(algo, episodes, names, policy)
        by_form = {}
        for key, (name, thr, ref) in known.items():
            form = (thr if name == 'soft_opc' else None, ref and name == 'soft_opc')
            if form not in by_form:
                by_form[form] = _stats(episodes, cols, qd_rev if form[1] else None, getattr(algo, 'gamma', 1.0), names, form[0])
            out[key] = by_form[form][name]
    return {k: out[k] for k in scorers}


def d3rlpy_eval(eval_episodes, policy, soft_opc_score=90):
    """``batchrl_trainer.d3rlpy_eval`` (script/batchrl_trainer.py:377-392): the reference's action match for a ``DiscreteBC``, action
    match and soft OPC otherwise - one pass -> dict."""
    names = ['discrete_action_match_mask'] + ([] if isinstance(policy.policy, R.DiscreteBC) else ['soft_opc'])
    res = evaluate_scorers(policy.policy, eval_episodes, names, return_threshold=soft_opc_score, policy=policy)
    out = {'discrete_action_match': res['discrete_action_match_mask']}
    if 'soft_opc' in res:
        out['soft_opc'] = res['soft_opc']
    return out
