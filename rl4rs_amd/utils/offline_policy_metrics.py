"""Off-policy estimators of the reference (rl4rs/utils/offline_policy_metrics.py:47-184) on the device: same names, argument
order and ``(value, second)`` return pairs (python floats).

    eval_IPS / eval_CIPS / eval_SNIPS(rewards [B], policy_prob [B], behavior_prob [B])   -> (E_t, confidence half-width)
    eval_doubly_robust(action_rhat_rewards [B], state_rewards [B], rewards [B], policy_prob [B], behavior_prob [B])
                                                                                        -> (mean(dr) / mean(rewards), sem(dr))
    eval_WIPS(step_rewards [B, T], policy_prob [B, T], behavior_prob [B, T], gamma=1.0)  -> (value, 0)
    eval_seq_doubly_robust(action_rhat_rewards [B, T], state_rewards [B, T], rewards [B, T], policy_prob, behavior_prob)
                                                                                        -> (value, 0)

Inputs are numpy arrays (or anything ``np.asarray`` takes) or device tensors of any float dtype; they are widened to float64 and
ALL arithmetic is float64 (``rl4rs_ope_episode_stats`` / ``rl4rs_ope_step_stats``: per-episode terms one lane per episode,
fixed-order reductions, two-pass variances, the t quantile on the host - no scipy).  The reference's result depends on the dtype
numpy happens to be handed (float32 probabilities give a float32 ``cumprod``): that accident is deliberately NOT reproduced.
Reproduced as they are: ``_calc_sequential_weigths`` divides the clipped running product by the batch size and clips again to
[0.1, 10] (so for a large batch every weight sits on 0.1 and WIPS is 1); SNIPS takes its point estimate from the clipped ratios;
the confidence widths use ``int(n_e)``; ``int(n_e) - 1 <= 0`` gives NaN like ``scipy.stats.t.ppf``.  Where the reference raises
(``int`` of a NaN / infinite effective sample size) the width here is NaN.
There is no CPU path: the functions need the GPU."""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from .._lib import OPE_STATS, check

def _shape(x):
    return tuple(x.shape) if hasattr(x, 'shape') else tuple(np.asarray(x).shape)


def _check_shapes(ndim, required, optional):
    """the arrays of one call agree in shape; checked before a device is looked for"""
    shape = _shape(required[0])
    if len(shape) != ndim or any(n < 1 for n in shape):
        raise ValueError('expected a non-empty %d-d array, got shape %r' % (ndim, shape))
    for x in list(required[1:]) + [x for x in optional if x is not None]:
        if _shape(x) != shape:
            raise ValueError('mismatched shapes: %r and %r' % (shape, _shape(x)))
    return shape


def _f64(x, device):
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        return x.detach().to(device=device, dtype=torch.float64).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64))).to(device)


def _device(*xs):
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    _lib.require_device()
    return torch.device('cuda', torch.cuda.current_device())


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def episode_stats(rewards, policy_prob, behavior_prob, action_rhat_rewards=None, state_rewards=None):
    """All per-episode statistics (dict keyed by ``_lib.OPE_STATS``) in one call."""
    (B,) = _check_shapes(1, (rewards, policy_prob, behavior_prob), (action_rhat_rewards, state_rewards))
    lib = _lib.load()
    dev = _device(rewards, policy_prob, behavior_prob)
    r, pp, bp, a, s = (_f64(x, dev) for x in (rewards, policy_prob, behavior_prob, action_rhat_rewards, state_rewards))
    out = (C.c_double * len(OPE_STATS))()
    with torch.cuda.device(dev):
        check(lib.rl4rs_ope_episode_stats(B, _ptr(r), _ptr(pp), _ptr(bp), _ptr(a), _ptr(s), out, _stream(dev)))
    return dict(zip(OPE_STATS, [float(v) for v in out]))


def step_stats(step_rewards, policy_prob, behavior_prob, action_rhat_rewards=None, state_rewards=None, gamma=1.0):
    """All per-step statistics (WIPS, SeqDR) in one call."""
    B, T = _check_shapes(2, (step_rewards, policy_prob, behavior_prob), (action_rhat_rewards, state_rewards))
    lib = _lib.load()
    dev = _device(step_rewards, policy_prob, behavior_prob)
    r, pp, bp, a, s = (_f64(x, dev) for x in (step_rewards, policy_prob, behavior_prob, action_rhat_rewards, state_rewards))
    out = (C.c_double * len(OPE_STATS))()
    with torch.cuda.device(dev):
        check(lib.rl4rs_ope_step_stats(B, T, _ptr(r), _ptr(pp), _ptr(bp), _ptr(a), _ptr(s), float(gamma), out, _stream(dev)))
    return dict(zip(OPE_STATS, [float(v) for v in out]))


def eval_DM(policy, obs):
    return policy(obs)


def eval_IPS(rewards, policy_prob, behavior_prob):
    s = episode_stats(rewards, policy_prob, behavior_prob)
    return s['ips'], s['ips_c']


def eval_CIPS(rewards, policy_prob, behavior_prob):
    s = episode_stats(rewards, policy_prob, behavior_prob)
    return s['cips'], s['cips_c']


def eval_SNIPS(rewards, policy_prob, behavior_prob):
    s = episode_stats(rewards, policy_prob, behavior_prob)
    return s['snips'], s['snips_c']


def eval_WIPS(step_rewards, policy_prob, behavior_prob, gamma=1.0):
    s = step_stats(step_rewards, policy_prob, behavior_prob, gamma=gamma)
    return s['wips'], s['wips_2']


def eval_doubly_robust(action_rhat_rewards, state_rewards, rewards, policy_prob, behavior_prob):
    s = episode_stats(rewards, policy_prob, behavior_prob, action_rhat_rewards, state_rewards)
    return s['dr'], s['dr_se']


def eval_seq_doubly_robust(action_rhat_rewards, state_rewards, rewards, policy_prob, behavior_prob):
    s = step_stats(rewards, policy_prob, behavior_prob, action_rhat_rewards, state_rewards)
    return s['seqdr'], s['seqdr_2']


def student_t_ppf(p, df):
    """``scipy.stats.t.ppf(p, df)`` from the library's host code (needs no device)."""
    return float(_lib.load().rl4rs_student_t_ppf(float(p), float(df)))
