"""Thin object wrappers over the C-ABI handles of librl4rs_hip.so.

PyTorch is used for device memory and stream handles only (``tensor.data_ptr()``,
``torch.cuda.current_stream().cuda_stream``); all compute goes through the C ABI.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from ._lib import check

# rl4rs_env_buffer ids (include/rl4rs_hip.h)
BUF_PREV_ACTIONS, BUF_ACTION_MASK, BUF_SPECIAL_MASK, BUF_DENSE, BUF_CATEGORY, BUF_SEQ0, BUF_SEQ1, \
    BUF_C_DENSE, BUF_C_CATEGORY, BUF_ERROR_FLAG = range(10)
DIEN_ALL_FEATURE, DIEN_SCORES, DIEN_QUERY, DIEN_H1, DIEN_N_ACTIVE, DIEN_ROW_REP, DIEN_ROW_ACTIVE = range(7)
DIEN_H1_FRAG, DIEN_LEAD = 7, 8

_MASK_DTYPES = {torch.uint8: 0, torch.int32: 1, torch.int64: 2, torch.float32: 3}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _dev_tensor(x, dtype, device):
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(x)).to(device=device, dtype=dtype).contiguous()


def to_device_async(x, dtype, device):
    """Host data (list / ndarray / CPU tensor) -> device tensor of ``dtype`` through pinned memory, without draining the
    queue (a pageable ``.to(device)`` blocks until every queued kernel has finished); device tensors pass through."""
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return x.to(device=device, dtype=dtype).contiguous()
    np_dtype = {torch.int32: np.int32, torch.int64: np.int64, torch.float32: np.float32, torch.float64: np.float64}[dtype]
    if isinstance(x, list) and dtype == torch.int32 and x and type(x[0]) is int:
        import array                                # a python list of ints (what offline_action hands out): half the cost of np.asarray
        h = np.frombuffer(array.array('i', x), dtype=np.int32)
    else:
        h = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x
        h = np.ascontiguousarray(np.asarray(h), dtype=np_dtype)
    p = torch.empty(h.shape, dtype=dtype, device='cpu', pin_memory=True)       # caching host allocator: no page pinning per call
    p.numpy()[...] = h
    return p.to(device, non_blocking=True)


def wait_stream():
    """Wait for everything queued on the current stream.  (Measured on the bench box: polling an event from python instead of
    hipStreamSynchronize - to shave its wake-up latency off every reference-shaped step - was no faster: 15.24 -> 15.26 ms per
    episode-batch; the runtime's own wait already spins before it parks.)"""
    torch.cuda.current_stream().synchronize()


class OfflineActionList(list):
    """The python list ``offline_action`` hands out in the reference-shaped modes, remembering the device-side copy of the
    same ids (part of the last transition record): handed back to ``env.step`` unchanged - the reference's canonical replay
    loop - the ids never cross PCIe again.  Any in-place change drops the device reference, so a modified list is converted
    and uploaded like any other."""
    __slots__ = ('_dev', '_tag')

    def __init__(self, values, dev=None, tag=None):
        list.__init__(self, values)
        self._dev, self._tag = dev, tag

    def _drop(self):
        self._dev = None

    def __reduce__(self):                       # pickles / copies as the plain list it is
        return (list, (list(self),))


def _mutator(name):
    base = getattr(list, name)

    def f(self, *a, **k):
        self._drop()
        return base(self, *a, **k)
    f.__name__ = name
    return f


for _n in ('__setitem__', '__delitem__', '__iadd__', '__imul__', 'append', 'extend', 'insert', 'pop', 'remove', 'reverse', 'sort', 'clear'):
    setattr(OfflineActionList, _n, _mutator(_n))


def to_host(t):
    """Device tensor -> numpy array through ONE pinned staging block of torch's caching host allocator (a pageable ``.cpu()``
    goes through an internal bounce buffer at a fraction of the PCIe rate).  The array aliases the pinned block, which goes
    back to the allocator's cache when the array is released."""
    h = torch.empty(t.shape, dtype=t.dtype, device='cpu', pin_memory=True)
    h.copy_(t, non_blocking=True)
    wait_stream()
    return h.numpy()


class DeviceEnv(object):
    """rl4rs_env handle: SlateState / SeqSlateState device state for one batch."""

    def __init__(self, config, catalog, is_seq, log_steps, violation_zeroes_reward, device=None):
        _lib.require_device()
        self.lib = _lib.load()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.B = int(config['batch_size'])
        self.T = int(config['max_steps'])
        self.A = int(config['action_size'])
        self.E = int(catalog.action_emb.shape[1])
        self.P = int(config.get('page_items', 9))
        self.L = int(config['maxlen'])
        self.Dn = int(config['dense_feature_num'])
        self.Cn = int(config['category_feature_num'])
        self.W = (self.A + 31) // 32
        self.is_seq = bool(is_seq)
        self.log_steps = int(log_steps)
        cfg = _lib.EnvCfg(self.B, self.T, self.A, self.E, self.P, int(catalog.item_dim), 32, 10, self.L,
                          self.Dn, self.Cn, self.log_steps, 1 if is_seq else 0,
                          1 if violation_zeroes_reward else 0)
        self.user_dense_dim, self.user_cat_dim = 32, 10
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.rl4rs_env_create(C.byref(cfg), C.byref(h)))
            self.h = h
            loc = np.ascontiguousarray(catalog.location_mask.astype(np.uint8))
            check(self.lib.rl4rs_env_set_catalog(
                self.h, catalog.item_vec.ctypes.data_as(C.c_void_p), catalog.price.ctypes.data_as(C.c_void_p),
                catalog.action_emb.ctypes.data_as(C.c_void_p), catalog.is_special.ctypes.data_as(C.c_void_p),
                loc.ctypes.data_as(C.c_void_p), _stream()))
        self.n_complete = self.lib.rl4rs_env_complete_rows(self.h)
        self._keep = None
        if 'env_rows_variant' in config:                       # A/B runs: catalogue staged in LDS (0, default) or read through L1 / L2 (1)
            self.set_option('rows_variant', config['env_rows_variant'])

    def set_option(self, name, value):
        """Kernel-path selection of this handle (rl4rs_env_set_option)."""
        check(self.lib.rl4rs_env_set_option(self.h, _lib.ENV_OPTS[name], int(value)))

    def close(self):
        if getattr(self, 'h', None) is not None and self.h:
            self.lib.rl4rs_env_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------- batch / reset
    def load_batch(self, exposed, feedback, history, user_dense, user_cat):
        d = self.device
        ex = _dev_tensor(exposed, torch.int32, d)
        fb = _dev_tensor(feedback, torch.int32, d)
        hi = _dev_tensor(history, torch.int32, d)
        ud = _dev_tensor(user_dense, torch.float32, d)
        uc = _dev_tensor(user_cat, torch.int32, d)
        assert ex.shape == (self.B, self.log_steps) and fb.shape == ex.shape, (ex.shape, self.log_steps)
        assert hi.shape == (self.B, self.L) and ud.shape == (self.B, 32) and uc.shape == (self.B, 10)
        check(self.lib.rl4rs_env_load_batch(self.h, _ptr(ex), _ptr(fb), _ptr(hi), _ptr(ud), _ptr(uc), _stream()))
        self._keep = (ex, fb, hi, ud, uc)     # keep sources alive until the async copies ran

    def load_lines(self, tables, n_lines, line_idx, uniq_idx=None, hist_unique=None):
        """rl4rs_env_load_lines: the sampled lines of the resident log tables -> batch buffers + start-of-episode state, and the
        batch's distinct histories -> ``hist_unique`` (int32 [n_uniq, L]), in ONE launch.  ``tables``: dict of the LogStore's
        device tensors; ``line_idx`` / ``uniq_idx``: int32 device tensors."""
        assert line_idx.dtype == torch.int32 and line_idx.numel() == self.B and line_idx.is_contiguous()
        n_uniq = 0 if uniq_idx is None else int(uniq_idx.numel())
        if n_uniq:
            assert uniq_idx.dtype == torch.int32 and uniq_idx.is_contiguous()
            assert hist_unique.dtype == torch.int32 and tuple(hist_unique.shape) == (n_uniq, self.L) and hist_unique.is_contiguous()
        ex = tables['exposed']
        assert ex.shape[1] == self.log_steps and tables['history'].shape[1] == self.L
        check(self.lib.rl4rs_env_load_lines(self.h, _ptr(ex), _ptr(tables['feedback']), _ptr(tables['history']),
                                            _ptr(tables['user_dense']), _ptr(tables['user_cat']), int(n_lines), int(ex.shape[1]),
                                            _ptr(line_idx), _ptr(uniq_idx), n_uniq, _ptr(hist_unique), _stream()))
        self._keep = (line_idx, uniq_idx, hist_unique)

    def reset(self):
        check(self.lib.rl4rs_env_reset(self.h, _stream()))

    # ------------------------------------------------------------------------ act
    def act_discrete(self, actions):
        a = _dev_tensor(actions, torch.int32, self.device).reshape(-1)
        assert a.numel() == self.B, (a.shape, self.B)
        check(self.lib.rl4rs_env_act_discrete(self.h, _ptr(a), _stream()))
        return a

    def act_conti(self, actions):
        if isinstance(actions, torch.Tensor):
            a = actions.to(self.device)
            if a.dtype not in (torch.float32, torch.float64):
                a = a.to(torch.float64)
            a = a.contiguous()
        else:
            a = np.asarray(actions)
            a = a.astype(np.float32 if a.dtype == np.float32 else np.float64)
            a = torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        assert a.shape == (self.B, self.E), (a.shape, (self.B, self.E))
        chosen = torch.empty(self.B, dtype=torch.int32, device=self.device)
        check(self.lib.rl4rs_env_act_conti(self.h, _ptr(a), 1 if a.dtype == torch.float64 else 0,
                                           _ptr(chosen), _stream()))
        return chosen

    # -------------------------------------------------------------------- queries
    @property
    def cur_steps(self):
        return self.lib.rl4rs_env_cur_steps(self.h)

    def is_reward_step(self):
        return bool(self.lib.rl4rs_env_is_reward_step(self.h))

    def buffer_ptr(self, which):
        p = C.c_void_p()
        n = C.c_int64()
        check(self.lib.rl4rs_env_buffer(self.h, which, C.byref(p), C.byref(n)))
        return p, n.value

    def snapshot(self, which):
        """Copy an env-owned buffer into a fresh torch tensor (device)."""
        p, n = self.buffer_ptr(which)
        B, nc = self.B, self.n_complete
        shapes = {
            BUF_PREV_ACTIONS: ((B, self.T), torch.int32), BUF_ACTION_MASK: ((B, self.W), torch.int32),
            BUF_SPECIAL_MASK: ((B, self.W), torch.int32), BUF_DENSE: ((B, self.Dn), torch.float32),
            BUF_CATEGORY: ((B, self.Cn), torch.int32), BUF_SEQ0: ((B, self.L), torch.int32),
            BUF_SEQ1: ((B, self.L), torch.int32), BUF_C_DENSE: ((B * nc, self.Dn), torch.float32),
            BUF_C_CATEGORY: ((B * nc, self.Cn), torch.int32), BUF_ERROR_FLAG: ((1,), torch.int32),
        }
        shape, dt = shapes[which]
        out = torch.empty(shape, dtype=dt, device=self.device)
        assert out.numel() * out.element_size() == n, (which, shape, n)
        check(self.lib.rl4rs_copy_d2d(_ptr(out), p, n, _stream()))
        return out

    def bits_to_mask(self, bits):
        """uint32 bit rows [B,W] -> int64 [B,A] (numpy), the reference's mask layout."""
        b = bits.cpu().numpy().view(np.uint32)
        k = np.arange(self.A)
        return ((b[:, k >> 5] >> (k & 31).astype(np.uint32)) & 1).astype(np.int64)

    def build_complete(self, rows_per_env=None):
        if rows_per_env is None:
            check(self.lib.rl4rs_env_build_complete(self.h, _stream()))
        else:
            check(self.lib.rl4rs_env_build_complete_rows(self.h, rows_per_env, _stream()))

    def build_ahead_rows(self, n, partition=None):
        """-> (dense f32 [B * n, Dn], cat i32 [B * n, Cn]): the state rows of the act just taken and of the n - 1 acts behind it under
        the logged actions (rl4rs_env_build_ahead_rows).  ``partition`` = (rep i32 [B], active i32 [n_active], n_active
        i32 [1]) device tensors: also -> (rep, active [B], n_active [1]), the copy in which envs whose later logged actions part
        from their representative's stand for themselves."""
        dense = torch.empty((self.B * n, self.Dn), dtype=torch.float32, device=self.device)
        cat = torch.empty((self.B * n, self.Cn), dtype=torch.int32, device=self.device)
        if partition is None:
            check(self.lib.rl4rs_env_build_ahead_rows(self.h, n, _ptr(dense), _ptr(cat), None, None, None, None, None, None, _stream()))
            return dense, cat
        rep, active, cnt = partition
        assert all(t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() for t in partition) and rep.numel() == self.B
        out = (torch.empty(self.B, dtype=torch.int32, device=self.device), torch.full((self.B,), -1, dtype=torch.int32, device=self.device),
               torch.zeros(1, dtype=torch.int32, device=self.device))
        check(self.lib.rl4rs_env_build_ahead_rows(self.h, n, _ptr(dense), _ptr(cat), _ptr(rep), _ptr(active), _ptr(cnt), _ptr(out[0]),
                                                  _ptr(out[1]), _ptr(out[2]), _stream()))
        return dense, cat, out

    def reward(self, probs, p_last=None):
        out = torch.empty(self.B, dtype=torch.float64, device=self.device)
        m = self.n_complete - (1 if p_last is not None else 0)
        assert probs.dtype == torch.float32 and probs.numel() == self.B * m
        assert p_last is None or (p_last.dtype == torch.float32 and p_last.numel() == self.B)
        check(self.lib.rl4rs_env_reward_split(self.h, _ptr(probs), _ptr(p_last), _ptr(out), _stream()))
        return out

    def violation(self):
        out = torch.empty(self.B, dtype=torch.int32, device=self.device)
        check(self.lib.rl4rs_env_violation(self.h, _ptr(out), _stream()))
        return out

    def obs_mask(self, dtype=torch.int64):
        out = torch.empty((self.B, self.A), dtype=dtype, device=self.device)
        check(self.lib.rl4rs_env_obs_mask(self.h, _ptr(out), _MASK_DTYPES[dtype], _stream()))
        return out

    def obs_mask_bits(self, out=None):
        """The same mask packed 32 actions per int32 word, [B, (A + 31) // 32] - the ``mask_bits`` the policy kernels take
        (``out``: a contiguous int32 [B, W] tensor to fill, e.g. a slice of a rollout buffer)."""
        if out is None:
            out = torch.empty((self.B, (self.A + 31) // 32), dtype=torch.int32, device=self.device)
        assert out.dtype == torch.int32 and tuple(out.shape) == (self.B, (self.A + 31) // 32) and out.is_contiguous()
        check(self.lib.rl4rs_env_obs_mask(self.h, _ptr(out), 4, _stream()))
        return out

    def offline_action(self, conti=False):
        ids = torch.empty(self.B, dtype=torch.int32, device=self.device)
        emb = torch.empty((self.B, self.E), dtype=torch.float64, device=self.device) if conti else None
        check(self.lib.rl4rs_env_offline_action(self.h, _ptr(ids), _ptr(emb), _stream()))
        return emb if conti else ids

    def offline_reward(self):
        out = torch.empty(self.B, dtype=torch.float64, device=self.device)
        check(self.lib.rl4rs_env_offline_reward(self.h, _ptr(out), _stream()))
        return out

    def predict_with_mask(self, scores, obs_tail):
        """policy_model.predict_with_mask: scores [N,A] f32, obs_tail [N, P+1] = previous actions | cur_step."""
        scores = scores.to(device=self.device, dtype=torch.float32).contiguous()
        tail = obs_tail.to(device=self.device)
        prev = tail[:, :-1].to(torch.int32).contiguous()
        cur = tail[:, -1].to(torch.int32).contiguous()
        N = scores.shape[0]
        out = torch.empty(N, dtype=torch.int32, device=self.device)
        check(self.lib.rl4rs_env_predict_with_mask(self.h, N, _ptr(scores), _ptr(prev), prev.shape[1], _ptr(cur),
                                                   _ptr(out), _stream()))
        return out

    def check_error_flag(self):
        flag = int(self.snapshot(BUF_ERROR_FLAG).item())
        if flag:
            raise IndexError("an action id outside [0, action_size) was passed to act() "
                             "(numpy would raise at rl4rs/env/slate.py:199)")


def knn(actions, action_emb_dev, mask=None):
    """SlateState.get_nearest_neighbor(_with_mask) on device: actions [n,E] (f32/f64) -> int32 [n]."""
    lib = _lib.load()
    dev = action_emb_dev.device
    a = actions if isinstance(actions, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(actions)))
    if a.dtype not in (torch.float32, torch.float64):
        a = a.to(torch.float64)
    a = a.to(dev).contiguous()
    n, E = a.shape
    out = torch.empty(n, dtype=torch.int32, device=dev)
    m = None
    if mask is not None:
        m = (torch.as_tensor(np.asarray(mask) >= 0.5) if not isinstance(mask, torch.Tensor) else (mask >= 0.5))
        m = m.to(device=dev, dtype=torch.uint8).contiguous()
        assert m.shape == (n, action_emb_dev.shape[0])
    check(lib.rl4rs_knn(_ptr(a), 1 if a.dtype == torch.float64 else 0, n, _ptr(action_emb_dev),
                        action_emb_dev.shape[0], E, _ptr(m), _ptr(out), _stream()))
    return out


SCORER_MODES = {'auto': 0, 'fp32': 1, 'fp16x2': 2}       # include/rl4rs_hip.h RL4RS_SCORER_*
class DeviceStepper(object):
    """rl4rs_stepper handle: an env bound to its scorer so that one call runs a whole transition
    (rl4rs_env_step_discrete / rl4rs_env_step_conti = RecSimBase._step, base.py:157-170)."""

    def __init__(self, env, net, slots, act_tail=True, obs_fold=True, partition_carry=True, step_overlap=True, reset_lane=True,
                 reward_lane=True, replay_ahead=True, reward_beside=True):
        """``act_tail=False`` (config['no_act_tail'] / RL4RS_NO_ACT_TAIL=1): rl4rs_env_step_discrete launches k_step_tail as it
        did and leaves no next-step logged actions (rl4rs_stepper_set_act_tail).  ``obs_fold=False``
        (config['no_reward_obs_fold'] / RL4RS_NO_REWARD_OBS_FOLD=1): a reward step runs its observation forward and then the
        reward forward of n - 1 rows per env, as it did (rl4rs_stepper_set_obs_fold).  ``partition_carry=False``
        (config['no_partition_carry'] / RL4RS_NO_PARTITION_CARRY=1): every scorer forward of a transition looks for its duplicate
        rows itself, as it did (rl4rs_stepper_set_partition_carry).  ``step_overlap=False`` (config['no_step_overlap'] /
        RL4RS_NO_STEP_OVERLAP=1): every transition runs on the caller's stream (rl4rs_stepper_set_step_overlap).
        ``reset_lane=False`` (config['no_reset_lane'] / RL4RS_NO_RESET_LANE=1): ``observe`` takes no lane;
        ``reward_lane=False`` (config['no_reward_lane'] / RL4RS_NO_REWARD_LANE=1): every reward step joins.
        ``replay_ahead=False`` (config['no_replay_ahead'] / RL4RS_NO_REPLAY_AHEAD=1): no transition scores the rows of the ones behind
        it (rl4rs_stepper_set_replay_ahead); ``'pinned'`` (config['replay_ahead'] = 'pinned' / RL4RS_REPLAY_AHEAD=pinned):
        also where the 64-row form of the AUGRU launch is pinned and not chosen by the automatic rule (small batches).
        ``reward_beside=False`` (config['no_reward_beside'] / RL4RS_NO_REWARD_BESIDE=1): the reward step behind a replay-ahead forward
        runs on lane 0 behind it and the scorer's second scratch set stays observation-sized (rl4rs_stepper_set_reward_beside,
        DESIGN 42)."""
        self.lib = _lib.load()
        self.env, self.net, self.slots = env, net, slots          # keep the handles and the slot table alive
        assert slots.dtype == torch.int32 and slots.is_contiguous() and slots.shape[1] == env.B
        h = C.c_void_p()
        attach = self.lib.rl4rs_env_attach_simnet if isinstance(net, DeviceSimnet) else self.lib.rl4rs_env_attach_scorer
        check(attach(env.h, net.h, _ptr(slots), int(slots.shape[0]), C.byref(h)))
        self.h = h
        self.act_tail = bool(act_tail)
        if not self.act_tail:
            check(self.lib.rl4rs_stepper_set_act_tail(self.h, 0))
        if not obs_fold:
            check(self.lib.rl4rs_stepper_set_obs_fold(self.h, 0))
        if not partition_carry:
            check(self.lib.rl4rs_stepper_set_partition_carry(self.h, 0))
        if not step_overlap:
            check(self.lib.rl4rs_stepper_set_step_overlap(self.h, 0))
        if not reset_lane:
            check(self.lib.rl4rs_stepper_set_reset_lane(self.h, 0))
        if not reward_lane:
            check(self.lib.rl4rs_stepper_set_reward_lane(self.h, 0))
        if replay_ahead is not True:         # False: off; 'pinned': also where the 64-row AUGRU form is pinned, not chosen
            check(self.lib.rl4rs_stepper_set_replay_ahead(self.h, 2 if replay_ahead == 'pinned' else 0))
        if not reward_beside:
            check(self.lib.rl4rs_stepper_set_reward_beside(self.h, 0))
        self.reset_lane = bool(step_overlap and reset_lane)
        self._distinct_hint = None
        self.B, self.A, self.E, self.W, self.device = env.B, env.A, env.E, env.W, env.device
        self.obs_dim = int(getattr(net, 'obs_dim', 256))         # 256 for DIEN / dnn / lstm, 256 + U + Cn*E for widedeep

    def close(self):
        if getattr(self, 'h', None) is not None and self.h:
            self.lib.rl4rs_stepper_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_distinct_hint(self, n):
        """Envs of the bound batch the scorer's row dedup is expected to leave (the batch's distinct log lines): decides whether a
        reward step folds its observation into the reward forward (rl4rs_stepper_set_distinct_hint).  None = the batch size."""
        n = self.B if n is None else max(1, min(int(n), self.B))
        if n != self._distinct_hint:
            check(self.lib.rl4rs_stepper_set_distinct_hint(self.h, n))
            self._distinct_hint = n

    def lane_stats(self):
        """(transitions run on lane 0, on lane 1, joins) since the stepper was created (rl4rs_stepper_lane_stats)."""
        a, b, j = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(self.lib.rl4rs_stepper_lane_stats(self.h, C.byref(a), C.byref(b), C.byref(j)))
        return int(a.value), int(b.value), int(j.value)

    def lane_stats_ex(self):
        """(reset forwards, reward steps) issued on a lane since the stepper was created (rl4rs_stepper_lane_stats_ex);
        ``lane_stats`` counts neither."""
        a, b = C.c_int64(0), C.c_int64(0)
        check(self.lib.rl4rs_stepper_lane_stats_ex(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def replay_stats(self):
        """(group forwards started, rows per env handed out, rows per env dropped) since the stepper was created
        (rl4rs_stepper_replay_stats)."""
        a, b, d = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(self.lib.rl4rs_stepper_replay_stats(self.h, C.byref(a), C.byref(b), C.byref(d)))
        return int(a.value), int(b.value), int(d.value)

    def reward_beside_stats(self):
        """(reward steps run on lane 1 beside a replay-ahead forward, bytes of the scorer's second scratch set) since the stepper was
        created (rl4rs_stepper_reward_beside_stats)."""
        a, b = C.c_int64(0), C.c_int64(0)
        check(self.lib.rl4rs_stepper_reward_beside_stats(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def observe(self):
        """rl4rs_stepper_observe: the observation behind a reset as a lane transition -> obs f32 [B, 256], or None where the lane
        rule says no (nothing was enqueued: the caller composes it).  The logged action of step 0 is then the stepper's own row
        (``next_offline_action``)."""
        if not self.reset_lane or not self.act_tail:
            return None
        obs = torch.empty((self.B, self.obs_dim), dtype=torch.float32, device=self.device)
        taken = C.c_int32(0)
        check(self.lib.rl4rs_stepper_observe(self.h, _ptr(obs), C.byref(taken), _stream()))
        return obs if taken.value else None

    def reward_rows(self):
        """Rows per env the last reward step's reward forward scored (rl4rs_stepper_reward_rows)."""
        return int(self.lib.rl4rs_stepper_reward_rows(self.h))

    def click_probs(self):
        """f32 [B, n_complete]: the click probabilities of the last reward step's complete-state rows (rl4rs_stepper_click_probs)."""
        out = torch.empty((self.B, self.env.n_complete), dtype=torch.float32, device=self.device)
        check(self.lib.rl4rs_stepper_click_probs(self.h, _ptr(out), _stream()))
        return out

    def step(self, actions, conti=False, want_reward=True, want_mask_bits=False):
        """-> (obs f32 [B, obs_dim], reward f64 [B] or None, mask_bits i32 [B, W] or None, chosen i32 [B])."""
        obs = torch.empty((self.B, self.obs_dim), dtype=torch.float32, device=self.device)
        reward = torch.empty(self.B, dtype=torch.float64, device=self.device) if want_reward else None
        bits = torch.empty((self.B, self.W), dtype=torch.int32, device=self.device) if want_mask_bits else None
        if conti:
            a = actions.to(self.device) if isinstance(actions, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(actions)).to(self.device)
            if a.dtype not in (torch.float32, torch.float64):
                a = a.to(torch.float64)
            a = a.contiguous()
            assert a.shape == (self.B, self.E), (a.shape, (self.B, self.E))
            chosen = torch.empty(self.B, dtype=torch.int32, device=self.device)
            check(self.lib.rl4rs_env_step_conti(self.h, _ptr(a), 1 if a.dtype == torch.float64 else 0, _ptr(chosen), _ptr(obs),
                                                _ptr(reward), None, _ptr(bits), _stream()))
        else:
            chosen = _dev_tensor(actions, torch.int32, self.device).reshape(-1)
            assert chosen.numel() == self.B, (chosen.shape, self.B)
            check(self.lib.rl4rs_env_step_discrete(self.h, _ptr(chosen), _ptr(obs), _ptr(reward), None, _ptr(bits), _stream()))
        return obs, reward, bits, chosen

    def next_offline_action(self, rows=None):
        """(step, int32 [B] device tensor) - the logged item ids of ``step`` the LAST ``step`` with discrete actions left in the
        stepper's memory (rl4rs_stepper_next_offline_action), or None.  The tensor aliases a row the stepper keeps for that step
        of an episode: it is rewritten by the same step of the next episode.  ``rows``: a dict of the caller's that remembers the
        alias tensors by address (kept outside the stepper: the aliases refer to it)."""
        if not self.act_tail:
            return None
        ptr, step = C.c_void_p(), C.c_int32(-1)
        check(self.lib.rl4rs_stepper_next_offline_action(self.h, C.byref(ptr), C.byref(step)))
        if step.value < 0 or not ptr.value:
            return None
        t = None if rows is None else rows.get(ptr.value)
        if t is None:
            t = _alias_i32(ptr.value, self.B, self.device, self)      # keeps this stepper (the owner of the memory) alive
            if rows is not None:
                rows[ptr.value] = t
        return int(step.value), t

    def offline_action_view(self):
        """Device view of the logged next-step actions the LAST step_record left in its record (int32 [B]; None if it wrote
        none).  Valid until the next step_record has read it: that call consumes its action ids before it rewrites this part."""
        last = getattr(self, '_last_record', None)
        if last is None or last[0].offline_action < 0:
            return None
        L, rec = last
        off = int(L.offline_action)
        return rec[off:off + self.B * 4].view(torch.int32)

    # ---- reference-shaped transitions: one library call, ONE device-to-host copy, one wait ----------------------------------
    def _layout(self, want, conti):
        key = (want, bool(conti))
        cache = self.__dict__.setdefault('_layouts', {})
        if key not in cache:
            L = _lib.StepRecord()
            check(self.lib.rl4rs_stepper_record_layout(self.h, want, 1 if conti else 0, C.byref(L)))
            rec = torch.empty(int(L.total_bytes), dtype=torch.uint8, device=self.device)
            cache[key] = (L, rec)
        return cache[key]

    def step_record(self, actions, conti=False, want=(), shadow=None):
        """rl4rs_env_step_record_host (the transition + its record's host part copied into a fresh pinned block: the int64
        mask of the rllib mode beside the scorer's kernels, the rest after the last one) -> ``StepResult`` of numpy
        views (obs float32 [B, obs_dim], or float64 [B, obs_dim + cols + 1] when 'd3rl_obs' is wanted; reward float64 [B];
        done uint8 [B]; chosen int32 [B]; mask int64 [B, A]; mask_bits uint32 [B, W]; click_p float32 [B, n]; offline_action
        int32 [B] / float64 [B, E]; status int32 [2]).  ``want``: names from rl4rs_amd._lib.STEP_WANT.
        ``shadow(result)`` (optional) runs after everything is enqueued and BEFORE the wait: the views exist (they alias the
        pinned block) but hold no data yet - the place for host work that only needs the objects, e.g. building the list of
        per-env dicts the reference's mask mode returns, while the GPU computes."""
        bits = 0
        for name in want:
            bits |= _lib.STEP_WANT[name]
        L, rec = self._layout(bits, conti)
        if actions is None:
            a = None                                        # observe_record: no transition
        elif conti:
            a = actions
            if not (isinstance(a, torch.Tensor) and a.is_cuda):
                a = np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)
                a = to_device_async(a, torch.float32 if a.dtype == np.float32 else torch.float64, self.device)
            elif a.dtype not in (torch.float32, torch.float64):
                a = a.to(torch.float64)
            a = a.contiguous()
            assert tuple(a.shape) == (self.B, self.E), (a.shape, (self.B, self.E))
            kind = 2 if a.dtype == torch.float64 else 1
        else:
            a = to_device_async(actions, torch.int32, self.device).reshape(-1)
            assert a.numel() == self.B, (a.shape, self.B)
            kind = 0
        self._last_record = (L, rec)
        nb = int(L.host_bytes)
        # the page-locked block of this record: the one the PREVIOUS call set aside while its kernels ran (same size), else a fresh one
        spare = self.__dict__.pop('_spare_block', None)
        host = spare if (spare is not None and spare.numel() == nb) else torch.empty(nb, dtype=torch.uint8, device='cpu', pin_memory=True)
        if a is None:
            check(self.lib.rl4rs_env_observe_record_host(self.h, 1 if conti else 0, bits, _ptr(rec), host.data_ptr(), _stream()))
        else:
            check(self.lib.rl4rs_env_step_record_host(self.h, _ptr(a), kind, bits, _ptr(rec), host.data_ptr(), _stream()))
        raw = host.numpy()
        B = self.B

        def view(off, dtype, shape):
            if off < 0:
                return None
            n = int(np.prod(shape)) * np.dtype(dtype).itemsize
            return raw[off:off + n].view(dtype).reshape(shape)

        r = StepResult()
        r._block = host
        r.status = view(L.status, np.int32, (2,))
        r.reward = view(L.reward, np.float64, (B,))
        r.done = view(L.done, np.uint8, (B,))
        r.chosen = view(L.chosen, np.int32, (B,))
        r.obs = (view(L.obs_d3rl, np.float64, (B, int(L.d3rl_cols))) if L.obs_d3rl >= 0 else view(L.obs, np.float32, (B, int(L.obs_dim))))
        r.mask = view(L.mask_i64, np.int64, (B, self.A))
        r.mask_bits = view(L.mask_bits, np.uint32, (B, self.W))
        r.click_p = view(L.click_p, np.float32, (B, self.env.n_complete))
        r.offline_action = view(L.offline_action, np.float64, (B, self.E)) if conti else view(L.offline_action, np.int32, (B,))
        if shadow is not None:
            shadow(r)
        self._spare_block = torch.empty(nb, dtype=torch.uint8, device='cpu', pin_memory=True)      # in the GPU's shadow: the next record's block
        wait_stream()
        return r

    def observe_record(self, conti=False, want=(), shadow=None):
        """rl4rs_env_observe_record_host: the record of the state the env is in (no transition; what a reset returns) in the
        same form as ``step_record``; reward / done / chosen of the result are meaningless."""
        return self.step_record(None, conti=conti, want=want, shadow=shadow)


class StepResult(object):
    """Host views of one transition record (DeviceStepper.step_record): numpy arrays aliasing ONE pinned block."""
    __slots__ = ('status', 'reward', 'done', 'chosen', 'obs', 'mask', 'mask_bits', 'click_p', 'offline_action', '_block')


AUGRU_KERNELS = {1: 'k_recur<256,augru>', 2: 'k_augru_h16'}


def parse_dien_opts(spec):
    """config['scorer_kernels'] -> sorted tuple of option names (rl4rs_amd._lib.DIEN_OPTS)."""
    if spec is None:
        return ()
    names = [x.strip().lower() for x in spec.split(',')] if isinstance(spec, str) else [str(x).strip().lower() for x in spec]
    names = sorted(set(n for n in names if n))
    bad = [n for n in names if n not in _lib.DIEN_OPTS]
    if bad:
        raise ValueError("unknown scorer_kernels option(s) %s; known: %s" % (bad, sorted(_lib.DIEN_OPTS)))
    return tuple(names)


class DeviceDien(object):
    """rl4rs_dien handle: DIEN scorer with its sequence cache."""

    def __init__(self, config, weights, max_rows, max_slots, device=None):
        _lib.require_device()
        self.lib = _lib.load()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.S = int(config['seq_num'])
        self.L = int(config['maxlen'])
        self.E = int(config['emb_size'])
        self.U = int(config['hidden_units'])
        self.Cn = int(config['category_feature_num'])
        self.Dn = int(config['dense_feature_num'])
        self.K = int(config['class_num'])
        self.max_rows, self.max_slots = int(max_rows), int(max_slots)
        self.F = self.S * 2 * self.E + self.U + (self.Cn + 1) * self.E
        # config['scorer_precision']: 'auto' (default: fp16x2 when the weights allow it; the RL4RS_SCORER environment variable
        # overrides the default for A/B runs - read HERE, the library itself never looks at the environment),
        # 'fp32' (exact-operand fp32 MFMA) or 'fp16x2' (fp16 hi+lo operand split, fp32 accumulate)
        precision = str(config.get('scorer_precision') or os.environ.get('RL4RS_SCORER') or 'auto').lower()
        if precision not in SCORER_MODES:
            raise ValueError("scorer_precision must be one of %s (got %r)" % (sorted(SCORER_MODES), precision))
        # config['scorer_kernels']: names of rl4rs_dien_cfg.kernel_opts bits (rl4rs_amd._lib.DIEN_OPTS; include/rl4rs_hip.h
        # RL4RS_DIEN_OPT_*), an iterable or a comma-separated string; the RL4RS_DIEN_OPTS environment variable is the default
        self.kernel_opts = parse_dien_opts(config.get('scorer_kernels', os.environ.get('RL4RS_DIEN_OPTS', '')))
        opt_bits = 0
        for name in self.kernel_opts:
            opt_bits |= _lib.DIEN_OPTS[name]
        cfg = _lib.DienCfg(self.L, self.E, self.U, self.Dn, self.Cn, int(config['category_hash_size']),
                           self.S, self.K, self.max_rows, self.max_slots, SCORER_MODES[precision], opt_bits)
        w = _lib.DienWeights()
        keep = []

        def fp(name):
            arr = np.ascontiguousarray(weights[name], dtype=np.float32)
            keep.append(arr)
            return arr.ctypes.data_as(_lib._FP)

        for name in ('cat_emb', 'dense_w1', 'dense_b1', 'dense_w2', 'dense_b2', 'seq_emb', 'obs_w', 'obs_b',
                     'out_w', 'out_b'):
            setattr(w, name, fp(name))
        for i in range(self.S):
            w.gru_gate_w[i] = fp('gru%d_gate_w' % i)
            w.gru_gate_b[i] = fp('gru%d_gate_b' % i)
            w.gru_cand_w[i] = fp('gru%d_cand_w' % i)
            w.gru_cand_b[i] = fp('gru%d_cand_b' % i)
            w.att_w1[i] = fp('att%d_w1' % i)
            w.att_b1[i] = fp('att%d_b1' % i)
            w.att_w2[i] = fp('att%d_w2' % i)
            w.att_b2[i] = fp('att%d_b2' % i)
            w.att_w3[i] = fp('att%d_w3' % i)
            w.att_b3[i] = fp('att%d_b3' % i)
            w.augru_gate_w[i] = fp('augru%d_gate_w' % i)
            w.augru_gate_b[i] = fp('augru%d_gate_b' % i)
            w.augru_cand_w[i] = fp('augru%d_cand_w' % i)
            w.augru_cand_b[i] = fp('augru%d_cand_b' % i)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.rl4rs_dien_create(C.byref(cfg), C.byref(w), _stream(), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, 'h', None) is not None and self.h:
            self.lib.rl4rs_dien_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def encode(self, s, ids, slot_base=0):
        """ids: int32 device tensor [n, L] (or a raw (ptr, n) pair)."""
        if isinstance(ids, tuple):
            ptr, n = ids
        else:
            ids = _dev_tensor(ids, torch.int32, self.device)
            assert ids.dim() == 2 and ids.shape[1] == self.L
            ptr, n = _ptr(ids), ids.shape[0]
            self._keep_ids = ids
        check(self.lib.rl4rs_dien_encode(self.h, s, ptr, n, slot_base, _stream()))

    def forward(self, R, group, dense, cat, slots, want_obs=True, want_prob=False, obs_out=None, want_obs_last=False):
        """dense/cat: device tensors or raw c_void_p pointers; slots: int32 device tensor [S, R/group].
        ``want_obs_last`` (with ``want_prob``): -> (obs, prob, obs_last f32 [R / group, 256]), the observation of the last row of
        each group (rl4rs_dien_set_obs_last)."""
        dp = dense if isinstance(dense, C.c_void_p) else _ptr(dense)
        cp = cat if isinstance(cat, C.c_void_p) else _ptr(cat)
        assert slots.dtype == torch.int32 and slots.numel() == self.S * (R // group)
        obs = None
        if want_obs:
            obs = obs_out if obs_out is not None else torch.empty((R, 256), dtype=torch.float32, device=self.device)
        prob = torch.empty(R, dtype=torch.float32, device=self.device) if want_prob else None
        last = None
        if want_obs_last:
            last = torch.empty((R // group, 256), dtype=torch.float32, device=self.device)
            check(self.lib.rl4rs_dien_set_obs_last(self.h, _ptr(last)))
        check(self.lib.rl4rs_dien_forward(self.h, R, group, dp, cp, _ptr(slots), _ptr(obs), _ptr(prob), _stream()))
        return (obs, prob, last) if want_obs_last else (obs, prob)

    def head_prob(self, obs):
        R = obs.shape[0]
        assert obs.dtype == torch.float32 and obs.is_contiguous() and obs.shape[1] == 256
        prob = torch.empty(R, dtype=torch.float32, device=self.device)
        check(self.lib.rl4rs_dien_head_prob(self.h, R, _ptr(obs), _ptr(prob), _stream()))
        return prob

    def snapshot(self, which, rows):
        p = C.c_void_p()
        n = C.c_int64()
        check(self.lib.rl4rs_dien_buffer(self.h, which, C.byref(p), C.byref(n)))
        if which == DIEN_H1_FRAG:                     # [max_slots + 1, step tiles, k-block, lane, 8], sequence input 0
            out = torch.empty((self.max_slots + 1, (self.L + 31) // 32, 8, 64, 8), dtype=torch.float32, device=self.device)
            assert out.numel() * 4 == n.value
            check(self.lib.rl4rs_copy_d2d(_ptr(out), p, n.value, _stream()))
            return out
        if which in (DIEN_N_ACTIVE, DIEN_ROW_REP, DIEN_ROW_ACTIVE, DIEN_LEAD):      # int32: row dedup of the last forward (an error where it is off); lead[]
            out = torch.empty(n.value // 4, dtype=torch.int32, device=self.device)
            check(self.lib.rl4rs_copy_d2d(_ptr(out), p, n.value, _stream()))
            return out
        if which == DIEN_ALL_FEATURE:
            shape = (self.max_rows, n.value // (4 * self.max_rows))      # F, or the Kh columns of the table form
        elif which == DIEN_SCORES:
            shape = (self.S, self.max_rows, self.L)
        elif which == DIEN_QUERY:
            shape = (self.max_rows, self.E)
        else:
            shape = (self.max_slots, self.L, self.E)
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        assert out.numel() * 4 == n.value
        check(self.lib.rl4rs_copy_d2d(_ptr(out), p, n.value, _stream()))
        return out

    # profiling (bench.py roofline)
    def set_row_order(self, order):
        """Processing order of the env groups of the following forwards (int32 device tensor, a permutation; None = identity):
        rl4rs_dien_set_row_order - a locality hint, results unchanged."""
        if order is not None:
            assert order.dtype == torch.int32 and order.is_contiguous() and order.is_cuda
        self._row_order = order                     # keep it alive
        check(self.lib.rl4rs_dien_set_row_order(self.h, _ptr(order), 0 if order is None else int(order.numel())))

    def set_augru_rows(self, rows):
        """Row-tile form of k_augru_x for the following forwards: 0 automatic, 32 or 64 (rl4rs_dien_set_augru_rows)."""
        check(self.lib.rl4rs_dien_set_augru_rows(self.h, int(rows)))

    def set_distinct_hint(self, n):
        """Distinct row groups the row dedup is expected to leave (rl4rs_dien_set_distinct_hint; None / 0 = the forward's rows)."""
        check(self.lib.rl4rs_dien_set_distinct_hint(self.h, int(n or 0)))

    def set_profiling(self, on):
        """0 / False off, 1 / True every kernel class, 2 only the AUGRU recurrence (rl4rs_dien_set_profiling)."""
        check(self.lib.rl4rs_dien_set_profiling(self.h, 2 if on == 2 else (1 if on else 0)))

    def profile_reset(self):
        check(self.lib.rl4rs_dien_profile_reset(self.h))

    def dedup_counts(self):
        """-> (forwards since profile_reset that launched k_row_dedup, forwards that took a carried partition instead)."""
        a, b = C.c_int64(), C.c_int64()
        check(self.lib.rl4rs_dien_dedup_counts(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_plan(self):
        """The launch plan of the last forward as a dict of its key=value tokens (rl4rs_dien_last_plan; {} before the first)."""
        buf = C.create_string_buffer(512)
        check(self.lib.rl4rs_dien_last_plan(self.h, buf, 512))
        return dict(tok.split('=', 1) for tok in buf.value.decode().split())

    def set_row_partition(self, rep, active, n_active):
        """The NEXT forward takes its duplicate row groups from these int32 device tensors (rl4rs_dien_set_row_partition)."""
        for t in (rep, active, n_active):
            assert t.dtype == torch.int32 and t.is_contiguous() and t.is_cuda
        self._partition = (rep, active, n_active)       # keep them alive
        check(self.lib.rl4rs_dien_set_row_partition(self.h, _ptr(rep), _ptr(active), _ptr(n_active), int(rep.numel())))

    def profile(self):
        out = {}
        for k in range(self.lib.rl4rs_dien_kernel_count()):
            ms = C.c_double()
            n = C.c_int64()
            check(self.lib.rl4rs_dien_profile_read(self.h, k, C.byref(ms), C.byref(n)))
            name = self.lib.rl4rs_dien_kernel_name(k).decode()
            if name == 'augru':
                name = self.augru_kernel                # the key bench.py's roofline looks up
            else:
                buf = C.create_string_buffer(160)       # what this handle really launches (mode- and option-dependent)
                check(self.lib.rl4rs_dien_kernel_label(self.h, k, buf, 160))
                name = buf.value.decode()
            out[name] = (ms.value, n.value)
        return out

    @property
    def scorer_mode(self):
        """'fp32' or 'fp16x2': what the handle resolved config['scorer_precision'] to."""
        m = C.c_int32()
        check(self.lib.rl4rs_dien_scorer_mode(self.h, C.byref(m)))
        return 'fp16x2' if m.value == 2 else 'fp32'

    def check_status(self):
        """Synchronising check of the handle's status bits: raises if the fp16x2 scorer left the fp16 range."""
        f = C.c_int32()
        check(self.lib.rl4rs_dien_status(self.h, C.byref(f), _stream()))
        if f.value & 1:
            raise _lib.Rl4rsHipError(
                "fp16x2 scorer: a recurrent state left the fp16 range (|h| >= 6e4 or NaN); the affected forwards are "
                "invalid - use config['scorer_precision'] = 'fp32' for this model")

    @property
    def augru_kernel(self):
        if self.scorer_mode == 'fp16x2' and 'augru_h16' not in self.kernel_opts:
            return 'k_augru_x'                      # dien.hip: the default fp16x2 recurrence ('augru_h16' selects the first generation)
        return AUGRU_KERNELS[SCORER_MODES[self.scorer_mode]]


SIMNET_ALGOS = {'dnn': 1, 'widedeep': 2, 'lstm': 3}          # include/rl4rs_hip.h RL4RS_SIMNET_*


class DeviceSimnet(object):
    """rl4rs_simnet handle: the dnn / widedeep / lstm simulator families (same calling pattern as DeviceDien)."""

    def __init__(self, config, weights, max_rows, max_slots, algo=None, device=None):
        _lib.require_device()
        self.lib = _lib.load()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.algo = str(algo if algo is not None else config.get('algo')).lower()
        if self.algo not in SIMNET_ALGOS:
            raise ValueError("algo must be one of %s (got %r)" % (sorted(SIMNET_ALGOS), self.algo))
        self.S = int(config['seq_num'])
        self.L = int(config['maxlen'])
        self.max_rows, self.max_slots = int(max_rows), int(max_slots)
        cfg = _lib.SimnetCfg(SIMNET_ALGOS[self.algo], self.L, int(config['emb_size']), int(config['hidden_units']),
                             int(config['dense_feature_num']), int(config['category_feature_num']),
                             int(config['category_hash_size']), self.S, int(config['class_num']), self.max_rows,
                             self.max_slots)
        w = _lib.SimnetWeights()
        keep = []

        def fp(name):
            arr = np.ascontiguousarray(weights[name], dtype=np.float32)
            keep.append(arr)
            return arr.ctypes.data_as(_lib._FP)

        for name in ('cat_emb', 'seq_emb', 'dense_w1', 'dense_b1', 'dense_w2', 'dense_b2', 'fc_w', 'fc_b', 'obs_w',
                     'obs_b', 'out_w', 'out_b', 'cat_gru_kernel', 'cat_gru_recurrent', 'cat_gru_bias'):
            if name in weights:
                setattr(w, name, fp(name))
        for i in range(self.S):
            if 'seq%d_gru_kernel' % i in weights:
                w.seq_gru_kernel[i] = fp('seq%d_gru_kernel' % i)
                w.seq_gru_recurrent[i] = fp('seq%d_gru_recurrent' % i)
                w.seq_gru_bias[i] = fp('seq%d_gru_bias' % i)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.rl4rs_simnet_create(C.byref(cfg), C.byref(w), _stream(), C.byref(h)))
        self.h = h
        d = C.c_int32()
        check(self.lib.rl4rs_simnet_obs_dim(self.h, C.byref(d)))
        self.obs_dim = d.value

    def close(self):
        if getattr(self, 'h', None) is not None and self.h:
            self.lib.rl4rs_simnet_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def encode(self, s, ids, slot_base=0):
        if isinstance(ids, tuple):
            ptr, n = ids
        else:
            ids = _dev_tensor(ids, torch.int32, self.device)
            assert ids.dim() == 2 and ids.shape[1] == self.L
            ptr, n = _ptr(ids), ids.shape[0]
            self._keep_ids = ids
        check(self.lib.rl4rs_simnet_encode(self.h, s, ptr, n, slot_base, _stream()))

    def forward(self, R, group, dense, cat, slots, want_obs=True, want_prob=False, obs_out=None):
        dp = dense if isinstance(dense, C.c_void_p) else _ptr(dense)
        cp = cat if isinstance(cat, C.c_void_p) else _ptr(cat)
        assert slots.dtype == torch.int32 and slots.numel() == self.S * (R // group)
        obs = None
        if want_obs:
            obs = obs_out if obs_out is not None else torch.empty((R, self.obs_dim), dtype=torch.float32, device=self.device)
        prob = torch.empty(R, dtype=torch.float32, device=self.device) if want_prob else None
        check(self.lib.rl4rs_simnet_forward(self.h, R, group, dp, cp, _ptr(slots), _ptr(obs), _ptr(prob), _stream()))
        return obs, prob

    def head_prob(self, obs):
        R = obs.shape[0]
        assert obs.dtype == torch.float32 and obs.is_contiguous() and obs.shape[1] == self.obs_dim
        prob = torch.empty(R, dtype=torch.float32, device=self.device)
        check(self.lib.rl4rs_simnet_head_prob(self.h, R, _ptr(obs), _ptr(prob), _stream()))
        return prob

    def check_status(self):
        pass

    # no-op profiling hooks so bench / facade code can treat every scorer alike
    def set_profiling(self, on):
        pass

    def profile_reset(self):
        pass

    def profile(self):
        return {}


SIMTRAIN_ORDER = {
    'dnn': ('cat_emb', 'dense_w1', 'dense_b1', 'dense_w2', 'dense_b2', 'fc_w', 'fc_b', 'obs_w', 'obs_b', 'out_w', 'out_b'),
    'widedeep': ('cat_emb', 'seq_emb', 'dense_w1', 'dense_b1', 'dense_w2', 'dense_b2', 'fc_w', 'fc_b', 'out_w', 'out_b'),
    # lstm: + the keras GRUs (category GRU, then one per sequence input; the names carry the sequence index)
    'lstm': ('cat_emb', 'seq_emb', 'dense_w1', 'dense_b1', 'dense_w2', 'dense_b2', 'obs_w', 'obs_b', 'out_w', 'out_b',
             'cat_gru_kernel', 'cat_gru_recurrent', 'cat_gru_bias'),
    # adversarial_slate.py (trainer only, head 'adversarial'): the concat feeds the output layer directly
    'adversarial_slate': ('cat_emb', 'seq_emb', 'dense_w1', 'dense_b1', 'dense_w2', 'dense_b2', 'out_w', 'out_b'),
}


SIMTRAIN_ALGOS = dict(SIMNET_ALGOS, adversarial_slate=4)       # include/rl4rs_hip.h RL4RS_SIMNET_ADVERSARIAL: trainer only
TRAIN_HEADS = {'item': 0, 'slate': 1, 'multiclass': 2, 'adversarial': 3}       # include/rl4rs_hip.h RL4RS_HEAD_*


def _simtrain_names(algo, seq_num):
    names = list(SIMTRAIN_ORDER[algo])
    if algo == 'lstm':
        for i in range(seq_num):
            names += ['seq%d_gru_kernel' % i, 'seq%d_gru_recurrent' % i, 'seq%d_gru_bias' % i]
    return names


class _FlatNet(object):
    """Shared plumbing of every trainable handle ``<_prefix>*``: flat parameters, gradient and Adam state, copied device to device
    on the current stream.  The setters keep their source tensors alive until the next call (no host wait: they sit on the
    data-parallel step path).  ``shapes``: (name, shape) of the arrays in flat order, where the wrapper knows them."""
    _prefix = None
    shapes = ()

    def _call(self, name):
        return getattr(self.lib, self._prefix + name)

    def close(self):
        if getattr(self, 'h', None) is not None and self.h:
            self._call('destroy')(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ptrs(self):
        """(parameters, gradient, count) of the handle's flat buffers"""
        p, g, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        check(self._call('params')(self.h, C.byref(p), C.byref(g), C.byref(n)))
        return p, g, n.value

    def _grad_ptr(self):
        _, g, n = self._ptrs()
        if g is None:
            raise TypeError('%s keeps no gradient of its own: it is the buffer its loss calls fill' % type(self).__name__)
        return g, n

    def _adam_ptrs(self):
        m, v, t = C.c_void_p(), C.c_void_p(), C.c_int64()
        check(self._call('adam_state')(self.h, C.byref(m), C.byref(v), C.byref(t)))
        return m, v, int(t.value)

    def _copy_out(self, src, n, out=None):
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=self.device)
        assert out.dtype == torch.float32 and out.numel() == n and out.is_contiguous() and out.is_cuda
        check(self.lib.rl4rs_copy_d2d(_ptr(out), src, n * 4, _stream()))
        return out

    def _copy_in(self, which, dst, n, src):
        src = src.to(device=self.device, dtype=torch.float32).contiguous()
        assert src.numel() == n, (src.numel(), n)
        check(self.lib.rl4rs_copy_d2d(dst, _ptr(src), n * 4, _stream()))
        self.__dict__.setdefault('_keep', {})[which] = src       # alive until the next copy into the same buffer

    def params(self, out=None):
        """Copy of the flat parameter buffer (device tensor); ``out``: a contiguous float32 device tensor to copy into."""
        p, _, n = self._ptrs()
        return self._copy_out(p, n, out)

    def flat_gradient(self, out=None):
        """Copy of the flat gradient the handle holds (device tensor)."""
        g, n = self._grad_ptr()
        return self._copy_out(g, n, out)

    def set_params(self, flat):
        p, _, n = self._ptrs()
        self._copy_in('params', p, n, flat)

    def set_flat_gradient(self, flat):
        g, n = self._grad_ptr()
        self._copy_in('grad', g, n, flat)

    flat_params, set_flat_params, grad = params, set_params, flat_gradient

    def _flat(self, which):
        """'params' or 'grad': the copy by name, as the trainers' tests ask for it"""
        return self.params() if which == 'params' else self.flat_gradient()

    def _split(self, flat):
        out, o = {}, 0
        for name, shape in self.shapes:
            k = int(np.prod(shape))
            out[name] = flat[o:o + k].reshape(shape)
            o += k
        return out

    def weights(self):
        """Current parameters as a dict of device tensors, by the names of ``shapes``."""
        return self._split(self.params())

    def gradients(self):
        return self._split(self.flat_gradient())

    def copy_from(self, other):
        """This handle's parameters <- ``other``'s, device to device."""
        check(self._call('copy_params')(self.h, other.h, _stream()))

    def adam_state(self):
        """(m, v, step): copies of the Adam moments (device tensors) and the step counter - what a checkpoint keeps."""
        m, v, t = self._adam_ptrs()
        return self._copy_out(m, self.n_params), self._copy_out(v, self.n_params), t

    def set_adam_state(self, m, v, step):
        pm, pv, _ = self._adam_ptrs()
        self._copy_in('adam_m', pm, self.n_params, m)
        self._copy_in('adam_v', pv, self.n_params, v)
        check(self._call('set_adam_step')(self.h, int(step)))


class DeviceSimTrainer(_FlatNet):
    """rl4rs_simtrain handle: supervised training of the 'dnn' / 'widedeep' / 'lstm' simulators on the device
    (script/supervised_train.py): forward with dropout, keras binary_crossentropy, backward, Adam.  ``weights()`` carries the
    names of rl4rs_amd.nets.simnets.simnet_spec; ``grad`` is the forward + backward here, the flat gradient is ``flat_gradient()``.
    ``head``: 'item' (labels [N]), or the slate-wise output layers 'slate' / 'multiclass' (the *_slate.py / *_slate_multiclass.py
    models; labels [N, 9] of 0 / 1), or 'adversarial' with algo 'adversarial_slate'."""
    _prefix = 'rl4rs_simtrain_'

    def _set_head(self, head):
        if head not in TRAIN_HEADS:
            raise ValueError("head must be one of %s (got %r)" % (sorted(TRAIN_HEADS), head))
        if (head == 'adversarial') != (self.algo == 'adversarial_slate'):
            raise ValueError("head 'adversarial' and algo 'adversarial_slate' come as a pair (got head %r, algo %r)" % (head, self.algo))
        self.head = head
        self.K = int(self.config['class_num']) if head == 'item' else (22 if head == 'multiclass' else 9)

    def __init__(self, config, weights, max_batch=256, algo=None, device=None, head='item'):
        _lib.require_device()
        self.lib = _lib.load()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.config = dict(config)
        self.algo = str(algo if algo is not None else config.get('algo', 'dnn')).lower()
        if self.algo not in SIMTRAIN_ORDER:
            raise NotImplementedError("device-side simulator training exists for %s (got %r)" % (sorted(SIMTRAIN_ORDER), self.algo))
        self._set_head(head)
        self.Cn, self.Dn = int(config['category_feature_num']), int(config['dense_feature_num'])
        self.S, self.L = int(config['seq_num']), int(config['maxlen'])
        self.max_batch = int(max_batch)
        cfg = _lib.SimnetCfg(SIMTRAIN_ALGOS[self.algo], self.L, int(config['emb_size']), int(config['hidden_units']),
                             self.Dn, self.Cn, int(config['category_hash_size']), self.S,
                             int(config['class_num']), self.max_batch, 1)
        w = _lib.SimnetWeights()
        keep = []
        self.shapes = []
        for name in _simtrain_names(self.algo, self.S):
            arr = np.ascontiguousarray(weights[name], dtype=np.float32)
            keep.append(arr)
            self.shapes.append((name, arr.shape))
            ptr = arr.ctypes.data_as(_lib._FP)
            if name.startswith('seq') and '_gru_' in name:
                getattr(w, 'seq_gru_' + name.split('_gru_')[1])[int(name[3:name.index('_')])] = ptr
            else:
                setattr(w, name, ptr)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.rl4rs_simtrain_create_head(C.byref(cfg), C.byref(w), TRAIN_HEADS[self.head], self.max_batch, _stream(),
                                                      C.byref(h)))
        self.h = h
        self.iteration = 0
        self.n_params = self._ptrs()[2]

    def masks(self, N):
        """The dropout keep-masks [N, hidden_units] (uint8) of the last grad / step call."""
        m1, m2 = C.c_void_p(), C.c_void_p()
        check(self._call('masks')(self.h, C.byref(m1), C.byref(m2)))
        U = int(self.config['hidden_units'])
        out = []
        for m in (m1, m2):
            t = torch.empty((N, U), dtype=torch.uint8, device=self.device)
            check(self.lib.rl4rs_copy_d2d(_ptr(t), m, N * U, _stream()))
            out.append(t)
        return out

    def _batch(self, dense, cat, labels, seqs):
        N = dense.shape[0]
        assert dense.dtype == torch.float32 and dense.shape == (N, self.Dn) and dense.is_contiguous()
        assert cat.dtype == torch.int32 and cat.shape == (N, self.Cn) and cat.is_contiguous()
        if labels is not None:
            labels = labels.to(torch.int32).contiguous()
            assert labels.shape == ((N,) if self.head == 'item' else (N, 9)), (self.head, tuple(labels.shape))
        sp = None
        if self.algo != 'dnn':
            assert seqs is not None and len(seqs) == self.S, "every family but dnn needs the seq_num sequence inputs"
            for q in seqs:
                assert q.dtype == torch.int32 and q.shape == (N, self.L) and q.is_contiguous()
            sp = (C.c_void_p * self.S)(*[_ptr(q) for q in seqs])
        return N, labels, sp

    def grad(self, dense, cat, labels, seqs=None, dropout_rate=0.2, seed=0, step=0):
        """Forward + loss + backward; returns the mean loss (device scalar tensor)."""
        N, labels, sp = self._batch(dense, cat, labels, seqs)
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        check(self._call('grad')(self.h, N, _ptr(dense), _ptr(cat), sp, _ptr(labels), dropout_rate, seed, step,
                                           _ptr(loss), _stream()))
        return loss

    def step(self, dense, cat, labels, seqs=None, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7, dropout_rate=0.2, seed=0):
        N, labels, sp = self._batch(dense, cat, labels, seqs)
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        check(self._call('step')(self.h, N, _ptr(dense), _ptr(cat), sp, _ptr(labels), lr, beta1, beta2, eps,
                                           dropout_rate, seed, self.iteration, _ptr(loss), _stream()))
        self.iteration += 1
        return loss

    def evaluate(self, dense, cat, labels=None, seqs=None):
        """Inference forward (no dropout, no backward; parameters, gradient and Adam state untouched) -> (pred [N, K], loss_rows
        [N]): the model output - softmax for 'item' (K = class_num) and 'multiclass' (K = 22), sigmoid (K = 9) otherwise - and the
        head's row losses (None without labels).  Device tensors; nothing waits for the host."""
        N, labels, sp = self._batch(dense, cat, labels, seqs)
        pred = torch.empty((N, self.K), dtype=torch.float32, device=self.device)
        rows = torch.empty(N, dtype=torch.float32, device=self.device) if labels is not None else None
        check(self._call('eval')(self.h, N, _ptr(dense), _ptr(cat), sp, _ptr(labels), _ptr(pred), _ptr(rows), _stream()))
        return pred, rows


DIENTRAIN_BASE = ('cat_emb', 'seq_emb', 'dense_w1', 'dense_b1', 'dense_w2', 'dense_b2', 'obs_w', 'obs_b', 'out_w', 'out_b')
DIENTRAIN_SEQ = ('gru%d_gate_w', 'gru%d_gate_b', 'gru%d_cand_w', 'gru%d_cand_b', 'att%d_w1', 'att%d_b1', 'att%d_w2', 'att%d_b2',
                 'att%d_w3', 'att%d_b3', 'augru%d_gate_w', 'augru%d_gate_b', 'augru%d_cand_w', 'augru%d_cand_b')


class DeviceDienTrainer(DeviceSimTrainer):
    """rl4rs_dientrain handle: supervised training of the DIEN simulator on the device (same interface as DeviceSimTrainer)."""
    _prefix = 'rl4rs_dientrain_'

    def __init__(self, config, weights, max_batch=256, device=None, head='item'):
        _lib.require_device()
        self.lib = _lib.load()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.config = dict(config)
        self.algo = 'dien'
        self._set_head(head)
        self.Cn, self.Dn = int(config['category_feature_num']), int(config['dense_feature_num'])
        self.S, self.L = int(config['seq_num']), int(config['maxlen'])
        self.max_batch = int(max_batch)
        cfg = _lib.DienCfg(self.L, int(config['emb_size']), int(config['hidden_units']), self.Dn, self.Cn,
                           int(config['category_hash_size']), self.S, int(config['class_num']), self.max_batch, 1, 0)
        w = _lib.DienWeights()
        keep = []
        self.shapes = []
        names = list(DIENTRAIN_BASE) + [n % i for i in range(self.S) for n in DIENTRAIN_SEQ]
        for name in names:
            arr = np.ascontiguousarray(weights[name], dtype=np.float32)
            keep.append(arr)
            self.shapes.append((name, arr.shape))
            ptr = arr.ctypes.data_as(_lib._FP)
            if name in DIENTRAIN_BASE:
                setattr(w, name, ptr)
            else:                                   # 'gru0_gate_w' -> field gru_gate_w[0]
                head, tail = name.split('_', 1)
                idx = int(''.join(ch for ch in head if ch.isdigit()))
                getattr(w, ''.join(ch for ch in head if not ch.isdigit()) + '_' + tail)[idx] = ptr
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.rl4rs_dientrain_create_head(C.byref(cfg), C.byref(w), TRAIN_HEADS[self.head], self.max_batch, _stream(),
                                                       C.byref(h)))
        self.h = h
        self.iteration = 0
        self.n_params = self._ptrs()[2]


class DeviceRawPolicy(object):
    """rl4rs_rawpolicy handle: the raw-state policy encoder (rllib_rawstate_model.py) with the action-mask rule,
    forward only.  Inputs are the raw feature tensors an env with config['rawstate_as_obs'] exposes."""

    def __init__(self, config, weights, max_rows, device=None):
        _lib.require_device()
        self.lib = _lib.load()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.S, self.L, self.A = int(config['seq_num']), int(config['maxlen']), int(config['action_size'])
        self.Cn, self.Dn = int(config['category_feature_num']), int(config['dense_feature_num'])
        self.W = (self.A + 31) // 32
        self.max_rows = int(max_rows)
        cfg = _lib.RawPolicyCfg(self.L, int(config['emb_size']), int(config['hidden_units']), self.Dn, self.Cn,
                                int(config['category_hash_size']), self.S, self.A, self.max_rows)
        w = _lib.RawPolicyWeights()
        keep = []
        for name, _ in _lib.RawPolicyWeights._fields_:
            arr = np.ascontiguousarray(weights[name], dtype=np.float32)
            keep.append(arr)
            setattr(w, name, arr.ctypes.data_as(_lib._FP))
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.rl4rs_rawpolicy_create(C.byref(cfg), C.byref(w), _stream(), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, 'h', None) is not None and self.h:
            self.lib.rl4rs_rawpolicy_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _inputs(self, cat, dense, seqs, mask_bits):
        N = cat.shape[0]
        assert cat.dtype == torch.int32 and cat.shape == (N, self.Cn) and cat.is_contiguous()
        assert dense.dtype == torch.float32 and dense.shape == (N, self.Dn) and dense.is_contiguous()
        assert len(seqs) == self.S
        for q in seqs:
            assert q.dtype == torch.int32 and q.shape == (N, self.L) and q.is_contiguous()
        if mask_bits is not None:
            assert mask_bits.dtype == torch.int32 and mask_bits.shape == (N, self.W) and mask_bits.is_contiguous()
        sp = (C.c_void_p * self.S)(*[_ptr(q) for q in seqs])
        return N, sp

    def _outs(self, N, want_logits):
        f = lambda: torch.empty(N, dtype=torch.float32, device=self.device)
        lg = torch.empty((N, self.A), dtype=torch.float32, device=self.device) if want_logits else None
        return f(), f(), f(), lg

    def act(self, cat, dense, seqs, mask_bits=None, seed=0, step=0, want_logits=False):
        """-> actions [N] int32, logp, value, entropy (float32 [N]), masked logits [N, A] or None."""
        N, sp = self._inputs(cat, dense, seqs, mask_bits)
        a = torch.empty(N, dtype=torch.int32, device=self.device)
        lp, v, ent, lg = self._outs(N, want_logits)
        check(self.lib.rl4rs_rawpolicy_act(self.h, N, _ptr(cat), _ptr(dense), sp, _ptr(mask_bits), seed, step, _ptr(a),
                                           _ptr(lp), _ptr(v), _ptr(ent), _ptr(lg), _stream()))
        return a, lp, v, ent, lg

    def evaluate(self, cat, dense, seqs, actions, mask_bits=None, want_logits=False):
        N, sp = self._inputs(cat, dense, seqs, mask_bits)
        actions = actions.to(torch.int32).contiguous()
        lp, v, ent, lg = self._outs(N, want_logits)
        check(self.lib.rl4rs_rawpolicy_evaluate(self.h, N, _ptr(cat), _ptr(dense), sp, _ptr(mask_bits), _ptr(actions),
                                                _ptr(lp), _ptr(v), _ptr(ent), _ptr(lg), _stream()))
        return lp, v, ent, lg


class _DevAlias(object):
    """__cuda_array_interface__ carrier: lets torch alias device memory owned by a library handle."""

    def __init__(self, ptr, count, owner):
        self.owner = owner
        self.__cuda_array_interface__ = {'shape': (int(count),), 'typestr': '<f4', 'data': (int(ptr), False), 'version': 2}


def _alias_i32(ptr, count, device, owner):
    a = _DevAlias(ptr, count, owner)
    a.__cuda_array_interface__['typestr'] = '<i4'
    with torch.cuda.device(device):
        t = torch.as_tensor(a, device=device)
    assert t.data_ptr() == int(ptr) and t.dtype == torch.int32
    return t


def _alias_f32(ptr, count, device, owner):
    with torch.cuda.device(device):
        t = torch.as_tensor(_DevAlias(ptr, count, owner), device=device)
    assert t.data_ptr() == int(ptr) and t.dtype == torch.float32
    return t


class DeviceRawTrainer(_FlatNet, DeviceRawPolicy):
    """rl4rs_rawtrain handle: the raw-state policy with A2C / PPO loss, backward and Adam on the device; as a Q network, the
    (double-)DQN loss on packed raw-state records, the greedy action and the per-variable-clipped Adam step."""
    A2C, PPO = 0, 1
    ORDER = ('cat_emb', 'seq_emb', 'dense_w1', 'dense_b1', 'dense_w2', 'dense_b2', 'ctx_w', 'ctx_b', 'head_w', 'head_b')
    _prefix = 'rl4rs_rawtrain_'         # weights(): head_w = [out_w | value_w], head_b = [out_b | value_b]

    def __init__(self, config, weights, max_rows, device=None):
        _lib.require_device()
        self.lib = _lib.load()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.S, self.L, self.A = int(config['seq_num']), int(config['maxlen']), int(config['action_size'])
        self.Cn, self.Dn = int(config['category_feature_num']), int(config['dense_feature_num'])
        self.W = (self.A + 31) // 32
        self.max_rows = int(max_rows)
        E, U = int(config['emb_size']), int(config['hidden_units'])
        H = int(config['category_hash_size'])
        cfg = self._cfg = _lib.RawPolicyCfg(self.L, E, U, self.Dn, self.Cn, H, self.S, self.A, self.max_rows)
        w = _lib.RawPolicyWeights()
        keep = []
        for name, _ in _lib.RawPolicyWeights._fields_:
            arr = np.ascontiguousarray(weights[name], dtype=np.float32)
            keep.append(arr)
            setattr(w, name, arr.ctypes.data_as(_lib._FP))
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.rl4rs_rawtrain_create(C.byref(cfg), C.byref(w), _stream(), C.byref(h)))
        self.h = h
        self.shapes = [('cat_emb', (H, E)), ('seq_emb', (H, E)), ('dense_w1', (self.Dn, U)), ('dense_b1', (U,)), ('dense_w2', (U, U)),
                       ('dense_b2', (U,)), ('ctx_w', (self.S * E + U + E, 256)), ('ctx_b', (256,)), ('head_w', (256, self.A + 1)),
                       ('head_b', (self.A + 1,))]

    def flat_view(self, which):
        """ZERO-COPY torch view of the handle's flat parameter ('params') or gradient ('grad') buffer: a data-parallel trainer
        all-reduces the gradient in place between loss_grad and adam_step, and broadcasts the parameters at start."""
        p, g, n = self._ptrs()
        return _alias_f32((p if which == 'params' else g).value, n, self.device, self)

    def table_rows(self):
        """(offset, rows, width) of the two embedding tables inside the flat buffers (cat_emb, seq_emb come first)."""
        (_, (H, E)) = self.shapes[0]
        return [(0, H, E), (H * E, H, E)]

    def act(self, cat, dense, seqs, mask_bits=None, seed=0, step=0, want_logits=False):
        N, sp = self._inputs(cat, dense, seqs, mask_bits)
        a = torch.empty(N, dtype=torch.int32, device=self.device)
        lp, v, ent, lg = self._outs(N, want_logits)
        check(self.lib.rl4rs_rawtrain_act(self.h, N, _ptr(cat), _ptr(dense), sp, _ptr(mask_bits), seed, step, _ptr(a), _ptr(lp),
                                          _ptr(v), _ptr(ent), _ptr(lg), _stream()))
        return a, lp, v, ent, lg

    def evaluate(self, cat, dense, seqs, actions, mask_bits=None, want_logits=False):
        N, sp = self._inputs(cat, dense, seqs, mask_bits)
        actions = actions.to(torch.int32).contiguous()
        lp, v, ent, lg = self._outs(N, want_logits)
        check(self.lib.rl4rs_rawtrain_evaluate(self.h, N, _ptr(cat), _ptr(dense), sp, _ptr(mask_bits), _ptr(actions), _ptr(lp),
                                               _ptr(v), _ptr(ent), _ptr(lg), _stream()))
        return lp, v, ent, lg

    def loss_grad(self, algo, cat, dense, seqs, actions, adv, ret, mask_bits=None, old_logp=None, old_value=None, old_logits=None,
                  vf_coeff=0.5, ent_coeff=0.01, clip=0.3, vf_clip=500.0, kl_coeff=0.2):
        """-> stats [pi_loss, vf_loss, entropy, kl] sums (device tensor); the gradient stays in the handle (gradients())."""
        N, sp = self._inputs(cat, dense, seqs, mask_bits)
        f = lambda t: None if t is None else t.to(torch.float32).contiguous()
        actions = actions.to(torch.int32).contiguous()
        adv, ret, old_logp, old_value, old_logits = f(adv), f(ret), f(old_logp), f(old_value), f(old_logits)
        stats = torch.empty(4, dtype=torch.float32, device=self.device)
        check(self.lib.rl4rs_rawtrain_loss_grad(self.h, algo, N, _ptr(cat), _ptr(dense), sp, _ptr(mask_bits), _ptr(actions), _ptr(adv),
                                                _ptr(ret), _ptr(old_logp), _ptr(old_value), _ptr(old_logits), vf_coeff, ent_coeff,
                                                clip, vf_clip, kl_coeff, _ptr(stats), _stream()))
        return stats

    def adam_step(self, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, grad_clip=0.0):
        check(self.lib.rl4rs_rawtrain_adam_step(self.h, lr, beta1, beta2, eps, grad_clip, _stream()))

    # ---- DQN on the raw handle (rl4rs_rawstate_* / rl4rs_rawtrain_dqn_loss_grad / _greedy / _adam_step_clip_by_var)
    @property
    def n_params(self):
        return self._ptrs()[2]

    @property
    def record_words(self):
        """REC: 32-bit words of one packed raw-state record [dense | cat | seq_0 .. | zero pad to a multiple of 4]."""
        return int(self.lib.rl4rs_rawstate_record_words(C.byref(self._cfg)))

    def pack_records(self, cat, dense, seqs, out=None):
        """The raw features of N rows as packed records float32 [N, REC] (the ids keep their int32 bit patterns)."""
        N, sp = self._inputs(cat, dense, seqs, None)
        REC = self.record_words
        rec = out if out is not None else torch.empty((N, REC), dtype=torch.float32, device=self.device)
        assert rec.dtype == torch.float32 and rec.shape == (N, REC) and rec.is_contiguous()
        check(self.lib.rl4rs_rawstate_pack(C.byref(self._cfg), N, _ptr(cat), _ptr(dense), sp, _ptr(rec), _stream()))
        return rec

    def dqn_loss_grad(self, target, rec, action, reward, done, next_rec, next_mask=None, weights=None, gamma=1.0, double_q=True,
                      td_out=None, want_next_action=False):
        """(Double-)DQN Huber loss on packed records (rl4rs_rawtrain_dqn_loss_grad); ``target``: float32 [n_params] in the flat
        layout.  The gradient stays in the handle (gradients() / flat_view('grad')).
        -> (td [N], stats[4] sums of {w * huber, Q(s)[a], y, |td|}, a* [N] or None)."""
        N, REC = rec.shape[0], self.record_words
        for t in (target, rec, reward, next_rec) + ((weights,) if weights is not None else ()):
            assert t.dtype == torch.float32 and t.is_contiguous()
        assert action.dtype == torch.int32 and done.dtype == torch.int32 and action.is_contiguous() and done.is_contiguous()
        assert target.numel() == self.n_params and rec.shape == (N, REC) and next_rec.shape == (N, REC)
        assert action.shape == (N,) and reward.shape == (N,) and done.shape == (N,) and (weights is None or weights.shape == (N,))
        if next_mask is not None:
            assert next_mask.dtype == torch.int32 and next_mask.shape == (N, self.W) and next_mask.is_contiguous()
        td = td_out if td_out is not None else torch.empty(N, dtype=torch.float32, device=self.device)
        assert td.dtype == torch.float32 and td.shape == (N,) and td.is_contiguous()
        stats = torch.empty(4, dtype=torch.float32, device=self.device)
        astar = torch.empty(N, dtype=torch.int32, device=self.device) if want_next_action else None
        check(self.lib.rl4rs_rawtrain_dqn_loss_grad(self.h, _ptr(target), N, _ptr(rec), _ptr(action), _ptr(reward), _ptr(done),
                                                    _ptr(next_rec), _ptr(next_mask), _ptr(weights), gamma, 1 if double_q else 0, _ptr(td),
                                                    _ptr(astar), _ptr(stats), _stream()))
        return td, stats, astar

    def greedy(self, cat, dense, seqs, mask_bits=None, want_q=False, out=None):
        """First maximum of the masked Q row (rl4rs_rawtrain_greedy) -> (actions int32 [N], masked Q [N, A] or None)."""
        N, sp = self._inputs(cat, dense, seqs, mask_bits)
        a = out if out is not None else torch.empty(N, dtype=torch.int32, device=self.device)
        assert a.dtype == torch.int32 and a.shape == (N,) and a.is_contiguous()
        q = torch.empty((N, self.A), dtype=torch.float32, device=self.device) if want_q else None
        check(self.lib.rl4rs_rawtrain_greedy(self.h, N, _ptr(cat), _ptr(dense), sp, _ptr(mask_bits), _ptr(a), _ptr(q), _stream()))
        return a, q

    def adam_step_clip_by_var(self, lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-8, var_clip=40.0):
        """Adam on the handle's gradient with each of the ten variables clipped by its own norm."""
        check(self.lib.rl4rs_rawtrain_adam_step_clip_by_var(self.h, lr, beta1, beta2, eps, var_clip, _stream()))

    def set_profiling(self, on):
        check(self.lib.rl4rs_rawtrain_set_profiling(self.h, 1 if on else 0))

    def profile(self):
        """Event times of the last dqn_loss_grad and adam_step_clip_by_var, microseconds by stage (waits for both)."""
        ms = (C.c_float * 5)()
        check(self.lib.rl4rs_rawtrain_profile(self.h, ms))
        return dict(zip(('forwards', 'rows', 'backward', 'sumsq', 'adam'), [1e3 * float(x) for x in ms]))


def gemm_f32(a, w, bias=None, act=0):
    """C = act(a @ w + bias) through rl4rs_gemm_f32 (tests)."""
    lib = _lib.load()
    M, K = a.shape
    K2, N = w.shape
    assert K == K2
    c = torch.empty((M, N), dtype=torch.float32, device=a.device)
    check(lib.rl4rs_gemm_f32(_ptr(a), a.stride(0), _ptr(w), w.stride(0), _ptr(bias), _ptr(c), N, M, N, K, act, _stream()))
    return c


def gemm_f32_packed(a, w_host, bias=None, act=0):
    """Same through the packed-weight kernel (w_host: numpy [K,N] float32)."""
    lib = _lib.load()
    M, K = a.shape
    w_host = np.ascontiguousarray(w_host, dtype=np.float32)
    K2, N = w_host.shape
    assert K == K2
    c = torch.empty((M, N), dtype=torch.float32, device=a.device)
    check(lib.rl4rs_gemm_f32_packed(_ptr(a), a.stride(0), w_host.ctypes.data_as(C.c_void_p), N, _ptr(bias), _ptr(c), N,
                                    M, N, K, act, _stream()))
    return c


def gemm_h16_packed(a, w_host, bias=None, act=0):
    """The fp16x2 form (operands as fp16 hi + lo pairs, three f16 MFMAs per product) of the packed-weight GEMM."""
    lib = _lib.load()
    M, K = a.shape
    w_host = np.ascontiguousarray(w_host, dtype=np.float32)
    K2, N = w_host.shape
    assert K == K2
    c = torch.empty((M, N), dtype=torch.float32, device=a.device)
    check(lib.rl4rs_gemm_h16_packed(_ptr(a), a.stride(0), w_host.ctypes.data_as(C.c_void_p), N, _ptr(bias), _ptr(c), N,
                                    M, N, K, act, _stream()))
    return c


def vtrace(behaviour_logp, target_logp, values, rewards, bootstrap_value=None, dones=None, gamma=1.0, clip_rho=1.0, clip_pg_rho=1.0,
           want_stats=True):
    """V-trace targets of time-major [T, B] device tensors (rl4rs_vtrace): log-probs / values float32, rewards float64,
    bootstrap_value float32 [B] or None (zeros), dones int32 or None.
    -> (vs [T, B], pg_adv [T, B], stats float64 [4] sums of {rho, min(rho, clip_rho), vs, pg_adv} or None)."""
    lib = _lib.load()
    T, B = values.shape
    for t in (behaviour_logp, target_logp, values):
        assert t.dtype == torch.float32 and tuple(t.shape) == (T, B) and t.is_contiguous() and t.is_cuda
    assert rewards.dtype == torch.float64 and tuple(rewards.shape) == (T, B) and rewards.is_contiguous()
    assert bootstrap_value is None or (bootstrap_value.dtype == torch.float32 and tuple(bootstrap_value.shape) == (B,)
                                       and bootstrap_value.is_contiguous())
    assert dones is None or (dones.dtype == torch.int32 and tuple(dones.shape) == (T, B) and dones.is_contiguous())
    vs = torch.empty((T, B), dtype=torch.float32, device=values.device)
    pg = torch.empty((T, B), dtype=torch.float32, device=values.device)
    stats = torch.empty(4, dtype=torch.float64, device=values.device) if want_stats else None
    with torch.cuda.device(values.device):
        check(lib.rl4rs_vtrace(T, B, _ptr(behaviour_logp), _ptr(target_logp), _ptr(values), _ptr(bootstrap_value), _ptr(rewards),
                               _ptr(dones), gamma, clip_rho, clip_pg_rho, _ptr(vs), _ptr(pg), _ptr(stats), _stream()))
    return vs, pg, stats


def _ope_outputs(N, A, device, logged, pi, q, actions_out, masked_out):
    """The outputs of one OPE step: fresh tensors, the caller's, or (pi / q) a device address -> (actions, pi, q, pi pointer, q pointer)."""
    assert logged is None or (logged.dtype == torch.int32 and logged.shape == (N,) and logged.is_contiguous() and logged.is_cuda)
    a = actions_out if actions_out is not None else torch.empty(N, dtype=torch.int32, device=device)
    assert a.dtype == torch.int32 and a.shape == (N,) and a.is_contiguous() and a.is_cuda
    assert masked_out is None or (masked_out.dtype == torch.float32 and tuple(masked_out.shape) == (N, A) and masked_out.is_contiguous()
                                  and masked_out.is_cuda)
    ptrs = []
    cols = []
    for col, needed in ((pi, logged is not None), (q, True)):
        if isinstance(col, int):
            ptrs.append(C.c_void_p(col))
            cols.append(None)
            continue
        if col is None and needed:
            col = torch.empty(N, dtype=torch.float64, device=device)
        assert col is None or (col.dtype == torch.float64 and col.shape == (N,) and col.is_contiguous() and col.is_cuda)
        ptrs.append(_ptr(col))
        cols.append(col)
    return a, cols[0], cols[1], ptrs[0], ptrs[1]


def ope_greedy_rows(scores, logged, mask_bits=None, mask_set=0, value=None, pi=None, q=None, actions_out=None, masked_out=None):
    """One OPE step of a score matrix (rl4rs_ope_greedy_rows): ``scores`` float32 [N, A] device tensor whose rows may be a view of a
    wider matrix (unit column stride), ``mask_bits`` int32 [N, (A + 31) // 32] or None, ``mask_set`` 0 (a forbidden column gets
    -3.4e38 added) or 1 (it is set to -3.4e38), ``value`` float32 [N] (any stride) or None -> (first-maximum actions int32 [N], pi
    float64 [N] = softmax(masked row)[logged], q float64 [N] = value, or the masked score of the chosen action).  ``pi`` / ``q`` /
    ``actions_out`` / ``masked_out`` as in ``DevicePolicy.ope_step``."""
    assert scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 2 and scores.stride(1) == 1
    N, A = scores.shape
    W = (A + 31) // 32
    assert mask_bits is None or (mask_bits.dtype == torch.int32 and tuple(mask_bits.shape) == (N, W) and mask_bits.is_contiguous())
    assert value is None or (value.is_cuda and value.dtype == torch.float32 and value.shape == (N,))
    a, pi, q, pi_p, q_p = _ope_outputs(N, A, scores.device, logged, pi, q, actions_out, masked_out)
    with torch.cuda.device(scores.device):
        check(_lib.load().rl4rs_ope_greedy_rows(N, _ptr(scores), A, scores.stride(0) if N > 1 else A, _ptr(mask_bits), int(mask_set),
                                                _ptr(logged), _ptr(value), value.stride(0) if value is not None and N > 1 else 1, _ptr(a),
                                                pi_p, q_p, _ptr(masked_out), _stream()))
    return a, pi, q


class DevicePolicy(_FlatNet):
    """rl4rs_policy handle: action-masked policy net (rllib_mask_model.py:7-64) with flat parameters."""
    A2C, PPO = 0, 1
    _prefix = 'rl4rs_policy_'

    def __init__(self, obs_dim, hidden, action_size, max_rows, params=None, seed=0, device=None):
        _lib.require_device()
        self.lib = _lib.load()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.obs_dim, self.hidden, self.action_size, self.max_rows = int(obs_dim), int(hidden), int(action_size), int(max_rows)
        self.n_params = self.lib.rl4rs_policy_param_count(self.obs_dim, self.hidden, self.action_size)
        if params is None:
            from .nets.policy import init_policy_params
            params = init_policy_params(self.obs_dim, self.hidden, self.action_size, seed)
        params = np.ascontiguousarray(params, dtype=np.float32)
        assert params.shape == (self.n_params,), (params.shape, self.n_params)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.rl4rs_policy_create(self.obs_dim, self.hidden, self.action_size, self.max_rows,
                                               params.ctypes.data_as(C.c_void_p), _stream(), C.byref(h)))
        self.h = h
        self.W = (self.action_size + 31) // 32
        # RL4RS_POLICY_OPTS="ppo_fused=0,ppo_rows=16": defaults for A/B runs, read here (the library never reads the environment)
        for item in filter(None, (x.strip() for x in os.environ.get('RL4RS_POLICY_OPTS', '').split(','))):
            k, _, v = item.partition('=')
            self.set_option(k.strip(), int(v))

    def set_option(self, name, value):
        """Kernel-path selection of this handle (rl4rs_policy_set_option): 'tile', 'ppo_fused', 'ppo_rows', 'resident_wgs', 'ppo_std'."""
        if name not in _lib.POLICY_OPTS:
            raise ValueError("unknown policy option %r; known: %s" % (name, sorted(_lib.POLICY_OPTS)))
        check(self.lib.rl4rs_policy_set_option(self.h, _lib.POLICY_OPTS[name], int(value)))

    def _ptrs(self):
        """rl4rs_policy_params has no gradient pointer (the gradient is the caller's buffer) and an int32 count"""
        p, n = C.c_void_p(), C.c_int32()
        check(self.lib.rl4rs_policy_params(self.h, C.byref(p), C.byref(n)))
        return p, None, n.value

    def _mask(self, mask_bits, N):
        if mask_bits is None:
            return None
        assert mask_bits.dtype == torch.int32 and mask_bits.shape == (N, self.W) and mask_bits.is_contiguous()
        return mask_bits

    def act(self, obs, mask_bits=None, seed=0, step=0, want_logits=False, out=None):
        """Sample actions.  ``out`` = (actions i32 [N], logp f32 [N], value f32 [N], logits f32 [N, A] or None): contiguous
        tensors to fill in place (slices of a rollout buffer) instead of fresh ones."""
        N = obs.shape[0]
        assert obs.dtype == torch.float32 and obs.shape == (N, self.obs_dim) and obs.is_contiguous()
        m = self._mask(mask_bits, N)
        if out is not None:
            a, lp, v, lg = out
            assert a.dtype == torch.int32 and lp.dtype == torch.float32 and v.dtype == torch.float32
            assert a.shape == (N,) and lp.shape == (N,) and v.shape == (N,) and a.is_contiguous() and lp.is_contiguous() and v.is_contiguous()
            assert lg is None or (lg.dtype == torch.float32 and tuple(lg.shape) == (N, self.action_size) and lg.is_contiguous())
        else:
            a = torch.empty(N, dtype=torch.int32, device=self.device)
            lp = torch.empty(N, dtype=torch.float32, device=self.device)
            v = torch.empty(N, dtype=torch.float32, device=self.device)
            lg = torch.empty((N, self.action_size), dtype=torch.float32, device=self.device) if want_logits else None
        ent = torch.empty(N, dtype=torch.float32, device=self.device)
        check(self.lib.rl4rs_policy_act(self.h, N, _ptr(obs), _ptr(m), seed & 0xffffffff, step & 0xffffffff, _ptr(a),
                                        _ptr(lp), _ptr(v), _ptr(ent), _ptr(lg), _stream()))
        return a, lp, v, ent, lg

    def evaluate(self, obs, actions, mask_bits=None, want_logits=False):
        N = obs.shape[0]
        m = self._mask(mask_bits, N)
        actions = actions.to(torch.int32).contiguous()
        lp = torch.empty(N, dtype=torch.float32, device=self.device)
        v = torch.empty(N, dtype=torch.float32, device=self.device)
        ent = torch.empty(N, dtype=torch.float32, device=self.device)
        lg = torch.empty((N, self.action_size), dtype=torch.float32, device=self.device) if want_logits else None
        check(self.lib.rl4rs_policy_evaluate(self.h, N, _ptr(obs), _ptr(m), _ptr(actions), _ptr(lp), _ptr(v), _ptr(ent),
                                             _ptr(lg), _stream()))
        return lp, v, ent, lg

    def loss_grad(self, algo, obs, actions, adv, ret, mask_bits=None, old_logp=None, old_value=None, old_logits=None,
                  vf_coeff=0.5, ent_coeff=0.01, clip=0.3, vf_clip=500.0, kl_coeff=0.2, grad_out=None):
        N = obs.shape[0]
        m = self._mask(mask_bits, N)
        g = grad_out if grad_out is not None else torch.empty(self.n_params, dtype=torch.float32, device=self.device)
        stats = torch.empty(4, dtype=torch.float32, device=self.device)
        f = lambda t: None if t is None else t.to(torch.float32).contiguous()
        actions = actions.to(torch.int32).contiguous()
        adv, ret, old_logp, old_value, old_logits = f(adv), f(ret), f(old_logp), f(old_value), f(old_logits)
        check(self.lib.rl4rs_policy_loss_grad(self.h, algo, N, _ptr(obs), _ptr(m), _ptr(actions), _ptr(adv), _ptr(ret),
                                              _ptr(old_logp), _ptr(old_value), _ptr(old_logits), vf_coeff, ent_coeff, clip,
                                              vf_clip, kl_coeff, _ptr(g), _ptr(stats), _stream()))
        return g, stats

    def ppo_epoch(self, obs, actions, adv, ret, mask_bits, old_logp, old_value, old_logits, minibatch=256, vf_coeff=0.5,
                  ent_coeff=0.0, clip=0.3, vf_clip=500.0, kl_coeff=0.2, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8,
                  grad_clip=0.0, grad_out=None):
        """One SGD pass over already shuffled samples (rl4rs_policy_ppo_epoch).  Returns 8 floats: [0:4] sums of
        {pi_loss, vf_loss, entropy, kl} over the last minibatch, [4:8] the same sums over every sample of the pass."""
        N = obs.shape[0]
        m = self._mask(mask_bits, N)
        g = grad_out if grad_out is not None else torch.empty(self.n_params, dtype=torch.float32, device=self.device)
        stats = torch.empty(8, dtype=torch.float32, device=self.device)
        f = lambda t: t.to(torch.float32).contiguous()
        obs, adv, ret, old_logp, old_value, old_logits = f(obs), f(adv), f(ret), f(old_logp), f(old_value), f(old_logits)
        actions = actions.to(torch.int32).contiguous()
        check(self.lib.rl4rs_policy_ppo_epoch(self.h, N, minibatch, _ptr(obs), _ptr(m), _ptr(actions), _ptr(adv), _ptr(ret),
                                              _ptr(old_logp), _ptr(old_value), _ptr(old_logits), vf_coeff, ent_coeff, clip,
                                              vf_clip, kl_coeff, lr, beta1, beta2, eps, grad_clip, _ptr(g), _ptr(stats),
                                              _stream()))
        return stats

    def ppo_minibatch_grad(self, mb_index, obs, actions, adv, ret, mask_bits, old_logp, old_value, old_logits, minibatch=256,
                           vf_coeff=0.5, ent_coeff=0.0, clip=0.3, vf_clip=500.0, kl_coeff=0.2, grad_out=None, stats_out=None):
        """Data-parallel form of the pass: gradient of minibatch ``mb_index`` of the shuffled samples, parameters untouched
        (rl4rs_policy_ppo_minibatch_grad).  All inputs must already be contiguous float32 / int32 device tensors of the whole
        pass (no per-call conversions: this runs once per minibatch).  -> (grad, stats[4] sums)."""
        N = obs.shape[0]
        g = grad_out if grad_out is not None else torch.empty(self.n_params, dtype=torch.float32, device=self.device)
        stats = stats_out if stats_out is not None else torch.empty(4, dtype=torch.float32, device=self.device)
        for t in (obs, adv, ret, old_logp, old_value, old_logits):
            assert t.dtype == torch.float32 and t.is_contiguous()
        assert actions.dtype == torch.int32 and actions.is_contiguous()
        m = self._mask(mask_bits, N)
        check(self.lib.rl4rs_policy_ppo_minibatch_grad(self.h, N, minibatch, mb_index, _ptr(obs), _ptr(m), _ptr(actions), _ptr(adv),
                                                       _ptr(ret), _ptr(old_logp), _ptr(old_value), _ptr(old_logits), vf_coeff,
                                                       ent_coeff, clip, vf_clip, kl_coeff, _ptr(g), _ptr(stats), _stream()))
        return g, stats

    def adam_step(self, grad, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, grad_clip=0.0):
        check(self.lib.rl4rs_policy_adam_step(self.h, _ptr(grad), lr, beta1, beta2, eps, grad_clip, _stream()))

    def dqn_loss_grad(self, target_params, obs, actions, rewards, dones, next_obs, next_mask_bits=None, weights=None, gamma=1.0,
                      double_q=True, grad_out=None, td_out=None, want_next_action=False):
        """(Double-)DQN Huber loss and gradient (rl4rs_policy_dqn_loss_grad).  All inputs are contiguous device tensors: obs /
        next_obs / rewards / weights float32, actions / dones int32, target_params float32 [n_params].
        -> (grad, td [N], stats[4] sums of {w * huber, Q(s)[a], y, |td|}, a* [N] or None)."""
        N = obs.shape[0]
        for t in (target_params, obs, rewards, next_obs) + ((weights,) if weights is not None else ()):
            assert t.dtype == torch.float32 and t.is_contiguous()
        assert actions.dtype == torch.int32 and dones.dtype == torch.int32 and actions.is_contiguous() and dones.is_contiguous()
        assert target_params.numel() == self.n_params and obs.shape == (N, self.obs_dim) and next_obs.shape == (N, self.obs_dim)
        assert actions.shape == (N,) and rewards.shape == (N,) and dones.shape == (N,) and (weights is None or weights.shape == (N,))
        m = self._mask(next_mask_bits, N)
        g = grad_out if grad_out is not None else torch.empty(self.n_params, dtype=torch.float32, device=self.device)
        td = td_out if td_out is not None else torch.empty(N, dtype=torch.float32, device=self.device)
        assert td.dtype == torch.float32 and td.shape == (N,) and td.is_contiguous()
        stats = torch.empty(4, dtype=torch.float32, device=self.device)
        astar = torch.empty(N, dtype=torch.int32, device=self.device) if want_next_action else None
        check(self.lib.rl4rs_policy_dqn_loss_grad(self.h, _ptr(target_params), N, _ptr(obs), _ptr(actions), _ptr(rewards), _ptr(dones),
                                                  _ptr(next_obs), _ptr(m), _ptr(weights), gamma, 1 if double_q else 0, _ptr(g), _ptr(td),
                                                  _ptr(astar), _ptr(stats), _stream()))
        return g, td, stats, astar

    def vtrace_loss_grad(self, R, T, B, obs, actions, behaviour_logp, rewards, mask_bits=None, dones=None, gamma=1.0, clip_rho=1.0,
                         clip_pg_rho=1.0, drop_last=True, vf_coeff=0.5, ent_coeff=0.01, grad_out=None, stats_out=None,
                         vtrace_stats_out=None, want_vtrace=False):
        """V-trace loss and gradient over R rollouts of [T, B] time-major rows (rl4rs_policy_vtrace_loss_grad).  All inputs are
        contiguous device tensors: obs / behaviour_logp float32, actions (and dones) int32, rewards float64.
        -> (grad, stats[4] sums of {policy loss, value loss, entropy, 0} over the kept rows, vtrace_stats float64 [4] sums of
        {rho, min(rho, clip_rho), vs, pg_adv}, (vs, pg_adv) float32 [R * T * B] or None)."""
        N = R * T * B
        assert obs.dtype == torch.float32 and obs.shape == (N, self.obs_dim) and obs.is_contiguous()
        assert actions.dtype == torch.int32 and actions.shape == (N,) and actions.is_contiguous()
        assert behaviour_logp.dtype == torch.float32 and behaviour_logp.shape == (N,) and behaviour_logp.is_contiguous()
        assert rewards.dtype == torch.float64 and rewards.shape == (N,) and rewards.is_contiguous()
        assert dones is None or (dones.dtype == torch.int32 and dones.shape == (N,) and dones.is_contiguous())
        m = self._mask(mask_bits, N)
        g = grad_out if grad_out is not None else torch.empty(self.n_params, dtype=torch.float32, device=self.device)
        stats = stats_out if stats_out is not None else torch.empty(4, dtype=torch.float32, device=self.device)
        vstats = vtrace_stats_out if vtrace_stats_out is not None else torch.empty(4, dtype=torch.float64, device=self.device)
        assert stats.dtype == torch.float32 and stats.numel() == 4 and vstats.dtype == torch.float64 and vstats.numel() == 4
        vs = torch.empty(N, dtype=torch.float32, device=self.device) if want_vtrace else None
        pg = torch.empty(N, dtype=torch.float32, device=self.device) if want_vtrace else None
        check(self.lib.rl4rs_policy_vtrace_loss_grad(self.h, R, T, B, _ptr(obs), _ptr(m), _ptr(actions), _ptr(behaviour_logp), _ptr(rewards),
                                                     _ptr(dones), gamma, clip_rho, clip_pg_rho, 1 if drop_last else 0, vf_coeff, ent_coeff,
                                                     _ptr(g), _ptr(stats), _ptr(vstats), _ptr(vs), _ptr(pg), _stream()))
        return g, stats, vstats, ((vs, pg) if want_vtrace else None)

    def copy_params_from(self, other):
        """This handle's parameters <- ``other``'s, a device-to-device copy (IMPALA's learner -> actor broadcast)."""
        src, _, n = other._ptrs()
        assert n == self.n_params
        check(self.lib.rl4rs_copy_d2d(self._ptrs()[0], src, n * 4, _stream()))

    def greedy(self, obs, mask_bits=None, want_q=False, out=None):
        """First maximum of the masked Q row (rl4rs_policy_greedy) -> (actions int32 [N], masked Q [N, A] or None)."""
        N = obs.shape[0]
        assert obs.dtype == torch.float32 and obs.shape == (N, self.obs_dim) and obs.is_contiguous()
        m = self._mask(mask_bits, N)
        a = out if out is not None else torch.empty(N, dtype=torch.int32, device=self.device)
        assert a.dtype == torch.int32 and a.shape == (N,) and a.is_contiguous()
        q = torch.empty((N, self.action_size), dtype=torch.float32, device=self.device) if want_q else None
        check(self.lib.rl4rs_policy_greedy(self.h, N, _ptr(obs), _ptr(m), _ptr(a), _ptr(q), _stream()))
        return a, q

    def ope_step(self, obs, mask_bits, logged, q_mode, pi=None, q=None, actions_out=None, masked_out=None):
        """One OPE step (rl4rs_policy_ope_step): two GEMMs and one row launch -> (greedy actions int32 [N], pi float64 [N] =
        softmax(masked logits)[logged], q float64 [N] = the masked Q of the chosen action (``q_mode`` 1) or the value head (0)).
        ``pi`` / ``q``: float64 [N] tensors to fill, or device addresses (a step of an ``OpeLog`` column; nothing is returned for
        them); ``masked_out``: float32 [N, A] to receive the masked row."""
        N = obs.shape[0]
        assert obs.dtype == torch.float32 and obs.shape == (N, self.obs_dim) and obs.is_contiguous()
        m = self._mask(mask_bits, N)
        a, pi, q, pi_p, q_p = _ope_outputs(N, self.action_size, self.device, logged, pi, q, actions_out, masked_out)
        check(self.lib.rl4rs_policy_ope_step(self.h, N, _ptr(obs), _ptr(m), _ptr(logged), int(q_mode), _ptr(a), pi_p, q_p, _ptr(masked_out),
                                             _stream()))
        return a, pi, q

    def adam_step_clip_by_var(self, grad, lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-8, var_clip=40.0):
        """Adam with every variable (W1, b1, W2e, b2e) clipped by its own norm (rl4rs_policy_adam_step_clip_by_var)."""
        check(self.lib.rl4rs_policy_adam_step_clip_by_var(self.h, _ptr(grad), lr, beta1, beta2, eps, var_clip, _stream()))

    def check_status(self):
        """Synchronises; raises if a persistent PPO pass gave up at a grid barrier (its workgroups were not co-resident)."""
        f = C.c_int32()
        check(self.lib.rl4rs_policy_status(self.h, C.byref(f), _stream()))
        if f.value & 1:
            raise RuntimeError("the persistent PPO pass timed out at a grid barrier (workgroups not co-resident: the GPU is shared or "
                               "partitioned); the pass is incomplete - use DevicePolicy.set_option('ppo_fused', 0) for the per-minibatch kernels")

    def status_words(self):
        """int32 [2] tensor aliasing the handle's status words (word 1 != 0: a persistent pass timed out); no synchronisation."""
        if getattr(self, '_status_words', None) is None:
            p = C.c_void_p()
            check(self.lib.rl4rs_policy_status_words(self.h, C.byref(p)))
            self._status_words = _alias_f32(p.value, 2, self.device, self).view(torch.int32)
        return self._status_words

    PASS_TIMEOUT_MESSAGE = ("the persistent PPO pass timed out at a grid barrier (workgroups not co-resident: the GPU is shared or "
                            "partitioned); the pass is incomplete - use DevicePolicy.set_option('ppo_fused', 0) for the per-minibatch kernels")


class DeviceGaussPolicy(_FlatNet):
    """rl4rs_gpolicy handle: the Gaussian actor-critic of the continuous on-policy learners (two tanh towers, a diagonal Gaussian
    over ``act_dim`` action components; rl4rs_amd/nets/gausspolicy.py has the flat layout)."""
    A2C, PPO = 0, 1
    _prefix = 'rl4rs_gpolicy_'

    def __init__(self, obs_dim, act_dim, max_rows, hidden=256, params=None, seed=0, device=None):
        from .nets import gausspolicy as G
        _lib.require_device()
        self.lib = _lib.load()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.obs_dim, self.hidden, self.act_dim, self.max_rows = int(obs_dim), int(hidden), int(act_dim), int(max_rows)
        self.n_params = int(self.lib.rl4rs_gpolicy_param_count(self.obs_dim, self.hidden, self.act_dim))
        self.shapes = G.shapes(self.obs_dim, self.act_dim, self.hidden)
        if params is None:
            params = G.init_gausspolicy_params(self.obs_dim, self.act_dim, self.hidden, seed)
        params = np.ascontiguousarray(params, dtype=np.float32)
        assert params.shape == (self.n_params,), (params.shape, self.n_params)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.rl4rs_gpolicy_create(self.obs_dim, self.hidden, self.act_dim, self.max_rows,
                                                params.ctypes.data_as(C.c_void_p), _stream(), C.byref(h)))
        self.h = h

    def _ptrs(self):
        p, g, n = _FlatNet._ptrs(self)
        return p, None, n                       # the gradient is the caller's buffer

    def _f32(self, t, shape):
        assert t.dtype == torch.float32 and tuple(t.shape) == tuple(shape) and t.is_contiguous() and t.is_cuda, (t.dtype, t.shape, shape)
        return t

    def _new(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    def act(self, obs, seed=0, step=0, deterministic=False, want_head=False, want_eps=False, out=None):
        """Draw actions (one launch).  ``out`` = (action [N, E], env_action [N, E], logp [N], value [N], head [N, 2E] or None):
        contiguous tensors to fill in place (slices of a rollout buffer).
        -> (action, env_action = clip(action, -1, 1), logp, value, entropy, head or None, eps or None)."""
        N, E = obs.shape[0], self.act_dim
        self._f32(obs, (N, self.obs_dim))
        if out is not None:
            a, ea, lp, v, hd = out
            self._f32(a, (N, E)); self._f32(ea, (N, E)); self._f32(lp, (N,)); self._f32(v, (N,))
            if hd is not None:
                self._f32(hd, (N, 2 * E))
        else:
            a, ea, lp, v = self._new(N, E), self._new(N, E), self._new(N), self._new(N)
            hd = self._new(N, 2 * E) if want_head else None
        ent = self._new(N)
        eps = self._new(N, E) if want_eps else None
        check(self.lib.rl4rs_gpolicy_act(self.h, N, _ptr(obs), seed & 0xffffffff, step & 0xffffffff, 1 if deterministic else 0, _ptr(a),
                                         _ptr(ea), _ptr(lp), _ptr(v), _ptr(ent), _ptr(hd), _ptr(eps), _stream()))
        return a, ea, lp, v, ent, hd, eps

    def evaluate(self, obs, actions, want_head=False):
        """-> (logp, value, entropy, head or None) of given (unclipped) actions [N, E]"""
        N, E = obs.shape[0], self.act_dim
        self._f32(obs, (N, self.obs_dim)); self._f32(actions, (N, E))
        lp, v, ent = self._new(N), self._new(N), self._new(N)
        hd = self._new(N, 2 * E) if want_head else None
        check(self.lib.rl4rs_gpolicy_evaluate(self.h, N, _ptr(obs), _ptr(actions), _ptr(lp), _ptr(v), _ptr(ent), _ptr(hd), _stream()))
        return lp, v, ent, hd

    def loss_grad(self, algo, obs, actions, adv, ret, old_logp=None, old_value=None, old_head=None, vf_coeff=0.5, ent_coeff=0.01,
                  clip=0.3, vf_clip=500.0, kl_coeff=0.2, grad_out=None, stats_out=None):
        """-> (flat gradient, stats[4] sums of {policy loss, value loss, entropy, kl})"""
        N = obs.shape[0]
        g = grad_out if grad_out is not None else self._new(self.n_params)
        stats = stats_out if stats_out is not None else self._new(4)
        f = lambda t: None if t is None else t.to(torch.float32).contiguous()
        obs, actions, adv, ret, old_logp, old_value, old_head = f(obs), f(actions), f(adv), f(ret), f(old_logp), f(old_value), f(old_head)
        check(self.lib.rl4rs_gpolicy_loss_grad(self.h, algo, N, _ptr(obs), _ptr(actions), _ptr(adv), _ptr(ret), _ptr(old_logp),
                                               _ptr(old_value), _ptr(old_head), vf_coeff, ent_coeff, clip, vf_clip, kl_coeff, _ptr(g),
                                               _ptr(stats), _stream()))
        return g, stats

    def ppo_epoch(self, obs, actions, adv, ret, old_logp, old_value, old_head, minibatch=256, vf_coeff=0.5, ent_coeff=0.0, clip=0.3,
                  vf_clip=500.0, kl_coeff=0.2, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, grad_clip=0.0, grad_out=None):
        """One SGD pass over already shuffled rows (rl4rs_gpolicy_ppo_epoch).  Returns 8 floats: [0:4] sums of
        {pi_loss, vf_loss, entropy, kl} over the last minibatch, [4:8] the same sums over every row of the pass."""
        N = obs.shape[0]
        g = grad_out if grad_out is not None else self._new(self.n_params)
        stats = self._new(8)
        f = lambda t: t.to(torch.float32).contiguous()
        obs, actions, adv, ret, old_logp, old_value, old_head = f(obs), f(actions), f(adv), f(ret), f(old_logp), f(old_value), f(old_head)
        check(self.lib.rl4rs_gpolicy_ppo_epoch(self.h, N, minibatch, _ptr(obs), _ptr(actions), _ptr(adv), _ptr(ret), _ptr(old_logp),
                                               _ptr(old_value), _ptr(old_head), vf_coeff, ent_coeff, clip, vf_clip, kl_coeff, lr, beta1,
                                               beta2, eps, grad_clip, _ptr(g), _ptr(stats), _stream()))
        return stats

    def ppo_minibatch_grad(self, mb_index, obs, actions, adv, ret, old_logp, old_value, old_head, minibatch=256, vf_coeff=0.5,
                           ent_coeff=0.0, clip=0.3, vf_clip=500.0, kl_coeff=0.2, grad_out=None, stats_out=None):
        """Data-parallel form of the pass: the gradient of minibatch ``mb_index`` of the shuffled rows, parameters untouched - the
        loss of rl4rs_gpolicy_loss_grad on that row range, which is what rl4rs_gpolicy_ppo_epoch runs per minibatch.  Inputs are
        contiguous float32 device tensors of the whole pass.  -> (grad, stats[4] sums)."""
        lo, hi = mb_index * minibatch, (mb_index + 1) * minibatch
        assert 0 <= lo and hi <= obs.shape[0]
        for t in (obs, actions, adv, ret, old_logp, old_value, old_head):
            assert t.dtype == torch.float32 and t.is_contiguous()
        return self.loss_grad(self.PPO, obs[lo:hi], actions[lo:hi], adv[lo:hi], ret[lo:hi], old_logp[lo:hi], old_value[lo:hi],
                              old_head[lo:hi], vf_coeff, ent_coeff, clip, vf_clip, kl_coeff, grad_out, stats_out)

    def adam_step(self, grad, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, grad_clip=0.0):
        check(self.lib.rl4rs_gpolicy_adam_step(self.h, _ptr(grad), lr, beta1, beta2, eps, grad_clip, _stream()))

    def vtrace_loss_grad(self, R, T, B, obs, actions, behaviour_logp, rewards, gamma=1.0, clip_rho=1.0, clip_pg_rho=1.0, drop_last=True,
                         vf_coeff=0.5, ent_coeff=0.01, grad_out=None, stats_out=None, vtrace_stats_out=None):
        """V-trace loss and gradient over R rollouts of [T, B] time-major rows (rl4rs_gpolicy_vtrace_loss_grad): obs / actions /
        behaviour_logp float32, rewards float64.  -> (grad, stats[4] sums of {policy loss, value loss, entropy, 0} over the kept
        rows, vtrace_stats float64 [4] sums of {rho, min(rho, clip_rho), vs, pg_adv})."""
        N = R * T * B
        self._f32(obs, (N, self.obs_dim)); self._f32(actions, (N, self.act_dim)); self._f32(behaviour_logp, (N,))
        assert rewards.dtype == torch.float64 and rewards.shape == (N,) and rewards.is_contiguous()
        g = grad_out if grad_out is not None else self._new(self.n_params)
        stats = stats_out if stats_out is not None else self._new(4)
        vstats = vtrace_stats_out if vtrace_stats_out is not None else torch.empty(4, dtype=torch.float64, device=self.device)
        assert stats.dtype == torch.float32 and stats.numel() == 4 and vstats.dtype == torch.float64 and vstats.numel() == 4
        check(self.lib.rl4rs_gpolicy_vtrace_loss_grad(self.h, R, T, B, _ptr(obs), _ptr(actions), _ptr(behaviour_logp), _ptr(rewards), gamma,
                                                      clip_rho, clip_pg_rho, 1 if drop_last else 0, vf_coeff, ent_coeff, _ptr(g),
                                                      _ptr(stats), _ptr(vstats), _stream()))
        return g, stats, vstats

    def copy_params_from(self, other):
        """This handle's parameters <- ``other``'s, a device-to-device copy (IMPALA's learner -> actor broadcast)."""
        self.copy_from(other)


class DeviceReplay(object):
    """rl4rs_replay handle: a ring of whole rollouts on the device with uniform / proportional-prioritized sampling."""
    _DTYPES = {'obs': torch.float32, 'mask': torch.int32, 'action': torch.int32, 'reward': torch.float32, 'done': torch.int32,
               'priority': torch.float64, 'max_priority': torch.float64}

    def __init__(self, obs_dim, action_size, max_steps, batch_size, buffer_size=100000, alpha=0.6, device=None):
        _lib.require_device()
        self.lib = _lib.load()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.obs_dim, self.action_size, self.T, self.B = int(obs_dim), int(action_size), int(max_steps), int(batch_size)
        self.W = (self.action_size + 31) // 32
        self.alpha = float(alpha)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.rl4rs_replay_create(self.obs_dim, self.action_size, self.T, self.B, int(buffer_size), self.alpha, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, 'h', None) is not None and self.h:
            self.lib.rl4rs_replay_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def counts(self):
        """(filled rows, capacity in rows, rollouts pushed so far): host bookkeeping, no synchronisation."""
        n, cap, pushes = C.c_int32(), C.c_int32(), C.c_int64()
        check(self.lib.rl4rs_replay_rows(self.h, C.byref(n), C.byref(cap), C.byref(pushes)))
        return n.value, cap.value, pushes.value

    @property
    def rows(self):
        return self.counts()[0]

    def _buffer(self, name):
        p, n = C.c_void_p(), C.c_int64()
        check(self.lib.rl4rs_replay_buffer(self.h, _lib.REPLAY_BUFS[name], C.byref(p), C.byref(n)))
        return p, n.value

    def column(self, name):
        """Copy of one column of the whole ring (capacity rows; ``max_priority``: one float64)."""
        p, n = self._buffer(name)
        out = torch.empty(n, dtype=self._DTYPES[name], device=self.device)
        check(self.lib.rl4rs_copy_d2d(_ptr(out), p, n * out.element_size(), _stream()))
        cap = self.counts()[1]
        return out.view(cap, -1) if name in ('obs', 'mask') else out

    def set_priorities(self, values):
        """Overwrite the first len(values) priorities (tests: a buffer with known priorities)."""
        v = values.to(device=self.device, dtype=torch.float64).contiguous()
        p, n = self._buffer('priority')
        assert v.numel() <= n
        check(self.lib.rl4rs_copy_d2d(p, _ptr(v), v.numel() * 8, _stream()))
        self._keep = v

    def push(self, obs, mask_bits, actions, rewards):
        """One rollout: obs f32 [T * B, obs_dim], mask words i32 [T * B, W], actions i32, rewards f64, all in row order t * B + b."""
        R = self.T * self.B
        assert obs.dtype == torch.float32 and obs.shape == (R, self.obs_dim) and obs.is_contiguous()
        assert mask_bits.dtype == torch.int32 and mask_bits.shape == (R, self.W) and mask_bits.is_contiguous()
        assert actions.dtype == torch.int32 and actions.shape == (R,) and actions.is_contiguous()
        assert rewards.dtype == torch.float64 and rewards.shape == (R,) and rewards.is_contiguous()
        check(self.lib.rl4rs_replay_push(self.h, _ptr(obs), _ptr(mask_bits), _ptr(actions), _ptr(rewards), _stream()))

    def new_batch(self, M, want_u=False):
        """Minibatch buffers for ``sample(out=...)``."""
        dev = self.device
        b = dict(obs=torch.empty((M, self.obs_dim), dtype=torch.float32, device=dev),
                 next_obs=torch.empty((M, self.obs_dim), dtype=torch.float32, device=dev),
                 next_mask=torch.empty((M, self.W), dtype=torch.int32, device=dev),
                 action=torch.empty(M, dtype=torch.int32, device=dev), reward=torch.empty(M, dtype=torch.float32, device=dev),
                 done=torch.empty(M, dtype=torch.int32, device=dev), idx=torch.empty(M, dtype=torch.int32, device=dev),
                 weight=torch.empty(M, dtype=torch.float32, device=dev))
        b['u'] = torch.empty(M, dtype=torch.float32, device=dev) if want_u else None
        return b

    def sample(self, M, prioritized=True, beta=0.4, seed=0, step=0, out=None, want_u=False, n_step=1, gamma=1.0):
        """Draw and gather M rows (rl4rs_replay_sample) -> dict obs, next_obs, next_mask, action, reward, done, idx, weight, u.
        ``n_step`` > 1 (rl4rs_replay_sample_nstep): the same draw with RLlib's adjust_nstep - reward = the discounted sum of the
        next min(n_step, T - t) rewards, done = (t + n_step >= T), successor = that many steps on."""
        b = out if out is not None else self.new_batch(M, want_u)
        assert b['obs'].shape[0] == M
        if int(n_step) != 1:
            check(self.lib.rl4rs_replay_sample_nstep(self.h, M, int(n_step), float(gamma), 1 if prioritized else 0, float(beta),
                                                     seed & 0xffffffff, step & 0xffffffff, _ptr(b['obs']), _ptr(b['next_obs']),
                                                     _ptr(b['next_mask']), _ptr(b['action']), _ptr(b['reward']), _ptr(b['done']),
                                                     _ptr(b['idx']), _ptr(b['weight']), _ptr(b.get('u')), _stream()))
            return b
        check(self.lib.rl4rs_replay_sample(self.h, M, 1 if prioritized else 0, float(beta), seed & 0xffffffff, step & 0xffffffff,
                                           _ptr(b['obs']), _ptr(b['next_obs']), _ptr(b['next_mask']), _ptr(b['action']), _ptr(b['reward']),
                                           _ptr(b['done']), _ptr(b['idx']), _ptr(b['weight']), _ptr(b.get('u')), _stream()))
        return b

    def update_priorities(self, idx, td):
        M = idx.shape[0]
        assert idx.dtype == torch.int32 and td.dtype == torch.float32 and td.shape == (M,) and idx.is_contiguous() and td.is_contiguous()
        check(self.lib.rl4rs_replay_update_priorities(self.h, M, _ptr(idx), _ptr(td), _stream()))

    def max_priority(self):
        """The largest |td| + 1e-6 ever set (1.0 at start); waits for the stream."""
        return float(self.column('max_priority').cpu()[0])


class DeviceDistQ(_FlatNet):
    """rl4rs_distq handle: the dueling distributional (C51) Q network of Rainbow with flat parameters
    W1, b1, W2, b2, Wa1, ba1, Wa2, ba2 [, Wv1, bv1, Wv2, bv2] (include/rl4rs_hip.h, "On-device Rainbow").  RLlib parity is
    unpinned (ray is absent).  ``params``: flat float32 host array, default ``init_distq_params(..., seed)``."""
    _prefix = 'rl4rs_distq_'

    def __init__(self, obs_dim, action_size, max_rows, num_atoms=8, v_min=0.0, v_max=1000.0, dueling=True, trunk=256, stream_hidden=128,
                 params=None, seed=0, device=None):
        _lib.require_device()
        self.lib = _lib.load()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.obs_dim, self.action_size, self.max_rows, self.num_atoms = int(obs_dim), int(action_size), int(max_rows), int(num_atoms)
        self.dueling, self.trunk, self.stream_hidden = bool(dueling), int(trunk), int(stream_hidden)
        self.v_min, self.v_max = float(v_min), float(v_max)
        self.cfg = _lib.DistqCfg(self.obs_dim, self.action_size, self.num_atoms, self.trunk, self.stream_hidden, 1 if self.dueling else 0,
                                 self.v_min, self.v_max, self.max_rows)
        n = self.lib.rl4rs_distq_param_count(C.byref(self.cfg))
        if n < 0:
            raise _lib.Rl4rsHipError(self.lib.rl4rs_last_error().decode())
        self.n_params = int(n)
        if params is None:
            from .nets.distq import init_distq_params
            params = init_distq_params(self.obs_dim, self.action_size, self.num_atoms, self.trunk, self.stream_hidden, self.dueling, seed)
        params = np.ascontiguousarray(params, dtype=np.float32)
        assert params.shape == (self.n_params,), (params.shape, self.n_params)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.rl4rs_distq_create(C.byref(self.cfg), params.ctypes.data_as(C.c_void_p), _stream(), C.byref(h)))
        self.h = h
        self.W = (self.action_size + 31) // 32

    def _mask(self, mask_bits, N):
        if mask_bits is None:
            return None
        assert mask_bits.dtype == torch.int32 and mask_bits.shape == (N, self.W) and mask_bits.is_contiguous()
        return mask_bits

    def _rows(self, obs, out):
        N = obs.shape[0]
        assert obs.dtype == torch.float32 and obs.shape == (N, self.obs_dim) and obs.is_contiguous()
        a = out if out is not None else torch.empty(N, dtype=torch.int32, device=self.device)
        assert a.dtype == torch.int32 and a.shape == (N,) and a.is_contiguous()
        return N, a

    def act(self, obs, mask_bits=None, temperature=1.0, seed=0, step=0, want_u=False, want_q=False, out=None):
        """SoftQ draw (rl4rs_distq_act) -> (actions int32 [N], u [N] or None, masked Q [N, A] or None)."""
        N, a = self._rows(obs, out)
        u = torch.empty(N, dtype=torch.float32, device=self.device) if want_u else None
        q = torch.empty((N, self.action_size), dtype=torch.float32, device=self.device) if want_q else None
        check(self.lib.rl4rs_distq_act(self.h, N, _ptr(obs), _ptr(self._mask(mask_bits, N)), float(temperature), seed & 0xffffffff,
                                       step & 0xffffffff, _ptr(a), _ptr(u), _ptr(q), _stream()))
        return a, u, q

    def greedy(self, obs, mask_bits=None, want_q=False, out=None):
        """First maximum of the masked Q row (rl4rs_distq_greedy) -> (actions int32 [N], masked Q [N, A] or None)."""
        N, a = self._rows(obs, out)
        q = torch.empty((N, self.action_size), dtype=torch.float32, device=self.device) if want_q else None
        check(self.lib.rl4rs_distq_greedy(self.h, N, _ptr(obs), _ptr(self._mask(mask_bits, N)), _ptr(a), _ptr(q), _stream()))
        return a, q

    def loss_grad(self, target_params, obs, actions, rewards, dones, next_obs, next_mask_bits=None, weights=None, gamma_n=1.0,
                  double_q=True, grad_out=None, td_out=None, want_next_action=False):
        """Categorical loss and gradient (rl4rs_distq_loss_grad).  All inputs are contiguous device tensors: obs / next_obs /
        rewards (the n-step return) / weights float32, actions / dones int32, target_params float32 [n_params]; gamma_n = gamma ^ n_step.
        -> (grad, td [N], stats[4] sums of {w * td, Q(s)[a], sum_i z_i m_i, td}, a* [N] or None)."""
        N = obs.shape[0]
        for t in (target_params, obs, rewards, next_obs) + ((weights,) if weights is not None else ()):
            assert t.dtype == torch.float32 and t.is_contiguous()
        assert actions.dtype == torch.int32 and dones.dtype == torch.int32 and actions.is_contiguous() and dones.is_contiguous()
        assert target_params.numel() == self.n_params and obs.shape == (N, self.obs_dim) and next_obs.shape == (N, self.obs_dim)
        assert actions.shape == (N,) and rewards.shape == (N,) and dones.shape == (N,) and (weights is None or weights.shape == (N,))
        m = self._mask(next_mask_bits, N)
        g = grad_out if grad_out is not None else torch.empty(self.n_params, dtype=torch.float32, device=self.device)
        assert g.dtype == torch.float32 and g.numel() == self.n_params and g.is_contiguous()
        td = td_out if td_out is not None else torch.empty(N, dtype=torch.float32, device=self.device)
        assert td.dtype == torch.float32 and td.shape == (N,) and td.is_contiguous()
        stats = torch.empty(4, dtype=torch.float32, device=self.device)
        astar = torch.empty(N, dtype=torch.int32, device=self.device) if want_next_action else None
        check(self.lib.rl4rs_distq_loss_grad(self.h, _ptr(target_params), N, _ptr(obs), _ptr(actions), _ptr(rewards), _ptr(dones),
                                             _ptr(next_obs), _ptr(m), _ptr(weights), float(gamma_n), 1 if double_q else 0, _ptr(g), _ptr(td),
                                             _ptr(astar), _ptr(stats), _stream()))
        return g, td, stats, astar

    def adam_step_clip_by_var(self, grad, lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-8, var_clip=40.0):
        """Adam with every variable clipped by its own norm (rl4rs_distq_adam_step_clip_by_var)."""
        check(self.lib.rl4rs_distq_adam_step_clip_by_var(self.h, _ptr(grad), lr, beta1, beta2, eps, var_clip, _stream()))

class DeviceContiReplay(DeviceReplay):
    """The same ring for the continuous-action env (rl4rs_replay_create_conti): ``DeviceReplay``'s methods with a float32 action
    column [act_dim] (``column('action')``) and no mask column.  The handle refuses the discrete push / sample."""
    _DTYPES = {'obs': torch.float32, 'action': torch.float32, 'reward': torch.float32, 'done': torch.int32, 'priority': torch.float64,
               'max_priority': torch.float64}

    def __init__(self, obs_dim, act_dim, max_steps, batch_size, buffer_size=100000, alpha=0.6, device=None):
        _lib.require_device()
        self.lib = _lib.load()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.obs_dim, self.act_dim, self.T, self.B = int(obs_dim), int(act_dim), int(max_steps), int(batch_size)
        self.alpha = float(alpha)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.rl4rs_replay_create_conti(self.obs_dim, self.act_dim, self.T, self.B, int(buffer_size), self.alpha, C.byref(h)))
        self.h = h

    def _buffer(self, name):
        return DeviceReplay._buffer(self, 'action_f32' if name == 'action' else name)

    def column(self, name):
        p, n = self._buffer(name)
        out = torch.empty(n, dtype=self._DTYPES[name], device=self.device)
        check(self.lib.rl4rs_copy_d2d(_ptr(out), p, n * out.element_size(), _stream()))
        cap = self.counts()[1]
        return out.view(cap, -1) if name in ('obs', 'action') else out

    def push(self, obs, actions, rewards):
        """One rollout: obs f32 [T * B, obs_dim], actions f32 [T * B, act_dim], rewards f64, all in row order t * B + b."""
        R = self.T * self.B
        assert obs.dtype == torch.float32 and obs.shape == (R, self.obs_dim) and obs.is_contiguous()
        assert actions.dtype == torch.float32 and actions.shape == (R, self.act_dim) and actions.is_contiguous()
        assert rewards.dtype == torch.float64 and rewards.shape == (R,) and rewards.is_contiguous()
        check(self.lib.rl4rs_replay_push_conti(self.h, _ptr(obs), _ptr(actions), _ptr(rewards), _stream()))

    def new_batch(self, M, want_u=False):
        dev = self.device
        b = dict(obs=torch.empty((M, self.obs_dim), dtype=torch.float32, device=dev),
                 next_obs=torch.empty((M, self.obs_dim), dtype=torch.float32, device=dev),
                 action=torch.empty((M, self.act_dim), dtype=torch.float32, device=dev),
                 reward=torch.empty(M, dtype=torch.float32, device=dev), done=torch.empty(M, dtype=torch.int32, device=dev),
                 idx=torch.empty(M, dtype=torch.int32, device=dev), weight=torch.empty(M, dtype=torch.float32, device=dev))
        b['u'] = torch.empty(M, dtype=torch.float32, device=dev) if want_u else None
        return b

    def sample(self, M, prioritized=True, beta=0.4, seed=0, step=0, out=None, want_u=False):
        """Draw and gather M rows (rl4rs_replay_sample_conti) -> dict obs, next_obs, action, reward, done, idx, weight, u."""
        b = out if out is not None else self.new_batch(M, want_u)
        assert b['obs'].shape[0] == M
        check(self.lib.rl4rs_replay_sample_conti(self.h, M, 1 if prioritized else 0, float(beta), seed & 0xffffffff, step & 0xffffffff,
                                                 _ptr(b['obs']), _ptr(b['next_obs']), _ptr(b['action']), _ptr(b['reward']), _ptr(b['done']),
                                                 _ptr(b['idx']), _ptr(b['weight']), _ptr(b.get('u')), _stream()))
        return b


class DeviceQNet(_FlatNet):
    """rl4rs_qnet handle: one offline-RL network (the reference's ``CustomVectorEncoder`` of rl4rs/nets/cql/encoder.py:9-67,
    or d3rlpy's plain ``VectorEncoder``, + d3rlpy's Linear head) with forward, backward and torch-style Adam on the device.
    ``params``: dict of float32 arrays stored [in, out]: fc1_w, fc1_b, (emb,) fc2_w, fc2_b, head_w, head_b."""
    _prefix = 'rl4rs_qnet_'

    def __init__(self, obs_dim, action_size, params, mask_size=0, emb_size=32, hidden1=256, hidden2=256, location_mask=None,
                 special_items=None, max_rows=256, device=None):
        _lib.require_device()
        self.lib = _lib.load()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.D, self.A, self.M, self.ES = int(obs_dim), int(action_size), int(mask_size), int(emb_size)
        self.H1, self.H2 = int(hidden1), int(hidden2)
        self.custom = self.M > 0
        self.max_rows = int(max_rows)
        f2 = self.H1 + self.M * self.ES if self.custom else self.H1
        n2 = self.A if self.custom else self.H2
        self.shapes = [('fc1_w', (self.D, self.H1)), ('fc1_b', (self.H1,))]
        if self.custom:
            self.shapes.append(('emb', (self.A, self.ES)))
        self.shapes += [('fc2_w', (f2, n2)), ('fc2_b', (n2,)), ('head_w', (n2, self.A)), ('head_b', (self.A,))]
        flat = []
        for name, shape in self.shapes:
            arr = np.ascontiguousarray(params[name], dtype=np.float32)
            if tuple(arr.shape) != tuple(shape):
                raise ValueError('qnet parameter %r has shape %r, expected %r' % (name, tuple(arr.shape), tuple(shape)))
            flat.append(arr.reshape(-1))
        flat = np.ascontiguousarray(np.concatenate(flat))
        loc = sp = None
        n_layers = 0
        if self.custom:
            loc = np.ascontiguousarray(np.asarray(location_mask) >= 0.5, dtype=np.uint8)
            if loc.ndim != 2 or loc.shape[1] != self.A:
                raise ValueError('location_mask must be [n_layers, action_size]')
            n_layers = loc.shape[0]
            sp = np.zeros(self.A, dtype=np.uint8)
            sp[np.asarray(list(special_items), dtype=np.int64)] = 1
        cfg = _lib.QNetCfg(self.D, self.A, self.M, self.ES, self.H1, 0 if self.custom else self.H2, n_layers, self.max_rows)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.rl4rs_qnet_create(C.byref(cfg), flat.ctypes.data_as(_lib._FP),
                                             loc.ctypes.data_as(C.c_void_p) if loc is not None else None,
                                             sp.ctypes.data_as(C.c_void_p) if sp is not None else None, _stream(), C.byref(h)))
        self.h = h
        self.n_params = int(flat.size)

    def check_status(self):
        flags = C.c_int32(0)
        check(self.lib.rl4rs_qnet_status(self.h, C.byref(flags), _stream()))
        if flags.value & 1:
            raise IndexError('offline-RL batch: an item id in an observation tail or an action is outside [0, action_size)')
        if flags.value & 2:
            raise IndexError('offline-RL batch: cur_step %% 9 // 3 selects a location_mask row that does not exist')

    def _obs(self, obs):
        obs = _dev_tensor(obs, torch.float32, self.device)
        if obs.dim() != 2 or obs.shape[1] != self.D or not 0 < obs.shape[0] <= self.max_rows:
            raise ValueError('obs must be [N <= %d, %d] (got %r)' % (self.max_rows, self.D, tuple(obs.shape)))
        return obs

    def forward(self, obs):
        """out [N, action_size]: Q values / imitator logits.  Keeps the activations for ``backward``."""
        obs = self._obs(obs)
        out = torch.empty((obs.shape[0], self.A), dtype=torch.float32, device=self.device)
        check(self.lib.rl4rs_qnet_forward(self.h, obs.shape[0], _ptr(obs), _ptr(out), _stream()))
        return out

    def backward(self, obs, dout):
        """Gradient of sum(out * dout) into the handle (after ``forward`` of the same rows)."""
        obs = self._obs(obs)
        dout = _dev_tensor(dout, torch.float32, self.device)
        assert tuple(dout.shape) == (obs.shape[0], self.A)
        check(self.lib.rl4rs_qnet_backward(self.h, obs.shape[0], _ptr(obs), _ptr(dout), _stream()))

    def adam_step(self, lr, beta1=0.9, beta2=0.999, eps=1e-8):
        check(self.lib.rl4rs_qnet_adam_step(self.h, lr, beta1, beta2, eps, _stream()))

    def imitation_loss(self, logits, actions, beta):
        """(loss2 = [mean nll, mean_n sum_k logits^2], dlogits) of ``nll + beta * mean(logits^2)``."""
        N = logits.shape[0]
        actions = _dev_tensor(actions, torch.int32, self.device)
        d = torch.empty_like(logits)
        rows = torch.empty((N, 2), dtype=torch.float32, device=self.device)
        loss2 = torch.empty(2, dtype=torch.float32, device=self.device)
        check(self.lib.rl4rs_qloss_imitation(self.h, N, _ptr(logits), _ptr(actions), beta, _ptr(d), _ptr(rows), _ptr(loss2), _stream()))
        return loss2, d

    def dqn_loss(self, q_t, actions, rewards, terminals, q_next, q_next_target, imitator_next=None, action_flexibility=0.3,
                 gamma=0.99, cql_alpha=0.0):
        """(loss2 = [mean huber TD, mean conservative], dq, best next action)."""
        N = q_t.shape[0]
        actions = _dev_tensor(actions, torch.int32, self.device)
        rewards = _dev_tensor(rewards, torch.float32, self.device)
        terminals = _dev_tensor(terminals, torch.float32, self.device)
        dq = torch.empty_like(q_t)
        rows = torch.empty((N, 2), dtype=torch.float32, device=self.device)
        loss2 = torch.empty(2, dtype=torch.float32, device=self.device)
        best = torch.empty(N, dtype=torch.int32, device=self.device)
        check(self.lib.rl4rs_qloss_dqn(self.h, N, _ptr(q_t), _ptr(actions), _ptr(rewards), _ptr(terminals), _ptr(q_next),
                                       _ptr(q_next_target), _ptr(imitator_next), action_flexibility, gamma, cql_alpha, _ptr(dq),
                                       _ptr(rows), _ptr(loss2), _ptr(best), _stream()))
        return loss2, dq, best

    def best_action(self, q, imitator_logits=None, action_flexibility=0.3):
        out = torch.empty(q.shape[0], dtype=torch.int32, device=self.device)
        check(self.lib.rl4rs_q_best_action(q.shape[0], self.A, _ptr(q), _ptr(imitator_logits), action_flexibility, _ptr(out), _stream()))
        return out


class DeviceAMLP(_FlatNet):
    """rl4rs_amlp handle: d3rlpy's default continuous-control network - ``VectorEncoderWithAction([256, 256], relu)`` on
    ``cat([x, action])`` (``act_dim = 0``: plain ``VectorEncoder``) + one Linear head - with forward, backward (parameter and
    action-input gradients) and torch-style Adam on the device.  ``params``: dict of float32 arrays stored [in, out]:
    fc1_w [obs_dim + act_dim, hidden1] (observation rows first), fc1_b, fc2_w, fc2_b, head_w, head_b.
    ``head_act``: 'none' or 'tanh'.  The building block of the continuous BCQ / CQL learners (``offline_rl.BCQ`` / ``CQL``)."""

    HEAD_ACTS = {'none': 0, 'elu': 1, 'sigmoid': 2, 'tanh': 3, 'relu': 4}
    _prefix = 'rl4rs_amlp_'

    def __init__(self, obs_dim, act_dim, out_dim, params, hidden1=256, hidden2=256, head_act='none', max_rows=256, max_grad_rows=None,
                 device=None):
        _lib.require_device()
        self.lib = _lib.load()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.D, self.E, self.K, self.H1, self.H2 = int(obs_dim), int(act_dim), int(out_dim), int(hidden1), int(hidden2)
        self.max_rows = int(max_rows)
        self.max_grad_rows = self.max_rows if max_grad_rows is None else int(max_grad_rows)
        self.shapes = [('fc1_w', (self.D + self.E, self.H1)), ('fc1_b', (self.H1,)), ('fc2_w', (self.H1, self.H2)), ('fc2_b', (self.H2,)),
                       ('head_w', (self.H2, self.K)), ('head_b', (self.K,))]
        flat = []
        for name, shape in self.shapes:
            arr = np.ascontiguousarray(params[name], dtype=np.float32)
            if tuple(arr.shape) != tuple(shape):
                raise ValueError('amlp parameter %r has shape %r, expected %r' % (name, tuple(arr.shape), tuple(shape)))
            flat.append(arr.reshape(-1))
        flat = np.ascontiguousarray(np.concatenate(flat))
        cfg = _lib.AmlpCfg(self.D, self.E, self.H1, self.H2, self.K, self.HEAD_ACTS[head_act], self.max_rows, self.max_grad_rows)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.rl4rs_amlp_create(C.byref(cfg), flat.ctypes.data_as(_lib._FP), _stream(), C.byref(h)))
        self.h = h
        self.n_params = int(flat.size)
        self.h16_ok = bool(self.lib.rl4rs_amlp_h16_ok(self.h))

    def soft_update_from(self, other, tau):
        check(self.lib.rl4rs_amlp_soft_update(self.h, other.h, tau, _stream()))

    def check_status(self):
        pass

    def _rows(self, obs, act, rep):
        assert obs.is_cuda and obs.dtype == torch.float32 and obs.is_contiguous() and obs.shape[1] == self.D
        n = obs.shape[0] * rep
        if self.E:
            assert act.is_cuda and act.dtype == torch.float32 and act.is_contiguous() and tuple(act.shape) == (n, self.E), \
                (tuple(act.shape), n, self.E)
        return n

    H16_MIN_ROWS = 4096      # below this the fused fp16x2 forward has nothing to win over the small fp32 forms

    def forward(self, obs, act=None, rep=1, out=None, nograd=False):
        """out [N, out_dim] for obs [N / rep, obs_dim] (each observation shared by ``rep`` consecutive action rows) and act
        [N, act_dim].  Keeps the activations for ``backward``.  ``nograd='fp16x2'``: the rows will never see a backward and may be
        computed in the scorer's fp16x2 arithmetic - one fused launch for the three layers (rl4rs_amlp_forward_h16) when the
        network's shape has that form and there are at least ``H16_MIN_ROWS`` rows; anything else is the fp32 forward."""
        n = self._rows(obs, act, rep)
        if out is None:
            out = torch.empty((n, self.K), dtype=torch.float32, device=self.device)
        # (the fused kernel moves 16-byte vectors: an action view at an odd row offset takes the fp32 path, as documented)
        aligned = obs.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and (act is None or act.data_ptr() % 16 == 0)
        if nograd == 'fp16x2' and self.h16_ok and n >= self.H16_MIN_ROWS and aligned:
            check(self.lib.rl4rs_amlp_forward_h16(self.h, n, rep, _ptr(obs), _ptr(act), _ptr(out), _stream()))
        else:
            check(self.lib.rl4rs_amlp_forward(self.h, n, rep, _ptr(obs), _ptr(act), _ptr(out), _stream()))
        return out

    def backward(self, obs, act, dout, rep=1, want_dact=False, want_param_grad=True):
        """Given the gradient wrt the head's PRE-activation output: parameter gradients into the handle, returns the gradient
        wrt ``act`` when ``want_dact``."""
        n = self._rows(obs, act, rep)
        assert dout.is_cuda and dout.dtype == torch.float32 and dout.is_contiguous() and dout.numel() == n * self.K
        dact = torch.empty((n, self.E), dtype=torch.float32, device=self.device) if want_dact else None
        check(self.lib.rl4rs_amlp_backward(self.h, n, rep, _ptr(obs), _ptr(act), _ptr(dout), _ptr(dact), 1 if want_param_grad else 0,
                                           _stream()))
        return dact

    def adam_step(self, lr, beta1=0.9, beta2=0.999, eps=1e-8):
        check(self.lib.rl4rs_amlp_adam_step(self.h, lr, beta1, beta2, eps, _stream()))


def amlp_adam_multi(nets, lrs, targets=None, tau=0.0, step=None, beta1=0.9, beta2=0.999, eps=1e-8):
    """The optimiser of one phase of an update as ONE launch (rl4rs_amlp_adam_multi): torch Adam with learning rate ``lrs[i]`` for
    every ``nets[i]`` (``step[i]`` False: no step, soft update only) and, where ``targets[i]`` is given, the soft target update
    target = (1 - tau) target + tau net from the stepped parameters."""
    lib = _lib.load()
    n = len(nets)
    targets = list(targets) if targets is not None else [None] * n
    step = list(step) if step is not None else [True] * n
    H = (C.c_void_p * n)(*[net.h for net in nets])
    T = (C.c_void_p * n)(*[(t.h if t is not None else None) for t in targets])
    LR = (C.c_float * n)(*[float(x) for x in lrs])
    DO = (C.c_int32 * n)(*[1 if x else 0 for x in step])
    check(lib.rl4rs_amlp_adam_multi(n, H, LR, DO, T, beta1, beta2, eps, float(tau), _stream()))


def amlp_forward_multi(nets, obs, act=None):
    """``net.forward(obs, act)`` for several networks with the same input widths on the SAME rows - the twin critics - as ONE launch
    when the call has the fused form (rl4rs_amlp_forward_multi).  Returns the list of outputs; every network keeps its activations
    for a following backward."""
    lib = _lib.load()
    n0 = nets[0]
    N = n0._rows(obs, act, 1)
    outs = [torch.empty((N, net.K), dtype=torch.float32, device=net.device) for net in nets]
    H = (C.c_void_p * len(nets))(*[net.h for net in nets])
    O = (C.c_void_p * len(nets))(*[_ptr(o) for o in outs])
    check(lib.rl4rs_amlp_forward_multi(len(nets), H, N, _ptr(obs), _ptr(act), O, _stream()))
    return outs


def amlp_backward_multi(nets, obs, act, douts, want_dact=False, want_param_grad=True):
    """``net.backward(obs, act, dout)`` for the networks of ``amlp_forward_multi`` as one input-gradient launch + one parameter-
    gradient launch (rl4rs_amlp_backward_multi).  Returns the list of action-input gradients (or None)."""
    lib = _lib.load()
    n0 = nets[0]
    N = n0._rows(obs, act, 1)
    for net, d in zip(nets, douts):
        assert d.is_cuda and d.dtype == torch.float32 and d.is_contiguous() and d.numel() == N * net.K
    dacts = [torch.empty((N, net.E), dtype=torch.float32, device=net.device) for net in nets] if want_dact else None
    H = (C.c_void_p * len(nets))(*[net.h for net in nets])
    DO = (C.c_void_p * len(nets))(*[_ptr(d) for d in douts])
    DA = (C.c_void_p * len(nets))(*[_ptr(d) for d in dacts]) if want_dact else None
    check(lib.rl4rs_amlp_backward_multi(len(nets), H, N, _ptr(obs), _ptr(act), DO, DA, 1 if want_param_grad else 0, _stream()))
    return dacts


def amlp_set_fused(on):
    """Fused minibatch forward / backward of the amlp networks on (default), off, or 2 = their 8-rows-per-workgroup form
    (rl4rs_amlp_set_fused; tests and A/B runs)."""
    check(_lib.load().rl4rs_amlp_set_fused(2 if on == 2 else (1 if on else 0)))


def cvae_sample(enc_out, eps, min_logstd=-20.0, max_logstd=2.0):
    """z = mu + exp(clamp(logstd)) * eps for enc_out [N, 2L] = [mu | logstd]."""
    lib = _lib.load()
    N, L = eps.shape
    z = torch.empty_like(eps)
    check(lib.rl4rs_cvae_sample(N, L, _ptr(enc_out), _ptr(eps), min_logstd, max_logstd, _ptr(z), _stream()))
    return z


def cvae_loss(decoded, actions, enc_out, min_logstd=-20.0, max_logstd=2.0):
    """(loss2 = [mean_n sum_e (y - a)^2, mean_n sum_l KL], gradient of the mse term wrt the decoder's pre-tanh output)."""
    lib = _lib.load()
    N, E = decoded.shape
    L = enc_out.shape[1] // 2
    d = torch.empty_like(decoded)
    rows = torch.empty((N, 2), dtype=torch.float32, device=decoded.device)
    loss2 = torch.empty(2, dtype=torch.float32, device=decoded.device)
    check(lib.rl4rs_cvae_loss(N, E, L, _ptr(decoded), _ptr(actions), _ptr(enc_out), min_logstd, max_logstd, _ptr(d), _ptr(rows), _ptr(loss2),
                              _stream()))
    return loss2, d


def cvae_encoder_grad(enc_out, eps, dz, beta, min_logstd=-20.0, max_logstd=2.0):
    lib = _lib.load()
    N, L = eps.shape
    d = torch.empty_like(enc_out)
    check(lib.rl4rs_cvae_encoder_grad(N, L, _ptr(enc_out), _ptr(eps), _ptr(dz), beta, min_logstd, max_logstd, _ptr(d), _stream()))
    return d


def residual_action(action, tanh_out, scale):
    lib = _lib.load()
    N, E = action.shape
    out = torch.empty_like(action)
    check(lib.rl4rs_residual_action(N, E, _ptr(action), _ptr(tanh_out), scale, _ptr(out), _stream()))
    return out


def residual_grad(action, tanh_out, scale, d_out):
    lib = _lib.load()
    N, E = action.shape
    d = torch.empty_like(action)
    check(lib.rl4rs_residual_grad(N, E, _ptr(action), _ptr(tanh_out), scale, _ptr(d_out), _ptr(d), _stream()))
    return d


def bcq_target(q1, q2, n, lam, rewards=None, terminals=None, gamma=0.99, want_best=False):
    """(y [B], best [B] or None): max over the n sampled actions of the lam-weighted twin value (q2 None: of q1)."""
    lib = _lib.load()
    B = q1.numel() // n
    y = torch.empty(B, dtype=torch.float32, device=q1.device)
    best = torch.empty(B, dtype=torch.int32, device=q1.device) if want_best else None
    check(lib.rl4rs_bcq_target(B, n, _ptr(q1), _ptr(q2), lam, _ptr(rewards), _ptr(terminals), gamma, _ptr(y), _ptr(best), _stream()))
    return y, best


def pick_rows(rows, best, n):
    lib = _lib.load()
    B, E = best.numel(), rows.shape[1]
    out = torch.empty((B, E), dtype=torch.float32, device=rows.device)
    check(lib.rl4rs_pick_rows(B, n, E, _ptr(rows), _ptr(best), _ptr(out), _stream()))
    return out


def critic_mse(q1, q2, y):
    """(loss2 = [mean (q1 - y)^2, mean (q2 - y)^2], dq1, dq2)."""
    lib = _lib.load()
    N = y.numel()
    dq1, dq2 = torch.empty_like(q1), torch.empty_like(q2)
    loss2 = torch.empty(2, dtype=torch.float32, device=y.device)
    check(lib.rl4rs_critic_mse(N, _ptr(q1), _ptr(q2), _ptr(y), _ptr(dq1), _ptr(dq2), _ptr(loss2), _stream()))
    return loss2, dq1, dq2


def squashed_sample(head, eps, rep=1, act_out=None, logp_out=None, out_rep=None, out_off=0, min_logstd=-20.0, max_logstd=2.0):
    """d3rlpy SquashedNormalPolicy sampling from head [R, 2A] = [mu | logstd]: (actions, log-probs).  ``eps`` [R * rep, A] Gaussian
    noise, or None for the deterministic best_action tanh(mu).  ``act_out`` [rows, A] / ``logp_out`` [rows] with ``out_rep`` /
    ``out_off``: write sample i of observation r to row r * out_rep + out_off + i % rep of caller-owned buffers."""
    lib = _lib.load()
    R, A = head.shape[0], head.shape[1] // 2
    N = R * rep
    if out_rep is None:
        out_rep = rep
    if act_out is None:
        act_out = torch.empty((R * out_rep, A), dtype=torch.float32, device=head.device)
    if logp_out is None and eps is not None:
        logp_out = torch.empty(R * out_rep, dtype=torch.float32, device=head.device)
    if eps is not None:
        assert eps.is_contiguous() and eps.dtype == torch.float32 and eps.numel() == N * A
    check(lib.rl4rs_squashed_sample(N, rep, A, _ptr(head), _ptr(eps), min_logstd, max_logstd, out_rep, out_off, _ptr(act_out), _ptr(logp_out),
                                    _stream()))
    return act_out, logp_out


def sac_actor_grad(head, eps, act, g_act, log_temp, min_logstd=-20.0, max_logstd=2.0):
    lib = _lib.load()
    B, A = act.shape
    d = torch.empty_like(head)
    check(lib.rl4rs_sac_actor_grad(B, A, _ptr(head), _ptr(eps), _ptr(act), _ptr(g_act), _ptr(log_temp), min_logstd, max_logstd, _ptr(d), _stream()))
    return d


def twin_min(q1, q2, want_grad=False):
    """(min(q1, q2), dq1, dq2): the selector of -mean min (None without ``want_grad``)."""
    lib = _lib.load()
    B = q1.numel()
    qmin = torch.empty(B, dtype=torch.float32, device=q1.device)
    dq1 = torch.empty_like(q1) if want_grad else None
    dq2 = torch.empty_like(q2) if want_grad else None
    check(lib.rl4rs_twin_min(B, _ptr(q1), _ptr(q2), _ptr(qmin), _ptr(dq1), _ptr(dq2), _stream()))
    return qmin, dq1, dq2


def cql_critic_loss(q1, q2, offs, m, y=None, alpha_w=None):
    """(sums6, dq1, dq2) of the continuous CQL critic loss over rows [B][m] (column 0 = dataset action): see
    rl4rs_cql_critic_loss.  ``y`` None: sums only."""
    lib = _lib.load()
    B = q1.numel() // m
    dq1 = torch.empty_like(q1) if y is not None else None
    dq2 = torch.empty_like(q2) if y is not None else None
    rows = torch.empty((B, 6), dtype=torch.float32, device=q1.device)
    sums = torch.empty(6, dtype=torch.float32, device=q1.device)
    check(lib.rl4rs_cql_critic_loss(B, m, _ptr(q1), _ptr(q2), _ptr(offs), _ptr(y), _ptr(alpha_w), _ptr(dq1), _ptr(dq2), _ptr(rows), _ptr(sums),
                                    _stream()))
    return sums, dq1, dq2


# ---- COMBO (csrc/combo.hpp) ------------------------------------------------------------------------------------------------------
def amlp_grad_stash(nets, bufs, add=False):
    """The join of two backward passes through the same handles (rl4rs_amlp_grad_stash; a backward WRITES the flat gradient): copy
    each net's flat gradient to ``bufs[i]``, or with ``add`` add ``bufs[i]`` into it - one launch for up to 4 nets."""
    lib = _lib.load()
    for net, b in zip(nets, bufs):
        assert b.is_cuda and b.dtype == torch.float32 and b.is_contiguous() and b.numel() >= net.n_params
    H = (C.c_void_p * len(nets))(*[net.h for net in nets])
    Bf = (C.c_void_p * len(nets))(*[_ptr(b) for b in bufs])
    check(lib.rl4rs_amlp_grad_stash(len(nets), H, Bf, 1 if add else 0, _stream()))


def combo_critic_loss(B, n_real, k, w, rows, t=None, c=None):
    """COMBO's critic loss (rl4rs_combo_critic_loss) over a minibatch of ``n_real`` real rows then F = B - n_real generated ones.
    ``t`` = (q1 [B], q2 [B], y [B]): the pass-T half -> (dq1, dq2).  ``c`` = (q1 [F * k], q2 [F * k], offs [F * k]): the pass-C half
    -> (sums6, dq1, dq2); the sums count the T half of the LAST call that had one with the same ``rows`` [4 B + 2 F] (this call's,
    when both halves are given: then -> (sums6, dq1t, dq2t, dq1c, dq2c)).  ``w``: the conservative weight, a one-element device tensor."""
    lib = _lib.load()
    F = B - n_real
    assert rows.is_cuda and rows.dtype == torch.float32 and rows.is_contiguous() and rows.numel() >= 4 * B + 2 * max(F, 0)
    tp, cp, out_t, out_c = [None] * 5, [None] * 5, (), ()
    if t is not None:
        assert all(x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() == B for x in t)
        out_t = (torch.empty_like(t[0]), torch.empty_like(t[1]))
        tp = [_ptr(x) for x in tuple(t) + out_t]
    sums = None
    if c is not None:
        assert all(x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() == F * k for x in c)
        out_c = (torch.empty_like(c[0]), torch.empty_like(c[1]))
        cp = [_ptr(x) for x in tuple(c) + out_c]
        sums = torch.empty(6, dtype=torch.float32, device=rows.device)
    check(lib.rl4rs_combo_critic_loss(B, n_real, k, tp[0], tp[1], tp[2], cp[0], cp[1], cp[2], _ptr(w), tp[3], tp[4], cp[3], cp[4], _ptr(rows),
                                      _ptr(sums), _stream()))
    return out_t if c is None else (sums,) + out_t + out_c


# ---- TD3 / DDPG (csrc/td3.hpp) ------------------------------------------------------------------------------------------------
def explore_ou(det_action, ou_state, theta=0.15, sigma=0.2, scale=0.1, seed=0, step=0, random_phase=False, out=None, want_eps=False):
    """RLlib's OrnsteinUhlenbeckNoise on a deterministic action [N, E] (rl4rs_explore_ou): advances ``ou_state`` ([N, E], or [E] /
    [1, E] shared by all rows) in place and returns (action, eps or None).  ``random_phase``: uniform actions, the state stays."""
    lib = _lib.load()
    N, E = det_action.shape
    rows = 1 if ou_state.numel() == E else N
    assert ou_state.numel() == rows * E and ou_state.dtype == torch.float32 and ou_state.is_contiguous() and ou_state.is_cuda
    assert det_action.dtype == torch.float32 and det_action.is_contiguous() and det_action.is_cuda
    if out is None:
        out = torch.empty_like(det_action)
    eps = torch.empty_like(det_action) if want_eps else None
    check(lib.rl4rs_explore_ou(N, E, rows, _ptr(det_action), _ptr(ou_state), theta, sigma, scale, seed & 0xffffffff, step & 0xffffffff,
                               1 if random_phase else 0, _ptr(out), _ptr(eps), _stream()))
    return out, eps


def td3_smooth_action(action, eps, target_noise=0.2, noise_clip=0.5, out=None):
    """clip(action + clip(target_noise * eps, -noise_clip, noise_clip), -1, 1)."""
    lib = _lib.load()
    N, E = action.shape
    assert eps.shape == action.shape and eps.dtype == torch.float32 and eps.is_contiguous() and action.is_contiguous()
    if out is None:
        out = torch.empty_like(action)
    check(lib.rl4rs_td3_smooth_action(N, E, _ptr(action), _ptr(eps), target_noise, noise_clip, _ptr(out), _stream()))
    return out


def td3_critic_loss(q1, q2, q1_targ, q2_targ, rewards, dones, weights=None, gamma=1.0, use_huber=False, huber_threshold=1.0,
                    td_out=None, stats_out=None):
    """RLlib DDPG / TD3 critic loss (rl4rs_td3_critic_loss) -> dict dq1, dq2 (None for a single critic), y, td, stats
    (sums of {w * error, q1, y, |td1|})."""
    lib = _lib.load()
    N = q1.numel()
    assert dones.dtype == torch.int32 and rewards.dtype == torch.float32 and dones.numel() == N and rewards.numel() == N
    dev = q1.device
    dq1 = torch.empty(N, dtype=torch.float32, device=dev)
    dq2 = torch.empty(N, dtype=torch.float32, device=dev) if q2 is not None else None
    y = torch.empty(N, dtype=torch.float32, device=dev)
    td = td_out if td_out is not None else torch.empty(N, dtype=torch.float32, device=dev)
    stats = stats_out if stats_out is not None else torch.empty(4, dtype=torch.float32, device=dev)
    check(lib.rl4rs_td3_critic_loss(N, _ptr(q1), _ptr(q2), _ptr(q1_targ), _ptr(q2_targ), _ptr(rewards), _ptr(dones), _ptr(weights), gamma,
                                    1 if use_huber else 0, huber_threshold, _ptr(dq1), _ptr(dq2), _ptr(y), _ptr(td), _ptr(stats), _stream()))
    return dict(dq1=dq1, dq2=dq2, y=y, td=td, stats=stats)


def tanh_head_grad(tanh_out, d_out):
    """d_out * (1 - tanh_out^2): the gradient wrt a tanh head's pre-activation."""
    lib = _lib.load()
    N, E = tanh_out.shape
    d = torch.empty_like(tanh_out)
    check(lib.rl4rs_tanh_head_grad(N, E, _ptr(tanh_out), _ptr(d_out), _ptr(d), _stream()))
    return d


def amlp_add_l2(net, l2):
    """grad += l2 * W on the three weight matrices of ``net``'s gradient (biases untouched)."""
    check(_lib.load().rl4rs_amlp_add_l2(net.h, float(l2), _stream()))


class DeviceExactK(_FlatNet):
    """rl4rs_exactk handle: Exact-K's pointer-network slate generator (include/rl4rs_hip.h, "On-device Exact-K"; flat layout in
    ``rl4rs_amd/nets/exactk.py``).  One shared candidate list 0..action_size-1.  Dropout is on in every call, as in the reference,
    whose eval stage also builds the generator with is_training=True.  TF parity is unpinned (TensorFlow 1.15 is absent).
    ``location_mask`` [3, A] and ``is_special`` [A]: ``CatalogTables.location_mask[:3]`` / ``.is_special``."""
    _prefix = 'rl4rs_exactk_'
    SLATE = 9

    def __init__(self, location_mask, is_special, max_rows, obs_dim=256, action_size=284, hidden_units=64, num_heads=4, num_blocks=2,
                 vocab=500, dropout_rate=0.1, params=None, seed=0, device=None):
        self.lib = _lib.load()
        self.obs_dim, self.action_size, self.hidden, self.heads, self.blocks = (int(obs_dim), int(action_size), int(hidden_units),
                                                                                 int(num_heads), int(num_blocks))
        self.vocab, self.max_rows, self.dropout_rate = int(vocab), int(max_rows), float(dropout_rate)
        self.cfg = _lib.ExactKCfg(self.obs_dim, self.hidden, self.heads, self.blocks, self.action_size, self.vocab, self.max_rows,
                                  self.dropout_rate)
        loc = np.ascontiguousarray(np.asarray(location_mask)[:3] >= 0.5, dtype=np.uint8)
        spc = np.ascontiguousarray(np.asarray(is_special) != 0, dtype=np.uint8)
        if loc.shape != (3, self.action_size) or spc.shape != (self.action_size,):
            raise ValueError('location_mask must be [3, action_size] and is_special [action_size]')
        n = self.lib.rl4rs_exactk_param_count(C.byref(self.cfg))
        if n < 0:
            raise _lib.Rl4rsHipError(self.lib.rl4rs_last_error().decode())
        self.n_params = int(n)
        if params is None:
            from .nets.exactk import init_exactk_params
            params = init_exactk_params(self.obs_dim, self.hidden, self.blocks, self.vocab, seed)
        params = np.ascontiguousarray(params, dtype=np.float32)
        assert params.shape == (self.n_params,), (params.shape, self.n_params)
        self.device = None
        h = C.c_void_p()
        if torch.cuda.is_available():
            self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
            with torch.cuda.device(self.device):
                check(self.lib.rl4rs_exactk_create(C.byref(self.cfg), params.ctypes.data_as(C.c_void_p), loc.ctypes.data_as(C.c_void_p),
                                                   spc.ctypes.data_as(C.c_void_p), _stream(), C.byref(h)))
        else:       # the shape and mask refusals come first; with neither a refusal nor a device this raises "no HIP device"
            check(self.lib.rl4rs_exactk_create(C.byref(self.cfg), params.ctypes.data_as(C.c_void_p), loc.ctypes.data_as(C.c_void_p),
                                               spc.ctypes.data_as(C.c_void_p), None, C.byref(h)))
        self.h = h

    def _obs(self, obs):
        N = obs.shape[0]
        assert obs.dtype == torch.float32 and obs.shape == (N, self.obs_dim) and obs.is_contiguous() and obs.is_cuda
        assert 1 <= N <= self.max_rows, (N, self.max_rows)
        return N

    def decode(self, obs, greedy=False, seed=0, step=0, want_logits=False, out=None):
        """A slate per row -> (path int32 [N, 9], logits [N, 9, A] or None): an inverse-CDF draw per step at
        u = uniform01(seed, step, row, t), or the first maximum (greedy)."""
        N = self._obs(obs)
        path = out if out is not None else torch.empty((N, self.SLATE), dtype=torch.int32, device=self.device)
        assert path.dtype == torch.int32 and path.shape == (N, self.SLATE) and path.is_contiguous()
        lg = torch.empty((N, self.SLATE, self.action_size), dtype=torch.float32, device=self.device) if want_logits else None
        check(self.lib.rl4rs_exactk_decode(self.h, N, _ptr(obs), 1 if greedy else 0, seed & 0xffffffff, step & 0xffffffff, _ptr(path),
                                           _ptr(lg), _stream()))
        return path, lg

    BEAM_MAX = 8

    def decode_beam(self, obs, beam_size=3, seed=0, step=0, want_trace=False):
        """Beam search over the pointer decoder -> (paths int32 [N, beam_size, 9], scores float32 [N, beam_size]: the sum of the 9
        log-probabilities, beam 0 the best, equal scores by the smaller parent * A + token), with the keep masks of ``decode`` at the
        same (seed, step).  ``want_trace``: also a dict of [N, 9, beam_size] tensors ``parent`` (the beam of step t - 1 that beam k of
        step t extends), ``token`` and ``score``."""
        N, B = obs.shape[0], int(beam_size)               # (the library refuses a beam_size or N out of range, with the reason)
        assert obs.dtype == torch.float32 and obs.shape == (N, self.obs_dim) and obs.is_contiguous() and obs.is_cuda
        paths = torch.empty((N, max(B, 0), self.SLATE), dtype=torch.int32, device=self.device)
        scores = torch.empty((N, max(B, 0)), dtype=torch.float32, device=self.device)
        trace = None
        if want_trace:
            trace = dict(parent=torch.empty((N, self.SLATE, max(B, 0)), dtype=torch.int32, device=self.device),
                         token=torch.empty((N, self.SLATE, max(B, 0)), dtype=torch.int32, device=self.device),
                         score=torch.empty((N, self.SLATE, max(B, 0)), dtype=torch.float32, device=self.device))
        tr = trace or dict(parent=None, token=None, score=None)
        check(self.lib.rl4rs_exactk_decode_beam(self.h, N, _ptr(obs), B, seed & 0xffffffff, step & 0xffffffff, _ptr(paths), _ptr(scores),
                                                _ptr(tr['parent']), _ptr(tr['token']), _ptr(tr['score']), _stream()))
        return (paths, scores, trace) if want_trace else (paths, scores)

    def loss_grad(self, obs, path, weights, seed=0, step=0, want_logits=False):
        """Teacher-forced loss mean_n(w_n sum_t CE) and its gradient into the handle's buffer (``grad()``)
        -> (stats float32[2] = {loss, targets outside the allowed set}, logits [N, 9, A] or None)."""
        N = self._obs(obs)
        assert path.dtype == torch.int32 and path.shape == (N, self.SLATE) and path.is_contiguous()
        assert weights.dtype == torch.float32 and weights.shape == (N,) and weights.is_contiguous()
        lg = torch.empty((N, self.SLATE, self.action_size), dtype=torch.float32, device=self.device) if want_logits else None
        stats = torch.empty(2, dtype=torch.float32, device=self.device)
        check(self.lib.rl4rs_exactk_loss_grad(self.h, N, _ptr(obs), _ptr(path), _ptr(weights), seed & 0xffffffff, step & 0xffffffff,
                                              _ptr(lg), _ptr(stats), _stream()))
        return stats, lg

    def adam_step(self, lr=1e-3, beta1=0.9, beta2=0.98, eps=1e-8, skip=None):
        """tf.train.AdamOptimizer step on the last gradient; ``skip``: int32[1] device tensor, non-zero = leave everything alone."""
        assert skip is None or (skip.dtype == torch.int32 and skip.numel() == 1 and skip.is_cuda)
        check(self.lib.rl4rs_exactk_adam_step(self.h, lr, beta1, beta2, eps, _ptr(skip), _stream()))


class DeviceExactKCritic(_FlatNet):
    """rl4rs_exactk_critic handle: the reference's Discriminator, obs -> 128 relu x 3 -> 1, the REINFORCE baseline of Exact-K."""
    _prefix = 'rl4rs_exactk_critic_'

    def __init__(self, max_rows, obs_dim=256, hidden=128, params=None, seed=0, device=None):
        _lib.require_device()
        self.lib = _lib.load()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.obs_dim, self.hidden, self.max_rows = int(obs_dim), int(hidden), int(max_rows)
        self.n_params = int(self.lib.rl4rs_exactk_critic_param_count(self.obs_dim, self.hidden))
        if params is None:
            from .nets.exactk import init_critic_params
            params = init_critic_params(self.obs_dim, self.hidden, seed)
        params = np.ascontiguousarray(params, dtype=np.float32)
        assert params.shape == (self.n_params,), (params.shape, self.n_params)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.rl4rs_exactk_critic_create(self.obs_dim, self.hidden, self.max_rows, params.ctypes.data_as(C.c_void_p),
                                                      _stream(), C.byref(h)))
        self.h = h

    def _obs(self, obs):
        N = obs.shape[0]
        assert obs.dtype == torch.float32 and obs.shape == (N, self.obs_dim) and obs.is_contiguous() and 1 <= N <= self.max_rows
        return N

    def forward(self, obs, out=None):
        N = self._obs(obs)
        v = out if out is not None else torch.empty(N, dtype=torch.float32, device=self.device)
        check(self.lib.rl4rs_exactk_critic_forward(self.h, N, _ptr(obs), _ptr(v), _stream()))
        return v

    def loss_grad(self, obs, target):
        """Gradient of sum_n (value_n - target_n)^2 into the handle's buffer -> (value [N] before any update, squared errors [N])."""
        N = self._obs(obs)
        assert target.dtype == torch.float32 and target.shape == (N,) and target.is_contiguous()
        v = torch.empty(N, dtype=torch.float32, device=self.device)
        err = torch.empty(N, dtype=torch.float32, device=self.device)
        check(self.lib.rl4rs_exactk_critic_loss_grad(self.h, N, _ptr(obs), _ptr(target), _ptr(v), _ptr(err), _stream()))
        return v, err

    def adam_step(self, lr=5e-3, beta1=0.9, beta2=0.98, eps=1e-8):
        check(self.lib.rl4rs_exactk_critic_adam_step(self.h, lr, beta1, beta2, eps, _stream()))


def sac_target(q1, q2, logp, log_temp, rewards, terminals, gamma):
    """SAC's soft target y = r + gamma (1 - terminal) (min(q1, q2) - exp(log_temp) logp)  (rl4rs_sac_target)."""
    lib = _lib.load()
    N = rewards.numel()
    for t in (q1, q2, logp, rewards, terminals):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == N
    assert log_temp.is_cuda and log_temp.dtype == torch.float32 and log_temp.numel() >= 1
    y = torch.empty(N, dtype=torch.float32, device=rewards.device)
    check(lib.rl4rs_sac_target(_ptr(q1), _ptr(q2), _ptr(logp), _ptr(log_temp), _ptr(rewards), _ptr(terminals), float(gamma), N, _ptr(y),
                               _stream()))
    return y


class DeviceDynamics(_FlatNet):
    """rl4rs_dyn handle: the probabilistic ensemble dynamics model (include/rl4rs_hip.h, "On-device ensemble dynamics model";
    layouts and initialisers in ``rl4rs_amd/dynamics.py``).  ``params`` / ``state``: flat float32 arrays in the header's layout."""
    _prefix = 'rl4rs_dyn_'
    VARIANCE_TYPES = {'max': 0, 'data': 1}

    def __init__(self, obs_dim, act_dim, params, state, hidden_units=(256, 128), members=5, max_rows=4096, max_grad_rows=512,
                 use_batch_norm=True, dropout_rate=0.2, use_dense=True, spectral_norm=True, device=None):
        self.lib = _lib.load()
        self.D, self.E, self.M = int(obs_dim), int(act_dim), int(members)
        self.H1, self.H2 = int(hidden_units[0]), int(hidden_units[1])
        self.O = self.D + 1
        self.max_rows, self.max_grad_rows = int(max_rows), int(max_grad_rows)
        self.cfg = _lib.DynCfg(self.D, self.E, self.H1, self.H2, self.M, self.max_rows, self.max_grad_rows, 1 if use_batch_norm else 0,
                               1 if use_dense else 0, 1 if spectral_norm else 0, float(dropout_rate))
        n = self.lib.rl4rs_dyn_param_count(C.byref(self.cfg))
        if n < 0:
            raise _lib.Rl4rsHipError(self.lib.rl4rs_last_error().decode())
        self.n_params = int(n)
        self.n_state = int(self.lib.rl4rs_dyn_state_count(C.byref(self.cfg)))
        self.n_stats = int(self.lib.rl4rs_dyn_stats_count(C.byref(self.cfg)))
        params = np.ascontiguousarray(params, dtype=np.float32)
        state = np.ascontiguousarray(state, dtype=np.float32)
        assert params.shape == (self.n_params,) and state.shape == (self.n_state,), (params.shape, self.n_params, state.shape, self.n_state)
        self.device = None
        h = C.c_void_p()
        if torch.cuda.is_available():
            self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
            with torch.cuda.device(self.device):
                check(self.lib.rl4rs_dyn_create(C.byref(self.cfg), params.ctypes.data_as(C.c_void_p), state.ctypes.data_as(C.c_void_p),
                                                _stream(), C.byref(h)))
        else:       # the shape refusals come first; with neither a refusal nor a device this raises "no HIP device"
            check(self.lib.rl4rs_dyn_create(C.byref(self.cfg), params.ctypes.data_as(C.c_void_p), state.ctypes.data_as(C.c_void_p), None,
                                            C.byref(h)))
        self.h = h

    def _state_ptrs(self):
        s, n, t, nt = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_int64()
        check(self.lib.rl4rs_dyn_state(self.h, C.byref(s), C.byref(n), C.byref(t), C.byref(nt)))
        return s, n.value, t, nt.value

    def state(self):
        """Copy of the non-trained state: u / v, running statistics, scaler constants (device tensor)."""
        s, n, _, _ = self._state_ptrs()
        return self._copy_out(s, n, None)

    def set_state(self, flat):
        s, n, _, _ = self._state_ptrs()
        self._copy_in('state', s, n, flat)

    def stats(self):
        """Copy of the last forward's statistics [members, 3 + 2 H1 + 2 H2]: sigma, batch mean / biased variance of both layers."""
        _, _, t, nt = self._state_ptrs()
        return self._copy_out(t, nt, None).view(self.M, -1)

    def _rows(self, x, a, cap):
        N = x.shape[0]
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == (N, self.D), tuple(x.shape)
        assert a.is_cuda and a.dtype == torch.float32 and a.is_contiguous() and tuple(a.shape) == (N, self.E), tuple(a.shape)
        assert 1 <= N <= cap, (N, cap)
        return N

    def forward(self, x, a, train=False, seed=0, step=0):
        """[members, N, 2 O] = [mu | bounded ls]; ``train``: batch statistics, dropout, one power iteration (the state moves)."""
        N = self._rows(x, a, self.max_grad_rows if train and self.max_grad_rows else self.max_rows)
        out = torch.empty((self.M, N, 2 * self.O), dtype=torch.float32, device=self.device)
        check(self.lib.rl4rs_dyn_forward(self.h, N, _ptr(x), _ptr(a), 1 if train else 0, seed & 0xffffffff, step & 0xffffffff, _ptr(out),
                                         _stream()))
        return out

    def loss_grad(self, x, a, next_x, next_r, mask, seed=0, step=0):
        """Per-member loss [members] and the gradient of their sum into the handle (``grad()``); ``mask`` float [members, N]."""
        N = self._rows(x, a, self.max_grad_rows)
        assert next_x.is_cuda and next_x.dtype == torch.float32 and next_x.is_contiguous() and tuple(next_x.shape) == (N, self.D)
        assert next_r.is_cuda and next_r.dtype == torch.float32 and next_r.is_contiguous() and next_r.numel() == N
        assert mask.is_cuda and mask.dtype == torch.float32 and mask.is_contiguous() and tuple(mask.shape) == (self.M, N)
        loss = torch.empty(self.M, dtype=torch.float32, device=self.device)
        check(self.lib.rl4rs_dyn_loss_grad(self.h, N, _ptr(x), _ptr(a), _ptr(next_x), _ptr(next_r), _ptr(mask), seed & 0xffffffff,
                                           step & 0xffffffff, _ptr(loss), _stream()))
        return loss

    def adam_step(self, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8):
        check(self.lib.rl4rs_dyn_adam_step(self.h, lr, beta1, beta2, eps, _stream()))

    def predict(self, x, a, indices=None, noise=None, seed=0, step=0, deterministic=False, variance_type='max', lam=None):
        """(next_x [N, D], reward [N], variance [N], member used int32 [N]) of one member per row; ``lam``: reward -= lam * variance."""
        N = self._rows(x, a, self.max_rows)
        if indices is not None:
            assert indices.is_cuda and indices.dtype == torch.int32 and indices.is_contiguous() and indices.numel() == N
        if noise is not None:
            assert noise.is_cuda and noise.dtype == torch.float32 and noise.is_contiguous() and tuple(noise.shape) == (self.M, N, self.O)
        nx = torch.empty((N, self.D), dtype=torch.float32, device=self.device)
        r = torch.empty(N, dtype=torch.float32, device=self.device)
        var = torch.empty(N, dtype=torch.float32, device=self.device)
        used = torch.empty(N, dtype=torch.int32, device=self.device)
        check(self.lib.rl4rs_dyn_predict(self.h, N, _ptr(x), _ptr(a), _ptr(indices), _ptr(noise), seed & 0xffffffff, step & 0xffffffff,
                                         1 if deterministic else 0, self.VARIANCE_TYPES[variance_type], 0 if lam is None else 1,
                                         0.0 if lam is None else float(lam), _ptr(nx), _ptr(r), _ptr(var), _ptr(used), _stream()))
        return nx, r, var, used


class DeviceSeq2Seq(object):
    """rl4rs_seq2seq handle: the MDP checker's one-layer encoder-decoder transformer and its beam search (include/rl4rs_hip.h,
    "The MDP checker's model"; flat layout and initialiser in ``rl4rs_amd/mdpchecker.py``).  Training pass, inference and beam search.  ``max_rows`` bounds the
    activation rows of a call: N * max(L, src_len) of ``forward``, N * max(beam, src_len) of ``beam``."""
    BEAM_MAX = 128

    def __init__(self, token_num, embed_dim, hidden_dim, src_len, tgt_len, max_rows, params, device=None):
        self.lib = _lib.load()
        self.token_num, self.embed_dim, self.hidden_dim = int(token_num), int(embed_dim), int(hidden_dim)
        self.src_len, self.tgt_len, self.max_rows = int(src_len), int(tgt_len), int(max_rows)
        self.cfg = _lib.Seq2SeqCfg(self.token_num, self.embed_dim, self.hidden_dim, self.src_len, self.tgt_len, self.max_rows)
        n = self.lib.rl4rs_seq2seq_param_count(C.byref(self.cfg))
        if n < 0:
            raise _lib.Rl4rsHipError(self.lib.rl4rs_last_error().decode())
        self.n_params = int(n)
        params = np.ascontiguousarray(params, dtype=np.float32)
        assert params.shape == (self.n_params,), (params.shape, self.n_params)
        self.h = None
        _lib.require_device()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.rl4rs_seq2seq_create(C.byref(self.cfg), params.ctypes.data_as(C.c_void_p), _stream(), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, 'h', None):
            torch.cuda.synchronize(self.device)
            self.lib.rl4rs_seq2seq_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def params(self):
        """the handle's flat parameters as a float32 device tensor (a view: writes go to the handle)"""
        p, n = C.c_void_p(), C.c_int64()
        check(self.lib.rl4rs_seq2seq_params(self.h, C.byref(p), None, C.byref(n)))
        return _alias_f32(p.value, n.value, self.device, self)

    def grad(self):
        g, n = C.c_void_p(), C.c_int64()
        check(self.lib.rl4rs_seq2seq_params(self.h, None, C.byref(g), C.byref(n)))
        return _alias_f32(g.value, n.value, self.device, self)

    def adam_state(self):
        """(m, v) views and the number of steps taken"""
        m, v, t = C.c_void_p(), C.c_void_p(), C.c_int64()
        check(self.lib.rl4rs_seq2seq_adam_state(self.h, C.byref(m), C.byref(v), C.byref(t)))
        return _alias_f32(m.value, self.n_params, self.device, self), _alias_f32(v.value, self.n_params, self.device, self), int(t.value)

    def set_adam_step(self, t):
        check(self.lib.rl4rs_seq2seq_set_adam_step(self.h, int(t)))

    def loss_grad(self, enc, dec_in, dec_out, dropout_rate=0.0, seed=0, step=0):
        """masked cross-entropy (device tensor [1]) and its gradient into ``grad()``"""
        enc = self._tokens(enc, self.src_len)
        N, L = enc.shape[0], int(dec_in.shape[1] if hasattr(dec_in, 'shape') else len(dec_in[0]))
        dec_in, dec_out = self._tokens(dec_in, L), self._tokens(dec_out, L)
        assert dec_in.shape[0] == N and dec_out.shape[0] == N
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.lib.rl4rs_seq2seq_loss_grad(self.h, N, _ptr(enc), _ptr(dec_in), _ptr(dec_out), L, float(dropout_rate),
                                                   seed & 0xffffffff, step & 0xffffffff, _ptr(loss), _stream()))
        return loss

    def adam_step(self, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7):
        with torch.cuda.device(self.device):
            check(self.lib.rl4rs_seq2seq_adam_step(self.h, lr, beta1, beta2, eps, _stream()))

    def set_params(self, flat):
        flat = np.ascontiguousarray(flat, dtype=np.float32)
        assert flat.shape == (self.n_params,), (flat.shape, self.n_params)
        self.params().copy_(torch.from_numpy(flat))

    def _tokens(self, x, width):
        t = _dev_tensor(x if isinstance(x, torch.Tensor) else np.asarray(x), torch.int32, self.device)
        assert t.dim() == 2 and t.shape[1] == width, (tuple(t.shape), width)
        return t

    def forward(self, enc, dec):
        """enc int [N, src_len], dec int [N, L] -> probabilities float32 [N, L, V] (device)"""
        enc = self._tokens(enc, self.src_len)
        N, L = enc.shape[0], int(np.shape(dec)[1])
        dec = self._tokens(dec, L)
        assert dec.shape[0] == N
        out = torch.empty((N, L, self.token_num), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.lib.rl4rs_seq2seq_forward(self.h, N, _ptr(enc), _ptr(dec), L, _ptr(out), _stream()))
        return out

    def beam(self, enc, beam, target_len, cand_bits=None, want_step_probs=False):
        """-> (paths int32 [N, beam, target_len + 1], scores float64 [N, beam], step_probs float32 [N, beam, target_len] or None),
        device tensors; ``cand_bits`` uint32 [N, ceil(V / 32)] (numpy).  The library refuses a beam, target_len or N out of range."""
        enc = self._tokens(enc, self.src_len)
        N, B, T = enc.shape[0], int(beam), int(target_len)
        bits = None
        if cand_bits is not None:
            cand_bits = np.ascontiguousarray(cand_bits, dtype=np.uint32)
            assert cand_bits.shape == (N, (self.token_num + 31) // 32), cand_bits.shape
            bits = _dev_tensor(cand_bits.view(np.int32), torch.int32, self.device)
        paths = torch.empty((N, max(B, 0), max(T, 0) + 1), dtype=torch.int32, device=self.device)
        scores = torch.empty((N, max(B, 0)), dtype=torch.float64, device=self.device)
        sp = torch.empty((N, max(B, 0), max(T, 0)), dtype=torch.float32, device=self.device) if want_step_probs else None
        with torch.cuda.device(self.device):
            check(self.lib.rl4rs_seq2seq_beam(self.h, N, _ptr(enc), B, T, _ptr(bits), _ptr(paths), _ptr(scores), _ptr(sp), _stream()))
        return paths, scores, sp
