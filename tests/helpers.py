"""Shared helpers for the parity tests (tests only)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def manifest():
    with open(os.path.join(GOLDEN, 'manifest.json')) as f:
        return json.load(f)


def load_scenario(name):
    m = manifest()[name]
    g = np.load(os.path.join(GOLDEN, name + '.npz'))
    cfg = dict(m['config'])
    cfg['iteminfo_file'] = os.path.join(GOLDEN, m['catalog'])
    cfg['support_conti_env'] = bool(m['conti'])
    if m['mask_flag']:
        cfg[m['mask_flag']] = True
    with open(os.path.join(GOLDEN, m['records'])) as f:
        records = [x for x in f.read().split('\n') if x]
    return m, cfg, records, g


def golden_equal(g, key, arr):
    """Bit-exact comparison of ``arr`` with golden array ``key``: stored whole, or (large float arrays of the batch-256
    scenario, make_golden.py::compact) as sha1 digest + shape + dtype + first rows."""
    import hashlib
    if key in g.files:
        return np.array_equal(arr, g[key])
    a = np.ascontiguousarray(arr)
    head = g[key + '__head']
    return (tuple(a.shape) == tuple(g[key + '__shape'].tolist()) and str(a.dtype) == str(g[key + '__dtype'])
            and np.array_equal(a[:len(head)], head)
            and hashlib.sha1(a.tobytes()).digest() == g[key + '__sha1'].tobytes())


def golden_has(g, key):
    return key in g.files or (key + '__sha1') in g.files


SCENARIOS = ['slate_discrete', 'slate_conti', 'seq36_discrete', 'seq36_conti', 'seq32_discrete',
             'seq32_conti', 'real_discrete', 'real_conti', 'slate256_discrete', 'seq36_b64_discrete', 'slate_onehot']


# ----------------------------------------------------------------------------------------------------------------------
# Facade fixtures (tests/golden/facade_*.npz, make_golden.py::facade_scenarios): whole episodes of the reference's own
# RecEnvBase(SlateRecEnv | SeqSlateRecEnv), recorded value by value with a type signature.  The same driver runs the
# reference (generator), the oracle (test_oracle_golden.py) and the HIP facade (test_gpu_facade.py).

FACADE_SCENARIOS = ['slate_plain', 'slate_rllib', 'slate_d3rl', 'slate_raw', 'slate_raw_rllib', 'slate_conti', 'slate_onehot',
                    'slate_info', 'slate_b1', 'seq36_plain', 'seq36_rllib', 'seq36_d3rl', 'seq36_conti', 'seq32_plain',
                    'seq32_rllib', 'sampling', 'vector']


def type_sig(v):
    """JSON-able type signature: python type, length, dict key order, numpy dtype and shape, recursively.  A list or tuple
    carries its first element's signature when every element has the same one ('first'), else every element's ('each')."""
    if isinstance(v, np.ndarray):
        return {'t': 'ndarray', 'dtype': str(v.dtype), 'shape': list(v.shape)}
    if isinstance(v, np.generic):
        return {'t': 'np.' + type(v).__name__}
    if isinstance(v, dict):
        return {'t': 'dict', 'keys': list(v), 'items': [type_sig(v[k]) for k in v]}
    if isinstance(v, (list, tuple)):
        sigs = [type_sig(x) for x in v]
        out = {'t': 'list' if isinstance(v, list) else 'tuple', 'len': len(v)}
        if sigs and all(s == sigs[0] for s in sigs):
            out['first'] = sigs[0]
        elif sigs:
            out['each'] = sigs
        return out
    for t in (bool, int, float, str):
        if isinstance(v, t):
            return {'t': t.__name__}
    return {'t': type(v).__name__}


def _flatten(key, v, out):
    """dicts and lists of dicts become one array per key ('<key>.<name>'), anything else np.asarray."""
    if isinstance(v, dict):
        for k in v:
            _flatten(key + '.' + k, v[k], out)
    elif isinstance(v, (list, tuple)) and len(v) and isinstance(v[0], dict):
        for k in v[0]:
            _flatten(key + '.' + k, [x[k] for x in v], out)
    else:
        out[key] = np.asarray(v)


STEP_PARTS = ('obs', 'reward', 'done', 'info')


def run_facade_script(env, script, action_for, vector=None, net_rows=None):
    """Drive ``env`` (a reference-shaped ``RecEnvBase``) through ``script`` (list of {'op': ...}).

    After every op: what the call returned, ``env.state``, ``user_id``, ``offline_action``, ``offline_reward``; after the
    ops that sample, the sampled record strings and ``_recData.sample_list``; ``net_rows()`` (if given) is the list of
    rows the simulator net scored per call since the previous op.  ``action_for(i, env)`` gives the action of op ``i``.
    Returns (values {'e<i>.<field>': ndarray}, signatures [ {field: type_sig} per op ])."""
    vals, sigs = {}, []
    for i, op in enumerate(script):
        kind = op['op']
        rec = {}
        if kind == 'seed':
            env.seed(op['seed'])
        elif kind == 'reset':
            rec['ret'] = env.reset(reset_file=op.get('reset_file', False))
        elif kind == 'reset_at':
            rec['ret'] = vector.reset_at(op['index'])
        elif kind in ('step', 'vector_step'):
            rec['action'] = a = action_for(i, env)
            ret = env.step(a) if kind == 'step' else vector.vector_step(a)
            rec['ret'] = ret
        else:
            assert kind == 'construct', kind
        rec['state'] = env.state
        rec['user_id'] = env.user_id
        rec['offline_action'] = env.offline_action
        rec['offline_reward'] = env.offline_reward
        sigs.append(dict((k, type_sig(v)) for k, v in rec.items()))
        for k, v in rec.items():
            if k == 'ret' and kind in ('step', 'vector_step'):
                assert len(v) == 4
                for part, x in zip(STEP_PARTS, v):
                    _flatten('e%d.ret.%s' % (i, part), x, vals)
            else:
                _flatten('e%d.%s' % (i, k), v, vals)
        if kind in ('construct', 'reset') or (kind == 'reset_at' and op['index'] == 0):
            vals['e%d.records' % i] = np.array([str(x) for x in env.samples.records])
            vals['e%d.sample_list' % i] = np.array([str(x) for x in env.sim._recData.sample_list])
        if net_rows is not None:
            vals['e%d.net_rows' % i] = np.asarray(net_rows(), dtype=np.int64).reshape(-1, 2)
    return vals, sigs


def dedup(vals, seen, name, min_bytes=1024):
    """An array bit-identical to one stored before (the stale ``state`` after a step; the observations an rllib-mode episode
    shares with the plain one) is stored as '<key>@ref' = the earlier key, '<fixture>:<key>' when it lives in another
    fixture.  ``seen`` (digest -> location) carries over from fixture to fixture."""
    import hashlib
    out = {}
    for k in sorted(vals, key=lambda s: (int(s.split('.')[0][1:]), s)):
        v = np.asarray(vals[k])                    # (np.ascontiguousarray would make a 0-d value 1-d)
        d = hashlib.sha1(str(v.dtype).encode() + str(v.shape).encode() + v.tobytes()).hexdigest()
        if v.nbytes >= min_bytes and d in seen:
            where = seen[d]
            out[k + '@ref'] = np.array(where[1] if where[0] == name else '%s:%s' % where)
        else:
            out[k] = v
            seen.setdefault(d, (name, k))
    return out


def load_facade(name):
    """(manifest entry, fixture dir paths resolved into config, {key: ndarray} with refs resolved, script, signatures)."""
    m = manifest()[name]
    g = np.load(os.path.join(GOLDEN, name + '.npz'))
    vals, others = {}, {}
    for k in g.files:
        if k.endswith('@ref'):
            where = str(g[k])
            if ':' in where:
                other, key = where.split(':')
                if other not in others:
                    others[other] = np.load(os.path.join(GOLDEN, other + '.npz'))
                vals[k[:-4]] = others[other][key]
            else:
                vals[k[:-4]] = g[where]
        elif k not in ('script', 'signatures'):
            vals[k] = g[k]
    cfg = dict(m['config'])
    cfg['iteminfo_file'] = os.path.join(GOLDEN, m['catalog'])
    cfg['sample_file'] = os.path.join(GOLDEN, m['records'])
    return m, cfg, vals, json.loads(str(g['script'])), json.loads(str(g['signatures']))


def recorded_action(vals, sigs, i):
    """The action op ``i`` passed, rebuilt with its recorded python type."""
    a, s = vals['e%d.action' % i], sigs[i]['action']
    if s['t'] == 'int':
        return int(a)
    if s['t'] == 'list':
        return a.tolist() if s['first']['t'] in ('int', 'float') else [x for x in a]
    assert s['t'] == 'ndarray'
    return a.astype(s['dtype'])


def facade_weights(m):
    """The simulator weights of a facade fixture, rebuilt from the recorded seed; their digest must match the manifest."""
    import hashlib
    from rl4rs_amd.nets.dien import init_dien_weights
    w = init_dien_weights(m['weights']['config'], **m['weights']['init'])
    h = hashlib.sha1()
    for k in sorted(w):
        h.update(k.encode())
        h.update(np.ascontiguousarray(w[k]).tobytes())
    assert h.hexdigest() == m['weights']['sha1'], 'init_dien_weights no longer rebuilds the fixture weights'
    return w


def compare_facade(want, got, obs_atol=0.0, rtol=0.0, atol=0.0, obs_dim=256):
    """Every recorded array against the run's.  Float arrays of the scorer's output ('obs' values, rewards, click_p) within
    the given bars (0 = bit-exact); everything else exact, with the same dtype."""
    assert sorted(got) == sorted(want), (sorted(set(got) ^ set(want)))
    for k in sorted(want):
        w, v = want[k], np.asarray(got[k])
        assert w.shape == v.shape, (k, w.shape, v.shape)
        part = k.split('.', 1)[1]
        scored = (part in ('ret', 'state') or part.startswith(('ret.obs', 'state.'))) and w.dtype.kind == 'f' and w.ndim and \
            not part.endswith(('dense_feature', 'action_mask', 'masked_actions', 'cur_steps'))
        if scored and (obs_atol or rtol or atol):
            n = obs_dim if w.shape[-1] > obs_dim else w.shape[-1]        # d3rl: [obs | masked_actions | cur_steps]
            assert np.abs(v[..., :n].astype(np.float64) - w[..., :n]).max() <= obs_atol, k
            assert np.array_equal(v[..., n:], w[..., n:]), k
        elif w.dtype.kind == 'f' and (part.startswith('ret.reward') or part.endswith('click_p')) and (rtol or atol):
            assert np.allclose(v, w, rtol=rtol, atol=atol), (k, v, w)
        else:
            assert v.dtype == w.dtype and np.array_equal(v, w), (k, v, w)


class CountingScorer(object):
    """Wraps an oracle scorer: obs as float32 (what keras hands back), prob as OracleDien gives it; logs rows per call."""

    def __init__(self, scorer):
        self.scorer = scorer
        self.calls = []
        self.last = None

    def obs(self, seq, dense, cat):
        self.calls.append((0, len(cat)))
        return np.asarray(self.scorer.obs(seq, dense, cat), dtype=np.float32)

    def prob(self, seq, dense, cat):
        self.calls.append((1, len(cat)))
        self.last = np.asarray(self.scorer.prob(seq, dense, cat), dtype=np.float32)
        return self.last

    def take_calls(self):
        out, self.calls = self.calls, []
        return out


class OracleFacade(object):
    """``oracle.env.OracleEnv`` behind the reference's ``RecEnvBase`` surface, for replaying a facade fixture: the
    ``obs_fn`` packaging of slate.py:244-279, click_p under ``simulator_info_fetch`` (slate.py:300-302), the state left
    stale by ``step`` (base.py:236-239) and ``rl4rs_amd``'s ``single_elem_support``.  The oracle does not sample: each
    reset takes the records the fixture recorded for it (the sampling itself is pinned in test_host_logic.py)."""

    def __init__(self, config, scorer, seq, records_at, sample_lists):
        from oracle.env import OracleEnv
        from rl4rs_amd.env.base import single_elem_support
        self.config = config
        self.batch_size = config['batch_size']
        self.seq = seq
        self.scorer = scorer
        self._records_at, self._sample_lists = list(records_at), list(sample_lists)
        self._unwrap = single_elem_support(lambda x: x)
        self.sim = type('Sim', (), {})()
        self.sim._recData = type('Data', (), {})()
        self._orc = OracleEnv(config, self._records_at[0], scorer, seq=seq)     # samples once, as RecEnvBase.__init__ does
        self.observation_space = self.action_space = None
        self.reset()

    def _obs_fn(self, o):
        B = self.batch_size
        if self.config.get('rawstate_as_obs', False):
            raw = [dict(category_feature=o['category_feature'][i], dense_feature=o['dense_feature'][i],
                        sequence_feature=o['sequence_feature'][i]) for i in range(B)]
            if self.config.get('support_rllib_mask', False):
                return [dict(action_mask=o['action_mask'][i], **raw[i]) for i in range(B)]
            return raw
        if self.config.get('support_rllib_mask', False):
            return [{'action_mask': o['action_mask'][i], 'obs': o['obs'][i]} for i in range(B)]
        if self.config.get('support_d3rl_mask', False):
            return np.concatenate([o['obs'], o['masked_actions'], o['cur_steps']], axis=-1)
        return o['obs']

    def reset(self, reset_file=False):
        records = self._records_at.pop(0)
        self.sim._recData.sample_list = self._sample_lists.pop(0)
        self.obs = self._obs_fn(self._orc.reset(records=records))
        self.samples = self._orc.samples
        self.infos = [{} for _ in range(self.batch_size)]
        return self.state

    def seed(self, sd=0):
        pass

    @property
    def state(self):
        return self._unwrap(self.obs)

    @property
    def user_id(self):
        return self._unwrap(self.samples.user)

    @property
    def offline_action(self):
        return self._unwrap(self.samples.offline_action)

    @property
    def offline_reward(self):
        return self._unwrap(self.samples.offline_reward)

    def step(self, action):
        from oracle.env import is_reward_step
        if not isinstance(action, (list, np.ndarray)):
            action = [action]
        o, reward, done, _ = self._orc.step(action)
        if self.config.get('simulator_info_fetch', False) and not self.seq and is_reward_step(self.samples):
            probs = self.scorer.last.reshape(self.batch_size, -1)
            for i in range(self.batch_size):
                self.infos[i].update({'click_p': probs[i]})
        return self._unwrap((self._obs_fn(o), reward, done, self.infos))


def oracle_facade_run(name, scorer=None):
    """Replay facade fixture ``name`` on the oracle; returns (recorded values, recorded signatures, run values, run
    signatures).  ``scorer`` defaults to the fp64 OracleDien with the fixture's seed-rebuilt weights."""
    from oracle.dien import OracleDien
    from rl4rs_amd.utils.rllib_vector_env import MyVectorEnvWrapper
    m, cfg, vals, script, sigs = load_facade(name)
    if scorer is None:
        scorer = OracleDien(facade_weights(m), m['weights']['config'], np.float64)
    scorer = CountingScorer(scorer)
    samples = [i for i, op in enumerate(script) if op['op'] in ('construct', 'reset')
               or (op['op'] == 'reset_at' and op['index'] == 0)]
    env = OracleFacade(cfg, scorer, m['seq'], [list(vals['e%d.records' % i]) for i in samples],
                       [list(vals['e%d.sample_list' % i]) for i in samples])
    vector = MyVectorEnvWrapper(env, cfg['batch_size']) if any(op['op'] == 'reset_at' for op in script) else None
    got, got_sigs = run_facade_script(env, script, lambda i, e: recorded_action(vals, sigs, i), vector=vector,
                                      net_rows=scorer.take_calls)
    return vals, sigs, got, got_sigs
