#!/usr/bin/env python
"""Generate golden fixtures by running the REFERENCE's own env classes.

Runs ONLY in the build container (needs /root/reference); never at test time, never on the GPU box.
Reference source is imported, not copied: the committed artefacts are data (inputs + expected
outputs) under tests/golden/*.npz|*.txt.

Recipe: stub modules for gym / tensorflow / ray, a restatement of Keras ``pad_sequences`` (the only
third-party function on the path), ``np.int = int``, an ``np.array`` inside rl4rs.env.slate / seqslate that falls back to
``dtype=object`` on the ragged ``get_complete_states()`` (numpy >= 1.24); the TF session, saver and
``tf.keras.backend.function`` are do-nothing stubs and ``rl4rs.nets.dien.get_model`` returns ``StubNet``, whose
'simulator_obs' / 'simulator_reward' layers call a numpy scorer.  With those, the reference's own classes run unmodified:

* state fixtures (``<scenario>.npz``): ``SlateState`` / ``SeqSlateState`` / ``FeatureUtil`` driven step by step; the reward
  is the reference's own ``SlateRecEnv.forward`` / ``SeqSlateRecEnv.forward(None, state)`` (scenario mask flag set in the
  simulator's config) with the reward layer returning the scenario's supplied ``probs_<t>``; ``c_seq/c_dense/c_cat_<t>``
  are the rows forward() handed to that layer.
* facade fixtures (``facade_<name>.npz``): whole episodes of ``RecEnvBase(SlateRecEnv | SeqSlateRecEnv)`` (and
  ``MyVectorEnvWrapper``) on ``catalog_synth.csv`` + ``records_facade_*.txt``, the net the fp64 ``oracle.dien.OracleDien``
  with ``init_dien_weights`` weights (seed, config and sha1 in manifest.json; not committed).  Every value the env hands
  out after construction, each reset and each step is recorded with its type signature (tests/helpers.py::
  run_facade_script), plus the rows the net scored per call.
* ``cache_windows.json``: ``RecDataBase.sample_cache`` windows over small files with blank lines.

usage: python tests/golden/make_golden.py
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = '/root/reference'
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.dirname(HERE))


def _pad_sequences(sequences, maxlen=None, dtype='int32', padding='pre', truncating='pre', value=0.):
    out = np.full((len(sequences), maxlen), value, dtype=dtype)
    for i, s in enumerate(sequences):
        s = list(s)
        if not len(s):
            continue
        t = s[-maxlen:] if truncating == 'pre' else s[:maxlen]
        t = np.asarray(t, dtype=dtype)
        if padding == 'post':
            out[i, :len(t)] = t
        else:
            out[i, -len(t):] = t
    return out


def install_stubs():
    np.int = int

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class _Space(object):
        def __init__(self, *a, **k):
            self.args, self.kw = a, k

    gym = mod('gym', Env=object)
    gym.spaces = mod('gym.spaces', Box=_Space, Discrete=_Space, Dict=_Space)
    mod('gym.envs')
    mod('gym.envs.registration', register=lambda **kw: None)
    tf = mod('tensorflow')
    mod('tensorflow.python')
    mod('tensorflow.python.data')
    mod('tensorflow.python.data.ops', dataset_ops=None)
    mod('tensorflow.keras')
    mod('tensorflow.keras.preprocessing')
    mod('tensorflow.keras.preprocessing.sequence', pad_sequences=_pad_sequences)
    # RecSimBase.__init__ / SlateRecEnv.__init__ (base.py:117-131, slate.py:225-237): graph, session, saver and two backend
    # functions over the layers named simulator_obs / simulator_reward of the model rl4rs.nets.<algo>.get_model returns
    tf.Graph = _Context
    tf.Session = _Context
    tf.ConfigProto = _Context
    tf.train = types.SimpleNamespace(Saver=_Context)
    tf.keras = sys.modules['tensorflow.keras']
    tf.keras.backend = mod('tensorflow.keras.backend', function=lambda inputs, output: (lambda feat: NET.run(output, feat)))
    mod('rl4rs.nets.dien', get_model=lambda config: NET)
    # MyVectorEnvWrapper (rl4rs/utils/rllib_vector_env.py) imports RLlib's VectorEnv and typing names
    mod('ray')
    mod('ray.rllib')
    mod('ray.rllib.utils')
    mod('ray.rllib.utils.typing', EnvActionType=object, EnvConfigDict=object, EnvInfoDict=object, EnvObsType=object,
        EnvType=object, PartialTrainerConfigDict=object)
    mod('ray.rllib.env')
    mod('ray.rllib.env.vector_env', VectorEnv=_VectorEnv)
    sys.path.insert(0, REF)
    import rl4rs.nets
    rl4rs.nets.dien = sys.modules['rl4rs.nets.dien']
    # slate.py:295 / seqslate.py:143 build np.array(get_complete_states()) of ragged rows: numpy >= 1.24 wants dtype=object
    import rl4rs.env.slate
    import rl4rs.env.seqslate
    rl4rs.env.slate.np = rl4rs.env.seqslate.np = _RaggedNumpy('numpy_ragged')
    return tf


class _Context(object):
    """tf.Graph / tf.Session / tf.ConfigProto / tf.train.Saver: context managers that do nothing."""

    def __init__(self, *a, **k):
        self.graph = self

    def as_default(self):
        return self

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def restore(self, sess, path):
        pass


class _VectorEnv(object):
    def __init__(self, observation_space, action_space, num_envs):
        self.observation_space, self.action_space, self.num_envs = observation_space, action_space, num_envs


class _RaggedNumpy(types.ModuleType):
    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def array(obj, *a, **k):
        try:
            return np.array(obj, *a, **k)
        except ValueError:
            k['dtype'] = object
            return np.array(obj, *a, **k)


class _Layer(object):
    def __init__(self, name):
        self.name = self.output = name


class StubNet(object):
    """The keras model the reference's simulator drives.  Its two backend functions receive the 4-tuple of
    ``feature_extraction``; 'simulator_obs' returns ``scorer.obs`` as float32, 'simulator_reward' returns [1-p, p] as
    float32 with p = ``probs`` when set (the legacy scenarios supply them), else ``scorer.prob``.  Every call is logged as
    (kind, rows) and its feature rows are kept in ``last``."""

    def __init__(self):
        self.layers = [_Layer('simulator_obs'), _Layer('simulator_reward')]
        self.input = 'input'
        self.scorer = None
        self.probs = None
        self.calls = []
        self.last = None

    def get_layer(self, name):
        return [x for x in self.layers if x.name == name][0]

    def run(self, layer, feat):
        seq, dense, cat = feat[0], feat[1], feat[2]
        self.last = (seq, dense, cat)
        self.calls.append((0 if layer == 'simulator_obs' else 1, len(cat)))
        if layer == 'simulator_obs':
            return np.asarray(self.scorer.obs(seq, dense, cat), dtype=np.float32)
        p = self.probs if self.probs is not None else self.scorer.prob(seq, dense, cat)
        p = np.asarray(p, dtype=np.float32).reshape(-1)
        return np.stack([np.float32(1) - p, p], axis=1)

    def take_calls(self):
        out, self.calls = self.calls, []
        return out


NET = StubNet()


def base_config(**kw):
    cfg = {"maxlen": 64, "batch_size": 6, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
           "category_feature_num": 21, "category_hash_size": 100000, "seq_num": 2, "emb_size": 128,
           "page_items": 9, "hidden_units": 128, "max_steps": 9, "action_emb_size": 32}
    cfg.update(kw)
    return cfg


def run_scenario(name, state_cls, FeatureUtil, cfg, records, seq, conti, rs, mask_flag, sim_cls, sample_file):
    """Drive one episode; returns dict of arrays keyed '<field>_<t>'."""
    cfg = dict(cfg)
    cfg['support_conti_env'] = conti
    st = state_cls(cfg, records)
    fu = FeatureUtil(cfg)
    B, T, A = cfg['batch_size'], cfg['max_steps'], cfg['action_size']
    g = {}
    feat, _ = fu.feature_extraction(st.state)
    g['seq_init'] = np.asarray(feat[0], dtype=np.int32)
    g['dense_init'] = np.asarray(feat[1], dtype=np.float32)
    g['cat_init'] = np.asarray(feat[2], dtype=np.int32)
    cfg_mask = st.config
    cfg_mask['support_rllib_mask'] = True
    g['obsmask_init'] = np.asarray(st.state['action_mask'], dtype=np.int64)
    cfg_mask['support_rllib_mask'] = False
    g['action_emb'] = np.asarray(st.action_emb, dtype=np.float64)
    g['user'] = np.array(st.user)
    # the reference's simulator, built as RecSimBase builds it; its forward() runs on the state driven here
    sim_cfg = dict(cfg, sample_file=sample_file, model_file='none')
    if mask_flag:
        sim_cfg[mask_flag] = True
    sim = sim_cls(sim_cfg, state_cls)
    for t in range(T):
        off = st.offline_action
        if conti:
            g['offline_action_%d' % t] = np.asarray(off, dtype=np.float64)
            # random direction, float32 like a policy net would emit; a few rows replay the logged embedding
            act = rs.randn(B, cfg['action_emb_size']).astype(np.float32)
            act[0] = np.asarray(off[0], dtype=np.float32)
            g['action_in_%d' % t] = act
            st.act(act)
        else:
            g['offline_action_%d' % t] = np.asarray(off, dtype=np.int64)
            act = np.asarray(off, dtype=np.int64)
            g['action_in_%d' % t] = act
            st.act(act)
        g['prev_actions_%d' % t] = np.asarray(st.prev_actions, dtype=np.int64).copy()
        g['action_mask_%d' % t] = np.asarray(st.action_mask, dtype=np.int64).copy()
        g['special_mask_%d' % t] = np.asarray(st.special_mask, dtype=np.int64).copy()
        feat, _ = fu.feature_extraction(st._state)
        g['seq_%d' % t] = np.asarray(feat[0], dtype=np.int32)
        g['dense_%d' % t] = np.asarray(feat[1], dtype=np.float32)
        g['cat_%d' % t] = np.asarray(feat[2], dtype=np.int32)
        # obs-side views (post-increment cur_steps)
        cfg_mask['support_rllib_mask'] = True
        if not (not seq and st.cur_steps // 3 > 3):
            g['obsmask_%d' % t] = np.asarray(st.state['action_mask'], dtype=np.int64)
        cfg_mask['support_rllib_mask'] = False
        cfg_mask['support_d3rl_mask'] = True
        s = st.state
        g['d3rl_prev_%d' % t] = np.asarray(s['masked_actions'], dtype=np.int64).copy()
        g['d3rl_cur_%d' % t] = np.asarray(s['cur_steps'], dtype=np.int64)
        cfg_mask['support_d3rl_mask'] = False
        # reward with a supplied probability array
        probs = rs.rand(B, cfg.get('page_items', 9) if seq else T).astype(np.float32)
        g['probs_%d' % t] = probs
        NET.probs, NET.last = probs, None
        reward = sim.forward(None, st)
        NET.probs = None
        g['reward_%d' % t] = np.asarray(reward, dtype=np.float64)
        if NET.last is not None:
            # the rows forward() handed to the reward layer, then the price and violation arrays it reduced with
            g['c_seq_%d' % t] = np.asarray(NET.last[0], dtype=np.int32)
            g['c_dense_%d' % t] = np.asarray(NET.last[1], dtype=np.float32)
            g['c_cat_%d' % t] = np.asarray(NET.last[2], dtype=np.int32)
            pa = st.prev_actions if not seq else st.prev_actions[:, :st.cur_steps]
            price = st.get_price(pa)
            g['price_%d' % t] = np.asarray(price if not seq else price[:, -cfg.get('page_items', 9):], dtype=np.float64)
            g['violation_%d' % t] = np.asarray(st.get_violation(), dtype=np.int64)
        g['offline_reward_%d' % t] = np.asarray(st.offline_reward, dtype=np.float64)
    g['offline_action_end'] = np.asarray(st.offline_action, dtype=np.float64 if conti else np.int64)
    g['violation_end'] = np.asarray(st.get_violation(), dtype=np.int64)
    return g


def compact(g, min_bytes=200000, head_rows=8):
    """Large float feature-row arrays (dense_*, c_dense_*) of a big-batch scenario are committed as a digest: '<key>__sha1' (sha1 of the C-order bytes),
    '<key>__shape', '<key>__dtype' and the first rows '<key>__head' - bit-exact comparison needs no more than that, and the
    fixture stays small.  tests/helpers.py::golden_equal understands both forms."""
    import hashlib
    out = {}
    for k, v in g.items():
        v = np.ascontiguousarray(v)
        if v.dtype.kind == 'f' and v.nbytes >= min_bytes and (k.startswith('dense_') or k.startswith('c_dense_')):
            out[k + '__sha1'] = np.frombuffer(hashlib.sha1(v.tobytes()).digest(), dtype=np.uint8).copy()
            out[k + '__shape'] = np.asarray(v.shape, dtype=np.int64)
            out[k + '__dtype'] = np.array(str(v.dtype))
            out[k + '__head'] = v[:head_rows].copy()
        else:
            out[k] = v
    return out


# facade scenarios: name -> (seq, T, B, config flags, script kind)
FACADE = {
    'slate_plain': (False, 9, 6, {}, 'two'),
    'slate_rllib': (False, 9, 6, {'support_rllib_mask': True}, 'two'),
    'slate_d3rl': (False, 9, 6, {'support_d3rl_mask': True}, 'two'),
    'slate_raw': (False, 9, 6, {'rawstate_as_obs': True}, 'one'),
    'slate_raw_rllib': (False, 9, 6, {'rawstate_as_obs': True, 'support_rllib_mask': True}, 'one'),
    'slate_conti': (False, 9, 6, {'support_conti_env': True}, 'one'),
    'slate_onehot': (False, 9, 6, {'support_conti_env': True, 'support_onehot_action': True}, 'one'),
    'slate_info': (False, 9, 6, {'simulator_info_fetch': True}, 'one'),
    'slate_b1': (False, 9, 1, {}, 'two'),
    'seq36_plain': (True, 36, 6, {}, 'one'),
    'seq36_rllib': (True, 36, 6, {'support_rllib_mask': True}, 'one'),
    'seq36_d3rl': (True, 36, 6, {'support_d3rl_mask': True}, 'one'),
    'seq36_conti': (True, 36, 6, {'support_conti_env': True}, 'one'),
    'seq32_plain': (True, 32, 6, {}, 'one'),
    'seq32_rllib': (True, 32, 6, {'support_rllib_mask': True}, 'one'),
    'sampling': (False, 9, 6, {'is_eval': False, 'cache_size': 7}, 'sampling'),
    'vector': (False, 9, 6, {'support_rllib_mask': True}, 'vector'),
}
FACADE_WEIGHTS = {'init': {'seed': 5, 'emb_scale': 0.5, 'bias_noise': 0.2}, 'category_hash_size': 5000}


def facade_script(kind, T):
    steps = lambda: [{'op': 'step', 't': t} for t in range(T)]
    if kind == 'two':
        return [{'op': 'construct'}] + steps() + [{'op': 'reset', 'reset_file': True}] + steps()
    if kind == 'one':
        return [{'op': 'construct'}] + steps() + [{'op': 'reset', 'reset_file': True}]
    if kind == 'sampling':
        # the constructor resets twice (base.py:186,226); four more resets wrap the 7-line cache at EOF twice
        return ([{'op': 'construct'}, {'op': 'seed', 'seed': 123}, {'op': 'reset'}] + steps()
                + [{'op': 'reset'}, {'op': 'reset'}, {'op': 'reset'}, {'op': 'reset', 'reset_file': True}] + steps()[:3])
    assert kind == 'vector'
    return ([{'op': 'construct'}, {'op': 'reset_at', 'index': 0}, {'op': 'reset_at', 'index': 3}]
            + [{'op': 'vector_step', 't': t} for t in range(T)])


def facade_scenarios(manifest, cat_path, special_ids):
    """Whole episodes of the reference's RecEnvBase(SlateRecEnv | SeqSlateRecEnv) with the oracle DIEN as its net."""
    import hashlib
    from rl4rs.env import RecEnvBase
    from rl4rs.env.slate import SlateState, SlateRecEnv
    from rl4rs.env.seqslate import SeqSlateState, SeqSlateRecEnv
    from rl4rs.utils.rllib_vector_env import MyVectorEnvWrapper
    from rl4rs_amd import synth
    from rl4rs_amd.nets.dien import init_dien_weights
    from oracle.dien import OracleDien
    from helpers import run_facade_script, dedup

    paths = {}
    for seq, pages, seed in ((False, 1, 5000), (True, 4, 6000)):
        name = 'records_facade_%s.txt' % ('seq' if seq else 'slate')
        recs = synth.make_records(11, pages=pages, seed=seed, illegal_frac=0.4, hash_size=5000, special_ids=special_ids)
        synth.write_records(os.path.join(HERE, name), recs)
        paths[seq] = name
    wcfg = base_config(category_hash_size=FACADE_WEIGHTS['category_hash_size'])
    w = init_dien_weights(wcfg, **FACADE_WEIGHTS['init'])
    h = hashlib.sha1()
    for k in sorted(w):
        h.update(k.encode())
        h.update(np.ascontiguousarray(w[k]).tobytes())
    NET.scorer = OracleDien(w, wcfg, np.float64)
    seen = {}
    for name, (seq, T, B, flags, kind) in sorted(FACADE.items()):
        cfg = base_config(batch_size=B, max_steps=T, category_hash_size=wcfg['category_hash_size'], is_eval=True, cache_size=B)
        cfg.update(flags)
        run_cfg = dict(cfg, iteminfo_file=cat_path, sample_file=os.path.join(HERE, paths[seq]), model_file='none')
        script = facade_script(kind, T)
        rs = np.random.RandomState(31)

        def action_for(i, env):
            t = script[i]['t']
            if env.config.get('support_conti_env', False):
                a = rs.randn(B, env.config['action_emb_size']).astype(np.float32)
                a[:B // 3] = np.asarray(env.offline_action[:B // 3], dtype=np.float32)     # a third replays the log
                return a
            a = env.offline_action
            if t % 4 == 3:
                # off-policy ids (duplicates / wrong layers -> violations) for the second half of the batch
                a = (list(a[:B // 2]) if B > 1 else []) + [int(x) for x in rs.randint(0, 284, size=B - B // 2)]
            return a

        np.random.seed(0)
        NET.take_calls()
        env = RecEnvBase((SeqSlateRecEnv if seq else SlateRecEnv)(run_cfg, SeqSlateState if seq else SlateState))
        vector = MyVectorEnvWrapper(env, B) if kind == 'vector' else None
        vals, sigs = run_facade_script(env, script, action_for, vector=vector, net_rows=NET.take_calls)
        g = dedup(vals, seen, 'facade_' + name)
        g['script'] = np.array(json.dumps(script))
        g['signatures'] = np.array(json.dumps(sigs))
        np.savez_compressed(os.path.join(HERE, 'facade_%s.npz' % name), **g)
        cfg['iteminfo_file'] = 'catalog_synth.csv'
        cfg['sample_file'] = paths[seq]
        manifest['facade_' + name] = {'config': cfg, 'seq': seq, 'catalog': 'catalog_synth.csv', 'records': paths[seq],
                                      'weights': {'config': wcfg, 'init': FACADE_WEIGHTS['init'], 'sha1': h.hexdigest()}}


def cache_windows():
    """The reference's RecDataBase.sample_cache (base.py:82-90) over small files with blank lines in odd places: six
    windows per file -> cache_windows.json (file text, cache size, windows)."""
    import tempfile
    from rl4rs.env import RecDataBase
    rng = np.random.RandomState(5)
    out = []
    with tempfile.TemporaryDirectory() as d:
        for trial in range(30):
            n = int(rng.randint(3, 40))
            lines = ['rec%d  ' % i if rng.rand() > 0.15 else ('' if rng.rand() > 0.5 else '   ') for i in range(n)]
            lines[1] = 'rec1'                                  # the line taken after a wrap
            text = '\n'.join(lines) + ('\n' if rng.rand() > 0.3 else '')
            cache = int(rng.randint(1, 25))
            path = os.path.join(d, 'log%d.csv' % trial)
            with open(path, 'w') as f:
                f.write(text)
            db = RecDataBase({'sample_file': path, 'cache_size': cache, 'is_eval': False}, None)
            windows = []
            for _ in range(6):
                db.reset()
                windows.append(list(db.sample_list))
            db.fp.close()
            out.append({'text': text, 'cache_size': cache, 'windows': windows})
    with open(os.path.join(HERE, 'cache_windows.json'), 'w') as f:
        json.dump(out, f, indent=0)


def main():
    install_stubs()
    from rl4rs.env.slate import SlateState, SlateRecEnv
    from rl4rs.env.seqslate import SeqSlateState, SeqSlateRecEnv
    from rl4rs.utils.datautil import FeatureUtil
    from rl4rs_amd import synth

    # ---------------- inputs (committed next to the expected outputs)
    cat_path = os.path.join(HERE, 'catalog_synth.csv')
    cat_text = synth.make_catalog_text(seed=1234)
    synth.write_text(cat_path, cat_text)
    sp = synth.special_ids_from_text(cat_text)
    rec_a = synth.make_records(6, pages=1, seed=1000, illegal_frac=0.5, special_ids=sp)
    rec_b = synth.make_records(6, pages=4, seed=2000, illegal_frac=0.5, special_ids=sp)
    rec_a_path, rec_b_path = os.path.join(HERE, 'records_slate.txt'), os.path.join(HERE, 'records_seq.txt')
    synth.write_records(rec_a_path, rec_a)
    synth.write_records(rec_b_path, rec_b)

    manifest = {}

    def emit(name, g, cfg, seq, conti, mask_flag, catalog, records):
        np.savez_compressed(os.path.join(HERE, name + '.npz'), **g)
        manifest[name] = {'config': cfg, 'seq': seq, 'conti': conti, 'mask_flag': mask_flag,
                          'catalog': catalog, 'records': records}

    for conti in (False, True):
        tag = 'conti' if conti else 'discrete'
        cfg = base_config(iteminfo_file=cat_path)
        g = run_scenario('slate_' + tag, SlateState, FeatureUtil, cfg, rec_a, False, conti,
                         np.random.RandomState(7), None, SlateRecEnv, rec_a_path)
        cfg['iteminfo_file'] = 'catalog_synth.csv'
        emit('slate_' + tag, g, cfg, False, conti, None, 'catalog_synth.csv', 'records_slate.txt')
        for T, flag in ((36, 'support_rllib_mask'), (32, None)):
            cfg = base_config(iteminfo_file=cat_path, max_steps=T)
            g = run_scenario('seq', SeqSlateState, FeatureUtil, cfg, rec_b, True, conti,
                             np.random.RandomState(11), flag, SeqSlateRecEnv, rec_b_path)
            cfg['iteminfo_file'] = 'catalog_synth.csv'
            emit('seq%d_%s' % (T, tag), g, cfg, True, conti, flag, 'catalog_synth.csv', 'records_seq.txt')

    # ---------------- support_onehot_action (slate.py:22-25; the continuous dataset of script/batchrl_trainer.py:224-225 is built
    # with it): the action embedding table is eye(284), a continuous action is a 284-d vector resolved by the masked K-NN
    cfg = base_config(iteminfo_file=cat_path, support_onehot_action=True)
    g = run_scenario('slate_onehot', SlateState, FeatureUtil, cfg, rec_a, False, True, np.random.RandomState(19), None,
                     SlateRecEnv, rec_a_path)
    assert g['action_emb'].shape == (284, 284) and g['action_in_0'].shape == (6, 284)
    cfg['iteminfo_file'] = 'catalog_synth.csv'
    emit('slate_onehot', g, cfg, False, True, None, 'catalog_synth.csv', 'records_slate.txt')

    # ---------------- BASELINE configs[0]: SlateRecEnv-v0 batch = 256, offline_action replay (the mask flags only change which
    # view of the state `state` returns - both views, obsmask_* and d3rl_*, are recorded at every step - so ONE episode serves
    # the plain, support_rllib_mask and support_d3rl_mask forms of the config)
    rec_c = synth.make_records(256, pages=1, seed=3000, illegal_frac=0.2, special_ids=sp)
    rec_c_path = os.path.join(HERE, 'records_slate256.txt')
    synth.write_records(rec_c_path, rec_c)
    cfg = base_config(iteminfo_file=cat_path, batch_size=256)
    g = run_scenario('slate256_discrete', SlateState, FeatureUtil, cfg, rec_c, False, False, np.random.RandomState(13), 'support_rllib_mask',
                     SlateRecEnv, rec_c_path)
    cfg['iteminfo_file'] = 'catalog_synth.csv'
    emit('slate256_discrete', compact(g), cfg, False, False, 'support_rllib_mask', 'catalog_synth.csv', 'records_slate256.txt')

    # ---------------- SeqSlateRecEnv-v0 at batch 64, 36 steps (4 pages), mask mode: the paging quirks (special-mask re-poisoning
    # across pages, page-0-only special check of get_violation, literal 9 of offline_reward) on a batch that fills two row tiles
    rec_d = synth.make_records(64, pages=4, seed=4000, illegal_frac=0.3, special_ids=sp)
    rec_d_path = os.path.join(HERE, 'records_seq64.txt')
    synth.write_records(rec_d_path, rec_d)
    cfg = base_config(iteminfo_file=cat_path, batch_size=64, max_steps=36)
    g = run_scenario('seq36_b64_discrete', SeqSlateState, FeatureUtil, cfg, rec_d, True, False, np.random.RandomState(17), 'support_rllib_mask',
                     SeqSlateRecEnv, rec_d_path)
    cfg['iteminfo_file'] = 'catalog_synth.csv'
    emit('seq36_b64_discrete', compact(g, min_bytes=60000), cfg, True, False, 'support_rllib_mask', 'catalog_synth.csv', 'records_seq64.txt')

    # ---------------- real data known answers (tutorial.ipynb cell 4 record + dataset/item_info.csv)
    # RL4RS dataset (c) fuxiAIlab, CC BY-SA 4.0 (reference LICENSE); one record and the public catalogue.
    nb = json.load(open(os.path.join(REF, 'tutorial.ipynb')))
    text = ''.join(nb['cells'][4]['outputs'][0]['text'])
    real_rec = text.split('\n')[1].strip()
    real_cat_src = os.path.join(REF, 'dataset', 'item_info.csv')
    real_cat = os.path.join(HERE, 'item_info_real.csv')
    synth.write_text(real_cat, open(real_cat_src).read())
    real_rec_path = os.path.join(HERE, 'records_real.txt')
    synth.write_records(real_rec_path, [real_rec])
    for conti in (False, True):
        tag = 'conti' if conti else 'discrete'
        cfg = base_config(iteminfo_file=real_cat, batch_size=1)
        g = run_scenario('real_' + tag, SlateState, FeatureUtil, cfg, [real_rec], False, conti,
                         np.random.RandomState(3), None, SlateRecEnv, real_rec_path)
        # tutorial cell 12: all-ones continuous action -> nearest item 53
        g['knn_ones'] = np.asarray(SlateState.get_nearest_neighbor(np.full((4, 32), 1), g['action_emb']))
        cfg['iteminfo_file'] = 'item_info_real.csv'
        emit('real_' + tag, g, cfg, False, conti, None, 'item_info_real.csv', 'records_real.txt')

    facade_scenarios(manifest, cat_path, sp)
    cache_windows()

    with open(os.path.join(HERE, 'manifest.json'), 'w') as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print('wrote', sorted(manifest))


if __name__ == '__main__':
    main()
