#!/usr/bin/env python
"""Generate the off-policy-evaluation fixtures (tests/golden/ope_*.npz) by running the REFERENCE's own code:

* ``ope_estimators.npz``  the six functions of rl4rs/utils/offline_policy_metrics.py on the float64 inputs of
  ``tests/ope_inputs.estimator_inputs`` (gamma 1.0 and 0.9 for WIPS);
* ``ope_tquantile.npz``   ``scipy.stats.t.ppf(0.99875, df)`` - what offline_policy_metrics.py:38 calls;
* ``ope_behavior.npz``    ``behavior_model.action_probs`` (rl4rs/policy/behavior_model.py:44-58) called unbound on a fake ``self``
  whose ``model.predict`` returns the seeded ``y [B, 382]``, layers 1..4;
* ``ope_loop.npz``        ``ope_eval`` (script/offline_evaluation.py:9-73) over the table-driven fakes of
  ``tests/ope_inputs.LoopTables``, its two printed arrays recorded.

The reference modules are loaded from their files under stub ``gym`` / ``tensorflow`` / ``rl4rs.*`` modules (nothing of them is
copied; the fixtures hold arrays, seeds and short tags only).  Needs the reference checkout and scipy: run it where both exist.

    python tests/golden/make_ope_golden.py [--out DIR]

It ends by re-loading what it wrote and comparing."""
import argparse
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = '/root/reference'
sys.path.insert(0, os.path.dirname(HERE))
import ope_inputs as I  # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def load_reference():
    """the three reference modules, imported under stubs for what they import but do not need here"""
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class _Session(object):
        def as_default(self):
            return self

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

    mod('gym')
    keras = mod('tensorflow.keras')
    mod('tensorflow', keras=keras, Session=_Session)
    mod('rl4rs')
    mod('rl4rs.utils')
    mod('rl4rs.policy')
    mod('rl4rs.utils.datautil', FeatureUtil=object)
    mod('rl4rs.policy.policy_model', policy_model=lambda algo, config: algo)
    metrics = _load('rl4rs.utils.offline_policy_metrics', os.path.join(REF, 'rl4rs', 'utils', 'offline_policy_metrics.py'))
    sys.modules['rl4rs.utils'].offline_policy_metrics = metrics
    behavior = _load('rl4rs.policy.behavior_model', os.path.join(REF, 'rl4rs', 'policy', 'behavior_model.py'))
    evaluation = _load('ref_offline_evaluation', os.path.join(REF, 'script', 'offline_evaluation.py'))
    return metrics, behavior, evaluation, _Session


def estimators(metrics):
    cases = np.asarray(I.ESTIMATOR_CASES, dtype=np.int64)
    expected = np.zeros((len(cases), len(I.ESTIMATOR_NAMES), 2))
    for i, (B, T, seed) in enumerate(I.ESTIMATOR_CASES):
        x = I.estimator_inputs(B, T, seed)
        ep = (x['rewards'], x['pi_mul'], x['mu_mul'])
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            expected[i] = [metrics.eval_IPS(*ep), metrics.eval_CIPS(*ep), metrics.eval_SNIPS(*ep),
                           metrics.eval_doubly_robust(x['episode_reward'], x['q_mean'], *ep),
                           metrics.eval_WIPS(x['step_rewards'], x['pi'], x['mu']),
                           metrics.eval_WIPS(x['step_rewards'], x['pi'], x['mu'], gamma=0.9),
                           metrics.eval_seq_doubly_robust(x['rhat'], x['q'], x['step_rewards'], x['pi'], x['mu'])]
    # conditions on the inputs, so that the fixture cannot hide a failure
    names = I.ESTIMATOR_NAMES
    for i, (B, T, seed) in enumerate(I.ESTIMATOR_CASES):
        if B >= 64:
            twelve = expected[i][[names.index(n) for n in ('CIPS', 'SNIPS', 'DR', 'WIPS', 'WIPS_gamma0.9', 'SeqDR')]]
            assert np.isfinite(twelve).all() and (np.abs(twelve) < 1e6).all(), (B, T, twelve)
    wips = expected[:, names.index('WIPS'), 0]
    assert (np.abs(wips - 1.0) > 1e-3).any(), wips
    assert np.isnan(expected[:, names.index('CIPS'), 1]).any(), 'no case records the int(n_e) - 1 <= 0 path'
    return dict(cases=cases, expected=expected)


def tquantile():
    import scipy.stats
    df = np.asarray(I.T_QUANTILE_DF, dtype=np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        expected = np.asarray([scipy.stats.t.ppf(I.T_QUANTILE_P, int(d)) for d in I.T_QUANTILE_DF], dtype=np.float64)
    assert np.isnan(expected[:2]).all() and np.isfinite(expected[2:]).all()
    return dict(df=df, p=np.float64(I.T_QUANTILE_P), expected=expected)


def behavior(behavior_mod, session_cls):
    y, actions = I.behavior_inputs()

    class _FakeSelf(object):
        sess = session_cls()
        featureutil = types.SimpleNamespace(feature_extraction=lambda inputs: [(None, None, None, None)])
        model = types.SimpleNamespace(predict=lambda inputs: y)

        @staticmethod
        def record2input(record, page=0):
            return record

    expected = np.stack([behavior_mod.behavior_model.action_probs(_FakeSelf(), None, actions, layer, page=0)
                         for layer in I.BEHAVIOR['layers']])
    assert expected.shape == (len(I.BEHAVIOR['layers']), len(actions)) and np.isfinite(expected).all()
    assert np.array_equal(expected[2], expected[3])           # layer 4 falls into the third range
    return dict(actions=actions, layers=np.asarray(I.BEHAVIOR['layers'], dtype=np.int64), expected=expected)


def loop(evaluation):
    cases = np.asarray(I.LOOP_CASES, dtype=np.int64)
    mean = np.full((len(cases), 4, 2), np.nan)
    std = np.full((len(cases), 4, 2), np.nan)
    for i, (B, T, with_model, seed) in enumerate(I.LOOP_CASES):
        fake = I.LoopTables(B, T, seed)
        printed = []
        evaluation.print = lambda *a, **k: printed.append(a)
        config = dict(epoch=I.LOOP_EPOCHS, batch_size=B, max_steps=T, page_items=9)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            evaluation.ope_eval(config, fake, fake, sample_model=fake if with_model else None)
        arrays = [a[0] for a in printed if len(a) == 1]
        assert len(arrays) == 2 and fake.epoch == I.LOOP_EPOCHS - 1 and fake.j == T
        if with_model:
            mean[i], std[i] = arrays
            assert np.isfinite(mean[i]).all() and (std[i][:, 0] > 0).all(), (B, T, std[i])
        else:
            assert np.isnan(arrays[0]).all() and np.isnan(arrays[1]).all()
    return dict(cases=cases, mean=mean, std=std)


def generate():
    metrics, behavior_mod, evaluation, session_cls = load_reference()
    return {'ope_estimators.npz': estimators(metrics), 'ope_tquantile.npz': tquantile(),
            'ope_behavior.npz': behavior(behavior_mod, session_cls), 'ope_loop.npz': loop(evaluation)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=HERE)
    args = ap.parse_args()
    files = generate()
    for name, arrays in files.items():
        path = os.path.join(args.out, name)
        np.savez(path, **arrays)
        with np.load(path) as z:
            assert sorted(z.files) == sorted(arrays)
            for k, v in arrays.items():
                assert np.array_equal(z[k], np.asarray(v), equal_nan=True) and z[k].dtype == np.asarray(v).dtype, (name, k)
        print('%s: %d bytes' % (name, os.path.getsize(path)))


if __name__ == '__main__':
    main()
