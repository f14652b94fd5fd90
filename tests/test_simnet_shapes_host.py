"""CPU checks, with the numpy restatement alone, that the cases of tests/test_gpu_simnet_shapes.py and the saturated-gate cases of
tests/test_gpu_simtrain_shapes.py are what those files say they are - from the very generators they import (tests/simnet_cases.py,
test_gpu_simtrain._simnet_case): the shape table lies inside what rl4rs_simnet_create admits, the 'saturated' cases do put keras
hard_sigmoid gates on both clamps while no lstm input of the older files puts a single one there (which is why the new cases exist),
the gradient cases keep clear of the kinks at +-2.5 and of the loss clamp, the yardsticks behind the bars are what the docstrings
quote, and the episode's histories lie on both sides of its maxlen."""
import os

import numpy as np
import pytest

import simnet_cases as sc
import test_gpu_simnet as old_scorer
import test_gpu_simtrain as old_train
import test_gpu_simtrain_shapes as shapes

SHARE = 0.10          # a 'saturated' case: at least this share of the gate pre-activations at or beyond each clamp


def _shares(pre):
    return float((pre <= -2.5).mean()), float((pre >= 2.5).mean())


def _train_preacts(kw, dtype=np.float64):
    from oracle.simnets import OracleSimnet
    w, dense, cat, labels, seqs = old_train._simnet_case(**kw)
    seq = np.stack(seqs, axis=1)
    return OracleSimnet('lstm', w, kw['cfg'], dtype), (seq, dense, cat)


@pytest.mark.parametrize('name', sorted(sc.SHAPES))
def test_shapes_lie_inside_what_create_admits(name):
    from rl4rs_amd.nets.simnets import init_simnet_weights, obs_dim
    algo, cfg = sc.SHAPES[name]
    for k, (lo, hi) in sc.CREATE_RANGES.items():
        assert lo <= cfg[k] <= hi, (name, k)
    for k, m in sc.CREATE_MULTIPLES.items():
        assert cfg[k] > 0 and cfg[k] % m == 0, (name, k)
    assert cfg['dense_feature_num'] > 0 and cfg['category_hash_size'] > 0
    if algo == 'lstm':
        assert cfg['emb_size'] == cfg['hidden_units'] == sc.LSTM_WIDTH
    if name == 'W2':
        assert obs_dim(cfg, algo) == 13216
    seq, dense, cat = sc.case_inputs(name, sc.TABLE_R)
    H = cfg['category_hash_size']
    assert seq.shape == (sc.TABLE_R, cfg['seq_num'], cfg['maxlen']) and cat.shape == (sc.TABLE_R, cfg['category_feature_num'])
    assert cat.min() == 0 and cat.max() == H - 1
    for s in range(cfg['seq_num']):
        assert seq[:, s].min() == 0 and seq[:, s].max() == H - 1, (name, s)
    assert set(init_simnet_weights(cfg, algo, seed=3)) >= {'cat_emb', 'out_w'}


def test_table_covers_the_listed_edges():
    cfgs = [sc.SHAPES[n][1] for n in sc.TABLE if sc.SHAPES[n][0] == 'lstm']
    assert {c['maxlen'] for c in cfgs} == {1, 16, 33} and {c['category_feature_num'] for c in cfgs} == {1, 13, 64}
    assert {c['seq_num'] for c in cfgs} == {1, 3, 4} and {c['class_num'] for c in cfgs} == {2, 3, 8}
    assert sc.ROW_COUNTS == [1, 31, 32, 33, 65] and sc.TABLE_R == 65
    assert sorted(sc.SHAPES[n][0] for n in sc.ROW_SWEEP.values()) == sorted(sc.ROW_SWEEP)


@pytest.mark.parametrize('name', sc.TABLE)
def test_fixed_bars_hold_on_the_table(name):
    """float32 alone stays under a quarter of the fixed bars on every table case, so simnet_cases.bar() returns them unchanged"""
    algo, cfg = sc.SHAPES[name]
    _, _, e_obs, e_prob = sc.yardstick(algo, sc.weights(name), cfg, *sc.case_inputs(name))
    assert e_obs <= sc.OBS_BAR / 4 and e_prob <= sc.PROB_BAR / 4, (e_obs, e_prob)
    assert sc.bar(sc.OBS_BAR, e_obs) == sc.OBS_BAR and sc.bar(sc.PROB_BAR, e_prob) == sc.PROB_BAR
    assert sc.bar(1.0, 0.3) == pytest.approx(1.2) and sc.bar(1.0, 0.25) == 1.0


@pytest.mark.parametrize('variant', sorted(sc.SAT_VARIANTS))
@pytest.mark.parametrize('name', sc.SATURATED)
def test_forward_cases_saturate_both_clamps(name, variant):
    from oracle.simnets import OracleSimnet
    algo, cfg = sc.SHAPES[name]
    x = sc.case_inputs(name)
    low, high = _shares(OracleSimnet(algo, sc.weights(name, saturated=variant), cfg, np.float64).gate_preacts(*x))
    assert low >= SHARE and high >= SHARE, (low, high)
    plain = OracleSimnet(algo, sc.weights(name), cfg, np.float64).gate_preacts(*x)
    assert np.abs(plain).max() < 2.5                  # the same case without the scaling: no gate off its linear arm
    if variant == 'kernel16':                         # keeps the fixed bars (test_gpu_simnet_shapes.py's docstring)
        _, _, e_obs, e_prob = sc.yardstick(algo, sc.weights(name, saturated=variant), cfg, *x)
        assert e_obs <= sc.OBS_BAR / 4 and e_prob <= sc.PROB_BAR / 4, (e_obs, e_prob)


@pytest.mark.parametrize('name', sorted(shapes.SATURATED))
def test_gradient_cases_saturate_and_keep_clear_of_the_kinks(name):
    """the conditions tests/test_gpu_simtrain_shapes.py states for its seeds: >= 10 % of the gate pre-activations at or beyond each
    clamp; none closer to +-2.5 than 10 x the largest float32-vs-float64 difference of one; every class probability inside
    [1e-6, 1 - 1e-6] (no dropout, so the training forward is this forward)"""
    kw = shapes.saturated_case(name)
    assert kw['rate'] == 0.0 and kw['N'] == 9 and kw['cfg']['maxlen'] == 4 and kw['cfg']['category_feature_num'] == 3
    o64, x = _train_preacts(kw)
    o32, _ = _train_preacts(kw, np.float32)
    pre = o64.gate_preacts(*x)
    e_pre = float(np.abs(o32.gate_preacts(*x).astype(np.float64) - pre).max())
    low, high = _shares(pre)
    assert low >= SHARE and high >= SHARE, (low, high)
    assert sc.kink_margin(pre) >= 10 * e_pre, (sc.kink_margin(pre), e_pre)
    p = o64.reward_probs(*x)
    assert p.min() >= 1e-6 and p.max() <= 1 - 1e-6
    # the hook is the x8 of simnet_cases and reaches the trainer's weights
    w = old_train._simnet_case(**kw)[0]
    w0 = old_train._simnet_case(**dict(kw, weight_hook=None))[0]
    assert np.array_equal(w['cat_gru_kernel'], w0['cat_gru_kernel'] * np.float32(8)) and np.array_equal(w['obs_w'], w0['obs_w'])
    assert np.array_equal(w['seq1_gru_recurrent'], w0['seq1_gru_recurrent'] * np.float32(8))


def test_gradient_cases_cover_every_gru_implementation():
    got = dict((n, shapes._gru_persistent(cfg, shapes.SATURATED_N)) for n, (cfg, _, _) in shapes.SATURATED.items())
    assert got == {'w128': True, 'w256': True, 'steps': False}
    assert shapes.SATURATED['w128'][0]['hidden_units'] == 128 and shapes.SATURATED['w256'][0]['hidden_units'] == 256
    steps = shapes.SATURATED['steps'][0]
    assert (steps['emb_size'], steps['hidden_units']) == (72, 96)


def _old_scorer_cases():
    from rl4rs_amd.nets.simnets import init_simnet_weights
    cfg = old_scorer.CFG
    for R in (5, 200):                                 # test_simnet_rowwise_matches_oracle
        yield 'rowwise %d' % R, cfg, init_simnet_weights(cfg, 'lstm', seed=3, emb_scale=0.5, bias_noise=0.2), \
            old_scorer._inputs(R, np.random.RandomState(R), cfg['category_hash_size'])
    rs = np.random.RandomState(11)                     # test_simnet_grouped_slots_prob_only
    seq_env, _, _ = old_scorer._inputs(7, rs, cfg['category_hash_size'])
    _, dense, cat = old_scorer._inputs(63, rs, cfg['category_hash_size'])
    yield 'grouped', cfg, init_simnet_weights(cfg, 'lstm', seed=4, emb_scale=0.3, bias_noise=0.1), (np.repeat(seq_env, 9, axis=0), dense, cat)


def test_no_older_scorer_input_saturates_a_gate():
    from oracle.simnets import OracleSimnet
    for tag, cfg, w, x in _old_scorer_cases():
        pre = OracleSimnet('lstm', w, cfg, np.float64).gate_preacts(*x)
        assert np.abs(pre).max() < 2.5, tag


@pytest.mark.parametrize('seq,T', [(False, 9), (True, 18)])
def test_no_older_episode_saturates_a_gate(tmp_path, seq, T):
    """test_gpu_simnet.py::test_episode_with_other_simulators, lstm: every scorer call of the oracle env's episode"""
    from rl4rs_amd import synth
    from rl4rs_amd.nets.simnets import init_simnet_weights
    from oracle.simnets import OracleSimnet
    from oracle.env import OracleEnv

    class Recording(OracleSimnet):
        largest = 0.0

        def obs(self, seq, dense, cat, pre=None):
            pre = []
            out = OracleSimnet.obs(self, seq, dense, cat, pre=pre)
            self.largest = max([self.largest] + [float(np.abs(p).max()) for p in pre])
            return out

    B = 10
    d = str(tmp_path)
    cat_path = os.path.join(d, 'item_info.csv')
    cat_text = synth.make_catalog_text(seed=21)
    synth.write_text(cat_path, cat_text)
    records = synth.make_records(B + 5, pages=2 if seq else 1, seed=8, illegal_frac=0.3, hash_size=5000,
                                 special_ids=synth.special_ids_from_text(cat_text))
    cfg = {"maxlen": 64, "batch_size": B, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
           "category_feature_num": 21, "category_hash_size": 5000, "seq_num": 2, "emb_size": 128,
           "page_items": 9, "hidden_units": 128, "max_steps": T, "action_emb_size": 32,
           "iteminfo_file": cat_path, "is_eval": True, "cache_size": B, "algo": 'lstm'}
    scorer = Recording('lstm', init_simnet_weights(cfg, 'lstm', seed=5, emb_scale=0.5, bias_noise=0.2), cfg, np.float64)
    orc = OracleEnv(cfg, records[:B], scorer, seq=seq)
    orc.reset()
    for t in range(T):
        orc.step(orc.samples.offline_action)
    assert 0.0 < scorer.largest < 2.5


def _old_train_cases():
    for N in (256, 700):                               # test_gradients_match_autograd
        for rate in (0.0, 0.2):
            yield dict(algo='lstm', rate=rate, N=N)
    yield dict(algo='lstm', rate=0.2, N=203)           # test_lstm_gradients_in_both_recurrence_tile_forms (N = 256: above)
    for N in (256, 43):                                # test_lstm_gradients_width_256_hard_gates
        yield dict(algo='lstm', rate=0.2, N=N, cfg=shapes.LSTM_VARIANTS['w256'][0], front_pad=True)
    for name in ('steps_width', 'steps_length', 'w128_cn13', 'w128_cn32'):      # test_lstm_gradients_other_configurations
        yield dict(algo='lstm', rate=0.2, N=43, cfg=shapes.LSTM_VARIANTS[name][0], front_pad=True)


@pytest.mark.parametrize('kw', list(_old_train_cases()), ids=lambda kw: '%d-%s-%s' % (kw['N'], kw['rate'], sorted(
    set(kw.get('cfg', {}).items()) - set(old_train.CFG.items()))))
def test_no_older_training_input_saturates_a_gate(kw):
    """the lstm batches of tests/test_gpu_simtrain.py and of the earlier tests of tests/test_gpu_simtrain_shapes.py (dropout acts on
    the dense tower only, so the gates do not depend on it)"""
    kw = dict(kw)
    kw.setdefault('cfg', old_train.CFG)
    o64, x = _train_preacts(kw)
    assert np.abs(o64.gate_preacts(*x)).max() < 2.5


def test_episode_histories_lie_on_both_sides_of_maxlen():
    _, records = sc.episode_records()
    assert len(records) == sc.EPISODE_B + 5
    lengths = sc.history_lengths(records[:sc.EPISODE_B])
    assert max(lengths) > sc.EPISODE_MAXLEN and min(lengths) < sc.EPISODE_MAXLEN, lengths
    assert 1 <= sc.EPISODE_MAXLEN <= 64


@pytest.mark.parametrize('name', sorted(shapes.SATURATED))
def test_float32_autograd_stays_under_a_quarter_of_the_gradient_bars(name):
    """oracle.simnets.loss_and_grad(dtype=float32), the yardstick of the saturated gradient cases: float32 arrays, and on each case
    within a quarter of the loss bar (1e-5 relative) and of the gradient bar (2e-4 of each array's largest entry) of the float64
    form - so _check_simnet_gradients keeps the file's own bars on them"""
    from oracle.simnets import loss_and_grad
    kw = shapes.saturated_case(name)
    w, dense, cat, labels, seqs = old_train._simnet_case(**kw)
    l64, g64 = loss_and_grad('lstm', w, dense, cat, labels, seqs, class_num=2)
    l32, g32 = loss_and_grad('lstm', w, dense, cat, labels, seqs, class_num=2, dtype=np.float32)
    assert abs(l32 - l64) <= 1e-5 * max(1.0, abs(l64)) / 4
    assert set(g32) == set(g64) == set(w)
    for k in g64:
        assert g32[k].dtype == np.float32 and g64[k].dtype == np.float64
        assert np.abs(g32[k] - g64[k]).max() <= 2e-4 * np.abs(g64[k]).max() / 4, k
