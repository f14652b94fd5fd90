"""CPU: the MDP checker's host side - the restatement's beam search against the reference's own output (tests/golden/mdp_beam_*.npz,
made by tests/golden/make_mdp_golden.py), the script's dataset windowing, the two experiments' printed quantities, Spearman with
ties, the refusals, and the C ABI's new symbols."""
import os
import re

import numpy as np
import pytest

import mdp_ref
from conftest import GOLDEN, REPO


@pytest.mark.parametrize('name', mdp_ref.GOLDEN_CASES)
def test_restatement_search_reproduces_the_reference(name):
    """the search the GPU tests lean on is the reference's beam_search, exactly: paths, order and float64 scores"""
    c = mdp_ref.load_case(GOLDEN, name)
    paths, scores, sp, margin = mdp_ref.beam_search_ref(mdp_ref.RefSeq2Seq(c['V'], c['d'], c['h'], c['flat']), c['enc'], c['K'], c['T'], c['C'])
    assert np.array_equal(paths, c['paths'])
    assert np.array_equal(scores, c['scores'])
    assert np.array_equal(sp.prod(axis=2), scores) or np.allclose(sp.prod(axis=2), scores, rtol=1e-14, atol=0)
    # the fixtures' seeds leave at least half of the users of every case clear of the error bar at every selection
    assert (margin > mdp_ref.BEAM_REL_BAR[c['d']]).mean() >= 0.5


def test_golden_cases_are_the_specified_ones():
    want = {'n3_v37_k4': (3, 37, 4, None, 64, 48), 'n70_v37_k8': (70, 37, 8, None, 64, 48), 'n4_v37_k1': (4, 37, 1, None, 64, 48),
            'n3_v50_k6_c9': (3, 50, 6, 9, 64, 48), 'n2_v290_k100': (2, 290, 100, None, 256, 128),
            'n2_v290_k20_c20': (2, 290, 20, 20, 256, 128)}
    for name, shape in want.items():
        c = mdp_ref.load_case(GOLDEN, name)
        assert (c['N'], c['V'], c['K'], c['C'], c['d'], c['h']) == shape
        assert os.path.getsize(os.path.join(GOLDEN, 'mdp_beam_%s.npz' % name)) < 64 * 1024
    c = mdp_ref.load_case(GOLDEN, 'n70_v37_k8')
    assert (c['S'], c['T']) == (5, 3) and ((c['enc'] == 0).sum(axis=1) > 0).sum() == 2


# ---------------------------------------------------------------- datasets
def test_build_dataset_fixed_window():
    from rl4rs_amd.mdpchecker import build_dataset
    items = [str(100 + i) for i in range(21)]
    lines = ['s1 ' + ','.join(items), 's2 ' + ','.join(items[:20]), 's3 ' + ','.join(reversed(items))]
    d = build_dataset(lines, 'rl4rs')
    assert d['source_len'] == 16 and d['encode_input'].shape == (2, 18) and d['decode_input'].shape == (2, 7)
    assert d['decode_output'].shape == (2, 7, 1)
    # one dictionary, grown over the sources first and then the targets
    assert d['encode_input'][0].tolist() == [1] + list(range(3, 19)) + [2]
    # s3's source is items 120 .. 105: 120 .. 116 are new and numbered 19 .. 23 before any target is looked at
    assert d['encode_input'][1].tolist() == [1, 19, 20, 21, 22, 23] + list(range(18, 7, -1)) + [2]
    assert d['decode_input'][0].tolist() == [1, 23, 22, 21, 20, 19, 2]
    assert d['decode_output'][0, :, 0].tolist() == [23, 22, 21, 20, 19, 2, 0]
    assert d['decode_input'][1].tolist() == [1, 7, 6, 5, 4, 3, 2]
    assert d['token_num'] == 3 + 21


def test_build_dataset_source_len_rule_and_sliding_window():
    from rl4rs_amd.mdpchecker import build_dataset, source_len_of
    assert (source_len_of('recsys15'), source_len_of('cikm2016'), source_len_of('lastfm'), source_len_of('rl4rs')) == (8, 5, 16, 16)
    items = [str(i) for i in range(40)]
    d = build_dataset(['u ' + ','.join(items)], 'recsys15')
    # the script's strides: np.random.seed(1), then randint(8, 13) // 6 per window while i + 13 < 40
    np.random.seed(1)
    starts, i = [], 0
    while i + 13 < 40:
        starts.append(i)
        i += np.random.randint(8, 13) // 6
    assert d['encode_input'].shape == (len(starts), 10)
    inv = {v: k for k, v in d['token_dict'].items()}
    assert [int(inv[r[1]]) for r in d['encode_input']] == starts
    assert [int(inv[r[1]]) for r in d['decode_input']] == [s + 8 for s in starts]
    d = build_dataset(['u ' + ','.join(items)], 'cikm2016')
    assert d['encode_input'].shape == (1, 7) and d['decode_input'].shape == (1, 7)


def test_rl4rs_sessions_from_dataset_a_records():
    from rl4rs_amd.mdpchecker import build_dataset, rl4rs_sessions
    records = open(os.path.join(GOLDEN, 'records_slate.txt')).read().split('\n')
    records = [r for r in records if r]
    short = records[0].split('@')
    short[1], short[5] = 'short', ','.join(short[5].split(',')[:15])
    records.insert(2, '@'.join(short))                            # 15 history ids: one too few
    lines = rl4rs_sessions(records)
    long = [r for r in records if len(r.split('@')[5].split(',')) >= 16]
    assert 0 < len(lines) == len(long) == len(records) - 1 and not any(l.startswith('short ') for l in lines)
    first = long[0].split('@')
    sid, items = lines[0].split(' ')
    assert sid == first[1] and items.split(',') == first[5].split(',')[-16:] + first[3].split(',')[:5]
    assert all(len(l.split(' ')[1].split(',')) == 21 for l in lines)
    d = build_dataset(lines, 'rl4rs')
    assert d['encode_input'].shape == (len(lines), 18) and d['decode_input'].shape == (len(lines), 7)
    assert d['encode_input'].max() < d['token_num'] and (d['encode_input'][:, 0] == 1).all() and (d['encode_input'][:, -1] == 2).all()


# ---------------------------------------------------------------- experiments
def test_experiments_reproduce_the_recorded_quantities():
    from rl4rs_amd import mdpchecker as M
    z = np.load(os.path.join(GOLDEN, 'mdp_experiments.npz'))
    B = int(z['cfg'][2])
    two = M.experiment_II(B, z['greedy_score'], z['beam_score'], z['hot_score'])
    assert np.abs(np.array(two) - z['experiment_II']).max() <= 1e-12
    one = M.experiment_I(z['token_probs'])
    assert one.shape == z['experiment_I'].shape and np.abs(one - z['experiment_I']).max() <= 1e-12


def test_experiment_II_slices_the_hot_beams_by_the_wide_beam_size():
    from rl4rs_amd import mdpchecker as M
    rs = np.random.RandomState(0)
    beam = -np.sort(-rs.rand(4, 100), axis=1)
    hot = -np.sort(-rs.rand(4, 20), axis=1)
    greedy = beam[:, :1]
    two = M.experiment_II(100, greedy, beam, hot)
    top5 = beam[:, :5].mean(axis=1)
    want = (np.mean(beam[:, :20].mean(axis=1) / top5), np.mean(greedy[:, 0] / top5), np.mean(hot[:, :5].mean(axis=1) / top5),
            np.mean(hot[:, :20].mean(axis=1) / top5))
    assert np.allclose(two, want, rtol=1e-14)
    beam[0, 1] = np.nan                                            # nanmean, as the script
    assert np.isfinite(M.experiment_II(100, greedy, beam, hot)).all()


def test_experiment_I_counts_a_constant_prefix_as_correlation_one():
    from rl4rs_amd import mdpchecker as M
    sp = np.random.RandomState(1).rand(2, 6, 3)
    sp[0, :, 0] = 0.25                                             # every beam of user 0 shares its first token: corrcoef is nan -> 1
    one = M.experiment_I(sp)
    only = M.experiment_I(sp[:1])
    assert only[0].tolist() == [1.0, 1.0] and np.allclose(one[-1], 1.0) and np.isfinite(one).all()


def test_spearman_with_ties_is_scipys():
    from rl4rs_amd.mdpchecker import spearman
    z = np.load(os.path.join(GOLDEN, 'mdp_experiments.npz'))
    assert len(np.unique(z['tie_x'])) < len(z['tie_x'])            # ties are there
    assert abs(spearman(z['tie_x'], z['tie_y']) - float(z['tie_spearman'])) <= 1e-12
    assert spearman([1, 2, 3, 4], [10, 20, 30, 40]) == pytest.approx(1.0)
    assert spearman([1, 1, 2, 2], [1, 2, 1, 2]) == pytest.approx(0.0)
    assert np.isnan(spearman([1, 1, 1], [1, 2, 3]))


# ---------------------------------------------------------------- refusals, layout, ABI
def test_unsupported_arguments_raise():
    from rl4rs_amd.mdpchecker import Seq2SeqTransformer, beam_search, token_probs
    for kw in (dict(encoder_num=2), dict(decoder_num=2), dict(head_num=4), dict(use_same_embed=True), dict(embed_dim=63),
               dict(dropout_rate=1.0)):
        with pytest.raises(ValueError):
            Seq2SeqTransformer(token_num=40, **kw)
    with pytest.raises(ValueError):
        Seq2SeqTransformer(token_num=3)

    class Other(object):
        def predict(self, x):
            raise AssertionError('no CPU path')
    enc = np.ones((2, 6), dtype=np.int32)
    with pytest.raises(TypeError):
        beam_search(Other(), enc, 2, 3)
    with pytest.raises(TypeError):
        token_probs(Other(), enc, enc[:, :1])
    m = Seq2SeqTransformer(token_num=40, embed_dim=16, hidden_dim=8)
    with pytest.raises(ValueError, match='candidates_size'):
        beam_search(m, enc, 4, 3, use_candidates=True, candidates_size=3)
    with pytest.raises(ValueError, match='candidates_size'):
        beam_search(m, enc, 4, 3, use_candidates=True)


def test_weights_round_trip_and_layout(tmp_path):
    import ctypes as C
    from rl4rs_amd import _lib
    from rl4rs_amd.build import build_lib
    from rl4rs_amd.mdpchecker import Seq2SeqTransformer, param_layout
    build_lib()
    lib = _lib.load()
    V, d, h = 41, 32, 20
    m = Seq2SeqTransformer(token_num=V, embed_dim=d, hidden_dim=h, seed=3)
    cfg = _lib.Seq2SeqCfg(V, d, h, 18, 7, 64)
    assert lib.rl4rs_seq2seq_param_count(C.byref(cfg)) == m.params.size == sum(int(np.prod(s)) for _, s in param_layout(V, d, h))
    assert [int(np.prod(s)) for _, s in param_layout(V, d, h)] == [int(np.prod(s)) for _, s in mdp_ref.layout(V, d, h)]
    w = m.get_weights()
    assert np.abs(w['encoder_embedding']).max() <= 0.05 and (w['encoder_ffn/ln_gamma'] == 1).all() and (w['output_bias'] == 0).all()
    assert abs(w['decoder_self_attention/Wq'].std() - np.sqrt(2.0 / (2 * d))) < 0.02
    path = str(tmp_path / 'w.npz')
    m.save_weights(path)
    other = Seq2SeqTransformer(token_num=V, embed_dim=d, hidden_dim=h, seed=4)
    assert not np.array_equal(other.params, m.params)
    other.load_weights(path)
    assert np.array_equal(other.params, m.params)
    with pytest.raises(ValueError):
        Seq2SeqTransformer(token_num=V + 1, embed_dim=d, hidden_dim=h).load_weights(path)


def test_library_refuses_bad_shapes_before_it_looks_for_a_device():
    import ctypes as C
    from rl4rs_amd import _lib
    from rl4rs_amd.build import build_lib
    build_lib()
    lib = _lib.load()
    for bad in ((3, 64, 48, 18, 7, 64), (4, 2, 1, 1, 1, 1 << 25), (40, 63, 48, 18, 7, 64), (40, 64, 48, 65, 7, 64), (40, 64, 48, 18, 0, 64), (40, 64, 48, 18, 7, 0),
                (60853, 256, 128, 7, 7, 1 << 20)):
        cfg = _lib.Seq2SeqCfg(*bad)
        assert lib.rl4rs_seq2seq_param_count(C.byref(cfg)) == -1, bad
        h = C.c_void_p()
        dummy = np.zeros(1, dtype=np.float32)
        assert lib.rl4rs_seq2seq_create(C.byref(cfg), dummy.ctypes.data_as(C.c_void_p), None, C.byref(h)) == -1 and not h.value, bad
    assert '2^31' in lib.rl4rs_last_error().decode()


def test_header_declares_the_seq2seq_symbols():
    from rl4rs_amd import _lib
    text = open(os.path.join(REPO, 'include', 'rl4rs_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(rl4rs_seq2seq_[a-z0-9_]+)\s*\(', text))
    assert declared == {'rl4rs_seq2seq_param_count', 'rl4rs_seq2seq_create', 'rl4rs_seq2seq_destroy', 'rl4rs_seq2seq_params',
                        'rl4rs_seq2seq_adam_state', 'rl4rs_seq2seq_set_adam_step', 'rl4rs_seq2seq_loss_grad', 'rl4rs_seq2seq_adam_step',
                        'rl4rs_seq2seq_forward', 'rl4rs_seq2seq_beam'}
    assert declared <= set(_lib.SIGNATURES)
