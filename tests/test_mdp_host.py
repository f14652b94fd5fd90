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


# ---------------------------------------------------------------- the cases of tests/test_gpu_mdp_shapes.py, checked without a device
def _offsets(V, d, h):
    out, o = {}, 0
    for name, shape in mdp_ref.layout(V, d, h):
        out[name] = o
        o += int(np.prod(shape))
    return out


def _gemm_constants():
    """the tiering constants of launch_gemm_f32, read from the source: a change there has to revisit the shape table"""
    text = open(os.path.join(REPO, 'rl4rs_amd', 'csrc', 'gemm.hip')).read()
    gbm, gbn = (int(v) for v in re.search(r'constexpr int GBM = (\d+), GBN = (\d+),', text).groups())
    small = int(re.search(r'SMALL_GEMM_MAX_BIG_BLOCKS = (\d+);', text).group(1))
    assert re.search(r'grid\.x \* grid\.y < SMALL_GEMM_MAX_BIG_BLOCKS \|\| N <= 32', text)
    assert re.search(r'if \(M >= 2048 && N >= 96 && K >= 32 && \(K & 3\) == 0 && \(N & 3\) == 0 && \(lda & 3\) == 0 && \(ldw & 3\) == 0', text)
    return gbm, gbn, small


def _gemm_form(M, N, K, lda, ldw, aligned=True):
    """the form launch_gemm_f32 takes (gemm.hip), restated"""
    gbm, gbn, small = _gemm_constants()
    if -(-M // gbm) * -(-N // gbn) < small or N <= 32:
        return 'small'
    if M >= 2048 and N >= 96 and K >= 32 and K % 4 == 0 and N % 4 == 0 and lda % 4 == 0 and ldw % 4 == 0 and aligned:
        return 't128'
    return 'f32'


def test_shape_cases_enter_the_paths_their_comments_name():
    cases = mdp_ref.SHAPE_CASES
    assert cases[:9] == ((3, 64, 64, 37, 64, 48), (4, 3, 9, 37, 64, 48), (5, 1, 1, 37, 64, 48), (5, 7, 5, 41, 66, 7), (5, 7, 5, 41, 100, 33),
                         (5, 7, 5, 41, 6, 1), (36, 64, 8, 292, 128, 100), (36, 64, 8, 292, 128, 102), (70, 64, 33, 292, 128, 100))
    assert sorted(mdp_ref.SHAPE_BARS) == list(range(len(cases))) and list(mdp_ref.SHAPE_DROP_HALF) == [4]
    text = open(os.path.join(REPO, 'rl4rs_amd', 'csrc', 'seq2seq.hip')).read()
    assert 'constexpr int S2S_MAXLEN = 64;' in text and 'constexpr int S2S_BEAM_MAX = 128;' in text
    assert 'return std::max(256, (Ns + 15) / 16);' in text                       # s2s_chunk
    chunk = lambda rows: max(256, (rows + 15) // 16)
    for i, (N, S, L, V, d, h) in enumerate(cases):
        V_, d_, h_, flat, enc, dec = mdp_ref.shape_case(i)
        assert (V_, d_, h_) == (V, d, h) and enc.shape == (N, S) and dec.shape == (N, L)
        assert (enc == 0).any() and (dec == 0).any() and enc.max() < V and dec.max() < V             # PAD keys on both sides
        out = mdp_ref.shape_targets(i)
        assert out.shape == dec.shape and ((dec != 0) & (out != 0)).any()
    assert cases[0][1] == cases[0][2] == 64                                          # every lane a key
    assert cases[1][2] > cases[1][1] and cases[2][1:3] == (1, 1)
    assert (mdp_ref.shape_case(2)[4][0] == 0).all() and mdp_ref.shape_case(2)[5][1, 0] == 0          # S = 1, L = 1: whole rows masked
    # widths: the tail guard of the 64-strides, and what the flat offsets do to 16-byte alignment
    for i, tail, d4, aligned_after_ffn in ((3, True, 2, False), (4, True, 0, False), (5, True, 2, False), (6, False, 0, True), (7, False, 0, False)):
        N, S, L, V, d, h = cases[i]
        o = _offsets(V, d, h)
        assert (d % 64 != 0) == tail and d % 4 == d4
        later = [o[k] % 4 == 0 for k in ('ef.W2', 'ds.Wq', 'dc.Wk', 'df.W1')]
        assert all(later) if aligned_after_ffn else not any(later), (i, later)
    assert all(_offsets(41, 66, 7)[k] % 4 for k in ('ds.Wq', 'dc.Wv', 'df.W2'))      # d % 4 == 2 and odd hidden: nothing behind ef.b1 aligned
    # row tiers
    form = lambda rows, n, k, **kw: _gemm_form(rows, n, k, k, n, **kw)
    for i in (6, 7):
        N, S, L, V, d, h = cases[i]
        assert N * S == 2304 and chunk(N * S) == 256 and -(-N * S // 256) == 9 and form(N * S, d, d) == 'small'
    N, S, L, V, d, h = cases[8]
    assert N * S == 4480 and chunk(N * S) == 280 and 280 % 16 and -(-N * S // 280) == 16
    assert N * L == 2310 and _gemm_form(N * L, V, d, d, (V + 3) & ~3) == 'small' and form(N * S, d, d) == 'small'
    for i, aligned in ((9, True), (10, False)):
        N, S, L, V, d, h = cases[i]
        assert chunk(N * S) == 380 and form(N * S, d, d) == 't128' and form(N * S, 2 * d // 2, d) == 't128'                  # ea, KV + D
        assert form(N * S, h, d, aligned=aligned) == ('t128' if aligned else 'f32')                                          # ef.W1
        assert form(N * S, d, h, aligned=aligned) == ('t128' if aligned else 'f32')                                          # ef.W2, K = hidden
        assert form(N * S, d, d, aligned=aligned) == ('t128' if aligned else 'f32')                                          # dc.Wk / Wv on the encoder rows
        assert V % 4 == 0 and _gemm_form(N * L, V, d, d, (V + 3) & ~3) == 't128'                                             # tied output layer
        assert (_offsets(V, d, h)['dc.Wk'] % 4 == 0) == aligned
    # every case stays inside what s2s_check_cfg admits
    assert all(S <= 64 and L <= 64 and d % 2 == 0 and d >= 2 and h >= 1 and V >= 4 for N, S, L, V, d, h in cases)


class _DetachedMax(mdp_ref.RefSeq2Seq):
    """the restatement with the max of the scores taken as a constant: its gradient lacks the max-shift term"""

    def _att(self, pre, xq, xkv, key_open, causal):
        import torch
        p = self.p
        q = xq @ p[pre + 'Wq'] + p[pre + 'bq']
        k = xkv @ p[pre + 'Wk'] + p[pre + 'bk']
        v = xkv @ p[pre + 'Wv'] + p[pre + 'bv']
        s = q @ k.transpose(1, 2) / np.sqrt(self.d)
        e = torch.exp(s - s.max(-1, keepdim=True).values.detach())
        mask = key_open[:, None, :].to(self.dtype)
        if causal:
            L = xq.shape[1]
            mask = mask * torch.tril(torch.ones(L, L, dtype=self.dtype))[None]
        e = e * mask
        a = e / (e.sum(-1, keepdim=True) + 1e-7)
        return self._ln(xq + self._drop((a @ v) @ p[pre + 'Wo'] + p[pre + 'bo'], pre), pre)


@pytest.mark.parametrize('causal', [False, True], ids=['pad', 'future'])
def test_masked_max_case_has_teeth(causal):
    """a reverse pass without the max-shift term misses the true gradient of this case by at least 100 bars in some tensor
    (measured: about 1.0 in ds.Wk under PAD, 0.38 under the causal mask), and the key biases' gradients are nothing"""
    V, d, h, flat, enc, dec, out = mdp_ref.masked_max_case(causal)
    assert (enc == 0).any() and (dec == 0).any()
    bar = mdp_ref.MASKED_MAX_BARS[causal]['grad']
    loss, want = mdp_ref.RefSeq2Seq(V, d, h, flat).loss_and_grad(enc, dec, out)
    loss_d, got = _DetachedMax(V, d, h, flat).loss_and_grad(enc, dec, out)
    assert loss_d == loss and np.isfinite(want).all()                               # the same forward
    err = mdp_ref.grad_errors(got, want, V, d, h)
    print('without the max shift: worst %s %.3g (bar %.3g), %d tensors above the bar' % (max(err, key=err.get), max(err.values()), bar,
                                                                                        sum(v > bar for v in err.values())))
    assert max(err.values()) >= 100 * bar
    o, top = _offsets(V, d, h), np.abs(want).max()
    for k in ('ea.bk', 'ds.bk', 'dc.bk'):
        assert np.abs(want[o[k]:o[k] + d]).max() < 1e-9 * top, k
    if not causal:                                                                  # the construction as specified
        E = flat[:V * d].reshape(V, d)
        assert E[0, d - 1] == 25 and (E[1:, d - 1] == 3).all() and (enc[:, 1::3] == 0).all() and (dec[:, 2::3] == 0).all()
        assert enc.shape == (5, 18) and dec.shape == (5, 7)
        assert np.array_equal(flat[o['ds.Wk']:o['ds.Wk'] + d * d].reshape(d, d), np.eye(d))
    else:
        assert (dec[:, -2] == 9).all() and not (dec[:, :-2] == 9).any() and not (enc == 9).any()


def test_masked_rows_case_in_the_restatement():
    V, d, h, flat, enc, dec, out, lost = mdp_ref.masked_rows_case()
    assert (enc[3] == 0).all() and dec[4, 0] == 1 and (dec[4, 1:] == 0).all() and lost
    assert not np.isin(enc, lost).any()
    _, g = mdp_ref.RefSeq2Seq(V, d, h, flat).loss_and_grad(enc, dec, out)
    assert np.isfinite(g).all()
    E = g[:V * d].reshape(V, d)
    assert not E[lost].any() and E[0].any()              # a token no source holds has no gradient; PAD's own row has one
    # a batch whose decoder inputs are all PAD has no position to average over: 0 / 0 in the restatement, where the library
    # promises loss 0 and a zero gradient (it divides by max(count, 1))
    with np.errstate(all='ignore'):
        loss, _ = mdp_ref.RefSeq2Seq(V, d, h, flat).loss_and_grad(enc, np.zeros_like(dec), out)
    assert np.isnan(loss)


@pytest.fixture(scope='module')
def shape_beam_refs():
    out = []
    for i in range(len(mdp_ref.BEAM_CASES)):
        c = mdp_ref.beam_case(i)
        c['margin'] = mdp_ref.beam_search_ref(mdp_ref.RefSeq2Seq(c['V'], c['d'], c['h'], c['flat']), c['enc'], c['K'], c['T'], c['C'])[3]
        out.append(c)
    return out


def test_beam_cases_leave_three_quarters_of_their_users_clear(shape_beam_refs):
    """at 4 x the float32 restatement's own error at least 75 % of a case's users keep every selection margin: the GPU test's
    `clear.mean() >= 0.5` is then a condition with room, not a measurement"""
    for i, c in enumerate(shape_beam_refs):
        share = (c['margin'] > mdp_ref.BEAM_BARS[i]).mean()
        print(mdp_ref.BEAM_CASES[i], 'clear share %.3f' % share)
        assert share >= 0.75, i


def test_beam_cases_sit_on_the_edges_their_comments_name():
    cases = {c[:6] for c in mdp_ref.BEAM_CASES}
    assert {(4, 6, 70, 64, 3, None), (4, 6, 70, 65, 3, None), (4, 6, 37, 4, 63, None), (24, 6, 292, 100, 3, None)} <= cases
    assert sorted(mdp_ref.BEAM_BARS) == list(range(len(mdp_ref.BEAM_CASES)))
    widest = [c for c in mdp_ref.BEAM_CASES if c[3] == 128]
    assert widest and all(c[0] >= 4 and c[2] == 129 and c[4] <= 3 for c in widest)
    assert any(c[5] is not None and c[3] in (65, 100) and c[3] <= c[5] <= c[3] + 4 for c in mdp_ref.BEAM_CASES)
    assert all(c[4] + 1 <= 64 and c[3] < c[2] for c in mdp_ref.BEAM_CASES)
    d = 64
    rows = {c[0]: c[0] * c[3] for c in mdp_ref.BEAM_CASES if c[2] == 292}
    assert rows == {24: 2400, 25: 2500}
    assert _gemm_form(2400, 292, d, d, 292) == 'small' and _gemm_form(2500, 292, d, d, 292) == 't128'
