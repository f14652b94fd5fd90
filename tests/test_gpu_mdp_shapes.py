"""GPU: the MDP checker's seq2seq transformer and its beam search (csrc/seq2seq.hip, seq2seq_train.hpp) away from the shapes of
tests/test_gpu_mdp.py and tests/test_gpu_mdp_train.py (d 64 / 256, hidden 48 / 128, S <= 18, L <= 7 < S, at most 810 rows, beams 1 .. 8,
20, 100), against the float64 restatement tests/mdp_ref.py and its beam search (pinned to the reference's by the golden files).

The cases, the path of the code each one enters and its bars stand in tests/mdp_ref.py (SHAPE_CASES, masked_rows_case,
masked_max_case, BEAM_CASES); tests/test_mdp_host.py checks on a CPU that the cases are where their comments say - the tier
arithmetic of launch_gemm_f32 included, which puts the LDS-tiled k_gemm_f32_t128 behind 96 workgroups of 128 x 64 and so behind 6017
rows at d = 128 (SHAPE_CASES 9 and 10, BEAM_CASES 6), not behind 2048 - and that the masked-max cases have teeth.

Bars: 4 x the float32 error of the restatement against itself in float64 at the very inputs of a case (`python tests/mdp_ref.py
shapes` on a CPU), a measured figure counting as at least float32's unit roundoff 2^-24.  Never a figure of the kernels.  Every test
prints what it measured beside its bar.

Both masked-max variants are in: the host check gives the causal one (a towering FUTURE key) teeth as well (a reverse pass
without the max-shift term misses ds.Wk by 0.38 of its size, the bar is 2.4e-5).

Measured on an MI355X, device error / bar (p: probabilities absolute, relative; l: loss relative; g: worst gradient tensor by
mdp_ref.grad_errors, the worst dropout setting):
  (3, 64, 64, 37, 64, 48)      64 keys, causal at 64 queries               p 3.8e-7 / 2.9e-6, 2.9e-6 / 1.7e-5  l 8.4e-8 / 3.4e-7  g 7.6e-7 / 1.2e-5
  (4, 3, 9, 37, 64, 48)        L > S                                       p 4.0e-7 / 2.0e-6, 2.4e-6 / 1.3e-5  l 1.3e-7 / 2.4e-7  g 1.7e-6 / 1.8e-5
  (5, 1, 1, 37, 64, 48)        one key, one query                          p 2.1e-7 / 2.3e-6, 1.4e-6 / 1.0e-5  l 3.2e-8 / 2.4e-7  g 5.0e-7 / 4.8e-6
  (5, 7, 5, 41, 66, 7)         d % 4 == 2, odd hidden, nothing aligned     p 2.5e-7 / 1.8e-6, 2.5e-6 / 1.8e-5  l 3.3e-8 / 4.0e-7  g 1.3e-6 / 1.2e-5
  (5, 7, 5, 41, 100, 33)       d % 64 != 0, dropout 0.5                    p 5.0e-7 / 2.7e-6, 2.8e-6 / 1.8e-5  l 1.5e-7 / 2.4e-7  g 3.1e-6 / 1.8e-5
  (5, 7, 5, 41, 6, 1)          narrowest widths                            p 2.3e-8 / 2.4e-7, 4.8e-7 / 1.5e-6  l 6.4e-8 / 2.4e-7  g 2.4e-5 / 3.6e-5
  (36, 64, 8, 292, 128, 100)   2304 rows, 9 partials, k_gemm_small         p 8.2e-7 / 7.2e-6, 5.8e-6 / 3.4e-5  l 5.0e-8 / 2.4e-7  g 6.8e-7 / 4.4e-6
  (36, 64, 8, 292, 128, 102)   the same, weights off alignment             p 9.5e-7 / 8.0e-6, 4.5e-6 / 4.8e-5  l 5.2e-8 / 2.4e-7  g 8.4e-7 / 6.4e-6
  (70, 64, 33, 292, 128, 100)  4480 rows, chunk 280, 16 partials           p 7.7e-7 / 6.8e-6, 5.3e-6 / 4.4e-5  l 4.0e-8 / 2.7e-7  g 9.7e-7 / 3.7e-6
  (95, 64, 26, 292, 128, 100)  6080 / 2470 rows, k_gemm_f32_t128           p 1.8e-6 / 9.2e-6, 1.1e-5 / 4.8e-5  l 8.9e-8 / 3.5e-7  g 5.8e-7 / 2.2e-6
  (95, 64, 26, 292, 128, 102)  the same, k_gemm_f32 behind ef.W1           p 2.8e-6 / 8.4e-6, 1.2e-5 / 4.4e-5  l 8.2e-8 / 4.4e-7  g 4.7e-7 / 2.5e-6
  all-PAD source / decoder row                                             p 3.0e-7 / 1.8e-6, 2.0e-6 / 1.6e-5  l 8.7e-8 / 2.4e-7  g 6.3e-7 / 7.6e-6
  whole batch PAD                                                          loss 0.0 and gradient 0.0, exactly
  masked max, PAD / future key                                             l 3.9e-8, 1.5e-8 / 2.4e-7  g 3.8e-6 / 8.8e-6, 2.1e-6 / 2.4e-5
  beams 64, 65, 65 + candidates 68 (V 70)                                  scores 2.2e-6 / 1.6e-5, step probabilities 1.8e-6; 3 of 4 users clear
  beam 128, V 129                                                          2.8e-6 / 1.6e-5, 1.8e-6; 7 of 8 clear
  target_len 63                                                            2.7e-6 / 1.5e-5, 1.1e-6; 4 of 4 clear
  2400 rows (k_gemm_small) / 2500 rows, candidates 104 (k_gemm_f32_t128)   2.9e-6, 4.4e-6 / 1.9e-5, 2.1e-6, 4.0e-6; 20 of 24, 21 of 25 clear
One case failed first: (5, 1, 1, 37, 64, 48) had 1.1e-5 in dc.Wq (5.5e-6 .. 6.3e-6 in ea.Wq, ea.Wk, dc.Wk) against 4.8e-6.  With one
key the scores cannot matter and those gradients are 0; k_s2s_attn_bwd_q formed the max-shift term as (1 - sum a) * dot, which left
the difference of two roundings there.  It now takes the term as the wave sum of the first terms (seq2seq_train.hpp);
the masked-max figure fell from 8.5e-6 to 3.8e-6 with it."""
import functools

import numpy as np
import pytest

import mdp_ref

pytestmark = pytest.mark.gpu


def _net(V, d, h, flat, S, L, N):
    from rl4rs_amd.device import DeviceSeq2Seq
    return DeviceSeq2Seq(V, d, h, S, L, N * max(S, L), flat)


def _model(V, d, h, flat, **kw):
    from rl4rs_amd.mdpchecker import Seq2SeqTransformer
    m = Seq2SeqTransformer(token_num=V, embed_dim=d, hidden_dim=h, **kw)
    m.set_weights(flat)
    return m


def _check_probs(got, want, bars):
    assert got.dtype == np.float32 and got.shape == want.shape
    err, rel = mdp_ref.probs_errors(got, want)
    print('abs %.3g (bar %.3g)  rel %.3g (bar %.3g)' % (err, bars['abs'], rel, bars['rel']))
    assert err <= bars['abs']
    assert rel <= bars['rel']


def _check_training(net, enc, dec, out, drop, want_loss, want, V, d, h, bars):
    """one loss_grad call against (want_loss, want); -> the device gradient (float64)"""
    rate, seed, step = drop or (0.0, 0, 0)
    net.grad().fill_(123.0)                                       # a tensor the pass did not write would show
    loss = float(net.loss_grad(enc, dec, out, rate, seed, step).cpu())
    got = net.grad().cpu().numpy().astype(np.float64)
    err = mdp_ref.grad_errors(got, want, V, d, h)
    worst = max(err, key=err.get)
    rel = abs(loss - want_loss) / want_loss
    print('dropout %s: loss %.8g want %.8g rel %.3g (bar %.3g); worst tensor %s %.3g (bar %.3g)'
          % (drop and drop[0], loss, want_loss, rel, bars['loss'], worst, err[worst], bars['grad']))
    bad = {k: v for k, v in err.items() if not v <= bars['grad']}
    assert not bad, bad
    assert rel <= bars['loss']
    return got


# ---------------------------------------------------------------- A: the shape table
@functools.lru_cache(maxsize=None)
def _shape_probs(i):
    V, d, h, flat, enc, dec = mdp_ref.shape_case(i)
    return mdp_ref.RefSeq2Seq(V, d, h, flat).predict([enc, dec])


SHAPE_IDS = ['n%d_s%d_l%d_v%d_d%d_h%d' % c for c in mdp_ref.SHAPE_CASES]


@pytest.mark.parametrize('i', range(len(mdp_ref.SHAPE_CASES)), ids=SHAPE_IDS)
def test_predict_matches_the_restatement(i):
    V, d, h, flat, enc, dec = mdp_ref.shape_case(i)
    assert (enc == 0).any() and (dec == 0).any()                 # PAD keys on both sides
    _check_probs(_model(V, d, h, flat).predict([enc, dec]), _shape_probs(i), mdp_ref.SHAPE_BARS[i])


@pytest.mark.parametrize('i', range(len(mdp_ref.SHAPE_CASES)), ids=SHAPE_IDS)
def test_loss_and_every_gradient_against_autograd(i):
    """dropout 0, (0.05, 7, 3) and, where the case carries it, 0.5, on one handle"""
    N, S, L, V, d, h = mdp_ref.SHAPE_CASES[i]
    _, _, _, flat, enc, dec = mdp_ref.shape_case(i)
    out = mdp_ref.shape_targets(i)
    net = _net(V, d, h, flat, S, L, N)
    drops = mdp_ref.shape_drops(i)
    assert drops[:2] == [None, (0.05, 7, 3)] and (i != 4 or drops[2][0] == 0.5)
    for drop in drops:
        want_loss, want = mdp_ref.RefSeq2Seq(V, d, h, flat).loss_and_grad(enc, dec, out, drop)
        _check_training(net, enc, dec, out, drop, want_loss, want, V, d, h, mdp_ref.SHAPE_BARS[i])


# ---------------------------------------------------------------- B: masked and degenerate attention rows
def test_all_pad_source_and_all_pad_decoder_row():
    """user 3 has nothing to attend to (a = 0 for every key, a zero attention output in the encoder and in cross-attention), user 4's
    decoder attends to <START> alone and is weighed at <START> alone"""
    V, d, h, flat, enc, dec, out, lost = mdp_ref.masked_rows_case()
    N, S, L = enc.shape[0], enc.shape[1], dec.shape[1]
    bars = mdp_ref.MASKED_ROWS_BARS
    ref = mdp_ref.RefSeq2Seq(V, d, h, flat)
    _check_probs(_model(V, d, h, flat).predict([enc, dec]), ref.predict([enc, dec]), bars)
    net = _net(V, d, h, flat, S, L, N)
    for drop in (None, mdp_ref.SHAPE_DROP):
        want_loss, want = ref.loss_and_grad(enc, dec, out, drop)
        got = _check_training(net, enc, dec, out, drop, want_loss, want, V, d, h, bars)
        # the tokens only user 3's source held are gone from the batch: no gradient for their rows of the encoder table, exactly,
        # as in the restatement; PAD's own row has one (PAD positions are queries like any other) and is held to the bar above
        for v in lost:
            assert not got[v * d:(v + 1) * d].any() and not want[v * d:(v + 1) * d].any(), v
        assert want[:d].any() and got[:d].any()


@pytest.mark.parametrize('drop', [None, mdp_ref.SHAPE_DROP], ids=['dropout0', 'dropout0.05'])
def test_a_batch_of_pad_decoder_inputs_has_loss_zero_and_a_zero_gradient(drop):
    """no position to average over: the restatement divides 0 by 0, the library divides by max(count, 1) and promises zeros"""
    N, S, L, V, d, h = mdp_ref.FORWARD_CASES[0]
    _, _, _, flat, enc, dec = mdp_ref.forward_case(0)
    net = _net(V, d, h, flat, S, L, N)
    net.grad().fill_(123.0)
    rate, seed, step = drop or (0.0, 0, 0)
    loss = net.loss_grad(enc, np.zeros_like(dec), mdp_ref.train_targets(0), rate, seed, step).cpu().numpy()
    g = net.grad().cpu().numpy()
    print('loss %r, largest |gradient| %r' % (float(loss[0]), float(np.abs(g).max())))
    assert loss[0] == 0.0 and not g.any()


@pytest.mark.parametrize('causal', [False, True], ids=['pad', 'future'])
def test_max_shift_term_when_a_masked_key_towers(causal):
    """mdp_ref.masked_max_case: the largest raw score of most rows belongs to a masked key and the open keys' e sum to within a few
    orders of magnitude of the normaliser's 1e-7, so dL/ds carries - [k = arg-max] (1 - sum a) dot at full weight.  A reverse pass
    without the term, or with the arg-max taken over the open keys only, misses by about 1.0 (PAD) / 0.38 (future key) in ds.Wk
    (tests/test_mdp_host.py).  The key biases' gradients, which the library writes as exact zeros, are below 1e-18 in float64."""
    V, d, h, flat, enc, dec, out = mdp_ref.masked_max_case(causal)
    N, S, L = enc.shape[0], enc.shape[1], dec.shape[1]
    want_loss, want = mdp_ref.RefSeq2Seq(V, d, h, flat).loss_and_grad(enc, dec, out)
    got = _check_training(_net(V, d, h, flat, S, L, N), enc, dec, out, None, want_loss, want, V, d, h, mdp_ref.MASKED_MAX_BARS[causal])
    o = 0
    for name, shape in mdp_ref.layout(V, d, h):
        n = int(np.prod(shape))
        if name.endswith('.bk'):
            assert not got[o:o + n].any(), name
        o += n


# ---------------------------------------------------------------- C: beam-search edges
@functools.lru_cache(maxsize=None)
def _beam_ref(i):
    c = mdp_ref.beam_case(i)
    c['ref'] = mdp_ref.RefSeq2Seq(c['V'], c['d'], c['h'], c['flat'])
    c['paths'], c['scores'], c['sp'], c['margin'] = mdp_ref.beam_search_ref(c['ref'], c['enc'], c['K'], c['T'], c['C'])
    return c


def _device_beam(c, enc=None, **kw):
    from rl4rs_amd.mdpchecker import beam_search_steps
    m = _model(c['V'], c['d'], c['h'], c['flat'], **kw)
    return beam_search_steps(m, c['enc'] if enc is None else enc, c['K'], c['T'], use_candidates=c['C'] is not None, candidates_size=c['C'])


def _path_products(c, paths):
    """the restatement's teacher-forced probability of every token along every path (a kept token is inside the candidate set, so
    the masks do not enter)"""
    N, K, T1 = paths.shape
    flat = paths.reshape(N * K, T1)
    pr = c['ref'].predict([np.repeat(c['enc'], K, axis=0), flat[:, :-1]])
    return np.take_along_axis(pr, flat[:, 1:, None], axis=2)[:, :, 0].reshape(N, K, T1 - 1)


BEAM_IDS = ['n%d_s%d_v%d_k%d_t%d_c%s_seed%d' % c for c in mdp_ref.BEAM_CASES]


@pytest.mark.parametrize('i', range(len(mdp_ref.BEAM_CASES)), ids=BEAM_IDS)
def test_beam_search_edges_against_the_restatement(i):
    c = _beam_ref(i)
    bar = mdp_ref.BEAM_BARS[i]
    N, K, T = c['N'], c['K'], c['T']
    paths, scores, sp = _device_beam(c)                           # step probabilities requested
    assert paths.shape == (N, K, T + 1) and scores.shape == (N, K) and sp.dtype == np.float32 and sp.shape == (N, K, T)
    # scores, best first, within the bar of the float64 search's
    assert (np.diff(scores, axis=1) <= 0).all() and (scores > 0).all()
    rel = np.abs(scores - c['scores']) / c['scores']
    clear = c['margin'] > bar
    print('score rel err %.3g (bar %.3g); %d of %d users clear; smallest margins %s' % (rel.max(), bar, clear.sum(), N, np.sort(c['margin'])[:3]))
    assert rel.max() <= bar
    # exact paths, order included, wherever float64 separates every selection by more than the bar
    assert clear.mean() >= 0.5
    assert np.array_equal(paths[clear], c['paths'][clear])
    # distinct paths per user, all from <START>, all inside the vocabulary
    assert (paths[:, :, 0] == 1).all() and paths.min() >= 0 and paths.max() < c['V']
    for n in range(N):
        assert len({tuple(p) for p in paths[n]}) == K, n
    # step probabilities: those of the float64 search where the paths are its own, and the restatement's along every returned path
    want_sp = _path_products(c, paths)
    sp_rel = np.abs(sp - want_sp) / want_sp
    print('step probability rel err %.3g' % sp_rel.max())
    assert sp_rel.max() <= bar
    assert (np.abs(sp[clear] - c['sp'][clear]) / c['sp'][clear]).max() <= bar
    # ... and they multiply to the score (float32 factors, float64 products: a few float64 roundings)
    prod = sp.astype(np.float64).prod(axis=2)
    assert np.array_equal(prod, scores) or (np.abs(prod - scores) / scores).max() <= 1e-12


def test_2400_beam_rows_in_uneven_calls_are_bitwise_the_same():
    c = _beam_ref(5)
    whole = _device_beam(c)
    parts = _device_beam(c, max_rows=7 * c['K'])                  # 7 users per call: 7, 7, 7 and 3
    for a, b in zip(whole, parts):
        assert np.array_equal(a, b)


def test_permuted_and_repeated_users_keep_their_beams_bit_for_bit():
    """a beam row reads the encoder rows of user r / live: users in another order, two of them copies of a third, one with nothing
    but PAD behind <START> - every user's output is what it was, the copies' outputs are their original's"""
    c = _beam_ref(5)
    enc = c['enc'].copy()
    enc[6, 1:] = 0
    enc[2], enc[17] = enc[11], enc[11]
    base = _device_beam(c, enc=enc)
    for a in base:
        assert np.array_equal(a[2], a[11]) and np.array_equal(a[17], a[11]) and not np.array_equal(a[6], a[11])
    assert np.isfinite(base[1]).all() and (base[1][6] > 0).all()
    perm = np.random.RandomState(5).permutation(c['N'])
    assert (perm != np.arange(c['N'])).sum() > c['N'] // 2
    for a, b in zip(base, _device_beam(c, enc=enc[perm])):
        assert np.array_equal(a[perm], b)
