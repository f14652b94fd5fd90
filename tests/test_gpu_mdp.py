"""GPU: the MDP checker's seq2seq transformer (rl4rs_seq2seq_forward) against the float64 restatement tests/mdp_ref.py, and its beam
search (rl4rs_seq2seq_beam) against what the reference's own beam_search returned for that restatement (tests/golden/mdp_beam_*.npz).

Every bar is 4 x the float32 error of the restatement itself at these inputs (mdp_ref.FWD_ABS_BAR / FWD_REL_BAR / BEAM_REL_BAR,
measured on a CPU by `python tests/mdp_ref.py`), never a figure of the kernels under test."""
import numpy as np
import pytest

import mdp_ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _model(V, d, h, flat, **kw):
    from rl4rs_amd.mdpchecker import Seq2SeqTransformer
    m = Seq2SeqTransformer(token_num=V, embed_dim=d, hidden_dim=h, **kw)
    m.set_weights(flat)
    return m


# ---------------------------------------------------------------- forward
@pytest.fixture(scope='module')
def forward_refs():
    out = []
    for i in range(len(mdp_ref.FORWARD_CASES)):
        V, d, h, flat, enc, dec = mdp_ref.forward_case(i)
        out.append(mdp_ref.RefSeq2Seq(V, d, h, flat).predict([enc, dec]))
    return out


def _check_probs(got, want, d):
    assert got.dtype == np.float32 and got.shape == want.shape
    err = np.abs(got - want)
    big = want > 1e-6
    rel = (err[big] / want[big]).max()
    print('abs %.3g (bar %.3g)  rel %.3g (bar %.3g)' % (err.max(), mdp_ref.FWD_ABS_BAR[d], rel, mdp_ref.FWD_REL_BAR[d]))
    assert err.max() <= mdp_ref.FWD_ABS_BAR[d]
    assert rel <= mdp_ref.FWD_REL_BAR[d]


@pytest.mark.parametrize('i', range(len(mdp_ref.FORWARD_CASES)))
def test_predict_matches_the_restatement(i, forward_refs):
    V, d, h, flat, enc, dec = mdp_ref.forward_case(i)
    assert (enc == 0).any() and (dec == 0).any()                 # PAD keys on both sides
    _check_probs(_model(V, d, h, flat).predict([enc, dec]), forward_refs[i], d)


def test_predict_of_one_position(forward_refs):
    """L = 1 (the first decode step) is the first position of the longer call: the decoder is causal"""
    V, d, h, flat, enc, dec = mdp_ref.forward_case(0)
    _check_probs(_model(V, d, h, flat).predict([enc, dec[:, :1]]), forward_refs[0][:, :1], d)


def test_predict_in_chunks_is_bitwise_the_same():
    V, d, h, flat, enc, dec = mdp_ref.forward_case(2)
    whole = _model(V, d, h, flat).predict([enc, dec])
    parts = _model(V, d, h, flat, max_rows=7 * 18).predict([enc, dec])       # 7 users per call: 7 calls
    assert np.array_equal(whole, parts)


# ---------------------------------------------------------------- beam search
@pytest.fixture(scope='module')
def beam_refs():
    """per golden case: the restatement's own search (margins, step probabilities), computed once"""
    out = {}
    for name in mdp_ref.GOLDEN_CASES:
        c = mdp_ref.load_case(GOLDEN, name)
        ref = mdp_ref.RefSeq2Seq(c['V'], c['d'], c['h'], c['flat'])
        c['ref'] = ref
        c['ref_paths'], c['ref_scores'], c['ref_sp'], c['margin'] = mdp_ref.beam_search_ref(ref, c['enc'], c['K'], c['T'], c['C'])
        out[name] = c
    return out


def _device_beam(c, **kw):
    from rl4rs_amd.mdpchecker import beam_search_steps
    m = _model(c['V'], c['d'], c['h'], c['flat'], **kw)
    return beam_search_steps(m, c['enc'], c['K'], c['T'], use_candidates=c['C'] is not None, candidates_size=c['C'])


def _path_products(c, paths):
    """the restatement's teacher-forced probability product along every path (candidate masks do not enter: a kept token is inside)"""
    N, K, T1 = paths.shape
    pr = c['ref'].predict([np.repeat(c['enc'], K, axis=0), paths.reshape(N * K, T1)[:, :-1]])
    step = np.take_along_axis(pr, paths.reshape(N * K, T1)[:, 1:, None], axis=2)[:, :, 0]
    return step.reshape(N, K, T1 - 1)


@pytest.mark.parametrize('name', mdp_ref.GOLDEN_CASES)
def test_beam_search_matches_the_reference(name, beam_refs):
    c = beam_refs[name]
    bar = mdp_ref.BEAM_REL_BAR[c['d']]
    paths, scores, sp = _device_beam(c)
    N, K, T = c['N'], c['K'], c['T']
    assert paths.dtype == np.int64 and paths.shape == (N, K, T + 1) and scores.dtype == np.float64 and scores.shape == (N, K)
    assert sp.dtype == np.float32 and sp.shape == (N, K, T)
    # 1. scores, best first, against the reference's
    assert (np.diff(scores, axis=1) <= 0).all()
    rel = np.abs(scores - c['scores']) / c['scores']
    print('%s: score rel err %.3g (bar %.3g)' % (name, rel.max(), bar))
    assert rel.max() <= bar
    # 2. every returned path has the score the restatement gives that path
    want_sp = _path_products(c, paths)
    rel = np.abs(scores - want_sp.prod(axis=2)) / want_sp.prod(axis=2)
    print('%s: path / score rel err %.3g' % (name, rel.max()))
    assert rel.max() <= bar
    # 3. distinct paths that begin with <START>
    assert (paths[:, :, 0] == 1).all() and paths.min() >= 0 and paths.max() < c['V']
    for n in range(N):
        assert len({tuple(p) for p in paths[n]}) == K
    # 4. exact paths, order included, wherever float64 separates every selection by more than the bar
    clear = c['margin'] > bar
    print('%s: %d of %d users have every selection margin above the bar' % (name, clear.sum(), N))
    assert clear.mean() >= 0.5
    assert np.array_equal(paths[clear], c['paths'][clear])
    # 5. the step probabilities multiply to the score (float32 factors, float64 product: a few float32 roundings)
    prod = sp.astype(np.float64).prod(axis=2)
    assert np.array_equal(prod, scores) or (np.abs(prod - scores) / scores).max() <= 1e-12
    assert (np.abs(sp - want_sp) / want_sp).max() <= bar


@pytest.mark.parametrize('V,K,Cn', [(600, 5, None), (513, 7, 12), (512, 7, None)])
def test_beam_search_on_either_side_of_the_wide_vocabulary_threshold(V, K, Cn):
    """up to 512 tokens a row's best `beam` are picked by one wave from registers, beyond that by a workgroup from memory: both
    against the restatement's search (itself pinned to the reference by the golden files), with candidates across the threshold"""
    N, S, T, d, h = 3, 6, 3, 64, 48
    flat = mdp_ref.random_params(V, d, h, 77)
    enc = np.random.RandomState(78).randint(3, V, size=(N, S)).astype(np.int32)
    enc[:, 0], enc[:, -1] = mdp_ref.START, mdp_ref.END
    ref = mdp_ref.RefSeq2Seq(V, d, h, flat)
    want_paths, want_scores, want_sp, margin = mdp_ref.beam_search_ref(ref, enc, K, T, Cn)
    c = dict(V=V, d=d, h=h, flat=flat, enc=enc, K=K, T=T, C=Cn)
    paths, scores, sp = _device_beam(c)
    bar = mdp_ref.BEAM_REL_BAR[d]
    rel = np.abs(scores - want_scores) / want_scores
    print('V %d: score rel err %.3g (bar %.3g), margins %s' % (V, rel.max(), bar, margin))
    assert rel.max() <= bar
    clear = margin > bar
    assert clear.mean() >= 0.5 and np.array_equal(paths[clear], want_paths[clear])
    assert (np.abs(sp - want_sp) / want_sp).max() <= bar


@pytest.mark.parametrize('V', [37, 600])
def test_equal_scores_go_to_the_smaller_beam_and_token(V):
    """tokens 5 and 9 share their decoder row and their output bias, which towers over the rest: every probability of 9 is that of
    5 bit for bit, as is everything that follows a 9 and a 5.  Of the four equal continuations of step 1 the two of beam 0 are kept,
    token 5 first (the per-wave and the per-workgroup selection)."""
    d, h = 64, 48
    m = _model(V, d, h, mdp_ref.random_params(V, d, h, 5))
    w = m.get_weights()
    w['decoder_embedding'][9] = w['decoder_embedding'][5]
    w['output_bias'][[5, 9]] = 25.0
    m.set_weights(w)
    enc = np.array([[1, 7, 8, 2], [1, 9, 5, 2], [1, 3, 0, 0]], dtype=np.int32)
    paths, scores, sp = m.beam(enc, 2, 2, None, True)
    assert np.array_equal(paths, np.tile(np.array([[1, 5, 5], [1, 5, 9]]), (3, 1, 1)))
    assert np.array_equal(scores[:, 0], scores[:, 1]) and np.array_equal(sp[:, 0], sp[:, 1]) and (scores > 0.2).all()
    paths, scores, _ = m.beam(enc, 1, 2, None, False)
    assert np.array_equal(paths, np.tile(np.array([[1, 5, 5]]), (3, 1, 1)))


def test_all_candidates_is_the_unmasked_search(beam_refs):
    c = beam_refs['n3_v50_k6_c9']
    m = _model(c['V'], c['d'], c['h'], c['flat'])
    plain = m.beam(c['enc'], c['K'], c['T'], None, True)
    every = np.tile(np.arange(c['V']), (c['N'], 1))
    masked = m.beam(c['enc'], c['K'], c['T'], every, True)
    for a, b in zip(plain, masked):
        assert np.array_equal(a, b)


def test_chunked_decoding_is_bitwise_the_same(beam_refs):
    c = beam_refs['n70_v37_k8']
    whole = _device_beam(c)
    parts = _device_beam(c, max_rows=9 * 8)                      # 9 users per call: 8 calls, the last one of 7 users
    for a, b in zip(whole, parts):
        assert np.array_equal(a, b)


def test_beam_limits_are_error_codes(beam_refs):
    from rl4rs_amd import _lib
    from rl4rs_amd.mdpchecker import beam_search
    c = beam_refs['n3_v37_k4']
    m = _model(c['V'], c['d'], c['h'], c['flat'])
    for beam in (c['V'], c['V'] + 5, 129, 0):
        with pytest.raises(_lib.Rl4rsHipError):
            beam_search(m, c['enc'], beam, c['T'])
    big = _model(300, 64, 48, mdp_ref.random_params(300, 64, 48, 1))
    with pytest.raises(_lib.Rl4rsHipError, match='128'):
        beam_search(big, c['enc'], 129, c['T'])
    with pytest.raises(ValueError, match='candidates_size'):
        beam_search(m, c['enc'], 6, c['T'], use_candidates=True, candidates_size=5)
    # ... and the library itself counts the bits it is given: 5 candidates for user 1, 6 for the others, beam 6
    few = np.tile(np.arange(3, 9), (c['N'], 1))
    few[1, 5] = few[1, 4]
    with pytest.raises(_lib.Rl4rsHipError, match='candidates_size'):
        m.beam(c['enc'], 6, c['T'], few)
    with pytest.raises(_lib.Rl4rsHipError, match='candidates_size'):      # bits at or above V do not count
        m._net.beam(c['enc'], 2, c['T'], np.array([[0, 1 << (c['V'] - 32) | 1 << 31]] * c['N'], dtype=np.uint32))
    assert m.beam(c['enc'], 6, c['T'], np.tile(np.arange(3, 9), (c['N'], 1)))[0].shape == (c['N'], 6, c['T'] + 1)
    paths, scores = beam_search(m, c['enc'], 4, c['T'])          # the handle still works after the refusals
    assert np.array_equal(paths, _device_beam(c)[0])


def test_decoder_module_keeps_the_reference_conventions(beam_refs):
    from rl4rs.mdpchecker import decoder
    c = beam_refs['n3_v37_k4']
    m = _model(c['V'], c['d'], c['h'], c['flat'])
    out, score = decoder.beam_search(m, c['enc'], c['K'], c['T'])
    assert out.dtype == np.int64 and out.shape == (c['N'], c['K'], c['T'] + 1) and score.dtype == np.float64
    step = decoder.decode_step(m, c['enc'], out[:, 0, :1], beam_size=c['K'])
    assert step.shape == (c['N'], c['K'], 2)
    first = c['ref'].predict([c['enc'], out[:, 0, :1]])[:, -1]
    assert np.array_equal(step[:, :, 1].astype(np.int64), np.argsort(-first, axis=1, kind='stable')[:, :c['K']])
    assert (np.diff(step[:, :, 0], axis=1) <= 0).all()
    tp = decoder.token_probs(m, c['enc'], out[:, 0, :2])
    assert tp.shape == (c['N'], c['V']) and np.allclose(tp.sum(axis=1), 1.0, atol=1e-5)
    with pytest.raises(TypeError):
        decoder.beam_search(c['ref'], c['enc'], c['K'], c['T'])


def _rel_gap(x):
    """smallest relative gap between two distinct values of x (inf when all are equal)"""
    u = np.unique(x)
    return np.inf if len(u) < 2 else float((np.diff(u) / u[1:]).min())


def test_experiments_from_device_beams():
    """Experiment II from device beams against the reference's beams: each ratio is a mean of quotients of means of scores, every
    score within the beam bar, so the ratios agree within twice the bar.  Experiment I reads the beam search's step probabilities."""
    from rl4rs_amd import mdpchecker as M
    z = np.load(GOLDEN + '/mdp_experiments.npz')
    N, V, B, hot, Cn, S, T, d, h, seed = (int(v) for v in z['cfg'])
    m = _model(V, d, h, mdp_ref.random_params(V, d, h, seed))
    enc = z['encode_input']
    _, g = M.beam_search(m, enc, 1, T)
    _, b, sp = M.beam_search_steps(m, enc, B, T)
    _, hs = M.beam_search(m, enc, hot, T, use_candidates=True, candidates_size=Cn)
    two = np.array(M.experiment_II(B, g, b, hs))
    bar = 2 * mdp_ref.BEAM_REL_BAR[d]
    print('experiment II', two, z['experiment_II'])
    assert (np.abs(two - z['experiment_II']) / z['experiment_II']).max() <= bar
    one = M.experiment_I(sp)
    assert one.shape == (T, 2) and np.allclose(one[-1], 1.0)
    # Pearson column against the recorded one, on the users whose beams are the reference's.  r = <x', y'> of the centred, normalised
    # prefix and sequence scores; a relative error e in every element of x moves x' by at most 2 e |x| / |x - mean x| (the same for y),
    # so |dr| <= 2 e (|x| / |x - mean| + |y| / |y - mean|), e = the beam bar; evaluated on the recorded probabilities
    paths, _, _ = M.beam_search_steps(m, enc, B, T)
    same = (paths == z['output_topk']).all(axis=(1, 2))
    assert same.mean() >= 0.5
    e = mdp_ref.BEAM_REL_BAR[d]
    cond = lambda x: np.linalg.norm(x) / np.linalg.norm(x - x.mean())
    ranked = 0
    for n in np.flatnonzero(same):
        want_p = z['token_probs'][n]
        seq = want_p.prod(axis=1)
        for i in range(T - 1):
            pre = want_p[:, :i + 1].prod(axis=1)
            if np.ptp(pre) == 0:
                continue
            got_pre, got_seq = sp[n][:, :i + 1].astype(np.float64).prod(axis=1), sp[n].astype(np.float64).prod(axis=1)
            assert abs(np.corrcoef(got_pre, got_seq)[0][1] - np.corrcoef(pre, seq)[0][1]) <= 2 * e * (cond(pre) + cond(seq)), (n, i)
            # Spearman: where no two distinct recorded scores lie within twice the bar of each other, errors within the bar cannot
            # swap a pair, and equal recorded scores (beams that share the prefix) are equal on the device too, their factors being
            # copies: the ranks are the recorded ones and so is the coefficient
            if min(_rel_gap(pre), _rel_gap(seq)) > 2 * e:
                ranked += 1
                assert abs(M.spearman(got_pre, got_seq) - M.spearman(pre, seq)) <= 1e-12, (n, i)
    print('spearman compared for %d (user, prefix) pairs' % ranked)
    assert ranked > 0
    if same.all():
        assert np.abs(one[:, 0] - z['experiment_I'][:, 0]).max() <= 2 * e * max(
            cond(z['token_probs'][n][:, :i + 1].prod(axis=1)) + cond(z['token_probs'][n].prod(axis=1))
            for n in range(N) for i in range(T) if np.ptp(z['token_probs'][n][:, :i + 1].prod(axis=1)) > 0)
