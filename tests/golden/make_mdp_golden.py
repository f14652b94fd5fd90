#!/usr/bin/env python
"""Generate tests/golden/mdp_beam_*.npz and mdp_experiments.npz by running the REFERENCE's own beam_search
(rl4rs/mdpchecker/decoder.py) with tests/mdp_ref.py's float64 model as its ``model``.

    python tests/golden/make_mdp_golden.py /path/to/reference/checkout

The reference module is loaded from its file (nothing of it is copied) under two stubs: ``np.int`` (removed from numpy) and a
``bottleneck`` whose ``partition`` is ``take_along_axis(a, argpartition(a, kth))`` - numpy's own partition / argpartition pair is
not aligned element by element, and the reference indexes one with the other.  The fixtures hold inputs, seeds and results only;
the weights are regenerated from the seed by mdp_ref.random_params.  mdp_experiments.npz also holds the quantities
script/mdpchecker/mdp_checker.py prints for Experiment II and I, computed here from the reference's beams with numpy and
scipy.stats.spearmanr.  Needs the reference checkout and scipy: run it where both exist.
"""
import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mdp_ref  # noqa: E402

# name: N, V, K, candidates, S, T, d, h, seed.  S counts <START> ... <END>; T = target_len
CASES = {
    'n3_v37_k4': dict(N=3, V=37, K=4, C=None, S=18, T=5, d=64, h=48, seed=11),
    'n70_v37_k8': dict(N=70, V=37, K=8, C=None, S=5, T=3, d=64, h=48, seed=12, pad_rows=(4, 33)),
    'n4_v37_k1': dict(N=4, V=37, K=1, C=None, S=18, T=5, d=64, h=48, seed=13),
    'n3_v50_k6_c9': dict(N=3, V=50, K=6, C=9, S=18, T=5, d=64, h=48, seed=14),
    'n2_v290_k100': dict(N=2, V=290, K=100, C=None, S=18, T=5, d=256, h=128, seed=133),
    'n2_v290_k20_c20': dict(N=2, V=290, K=20, C=20, S=18, T=5, d=256, h=128, seed=16),
}
EXPERIMENTS = dict(N=6, V=60, beam=40, hot=20, C=20, S=18, T=5, d=64, h=48, seed=21)


def load_reference_decoder(ref):
    if not hasattr(np, 'int'):
        np.int = int
    bn = types.ModuleType('bottleneck')
    bn.argpartition = lambda a, kth, axis=-1: np.argpartition(a, kth, axis=axis)
    bn.partition = lambda a, kth, axis=-1: np.take_along_axis(a, np.argpartition(a, kth, axis=axis), axis=axis)
    sys.modules['bottleneck'] = bn
    spec = importlib.util.spec_from_file_location('ref_mdp_decoder', os.path.join(ref, 'rl4rs', 'mdpchecker', 'decoder.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def encoder_tokens(c):
    rs = np.random.RandomState(c['seed'] + 1000)
    enc = rs.randint(3, c['V'], size=(c['N'], c['S'])).astype(np.int64)
    enc[:, 0], enc[:, -1] = mdp_ref.START, mdp_ref.END
    for r in c.get('pad_rows', ()):              # a shorter source: <END> one earlier, then <PAD>
        enc[r, -2], enc[r, -1] = mdp_ref.END, mdp_ref.PAD
    return enc


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def main(ref):
    from scipy.stats import spearmanr
    dec = load_reference_decoder(ref)
    for name, c in CASES.items():
        model = mdp_ref.RefSeq2Seq(c['V'], c['d'], c['h'], mdp_ref.random_params(c['V'], c['d'], c['h'], c['seed']))
        enc = encoder_tokens(c)
        topk, score = quiet(dec.beam_search, model, enc, c['K'], c['T'], use_candidates=c['C'] is not None, candidates_size=c['C'])
        _, _, _, margin = mdp_ref.beam_search_ref(model, enc, c['K'], c['T'], c['C'])
        print('%-18s min margin per user: median %.3g, share above 1e-4: %.2f' % (name, np.median(margin), np.mean(margin > 1e-4)))
        np.savez_compressed(os.path.join(HERE, 'mdp_beam_%s.npz' % name), encode_input=enc.astype(np.int32),
                            output_topk=np.asarray(topk, dtype=np.int32), beam_score=np.asarray(score, dtype=np.float64),
                            cfg=np.array([c['N'], c['V'], c['K'], c['C'] or 0, c['S'], c['T'], c['d'], c['h'], c['seed']], dtype=np.int64))
    c = EXPERIMENTS
    model = mdp_ref.RefSeq2Seq(c['V'], c['d'], c['h'], mdp_ref.random_params(c['V'], c['d'], c['h'], c['seed']))
    enc = encoder_tokens(c)
    B, T, N = c['beam'], c['T'], c['N']
    _, g_score = quiet(dec.beam_search, model, enc, 1, T)
    topk, b_score = quiet(dec.beam_search, model, enc, B, T)
    _, h_score = quiet(dec.beam_search, model, enc, c['hot'], T, use_candidates=True, candidates_size=c['C'])
    n5, n20 = int(B * 0.05), int(B * 0.2)
    top5 = np.nanmean(b_score[:, :n5], axis=1)
    ratios = [np.nanmean(np.nanmean(s, axis=1) / top5) for s in (b_score[:, :n20], g_score, h_score[:, :n5], h_score[:, :n20])]
    # Experiment I: the probability of every token of every beam, one teacher-forced prediction per (beam, prefix length)
    probs = np.zeros((N, B, T))
    for j in range(B):
        for i in range(T):
            p = quiet(dec.token_probs, model, enc, topk[:, j, :i + 1])
            probs[:, j, i] = p[np.arange(N), topk[:, j, i + 1]]
    metrics = np.zeros((N, T, 2))
    for n in range(N):
        seq = np.prod(probs[n], axis=1)
        for i in range(T):
            pre = np.prod(probs[n][:, :i + 1], axis=1)
            metrics[n, i] = (np.corrcoef(pre, seq)[0][1], spearmanr(pre, seq)[0])
    metrics = np.nan_to_num(metrics, nan=1.0)
    # Spearman with ties: prefixes shared by several beams give equal prefix scores
    tie_x = np.round(probs[0][:, 0], 3)
    tie_y = np.prod(probs[0], axis=1)
    np.savez_compressed(os.path.join(HERE, 'mdp_experiments.npz'), encode_input=enc.astype(np.int32),
                        cfg=np.array([N, c['V'], B, c['hot'], c['C'], c['S'], T, c['d'], c['h'], c['seed']], dtype=np.int64),
                        greedy_score=g_score, beam_score=b_score, hot_score=h_score, output_topk=np.asarray(topk, dtype=np.int32),
                        token_probs=probs, experiment_II=np.array(ratios), experiment_I=np.nanmean(metrics, axis=0),
                        tie_x=tie_x, tie_y=tie_y, tie_spearman=np.array(spearmanr(tie_x, tie_y)[0]))
    print('experiment II', ratios)
    print('experiment I', np.nanmean(metrics, axis=0))


if __name__ == '__main__':
    main(sys.argv[1])
