"""float64 restatement of rl4rs_exactk_decode_beam (include/rl4rs_hip.h): beam search over Exact-K's pointer decoder, built on
tests/exactk_ref.py by import.

Test infrastructure only.  It is written STATELESSLY: the logits of step t for a set of prefixes are
``exactk_ref.run_decoder(..., path=prefix)[0][:, t]`` (they depend on path[:, :t] alone), with the beams of all rows stacked as
N * L decoder rows over a repeated encoder output, so that a step is one call.  That runs the whole decoder once per step and is
slow, and it shares nothing with an implementation that carries LSTM states, histories and ancestor tables from step to step,
which is the point.

The algorithm (the textbook one; the reference's own BEAMSEARCH decoder is not restated, DESIGN.md section 19 says why): the beams
of a row share the encoder output (dropout pass 1, the masks of ``exactk_ref.decode``); each has its own prefix and hence its own
allowed set; step t scores every allowed candidate a of every live beam b as acc[b] + (logit[b, a] - logsumexp(logit[b, :])); the
best B become the new beams in descending order, equal scores by the smaller flat index b * A + a; one beam is live at step 0.

Score bar.  An accumulated score near 9 ln A = 51 has a float32 spacing of 3.8e-6, the size of the logit bars themselves, so the
bar is measured like the project's other bars: the same restatement in float32 against float64 ALONG THE FLOAT64 SEARCH'S OWN
PREFIXES (``score_yardstick``), the largest absolute error of a selected score over all steps and beams, recorded per case in
MEASURED_SCORE; the bar is exactk_ref.BAR_FACTOR x that.  Measured on the CPU against the restatement, never against the device."""
import numpy as np
import torch

import exactk_ref as R

T = R.T


class Beam(object):
    """Parameters and encoder output of one (inputs, seed, step) in one dtype; every query below is a pure function of it."""

    def __init__(self, flat, obs, dm, loc, special, seed=0, step=0, dtype=torch.float64):
        with torch.no_grad():
            _, self.p = R._params(flat, dm, dtype)
            self.enc = R.encode(self.p, torch.tensor(np.asarray(obs), dtype=dtype), dm, seed, step, 1)
        self.dm, self.loc, self.special, self.dtype, self.N = dm, np.asarray(loc), np.asarray(special), dtype, len(obs)
        self.pad = R.PAD if dtype == torch.float64 else R.PAD32

    def logits(self, prefixes, t):
        """prefixes int [N, L, 9] (entries from t on are ignored) -> torch logits [N, L, A] of step t, the padding value on the
        disallowed entries."""
        prefixes = np.asarray(prefixes)
        N, L = prefixes.shape[:2]
        assert N == self.N
        path = np.zeros((N * L, T), dtype=np.int32)
        path[:, :t] = prefixes.reshape(N * L, T)[:, :t]
        with torch.no_grad():
            enc = self.enc.repeat_interleave(L, dim=0)
            lg = R.run_decoder(self.p, enc, self.dm, self.loc, self.special, path=path)[0][:, t]
        return lg.reshape(N, L, self.dm.A)

    def candidate_scores(self, prefixes, t, acc=None):
        """acc[b] + (logit[b, a] - logsumexp(logit[b, :])) of every candidate of every live beam, evaluated in the context's dtype
        -> float64 numpy [N, L, A], -inf on the disallowed entries.  acc [N, L] (default 0)."""
        lg = self.logits(prefixes, t)
        ok = (lg != self.pad).numpy()
        a = torch.zeros(lg.shape[:2], dtype=self.dtype) if acc is None else torch.tensor(np.asarray(acc), dtype=self.dtype)
        s = a[:, :, None] + (lg - torch.logsumexp(lg, dim=2, keepdim=True))
        return np.where(ok, s.numpy().astype(np.float64), -np.inf)


def replay(parent, token):
    """A trace (parent, token int [N, 9, B]) -> (list over t of the prefixes BEFORE step t, int32 [N, L_t, 9] with L_0 = 1,
    final paths [N, B, 9])."""
    parent, token = np.asarray(parent), np.asarray(token)
    N = parent.shape[0]
    rows = np.arange(N)[:, None]
    pre, out = np.zeros((N, 1, T), dtype=np.int32), []
    for t in range(T):
        out.append(pre)
        assert (parent[:, t] >= 0).all() and (parent[:, t] < pre.shape[1]).all()
        new = pre[rows, parent[:, t]].copy()
        new[:, :, t] = token[:, t]
        pre = new
    return out, pre


def scores_along(ctx, parent, token):
    """The candidate scores of ctx along a given trace, the accumulated part recomputed in ctx's dtype along the trace's own
    prefixes -> (list over t of S [N, L_t, A], the trace's selected scores [N, 9, B])."""
    parent, token = np.asarray(parent), np.asarray(token)
    N, _, B = parent.shape
    rows = np.arange(N)[:, None]
    pres, _ = replay(parent, token)
    acc, S_all, sel = None, [], np.zeros((N, T, B))
    for t in range(T):
        S = ctx.candidate_scores(pres[t], t, acc)
        S_all.append(S)
        acc = S[rows, parent[:, t], token[:, t]]
        sel[:, t] = acc
    return S_all, sel


def select(S, B):
    """The best B of the candidates S [N, L, A] in descending order, equal scores by the smaller flat index
    -> (parent, token, score [N, B], gap [N]: the smallest difference between neighbours among the top B + 1 candidates)."""
    N, L, A = S.shape
    flat = S.reshape(N, L * A)
    order = np.argsort(-flat, axis=1, kind='stable')
    top = order[:, :B]
    score = np.take_along_axis(flat, top, axis=1)
    assert np.isfinite(score).all(), 'fewer than B candidates'
    lead = np.take_along_axis(flat, order[:, :B + 1], axis=1)
    d = lead[:, :-1] - lead[:, 1:]                    # (inf against a disallowed entry: no neighbour there)
    return top // A, top % A, score, d.min(axis=1)


def search(ctx, B):
    """-> (paths int32 [N, B, 9], scores [N, B], trace dict(parent, token, score [N, 9, B], gap [N, 9]))"""
    N = ctx.N
    rows = np.arange(N)[:, None]
    pre, acc = np.zeros((N, 1, T), dtype=np.int32), None
    tr = dict(parent=np.zeros((N, T, B), dtype=np.int32), token=np.zeros((N, T, B), dtype=np.int32), score=np.zeros((N, T, B)),
              gap=np.zeros((N, T)))
    for t in range(T):
        par, tok, acc, gap = select(ctx.candidate_scores(pre, t, acc), B)
        tr['parent'][:, t], tr['token'][:, t], tr['score'][:, t], tr['gap'][:, t] = par, tok, acc, gap
        new = pre[rows, par].copy()
        new[:, :, t] = tok
        pre = new
    return pre, acc, tr


def beam_search(flat, obs, dm, loc, special, B, seed=0, step=0, dtype=torch.float64):
    return search(Beam(flat, obs, dm, loc, special, seed, step, dtype), B)


def firm_rows(gap, bar):
    """bool [N]: every gap among the row's top B + 1 candidates is above two score bars at every step."""
    return (np.asarray(gap) > 2.0 * bar).all(axis=1)


# ---- cases ---------------------------------------------------------------------------------------------------------------
# (shape index of exactk_ref.GPU_SHAPES at dropout 0.1, B), each at its exactk_ref.DECODE_STREAMS[i]
CASES = ((0, 3), (1, 3), (3, 3), (3, 1), (3, 2), (3, 8))


def case_ctx(i, dtype=torch.float64):
    c = R.case(i, 0.1)
    seed, step = R.DECODE_STREAMS[i]
    return c, Beam(c['flat'], c['obs'], c['dm'], c['loc'], c['special'], seed, step, dtype)


def score_yardstick(i, B):
    """Largest |float32 - float64| of a selected score over all rows, steps and beams, along the float64 search's own prefixes
    -> (error, the float64 search's (paths, scores, trace))."""
    c, c64 = case_ctx(i)
    out = search(c64, B)
    tr = out[2]
    _, s32 = scores_along(case_ctx(i, torch.float32)[1], tr['parent'], tr['token'])
    return float(np.abs(s32 - tr['score']).max()), out


# score_yardstick(i, B), measured on the CPU (tests/test_exactk_beam_host.py reproduces them within a factor of 2)
MEASURED_SCORE = {
    (0, 3): 6.39e-06,
    (1, 3): 4.53e-06,
    (3, 3): 3.93e-06,
    (3, 1): 3.21e-06,
    (3, 2): 3.53e-06,
    (3, 8): 4.59e-06,
}


def score_bar(i, B):
    return R.BAR_FACTOR * MEASURED_SCORE[(i, B)]


# ---- the hand-built case in which greedy is not the best slate -----------------------------------------------------------------
# make_case(TINY_SHAPE, seed) with the two attention score vectors scaled by 4, which takes the logits off the near-flat profile of
# a fresh network.  Seeds 0 - 39 were walked at scales 1, 4, 16 with the float64 restatement alone, for a row whose best slate opens
# with the SECOND-best first item; seed 32, row 2 has the widest margin: greedy plays [2 6 1 3 7 9 0 4 8], beam 0 of B = 3 plays
# [1 2 6 3 7 9 0 4 8] and scores 0.049 more (sum of log-probabilities), with every gap among the top four candidates above 4e-3.
TINY = dict(seed=32, scale=4.0, scaled=('pointer_v', 'glimpse_v'), row=2, margin=0.04)


def tiny_case():
    """exactk_ref.TINY_SHAPE (A = 11, 3 rows), hand-built so that greedy is not the best slate on row TINY['row']."""
    c = R.make_case(R.TINY_SHAPE, TINY['seed'], 0.0)
    p = c['dm'].split(c['flat'])
    for name in TINY['scaled']:
        p[name] *= np.float32(TINY['scale'])
    return c

