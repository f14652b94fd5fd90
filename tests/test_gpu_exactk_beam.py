"""GPU: rl4rs_exactk_decode_beam (beam search over Exact-K's pointer decoder, one user per workgroup with all of its beams) against
the float64 restatement tests/exactk_beam_ref.py, and the trainer's eval_mode='beam'.

Cases: exactk_ref.case(i, 0.1) at exactk_ref.DECODE_STREAMS[i]; i in (0, 1, 3) at B = 3 (284 candidates at 37 rows; 75 at 5 rows;
64 candidates, two blocks, at 33 rows: none a multiple of the wave in both A and N; the random masks make 15 % of the candidates
special, so the beams of a user differ in their special-item state) and i = 3 at B in (1, 2, 8).

The score bar of a case is exactk_ref.BAR_FACTOR x exactk_beam_ref.MEASURED_SCORE: the float32 restatement's error against the
float64 one along the float64 search's own prefixes, measured on the CPU.  The per-step check excludes no row: it follows the
DEVICE's prefixes (rebuilt from its trace) and asks that what the device selected is, within the bar, what float64 would select
there.  Whole paths are compared on the rows that are firm in the restatement's own search (every gap among the top B + 1
candidates above two bars at every step; tests/test_exactk_beam_host.py counts them)."""
import functools
import os

import numpy as np
import pytest

import exactk_beam_ref as BR
import exactk_ref as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _ctx(i):
    """(case, float64 context): computed once, shared, never modified"""
    return BR.case_ctx(i)


@functools.lru_cache(maxsize=None)
def _ref(i, B):
    return BR.search(_ctx(i)[1], B)


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _net(c, max_rows=None):
    from rl4rs_amd.device import DeviceExactK
    dm = c['dm']
    return DeviceExactK(c['loc'], c['special'], max_rows=max_rows or c['N'], obs_dim=dm.od, action_size=dm.A, hidden_units=dm.H,
                        num_heads=dm.heads, num_blocks=dm.blocks, vocab=dm.vocab, dropout_rate=dm.rate, params=c['flat'])


def _np(x):
    return x.cpu().numpy()


@pytest.mark.parametrize('i,B', BR.CASES)
def test_every_row_step_selects_what_float64_selects_there(i, B):
    c, ctx = _ctx(i)
    seed, step = R.DECODE_STREAMS[i]
    bar = BR.score_bar(i, B)
    N, A = c['N'], c['dm'].A
    net = _net(c)
    paths, scores, tr = net.decode_beam(_t(c['obs']), beam_size=B, seed=seed, step=step, want_trace=True)
    paths, scores = _np(paths), _np(scores)
    par, tok, sc = _np(tr['parent']), _np(tr['token']), _np(tr['score'])
    net.close()
    assert paths.shape == (N, B, R.T) and scores.shape == (N, B) and par.shape == tok.shape == sc.shape == (N, R.T, B)
    assert (par[:, 0] == 0).all() and ((par >= 0) & (par < B)).all() and ((tok >= 0) & (tok < A)).all()
    S_all, sel = BR.scores_along(ctx, par, tok)                      # float64 along the device's own prefixes
    rows = np.arange(N)[:, None]
    worst = dict(score=0.0, passed_over=-np.inf, order=-np.inf)
    for t in range(R.T):
        S = S_all[t]
        flat = par[:, t].astype(np.int64) * A + tok[:, t]
        assert all(len(set(r.tolist())) == B for r in flat), t                           # B distinct (parent, token) pairs
        assert np.isfinite(sel[:, t]).all(), t                                           # each in its beam's allowed set
        worst['score'] = max(worst['score'], np.abs(sc[:, t].astype(np.float64) - sel[:, t]).max())
        rest = S.copy()
        rest[rows, par[:, t], tok[:, t]] = -np.inf
        worst['passed_over'] = max(worst['passed_over'], (rest.reshape(N, -1).max(axis=1) - sel[:, t].min(axis=1)).max())
        if B > 1:
            worst['order'] = max(worst['order'], (sel[:, t, 1:] - sel[:, t, :-1]).max())
        # the device's own scores: exactly non-increasing, equal scores by the smaller flat index
        d = np.diff(sc[:, t], axis=1)
        assert (d <= 0).all(), t
        assert (np.diff(flat, axis=1)[d == 0] > 0).all(), t
    print('case %s: score err %.3g (bar %.3g); best candidate passed over %.3g, selected out of order %.3g (allowed %.3g)'
          % ((i, B), worst['score'], bar, worst['passed_over'], worst['order'], 2.0 * bar))
    assert worst['score'] <= bar
    assert worst['passed_over'] <= 2.0 * bar
    assert worst['order'] <= 2.0 * bar
    # paths and scores are what the trace implies
    assert np.array_equal(BR.replay(par, tok)[1], paths)
    assert np.array_equal(sc[:, -1], scores)
    for b in range(B):
        assert all(len(set(r.tolist())) == R.T for r in paths[:, b])
    # firm rows: the restatement's own beams, order included
    ref_paths, _, ref_tr = _ref(i, B)
    firm = BR.firm_rows(ref_tr['gap'], bar)
    print('case %s: %d of %d rows firm' % ((i, B), int(firm.sum()), N))
    assert np.array_equal(paths[firm], ref_paths[firm])


@pytest.mark.parametrize('i', (0, 1, 3))
def test_one_beam_is_the_greedy_decode(i):
    """paths[:, 0] of B = 1 equals decode(greedy=True) at the same (seed, step) on every row whose float64 top-two logit gap is at
    least ten logit bars at each step (the rule of test_gpu_exactk.test_greedy_and_sampled_paths)."""
    c, _ = _ctx(i)
    seed, step = R.DECODE_STREAMS[i]
    logit_bar = R.bars((i, 0.1))[0]
    net = _net(c)
    obs = _t(c['obs'])
    paths, scores = net.decode_beam(obs, beam_size=1, seed=seed, step=step)
    greedy, _ = net.decode(obs, greedy=True, seed=seed, step=step)
    paths, greedy = _np(paths), _np(greedy)
    net.close()
    ref = R.logits_of(c['flat'], c['obs'], greedy, c['dm'], c['loc'], c['special'], seed=seed, step=step, pas=1).astype(np.float64)
    firm = (R.top_two_gap(ref) >= 10.0 * logit_bar).all(axis=1)
    print('B = 1 against greedy: %d of %d rows compared, %d equal' % (int(firm.sum()), c['N'], int((paths[:, 0] == greedy).all(axis=1).sum())))
    assert np.array_equal(paths[firm, 0], greedy[firm])


def test_identical_calls_are_bit_identical_and_the_trace_is_optional():
    import torch
    c, _ = _ctx(3)
    seed, step = R.DECODE_STREAMS[3]
    net = _net(c)
    obs = _t(c['obs'])
    p1, s1, t1 = net.decode_beam(obs, beam_size=3, seed=seed, step=step, want_trace=True)
    p2, s2, t2 = net.decode_beam(obs, beam_size=3, seed=seed, step=step, want_trace=True)
    assert torch.equal(p1, p2) and torch.equal(s1, s2) and all(torch.equal(t1[k], t2[k]) for k in ('parent', 'token', 'score'))
    p3, s3 = net.decode_beam(obs, beam_size=3, seed=seed, step=step)
    assert torch.equal(p1, p3) and torch.equal(s1, s3)
    p4, _ = net.decode_beam(obs, beam_size=3, seed=seed, step=step + 1)                  # other keep masks
    assert not torch.equal(p1, p4)
    net.close()


def test_beam_scratch_is_its_own():
    """N = 33, B = 8 and then N = 5, B = 2 on one handle equal a fresh handle; loss_grad and a greedy decode after a decode_beam equal
    those of a handle that never ran beam search, bit for bit."""
    import torch
    c, _ = _ctx(3)
    seed, step = R.DECODE_STREAMS[3]
    obs, path, w = _t(c['obs']), _t(c['path']), _t(c['w'])
    small = _t(c['obs'][:5])
    used, fresh = _net(c), _net(c)
    big = used.decode_beam(obs, beam_size=8, seed=seed, step=step, want_trace=True)
    assert bool(torch.isfinite(big[1]).all())
    after = used.decode_beam(small, beam_size=2, seed=seed, step=step, want_trace=True)
    alone = fresh.decode_beam(small, beam_size=2, seed=seed, step=step, want_trace=True)
    assert torch.equal(after[0], alone[0]) and torch.equal(after[1], alone[1])
    assert all(torch.equal(after[2][k], alone[2][k]) for k in ('parent', 'token', 'score'))
    fresh.close()

    def rest(net):
        stats, lg = net.loss_grad(obs, path, w, seed=5, step=7, want_logits=True)
        return [stats, lg, net.grad().clone()] + list(net.decode(obs, greedy=True, seed=seed, step=step, want_logits=True))

    never = _net(c)
    a, b = rest(used), rest(never)
    for name, x, y in zip(('stats', 'logits', 'gradient', 'greedy path', 'greedy logits'), a, b):
        assert torch.equal(x, y), name
    assert float(a[2].abs().max()) > 0
    used.close()
    never.close()


def test_refusals_name_their_reason():
    from rl4rs_amd._lib import Rl4rsHipError
    c, _ = _ctx(1)
    net = _net(c)
    obs = _t(c['obs'])
    for beam in (0, 9):
        with pytest.raises(Rl4rsHipError, match=r'beam %d outside \[1, 8\]' % beam):
            net.decode_beam(obs, beam_size=beam)
    with pytest.raises(Rl4rsHipError, match=r'N 6 outside \[1, max_rows = 5\]'):
        net.decode_beam(_t(np.concatenate([c['obs'], c['obs'][:1]])), beam_size=3)
    paths, scores = net.decode_beam(obs, beam_size=3)                                    # the handle is as good as before
    assert np.isfinite(_np(scores)).all()
    net.close()


# ---- the trainer ---------------------------------------------------------------------------------------------------------------
def _env(d, B=8, T=9):
    import rl4rs_amd
    from rl4rs_amd import synth
    from rl4rs_amd.env.slate import SlateRecEnv, SlateState
    text = synth.make_catalog_text(seed=4)
    synth.write_text(os.path.join(d, 'c.csv'), text)
    recs = synth.make_records(300, seed=2, hash_size=2000, special_ids=synth.special_ids_from_text(text))
    synth.write_records(os.path.join(d, 'log.csv'), recs)
    cfg = {"maxlen": 64, "batch_size": B, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
           "category_feature_num": 21, "category_hash_size": 2000, "seq_num": 2, "emb_size": 128, "page_items": 9,
           "hidden_units": 128, "max_steps": T, "action_emb_size": 32, "sample_file": os.path.join(d, 'log.csv'),
           "iteminfo_file": os.path.join(d, 'c.csv'), "cache_size": 256, "model_seed": 3, "return_tensors": True}
    return rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))


def test_trainer_evaluates_beam_zero(tmp_path):
    """eval_mode='beam': the mean reward of an evaluation equals playing decode_beam(...)[0][:, 0] by hand on the same users;
    eval_mode='greedy' (the default) equals playing decode(greedy=True) by hand, as before."""
    import torch
    from rl4rs_amd.train import ExactKTrainer
    env = _env(str(tmp_path))
    env.seed(5)

    def by_hand(tr, decode):
        state = np.random.get_state()
        try:
            np.random.seed(0)
            obs0 = tr._obs(env.reset(reset_file=True))
            return float(tr._play(decode(tr.policy, obs0)).to(torch.float64).mean().item())
        finally:
            np.random.set_state(state)

    out = {}
    for mode, kw, decode in (('default', {}, lambda p, o: p.decode(o, greedy=True, seed=1, step=0)[0]),
                             ('greedy', dict(eval_mode='greedy'), lambda p, o: p.decode(o, greedy=True, seed=1, step=0)[0]),
                             ('beam', dict(eval_mode='beam', beam_size=3),
                              lambda p, o: p.decode_beam(o, beam_size=3, seed=1, step=0)[0][:, 0].contiguous())):
        tr = ExactKTrainer(env, seed=1, init_seed=2, **kw)
        a, b = tr.evaluate(), tr.evaluate()
        assert a == b and np.isfinite(a)
        assert a == by_hand(tr, decode), mode
        out[mode] = a
        tr.close()
    print('evaluation: greedy %.6f, beam 0 of 3 %.6f' % (out['greedy'], out['beam']))
    assert out['default'] == out['greedy']
