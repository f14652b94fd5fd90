"""The raw-state training handle (rl4rs_rawtrain_* in rawtrain.hpp, the DQN entry points of rawdqn.hpp) at the row counts its trainers
run at: every form the shared sample-axis reductions and the fp32 GEMMs take by row count, which the 150 / 300 / 700-row tests never
enter.  tests/rawstate_rows_cases.py holds the (configuration, rows) table and, beside each case, the form of every GEMM, gradient
and st_back; tests/test_rawtrain_scratch_host.py sizes the scratch of every case on the host (u512_* could not run before
rawtrain_scratch.hpp counted dense_w2).

References: oracle.policy.rawstate_forward / rawstate_loss_and_grad (A2C / PPO) and tests/rawdqn_ref.py (DQN), float64.
Bars, none of them new:
  A2C / PPO  forward 2e-4, gradients 3e-4 of each array's largest entry, statistics rtol 2e-4 / atol 1e-3 - the floors of
             tests/test_gpu_policy.py - each times max(1, e32(case) / e32(floor configuration)), e32 the float32 evaluation of the
             restatement against its float64 evaluation on the same inputs (tests/test_gpu_policy_shapes.py: _raw_floor_e32, _ratio)
  DQN        4 x the restatement's own float32 error, statistics floored at 2^-24 (tests/test_gpu_rawdqn.py: _bars, MARGIN)
  Adam       1e-6 from the closed form of the first step (both files above)
  trainer    max(2e-5, 4 x the float32 restatement's distance from the float64 one) per parameter array; 2e-5 is the Adam bar of
             tests/test_gpu_dqn.py
Greedy actions and a*: the float64 first maximum, except on rows whose two largest masked float64 Q lie within 1e-4 (the empty-mask
row is one: every masked value is float32.min); at most max(2, N // 100) such rows, a condition the seeds are chosen under on the
CPU.  Where the device's a* differs on such a row the DQN reference bootstraps from the device's.

Measured on an MI355X (every test prints its figures under -s).  e32 is the CPU's: another host's BLAS gives other ratios.
  floor configuration: forward e32 2.19e-6, gradient e32 4.72e-7 (A2C) / 6.91e-7 (PPO)
  case           near-tie  forward e32 / ratio / worst error   A2C e32 / ratio   PPO e32 / ratio   worst gradient, relative (bar)
  base_n1030     1 of 10   2.81e-6 / 1.28 / 2.7e-6             6.16e-7 / 1.31    8.50e-7 / 1.23    ctx_w 7.5e-7 (3.9e-4)
  base_n2100     1 of 21   2.65e-6 / 1.21 / 2.5e-6             1.64e-6 / 3.48    1.52e-6 / 2.21    dense_w1 5.7e-7 (6.6e-4)
  base_n4100     1 of 41   2.86e-6 / 1.30 / 2.8e-6             2.20e-6 / 4.66    1.43e-6 / 2.06    seq_emb 4.6e-7 (6.2e-4)
  odd_n4100      1 of 41   1.44e-6 / 1    / 1.8e-6             1.11e-6 / 2.35    1.92e-6 / 2.78    seq_emb 5.0e-7 (7.0e-4)
  u512_n2100     1 of 21   1.62e-6 / 1    / 1.9e-6             7.98e-7 / 1.69    1.21e-6 / 1.75    dense_w1 5.0e-7 (5.1e-4)
  u512d64_n2100  2 of 21   2.38e-6 / 1.08 / 2.4e-6             1.01e-6 / 2.15    1.97e-6 / 2.85    dense_w1 5.0e-7 (6.5e-4)
  (near-tie: such rows found, of the number the cap allows - the one found everywhere is the empty-mask row; greedy equalled the float64 first maximum on every row of every case, the
  statistics agreed to 1e-7 relative, each global-norm-clipped Adam step was 2.9e-8 .. 3.0e-8 from its closed form)
  DQN, share of the 4 x e32 bar (double_q 1 / 0); near-tie bootstrapping rows per selecting net; a* differed from float64 nowhere
  case           near-tie   td            statistics    gradients (worst variable)                       clipped Adam
  base_n1030     0, 0       0.19 / 0.17   0.12 / 0.12   0.53 / 0.55 (dense_w1 6.9e-7 / 7.4e-7)           3.1e-8
  base_n4100     1, 0       0.16 / 0.29   0.25 / 0.25   0.84 / 0.77 (head_w 8.3e-7 / 8.4e-7, e32 2.5e-7)  3.0e-8
  odd_n4100      0, 1       0.15 / 0.15   0.02 / 0.01   0.74 / 0.80 (head_w 7.1e-7 / 7.2e-7, e32 2.4e-7)  2.9e-8
  u512_n2100     0, 1       0.26 / 0.27   0.05 / 0.11   0.32 / 0.28                                      3.0e-8
  (head_w at 4100 rows: k_dqn_w2_grad adds the 1367 rows that share one action one after the other; the tables' atomics stay at 3e-7)
  records against arrays (base_n2100, u512d64_n2100): a* equals greedy on 2100 of 2100 rows, double_q 1 and 0
  fewer rows after 4100 (base / odd): two fresh handles agreed bit for bit on everything but the two tables, and so did the used
  handle with a fresh one; PPO gradients of the 1030- and 70-row calls at most 7.5e-7 / 3.0e-7 relative (bars 3.0e-4 .. 3.4e-4, ratios
  1 .. 1.13); the 70-row DQN call used 0.22 (td), 0.38 (statistics), 0.22 (gradients) of its bars
  trainer, 1152 rows: worst parameter head_w 2.3e-6 from float64 (float32 restatement 1.6e-6, bar 2e-5); the others below 1.2e-7"""
import functools

import numpy as np
import pytest

import rawdqn_ref as R
import rawstate_rows_cases as T
from test_gpu_policy_shapes import KW, _bits, _entropy, _ratio, _raw_floor_e32, _raw_inputs, _raw_loss_args
from test_gpu_rawdqn import GAMMA, MARGIN, _as_f32, _bars, _env, _flat, _grad_err, _stats_err, _t, _weights

pytestmark = pytest.mark.gpu

NEAR_TIE = 1e-4
EMPTY_NEXT_MASK_ROW = 5


def _cap(N):
    return max(2, N // 100)


def _near_ties(q):
    """rows whose two largest masked float64 values lie within NEAR_TIE"""
    top = np.sort(q, axis=1)[:, -2:]
    return (top[:, 1] - top[:, 0]) <= NEAR_TIE


# ---- inputs and float64 references, computed once ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name):
    from oracle import policy as OP
    cfg, N = T.CASES[name]
    w, v, tv = _weights(cfg)
    for seed in range(300, 320):
        rs = np.random.RandomState(seed)
        cat, dense, seqs, mask, bits = _raw_inputs(cfg, N, rs)
        logits, value = OP.rawstate_forward(w, cat, dense, seqs, mask)
        tie = _near_ties(logits)
        if tie.sum() <= _cap(N):
            break
    else:
        raise AssertionError('no input seed keeps the near-ties of %s under %d rows' % (name, _cap(N)))
    l32, v32 = OP.rawstate_forward(w, cat, dense, seqs, mask, dtype=np.float32)
    ok = mask > 0
    e32 = max(np.abs(l32.astype(np.float64)[ok] - logits[ok]).max(), np.abs(v32.astype(np.float64) - value).max())
    lsm = OP.log_softmax(logits)
    actions = (mask * rs.rand(*mask.shape)).argmax(axis=1)             # a legal action of every row that has one
    args = _raw_loss_args(w, cat, dense, seqs, mask, actions, rs)
    return dict(cfg=cfg, N=N, w=w, v=v, tv=tv, seed=seed, cat=cat, dense=dense, seqs=seqs, mask=mask, bits=bits, logits=logits, value=value,
                lsm=lsm, ent=_entropy(lsm), tie=tie, e32=e32, args=args)


def _rows(args, lo):
    """the loss arguments of the rows from ``lo`` on"""
    return tuple([q[lo:] for q in a] if isinstance(a, list) else a[lo:] for a in args)


@functools.lru_cache(maxsize=None)
def _grad_ref(name, algo, lo=0):
    """-> (float64 gradients, float64 statistics, bar ratio, e32) of the A2C / PPO loss over the rows from ``lo`` on"""
    from oracle import policy as OP
    c = _case(name)
    args = _rows(c['args'], lo)
    g64, s64 = OP.rawstate_loss_and_grad(algo, c['w'], *args, **KW)
    g32, _ = OP.rawstate_loss_and_grad(algo, c['w'], *args, dtype=np.float32, **KW)
    e32 = max(np.abs(g32[k].astype(np.float64) - g64[k]).max() / max(np.abs(g64[k]).max(), 1e-8) for k in g64)
    return g64, s64, _ratio(e32, _raw_floor_e32()[1][algo]), e32


def _dqn_batch(cfg, N, seed):
    """tests/test_gpu_rawdqn.py's minibatch at N rows: terminal rows with poisoned successors (NaN dense, ids >= H and < 0), a third
    of the rows sharing one action, one action nobody takes, one empty next mask, weights in [0.2, 2]."""
    rs = np.random.RandomState(seed)
    H, A = cfg['category_hash_size'], cfg['action_size']

    def obs():
        cat, dense, seqs, _, _ = _raw_inputs(cfg, N, rs)
        return cat, dense, seqs
    rec = R.pack_records(cfg, *obs())
    ncat, ndense, nseqs = obs()
    done = (rs.rand(N) < 0.25).astype(np.int32)
    done[EMPTY_NEXT_MASK_ROW] = 0
    done[[0, 1, 2, N - 1]] = 1
    term = done.astype(bool)
    ndense[term] = np.nan
    ncat[term] = np.where(rs.rand(int(term.sum()), ncat.shape[1]) < 0.5, H + 5, 1 << 30).astype(np.int32)
    for q in nseqs:
        q[term] = -rs.randint(1, 1000, size=(int(term.sum()), q.shape[1])).astype(np.int32)
    mask = (rs.rand(N, A) < 0.4).astype(np.float64)
    mask[np.arange(N), rs.randint(0, A, size=N)] = 1.0
    mask[EMPTY_NEXT_MASK_ROW] = 0.0
    untaken = 3 % A
    act = rs.randint(0, A - 1, size=N)
    act[act >= untaken] += 1
    act[::3] = act[0]
    return dict(rec=rec, next_rec=R.pack_records(cfg, ncat, ndense, nseqs), act=act.astype(np.int32), rew=(rs.rand(N) * 2).astype(np.float32),
                done=done, mask=mask, bits=_bits(mask.astype(np.int64)), weights=(0.2 + 1.8 * rs.rand(N)).astype(np.float32), untaken=untaken)


def _dqn_ref(cfg, v, tv, b, double_q, dtype, astar=None, want_grad=True):
    return R.loss_and_grad(v, tv, cfg, b['rec'], b['act'], b['rew'], b['done'], b['next_rec'], b['mask'], weights=b['weights'], gamma=GAMMA,
                           double_q=double_q, dtype=dtype, want_grad=want_grad, astar=astar)


@functools.lru_cache(maxsize=None)
def _dqn_case(cfg_name, N):
    """The DQN minibatch of N rows at the configuration of case ``cfg_name``: the first data seed at which, for either selecting net,
    at most max(2, N // 100) bootstrapping rows have their two largest masked float64 Q(s') within NEAR_TIE."""
    cfg = T.CASES[cfg_name][0]
    w, v, tv = _weights(cfg)
    for seed in range(400, 420):
        b = _dqn_batch(cfg, N, seed)
        ties = [int((_dqn_ref(cfg, v, tv, b, dq, np.float64, want_grad=False)['gap'] <= NEAR_TIE).sum()) for dq in (True, False)]
        if max(ties) <= _cap(N):
            return cfg, w, v, tv, b, seed, ties
    raise AssertionError('no data seed keeps the near-ties of %s at %d rows under the cap' % (cfg_name, N))


@functools.lru_cache(maxsize=None)
def _dqn_refs(cfg_name, N, double_q):
    cfg, w, v, tv, b, seed, ties = _dqn_case(cfg_name, N)
    return _dqn_ref(cfg, v, tv, b, double_q, np.float64), _dqn_ref(cfg, v, tv, b, double_q, np.float32)


# ---- device calls ------------------------------------------------------------------------------------------------------------
def _trainer(cfg, w, max_rows):
    from rl4rs_amd.device import DeviceRawTrainer
    return DeviceRawTrainer(cfg, w, max_rows=max_rows)


def _obs_dev(c, lo=0):
    return _t(c['cat'][lo:]), _t(c['dense'][lo:]), [_t(q[lo:]) for q in c['seqs']], _t(c['bits'][lo:])


def _loss_call(tr, algo, args):
    """rl4rs_rawtrain_loss_grad on ``args`` -> (statistics, {variable: gradient}) as torch tensors (clones: the handle is reused)"""
    cat, dense, seqs, mask, actions, adv, ret, old_logp, old_value, old_logits = args
    f = lambda x: _t(np.asarray(x, dtype=np.float32))
    stats = tr.loss_grad(algo, _t(cat), _t(dense), [_t(q) for q in seqs], _t(actions.astype(np.int32)), f(adv), f(ret),
                         mask_bits=_t(_bits(mask)), old_logp=f(old_logp), old_value=f(old_value), old_logits=f(old_logits), **KW)
    return stats.clone(), dict((k, x.clone()) for k, x in tr.gradients().items())


def _check_grads(tag, stats, g, g64, s64, r_g, tables_only=False):
    g = dict((k, x.cpu().numpy()) for k, x in g.items())
    assert set(g) == set(g64)
    for k in sorted(g64):
        if tables_only and k not in R.TABLES:
            continue
        scale = max(np.abs(g64[k]).max(), 1e-8)
        err = np.abs(g[k] - g64[k]).max()
        print('%s %s: gradient %.3g of max %.3g (relative %.3g, bar %.3g)' % (tag, k, err, scale, err / scale, 3e-4 * r_g))
        assert np.isfinite(g[k]).all() and err < 3e-4 * r_g * scale, (tag, k, err, scale)
    if not tables_only:
        s = stats.cpu().numpy()
        print('%s statistics %s against %s (rtol %.3g atol %.3g)' % (tag, s, s64, 2e-4 * r_g, 1e-3 * r_g))
        assert np.allclose(s, s64, rtol=2e-4 * r_g, atol=1e-3 * r_g), (tag, s, s64)


def _dqn_call(tr, tv, b, double_q):
    td, stats, astar = tr.dqn_loss_grad(_t(_flat(tv)), _as_f32(b['rec']), _t(b['act']), _t(b['rew']), _t(b['done']), _as_f32(b['next_rec']),
                                        _t(b['bits']), weights=_t(b['weights']), gamma=GAMMA, double_q=double_q, want_next_action=True)
    return td.clone(), stats.clone(), astar.clone(), dict((k, x.clone()) for k, x in tr.gradients().items())


def _check_dqn(tag, cfg_name, N, double_q, out):
    """td, statistics, a* and the ten gradients of one dqn_loss_grad against the restatement"""
    cfg, w, v, tv, b, seed, ties = _dqn_case(cfg_name, N)
    r64, r32 = _dqn_refs(cfg_name, N, double_q)
    td, stats, astar, g = [x.cpu().numpy() for x in out[:3]] + [dict((k, x.cpu().numpy()) for k, x in out[3].items())]
    term = b['done'].astype(bool)
    assert (astar[term] == -1).all()
    assert not r64['boot'][EMPTY_NEXT_MASK_ROW] and r64['y'][EMPTY_NEXT_MASK_ROW] == float(b['rew'][EMPTY_NEXT_MASK_ROW])
    differ = ~term & (astar != r64['astar'])
    print('%s seed %d: %s near-tie rows in float64 (cap %d), a* differs on %d' % (tag, seed, ties, _cap(N), differ.sum()))
    assert (r64['gap'][differ] <= NEAR_TIE).all() and differ.sum() <= _cap(N), (tag, np.nonzero(differ)[0], r64['gap'][differ])
    if differ.any():
        legal = b['mask'][np.nonzero(differ)[0], astar[differ]]
        assert (legal > 0).all()
        r64, r32 = [_dqn_ref(cfg, v, tv, b, double_q, dt, astar=np.maximum(astar, 0)) for dt in (np.float64, np.float32)]
    bar = _bars(r32, r64)
    err = dict(td=np.abs(td.astype(np.float64) - r64['td']).max(), stats=_stats_err(stats, r64['stats']), grad=_grad_err(g, r64['grad']))
    for k in R.ORDER:
        e = np.abs(g[k].astype(np.float64) - r64['grad'][k]).max() / max(np.abs(r64['grad'][k]).max(), 1e-8)
        print('%s %s: gradient relative %.3g (bar %.3g)' % (tag, k, e, MARGIN * bar['grad']))
    print('%s: ' % tag + '  '.join('%s device %.3g e32 %.3g (share of the bar %.2f)' % (k, err[k], bar[k], err[k] / (MARGIN * bar[k])) for k in sorted(err)))
    assert np.isfinite(td).all() and np.isfinite(stats).all() and all(np.isfinite(x).all() for x in g.values())
    for k in sorted(err):
        assert err[k] <= MARGIN * bar[k], (tag, k, err[k], bar[k])
    # exact zeros: the value column and the action columns nobody took
    idle = np.setdiff1d(np.arange(cfg['action_size'] + 1), np.unique(b['act']))
    assert cfg['action_size'] in idle and b['untaken'] in idle and np.bincount(b['act']).max() >= N // 3
    assert (g['head_w'][:, idle] == 0).all() and (g['head_b'][idle] == 0).all()
    return r64


def _same_bits(tag, a, b, skip=()):
    """two (..., {variable: gradient}) results: every tensor but the gradients named in ``skip`` bit for bit"""
    import torch
    for i, (x, y) in enumerate(zip(a[:-1], b[:-1])):
        assert torch.equal(x, y), (tag, 'output %d' % i)
    for k in R.ORDER:
        if k not in skip:
            assert torch.equal(a[-1][k], b[-1][k]), (tag, k)


# ---- 1. forward, actions, greedy ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(T.CASES))
def test_forward_and_actions(name):
    import torch
    from rl4rs_amd.device import DeviceRawPolicy
    c = _case(name)
    cfg, N, mask = c['cfg'], c['N'], c['mask']
    A = cfg['action_size']
    bar = 2e-4 * _ratio(c['e32'], _raw_floor_e32()[0])
    print('%s seed %d: forward e32 %.3g (floor %.3g), bar %.3g; %d near-tie rows (cap %d)' % (name, c['seed'], c['e32'], _raw_floor_e32()[0], bar,
                                                                                         c['tie'].sum(), _cap(N)))
    assert c['tie'].sum() <= _cap(N) and c['tie'][2]                  # row 2 allows nothing: all its masked values are equal
    cat, dense, seqs, bits = _obs_dev(c)
    ok, live = mask > 0, mask.any(axis=1)
    trainer = _trainer(cfg, c['w'], N)
    for kind, pol in (('policy', DeviceRawPolicy(cfg, c['w'], max_rows=N)), ('trainer', trainer)):
        a, lp, v, ent, lg = pol.act(cat, dense, seqs, bits, seed=5, step=3, want_logits=True)
        a_np, lg_np = a.cpu().numpy(), lg.cpu().numpy()
        assert ((a_np >= 0) & (a_np < A)).all() and mask[np.arange(N)[live], a_np[live]].all()
        assert torch.equal(a, pol.act(cat, dense, seqs, bits, seed=5, step=3)[0])
        errs = dict(logits=np.abs(lg_np[ok] - c['logits'][ok]).max(), value=np.abs(v.cpu().numpy() - c['value']).max(),
                    logp=np.abs(lp.cpu().numpy() - c['lsm'][np.arange(N), a_np]).max(), entropy=np.abs(ent.cpu().numpy() - c['ent']).max())
        print('%s %s forward: %s  bar %.3g' % (name, kind, ' '.join('%s %.3g' % kv for kv in sorted(errs.items())), bar))
        assert max(errs.values()) < bar, (name, kind, errs)
        assert (lg_np[~ok] < -1e37).all()
        lp2, v2, ent2, _ = pol.evaluate(cat, dense, seqs, a, bits)
        assert torch.equal(lp, lp2) and torch.equal(v, v2) and torch.equal(ent, ent2)
        if pol is not trainer:
            pol.close()
    ga, gq = trainer.greedy(cat, dense, seqs, bits, want_q=True)
    ga, gq = ga.cpu().numpy(), gq.cpu().numpy()
    want = c['logits'].argmax(axis=1)
    differ = ga != want
    print('%s greedy: differs from the float64 first maximum on %d rows, all near-ties; masked Q %.3g from float64' % (
        name, differ.sum(), np.abs(gq[ok] - c['logits'][ok]).max()))
    assert not (differ & ~c['tie']).any(), np.nonzero(differ & ~c['tie'])[0]
    assert ga[2] == 0 and np.abs(gq[ok] - c['logits'][ok]).max() < bar and (gq[~ok] < -1e37).all()
    trainer.close()


# ---- 2. A2C / PPO gradients, Adam ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(T.CASES))
def test_a2c_ppo_gradients_and_adam(name):
    c = _case(name)
    trainer = _trainer(c['cfg'], c['w'], c['N'])
    for algo in (0, 1):
        g64, s64, r_g, e32 = _grad_ref(name, algo)
        print('%s algo %d: gradient e32 %.3g (floor %.3g), ratio %.3g' % (name, algo, e32, _raw_floor_e32()[1][algo], r_g))
        stats, g = _loss_call(trainer, algo, c['args'])
        _check_grads('%s algo %d' % (name, algo), stats, g, g64, s64, r_g)
    before, gflat = trainer._flat('params').cpu().numpy().astype(np.float64), trainer._flat('grad').cpu().numpy().astype(np.float64)
    trainer.adam_step(lr=1e-3, grad_clip=10.0)
    after = trainer._flat('params').cpu().numpy().astype(np.float64)
    gc = gflat * min(1.0, 10.0 / np.sqrt((gflat ** 2).sum()))
    lr_t = 1e-3 * np.sqrt(1 - 0.999) / (1 - 0.9)
    err = np.abs(after - (before - lr_t * (0.1 * gc) / (np.sqrt(0.001 * gc * gc) + 1e-8))).max()
    print('%s clipped Adam step: %.3g from the closed form (bar 1e-6), gradient norm %.4g' % (name, err, np.sqrt((gflat ** 2).sum())))
    assert err < 1e-6
    trainer.close()


# ---- 3. DQN on packed records --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('double_q', [True, False])
@pytest.mark.parametrize('name', T.DQN_CASES)
def test_dqn_loss_gradient_and_adam(name, double_q):
    cfg, N = T.CASES[name]
    _, w, v, tv, b, seed, ties = _dqn_case(name, N)
    tr = _trainer(cfg, w, N)
    out = _dqn_call(tr, tv, b, double_q)
    _check_dqn('%s double_q %d' % (name, double_q), name, N, double_q, out)
    g = dict((k, x.cpu().numpy().astype(np.float64)) for k, x in out[3].items())
    norms = R.var_norms(g)
    clip = float(np.median(norms))
    assert (norms > clip).any() and (norms < clip).any()
    before = dict((k, x.cpu().numpy()) for k, x in tr.weights().items())
    tr.adam_step_clip_by_var(lr=1e-3, var_clip=clip)
    after = dict((k, x.cpu().numpy()) for k, x in tr.weights().items())
    want = R.adam_clip_by_var_first_step(before, g, 1e-3, clip)
    err = max(np.abs(after[k].astype(np.float64) - want[k]).max() for k in R.ORDER)
    print('%s double_q %d clipped Adam step: %.3g from the closed form (bar 1e-6); norms %s clip %.4g' % (name, double_q, err, np.round(norms, 4), clip))
    assert err < 1e-6
    tr.close()


@pytest.mark.parametrize('name', T.RECORD_CASES)
def test_forward_from_records_gives_the_bits_of_the_forward_from_arrays(name):
    """rawdqn.hpp: "a forward from records gives the bits of a forward from the unpacked arrays".  greedy reads the arrays (dense rows
    Dn floats apart), the selecting forward of dqn_loss_grad reads records (REC apart) holding the same rows; every row is
    non-terminal.  The a* of a double-Q call (online net) and of a plain call whose target is the online net's own parameters equal
    greedy's actions on every row, the empty-mask row included."""
    c = _case(name)
    cfg, N = c['cfg'], c['N']
    assert T.dims(cfg)[2] != cfg['dense_feature_num']
    tr = _trainer(cfg, c['w'], N)
    cat, dense, seqs, bits = _obs_dev(c)
    ga = tr.greedy(cat, dense, seqs, bits)[0].cpu().numpy()
    rec = tr.pack_records(cat, dense, seqs)
    assert np.array_equal(R.as_words(rec.cpu().numpy()), R.pack_records(cfg, c['cat'], c['dense'], c['seqs']))
    rs = np.random.RandomState(1)
    act, rew = _t(rs.randint(0, cfg['action_size'], size=N).astype(np.int32)), _t(rs.rand(N).astype(np.float32))
    done = _t(np.zeros(N, dtype=np.int32))
    for double_q, target in ((True, _t(_flat(c['tv']))), (False, tr.params().clone())):
        td, stats, astar = tr.dqn_loss_grad(target, rec, act, rew, done, rec, bits, gamma=GAMMA, double_q=double_q, want_next_action=True)
        astar = astar.cpu().numpy()
        print('%s double_q %d: a* from records differs from greedy on arrays in %d of %d rows' % (name, double_q, (astar != ga).sum(), N))
        assert np.array_equal(astar, ga) and np.isfinite(td.cpu().numpy()).all()
    tr.close()


# ---- 4. fewer rows after a full batch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['base_n4100', 'odd_n4100'])
def test_fewer_rows_after_a_full_batch(name):
    """One handle of max_rows 4100: the 4100-row PPO call, then PPO on the last 1030 and on the last 70 rows (row i of a small call is
    not row i of the large one), then a 70-row dqn_loss_grad - on activations, terms, d_ctx and chunk partials that hold the larger
    calls' values.  Each small call against float64 at the bars and against a fresh handle of max_rows = its rows: the plans depend
    on the call's rows only and the reductions are fixed-order, so statistics, td, a* and the eight non-table gradients are bit
    for bit the fresh handle's - as two fresh handles are each other's, which is established first.  The two tables' gradients come
    from float atomics (k_emb_mean_bwd / k_rec_emb_mean_bwd): compared at the float64 bar only."""
    c = _case(name)
    cfg, N = c['cfg'], c['N']
    used = _trainer(cfg, c['w'], N)
    _loss_call(used, 1, c['args'])
    for n in (1030, 70):
        lo = N - n
        tag = '%s last %d rows' % (name, n)
        g64, s64, r_g, e32 = _grad_ref(name, 1, lo)
        args = _rows(c['args'], lo)
        fresh = []
        for _ in range(2):
            h = _trainer(cfg, c['w'], n)
            fresh.append(_loss_call(h, 1, args))
            h.close()
        _same_bits(tag + ', two fresh handles', fresh[0], fresh[1], skip=R.TABLES)
        got = _loss_call(used, 1, args)
        print('%s: gradient e32 %.3g ratio %.3g' % (tag, e32, r_g))
        _check_grads(tag + ' (used handle)', got[0], got[1], g64, s64, r_g)
        _check_grads(tag + ' (fresh handle)', fresh[0][0], fresh[0][1], g64, s64, r_g, tables_only=True)
        _same_bits(tag + ', used against fresh', got, fresh[0], skip=R.TABLES)
    n = 70
    _, w, v, tv, b, seed, ties = _dqn_case(name, n)
    fresh = []
    for _ in range(2):
        h = _trainer(cfg, w, n)
        fresh.append(_dqn_call(h, tv, b, True))
        h.close()
    _same_bits('%s dqn, two fresh handles' % name, fresh[0], fresh[1], skip=R.TABLES)
    got = _dqn_call(used, tv, b, True)
    _check_dqn('%s dqn 70 rows (used handle)' % name, name, n, True, got)
    _check_dqn('%s dqn 70 rows (fresh handle)' % name, name, n, True, fresh[0])
    _same_bits('%s dqn, used against fresh' % name, got, fresh[0], skip=R.TABLES)
    used.close()


# ---- 5. the A2C trainer's one 1152-row call -----------------------------------------------------------------------------------
def _clipped_adam_first_step(params, grad, lr, grad_clip, dtype):
    """Closed form of the first TF-form Adam step from zero moments with the global-norm clip, evaluated in ``dtype``"""
    f = np.dtype(dtype).type
    g = dict((k, np.asarray(x, dtype=dtype)) for k, x in grad.items())
    norm = np.sqrt(sum((x * x).sum(dtype=dtype) for x in g.values()))
    scale = min(f(1.0), f(grad_clip) / norm)
    lr_t = f(lr) * np.sqrt(f(1) - f(0.999)) / (f(1) - f(0.9))
    out = {}
    for k, x in g.items():
        gc = x * scale
        out[k] = np.asarray(params[k], dtype=dtype) - lr_t * (f(0.1) * gc) / (np.sqrt(f(0.001) * gc * gc) + f(1e-8))
    return out


def test_a2c_train_iteration_updates_as_the_restatement(tmp_path):
    """RawStateTrainer(A2C) at batch_size 128: its one loss_grad call covers 128 * 9 = 1152 rows (k_gemm_tn in 3 chunks, chunked
    st_cs).  After one train_iteration: returns and advantages recomputed from the rollout in tr.buf (float64 reward-to-go, rounded
    to the float32 the device was handed; advantage = return - the value the device recorded), rawstate_loss_and_grad and the
    clipped Adam step from the initial weights, against the device's ten parameter arrays."""
    from oracle import policy as OP
    from rl4rs_amd.nets.rawpolicy import init_rawpolicy_weights
    from rl4rs_amd.train import RawStateTrainer
    B, Tn = 128, 9
    env = _env(tmp_path, B, Tn)
    cfg = env.config
    w0 = init_rawpolicy_weights(cfg, seed=0)
    tr = RawStateTrainer(env, algo='A2C', seed=1, lr=1e-3, weights=w0)
    assert tr.policy.max_rows == B * Tn == 1152
    out = tr.train_iteration()
    assert np.isfinite(list(out.values())).all()
    b = tr.buf
    host = lambda x: x.cpu().numpy()
    rew = host(b['rew']).astype(np.float64).reshape(Tn, B)
    ret = np.flip(np.cumsum(np.flip(rew, axis=0), axis=0), axis=0).reshape(-1).astype(np.float32)
    adv = ret - host(b['val'])                                          # float32, as the device forms it
    mask = R.unpack_bits(host(b['mask']), cfg['action_size'])
    args = (host(b['cat']), host(b['dense']), [host(q) for q in b['seqs']], mask, host(b['act']), adv.astype(np.float64), ret.astype(np.float64))
    assert mask[np.arange(B * Tn), args[4]].all()
    p0 = R.flat_weights(w0)
    new = {}
    for dt in (np.float64, np.float32):
        g, _ = OP.rawstate_loss_and_grad(0, w0, *args, vf_coeff=0.5, ent_coeff=0.01, dtype=dt)
        new[dt] = _clipped_adam_first_step(p0, g, 1e-3, 10.0, dt)
    dev = dict((k, host(x)) for k, x in tr.policy.weights().items())
    bad = []
    for k in R.ORDER:
        d32 = np.abs(new[np.float32][k].astype(np.float64) - new[np.float64][k]).max()
        err = np.abs(dev[k].astype(np.float64) - new[np.float64][k]).max()
        bar = max(2e-5, 4.0 * d32)
        moved = np.abs(new[np.float64][k] - p0[k]).max()
        print('trainer %s: device %.3g from float64, float32 restatement %.3g, bar %.3g (the step moved it by %.3g)' % (k, err, d32, bar, moved))
        assert moved > 1e-4
        if not err <= bar:
            bad.append((k, err, bar))
    assert not bad, bad
