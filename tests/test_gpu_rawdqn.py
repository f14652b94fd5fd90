"""On-device raw-state DQN (rl4rs_rawstate_* / rl4rs_rawtrain_dqn_loss_grad / _greedy / _adam_step_clip_by_var, RawDQNTrainer)
against the float64 restatement tests/rawdqn_ref.py, at the configurations of tests/test_gpu_policy_shapes.py.

The bar of every comparison is measured, not fixed: the float32 run of the restatement against its float64 run on the same inputs,
and the device is allowed 4 x that (the project's margin for a different summation order: MFMA tiles against numpy).  Every test
prints both numbers.

Measured on an MI355X (share of the bar the device used, worst case over double_q / weights): see DESIGN.md, "Raw-state DQN"."""
import functools
import os

import numpy as np
import pytest

import rawdqn_ref as R
from test_gpu_policy_shapes import RAW_CFGS, RAW_FLOOR, _bits

pytestmark = pytest.mark.gpu

CFGS = dict(RAW_CFGS, floor=RAW_FLOOR)
N_ROWS = 150                # two full 64-row ballots of the head-gradient kernel plus a ragged one; N % 4 != 0
GAMMA = 0.97
MARGIN = 4.0
EMPTY_MASK_ROWS = (5, 70, 140)


def _weights(cfg):
    from rl4rs_amd.nets.rawpolicy import init_rawpolicy_weights
    w = init_rawpolicy_weights(cfg, seed=2, emb_scale=0.5, head_std=1.0, bias_noise=0.2)
    v = R.flat_weights(w)
    rs = np.random.RandomState(77)
    tv = dict((k, x + (rs.randn(*x.shape) * 0.02).astype(np.float32)) for k, x in v.items())
    return w, v, tv


def _obs(cfg, N, rs):
    H = cfg['category_hash_size']
    cat = rs.randint(0, H, size=(N, cfg['category_feature_num'])).astype(np.int32)
    dense = np.abs(rs.randn(N, cfg['dense_feature_num']) * 2).astype(np.float32)
    seqs = [rs.randint(0, H, size=(N, cfg['maxlen'])).astype(np.int32) for _ in range(cfg['seq_num'])]
    return cat, dense, seqs


def _make_batch(cfg, seed):
    rs = np.random.RandomState(seed)
    N, H, A = N_ROWS, cfg['category_hash_size'], cfg['action_size']
    rec = R.pack_records(cfg, *_obs(cfg, N, rs))
    ncat, ndense, nseqs = _obs(cfg, N, rs)
    done = (rs.rand(N) < 0.25).astype(np.int32)
    done[list(EMPTY_MASK_ROWS)] = 0
    done[[0, 1, 2, N - 1]] = 1
    term = done.astype(bool)
    # terminal rows: poisoned successors (NaN dense, ids >= H and < 0)
    ndense[term] = np.nan
    ncat[term] = np.where(rs.rand(int(term.sum()), ncat.shape[1]) < 0.5, H + 5, 1 << 30).astype(np.int32)
    for q in nseqs:
        q[term] = -rs.randint(1, 1000, size=(int(term.sum()), q.shape[1])).astype(np.int32)
    nrec = R.pack_records(cfg, ncat, ndense, nseqs)
    mask = (rs.rand(N, A) < 0.4).astype(np.float64)
    mask[np.arange(N), rs.randint(0, A, size=N)] = 1.0
    mask[list(EMPTY_MASK_ROWS)] = 0.0
    untaken = 3 % A
    act = rs.randint(0, A - 1, size=N)
    act[act >= untaken] += 1
    act[::3] = act[0]                                          # many rows share one action
    return dict(rec=rec, next_rec=nrec, next_obs=(ncat, ndense, nseqs), act=act.astype(np.int32), rew=(rs.rand(N) * 2).astype(np.float32),
                done=done, mask=mask, bits=_bits(mask.astype(np.int64)), weights=(0.2 + 1.8 * rs.rand(N)).astype(np.float32),
                untaken=untaken)


def _ref(cfg, v, tv, b, double_q, weighted, dtype, want_grad=True):
    return R.loss_and_grad(v, tv, cfg, b['rec'], b['act'], b['rew'], b['done'], b['next_rec'], b['mask'],
                           weights=b['weights'] if weighted else None, gamma=GAMMA, double_q=double_q, dtype=dtype, want_grad=want_grad)


def _q_e32(r32, r64, mask):
    ok = (mask > 0) & r64['boot'][:, None]
    return np.abs(r32['q_sel'].astype(np.float64)[ok] - r64['q_sel'][ok]).max()


@functools.lru_cache(maxsize=None)
def _case(name):
    """Weights and the minibatch of configuration ``name``.  The data seed is the first one at which, in the restatement, every
    bootstrapping row's gap between the two largest masked Q(s') exceeds 100 x the restatement's own float32 error on Q - for both
    selecting nets - so no row has to be excluded for a near-tie.  Chosen on the CPU from the restatement alone."""
    cfg = CFGS[name]
    w, v, tv = _weights(cfg)
    for seed in range(100, 140):
        b = _make_batch(cfg, seed)
        ok = True
        for dq in (True, False):
            r64 = _ref(cfg, v, tv, b, dq, False, np.float64, want_grad=False)
            r32 = _ref(cfg, v, tv, b, dq, False, np.float32, want_grad=False)
            ok = ok and r64['gap'].min() > 100.0 * _q_e32(r32, r64, b['mask'])
        if ok:
            return cfg, w, v, tv, b, seed
    raise AssertionError('no data seed keeps every row away from a near-tie at %s' % name)


@functools.lru_cache(maxsize=None)
def _refs(name, double_q, weighted):
    cfg, w, v, tv, b, seed = _case(name)
    return _ref(cfg, v, tv, b, double_q, weighted, np.float64), _ref(cfg, v, tv, b, double_q, weighted, np.float32)


def _grad_err(g, g64):
    return max(np.abs(np.asarray(g[k], dtype=np.float64) - g64[k]).max() / max(np.abs(g64[k]).max(), 1e-8) for k in g64)


def _stats_err(s, s64):
    return (np.abs(np.asarray(s, dtype=np.float64) - s64) / np.maximum(np.abs(s64), 1.0)).max()


def _bars(r32, r64):
    """The restatement's own float32 error per quantity.  ``stats`` is four numbers only, so its measured error is a draw that can
    fall far below what float32 can represent at all (1.45e-8 relative was seen, and 9.2e-8 for the same inputs on another host's
    BLAS); it is floored at float32's unit roundoff 2^-24: no float32 output is expected closer to the float64 value than its own
    rounding.  td (150 numbers) and the gradients (thousands) need no floor."""
    return dict(td=np.abs(r32['td'].astype(np.float64) - r64['td']).max(), stats=max(_stats_err(r32['stats'], r64['stats']), 2.0 ** -24),
                grad=_grad_err(r32['grad'], r64['grad']))


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _as_f32(words):
    return _t(np.ascontiguousarray(words, dtype=np.int32).view(np.float32))


def _flat(v):
    return np.concatenate([np.asarray(v[k], dtype=np.float32).ravel() for k in R.ORDER])


def _trainer(cfg, w, max_rows=N_ROWS):
    from rl4rs_amd.device import DeviceRawTrainer
    return DeviceRawTrainer(cfg, w, max_rows=max_rows)


def _loss_call(tr, tv, b, double_q, weighted):
    return tr.dqn_loss_grad(_t(_flat(tv)), _as_f32(b['rec']), _t(b['act']), _t(b['rew']), _t(b['done']), _as_f32(b['next_rec']),
                            _t(b['bits']), weights=_t(b['weights']) if weighted else None, gamma=GAMMA, double_q=double_q,
                            want_next_action=True)


# ---- 1. records ------------------------------------------------------------------------------------------------------
def _special_obs(cfg, N, rs):
    cat, dense, seqs = _obs(cfg, N, rs)
    cat[0, 0] = 0                   # id 0; every id below 2^23 reads as a denormal float32
    cat[1, 0] = 1
    seqs[0][2, 0] = -1              # reads as a NaN
    cat[N - 1, -1] = 8388607
    return cat, dense, seqs


@pytest.mark.parametrize('name,N', [('floor', 70), ('R2', 5)])
def test_pack_on_the_device_equals_the_numpy_pack(name, N):
    import torch
    cfg = CFGS[name]
    w = _weights(cfg)[0]
    cat, dense, seqs = _special_obs(cfg, N, np.random.RandomState(9))
    want = R.pack_records(cfg, cat, dense, seqs)
    tr = _trainer(cfg, w, max_rows=N)
    assert tr.record_words == R.record_fields(cfg)[0] == want.shape[1]
    rec = tr.pack_records(_t(cat), _t(dense), [_t(q) for q in seqs])
    assert rec.dtype == torch.float32 and tuple(rec.shape) == want.shape
    assert np.array_equal(R.as_words(rec.cpu().numpy()), want)
    tr.close()


@pytest.mark.parametrize('name,drop', [('floor', 0), ('R2', 1)])
def test_ring_keeps_records_bit_for_bit(name, drop):
    """A rollout-shaped push (T = 3, B = 8) of records and a sample of 16: obs / next obs are the words of the rows ``idx`` names and
    of their successors.  drop = 1 cuts the last pad word off (obs_dim 11: not a multiple of 4, the ring's scalar copy path)."""
    import torch
    from rl4rs_amd.device import DeviceReplay
    cfg = CFGS[name]
    T, B, A = 3, 8, cfg['action_size']
    rs = np.random.RandomState(10)
    words = R.pack_records(cfg, *_special_obs(cfg, T * B, rs))
    words = np.ascontiguousarray(words[:, :words.shape[1] - drop])
    OD = words.shape[1]
    assert (OD % 4 == 0) == (drop == 0)
    ring = DeviceReplay(OD, A, T, B, buffer_size=10 * T * B)
    mask = np.ones((T * B, A), dtype=np.int64)
    ring.push(_as_f32(words), _t(_bits(mask)), _t(rs.randint(0, A, size=T * B).astype(np.int32)), _t(rs.rand(T * B)))
    s = ring.sample(16, prioritized=False, seed=3, step=1)
    idx = s['idx'].cpu().numpy()
    done = idx // B == T - 1
    assert np.array_equal(s['done'].cpu().numpy() != 0, done) and done.any() and not done.all()
    assert np.array_equal(R.as_words(s['obs'].cpu().numpy()), words[idx])
    assert np.array_equal(R.as_words(s['next_obs'].cpu().numpy()), words[np.where(done, idx, idx + B)])
    ring.close()


# ---- 2. loss and gradient --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CFGS))
def test_loss_and_gradient_against_the_restatement(name):
    cfg, w, v, tv, b, seed = _case(name)
    A, H = cfg['action_size'], cfg['category_hash_size']
    term = b['done'].astype(bool)
    cat_s, _, seqs_s = R.unpack_records(cfg, b['rec'])
    touched = dict(cat_emb=np.unique(np.clip(cat_s, 0, H - 1)), seq_emb=np.unique(np.clip(np.concatenate([q.ravel() for q in seqs_s]), 0, H - 1)))
    taken = np.unique(b['act'])
    assert b['untaken'] not in taken and np.bincount(b['act']).max() >= N_ROWS // 3
    tr = _trainer(cfg, w)
    for double_q in (True, False):
        for weighted in (False, True):
            r64, r32 = _refs(name, double_q, weighted)
            # the precondition: the reference alone stays clear of near-ties (and so its float32 run picks the same a*)
            assert r64['gap'].min() > 100.0 * _q_e32(r32, r64, b['mask']), (name, seed)
            assert np.array_equal(r32['astar'], r64['astar'])
            assert not r64['boot'][list(EMPTY_MASK_ROWS)].any()
            assert np.array_equal(r64['y'][list(EMPTY_MASK_ROWS)], b['rew'][list(EMPTY_MASK_ROWS)].astype(np.float64))
            bar = _bars(r32, r64)
            td, stats, astar = _loss_call(tr, tv, b, double_q, weighted)
            g = dict((k, x.cpu().numpy()) for k, x in tr.gradients().items())
            td, stats, astar = td.cpu().numpy(), stats.cpu().numpy(), astar.cpu().numpy()
            err = dict(td=np.abs(td.astype(np.float64) - r64['td']).max(), stats=_stats_err(stats, r64['stats']), grad=_grad_err(g, r64['grad']))
            print('%s double_q %d weighted %d seed %d: ' % (name, double_q, weighted, seed) +
                  '  '.join('%s device %.3g e32 %.3g (share of the bar %.2f)' % (k, err[k], bar[k], err[k] / (MARGIN * bar[k])) for k in sorted(err)))
            assert np.isfinite(td).all() and np.isfinite(stats).all() and all(np.isfinite(x).all() for x in g.values())
            assert (astar[term] == -1).all() and np.array_equal(astar[~term], r64['astar'][~term])
            for k in sorted(err):
                assert err[k] <= MARGIN * bar[k], (name, double_q, weighted, k, err[k], bar[k])
            # exact zeros: the value column, the action columns nobody took, the table rows no id touched
            idle = np.setdiff1d(np.arange(A + 1), taken)
            assert A in idle and b['untaken'] in idle
            assert (g['head_w'][:, idle] == 0).all() and (g['head_b'][idle] == 0).all()
            assert (g['head_w'][:, taken] != 0).any(axis=0).all()
            for k in R.TABLES:
                rest = np.setdiff1d(np.arange(H), touched[k])
                assert rest.size > 0 and (g[k][rest] == 0).all()
    tr.close()


# ---- 3. reproducibility ----------------------------------------------------------------------------------------------
def test_two_calls_are_bit_identical_but_for_the_tables():
    import torch
    name = 'R1'
    cfg, w, v, tv, b, seed = _case(name)
    r64, r32 = _refs(name, True, True)
    bar = _bars(r32, r64)['grad']
    tr = _trainer(cfg, w)
    runs = []
    for _ in range(2):
        td, stats, astar = _loss_call(tr, tv, b, True, True)
        runs.append((td.clone(), stats.clone(), astar.clone(), tr.gradients()))
    (td0, st0, a0, g0), (td1, st1, a1, g1) = runs
    assert torch.equal(td0, td1) and torch.equal(st0, st1) and torch.equal(a0, a1)
    for k in R.ORDER:
        if k in R.TABLES:
            d = (g0[k] - g1[k]).abs().max().item() / max(g0[k].abs().max().item(), 1e-8)
            print('%s: run-to-run difference %.3g of the largest entry (bar %.3g)' % (k, d, MARGIN * bar))
            assert d <= MARGIN * bar
        else:
            assert torch.equal(g0[k], g1[k]), k
    tr.close()


# ---- 4. clipped Adam -------------------------------------------------------------------------------------------------
def _adam_check(cfg, w, grad_flat):
    """One per-variable-clipped step from zero moments on ``grad_flat`` against the float64 closed form; var_clip = the median of
    the ten float64 norms, so some variables clip and some do not.  Then: a second handle takes the bit-identical step."""
    import torch
    tr, tr2 = _trainer(cfg, w, max_rows=8), _trainer(cfg, w, max_rows=8)
    for h in (tr, tr2):
        h.set_flat_gradient(grad_flat)
    g = dict((k, x.cpu().numpy().astype(np.float64)) for k, x in tr.gradients().items())
    norms = R.var_norms(g)
    clip = float(np.median(norms))
    assert (norms > clip).any() and (norms < clip).any()
    before = dict((k, x.cpu().numpy()) for k, x in tr.weights().items())
    for h in (tr, tr2):
        h.adam_step_clip_by_var(lr=1e-3, var_clip=clip)
    after = dict((k, x.cpu().numpy()) for k, x in tr.weights().items())
    want = R.adam_clip_by_var_first_step(before, g, 1e-3, clip)
    err = max(np.abs(after[k].astype(np.float64) - want[k]).max() for k in R.ORDER)
    print('clipped Adam step: %.3g from the closed form (bar 1e-6); norms %s clip %.4g' % (err, np.round(norms, 4), clip))
    assert err < 1e-6
    assert torch.equal(tr.params(), tr2.params())
    tr.close()
    tr2.close()


def test_clipped_adam_step_at_the_floor_configuration():
    import torch
    cfg, w, v, tv, b, seed = _case('floor')
    tr = _trainer(cfg, w)
    _loss_call(tr, tv, b, True, True)
    grad = tr.flat_gradient()
    tr.close()
    _adam_check(cfg, w, grad)
    # var_clip = 0 is rl4rs_rawtrain_adam_step without a clip, bit for bit
    a, c = _trainer(cfg, w, max_rows=8), _trainer(cfg, w, max_rows=8)
    for h in (a, c):
        h.set_flat_gradient(grad)
    a.adam_step_clip_by_var(lr=1e-3, var_clip=0.0)
    c.adam_step(lr=1e-3, grad_clip=0.0)
    assert torch.equal(a.params(), c.params()) and not torch.equal(a.params(), _t(_flat(v)))
    a.close()
    c.close()


def test_clipped_adam_step_when_a_variable_spans_many_tiles():
    """H = 40 000, E = 128: each table is 5.12 M elements = 312.5 tiles of 16 384, so the first boundary falls inside a tile and the
    eight small variables share the tiles behind the second table.  A dense random gradient makes every tile count."""
    import torch
    from rl4rs_amd.nets.rawpolicy import init_rawpolicy_weights
    cfg = dict(RAW_FLOOR, category_hash_size=40000)
    w = init_rawpolicy_weights(cfg, seed=2, emb_scale=0.5, head_std=1.0, bias_noise=0.2)
    n = sum(int(np.prod(x.shape)) for x in R.flat_weights(w).values())
    assert (40000 * 128) % 16384 != 0
    gen = torch.Generator(device='cuda')
    gen.manual_seed(5)
    grad = torch.randn(n, generator=gen, device='cuda', dtype=torch.float32) * 0.01
    _adam_check(cfg, w, grad)


# ---- 5. greedy -------------------------------------------------------------------------------------------------------
def test_greedy_is_the_first_maximum_under_the_mask():
    name = 'floor'
    cfg, w, v, tv, b, seed = _case(name)
    r64, r32 = _refs(name, True, False)
    live = ~b['done'].astype(bool)                              # the successors of the non-terminal rows: clean records
    cat, dense, seqs = [x[live] for x in b['next_obs'][:2]] + [[q[live] for q in b['next_obs'][2]]]
    mask, bits = b['mask'][live], b['bits'][live]
    tr = _trainer(cfg, w)
    a, q = tr.greedy(_t(cat), _t(dense), [_t(s) for s in seqs], _t(bits), want_q=True)
    a, q = a.cpu().numpy(), q.cpu().numpy()
    want_a, want_q = r64['q_sel'][live].argmax(axis=1), r64['q_sel'][live]
    empty = ~(mask > 0).any(axis=1)
    assert empty.sum() == len(EMPTY_MASK_ROWS) and (a[empty] == 0).all()
    assert np.array_equal(a, want_a)
    ok = mask > 0
    e32 = np.abs(r32['q_sel'][live].astype(np.float64)[ok] - want_q[ok]).max()
    err = np.abs(q.astype(np.float64)[ok] - want_q[ok]).max()
    print('greedy: masked Q device %.3g e32 %.3g' % (err, e32))
    assert err <= MARGIN * e32 and (q[~ok] < -1e37).all()
    a2 = tr.greedy(_t(cat), _t(dense), [_t(s) for s in seqs], _t(bits))[0].cpu().numpy()
    assert np.array_equal(a, a2)
    tr.close()


# ---- 6. trainer ------------------------------------------------------------------------------------------------------
def _env(tmp_path, B, T, **extra):
    import rl4rs_amd
    from rl4rs_amd import synth
    from rl4rs.env.slate import SlateRecEnv, SlateState
    d = str(tmp_path)
    cat_path, log_path = os.path.join(d, 'item_info.csv'), os.path.join(d, 'log.csv')
    if not os.path.exists(cat_path):
        cat_text = synth.make_catalog_text(seed=21)
        synth.write_text(cat_path, cat_text)
        synth.write_records(log_path, synth.make_records(B + 3, pages=1, seed=8, illegal_frac=0.0, hash_size=5000,
                                                         special_ids=synth.special_ids_from_text(cat_text)))
    cfg = {"maxlen": 64, "batch_size": B, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
           "category_feature_num": 21, "category_hash_size": 5000, "seq_num": 2, "emb_size": 128,
           "page_items": 9, "hidden_units": 128, "max_steps": T, "action_emb_size": 32,
           "sample_file": log_path, "iteminfo_file": cat_path, "is_eval": False, "cache_size": B, "model_seed": 3,
           "support_rllib_mask": True, "rawstate_as_obs": True, "return_tensors": True}
    cfg.update(extra)
    env = rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))
    env.seed(5)
    return env


def test_raw_dqn_trainer(tmp_path):
    import torch
    from rl4rs_amd.train import RawDQNTrainer
    B, T, M = 64, 9, 128
    env = _env(tmp_path, B, T)
    cfg = env.config
    tr = RawDQNTrainer(env, seed=1, lr=1e-3, learning_starts=0, train_batch_size=M, updates_per_rollout=2, keep_last_batch=True)
    assert tr.OD == tr.policy.record_words == 584
    w0 = tr.policy.weights()
    outs = []
    for it in range(3):
        outs.append(tr.train_iteration())
        # 576 sampled steps a call >= target_network_update_freq 200: every call ends with a target copy
        assert torch.equal(tr.target, tr.policy.params())
    assert all(np.isfinite(list(o.values())).all() for o in outs)
    assert outs[-1]['iteration'] == 3 and outs[-1]['buffer_rows'] == 3 * B * T and outs[-1]['num_updates'] == 3 * 2
    assert outs[-1]['num_target_updates'] == 3
    w1 = tr.policy.weights()
    assert not torch.equal(w0['ctx_w'], w1['ctx_w'])
    assert ((w0['cat_emb'] != w1['cat_emb']).any(dim=1).sum().item() > 0) or ((w0['seq_emb'] != w1['seq_emb']).any(dim=1).sum().item() > 0)
    # one more update by hand: its td against the restatement on the records it drew and the parameters it started from
    before, target = tr.policy.params().cpu().numpy(), tr.target.cpu().numpy()
    tr.update()
    assert not torch.equal(tr.target, tr.policy.params())
    lb = dict((k, x.cpu().numpy()) for k, x in tr.last_batch.items())
    args = (R.split_flat(before, cfg), R.split_flat(target, cfg), cfg, R.as_words(lb['obs']), lb['action'], lb['reward'], lb['done'],
            R.as_words(lb['next_obs']), R.unpack_bits(lb['next_mask'], cfg['action_size']))
    kw = dict(weights=lb['weight'], gamma=1.0, double_q=True, want_grad=False)
    r64, r32 = R.loss_and_grad(*args, **kw), R.loss_and_grad(*args, dtype=np.float32, **kw)
    bar = np.abs(r32['td'].astype(np.float64) - r64['td']).max()
    err = np.abs(lb['td'].astype(np.float64) - r64['td']).max()
    print('trainer: td of the last update device %.3g e32 %.3g' % (err, bar))
    assert err <= MARGIN * bar
    assert (lb['next_action'][lb['done'] != 0] == -1).all()
    e1, e2 = tr.evaluate(1, seed=4), tr.evaluate(1, seed=4)
    assert np.isfinite(e1) and e1 == e2
    with pytest.raises(NotImplementedError):
        tr.save(os.path.join(str(tmp_path), 'ckpt.npz'))
    with pytest.raises(NotImplementedError):
        tr.restore(os.path.join(str(tmp_path), 'ckpt.npz'))
    for kw in (dict(n_step=3), dict(softq_temperature=0.5)):
        with pytest.raises(ValueError):
            RawDQNTrainer(env, **kw)
    tr.close()
    plain = _env(tmp_path, B, T, rawstate_as_obs=False)
    with pytest.raises(AssertionError, match='rawstate_as_obs'):
        RawDQNTrainer(plain)
