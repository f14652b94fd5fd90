"""The float64 restatement of the raw-state DQN (tests/rawdqn_ref.py) checked on the host: its autograd gradient against central
differences, the terminal-row and empty-mask rules, the record layout, and the C header's declarations."""
import os
import re

import numpy as np
import pytest

import rawdqn_ref as R
from test_gpu_policy_shapes import RAW_CFGS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(cfg, N, seed):
    """A small minibatch at ``cfg``: online / target variables, records of s and s', actions, rewards, dones, next mask, weights."""
    from rl4rs_amd.nets.rawpolicy import init_rawpolicy_weights
    rs = np.random.RandomState(seed)
    H, A = cfg['category_hash_size'], cfg['action_size']
    w = init_rawpolicy_weights(cfg, seed=2, emb_scale=0.5, head_std=1.0, bias_noise=0.2)
    v = R.flat_weights(w)
    tv = dict((k, x + (rs.randn(*x.shape) * 0.05).astype(np.float32)) for k, x in v.items())

    def obs():
        cat = rs.randint(0, H, size=(N, cfg['category_feature_num'])).astype(np.int32)
        dense = np.abs(rs.randn(N, cfg['dense_feature_num']) * 2).astype(np.float32)
        seqs = [rs.randint(0, H, size=(N, cfg['maxlen'])).astype(np.int32) for _ in range(cfg['seq_num'])]
        return R.pack_records(cfg, cat, dense, seqs)
    rec, nrec = obs(), obs()
    mask = (rs.rand(N, A) < 0.6).astype(np.float64)
    mask[np.arange(N), rs.randint(0, A, size=N)] = 1.0
    return dict(v=v, tv=tv, rec=rec, next_rec=nrec, act=rs.randint(0, A, size=N), rew=(rs.rand(N) * 2).astype(np.float32),
                done=(rs.rand(N) < 0.3).astype(np.int32), next_mask=mask, weights=(0.2 + 1.8 * rs.rand(N)).astype(np.float32))


def _run(cfg, c, **kw):
    args = dict(gamma=0.97, double_q=True)
    args.update(kw)
    weights = args.pop('weights', c['weights'])
    return R.loss_and_grad(args.pop('v', c['v']), c['tv'], cfg, c['rec'], c['act'], c['rew'], c['done'], args.pop('next_rec', c['next_rec']),
                           args.pop('next_mask', c['next_mask']), weights=weights, **args)


@pytest.mark.parametrize('double_q', [True, False])
def test_gradient_against_central_differences(double_q):
    """At R2 (L = 1, S = 1, A = 2): up to 40 entries of every variable - those with the largest gradient and a few where it is
    zero - against (loss(p + h) - loss(p - h)) / 2h in float64."""
    cfg = RAW_CFGS['R2']
    c = _case(cfg, 12, seed=11)
    out = _run(cfg, c, double_q=double_q)
    assert np.abs(np.abs(out['td']) - 1.0).min() > 1e-3         # no row sits on the Huber kink
    h = 1e-6
    rs = np.random.RandomState(5)
    for name in R.ORDER:
        g = out['grad'][name]
        flat = np.abs(g).ravel()
        pick = np.unique(np.concatenate([np.argsort(-flat)[:32], rs.randint(0, flat.size, size=8)]))
        for i in pick:
            vals = []
            for sgn in (1.0, -1.0):
                v = dict(c['v'])
                p = np.array(v[name], dtype=np.float64)
                p.ravel()[i] += sgn * h
                v[name] = p
                vals.append(_run(cfg, c, v=v, double_q=double_q, want_grad=False)['loss'])
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - g.ravel()[i]) < 1e-7 + 1e-5 * abs(g.ravel()[i]), (name, i, fd, g.ravel()[i])


def test_terminal_row_ignores_its_successor():
    """A terminal row whose successor record is NaN / out-of-range ids gives the td, loss and gradient of a clean successor."""
    cfg = RAW_CFGS['R2']
    c = _case(cfg, 12, seed=12)
    c['done'][:4] = 1
    clean = _run(cfg, c)
    bad = c['next_rec'].copy()
    _, f = R.record_fields(cfg)
    o, n = f['dense']
    bad[:4, o:o + n] = np.array([np.nan], dtype=np.float32).view(np.int32)[0]
    o, n = f['cat']
    bad[:4, o:o + n] = cfg['category_hash_size'] + 7
    o, n = f['seq0']
    bad[:4, o:o + n] = -3
    out = _run(cfg, c, next_rec=bad)
    assert np.isfinite(out['td']).all() and np.isfinite(out['loss'])
    assert np.array_equal(out['td'], clean['td']) and out['loss'] == clean['loss']
    assert (out['astar'][:4] == -1).all()
    for k in R.ORDER:
        assert np.isfinite(out['grad'][k]).all() and np.array_equal(out['grad'][k], clean['grad'][k])


def test_empty_next_mask_bootstraps_nothing():
    """A non-terminal row whose successor allows no action gets y = r."""
    cfg = RAW_CFGS['R2']
    c = _case(cfg, 12, seed=13)
    c['done'][:] = 0
    c['next_mask'][:3] = 0.0
    out = _run(cfg, c)
    assert not out['boot'][:3].any() and out['boot'][3:].all()
    assert np.array_equal(out['y'][:3], c['rew'][:3].astype(np.float64))
    assert (np.abs(out['y'][3:] - c['rew'][3:]) > 0).all()


@pytest.mark.parametrize('name', ['floor', 'R1', 'R2', 'R3'])
def test_record_layout_round_trip(name):
    """Every field sits at the documented offset, the pad is zero, REC is a multiple of 4, and unpack gives the inputs back."""
    from test_gpu_policy_shapes import RAW_FLOOR
    cfg = RAW_FLOOR if name == 'floor' else RAW_CFGS[name]
    rs = np.random.RandomState(3)
    N, Dn, Cn, L, S = 5, cfg['dense_feature_num'], cfg['category_feature_num'], cfg['maxlen'], cfg['seq_num']
    cat = rs.randint(-2, 1 << 20, size=(N, Cn)).astype(np.int32)
    dense = rs.randn(N, Dn).astype(np.float32)
    seqs = [rs.randint(0, 1 << 20, size=(N, L)).astype(np.int32) for _ in range(S)]
    REC, f = R.record_fields(cfg)
    assert REC % 4 == 0 and 0 <= REC - (Dn + Cn + S * L) < 4
    if name == 'floor':
        assert REC == 584
    if name == 'R2':
        assert REC == 12
    rec = R.pack_records(cfg, cat, dense, seqs)
    assert rec.shape == (N, REC) and rec.dtype == np.int32
    assert np.array_equal(rec[:, :Dn], dense.view(np.int32))
    assert np.array_equal(rec[:, Dn:Dn + Cn], cat)
    for s in range(S):
        assert np.array_equal(rec[:, Dn + Cn + s * L:Dn + Cn + (s + 1) * L], seqs[s])
    assert (rec[:, Dn + Cn + S * L:] == 0).all()
    c2, d2, s2 = R.unpack_records(cfg, rec)
    assert np.array_equal(c2, cat) and np.array_equal(d2.view(np.int32), dense.view(np.int32))
    assert all(np.array_equal(a, b) for a, b in zip(s2, seqs))


def test_header_declares_the_new_entry_points():
    with open(os.path.join(REPO, 'include', 'rl4rs_hip.h')) as fh:
        text = fh.read()
    for sym in ('rl4rs_rawstate_record_words', 'rl4rs_rawstate_pack', 'rl4rs_rawtrain_dqn_loss_grad', 'rl4rs_rawtrain_greedy',
                'rl4rs_rawtrain_adam_step_clip_by_var'):
        assert re.search(r'\b(int|int32_t)\s+%s\s*\(' % sym, text), sym
    from rl4rs_amd import _lib
    for sym in ('rl4rs_rawstate_record_words', 'rl4rs_rawstate_pack', 'rl4rs_rawtrain_dqn_loss_grad', 'rl4rs_rawtrain_greedy',
                'rl4rs_rawtrain_adam_step_clip_by_var'):
        assert sym in _lib.SIGNATURES, sym
