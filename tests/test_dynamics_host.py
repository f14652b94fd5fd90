"""CPU: the restatement the dynamics kernels are checked against (tests/dynamics_ref.py) is itself checked - its autograd
gradient against central finite differences - together with the host-side pieces of the feature: the min-max scaler, MOPO's FIFO
and minibatch split (driven by a stub dynamics object), rl4rs_dyn_create's refusals through the built library, and the
discrete-action refusal."""
import ctypes as C

import numpy as np
import pytest
import torch

import dynamics_ref as R


@pytest.fixture(scope='module')
def lib():
    from rl4rs_amd.build import build_lib
    build_lib()
    from rl4rs_amd import _lib
    return _lib.load()


def test_restatement_gradient_matches_finite_differences():
    """2 members, (D, E, H1, H2) = (5, 2, 6, 4), 7 rows, training-mode batch norm and dropout, scalers on.  u and v are held (no power
    iteration): with them constant sigma = u^T W v is what the analytic backward differentiates, and a finite difference sees the
    same function."""
    from rl4rs_amd import dynamics as dyn
    D, E, H1, H2, M, B = 5, 2, 6, 4, 2, 7
    case = R.make_case(D, E, H1, H2, M, B, seed=3)
    cfg = R.default_cfg(power_iter=False, seed=5, step=2)
    dt = torch.float64
    shapes = dyn.param_shapes(D, E, H1, H2)

    def total(flat):
        P = dyn.unflatten(flat, shapes, M)
        outs, Pt, xa = R.forward(P, case['S'], case['x'], case['a'], True, cfg, dt, case['sc'])
        nxt_s, rew_s = R.scale_obs(case['nxt'], case['sc'], dt), R.scale_rew(case['rew'], case['sc'], dt)
        mask = torch.as_tensor(case['mask'], dtype=dt)
        return float(sum(R.member_loss(o, xa, nxt_s, rew_s, mask[m], p) for m, (o, p) in enumerate(zip(outs, Pt))))

    flat = R.flat_params(case).astype(np.float64)
    ref = R.loss_grad(case['P'], case['S'], case['x'], case['a'], case['nxt'], case['rew'], case['mask'], cfg, dt, case['sc'])
    R.check_conditions(ref['outs'])
    assert case['mask'].sum(axis=1).min() >= 1
    analytic = np.concatenate([np.asarray(g[name], np.float64).reshape(-1) for g in ref['grads'] for name, _ in shapes])
    assert abs(total(flat) - ref['loss'].sum()) < 1e-12
    h = 1e-6
    worst = 0.0
    for i in range(flat.size):
        up, dn = flat.copy(), flat.copy()
        up[i] += h
        dn[i] -= h
        fd = (total(up) - total(dn)) / (2 * h)
        worst = max(worst, abs(fd - analytic[i]))
    # central differences of a smooth function: error O(h^2 f''') + O(eps / h) ~ 1e-9 at h = 1e-6 in float64
    assert worst < 1e-7, worst
    assert np.abs(analytic).max() > 1e-3


def test_keep_mask_rate_and_determinism():
    k = R.keep_mask(3, 4, 1, 0, 400, 300, 0.2)
    assert abs(k.mean() - 0.8) < 0.01
    assert (k == R.keep_mask(3, 4, 1, 0, 400, 300, 0.2)).all() and (k != R.keep_mask(3, 4, 1, 1, 400, 300, 0.2)).any()


def test_min_max_scaler_round_trip_and_constant_column():
    from rl4rs_amd.dynamics import MinMaxScaler
    rs = np.random.RandomState(0)
    x = rs.standard_normal((50, 6)).astype(np.float32)
    x[:, 2] = 1.25                                   # a constant column
    sc = MinMaxScaler(x)
    t = torch.from_numpy(x)
    y = sc.transform(t)
    assert float(y.min()) == 0.0 and float(y.max()) == 1.0
    assert (y[:, 2] == 0).all()                      # max == min maps to 0, nothing divides by zero
    assert torch.isfinite(y).all()
    back = sc.reverse_transform(y)
    assert (back[:, 2] == 1.25).all()
    assert float((back - t).abs().max()) < 4 * 2.0 ** -23 * float(t.abs().max() + sc.range.max())
    # the restatement's scaling is the same function
    ref = R.scale_obs(x, dict(obs_min=sc.min.numpy(), obs_range=sc.range.numpy()), torch.float32)
    assert torch.equal(ref, y)


class _StubDynamics(object):
    """next = s + 1, reward = row sum of the action, variance = 0.5 (penalised with lam like the real one)"""

    def __init__(self):
        self.calls = []

    def predict(self, s, a, with_variance=False, lam=None, step=0, indices=None, noise=None):
        self.calls.append((s.shape[0], step))
        var = torch.full((s.shape[0], 1), 0.5)
        r = a.sum(dim=1, keepdim=True) - (lam or 0.0) * var
        return s + 1.0, r, var


def test_fifo_eviction_order_and_growth():
    from rl4rs_amd.offline_rl import GeneratedFIFO
    f = GeneratedFIFO(10)

    def rows(lo, n):
        v = torch.arange(lo, lo + n, dtype=torch.float32)
        return v[:, None].repeat(1, 3), v[:, None].repeat(1, 2), v, v[:, None].repeat(1, 3) + 0.5, torch.zeros(n)

    f.append(*rows(0, 4))
    assert len(f) == 4 and f.cols[0].shape[0] == 4          # sized to what was generated
    f.append(*rows(4, 4))
    assert len(f) == 8 and f.cols[0].shape[0] <= 10
    f.append(*rows(8, 5))                                   # 13 rows through a buffer of 10: rows 0, 1, 2 are gone
    assert len(f) == 10 and f.cols[0].shape[0] == 10
    got = f.oldest_first()
    assert got[2].tolist() == [float(i) for i in range(3, 13)]
    assert got[0][:, 0].tolist() == got[2].tolist() and (got[3][:, 0] - 0.5).tolist() == got[2].tolist()
    f.append(*rows(13, 25))                                 # more than maxlen at once: the newest 10 stay
    assert f.oldest_first()[2].tolist() == [float(i) for i in range(28, 38)]
    f.append(*rows(38, 3))
    assert f.oldest_first()[2].tolist() == [float(i) for i in range(31, 41)]


def test_rollout_and_minibatch_split_with_a_stub_dynamics():
    from rl4rs_amd.offline_rl import GeneratedFIFO, mixed_minibatch, model_rollout
    dyn = _StubDynamics()
    fifo = GeneratedFIFO(1000)
    start = torch.zeros((6, 3))
    end = model_rollout(lambda s, h: torch.full((s.shape[0], 2), float(h)), dyn, start, horizon=4, lam=2.0, fifo=fifo, step0=7)
    assert dyn.calls == [(6, 7), (6, 8), (6, 9), (6, 10)]
    assert len(fifo) == 24 and (end == 4.0).all()
    obs, act, rew, nxt, ter = fifo.oldest_first()
    for h in range(4):
        sl = slice(6 * h, 6 * h + 6)
        assert (obs[sl] == h).all() and (nxt[sl] == h + 1).all() and (act[sl] == h).all() and (ter[sl] == 0).all()
        assert (rew[sl] == 2.0 * h - 2.0 * 0.5).all()            # r - lam * variance
    real = [torch.full((50, 3), -1.0), torch.zeros((50, 2)), torch.zeros(50), torch.zeros((50, 3)), torch.ones(50)]
    gen = torch.Generator().manual_seed(1)
    for batch, ratio, want in ((100, 0.05, 5), (256, 0.05, 13), (10, 0.5, 5), (8, 0.0, 0), (8, 1.0, 8)):
        rows, n_real = mixed_minibatch(real, fifo, batch, ratio, gen)
        assert n_real == want == int(round(ratio * batch))
        assert all(t.shape[0] == batch for t in rows)
        assert (rows[0][:n_real] == -1).all() and (rows[0][n_real:] >= 0).all()       # real rows first, the rest generated
        assert (rows[4][:n_real] == 1).all() and (rows[4][n_real:] == 0).all()
    a, _ = mixed_minibatch(real, fifo, 64, 0.05, torch.Generator().manual_seed(9))
    b, _ = mixed_minibatch(real, fifo, 64, 0.05, torch.Generator().manual_seed(9))
    assert all(torch.equal(x, y) for x, y in zip(a, b))                                # a seeded generator decides
    rows, n_real = mixed_minibatch(real, GeneratedFIFO(10), 16, 0.05, gen)               # nothing generated yet: all real
    assert n_real == 16 and (rows[0] == -1).all()


def test_create_refusals_come_before_the_device(lib):
    from rl4rs_amd import _lib
    dummy = np.zeros(4, dtype=np.float32)
    p = dummy.ctypes.data_as(C.c_void_p)

    def create(**kw):
        f = dict(obs_dim=266, act_dim=32, hidden1=256, hidden2=128, members=5, max_rows=4096, max_grad_rows=512, use_batch_norm=1,
                 use_dense=1, spectral_norm=1, dropout_rate=0.2)
        f.update(kw)
        cfg = _lib.DynCfg(*[f[n] for n, _ in _lib.DynCfg._fields_])
        h = C.c_void_p()
        rc = lib.rl4rs_dyn_create(C.byref(cfg), p, p, None, C.byref(h))
        return rc, lib.rl4rs_last_error().decode(), h, lib.rl4rs_dyn_param_count(C.byref(cfg))

    # the widest scratch array of the default shape is [5, max_rows, 534] floats = 10680 bytes per row: 201075 rows stay under 2^31
    for kw, words in ((dict(max_rows=201076), ('max_rows', '2^31', '201075')), (dict(members=17), ('n_ensembles', '16')),
                      (dict(members=0), ('n_ensembles',)), (dict(act_dim=0), ('continuous',)), (dict(dropout_rate=1.0), ('dropout',)),
                      (dict(obs_dim=20000, max_rows=16, max_grad_rows=16), ('LDS', '163840')), (dict(max_grad_rows=5000), ('max_grad_rows',)),
                      (dict(hidden1=70000), ('hidden_units',))):
        rc, msg, h, n = create(**kw)
        assert rc == -1 and not h.value and n == -1, (kw, rc, msg)
        for w in words:
            assert w in msg, (kw, msg)
    per_member = 298 * 256 + 3 * 256 + (256 + 298) * 128 + 3 * 128 + 128 * 534 + 534 + 2 * 267
    cfg = _lib.DynCfg(266, 32, 256, 128, 5, 201075, 512, 1, 1, 1, 0.2)
    assert lib.rl4rs_dyn_param_count(C.byref(cfg)) == 5 * per_member
    if lib.rl4rs_device_count() <= 0:
        # the bound itself is admitted: the call gets as far as the device check (with a device it would go on to allocate)
        rc, msg, h, n = create(max_rows=201075)
        assert rc == -2 and 'no HIP device' in msg, (rc, msg)


def test_discrete_action_is_refused():
    from rl4rs_amd.dynamics import ProbabilisticEnsembleDynamics
    with pytest.raises(ValueError, match='continuous actions only'):
        ProbabilisticEnsembleDynamics({'action_emb_size': 32}, 266, discrete_action=True)
    with pytest.raises(ValueError, match='variance_type'):
        ProbabilisticEnsembleDynamics({'action_emb_size': 32}, 266, variance_type='mean')
