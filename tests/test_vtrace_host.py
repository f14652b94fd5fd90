"""CPU: the float64 V-trace restatement (tests/vtrace_ref.py) against closed forms, and the argument checks of the two C entry
points, which run before anything touches a device."""
import ctypes as C

import numpy as np

import vtrace_ref as VR


def _draw(T, B, seed):
    rs = np.random.RandomState(seed)
    return dict(blp=rs.uniform(-3, -1, (T, B)), tlp=rs.uniform(-3, -1, (T, B)), V=rs.randn(T, B) * 50 + 100,
                r=rs.rand(T, B) * 100, boot=rs.randn(B) * 50 + 100)


def test_on_policy_undiscounted_is_the_reward_to_go_plus_bootstrap():
    """rho = 1, no dones, gamma 1: the deltas telescope, vs_t = sum_{k >= t} r_k + bootstrap, and pg_adv_t = vs_t - V_t."""
    d = _draw(7, 5, 0)
    o = VR.vtrace(d['blp'], d['blp'], d['V'], d['r'], d['boot'], None, 1.0, 1.0, 1.0)
    togo = np.cumsum(d['r'][::-1], axis=0)[::-1] + d['boot'][None]
    assert np.abs(o['vs'] - togo).max() < 1e-10
    assert np.abs(o['pg_adv'] - (togo - d['V'])).max() < 1e-10
    assert np.array_equal(o['rho'], np.ones((7, 5)))
    # without a bootstrap it is the plain reward-to-go
    o0 = VR.vtrace(d['blp'], d['blp'], d['V'], d['r'], None, None, 1.0, 1.0, 1.0)
    assert np.abs(o0['vs'] - (togo - d['boot'][None])).max() < 1e-10


def test_a_done_cuts_the_scan():
    """done at step t: vs and pg_adv of steps <= t do not depend on anything after t (values, rewards, weights, bootstrap)."""
    T, B, t_done = 9, 4, 4
    d, e = _draw(T, B, 1), _draw(T, B, 2)
    dones = np.zeros((T, B), dtype=np.int32)
    dones[t_done, :3] = 1                                    # column 3 has no done: it must change
    a = VR.vtrace(d['blp'], d['tlp'], d['V'], d['r'], d['boot'], dones, 0.9, 1.0, 0.7)
    mix = dict((k, np.concatenate([d[k][:t_done + 1], e[k][t_done + 1:]])) for k in ('blp', 'tlp', 'V', 'r'))
    b = VR.vtrace(mix['blp'], mix['tlp'], mix['V'], mix['r'], e['boot'], dones, 0.9, 1.0, 0.7)
    for k in ('vs', 'pg_adv'):
        assert np.array_equal(a[k][:t_done + 1, :3], b[k][:t_done + 1, :3]), k
        assert not np.array_equal(a[k][:t_done + 1, 3], b[k][:t_done + 1, 3]), k
    # at the done step itself the target is the reward alone
    rho = np.exp(d['tlp'][t_done] - d['blp'][t_done])
    want = d['V'][t_done] + np.minimum(1.0, rho) * (d['r'][t_done] - d['V'][t_done])
    assert np.abs(a['vs'][t_done, :3] - want[:3]).max() < 1e-10


def test_clip_rho_zero_leaves_the_values():
    d = _draw(6, 3, 3)
    o = VR.vtrace(d['blp'], d['tlp'], d['V'], d['r'], d['boot'], None, 0.9, 0.0, 0.7)
    assert np.array_equal(o['vs'], d['V'])
    # pg_adv then bootstraps from the untouched values
    rho = np.exp(d['tlp'] - d['blp'])
    nxt = np.concatenate([d['V'][1:], d['boot'][None]])
    g = float(np.float32(0.9))
    assert np.abs(o['pg_adv'] - np.minimum(float(np.float32(0.7)), rho) * (d['r'] + g * nxt - d['V'])).max() < 1e-10


def test_the_two_thresholds_are_not_interchangeable():
    d = _draw(5, 6, 4)
    a = VR.vtrace(d['blp'], d['tlp'], d['V'], d['r'], d['boot'], None, 1.0, 1.0, 0.7)
    b = VR.vtrace(d['blp'], d['tlp'], d['V'], d['r'], d['boot'], None, 1.0, 0.7, 1.0)
    assert not np.allclose(a['vs'], b['vs']) and not np.allclose(a['pg_adv'], b['pg_adv'])


def test_rollouts_drop_last_uses_the_last_value_and_nothing_else_of_that_step():
    R, T, B = 2, 4, 3
    rs = np.random.RandomState(5)
    N = R * T * B
    blp, tlp, V, r = rs.uniform(-3, -1, N), rs.uniform(-3, -1, N), rs.randn(N) * 50, rs.rand(N) * 100
    vs, pg = VR.vtrace_rollouts(R, T, B, blp, tlp, V, r, None, 1.0, 1.0, 1.0, drop_last=True)
    rows = VR.kept_rows(R, T, B, True)
    assert len(rows) == R * (T - 1) * B
    dropped = np.setdiff1d(np.arange(N), rows)
    assert np.array_equal(dropped, np.concatenate([np.arange(3 * B, 4 * B), np.arange(7 * B, 8 * B)]))
    assert not vs[dropped].any() and not pg[dropped].any()
    blp2, tlp2, r2 = blp.copy(), tlp.copy(), r.copy()
    blp2[dropped], tlp2[dropped], r2[dropped] = -9.0, -0.5, 1e6
    vs2, pg2 = VR.vtrace_rollouts(R, T, B, blp2, tlp2, V, r2, None, 1.0, 1.0, 1.0, drop_last=True)
    assert np.array_equal(vs, vs2) and np.array_equal(pg, pg2)
    V2 = V.copy()
    V2[dropped] += 1.0
    assert not np.array_equal(vs, VR.vtrace_rollouts(R, T, B, blp, tlp, V2, r, None, 1.0, 1.0, 1.0, drop_last=True)[0])
    # all T steps: the kept rows are every row, the bootstrap is zero
    vs_all, _ = VR.vtrace_rollouts(R, T, B, blp, blp, V, r, None, 1.0, 1.0, 1.0, drop_last=False)
    togo = np.cumsum(r.reshape(R, T, B)[:, ::-1], axis=1)[:, ::-1].reshape(-1)
    assert np.abs(vs_all - togo).max() < 1e-10
    assert np.array_equal(VR.kept_rows(R, T, B, False), np.arange(N))


def test_entry_points_refuse_bad_arguments():
    """RL4RS_REQUIRE runs before any launch: both calls return RL4RS_EINVAL (-1) with a message, no device needed."""
    from rl4rs_amd.build import build_lib
    build_lib()
    from rl4rs_amd import _lib
    lib = _lib.load()
    buf = np.zeros(16, dtype=np.float64)
    p = C.c_void_p(buf.ctypes.data)
    null = C.c_void_p(0)

    def vt(T, B, blp=p, tlp=p, val=p, rew=p, vs=p, pg=p):
        rc = lib.rl4rs_vtrace(T, B, blp, tlp, val, null, rew, null, 1.0, 1.0, 1.0, vs, pg, null, null)
        return rc, lib.rl4rs_last_error().decode()

    for T, B in ((0, 4), (4, 0), (-1, 4)):
        rc, msg = vt(T, B)
        assert rc == -1 and 'vtrace' in msg, (T, B, rc, msg)
    for name in ('blp', 'tlp', 'val', 'rew', 'vs', 'pg'):
        rc, msg = vt(2, 2, **{name: null})
        assert rc == -1 and 'null' in msg, (name, rc, msg)
    rc = lib.rl4rs_policy_vtrace_loss_grad(null, 1, 2, 2, p, null, p, p, p, null, 1.0, 1.0, 1.0, 1, 0.5, 0.01, p, null, null, null, null, null)
    assert rc == -1 and 'null' in lib.rl4rs_last_error().decode()
