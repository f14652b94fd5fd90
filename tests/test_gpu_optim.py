"""GPU: every trainable handle's Adam step, optimiser-state round trip and parameter copy against a NumPy model that evaluates the
kernels' float32 expressions in the kernels' order, with the host's bias correction in float64 and then the cast to float32.

The build forbids contraction and sqrtf / division are correctly rounded, so the model is expected to give the device's bits:
every comparison is exact equality (ULP bound 0).  Measured on an MI355X with the library of the commit before the optimiser code
moved into csrc/optim.hpp, and with the library after it: 0 ULP in all 39 comparisons, both times.  Uses the public wrappers and
the rl4rs_X_params pointers only, so it does not depend on where that code lives."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
LR, B1, B2, EPS = 3e-3, 0.9, 0.98, 1e-7       # none of them a wrapper default
STEP0 = 7                                      # the state starts here: the bias correction is not the trivial first one


# ---------------------------------------------------------------------------------------------------------------- the NumPy model
def _f(x):
    """a Python float as the library receives it: rounded to float32, then widened"""
    return float(F(x))


def _corr_tf(lr, b1, b2, t):
    """tf.train.AdamOptimizer: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t)"""
    return F(_f(lr) * math.sqrt(1.0 - math.pow(_f(b2), float(t))) / (1.0 - math.pow(_f(b1), float(t))))


def _corr_torch(lr, b1, b2, eps, t):
    """torch.optim.Adam in the TF kernel: (lr_t, eps c2)"""
    c2 = math.sqrt(1.0 - math.pow(_f(b2), float(t)))
    return F(_f(lr) * c2 / (1.0 - math.pow(_f(b1), float(t)))), F(_f(eps) * c2)


def _corr_div(lr, b1, b2, t):
    """torch.optim.Adam, division form: (step_size, 1 / sqrt(1 - b2^t))"""
    return F(_f(lr) / (1.0 - math.pow(_f(b1), float(t)))), F(1.0 / math.sqrt(1.0 - math.pow(_f(b2), float(t))))


def _sumsq(g):
    """k_sumsq / k_sumsq_vars: thread t adds g[t], g[t + 256], ... in order, then the 256 partials meet in a halving tree"""
    sq = np.zeros((len(g) + 255) // 256 * 256, F)
    sq[:len(g)] = g * g
    s = np.zeros(256, F)
    for row in sq.reshape(-1, 256):
        s = s + row
    o = 128
    while o:
        s[:o] = s[:o] + s[o:2 * o]
        o //= 2
    return s[0]


def _moments(m, v, g, b1, b2):
    b1, b2 = F(b1), F(b2)
    return b1 * m + (F(1) - b1) * g, b2 * v + (F(1) - b2) * g * g


def _adam_tf(p, m, v, g, lr_t, b1, b2, eps, clip=0.0, segs=None):
    """k_adam / k_adam_vars; ``segs``: the variables' end offsets (clip by each variable's own norm), None: one global norm"""
    g = g.copy()
    if clip > 0.0:
        lo = 0
        for hi in (segs if segs is not None else [len(g)]):
            norm = np.sqrt(_sumsq(g[lo:hi]))
            if norm > F(clip):
                g[lo:hi] = g[lo:hi] * (F(clip) / norm)
            lo = hi
    mi, vi = _moments(m, v, g, b1, b2)
    return p - lr_t * mi / (np.sqrt(vi) + F(eps)), mi, vi


def _adam_div(p, m, v, g, step_size, inv_sqrt_bc2, b1, b2, eps):
    """k_adam_div"""
    mi, vi = _moments(m, v, g, b1, b2)
    return p - step_size * (mi / (np.sqrt(vi) * inv_sqrt_bc2 + F(eps))), mi, vi


# ------------------------------------------------------------------------------------------------------------------------ helpers
def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _np(t):
    return t.cpu().numpy()


def _state(n, seed):
    """seeded parameters, first moment, (positive) second moment"""
    rs = np.random.RandomState(seed)
    return rs.randn(n).astype(F), (0.1 * rs.randn(n)).astype(F), np.square(0.1 * rs.randn(n)).astype(F)


def _grads(n, seed, scales=(1.0, 0.01)):
    rs = np.random.RandomState(seed + 1000)
    return [(s * rs.randn(n)).astype(F) for s in scales]


def _ulp(a, b):
    """largest distance in float32 roundings (same-sign finite values)"""
    assert a.dtype == F and b.dtype == F and a.shape == b.shape
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


def _same(tag, got, want, bound=0):
    """got = (params, m, v, step) of the device, want of the model"""
    for name, a, b in zip(('params', 'm', 'v'), got[:3], want[:3]):
        u = _ulp(a, b)
        print('%s %s: %d ULP' % (tag, name, u))
        assert u <= bound, (tag, name, u)
    assert got[3] == want[3], (tag, got[3], want[3])


def _write_grad(net, prefix, g):
    """the handle's own gradient buffer <- g, through the rl4rs_X_params pointers"""
    import torch
    from rl4rs_amd._lib import check
    from rl4rs_amd.device import _ptr, _stream
    p, gp, n = C.c_void_p(), C.c_void_p(), C.c_int64()
    check(getattr(net.lib, prefix + '_params')(net.h, C.byref(p), C.byref(gp), C.byref(n)))
    assert n.value == len(g)
    src = _cuda(g)
    check(net.lib.rl4rs_copy_d2d(gp, _ptr(src), n.value * 4, _stream()))
    torch.cuda.synchronize()


def _round_trip(net, get, put):
    """put(get()) and set_adam_state(*adam_state()) keep every bit"""
    import torch
    p0 = get().clone()
    m0, v0, t0 = net.adam_state()
    put(p0.clone())
    net.set_adam_state(m0.clone(), v0.clone(), t0)
    torch.cuda.synchronize()
    m1, v1, t1 = net.adam_state()
    assert torch.equal(get(), p0) and torch.equal(m1, m0) and torch.equal(v1, v0) and t1 == t0


# ------------------------------------------------------------------------------------------------------------------------- policy
OD, HID, A = 256, 64, 284


def _policy(seed):
    from rl4rs_amd.device import DevicePolicy
    pol = DevicePolicy(OD, HID, A, max_rows=8)
    p, m, v = _state(pol.n_params, seed)
    pol.set_params(_cuda(p))
    pol.set_adam_state(_cuda(m), _cuda(v), STEP0)
    return pol, p, m, v


def _policy_got(pol):
    m, v, t = pol.adam_state()
    return _np(pol.params()), _np(m), _np(v), t


@pytest.mark.parametrize('clip', [0.0, 4.0])
def test_policy_adam_step(clip):
    pol, p, m, v = _policy(1)
    grads = _grads(pol.n_params, 1)
    norms = [float(np.sqrt(_sumsq(g))) for g in grads]
    assert norms[0] > 4.0 > norms[1], norms                    # one gradient above the clip, one below
    for k, g in enumerate(grads):
        pol.adam_step(_cuda(g), lr=LR, beta1=B1, beta2=B2, eps=EPS, grad_clip=clip)
        p, m, v = _adam_tf(p, m, v, g, _corr_tf(LR, B1, B2, STEP0 + k + 1), B1, B2, EPS, clip)
    _same('policy clip=%g' % clip, _policy_got(pol), (p, m, v, STEP0 + 2))
    _round_trip(pol, pol.params, pol.set_params)


def test_policy_adam_step_clip_by_var():
    pol, p, m, v = _policy(2)
    ends = np.cumsum([OD * HID, HID, HID * (A + 1), A + 1])
    for k, scales in enumerate([(1.0, 0.01, 0.5, 0.02), (0.001, 2.0, 0.3, 0.001)]):
        g = _grads(pol.n_params, 2 + k, (1.0,))[0]
        lo, active = 0, []
        for hi, s in zip(ends, scales):
            g[lo:hi] *= F(s)
            active.append(np.sqrt(_sumsq(g[lo:hi])) > 4.0)
            lo = hi
        assert any(active) and not all(active), active         # variables on either side of the clip
        pol.adam_step_clip_by_var(_cuda(g), lr=LR, beta1=B1, beta2=B2, eps=EPS, var_clip=4.0)
        p, m, v = _adam_tf(p, m, v, g, _corr_tf(LR, B1, B2, STEP0 + k + 1), B1, B2, EPS, 4.0, ends)
    _same('policy clip_by_var', _policy_got(pol), (p, m, v, STEP0 + 2))


def test_policy_copy_params_from():
    import torch
    a, b = _policy(3)[0], _policy(4)[0]
    assert not torch.equal(a.params(), b.params())
    b.copy_params_from(a)
    assert torch.equal(a.params(), b.params())


# ------------------------------------------------------------------------------------------------------------------------- dist-Q
def test_distq_adam_step_clip_by_var():
    import torch
    from rl4rs_amd.device import DeviceDistQ
    from rl4rs_amd.nets import distq
    od, na, atoms = 256, 50, 5                                  # dueling: 12 variables, three rounds of four
    ends = np.cumsum([int(np.prod(s)) for s in distq.shapes(od, na, atoms)])
    net = DeviceDistQ(od, na, max_rows=8, num_atoms=atoms, v_min=-2.0, v_max=6.0)
    other = DeviceDistQ(od, na, max_rows=8, num_atoms=atoms, v_min=-2.0, v_max=6.0, seed=1)
    assert len(ends) == 12 and ends[-1] == net.n_params
    p, m, v = _state(net.n_params, 5)
    net.set_params(_cuda(p))
    net.set_adam_state(_cuda(m), _cuda(v), STEP0)
    for k in range(2):
        g = _grads(net.n_params, 5 + k, (1.0,))[0]
        lo, active = 0, []
        for i, hi in enumerate(ends):
            g[lo:hi] *= F(0.01 if (i + k) % 2 else 1.0)
            active.append(np.sqrt(_sumsq(g[lo:hi])) > 1.5)
            lo = hi
        assert any(active) and not all(active), active
        net.adam_step_clip_by_var(_cuda(g), lr=LR, beta1=B1, beta2=B2, eps=EPS, var_clip=1.5)
        p, m, v = _adam_tf(p, m, v, g, _corr_tf(LR, B1, B2, STEP0 + k + 1), B1, B2, EPS, 1.5, ends)
    mm, vv, t = net.adam_state()
    _same('distq', (_np(net.params()), _np(mm), _np(vv), t), (p, m, v, STEP0 + 2))
    _round_trip(net, net.params, net.set_params)
    assert not torch.equal(other.params(), net.params())
    other.copy_from(net)
    assert torch.equal(other.params(), net.params())


# ------------------------------------------------------------------------------------------------------------------- Q-net, AMLP
def _qnet(seed):
    from rl4rs_amd.device import DeviceQNet
    from rl4rs_amd.offline_rl import init_qnet_params
    return DeviceQNet(11, 7, init_qnet_params(11, 7, 0, hidden1=33, hidden2=65, seed=seed), hidden1=33, hidden2=65, max_rows=16)


def _amlp(seed):
    from rl4rs_amd.device import DeviceAMLP
    from rl4rs_amd.offline_rl import init_ddpg_params
    return DeviceAMLP(20, 5, 1, init_ddpg_params(20, 5, 1, 24, 20, seed=seed), hidden1=24, hidden2=20, max_rows=8)


def _flat_got(net):
    m, v, t = net.adam_state()
    return _np(net.flat_params()), _np(m), _np(v), t


@pytest.mark.parametrize('make', [_qnet, _amlp], ids=['qnet', 'amlp'])
def test_torch_form_adam_step(make):
    import torch
    net, other = make(1), make(2)
    assert net.n_params > 256
    p, m, v = _state(net.n_params, 7)
    net.set_flat_params(_cuda(p))
    net.set_adam_state(_cuda(m), _cuda(v), STEP0)
    for k, g in enumerate(_grads(net.n_params, 7)):
        net.set_flat_gradient(_cuda(g))
        net.adam_step(LR, beta1=B1, beta2=B2, eps=EPS)
        lr_t, eps_t = _corr_torch(LR, B1, B2, EPS, STEP0 + k + 1)
        p, m, v = _adam_tf(p, m, v, g, lr_t, B1, B2, eps_t)
    _same(make.__name__, _flat_got(net), (p, m, v, STEP0 + 2))
    _round_trip(net, net.flat_params, net.set_flat_params)
    assert not torch.equal(other.flat_params(), net.flat_params())
    other.copy_from(net)
    assert torch.equal(other.flat_params(), net.flat_params())


def test_amlp_adam_multi_with_target():
    from rl4rs_amd.device import amlp_adam_multi
    tau = 0.05
    nets, targ = [_amlp(1), _amlp(2)], _amlp(3)
    n = nets[0].n_params
    st = [_state(n, 11 + i) for i in range(2)]
    tp = _state(n, 13)[0]
    targ.set_flat_params(_cuda(tp))
    for net, (p, m, v) in zip(nets, st):
        net.set_flat_params(_cuda(p))
        net.set_adam_state(_cuda(m), _cuda(v), STEP0)
    lrs = (LR, 0.5 * LR)
    grads = [_grads(n, 11 + i) for i in range(2)]
    for k in range(2):
        for i, net in enumerate(nets):
            net.set_flat_gradient(_cuda(grads[i][k]))
        amlp_adam_multi(nets, lrs, targets=[None, targ], tau=tau, beta1=B1, beta2=B2, eps=EPS)
        for i in range(2):
            lr_t, eps_t = _corr_torch(lrs[i], B1, B2, EPS, STEP0 + k + 1)
            st[i] = _adam_tf(st[i][0], st[i][1], st[i][2], grads[i][k], lr_t, B1, B2, eps_t)
        tp = (F(1) - F(tau)) * tp + F(tau) * st[1][0]
    for i, net in enumerate(nets):
        _same('adam_multi net %d' % i, _flat_got(net), st[i] + (STEP0 + 2,))
    assert _ulp(_np(targ.flat_params()), tp) == 0
    assert targ.adam_state()[2] == 0


# ------------------------------------------------------------------------------------------------- Exact-K, its critic, dynamics
def _flatnet_got(net):
    m, v, t = net.adam_state()
    return _np(net.params()), _np(m), _np(v), t


def _exactk():
    import exactk_ref as R
    from rl4rs_amd.device import DeviceExactK
    c = R.case(3, 0.0)
    dm = c['dm']
    return DeviceExactK(c['loc'], c['special'], max_rows=4, obs_dim=dm.od, action_size=dm.A, hidden_units=dm.H, num_heads=dm.heads,
                        num_blocks=dm.blocks, vocab=dm.vocab, dropout_rate=dm.rate, params=c['flat'])


@pytest.mark.parametrize('skip', [0, 1])
def test_exactk_adam_step(skip):
    net = _exactk()
    p, m, v = _state(net.n_params, 17)
    net.set_params(_cuda(p))
    net.set_adam_state(_cuda(m), _cuda(v), STEP0)
    flag = _cuda(np.array([skip], np.int32))
    for k, g in enumerate(_grads(net.n_params, 17)):
        _write_grad(net, 'rl4rs_exactk', g)
        net.adam_step(lr=LR, beta1=B1, beta2=B2, eps=EPS, skip=flag)
        if not skip:
            p, m, v = _adam_tf(p, m, v, g, _corr_tf(LR, B1, B2, STEP0 + k + 1), B1, B2, EPS)
    # skip: nothing moves, bit for bit, and the step counter still advances
    _same('exactk skip=%d' % skip, _flatnet_got(net), (p, m, v, STEP0 + 2))
    _round_trip(net, net.params, net.set_params)


def test_exactk_adam_step_without_a_flag():
    net = _exactk()
    p, m, v = _state(net.n_params, 18)
    net.set_params(_cuda(p))
    net.set_adam_state(_cuda(m), _cuda(v), STEP0)
    g = _grads(net.n_params, 18)[0]
    _write_grad(net, 'rl4rs_exactk', g)
    net.adam_step(lr=LR, beta1=B1, beta2=B2, eps=EPS)
    _same('exactk no flag', _flatnet_got(net), _adam_tf(p, m, v, g, _corr_tf(LR, B1, B2, STEP0 + 1), B1, B2, EPS) + (STEP0 + 1,))


def test_exactk_critic_adam_step():
    from rl4rs_amd.device import DeviceExactKCritic
    net = DeviceExactKCritic(4)
    p, m, v = _state(net.n_params, 19)
    net.set_params(_cuda(p))
    net.set_adam_state(_cuda(m), _cuda(v), STEP0)
    for k, g in enumerate(_grads(net.n_params, 19)):
        _write_grad(net, 'rl4rs_exactk_critic', g)
        net.adam_step(lr=LR, beta1=B1, beta2=B2, eps=EPS)
        p, m, v = _adam_tf(p, m, v, g, _corr_tf(LR, B1, B2, STEP0 + k + 1), B1, B2, EPS)
    _same('exactk critic', _flatnet_got(net), (p, m, v, STEP0 + 2))
    _round_trip(net, net.params, net.set_params)


def test_dynamics_adam_step():
    import dynamics_ref as R
    from rl4rs_amd.device import DeviceDynamics
    D, E, H1, H2, M, B = 37, 5, 24, 12, 3, 33
    case = R.make_case(D, E, H1, H2, M, B, 12)
    net = DeviceDynamics(D, E, R.flat_params(case), R.flat_state(case), (H1, H2), M, max_rows=B, max_grad_rows=B)
    p, m, v = _state(net.n_params, 23)
    net.set_params(_cuda(p))
    net.set_adam_state(_cuda(m), _cuda(v), STEP0)
    for k, g in enumerate(_grads(net.n_params, 23)):
        _write_grad(net, 'rl4rs_dyn', g)
        net.adam_step(lr=LR, beta1=B1, beta2=B2, eps=EPS)
        step_size, inv = _corr_div(LR, B1, B2, STEP0 + k + 1)
        p, m, v = _adam_div(p, m, v, g, step_size, inv, B1, B2, EPS)
    _same('dynamics', _flatnet_got(net), (p, m, v, STEP0 + 2))
    _round_trip(net, net.params, net.set_params)
