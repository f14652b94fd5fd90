"""CPU: the host side of COMBO.  The float64 restatement the device is compared with (tests/combo_ref.py) has its conservative
term's gradient checked against central finite differences; rl4rs_combo_critic_loss / rl4rs_combo_update refuse an empty half, no
action samples, a null handle and a misaligned workspace with a message each and without a device; the workspace grows with the
generated half; the new symbols are exported and declared; the learner's constructor refusals; and COMBO.fit hands update the
n_real its minibatch was built with, real rows first (a stub dynamics, a stubbed update)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import combo_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('rl4rs_amlp_grad_stash', 'rl4rs_combo_critic_loss', 'rl4rs_combo_workspace_floats', 'rl4rs_combo_workspace_offset',
               'rl4rs_combo_update')


@pytest.fixture(scope='module')
def lib():
    from rl4rs_amd.build import build_lib
    build_lib()
    from rl4rs_amd import _lib
    return _lib.load()


def test_conservative_term_gradient_matches_finite_differences():
    """(D, A, H) = (5, 2, 6), 7 rows of which 3 real, n = 2, w = 1.7: the autograd gradient of the conservative term wrt every
    parameter of both critics against central differences (step and bar of test_dynamics_host.py)."""
    from rl4rs_amd.offline_rl import init_amlp_params
    D, A, H, B, n_real, n, w = 5, 2, 6, 7, 3, 2, 1.7
    F = B - n_real
    dt = torch.float64
    rs = np.random.RandomState(4)
    f = lambda *s: rs.standard_normal(s)
    obs, act, nxt = f(B, D), np.tanh(f(B, A)), f(B, D)
    noise = (f(F * n, A), f(F * n, A), rs.uniform(-1, 1, size=(F, n, A)))
    policy = R.MLP(init_amlp_params(D, 0, 2 * A, hidden1=H, hidden2=H, seed=1, heads=2), dt)
    acts, offs = R.conservative_rows(policy, obs[n_real:], nxt[n_real:], n, noise)
    assert tuple(acts.shape) == (F, 3 * n, A) and float((offs[:, 2 * n:] - A * np.log(0.5)).abs().max()) == 0.0
    base = [init_amlp_params(D, A, 1, hidden1=H, hidden2=H, seed=s) for s in (2, 3)]
    for p in base:                                   # biases off zero so that units are active on some rows and not on others
        for k in ('fc1_b', 'fc2_b', 'head_b'):
            p[k] = p[k] + 0.3 * rs.standard_normal(p[k].shape).astype(np.float32)
    keys = [(c, k) for c in range(2) for k in sorted(base[c])]
    flat0 = np.concatenate([np.asarray(base[c][k], np.float64).reshape(-1) for c, k in keys])
    y = torch.zeros(B, dtype=dt)

    def nets(flat):
        out, o = [{}, {}], 0
        for c, k in keys:
            sz = base[c][k].size
            out[c][k] = flat[o:o + sz].reshape(base[c][k].shape)
            o += sz
        return [R.MLP(p, dt) for p in out]

    def value(flat):
        return float(R.critic_terms(nets(flat), obs, act, y, n_real, acts, offs, w)['conservative'].detach())

    qs = nets(flat0)
    R.critic_terms(qs, obs, act, y, n_real, acts, offs, w)['conservative'].backward()
    analytic = np.concatenate([qs[c].grads()[k].reshape(-1) for c, k in keys])
    h, worst = 1e-6, 0.0
    for i in range(flat0.size):
        up, dn = flat0.copy(), flat0.copy()
        up[i] += h
        dn[i] -= h
        worst = max(worst, abs((value(up) - value(dn)) / (2 * h) - analytic[i]))
    # central differences of a smooth function: error O(h^2 f''') + O(eps / h) ~ 1e-9 at h = 1e-6 in float64
    assert worst < 1e-7, worst
    assert np.abs(analytic).max() > 1e-3


def test_the_restatement_weights_and_splits_the_terms():
    """doubling w doubles the conservative term and leaves TD alone; the data term sees the real rows only, the logsumexp the
    generated rows only (moving a generated row's dataset action moves TD but not the conservative term)"""
    from rl4rs_amd.offline_rl import init_amlp_params
    D, A, B, n_real, n = 5, 2, 6, 2, 2
    F, dt = B - n_real, torch.float64
    rs = np.random.RandomState(1)
    f = lambda *s: rs.standard_normal(s)
    obs, act, nxt, y = f(B, D), np.tanh(f(B, A)), f(B, D), torch.as_tensor(f(B))
    policy = R.MLP(init_amlp_params(D, 0, 2 * A, hidden1=8, hidden2=8, seed=1, heads=2), dt)
    qs = [R.MLP(init_amlp_params(D, A, 1, hidden1=8, hidden2=8, seed=s), dt) for s in (2, 3)]
    acts, offs = R.conservative_rows(policy, obs[n_real:], nxt[n_real:], n, (f(F * n, A), f(F * n, A), rs.uniform(-1, 1, size=(F, n, A))))
    val = lambda terms, k: float(terms[k].detach())
    one, two = [R.critic_terms(qs, obs, act, y, n_real, acts, offs, w) for w in (1.0, 2.0)]
    assert abs(val(two, 'conservative') - 2 * val(one, 'conservative')) < 1e-12 and val(two, 'td') == val(one, 'td')
    act2 = act.copy()
    act2[n_real:] *= 0.5
    moved = R.critic_terms(qs, obs, act2, y, n_real, acts, offs, 1.0)
    assert val(moved, 'conservative') == val(one, 'conservative') and val(moved, 'td') != val(one, 'td')


def _loss_args(n_ptr=14):
    buf = np.zeros(64, dtype=np.float32)
    return buf, [buf.ctypes.data_as(C.c_void_p)] * n_ptr


def test_critic_loss_refusals_come_before_the_device(lib):
    buf, p = _loss_args()
    call = lambda B, n_real, k, ptrs=p: (lib.rl4rs_combo_critic_loss(B, n_real, k, *ptrs), lib.rl4rs_last_error().decode())
    seen = set()
    for args, words in (((8, 0, 6), ('n_real=0', 'no real row')), ((8, 8, 6), ('n_real=8', 'no generated row')),
                        ((8, 3, 0), ('0 action samples',))):
        rc, msg = call(*args)
        assert rc == -1, (args, rc, msg)
        for w_ in words:
            assert w_ in msg, (args, msg)
        seen.add(msg)
    null_w = list(p)
    null_w[6] = None                                 # the weight scalar
    rc, msg = call(8, 3, 6, null_w)
    assert rc == -1 and 'null argument' in msg, msg
    seen.add(msg)
    half = list(p)
    half[1] = None                                   # q2 of the pass-T half while the rest of that half is given
    rc, msg = call(8, 3, 6, half)
    assert rc == -1 and 'pass-T half' in msg, msg
    seen.add(msg)
    assert len(seen) == 5                            # each its own message


def _step(lib, **kw):
    from rl4rs_amd import _lib
    buf = np.zeros(64, dtype=np.float32)
    base = buf.ctypes.data
    base += (-base) % 16
    f = dict((n, base) for n, t in _lib.ComboStep._fields_ if t is C.c_void_p)
    f.update(B=8, n_real=3, n=2, A=4, gamma=0.99, tau=0.005, actor_lr=1e-4, critic_lr=3e-4, temp_lr=1e-4, conservative_weight=1.0,
             do_actor=1, reserved=0, temp_step=0)
    f.update(kw)
    st = _lib.ComboStep(*[f[n] for n, _ in _lib.ComboStep._fields_])
    rc = lib.rl4rs_combo_update(C.byref(st), None)
    return rc, lib.rl4rs_last_error().decode(), buf


def test_update_refusals_come_before_the_device(lib):
    """every refusal returns before a handle is read or anything is launched: the handles here are not handles at all, and this
    machine may have no device"""
    seen = set()
    for kw, words in ((dict(n_real=0), ('n_real=0', 'no real row')), (dict(n_real=8), ('n_real=8 of B=8', 'no generated row')),
                      (dict(n=0), ('0 action samples',)), (dict(q2=None), ('null handle',)), (dict(policy=None), ('null handle',)),
                      (dict(metrics_dev=None), ('null argument',))):
        rc, msg, _ = _step(lib, **kw)
        assert rc == -1, (kw, rc, msg)
        for w_ in words:
            assert w_ in msg, (kw, msg)
        seen.add(msg)
    buf = np.zeros(64, dtype=np.float32)
    base = buf.ctypes.data
    base += (-base) % 16
    rc, msg, _ = _step(lib, workspace_dev=base + 4)
    assert rc == -1 and 'workspace_dev' in msg and '16-byte' in msg, msg
    seen.add(msg)
    assert len(seen) == 6                            # (the two null handles share theirs)


def test_workspace_is_positive_and_grows_with_the_generated_half(lib):
    sizes = [lib.rl4rs_combo_workspace_floats(256, n_real, 10, 32) for n_real in (255, 192, 128, 64, 1)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    # the F * 3n sample rows: actions [A], offset, two values and two gradients each
    assert sizes[2] - sizes[1] >= 64 * 30 * (32 + 5)
    for bad in ((256, 0, 10, 32), (256, 256, 10, 32), (256, 128, 0, 32), (0, 0, 10, 32)):
        assert lib.rl4rs_combo_workspace_floats(*bad) == -1 and 'bad sizes' in lib.rl4rs_last_error().decode()
    y0, s0 = [lib.rl4rs_combo_workspace_offset(256, 128, 10, 32, what) for what in (0, 1)]
    assert 0 < y0 < s0 and s0 + 6 <= sizes[2] and y0 % 4 == 0 and s0 % 4 == 0
    assert lib.rl4rs_combo_workspace_offset(256, 128, 10, 32, 2) == -1


def test_new_symbols_are_exported_bound_and_declared(lib):
    from rl4rs_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'rl4rs_hip.h')).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert re.search(r'\b%s\s*\(' % name, text), name
    # the ctypes mirror of rl4rs_combo_step has the header's fields in the header's order
    body = re.search(r'typedef struct rl4rs_combo_step \{(.*?)\} rl4rs_combo_step;', text, flags=re.S).group(1)
    names = [part.split()[-1] for decl in body.split(';') if decl.strip() for part in decl.replace('*', ' ').split(',')]
    assert names == [n for n, _ in _lib.ComboStep._fields_], names


def test_constructor_refusals_need_no_device():
    from rl4rs_amd.offline_rl import COMBO, MOPO
    assert issubclass(COMBO, MOPO)
    cfg = {'action_emb_size': 4}
    with pytest.raises(NotImplementedError, match='soft_q_backup'):
        COMBO(cfg, 10, None, soft_q_backup=True)
    with pytest.raises(ValueError, match='lam must be 0'):
        COMBO(cfg, 10, None, lam=1.0)
    with pytest.raises(ValueError, match='continuous actions only'):
        COMBO(cfg, 10, None, discrete_action=True)
    for kw in (dict(real_ratio=1.0), dict(real_ratio=0.0), dict(n_action_samples=0), dict(batch_size=1)):
        with pytest.raises(ValueError, match='both real and generated rows'):
            COMBO(cfg, 10, None, **kw)


class _StubDynamics(object):
    """next = s + 1, reward = row sum of the action, variance = 0.5; a penalty would show in the reward"""

    def __init__(self):
        self.lams = []

    def predict(self, s, a, with_variance=False, lam=None, step=0, indices=None, noise=None):
        self.lams.append(lam)
        var = torch.full((s.shape[0], 1), 0.5)
        return s + 1.0, a.sum(dim=1, keepdim=True) - (lam or 0.0) * var, var


def _stub_learner(batch, real_ratio, total_step=0):
    """a COMBO without a device: what fit touches, and nothing else"""
    from rl4rs_amd.offline_rl import COMBO, GeneratedFIFO
    c = COMBO.__new__(COMBO)
    c.device, c.A, c.batch_size, c.real_ratio = torch.device('cpu'), 2, batch, real_ratio
    c.rollout_interval, c.rollout_horizon, c.rollout_batch_size, c.lam = 4, 2, 5, None
    c.total_step, c.dynamics, c.generated = total_step, _StubDynamics(), GeneratedFIFO(1000)
    c._gen = torch.Generator().manual_seed(3)
    c.sample_action = lambda obs, eps=None: torch.full((obs.shape[0], 2), 0.25)
    c.calls = []

    def update(obs, act, rew, nxt, ter, n_real, noise=None):
        c.calls.append((n_real, obs.clone(), rew.clone(), ter.clone(), len(c.generated)))
        c.total_step += 1
        return {'critic_loss': torch.tensor(float(n_real))}

    c.update = update
    return c


@pytest.mark.parametrize('batch,ratio', [(10, 0.5), (9, 0.5), (16, 0.05), (7, 0.7)])
def test_fit_passes_the_split_of_its_minibatch_real_rows_first(batch, ratio):
    real = [torch.full((50, 3), -1.0), torch.zeros((50, 2)), torch.full((50,), 7.0), torch.zeros((50, 3)), torch.ones(50)]
    c = _stub_learner(batch, ratio, total_step=1)            # not a multiple of the interval: the rollout still precedes the first update
    out = c.fit(real, 6)
    want = int(round(ratio * batch))
    assert 0 < want < batch and len(c.calls) == 6 and out['critic_loss'] == [float(want)] * 6
    for n_real, obs, rew, ter, held in c.calls:
        assert n_real == want and obs.shape[0] == batch and held >= 10        # never an empty generated half
        assert (ter[:n_real] == 1).all() and (ter[n_real:] == 0).all()        # real rows first, then generated ones
        assert (rew[:n_real] == 7).all() and (rew[n_real:] == 0.5).all()      # a + a, no variance penalty
    assert c.dynamics.lams and all(l is None for l in c.dynamics.lams)
    assert len(c.generated) == 10 * 2                        # before update 1 (nothing generated yet) and at total_step 4


def test_fit_refuses_discrete_actions_as_mopo_does():
    real = [torch.zeros((20, 3)), torch.zeros(20, dtype=torch.int64), torch.zeros(20), torch.zeros((20, 3)), torch.zeros(20)]
    with pytest.raises(AssertionError, match='continuous actions'):
        _stub_learner(8, 0.5).fit(real, 1)
