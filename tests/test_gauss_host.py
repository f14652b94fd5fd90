"""CPU: the restatement of the Gaussian actor-critic (tests/gauss_ref.py) against torch.distributions and autograd, the flat layout
against the library's count and the initialiser, and the argument checks of the rl4rs_gpolicy_* entry points, which run before
anything touches a device."""
import ctypes as C

import numpy as np
import pytest
import torch

import gauss_ref as R


def _heads(N, E, seed):
    """head / old head [N, 2E] with log_std drawn from [-8, 3], actions a few standard deviations around the mean"""
    rs = np.random.RandomState(seed)
    mk = lambda: torch.tensor(np.concatenate([rs.randn(N, E) * 2.0, rs.uniform(-8.0, 3.0, (N, E))], axis=1))
    head, old = mk(), mk()
    a = head[:, :E] + torch.exp(head[:, E:]) * torch.tensor(rs.randn(N, E) * 1.5)
    return head, old, a


@pytest.mark.parametrize('N,E', [(64, 32), (7, 1), (33, 3), (5, 64)])
def test_distribution_matches_torch_distributions(N, E):
    head, old, a = _heads(N, E, 10 + E)
    new_d = torch.distributions.Normal(head[:, :E], torch.exp(head[:, E:]))
    old_d = torch.distributions.Normal(old[:, :E], torch.exp(old[:, E:]))
    rel = lambda x, y: (x - y).abs().max().item() / max(1.0, y.abs().max().item())
    assert rel(R.logp(head, a), new_d.log_prob(a).sum(dim=1)) < 1e-12
    assert rel(R.entropy(head), new_d.entropy().sum(dim=1)) < 1e-12
    assert rel(R.kl(old, head), torch.distributions.kl_divergence(old_d, new_d).sum(dim=1)) < 1e-12
    assert R.kl(head, head).abs().max().item() < 1e-12


@pytest.mark.parametrize('N,E', [(16, 32), (4, 1), (9, 3)])
def test_closed_form_head_derivatives_match_autograd(N, E):
    head, old, a = _heads(N, E, 20 + E)
    d_lp, d_en, d_kl = R.head_derivatives(head, a, old)
    for fn, want in ((lambda h: R.logp(h, a), d_lp), (R.entropy, d_en), (lambda h: R.kl(old, h), d_kl)):
        h = head.clone().requires_grad_(True)
        fn(h).sum().backward()
        assert (h.grad - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize('D,H,E', [(256, 256, 32), (40, 64, 3), (7, 128, 1), (3072, 256, 32), (256, 256, 64)])
def test_param_count_and_flat_layout(D, H, E):
    from rl4rs_amd import _lib
    from rl4rs_amd.nets import gausspolicy as G
    lib = _lib.load()
    n = 2 * (D * H + H + H * H + H) + H * 2 * E + 2 * E + H + 1
    assert lib.rl4rs_gpolicy_param_count(D, H, E) == n == G.param_count(D, E, H) == R.param_count(D, H, E)
    if (D, H, E) == (256, 256, 32):
        assert n == 279873
    flat = G.init_gausspolicy_params(D, E, H, seed=3)
    assert flat.dtype == np.float32 and flat.shape == (n,)
    # offsets of every array, in the documented order
    off, o = G.offsets(D, E, H), 0
    for name, shape in (('W1', (D, H)), ('b1', (H,)), ('W2', (H, H)), ('b2', (H,)), ('W3', (H, 2 * E)), ('b3', (2 * E,)),
                        ('V1', (D, H)), ('c1', (H,)), ('V2', (H, H)), ('c2', (H,)), ('V3', (H, 1)), ('c3', (1,))):
        assert off[name] == o, name
        o += int(np.prod(shape))
    assert o == n
    w, wr = G.split(flat, D, E, H), R.split(flat, D, H, E)
    for name in R.NAMES:
        assert np.array_equal(w[name], wr[name])
        if w[name].ndim == 1:
            assert not w[name].any(), name                                   # zero biases
        else:                                                                 # normc: every column has norm std
            std = 0.01 if name in ('W3', 'V3') else 1.0
            assert np.abs(np.sqrt((w[name].astype(np.float64) ** 2).sum(axis=0)) - std).max() < 1e-6 * std, name
    assert not np.array_equal(flat, G.init_gausspolicy_params(D, E, H, seed=4))


@pytest.mark.parametrize('dims', [(260, 64, 3), (515, 128, 5)], ids=lambda d: 'D%d-H%d-E%d' % d)
def test_a_forward_that_drops_the_last_staging_pass_would_show(dims):
    """k_gp_fwd stages the observation 256 columns at a time; at D = 260 and D = 515 the last pass holds 4 and 3 columns.  On the
    inputs and with the bars of tests/test_gpu_gauss_policy.py, a forward that ignores the columns from 256 on - and one that
    ignores the last pass alone - misses head and value by more than ten times their bars: the GPU test can tell."""
    import test_gpu_gauss_policy as GT
    D = dims[0]
    b = GT._base(dims)
    assert b['obs'].shape == (33, D) and D % 256 in (3, 4)
    for first_dropped in sorted({256, D - D % 256}):
        obs = b['obs'].copy()
        obs[:, first_dropped:] = 0.0
        with torch.no_grad():
            head, value = R.forward(b['flat'], obs, dims)
        for k, got in (('head', head), ('value', value)):
            for n in (1, 33):                                               # at both row counts the shape runs at
                miss = np.abs(got.numpy()[:n] - b['ref'][k][:n]).max()
                print('D%d columns from %d on dropped, %d rows: %s misses by %.3g (bar %.3g)' % (D, first_dropped, n, k, miss, b['bars'][k]))
                assert miss > 10.0 * b['bars'][k], (k, n, miss, b['bars'][k])


def test_entry_points_refuse_bad_arguments_before_touching_a_device():
    from rl4rs_amd import _lib
    lib = _lib.load()
    buf = np.zeros(300000, dtype=np.float32)
    p = buf.ctypes.data_as(C.c_void_p)

    def create(D, H, E, rows, params=p):
        h = C.c_void_p()
        rc = lib.rl4rs_gpolicy_create(D, H, E, rows, params, None, C.byref(h))
        return rc, lib.rl4rs_last_error().decode(), h

    for args, word in (((0, 256, 32, 8), 'obs_dim'), ((4097, 256, 32, 8), 'obs_dim'), ((256, 96, 32, 8), 'hidden'),
                       ((256, 512, 32, 8), 'hidden'), ((256, 256, 65, 8), 'act_dim'), ((256, 256, 0, 8), 'act_dim'),
                       ((256, 256, 284, 8), 'act_dim'), ((256, 256, 32, 0), 'max_rows')):
        rc, msg, h = create(*args)
        assert rc == -1 and not h.value and word in msg, (args, rc, msg)       # RL4RS_EINVAL, no handle
    rc, msg, h = create(256, 256, 32, 8, None)
    assert rc == -1 and not h.value
    if lib.rl4rs_device_count() <= 0:                                        # an admitted shape gets as far as the device check
        rc, msg, h = create(256, 256, 32, 8)
        assert rc == -2 and 'no HIP device' in msg, (rc, msg)
    # a null handle is refused by every call that takes one
    z = None
    calls = (lambda: lib.rl4rs_gpolicy_params(z, p, p, p), lambda: lib.rl4rs_gpolicy_adam_state(z, p, p, p),
             lambda: lib.rl4rs_gpolicy_set_adam_step(z, 3), lambda: lib.rl4rs_gpolicy_copy_params(z, z, None),
             lambda: lib.rl4rs_gpolicy_act(z, 4, p, 0, 0, 0, p, p, p, p, p, p, p, None),
             lambda: lib.rl4rs_gpolicy_evaluate(z, 4, p, p, p, p, p, p, None),
             lambda: lib.rl4rs_gpolicy_loss_grad(z, 0, 4, p, p, p, p, p, p, p, 0.5, 0.01, 0.3, 500.0, 0.2, p, p, None),
             lambda: lib.rl4rs_gpolicy_adam_step(z, p, 1e-4, 0.9, 0.999, 1e-8, 0.0, None),
             lambda: lib.rl4rs_gpolicy_ppo_epoch(z, 8, 4, p, p, p, p, p, p, p, 0.5, 0.0, 0.3, 500.0, 0.2, 1e-4, 0.9, 0.999, 1e-8, 0.0, p, p, None),
             lambda: lib.rl4rs_gpolicy_vtrace_loss_grad(z, 1, 2, 4, p, p, p, p, 1.0, 1.0, 1.0, 1, 0.5, 0.01, p, p, p, None))
    for i, call in enumerate(calls):
        assert call() == -1, i
    assert lib.rl4rs_gpolicy_destroy(None) == 0
    assert lib.rl4rs_gpolicy_param_count(0, 256, 32) == 0


def test_trainers_refuse_the_other_action_space():
    from rl4rs_amd.train import ContiTrainer, Trainer

    class Env(object):
        def __init__(self, **cfg):
            self.config = dict(batch_size=8, max_steps=9, action_size=284, return_tensors=True, **cfg)

    with pytest.raises(AssertionError, match='ContiTrainer'):
        Trainer(Env(support_conti_env=True))
    with pytest.raises(AssertionError, match='continuous'):
        ContiTrainer(Env())
    with pytest.raises(ValueError, match='support_onehot_action'):
        ContiTrainer(Env(support_conti_env=True, support_onehot_action=True))
    with pytest.raises(ValueError, match='rawstate_as_obs'):
        ContiTrainer(Env(support_conti_env=True, rawstate_as_obs=True))
    with pytest.raises(ValueError):
        ContiTrainer(Env(support_conti_env=True), algo='DQN')
