"""The policy net away from its one default shape (obs_dim 256, hidden 64 / 128, 284 actions - all that tests/test_gpu_policy.py
runs): every kernel form rl4rs_policy_* picks by shape, against the float64 restatement (oracle/policy.py).

Forms (policy.hip's selection code): k_policy_tile_std at the default shape; k_policy_tile where its tiling and its LDS fit
(hidden % 64 == 0, hidden / 32 in {2, 4, 8}, obs_dim % 32 == 0, ...); otherwise one wave per sample, k_policy_forward<true / false>
and k_policy_train with W2 staged in LDS or read from memory.  PPO passes: k_ppo_pass<false> where the pass fits (action_size >= 255,
16- / 32-row workgroups pinned), else the per-minibatch chain.  Every batch holds one row with every action allowed, one with only
the last action allowed (the tail bit of the last mask word) and one with no allowed action (the reference's mask term makes every
logit float32.min: a uniform distribution, logp = -log(A)).

Bars: the floors of the existing tests (logits / value / entropy 2e-5, logp 3e-5, gradient 2e-4 of its largest entry, statistics
rtol 2e-4 / atol 1e-3, raw-state forward 2e-4, raw-state gradients 3e-4 relative), each scaled by max(1, e32(case) / e32(floor's
shape)), where e32 is the error of the same formula evaluated in float32 on the CPU against float64 on the same inputs (the
reference form's own rounding, never the kernel's).  PPO passes against float64: the pass-versus-chain criterion of
tests/test_gpu_policy.py::test_ppo_epoch_equals_minibatch_sequence."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LR = 1e-3
KW = dict(vf_coeff=0.5, ent_coeff=0.01, clip=0.3, vf_clip=30.0, kl_coeff=0.2)
PPO_KW = dict(vf_coeff=0.5, ent_coeff=0.01, clip=0.3, vf_clip=500.0, kl_coeff=0.2)
# largest action_size rl4rs_policy_create takes at obs_dim 256 / hidden 64: 16 * (256 + 64 + 2 * (A + 1)) bytes <= 160 KB
A_MAX = (160 * 1024 // 16 - 256 - 64) // 2 - 1

# (od, hid, A, MB, options); comments: act + evaluate form / loss_grad form / ppo_epoch form
CASES = {
    'default_mb128': (256, 64, 284, 128, {}),                        # tile_std / tile_std / k_ppo_pass<false> (MB % 256 != 0)
    'default_tile_off': (256, 64, 284, 256, {'tile': 0, 'ppo_fused': 0}),   # k_policy_forward / k_policy_train staged / chain
    'hid256': (256, 256, 284, 256, {}),                              # k_policy_tile NT1 = 8 / tile / chain (pass LDS 177 KB)
    'a255': (256, 64, 255, 128, {}),                                 # tile / tile / k_ppo_pass<false>, smallest A it takes (AE 256)
    'a254': (256, 64, 254, 256, {}),                                 # tile / tile / chain (AE < 256)
    'a256_rows': (256, 64, 256, 256, {'ppo_rows': (16, 32)}),        # tile / tile / k_ppo_pass<false> 16- and 32-row, W = 8
    'a300': (256, 64, 300, 256, {}),                                 # tile / tile / k_ppo_pass<false>, W = 10
    'hid96': (256, 96, 284, 128, {}),                                # one-wave / staged / chain
    'hid192': (256, 192, 284, 256, {}),                              # one-wave / unstaged / chain
    'hid1024': (256, 1024, 284, 256, {}),                            # one-wave / unstaged / chain (largest hidden create takes)
    'od266': (266, 64, 284, 256, {}),                                # one-wave (OD % 32 != 0) / staged / chain
    'od3072': (3072, 64, 284, 256, {}),                              # tile (~142 KB) / tile (~152 KB) / chain (widedeep width)
    'od3584': (3584, 64, 284, 256, {}),                              # tile / staged (tile<2> needs 164 KB) / chain
    'od4000_hid96': (4000, 96, 284, 128, {}),                        # one-wave at 70 KB / unstaged at 73 KB / chain
    'a2': (100, 32, 2, 128, {}),                                     # one-wave / staged / chain
    'a33': (256, 64, 33, 128, {}),                                   # tile / tile / chain (one-bit tail word, A < 64)
    'a1900': (256, 64, 1900, 256, {}),                               # tile (103 KB) / one-wave unstaged (tile<2> > 160 KB) / chain
    'lds_boundary': (256, 64, A_MAX, 256, {}),                       # one-wave (tile > 160 KB) / unstaged at 160 KB / chain
}
FREQ_A = (2, 33, 300)


def _data(N, rs, od=256, A=284):
    """tests/test_gpu_policy.py's generator at any width, plus the special rows: 0 = every action allowed, 1 = only the last
    action allowed, 2 = no action allowed."""
    obs = rs.randn(N, od).astype(np.float32)
    mask = (rs.rand(N, A) < 0.4).astype(np.int64)
    mask[np.arange(N), rs.randint(0, A, size=N)] = 1
    mask[0] = 1
    if N > 1:
        mask[1] = 0
        mask[1, A - 1] = 1
    if N > 2:
        mask[2] = 0
    return obs, mask, _bits(mask)


def _bits(mask):
    N, A = mask.shape
    W = (A + 31) // 32
    pad = np.zeros((N, W * 32), dtype=np.uint64)
    pad[:, :A] = mask
    return (pad.reshape(N, W, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32).view(np.int32)


def _params(od, hid, A, rs, seed=3):
    from rl4rs_amd.nets.policy import init_policy_params
    flat = init_policy_params(od, hid, A, seed)
    return flat + (rs.randn(flat.size) * 0.05).astype(np.float32)


def _entropy(lsm):
    p = np.exp(lsm)
    return -np.where(p > 0, p * lsm, 0.0).sum(axis=1)


def _e32_forward(flat, obs, mask, od, hid, A):
    from oracle import policy as OP
    l64, v64 = OP.forward(flat, obs, mask, od=od, hid=hid, A=A)
    l32, v32 = OP.forward(flat, obs, mask, od=od, hid=hid, A=A, dtype=np.float32)
    ok = mask > 0
    return max(np.abs(l32.astype(np.float64)[ok] - l64[ok]).max(), np.abs(v32.astype(np.float64) - v64).max())


def _e32_grad(algo, args, kw, od, hid, A):
    from oracle import policy as OP
    g64, _ = OP.loss_and_grad(algo, *args, od=od, hid=hid, A=A, **kw)
    g32, _ = OP.loss_and_grad(algo, *args, od=od, hid=hid, A=A, dtype=np.float32, **kw)
    return np.abs(g32.astype(np.float64) - g64).max() / np.abs(g64).max()


@functools.lru_cache(maxsize=None)
def _floor_e32_forward():
    """e32 of the logits at the floor's shape (tests/test_gpu_policy.py::test_wider_hidden_layer_takes_the_same_paths: 256 / 128 / 284)"""
    rs = np.random.RandomState(21)
    obs, mask, _ = _data(1027, rs)
    return _e32_forward(_params(256, 128, 284, rs, 6), obs, mask, 256, 128, 284)


@functools.lru_cache(maxsize=None)
def _floor_e32_grad(algo):
    """relative e32 of the gradient at the floor's shape (test_loss_gradients_match_autograd: 256 / 64 / 284, N = 1500)"""
    rs = np.random.RandomState(algo + 1)
    N = 1500
    obs, mask, _ = _data(N, rs)
    flat = _params(256, 64, 284, rs, 1)
    args = _loss_inputs(flat, obs, mask, np.argmax(mask, axis=1), rs, 256, 64, 284)
    return _e32_grad(algo, args, KW, 256, 64, 284)


def _loss_inputs(flat, obs, mask, actions, rs, od, hid, A):
    """(flat, obs, mask, actions, adv, ret, old_logp, old_value, old_logits) as float64 arrays holding exactly what the device gets"""
    from oracle import policy as OP
    N = obs.shape[0]
    old = flat + (rs.randn(flat.size) * 0.01).astype(np.float32)
    old_logits, old_value = OP.forward(old, obs, mask, od=od, hid=hid, A=A)
    old_logp = OP.log_softmax(old_logits)[np.arange(N), actions]
    f32 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)
    adv, ret = f32(rs.randn(N) * 3), f32(rs.randn(N) * 50 + 100)
    return (flat, obs, mask, np.asarray(actions), adv, ret, f32(old_logp), f32(old_value), f32(np.maximum(old_logits, -3.4e38)))


def _ratio(e_case, e_floor):
    return max(1.0, e_case / e_floor)


def _policy(od, hid, A, N, flat, opts=None):
    from rl4rs_amd.device import DevicePolicy
    pol = DevicePolicy(od, hid, A, max_rows=N, params=flat)
    for k, v in (opts or {}).items():
        if k != 'ppo_rows':
            pol.set_option(k, v)
    return pol


def _check_forward(pol, obs, mask, bits, ref, bar_f, bar_lp, tag):
    """act (draws legal, reproducible, outputs against float64) and evaluate of the draws (bit-identical to act)."""
    import torch
    logits, value, lsm, ent_ref = ref
    N = obs.shape[0]
    o, b = torch.from_numpy(obs).cuda(), torch.from_numpy(bits).cuda()
    a, lp, v, ent, lg = pol.act(o, b, seed=5, step=7, want_logits=True)
    a_np, lg_np = a.cpu().numpy(), lg.cpu().numpy()
    live = mask.any(axis=1)
    assert ((a_np >= 0) & (a_np < mask.shape[1])).all()
    assert mask[np.arange(N)[live], a_np[live]].all(), tag                    # never a masked action
    assert torch.equal(a, pol.act(o, b, seed=5, step=7)[0]), tag              # same (seed, step), same draws
    ok = mask > 0
    errs = dict(logits=np.abs(lg_np[ok] - logits[ok]).max(), value=np.abs(v.cpu().numpy() - value).max(),
                logp=np.abs(lp.cpu().numpy() - lsm[np.arange(N), a_np]).max(), entropy=np.abs(ent.cpu().numpy() - ent_ref).max())
    print('%s forward: %s  bar %.3g (logp %.3g)' % (tag, ' '.join('%s %.3g' % kv for kv in sorted(errs.items())), bar_f, bar_lp))
    assert np.isfinite(lp.cpu().numpy()).all() and np.isfinite(ent.cpu().numpy()).all(), tag
    assert (lg_np[~ok] < -1e37).all(), tag
    assert errs['logits'] < bar_f and errs['value'] < bar_f and errs['entropy'] < bar_f, (tag, errs)
    assert errs['logp'] < bar_lp, (tag, errs)
    lp2, v2, ent2, _ = pol.evaluate(o, a, b)
    assert torch.equal(lp2, lp) and torch.equal(v2, v) and torch.equal(ent2, ent), tag
    return a_np


def _check_loss_grad(pol, args, refs, r_g, tag):
    """A2C and PPO gradients + statistics against float64 autograd; returns the device's A2C gradient."""
    import torch
    t = lambda x, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(x)).to(dt).cuda()
    flat, obs, mask, actions, adv, ret, old_logp, old_value, old_logits = args
    b = t(_bits(mask), torch.int32)
    out = None
    for algo in (0, 1):
        g, stats = pol.loss_grad(algo, t(obs), t(actions, torch.int32), t(adv), t(ret), mask_bits=b, old_logp=t(old_logp),
                                 old_value=t(old_value), old_logits=t(old_logits), **KW)
        g_ref, s_ref = refs[algo]
        err, scale = np.abs(g.cpu().numpy() - g_ref).max(), np.abs(g_ref).max()
        print('%s loss_grad algo %d: gradient %.3g of max %.3g (relative %.3g, bar %.3g); stats %s vs %s' % (
            tag, algo, err, scale, err / scale, 2e-4 * r_g, stats.cpu().numpy(), s_ref))
        assert err < 2e-4 * r_g * scale, (tag, algo, err, scale)
        assert np.allclose(stats.cpu().numpy(), s_ref, rtol=2e-4 * r_g, atol=1e-3 * r_g), (tag, algo, stats, s_ref)
        if algo == 0:
            out = g
    return out


def _check_adam(pol, g):
    """One Adam step with the global-norm clip: the closed form of test_loss_gradients_match_autograd (step 1 of a fresh handle)."""
    before = pol.params().cpu().numpy().astype(np.float64)
    pol.adam_step(g, lr=1e-3, grad_clip=10.0)
    after = pol.params().cpu().numpy().astype(np.float64)
    g_np = g.cpu().numpy().astype(np.float64)
    gc = g_np * min(1.0, 10.0 / np.sqrt((g_np ** 2).sum()))
    lr_t = 1e-3 * np.sqrt(1 - 0.999) / (1 - 0.9)
    expect = before - lr_t * (0.1 * gc) / (np.sqrt(0.001 * gc * gc) + 1e-8)
    assert np.abs(after - expect).max() < 1e-6


def _ppo_reference(args, MB, passes, od, hid, A):
    """float64 restatement of `passes` SGD passes (OP.ppo_train_call's minibatch loop, no KL-coefficient update; trailing rows
    dropped) -> (params, m, v, t)."""
    from oracle import policy as OP
    flat, obs, mask, actions, adv, ret, old_logp, old_value, old_logits = args
    N = obs.shape[0]
    p = flat.astype(np.float64)
    m, v, step = np.zeros_like(p), np.zeros_like(p), 0
    for _ in range(passes):
        for lo in range(0, N - MB + 1, MB):
            s = slice(lo, lo + MB)
            g, _ = OP.loss_and_grad(1, p, obs[s], mask[s], actions[s], adv[s], ret[s], old_logp[s], old_value[s], old_logits[s],
                                    od=od, hid=hid, A=A, **PPO_KW)
            p, m, v, step = OP.adam_update(p, m, v, step, g, LR)
    return p, m, v, step


def _run_ppo(pol, args, MB, passes):
    import torch
    t = lambda x, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(x)).to(dt).cuda()
    flat, obs, mask, actions, adv, ret, old_logp, old_value, old_logits = args
    o, b, a = t(obs), t(_bits(mask), torch.int32), t(actions, torch.int32)
    for _ in range(passes):
        pol.ppo_epoch(o, a, t(adv), t(ret), b, t(old_logp), t(old_value), t(old_logits), minibatch=MB, lr=LR, **PPO_KW)
    pol.check_status()


def _check_ppo(pol, ref, flat, od, hid, A, r_g, tag):
    p_ref, m_ref, v_ref, t_ref = ref
    w = pol.params().cpu().numpy().astype(np.float64)
    m, v, t = pol.adam_state()
    m, v = m.cpu().numpy().astype(np.float64), v.cpu().numpy().astype(np.float64)
    diff = np.abs(w - p_ref)
    steps = t_ref
    moved = np.abs(p_ref - flat.astype(np.float64))
    print('%s ppo_epoch: params within 2e-5 %.5f, max %.3g (cap %.3g), median moved %.3g' % (
        tag, (diff < 2e-5).mean(), diff.max(), 2 * steps * LR, np.median(diff[moved > 1e-4])))
    assert t == steps, (tag, t, steps)
    assert (diff < 2e-5).mean() > 0.999, (tag, (diff < 2e-5).mean())
    assert diff.max() <= 2 * steps * LR, (tag, diff.max())
    assert np.median(diff[moved > 1e-4]) < 1e-6, tag
    # Adam moments, per parameter array [W1 | b1 | W2e | b2e]: m averages gradients, each good to the gradient bar (2e-4 * r_g of
    # the array's largest entry), v averages their squares (twice that, relative); same 0.1 % allowance as the parameters
    o = 0
    for k, n in (('W1', od * hid), ('b1', hid), ('W2e', hid * (A + 1)), ('b2e', A + 1)):
        s = slice(o, o + n)
        o += n
        fm = (np.abs(m[s] - m_ref[s]) <= 2e-4 * r_g * np.abs(m_ref[s]).max()).mean()
        fv = (np.abs(v[s] - v_ref[s]) <= 4e-4 * r_g * np.abs(v_ref[s]).max()).mean()
        print('%s   adam %s: m within bar %.5f (max err %.3g of max %.3g), v within bar %.5f (max err %.3g of max %.3g)' % (
            tag, k, fm, np.abs(m[s] - m_ref[s]).max(), np.abs(m_ref[s]).max(), fv, np.abs(v[s] - v_ref[s]).max(), np.abs(v_ref[s]).max()))
        assert fm > 0.999 and fv > 0.999, (tag, k, fm, fv)


@pytest.mark.parametrize('name', sorted(CASES))
def test_policy_shape(name):
    """act / evaluate / loss_grad / adam_step / two PPO passes of one shape against float64, in every form it can take"""
    import torch
    from oracle import policy as OP
    od, hid, A, MB, opts = CASES[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    N = 4 * MB + 37
    obs, mask, bits = _data(N, rs, od, A)
    flat = _params(od, hid, A, rs)
    logits, value = OP.forward(flat, obs, mask, od=od, hid=hid, A=A)
    lsm = OP.log_softmax(logits)
    ref = (logits, value, lsm, _entropy(lsm))
    assert np.isfinite(lsm).all()
    e_f = _e32_forward(flat, obs, mask, od, hid, A)
    r_f = _ratio(e_f, _floor_e32_forward())
    print('%s: e32 forward %.3g (floor shape %.3g)' % (name, e_f, _floor_e32_forward()))
    # the actions of the gradient checks: the device's own draws (the no-action row included)
    pol = _policy(od, hid, A, N, flat, opts)
    actions = _check_forward(pol, obs, mask, bits, ref, 2e-5 * r_f, 3e-5 * r_f, name)
    args = _loss_inputs(flat, obs, mask, actions, rs, od, hid, A)
    refs = dict((algo, OP.loss_and_grad(algo, *args, od=od, hid=hid, A=A, **KW)) for algo in (0, 1))
    e_g = [_e32_grad(algo, args, KW, od, hid, A) for algo in (0, 1)]
    r_g = max(_ratio(e_g[algo], _floor_e32_grad(algo)) for algo in (0, 1))
    print('%s: e32 gradient %s (floor shape %s), ratio %.3g' % (name, e_g, [_floor_e32_grad(0), _floor_e32_grad(1)], r_g))
    g = _check_loss_grad(pol, args, refs, r_g, name)
    _check_adam(pol, g)
    # the one-wave kernels as well wherever the tiled ones ran
    if opts.get('tile', 1):
        alt = _policy(od, hid, A, N, flat, dict(opts, tile=0))
        _check_forward(alt, obs, mask, bits, ref, 2e-5 * r_f, 3e-5 * r_f, name + ' tile=0')
        _check_loss_grad(alt, args, refs, r_g, name + ' tile=0')
        alt.close()
    if A in FREQ_A:                              # sampling follows the masked softmax: 20 000 copies of row 3
        rep = 20000
        big = _policy(od, hid, A, rep, flat)
        o = torch.from_numpy(np.repeat(obs[3:4], rep, axis=0)).cuda()
        b = torch.from_numpy(np.repeat(bits[3:4], rep, axis=0)).cuda()
        aa = big.act(o, b, seed=11, step=0)[0].cpu().numpy()
        freq = np.bincount(aa, minlength=A) / float(rep)
        dev = np.abs(freq - np.exp(lsm[3])).max()
        print('%s sample frequencies: max |freq - p| %.4f' % (name, dev))
        assert dev < 0.02
        big.close()
    # two PPO passes against the float64 restatement: the pass (where it fits) and the per-minibatch chain
    ppo_ref = _ppo_reference(args, MB, 2, od, hid, A)
    rows = opts.get('ppo_rows', (None,))
    for fused in ((0,) if opts.get('ppo_fused', 1) == 0 else (1, 0)):
        for r in (rows if fused else (None,)):
            p = _policy(od, hid, A, N, flat, dict(opts, ppo_fused=fused))
            if r is not None:
                p.set_option('ppo_rows', r)
            _run_ppo(p, args, MB, 2)
            _check_ppo(p, ppo_ref, flat, od, hid, A, r_g, '%s ppo_fused=%d rows=%s' % (name, fused, r))
            p.close()
    if 'ppo_rows' in opts:                     # PPO_ROWS = 0 is automatic again: bit-identical to a fresh handle
        pinned, fresh = _policy(od, hid, A, N, flat), _policy(od, hid, A, N, flat)
        pinned.set_option('ppo_rows', 16)
        pinned.set_option('ppo_rows', 0)
        _run_ppo(pinned, args, MB, 2)
        _run_ppo(fresh, args, MB, 2)
        assert torch.equal(pinned.params(), fresh.params())
        assert all(torch.equal(x, y) for x, y in zip(pinned.adam_state()[:2], fresh.adam_state()[:2]))
    pol.close()


@pytest.mark.parametrize('N', [1, 5])
def test_policy_tiny_batches(N):
    """N = 1 and 5 (one ragged 8-row tile; rows past N repeat the last live row) at a tiled non-default shape, both forms"""
    from oracle import policy as OP
    od, hid, A = 256, 64, 300
    rs = np.random.RandomState(N)
    obs, mask, bits = _data(N, rs, od, A)
    flat = _params(od, hid, A, rs)
    logits, value = OP.forward(flat, obs, mask, od=od, hid=hid, A=A)
    lsm = OP.log_softmax(logits)
    r_f = _ratio(_e32_forward(flat, obs, mask, od, hid, A), _floor_e32_forward())
    actions = None
    for tile in (1, 0):
        pol = _policy(od, hid, A, N, flat, dict(tile=tile))
        a = _check_forward(pol, obs, mask, bits, (logits, value, lsm, _entropy(lsm)), 2e-5 * r_f, 3e-5 * r_f, 'N=%d tile=%d' % (N, tile))
        if actions is None:
            actions = a
            args = _loss_inputs(flat, obs, mask, actions, rs, od, hid, A)
            refs = dict((algo, OP.loss_and_grad(algo, *args, od=od, hid=hid, A=A, **KW)) for algo in (0, 1))
            r_g = max(_ratio(_e32_grad(algo, args, KW, od, hid, A), _floor_e32_grad(algo)) for algo in (0, 1))
        _check_loss_grad(pol, args, refs, r_g, 'N=%d tile=%d' % (N, tile))
        pol.close()


def test_long_chunk_gradient_reduction():
    """N = 33 000 at a one-wave shape (hidden 96): more than 64 chunks of 512 samples, so the gradient GEMMs take the longer chunks
    of policy.hip's reduction (chunk 576, 58 partial matrices); A2C gradient and statistics against float64"""
    import torch
    from oracle import policy as OP
    od, hid, A, N = 256, 96, 284, 33000
    rs = np.random.RandomState(33)
    obs, mask, bits = _data(N, rs, od, A)
    flat = _params(od, hid, A, rs)
    pol = _policy(od, hid, A, N, flat)
    logits, _ = OP.forward(flat, obs, mask, od=od, hid=hid, A=A)
    a = pol.act(torch.from_numpy(obs).cuda(), torch.from_numpy(bits).cuda(), seed=2, step=0)[0].cpu().numpy()
    args = _loss_inputs(flat, obs, mask, a, rs, od, hid, A)
    g_ref, s_ref = OP.loss_and_grad(0, *args, od=od, hid=hid, A=A, **KW)
    r_g = _ratio(_e32_grad(0, args, KW, od, hid, A), _floor_e32_grad(0))
    t = lambda x, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(x)).to(dt).cuda()
    g, stats = pol.loss_grad(0, t(obs), t(a, torch.int32), t(args[4]), t(args[5]), mask_bits=t(bits, torch.int32), **KW)
    err, scale = np.abs(g.cpu().numpy() - g_ref).max(), np.abs(g_ref).max()
    print('long chunks: gradient %.3g of max %.3g (relative %.3g, bar %.3g)' % (err, scale, err / scale, 2e-4 * r_g))
    assert err < 2e-4 * r_g * scale
    assert np.allclose(stats.cpu().numpy(), s_ref, rtol=2e-4 * r_g, atol=1e-3 * r_g), (stats, s_ref)


def test_create_refuses_a_shape_no_form_can_run():
    """The LDS limit is checked at create, before any launch: A_MAX (the boundary case above) is taken, A_MAX + 1 refused with a
    message naming the limit; so are a wider observation and a wider hidden layer at the same budget."""
    from rl4rs_amd.device import DevicePolicy
    from rl4rs_amd._lib import Rl4rsHipError
    ok = DevicePolicy(256, 64, A_MAX, max_rows=4)
    ok.close()
    for od, hid, A in ((256, 64, A_MAX + 1), (160 * 1024 // 16 - 64 - 2 * 285 + 1, 64, 284), (9000, 1024, 284)):
        with pytest.raises(Rl4rsHipError, match='LDS'):
            DevicePolicy(od, hid, A, max_rows=4)


# ---- raw-state policy (rl4rs_rawpolicy_* / rl4rs_rawtrain_*) at other configurations -------------------------------------------
RAW_FLOOR = {"maxlen": 64, "action_size": 284, "dense_feature_num": 432, "category_feature_num": 21, "category_hash_size": 3000,
             "seq_num": 2, "emb_size": 128, "hidden_units": 128}
RAW_CFGS = {
    'R1': dict(maxlen=33, category_feature_num=13, hidden_units=96, dense_feature_num=61, seq_num=3, emb_size=72, action_size=100,
               category_hash_size=3000),
    'R2': dict(maxlen=1, seq_num=1, category_feature_num=1, emb_size=32, hidden_units=32, action_size=2, dense_feature_num=7,
               category_hash_size=500),
    'R3': dict(maxlen=16, seq_num=4, category_feature_num=32, emb_size=128, hidden_units=128, action_size=300, dense_feature_num=432,
               category_hash_size=3000),
}


def _raw_inputs(cfg, N, rs):
    H = cfg['category_hash_size']
    cat = rs.randint(0, H, size=(N, cfg['category_feature_num'])).astype(np.int32)
    dense = np.abs(rs.randn(N, cfg['dense_feature_num']) * 2).astype(np.float32)
    seqs = [rs.randint(0, H, size=(N, cfg['maxlen'])).astype(np.int32) for _ in range(cfg['seq_num'])]
    _, mask, bits = _data(N, rs, 1, cfg['action_size'])
    return cat, dense, seqs, mask, bits


def _raw_e32_forward(w, cat, dense, seqs, mask):
    from oracle import policy as OP
    l64, v64 = OP.rawstate_forward(w, cat, dense, seqs, mask)
    l32, v32 = OP.rawstate_forward(w, cat, dense, seqs, mask, dtype=np.float32)
    ok = mask > 0
    return max(np.abs(l32.astype(np.float64)[ok] - l64[ok]).max(), np.abs(v32.astype(np.float64) - v64).max())


def _raw_e32_grad(algo, w, args, kw):
    from oracle import policy as OP
    g64, _ = OP.rawstate_loss_and_grad(algo, w, *args, **kw)
    g32, _ = OP.rawstate_loss_and_grad(algo, w, *args, dtype=np.float32, **kw)
    return max(np.abs(g32[k].astype(np.float64) - g64[k]).max() / max(np.abs(g64[k]).max(), 1e-8) for k in g64)


def _raw_loss_args(w, cat, dense, seqs, mask, actions, rs):
    from oracle import policy as OP
    N = cat.shape[0]
    old_w = dict((k, v + (rs.randn(*v.shape) * 0.01).astype(np.float32)) for k, v in w.items())
    old_logits, old_value = OP.rawstate_forward(old_w, cat, dense, seqs, mask)
    f32 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)
    old_logp = OP.log_softmax(old_logits)[np.arange(N), actions]
    return (cat, dense, seqs, mask, np.asarray(actions), f32(rs.randn(N) * 3), f32(rs.randn(N) * 50 + 100), f32(old_logp),
            f32(old_value), f32(np.maximum(old_logits, -3.4e38)))


@functools.lru_cache(maxsize=None)
def _raw_floor_e32():
    """(forward e32, {algo: gradient e32}) at the configuration of the existing raw-state tests (N = 300 / 700)"""
    from rl4rs_amd.nets.rawpolicy import init_rawpolicy_weights
    w = init_rawpolicy_weights(RAW_FLOOR, seed=2, emb_scale=0.5, head_std=1.0, bias_noise=0.2)
    rs = np.random.RandomState(4)
    cat, dense, seqs, mask, _ = _raw_inputs(RAW_FLOOR, 300, rs)
    e_f = _raw_e32_forward(w, cat, dense, seqs, mask)
    rs = np.random.RandomState(3)
    cat, dense, seqs, mask, _ = _raw_inputs(RAW_FLOOR, 700, rs)
    args = _raw_loss_args(w, cat, dense, seqs, mask, np.argmax(mask, axis=1), rs)
    return e_f, dict((algo, _raw_e32_grad(algo, w, args, KW)) for algo in (0, 1))


@pytest.mark.parametrize('name', sorted(RAW_CFGS))
def test_rawstate_policy_other_configurations(name):
    """DeviceRawPolicy / DeviceRawTrainer act + evaluate against OP.rawstate_forward, A2C / PPO gradients against
    OP.rawstate_loss_and_grad, one clipped Adam step against its closed form"""
    import torch
    from rl4rs_amd.device import DeviceRawPolicy, DeviceRawTrainer
    from rl4rs_amd.nets.rawpolicy import init_rawpolicy_weights
    from oracle import policy as OP
    cfg = RAW_CFGS[name]
    A = cfg['action_size']
    rs = np.random.RandomState(sum(map(ord, name)))
    N = 300
    w = init_rawpolicy_weights(cfg, seed=2, emb_scale=0.5, head_std=1.0, bias_noise=0.2)
    cat, dense, seqs, mask, bits = _raw_inputs(cfg, N, rs)
    logits, value = OP.rawstate_forward(w, cat, dense, seqs, mask)
    lsm = OP.log_softmax(logits)
    ent_ref = _entropy(lsm)
    e_floor, eg_floor = _raw_floor_e32()
    r_f = _ratio(_raw_e32_forward(w, cat, dense, seqs, mask), e_floor)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    dseqs = [t(s) for s in seqs]
    ok = mask > 0
    live = mask.any(axis=1)
    trainer = DeviceRawTrainer(cfg, w, max_rows=N)
    actions = None
    for kind, pol in (('policy', DeviceRawPolicy(cfg, w, max_rows=N)), ('trainer', trainer)):
        a, lp, v, ent, lg = pol.act(t(cat), t(dense), dseqs, t(bits), seed=5, step=3, want_logits=True)
        a_np = a.cpu().numpy()
        assert mask[np.arange(N)[live], a_np[live]].all() and ((a_np >= 0) & (a_np < A)).all()
        assert torch.equal(a, pol.act(t(cat), t(dense), dseqs, t(bits), seed=5, step=3)[0])
        errs = dict(logits=np.abs(lg.cpu().numpy()[ok] - logits[ok]).max(), value=np.abs(v.cpu().numpy() - value).max(),
                    logp=np.abs(lp.cpu().numpy() - lsm[np.arange(N), a_np]).max(), entropy=np.abs(ent.cpu().numpy() - ent_ref).max())
        print('%s %s forward: %s  bar %.3g' % (name, kind, ' '.join('%s %.3g' % kv for kv in sorted(errs.items())), 2e-4 * r_f))
        assert max(errs.values()) < 2e-4 * r_f, (name, kind, errs)
        assert (lg.cpu().numpy()[~ok] < -1e37).all()
        lp2, v2, ent2, _ = pol.evaluate(t(cat), t(dense), dseqs, a, t(bits))
        assert torch.equal(lp, lp2) and torch.equal(v, v2) and torch.equal(ent, ent2)
        if actions is None:
            actions = a_np
    args = _raw_loss_args(w, cat, dense, seqs, mask, actions, rs)
    f = lambda x: t(np.asarray(x, dtype=np.float32))
    for algo in (0, 1):
        stats = trainer.loss_grad(algo, t(cat), t(dense), dseqs, t(actions.astype(np.int32)), f(args[5]), f(args[6]), mask_bits=t(bits),
                                  old_logp=f(args[7]), old_value=f(args[8]), old_logits=f(args[9]), **KW)
        g = dict((k, x.cpu().numpy()) for k, x in trainer.gradients().items())
        g_ref, s_ref = OP.rawstate_loss_and_grad(algo, w, *args, **KW)
        r_g = _ratio(_raw_e32_grad(algo, w, args, KW), eg_floor[algo])
        assert set(g) == set(g_ref)
        for k in sorted(g_ref):
            scale = max(np.abs(g_ref[k]).max(), 1e-8)
            err = np.abs(g[k] - g_ref[k]).max()
            print('%s algo %d %s: gradient %.3g of max %.3g (relative %.3g, bar %.3g)' % (name, algo, k, err, scale, err / scale, 3e-4 * r_g))
            assert err < 3e-4 * r_g * scale, (name, algo, k, err, scale)
        assert np.allclose(stats.cpu().numpy(), s_ref, rtol=2e-4 * r_g, atol=1e-3 * r_g), (name, algo, stats, s_ref)
    before, gflat = trainer._flat('params').cpu().numpy().astype(np.float64), trainer._flat('grad').cpu().numpy().astype(np.float64)
    trainer.adam_step(lr=1e-3, grad_clip=10.0)
    after = trainer._flat('params').cpu().numpy().astype(np.float64)
    gc = gflat * min(1.0, 10.0 / np.sqrt((gflat ** 2).sum()))
    lr_t = 1e-3 * np.sqrt(1 - 0.999) / (1 - 0.9)
    assert np.abs(after - (before - lr_t * (0.1 * gc) / (np.sqrt(0.001 * gc * gc) + 1e-8))).max() < 1e-6
    trainer.close()


# ---- Trainer on the widedeep simulator: 3072-wide observations ------------------------------------------------------------------
def _unpack(bits, A=284):
    b = bits.view(np.uint32)
    return ((b[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1).reshape(b.shape[0], -1)[:, :A].astype(np.float64)


def _widedeep_env(tmp_path):
    from test_gpu_train_dp import _env, _make_cfg
    cfg = _make_cfg(str(tmp_path), 0, B=64, T=9)
    cfg['algo'] = 'widedeep'
    return _env(cfg)


def test_trainer_on_widedeep_observations_a2c(tmp_path):
    """Trainer takes the observation width from env.observation_space (256 + 128 + 21 * 128 = 3072 with the widedeep simulator):
    two A2C train calls teacher-forced against OP.a2c_train_call(od=3072), with the assertions of
    test_gpu_fullsize.py::test_full_size_seqslate_a2c"""
    from rl4rs_amd.train import Trainer
    from oracle import policy as OP
    env = _widedeep_env(tmp_path)
    assert env.observation_space.shape == (3072,)
    tr = Trainer(env, algo='A2C', seed=11, init_seed=3, keep_last_batch=True)
    assert tr.buf['obs'].shape[1] == 3072 and tr.policy.obs_dim == 3072
    flat = tr.params().cpu().numpy().astype(np.float64)
    state = (flat, np.zeros_like(flat), np.zeros_like(flat), 0)
    for it in range(2):
        out = tr.train_iteration()
        lb = tr.last_batch
        batch = dict((k, lb[k].cpu().numpy()) for k in ('obs', 'act', 'mask', 'adv', 'ret'))
        assert ((batch['act'] >= 0) & (batch['act'] < 284)).all()
        assert env.samples.get_violation().all()
        state, sums, norm, g = OP.a2c_train_call(state, batch, 1e-4, _unpack, od=3072)
        got = tr.params().cpu().numpy()
        g_ref = g * max(norm / 10.0, 1.0)
        g_dev = tr.grad.cpu().numpy().astype(np.float64)
        print('widedeep A2C call %d: gradient %.3g of max %.3g, norm %.3g' % (it, np.abs(g_dev - g_ref).max(), np.abs(g_ref).max(), norm))
        assert np.abs(g_dev - g_ref).max() < 2e-3 * np.abs(g_ref).max(), (it, np.abs(g_dev - g_ref).max(), np.abs(g_ref).max())
        solid = np.abs(g_dev - g_ref) <= 0.01 * np.abs(g_ref)
        assert solid.mean() > 0.9, solid.mean()
        assert np.abs(got - state[0])[solid].max() < 5e-6, (it, np.abs(got - state[0])[solid].max())
        assert np.abs(got - state[0]).max() <= 2.2e-4 * (it + 1)
        N = batch['obs'].shape[0]
        assert np.allclose([out['policy_loss'] / N, out['vf_loss'] / N, out['entropy'] / N], sums[:3] / N, rtol=2e-3, atol=1e-4), (out, sums)
    tr.close()


def test_trainer_on_widedeep_observations_ppo(tmp_path):
    """Two PPO train calls on the 3072-wide observations against OP.ppo_train_call(od=3072), with the assertions of
    test_gpu_train_dp.py::test_trainer_tracks_fp64_ppo_restatement"""
    from rl4rs_amd.train import Trainer
    from oracle import policy as OP
    env = _widedeep_env(tmp_path)
    env.seed(7)
    tr = Trainer(env, algo='PPO', seed=3, init_seed=9, lr=1e-3, minibatch=128, keep_last_batch=True, kl_target=0.01)
    assert tr.buf['obs'].shape[1] == 3072
    flat = tr.params().cpu().numpy().astype(np.float64)
    state = (flat, np.zeros_like(flat), np.zeros_like(flat), 0)
    kl_coeff = 0.2
    for it in range(2):
        st = tr.train_iteration()
        lb = tr.last_batch
        assert lb['kl_coeff'] == kl_coeff
        batch = dict((k, lb[k].cpu().numpy()) for k in ('obs', 'act', 'mask', 'adv', 'ret', 'logp', 'val', 'logits'))
        state, ref = OP.ppo_train_call(state, batch, 128, 1e-3, kl_coeff, 0.01, _unpack, od=3072)
        got = tr.params().cpu().numpy()
        print('widedeep PPO call %d: params max diff %.3g' % (it, np.abs(got - state[0]).max()))
        assert np.abs(got - state[0]).max() < 2e-5, (it, np.abs(got - state[0]).max())
        assert abs(st['kl_mean'] - ref['kl_mean']) < 1e-5 + 1e-3 * abs(ref['kl_mean'])
        assert np.allclose([st['policy_loss'] / 128, st['vf_loss'] / 128, st['entropy'] / 128, st['kl'] / 128], ref['last'],
                           rtol=2e-3, atol=1e-4)
        kl_coeff = ref['kl_coeff']
        assert st['kl_coeff'] == kl_coeff
    tr.close()
