"""TEST INFRASTRUCTURE ONLY - torch restatement of the Gaussian actor-critic (rl4rs_amd/csrc/gausspolicy.hip, rl4rs_amd.train.ContiTrainer):
RLlib 1.5.1's FullyConnectedNetwork under MODEL_DEFAULTS, its DiagGaussian and the A2C / PPO / V-trace losses as the `is_conti`
branches of the reference's script/modelfree_train.py:219-234,271-286,315-330,362-377 configure them.

PARITY UNPINNED: ray is absent and the reference holds no vector for these learners; what follows restates the published form -
  fcnet            actor  head = tanh(tanh(x W1 + b1) W2 + b2) W3 + b3 = [mean | log_std];  critic V = tanh(tanh(x V1 + c1) V2 + c2) V3 + c3
  DiagGaussian     z = (a - mean) exp(-log_std);  logp = sum(-z^2 / 2 - log_std) - E log(2 pi) / 2;  entropy = sum(log_std + log(2 pi e) / 2);
                   kl(old || new) = sum(ls_n - ls_o + (exp(2 ls_o) + (mu_o - mu_n)^2) / (2 exp(2 ls_n)) - 1 / 2)
  losses           the formulas of oracle.policy (A2C: sums; PPO: means, KL(old || new), value clipping around the old value)
Every function runs in the dtype it is given: float64 is the reference, the same code in float32 on the CPU measures what float32
costs at a shape (the bars of tests/test_gpu_gauss_policy.py are 4 x that)."""
import math

import numpy as np
import torch

from td3_ref import normal01          # noqa: F401  (the library's counter RNG: the noise of rl4rs_gpolicy_act)
import vtrace_ref as VR

NAMES = ('W1', 'b1', 'W2', 'b2', 'W3', 'b3', 'V1', 'c1', 'V2', 'c2', 'V3', 'c3')
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def shapes(D, H, E):
    return (('W1', (D, H)), ('b1', (H,)), ('W2', (H, H)), ('b2', (H,)), ('W3', (H, 2 * E)), ('b3', (2 * E,)),
            ('V1', (D, H)), ('c1', (H,)), ('V2', (H, H)), ('c2', (H,)), ('V3', (H, 1)), ('c3', (1,)))


def param_count(D, H, E):
    return 2 * (D * H + H + H * H + H) + H * 2 * E + 2 * E + H + 1


def split(flat, D, H, E):
    out, o = {}, 0
    for name, s in shapes(D, H, E):
        k = int(np.prod(s))
        out[name] = flat[o:o + k].reshape(s)
        o += k
    assert o == flat.shape[0]
    return out


def _t(x, dtype):
    return x.to(dtype) if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x)).to(dtype)


def forward(flat, obs, dims, dtype=torch.float64):
    """-> (head [N, 2E], value [N]) as tensors of ``dtype`` (flat may carry a graph)"""
    D, H, E = dims
    w = split(_t(flat, dtype), D, H, E)
    x = _t(obs, dtype)
    h = torch.tanh(torch.tanh(x @ w['W1'] + w['b1']) @ w['W2'] + w['b2'])
    c = torch.tanh(torch.tanh(x @ w['V1'] + w['c1']) @ w['V2'] + w['c2'])
    return h @ w['W3'] + w['b3'], (c @ w['V3'] + w['c3'])[:, 0]


def logp(head, a):
    E = head.shape[1] // 2
    mean, ls = head[:, :E], head[:, E:]
    z = (a - mean) * torch.exp(-ls)
    return (-0.5 * z * z - ls).sum(dim=1) - E * HALF_LOG_2PI


def entropy(head):
    E = head.shape[1] // 2
    return (head[:, E:] + (HALF_LOG_2PI + 0.5)).sum(dim=1)


def kl(old_head, head):
    E = head.shape[1] // 2
    mo, lo, mn, ln = old_head[:, :E], old_head[:, E:], head[:, :E], head[:, E:]
    return (ln - lo + (torch.exp(2.0 * lo) + (mo - mn) ** 2) / (2.0 * torch.exp(2.0 * ln)) - 0.5).sum(dim=1)


def head_derivatives(head, a, old_head=None):
    """The closed forms the loss kernel uses: (d logp / d head, d entropy / d head, d kl / d head or None), each [N, 2E]."""
    E = head.shape[1] // 2
    mean, ls = head[:, :E], head[:, E:]
    inv = torch.exp(-ls)
    z = (a - mean) * inv
    d_lp = torch.cat([z * inv, z * z - 1.0], dim=1)
    d_en = torch.cat([torch.zeros_like(ls), torch.ones_like(ls)], dim=1)
    d_kl = None
    if old_head is not None:
        mo, lo = old_head[:, :E], old_head[:, E:]
        inv2 = torch.exp(-2.0 * ls)
        d_kl = torch.cat([-(mo - mean) * inv2, 1.0 - (torch.exp(2.0 * lo) + (mo - mean) ** 2) * inv2], dim=1)
    return d_lp, d_en, d_kl


def act(flat, obs, dims, seed, step, deterministic=False, dtype=torch.float64):
    """rl4rs_gpolicy_act -> dict(action, env_action, logp, value, entropy, head, eps); the noise row is the row's position"""
    D, H, E = dims
    with torch.no_grad():
        head, value = forward(flat, obs, dims, dtype)
        n, e = np.meshgrid(np.arange(head.shape[0]), np.arange(E), indexing='ij')
        eps = _t(normal01(seed, step, n, e), dtype)
        a = head[:, :E] if deterministic else head[:, :E] + torch.exp(head[:, E:]) * eps
        return dict(action=a, env_action=a.clamp(-1.0, 1.0), logp=logp(head, a), value=value, entropy=entropy(head), head=head, eps=eps)


def row_terms(algo, head, v, a, adv, ret, old_logp=None, old_value=None, old_head=None, clip=0.3, vf_clip=500.0):
    """Per-row (policy loss, value loss, entropy, kl, ratio-clip binds, value-clip binds) of the A2C (0) / PPO (1) loss"""
    lp, ent = logp(head, a), entropy(head)
    if algo == 0:
        z = torch.zeros_like(lp)
        return -lp * adv, 0.5 * (v - ret) ** 2, ent, z, z.bool(), z.bool()
    ratio = torch.exp(lp - old_logp)
    s1, s2 = adv * ratio, adv * ratio.clamp(1.0 - clip, 1.0 + clip)
    l1 = (v - ret) ** 2
    vc = old_value + (v - old_value).clamp(-vf_clip, vf_clip)
    l2 = (vc - ret) ** 2
    return -torch.minimum(s1, s2), torch.maximum(l1, l2), ent, kl(old_head, head), s2 < s1, (v - old_value).abs() > vf_clip


def loss_and_grad(algo, flat, obs, actions, adv, ret, dims, old_logp=None, old_value=None, old_head=None, vf_coeff=0.5, ent_coeff=0.01,
                  clip=0.3, vf_clip=500.0, kl_coeff=0.2, dtype=torch.float64):
    """rl4rs_gpolicy_loss_grad -> (grad [n] numpy float64, stats [4] sums, dict(ratio_clipped, value_clipped) bool arrays)"""
    p = _t(flat, dtype).clone().requires_grad_(True)
    f = lambda x: None if x is None else _t(x, dtype)
    a, adv, ret, old_logp, old_value, old_head = f(actions), f(adv), f(ret), f(old_logp), f(old_value), f(old_head)
    head, v = forward(p, obs, dims, dtype)
    pi, vf, ent, k, rc, vc = row_terms(algo, head, v, a, adv, ret, old_logp, old_value, old_head, clip, vf_clip)
    total = pi + vf_coeff * vf - ent_coeff * ent + (kl_coeff * k if algo == 1 else 0.0)
    loss = total.sum() if algo == 0 else total.mean()
    loss.backward()
    stats = np.array([pi.sum().item(), vf.sum().item(), ent.sum().item(), k.sum().item()])
    return p.grad.detach().double().numpy(), stats, dict(ratio_clipped=rc.numpy(), value_clipped=vc.numpy())


def adam_tf(p, g, m, v, t, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, grad_clip=0.0, dtype=np.float64):
    """tf.train.AdamOptimizer after tf.clip_by_global_norm (grad_clip > 0); t = the step being taken (1-based); numpy arrays of
    ``dtype``.  The hyper-parameters and lr_t are the float32 values the C ABI and the kernel receive."""
    p, g, m, v = (np.asarray(x, dtype=dtype) for x in (p, g, m, v))
    c = lambda x: dtype(np.float32(x))
    b1, b2, eps = c(beta1), c(beta2), c(eps)
    if grad_clip > 0.0:
        norm = np.sqrt((g * g).sum(dtype=dtype))
        if norm > c(grad_clip):
            g = g * (c(grad_clip) / norm)
    lr_t = c(float(np.float32(lr)) * math.sqrt(1.0 - float(np.float32(beta2)) ** t) / (1.0 - float(np.float32(beta1)) ** t))
    m = b1 * m + (dtype(1.0) - b1) * g
    v = b2 * v + (dtype(1.0) - b2) * g * g
    return p - lr_t * m / (np.sqrt(v) + eps), m, v


def vtrace_loss_and_grad(flat, obs, actions, behaviour_logp, rewards, R, T, B, dims, gamma=1.0, clip_rho=1.0, clip_pg_rho=1.0, drop_last=True,
                         vf_coeff=0.5, ent_coeff=0.01, dtype=torch.float64):
    """rl4rs_gpolicy_vtrace_loss_grad: evaluate every row, V-trace per rollout (tests/vtrace_ref.py, float64 on the evaluation's
    numbers as the device's scan is), the A2C-form loss on the kept rows with vs / pg_adv held constant.
    -> (grad, stats [4], vtrace sums [4] of {rho, min(rho, clip_rho), vs, pg_adv} over the kept rows, rho of the kept rows)"""
    with torch.no_grad():
        head, v = forward(flat, obs, dims, dtype)
        tlp = logp(head, _t(actions, dtype))
    tlp, v = tlp.double().numpy(), v.double().numpy()
    vs, pg = VR.vtrace_rollouts(R, T, B, behaviour_logp, tlp, v, rewards, None, gamma, clip_rho, clip_pg_rho, drop_last)
    rows = VR.kept_rows(R, T, B, drop_last)
    g, stats, _ = loss_and_grad(0, flat, np.asarray(obs)[rows], np.asarray(actions)[rows], pg[rows], vs[rows], dims, vf_coeff=vf_coeff,
                                ent_coeff=ent_coeff, dtype=dtype)
    rho = np.exp(tlp[rows] - np.asarray(behaviour_logp, dtype=np.float64)[rows])
    vstats = np.array([rho.sum(), np.minimum(rho, float(np.float32(clip_rho))).sum(), vs[rows].sum(), pg[rows].sum()])
    return g, stats, vstats, rho


def block_rel_err(g, ref, dims):
    """name -> max |g - ref| / max |ref| per parameter block (a block whose reference is all zero reports max |g|)"""
    D, H, E = dims
    out = {}
    gs, rs = split(np.asarray(g, dtype=np.float64), D, H, E), split(np.asarray(ref, dtype=np.float64), D, H, E)
    for name in NAMES:
        scale = np.abs(rs[name]).max()
        out[name] = np.abs(gs[name] - rs[name]).max() / (scale if scale > 0.0 else 1.0)
    return out


def make_params(dims, seed=0, ls_lo=-3.0, ls_hi=1.0, head_scale=30.0, value_scale=50.0):
    """Parameters that exercise the kernels: RLlib's initialisation with both output layers scaled up (the 0.01 normc heads are
    nearly constant) and the log_std biases spread over [ls_lo, ls_hi]."""
    from rl4rs_amd.nets.gausspolicy import init_gausspolicy_params
    D, H, E = dims
    flat = init_gausspolicy_params(D, E, H, seed).astype(np.float64)
    w = split(flat, D, H, E)
    w['W3'] *= head_scale
    w['W3'][:, E:] *= 0.1
    w['V3'] *= value_scale
    w['b3'][E:] = np.linspace(ls_lo, ls_hi, E) if E > 1 else -1.0
    rs = np.random.RandomState(seed + 77)
    for b in ('b1', 'b2', 'c1', 'c2', 'c3'):
        w[b][...] = 0.1 * rs.randn(*w[b].shape)
    w['b3'][:E] = 0.1 * rs.randn(E)
    return flat.astype(np.float32)
