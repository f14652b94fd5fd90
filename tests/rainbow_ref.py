"""float64 restatement of the on-device Rainbow (include/rl4rs_hip.h, "On-device Rainbow"): the dueling distributional network,
the categorical Bellman projection, the cross-entropy loss with its hand-written gradient, the n-step row rule, the SoftQ inverse
CDF and the per-variable-clipped Adam step.

Test infrastructure only.  PARITY UNPINNED: ray 1.5.1 (dqn_tf_policy, distributional_q_tf_model, adjust_nstep) is absent, so this
restates their published form as script/modelfree_train.py:50-53,146-178 configures them; tests/test_rainbow_host.py checks the
gradient below against torch float64 autograd of the same loss."""
import numpy as np

from oracle import policy as OP

F32_MIN = -3.4028235e38
NAMES = ('W1', 'b1', 'W2', 'b2', 'Wa1', 'ba1', 'Wa2', 'ba2', 'Wv1', 'bv1', 'Wv2', 'bv2')


class Dims(object):
    def __init__(self, od=256, A=284, atoms=8, trunk=256, sh=128, dueling=True, v_min=0.0, v_max=1000.0):
        self.od, self.A, self.atoms, self.trunk, self.sh, self.dueling = int(od), int(A), int(atoms), int(trunk), int(sh), bool(dueling)
        self.v_min, self.v_max = float(v_min), float(v_max)
        self.dz = (self.v_max - self.v_min) / (self.atoms - 1)
        self.z = self.v_min + np.arange(self.atoms, dtype=np.float64) * self.dz

    def shapes(self):
        od, A, K, T, S = self.od, self.A, self.atoms, self.trunk, self.sh
        s = [(od, T), (T,), (T, T), (T,), (T, S), (S,), (S, A * K), (A * K,)]
        if self.dueling:
            s += [(T, S), (S,), (S, K), (K,)]
        return s

    def n_params(self):
        return int(sum(int(np.prod(s)) for s in self.shapes()))

    def ends(self):
        return np.cumsum([int(np.prod(s)) for s in self.shapes()])


def split(flat, dm):
    out, o = {}, 0
    for name, shp in zip(NAMES, dm.shapes()):
        n = int(np.prod(shp))
        out[name] = flat[o:o + n].reshape(shp)
        o += n
    assert o == len(flat)
    return out


def join(parts, dm):
    return np.concatenate([np.asarray(parts[n]).ravel() for n, _ in zip(NAMES, dm.shapes())])


def hidden(p, x, dm):
    h1 = np.tanh(x @ p['W1'] + p['b1'])
    h2 = np.tanh(h1 @ p['W2'] + p['b2'])
    ha = np.maximum(h2 @ p['Wa1'] + p['ba1'], 0.0)
    hv = np.maximum(h2 @ p['Wv1'] + p['bv1'], 0.0) if dm.dueling else None
    return h1, h2, ha, hv


def forward(flat, obs, dm):
    """-> (logits [N, A, atoms], p [N, A, atoms], Q [N, A])"""
    p = split(np.asarray(flat, dtype=np.float64), dm)
    x = np.asarray(obs, dtype=np.float64)
    _, _, ha, hv = hidden(p, x, dm)
    adv = (ha @ p['Wa2'] + p['ba2']).reshape(len(x), dm.A, dm.atoms)
    if dm.dueling:
        v = hv @ p['Wv2'] + p['bv2']
        logits = v[:, None, :] + adv - adv.mean(axis=1, keepdims=True)
    else:
        logits = adv
    e = np.exp(logits - logits.max(axis=2, keepdims=True))
    pr = e / e.sum(axis=2, keepdims=True)
    return logits, pr, (pr * dm.z).sum(axis=2)


def masked_q(q, mask):
    """The device's rule: a disallowed action's Q becomes the mask's -3.4028235e38; mask None = all allowed."""
    return q if mask is None else np.where(np.asarray(mask) > 0, q, F32_MIN)


# ---- projection ----------------------------------------------------------------------------------------------------------
def project(R, boot, p_next, gamma_n, dm, dtype=np.float64):
    """m [N, atoms]: the categorical projection exactly as RLlib's QLoss writes it.  Rows with boot False (terminal, or a
    successor that allows nothing) project the single point clip(R): r_tau_j = clip(R) for every j and sum_j p'_j = 1, a SELECT -
    p_next is not read there.
    ``dtype`` float32 repeats the arithmetic in single precision (the yardstick of the GPU tests' error bars)."""
    f = dtype
    R = np.asarray(R, dtype=f)
    p_next = np.asarray(p_next, dtype=f)
    N, K = len(R), dm.atoms
    m = np.zeros((N, K), dtype=f)
    rows = np.arange(N)
    vmin, vmax, dz, top = f(dm.v_min), f(dm.v_max), f(f(dm.v_max - dm.v_min) / f(K - 1)), f(K - 1)
    for j in range(K):
        r_tau = np.clip(np.where(boot, R + f(gamma_n) * (vmin + f(j) * dz), R), vmin, vmax)
        b = np.minimum((r_tau - vmin) / dz, top)         # (the min only guards the rounding of the division at v_max)
        lo, up = np.floor(b), np.ceil(b)
        eq = (up - lo < 0.5).astype(f)
        pj = np.where(boot, p_next[:, j], f(1.0 if j == 0 else 0.0))  # no bootstrap: the whole mass, once, at clip(R)
        np.add.at(m, (rows, lo.astype(np.int64)), pj * (up - b + eq))
        np.add.at(m, (rows, up.astype(np.int64)), pj * (b - lo))
    return m


# ---- loss ----------------------------------------------------------------------------------------------------------------
def next_action(flat, tflat, next_obs, next_mask, done, double_q, dm):
    """-> (a* [N] first maximum of the masked Q(s') of the selecting net, boot [N], gap [N] top-two gap of that masked row (inf
    where the row does not bootstrap), p' [N, A, atoms] of the TARGET net).  Terminal rows' successors are not read."""
    done = np.asarray(done).astype(bool)
    nobs = np.where(done[:, None], 0.0, np.asarray(next_obs, dtype=np.float64))
    N = len(done)
    mask = np.ones((N, dm.A)) if next_mask is None else np.where(done[:, None], 1.0, np.asarray(next_mask, dtype=np.float64))
    _, p_t, q_t = forward(tflat, nobs, dm)
    q_sel = forward(flat, nobs, dm)[2] if double_q else q_t
    q_sel = masked_q(q_sel, mask)
    astar = q_sel.argmax(axis=1)
    boot = ~done & (mask > 0).any(axis=1)
    top = np.sort(q_sel, axis=1)[:, -2:]
    gap = np.where(boot, top[:, 1] - top[:, 0], np.inf)
    return astar, boot, gap, p_t


def loss_and_grad(flat, tflat, obs, act, rew, done, next_obs, next_mask, weights, gamma_n, double_q, dm, astar=None):
    """-> dict(loss, grad, td, m, qsa, astar, astar_ref, boot, gap, stats, g).  ``astar`` (optional) overrides the argmax on the rows
    that bootstrap (teacher forcing with the device's choice on near-ties).  loss = mean(w * td), td = the softmax cross-entropy
    of the taken action's logits against the projected target; g = w / N (softmax - m) is d loss / d logits(s)[a, :]."""
    flat = np.asarray(flat, dtype=np.float64)
    tflat = np.asarray(tflat, dtype=np.float64)
    N = len(act)
    act = np.asarray(act, dtype=np.int64)
    rows = np.arange(N)
    a_ref, boot, gap, p_t = next_action(flat, tflat, next_obs, next_mask, done, double_q, dm)
    a_use = a_ref if astar is None else np.where(boot, np.asarray(astar, dtype=np.int64), a_ref)
    m = project(rew, boot, p_t[rows, a_use], gamma_n, dm)
    p = split(flat, dm)
    x = np.asarray(obs, dtype=np.float64)
    h1, h2, ha, hv = hidden(p, x, dm)
    K, A = dm.atoms, dm.A
    Wa2 = p['Wa2'].reshape(dm.sh, A, K)
    adv_a = np.einsum('nk,knj->nj', ha, Wa2[:, act, :]) + p['ba2'].reshape(A, K)[act]
    if dm.dueling:
        Wbar, bbar = Wa2.mean(axis=1), p['ba2'].reshape(A, K).mean(axis=0)
        logit = (hv @ p['Wv2'] + p['bv2']) + adv_a - (ha @ Wbar + bbar)
    else:
        logit = adv_a
    sh = logit - logit.max(axis=1, keepdims=True)
    lsm = sh - np.log(np.exp(sh).sum(axis=1, keepdims=True))
    sm = np.exp(lsm)
    td = -(m * lsm).sum(axis=1)
    w = np.ones(N) if weights is None else np.asarray(weights, dtype=np.float64)
    g = (w / N)[:, None] * (sm - m)
    # head: dV = g, dAdv[a', :] = g (delta(a' = a) - 1 / A)
    gWa2 = np.zeros((dm.sh, A, K))
    gba2 = np.zeros((A, K))
    np.add.at(gWa2.transpose(1, 0, 2), act, ha[:, :, None] * g[:, None, :])
    np.add.at(gba2, act, g)
    d_ha = np.einsum('nj,knj->nk', g, Wa2[:, act, :])
    grads = {}
    if dm.dueling:
        gWa2 -= (ha.T @ g)[:, None, :] / A
        gba2 -= g.sum(axis=0)[None, :] / A
        d_ha -= g @ Wbar.T
        grads['Wv2'], grads['bv2'] = hv.T @ g, g.sum(axis=0)
        d_hv = (g @ p['Wv2'].T) * (hv > 0)
        grads['Wv1'], grads['bv1'] = h2.T @ d_hv, d_hv.sum(axis=0)
    d_ha = d_ha * (ha > 0)
    grads['Wa2'], grads['ba2'] = gWa2.reshape(dm.sh, A * K), gba2.ravel()
    grads['Wa1'], grads['ba1'] = h2.T @ d_ha, d_ha.sum(axis=0)
    d_h2 = d_ha @ p['Wa1'].T + (d_hv @ p['Wv1'].T if dm.dueling else 0.0)
    d2 = d_h2 * (1.0 - h2 * h2)
    grads['W2'], grads['b2'] = h1.T @ d2, d2.sum(axis=0)
    d1 = (d2 @ p['W2'].T) * (1.0 - h1 * h1)
    grads['W1'], grads['b1'] = x.T @ d1, d1.sum(axis=0)
    qsa = (sm * dm.z).sum(axis=1)
    ez = (m * dm.z).sum(axis=1)
    stats = np.array([(w * td).sum(), qsa.sum(), ez.sum(), td.sum()])
    return dict(loss=(w * td).mean(), grad=join(grads, dm), td=td, m=m, qsa=qsa, astar=a_use, astar_ref=a_ref, boot=boot, gap=gap,
                stats=stats, g=g)


def loss_autograd(flat, m, obs, act, weights, dm, dtype=None):
    """torch autograd (float64 unless ``dtype``) of mean(w * cross-entropy) with the projected targets m held constant ->
    (loss, grad, td, Q(s)[a])."""
    import torch
    dtype = dtype or torch.float64
    t = lambda v: torch.as_tensor(np.asarray(v), dtype=dtype)
    prm = t(flat).clone().requires_grad_(True)
    p, o = {}, 0
    for name, shp in zip(NAMES, dm.shapes()):
        n = int(np.prod(shp))
        p[name] = prm[o:o + n].reshape(shp)
        o += n
    x = t(obs)
    h2 = torch.tanh(torch.tanh(x @ p['W1'] + p['b1']) @ p['W2'] + p['b2'])
    adv = (torch.relu(h2 @ p['Wa1'] + p['ba1']) @ p['Wa2'] + p['ba2']).reshape(len(x), dm.A, dm.atoms)
    if dm.dueling:
        v = torch.relu(h2 @ p['Wv1'] + p['bv1']) @ p['Wv2'] + p['bv2']
        logits = v[:, None, :] + adv - adv.mean(dim=1, keepdim=True)
    else:
        logits = adv
    idx = torch.as_tensor(np.asarray(act), dtype=torch.int64)
    la = logits[torch.arange(len(x)), idx]
    lsm = torch.log_softmax(la, dim=1)
    td = -(t(m) * lsm).sum(dim=1)
    w = torch.ones_like(td) if weights is None else t(weights)
    loss = (w * td).mean()
    loss.backward()
    qsa = (torch.softmax(la, dim=1) * t(dm.z)).sum(dim=1)
    return loss.item(), prm.grad.numpy(), td.detach().numpy(), qsa.detach().numpy()


def forward_torch(flat, obs, dm, dtype):
    """(p [N, A, atoms], Q [N, A]) by an eager torch forward in ``dtype`` (the fp32 yardstick of the error bars)."""
    import torch
    t = lambda v: torch.as_tensor(np.asarray(v), dtype=dtype)
    p = dict((k, t(v)) for k, v in split(np.asarray(flat), dm).items())
    x = t(obs)
    h2 = torch.tanh(torch.tanh(x @ p['W1'] + p['b1']) @ p['W2'] + p['b2'])
    adv = (torch.relu(h2 @ p['Wa1'] + p['ba1']) @ p['Wa2'] + p['ba2']).reshape(len(x), dm.A, dm.atoms)
    if dm.dueling:
        v = torch.relu(h2 @ p['Wv1'] + p['bv1']) @ p['Wv2'] + p['bv2']
        adv = v[:, None, :] + adv - adv.mean(dim=1, keepdim=True)
    pr = torch.softmax(adv, dim=2)
    return pr.numpy(), (pr * t(dm.z)).sum(dim=2).numpy()


# ---- n-step ---------------------------------------------------------------------------------------------------------------
def nstep_row(idx, rew_ring, T, B, n, gamma):
    """RLlib's adjust_nstep on complete episodes for ring rows ``idx`` (row order (slot * T + t) * B + b) ->
    (R float64, done, successor row or -1, k)."""
    idx = np.asarray(idx, dtype=np.int64)
    t = (idx % (T * B)) // B
    k = np.minimum(n, T - t)
    R = np.zeros(len(idx))
    for i, (r, kk) in enumerate(zip(idx, k)):
        disc, s = 1.0, 0.0
        for j in range(int(kk)):
            s += disc * float(rew_ring[r + j * B])
            disc *= gamma
        R[i] = s
    done = t + n >= T
    return R, done, np.where(done, -1, idx + k * B), k


# ---- exploration ----------------------------------------------------------------------------------------------------------
def softq_cdf(q, mask, temperature=1.0):
    """Inclusive prefix sums [N, A] of exp((Q - max) / temperature) over the allowed actions."""
    qm = masked_q(np.asarray(q, dtype=np.float64), mask)
    e = np.exp((qm - qm.max(axis=1, keepdims=True)) / temperature)
    if mask is not None:
        e = np.where(np.asarray(mask) > 0, e, 0.0)
    return np.cumsum(e, axis=1)


def softq_draw(cdf, u):
    """action = the smallest a with cdf[a] > u * total -> (action, distance of u to the nearest CDF edge in units of the total)"""
    total = cdf[:, -1]
    mass = np.asarray(u, dtype=np.float64) * total
    a = np.minimum((cdf <= mass[:, None]).sum(axis=1), cdf.shape[1] - 1)
    edges = np.concatenate([np.zeros((len(cdf), 1)), cdf], axis=1)
    rows = np.arange(len(cdf))
    dist = np.minimum(np.abs(mass - edges[rows, a]), np.abs(edges[rows, a + 1] - mass)) / np.where(total > 0, total, 1.0)
    return np.where(total > 0, a, 0), np.where(total > 0, dist, np.inf)        # a row that allows nothing: action 0, decided


# ---- optimiser ------------------------------------------------------------------------------------------------------------
def adam_clip_by_var(flat, m, v, t, grad, lr, var_clip, dm, beta1=0.9, beta2=0.999, eps=1e-8):
    """tf.clip_by_norm per variable (8, or 12 with dueling), then oracle.policy.adam_update -> (flat, m, v, t)."""
    g = np.array(grad, dtype=np.float64)
    lo = 0
    for hi in dm.ends():
        norm = np.sqrt((g[lo:hi] ** 2).sum())
        if var_clip > 0 and norm > var_clip:
            g[lo:hi] *= var_clip / norm
        lo = hi
    return OP.adam_update(flat, m, v, t, g, lr, beta1, beta2, eps)


def unpack_bits(bits, A):
    b = np.ascontiguousarray(bits).view(np.uint32)
    return ((b[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1).reshape(b.shape[0], -1)[:, :A].astype(np.float64)


# ---- shared test inputs ---------------------------------------------------------------------------------------------------
# (od, A, atoms, N, dueling, double_q, masked) -> (v_min, v_max, gamma_n, the reward R0 at which every b_j is an integer)
GPU_SHAPES = [
    (256, 284, 8, 1024, 1, 1, 0),         # the reference shape
    (256, 284, 8, 1003, 1, 1, 1),         # N off the tile
    (256, 50, 5, 517, 1, 0, 0),           # A not a multiple of 32, odd atom count
    (100, 75, 51, 333, 0, 1, 1),          # no value stream, classic 51 atoms, narrow obs
    (256, 284, 2, 77, 1, 1, 0),           # the smallest support
]
CASE_SEEDS = [0, 0, 0, 0, 2]            # (seed 0 of the last shape leaves 1 of its 62 bootstrapping rows under the gap bar: 1.6 %)
# Max errors of fp32_yardstick (an fp32 eager-torch CPU forward / backward) on these very inputs: Q abs, td abs, gradient relative to
# the reference gradient's max-norm.  The GPU tests' bars are BAR_FACTOR x these (the accumulation order differs between
# implementations); the a* / greedy gap bar is ten times the Q bar.
MEASURED = [dict(q=2.84e-4, td=1.10e-6, grad_rel=8.29e-8), dict(q=3.17e-4, td=8.91e-7, grad_rel=7.33e-8),
            dict(q=2.68e-6, td=9.95e-7, grad_rel=2.05e-7), dict(q=5.92e-7, td=9.88e-7, grad_rel=1.13e-6),
            dict(q=3.78e-4, td=4.30e-7, grad_rel=4.25e-7)]
BAR_FACTOR = 4.0
SUPPORT = {8: (0.0, 1000.0, 1.0, 0.0), 5: (-2.0, 6.0, 1.0, 0.0), 51: (-2.0, 6.0, 0.5, -1.0), 2: (0.0, 1000.0, 1.0, 0.0)}


def pack_bits(mask):
    N, A = mask.shape
    bits = np.zeros((N, (A + 31) // 32), dtype=np.uint32)
    for k in range(A):
        bits[:, k >> 5] |= (mask[:, k].astype(np.uint32) << np.uint32(k & 31))
    return bits.view(np.int32)


RELU_MARGIN = 1e-5


def relu_margin(flat, obs, dm):
    """Per row: the smallest |pre-activation| over the units of the two relu stream layers (float64)."""
    p = split(np.asarray(flat, dtype=np.float64), dm)
    x = np.asarray(obs, dtype=np.float64)
    h2 = np.tanh(np.tanh(x @ p['W1'] + p['b1']) @ p['W2'] + p['b2'])
    m = np.abs(h2 @ p['Wa1'] + p['ba1']).min(axis=1)
    if dm.dueling:
        m = np.minimum(m, np.abs(h2 @ p['Wv1'] + p['bv1']).min(axis=1))
    return m


def make_case(shape, seed=0, trunk=256, sh=128, support=None, margin=None):
    """Inputs of one loss / gradient case.  Rewards: a fifth of the rows sit where every b_j is an exact integer (R0 and R0 + dz;
    with gamma_n 0.5 every other j), some exceed v_max, some are below v_min, the rest spread over the support.  In the masked
    cases one non-terminal successor allows nothing (row ``k``).  ``support`` = (v_min, v_max, gamma_n, R0), default SUPPORT[atoms];
    ``margin``: how far every stream pre-activation of s stays from 0, default RELU_MARGIN.  A one-row case is set by hand: the
    row bootstraps and its reward is R0 + dz."""
    from rl4rs_amd.nets.distq import init_distq_params
    od, A, atoms, N, dueling, double_q, masked = shape
    v_min, v_max, gamma_n, r0 = SUPPORT[atoms] if support is None else support
    margin = RELU_MARGIN if margin is None else margin
    dm = Dims(od, A, atoms, trunk, sh, bool(dueling), v_min, v_max)
    rs = np.random.RandomState(N + A + atoms + seed)
    n = dm.n_params()
    flat = init_distq_params(od, A, atoms, trunk, sh, bool(dueling), seed=1) + (rs.randn(n) * 0.03).astype(np.float32)
    tflat = flat + (rs.randn(n) * 0.02).astype(np.float32)
    obs, nobs = rs.randn(N, od).astype(np.float32), rs.randn(N, od).astype(np.float32)
    # the loss is not differentiable where a stream unit's pre-activation is 0, and fp32 decides the sign of a value within its
    # rounding of 0 either way: rows of s with such a unit are drawn again (RELU_MARGIN exceeds 4 x the largest fp32 error of these
    # pre-activations, which fp32_yardstick measures at 1.9e-6 on GPU_SHAPES; a wider trunk passes its own margin, shape_margin)
    while True:
        near = relu_margin(flat, obs, dm) < margin
        if not near.any():
            break
        obs[near] = rs.randn(int(near.sum()), od).astype(np.float32)
    mask = (rs.rand(N, A) < 0.4).astype(np.int64)
    mask[np.arange(N), rs.randint(0, A, size=N)] = 1
    done = (rs.rand(N) < 0.15).astype(np.int32)
    done[-1] = 1
    if N == 1:
        done[0] = 0
    k = int(np.nonzero(done == 0)[0][0])
    if masked:
        mask[k] = 0
    else:
        mask = None
    span = v_max - v_min
    rew = (v_min + (rs.rand(N) * 1.2 - 0.1) * span * 0.5).astype(np.float32)
    kind = rs.rand(N)
    rew[kind < 0.1] = r0
    rew[(kind >= 0.1) & (kind < 0.2)] = r0 + dm.dz
    rew[(kind >= 0.2) & (kind < 0.25)] = v_max + 0.3 * span
    rew[(kind >= 0.25) & (kind < 0.3)] = v_min - 0.2 * span - 1.0
    if N == 1:
        rew[0] = r0 + dm.dz
    act = rs.randint(0, A, size=N).astype(np.int32)
    w = (rs.rand(N) + 0.1).astype(np.float32)
    return dict(dm=dm, flat=flat, tflat=tflat, obs=obs, nobs=nobs, mask=mask, bits=None if mask is None else pack_bits(mask), done=done,
                act=act, rew=rew, w=w, k=k, gamma_n=gamma_n, double_q=bool(double_q), masked=bool(masked), N=N, margin=margin)


def fp32_yardstick(c):
    """Max errors of an fp32 eager-torch CPU forward / backward of the restatement against the float64 restatement on the inputs
    of case ``c`` -> dict(q, pre, td, grad_rel, left_out, td_max): Q(s') abs, the advantage stream's pre-activations abs, td abs,
    gradient relative to the reference gradient's max-norm, the fraction of bootstrapping rows whose float64 top-two gap is under
    ten times the Q bar, and the largest float64 |td| (the scale of the td figure)."""
    import torch
    dm = c['dm']
    ref = loss_and_grad(c['flat'], c['tflat'], c['obs'], c['act'], c['rew'], c['done'], c['nobs'], c['mask'], c['w'], c['gamma_n'],
                        c['double_q'], dm)
    nobs = np.where(c['done'][:, None] != 0, 0.0, c['nobs']).astype(np.float32)
    q64 = forward(c['flat'] if c['double_q'] else c['tflat'], nobs, dm)[2]
    q32 = forward_torch(c['flat'] if c['double_q'] else c['tflat'], nobs, dm, torch.float32)[1]
    p32 = forward_torch(c['tflat'], nobs, dm, torch.float32)[0]
    m32 = project(c['rew'], ref['boot'], p32[np.arange(c['N']), ref['astar']], c['gamma_n'], dm, dtype=np.float32)
    _, g32, td32, _ = loss_autograd(c['flat'], m32, c['obs'], c['act'], c['w'], dm, dtype=torch.float32)
    q_err = float(np.abs(q32 - q64).max())
    p32 = dict((k, torch.as_tensor(v, dtype=torch.float32)) for k, v in split(np.asarray(c['flat']), dm).items())
    x32 = torch.as_tensor(c['obs'], dtype=torch.float32)
    pre32 = (torch.tanh(torch.tanh(x32 @ p32['W1'] + p32['b1']) @ p32['W2'] + p32['b2']) @ p32['Wa1'] + p32['ba1']).numpy()
    p64 = split(np.asarray(c['flat'], dtype=np.float64), dm)
    pre64 = hidden(p64, c['obs'].astype(np.float64), dm)[1] @ p64['Wa1'] + p64['ba1']
    boot = ref['boot']
    left = float((boot & (ref['gap'] < 10.0 * BAR_FACTOR * q_err)).sum()) / max(1, int(boot.sum()))
    return dict(q=q_err, pre=float(np.abs(pre32 - pre64).max()), td=float(np.abs(td32 - ref['td']).max()), grad_rel=float(np.abs(g32 - ref['grad']).max() / np.abs(ref['grad']).max()),
                left_out=left, td_max=float(np.abs(ref['td']).max()))


# ---- cases off the one net width ---------------------------------------------------------------------------------------------
# ((od, A, atoms, N, dueling, double_q, masked, trunk, sh), (v_min, v_max, gamma_n, R0)): the ends of what rl4rs_distq_create admits
SHAPE_CASES = [
    ((24, 2, 64, 33, 1, 1, 0, 32, 32), (0.0, 1000.0, 1.0, 0.0)),       # A = 2, atoms = 64, narrowest net, one row in a second head tile
    ((100, 512, 3, 65, 1, 1, 1, 64, 256), (-2.0, 6.0, 1.0, 0.0)),      # A = 512, widest stream, AP = 4 with an idle lane, masked
    ((2048, 65, 33, 31, 0, 0, 1, 1024, 64), (-2.0, 6.0, 0.5, -1.0)),   # widest obs and trunk, atoms = 33, no value stream, target picks a*
    ((40, 130, 16, 1, 1, 1, 0, 96, 96), (0.0, 1000.0, 1.0, 0.0)),      # one row, AT == AP, widths that are no power of two
    ((8, 4, 2, 16500, 1, 1, 0, 32, 32), (0.0, 1000.0, 1.0, 0.0)),      # more than 64 chunks of 256 rows: the re-chunked reductions
]
SHAPE_SEEDS = [0, 0, 1, 0, 0]           # (seed 0 of the third case draws no reward above v_max among its 31 rows)
YARD_SEEDS = (0, 1, 2)
# shape_yardstick of every case: the worst of fp32_yardstick over YARD_SEEDS (a single row can land on its float64 value by luck),
# no figure counted for less than one fp32 rounding (2^-24) of the quantity's scale: max |z| for Q, max(1, |td|) for td, 1 for the
# relative gradient error.  Bars as for MEASURED: BAR_FACTOR x these.  ``pre``: the error of the advantage stream's pre-activations.
MEASURED_SHAPES = [dict(q=9.25e-5, td=1.54e-6, grad_rel=9.19e-7, pre=5.24e-7), dict(q=1.17e-6, td=4.18e-7, grad_rel=3.02e-7, pre=5.39e-7),
                   dict(q=5.98e-7, td=9.58e-7, grad_rel=1.25e-6, pre=3.25e-6), dict(q=1.25e-4, td=1.90e-7, grad_rel=1.54e-6, pre=3.49e-7),
                   dict(q=2.12e-4, td=4.46e-7, grad_rel=5.96e-8, pre=5.79e-7)]
U32 = 2.0 ** -24


def shape_margin(i):
    """RELU_MARGIN rests on a 1.9e-6 pre-activation error; a 1024-wide trunk measures more, so every case keeps its stream
    pre-activations 4 x its own measured error away from 0 (never less than RELU_MARGIN)."""
    return max(RELU_MARGIN, 4.0 * MEASURED_SHAPES[i]['pre'])


def shape_case(i, seed=None, margin=None):
    shape, support = SHAPE_CASES[i]
    return make_case(shape[:7], SHAPE_SEEDS[i] if seed is None else seed, trunk=shape[7], sh=shape[8], support=support,
                     margin=shape_margin(i) if margin is None else margin)


def shape_yardstick(i, margin=None):
    """-> dict(q, td, grad_rel, pre): the worst of fp32_yardstick over YARD_SEEDS with the floors stated at MEASURED_SHAPES"""
    out = dict(q=0.0, td=0.0, grad_rel=0.0, pre=0.0)
    for seed in YARD_SEEDS:
        c = shape_case(i, seed, margin)
        y = fp32_yardstick(c)
        td_scale = max(1.0, y['td_max'])
        floors = dict(q=U32 * float(np.abs(c['dm'].z).max()), td=U32 * td_scale, grad_rel=U32, pre=0.0)
        out = dict((k, max(out[k], y[k], floors[k])) for k in out)
    return out


def softq_edge_bar(q_bar, temperature):
    """How far (in units of the total) u must stay from a CDF edge for the draw to be decided.  The normalised prefix is
    c = sum_{i <= a} e_i / sum_i e_i with e_i = exp((Q_i - max) / T); the max is a common factor and cancels.  Q errors up to eps
    multiply every e_i by a factor in [exp(-eps / T), exp(eps / T)], which moves c by at most c (1 - c) (exp(2 eps / T) - 1)
    <= 0.55 eps / T for eps / T < 0.1; 1e-5 covers the fp32 rounding of up to 512 terms of the prefix sum itself."""
    assert q_bar / temperature < 0.1
    return 0.55 * q_bar / temperature + 1e-5
