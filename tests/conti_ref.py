"""Crafted inputs and float64 references for the continuous learners' networks and loss kernels away from their default shape
(csrc/contirl.hpp, csrc/amlp_fused.hpp), shared by tests/test_conti_shapes_host.py (no GPU: proves what the inputs are built to
show) and tests/test_gpu_conti_shapes.py (the device against these references).

Every leaf reference is a few lines of numpy written from the formulas in the kernels' header comments, with the arithmetic type
as a parameter: float64 is the reference, the SAME function in float32 on the very inputs of a case is the case's yardstick
(what rounding alone does to the result).  A GPU comparison that has no fixed project bar allows BAR_FACTOR x that yardstick
(the device adds in another order), with a floor of a few fp32 roundings of the result's scale so that a yardstick that happens
to be exact does not demand bit equality.  The network reference is oracle.offline_conti.OracleAMLP (float64, and float32 as
the yardstick)."""
import functools

import numpy as np

BAR_FACTOR = 4.0                      # the project's factor between an fp32 yardstick and a device bar (tests/exactk_ref.py)
FLOOR = 4.0 * 2.0 ** -23              # x the result's scale: a few fp32 roundings
LO, HI = -20.0, 2.0                   # the logstd clamp of ConditionalVAE / SquashedNormalPolicy


def bar(yardstick, scale):
    return max(BAR_FACTOR * yardstick, FLOOR * scale)


def err_scale(got, want):
    """(max |got - want|, max |want|) in float64"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max()), float(np.abs(want).max())


# ---------------------------------------------------------------------------------------------------------------- networks (A1 - A3)
# (obs_dim, act_dim, out_dim, head_act, rows): what each reaches is in the docstring of tests/test_gpu_conti_shapes.py
AMLP_CASES = [
    (10, 5, 3, 'none', 5), (59, 5, 1, 'none', 1), (60, 5, 7, 'tanh', 9), (37, 0, 33, 'relu', 6), (40, 64, 64, 'sigmoid', 12),
    (40, 33, 2, 'elu', 11), (300, 1, 1, 'none', 3), (1400, 8, 4, 'none', 5), (4064, 32, 1, 'none', 5), (4065, 32, 1, 'none', 5),
    (266, 32, 1, 'none', 1), (266, 32, 1, 'none', 3), (266, 32, 1, 'none', 1024), (266, 32, 1, 'none', 1025),
    (266, 32, 1, 'none', 2048), (266, 32, 1, 'none', 2049), (266, 32, 32, 'tanh', 1025),
]


def amlp_id(c):
    return '%dx%dx%d-%s-N%d' % c


def amlp_wide(c):
    """first-layer sums longer than the 300 the project's own bars were set for: the yardstick decides"""
    return c[0] + c[1] > 300


def amlp_params(D, E, K, seed, heads=1, scale=1.0):
    """init_amlp_params with the biases moved off zero (a wrong bias index is invisible otherwise), as tests/test_gpu_amlp_h16.py"""
    from rl4rs_amd.offline_rl import init_amlp_params
    p = init_amlp_params(D, E, K, seed=seed, heads=heads)
    rs = np.random.RandomState(seed + 7919)
    for k in ('fc1_b', 'fc2_b', 'head_b'):
        p[k] = (0.1 * rs.standard_normal(p[k].shape)).astype(np.float32)
    if scale != 1.0:
        p = dict((k, (v * np.float32(scale)).astype(np.float32)) for k, v in p.items())
    return p


def unflat(v, D, E, K, H=256):
    out, o = {}, 0
    for k, shape in (('fc1_w', (D + E, H)), ('fc1_b', (H,)), ('fc2_w', (H, H)), ('fc2_b', (H,)), ('head_w', (H, K)), ('head_b', (K,))):
        n = int(np.prod(shape))
        out[k] = np.asarray(v[o:o + n]).reshape(shape)
        o += n
    return out


def head_dpre(w, o, head_act):
    """gradient wrt the head's PRE-activation given the gradient w wrt its output o (the device backward takes the former)"""
    if head_act == 'tanh':
        return w * (1.0 - o * o)
    if head_act == 'sigmoid':
        return w * o * (1.0 - o)
    if head_act == 'relu':
        return w * (o > 0)
    if head_act == 'elu':
        return w * np.where(o > 0, 1.0, o + 1.0)
    return w


def amlp_inputs(D, E, K, N, seed):
    """unit-scale observations, actions of half that, and the weights w of the scalar sum(out * w) that is differentiated"""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((N, D)).astype(np.float32)
    a = (0.5 * rs.standard_normal((N, E))).astype(np.float32) if E else None
    w = rs.standard_normal((N, K)).astype(np.float32)
    return x, a, w


def amlp_eval(params, head_act, x, a, w, dtype):
    """forward, every parameter gradient and the action-input gradient of sum(out * w), all in ``dtype`` on the CPU"""
    import torch
    from oracle.offline_conti import OracleAMLP
    net = OracleAMLP(params, head_act, dtype=dtype)
    at = torch.tensor(a, dtype=dtype, requires_grad=True) if a is not None else None
    out = net(x, at)
    (out * torch.as_tensor(w, dtype=dtype)).sum().backward()
    r = dict(out=out.detach().numpy().astype(np.float64), grads=dict((k, np.asarray(v, np.float64)) for k, v in net.grads().items()))
    r['dact'] = at.grad.numpy().astype(np.float64) if a is not None else None
    return r


@functools.lru_cache(maxsize=None)
def amlp_case(case):
    """inputs, float64 reference and float32 yardstick of one AMLP_CASES row (computed once, shared, never written to)"""
    import torch
    D, E, K, head_act, N = case
    seed = 1000 + AMLP_CASES.index(case)
    params = amlp_params(D, E, K, seed)
    x, a, w = amlp_inputs(D, E, K, N, seed + 1)
    ref = amlp_eval(params, head_act, x, a, w, torch.float64)
    f32 = amlp_eval(params, head_act, x, a, w, torch.float32)
    yard = dict(out=err_scale(f32['out'], ref['out']))
    for k in ref['grads']:
        yard[k] = err_scale(f32['grads'][k], ref['grads'][k])
    if E:
        yard['dact'] = err_scale(f32['dact'], ref['dact'])
    dpre = np.ascontiguousarray(head_dpre(w.astype(np.float64), ref['out'], head_act), np.float32)
    return dict(params=params, x=x, a=a, w=w, dpre=dpre, ref=ref, yard=yard)


def stale_pair(seed=77):
    """A3: two unrelated parameter draws of the (266, 32, 1) critic - P1 from another seed and scaled by -1.5 - so that a backward
    through P0's transposed weights under P1's parameters is wrong by O(1), not by rounding"""
    return amlp_params(266, 32, 1, seed), amlp_params(266, 32, 1, seed + 1, scale=-1.5)


# ------------------------------------------------------------------------------------------------------- leaf formulas (A5), by dtype
def _c(dt, *xs):
    return [None if x is None else np.asarray(x, dt) for x in xs]


def cvae(enc, eps, y, a, dz, beta, dt):
    """ConditionalVAE: z = mu + exp(clamp(logstd)) eps; loss2 = {mean_n sum_e (y - a)^2, mean_n sum_l KL(N(mu, sigma) || N(0, 1))};
    d_dec = d mse / d(pre-tanh decoder output) = 2 (y - a)(1 - y^2) / (N E); d_enc = gradient wrt [mu | logstd] given dz, with
    beta * mean KL: dz + k mu | [lo <= raw <= hi] (dz eps sigma + k (sigma^2 - 1)), k = beta / (N L)"""
    enc, eps, y, a, dz = _c(dt, enc, eps, y, a, dz)
    N, L = eps.shape
    E = y.shape[1]
    mu, raw = enc[:, :L], enc[:, L:]
    ls = np.clip(raw, dt(LO), dt(HI))
    sig = np.exp(ls)
    z = mu + sig * eps
    d = y - a
    kl = dt(0.5) * (np.exp(dt(2) * ls) + mu * mu - dt(1)) - ls
    loss2 = np.array([(d * d).sum(axis=1).sum() / dt(N), kl.sum(axis=1).sum() / dt(N)], dt)
    d_dec = (dt(2) / (dt(N) * dt(E))) * d * (dt(1) - y * y)
    k = dt(beta) / (dt(N) * dt(L))
    inside = (raw >= dt(LO)) & (raw <= dt(HI))
    d_enc = np.concatenate([dz + k * mu, np.where(inside, dz * eps * sig + k * (sig * sig - dt(1)), dt(0))], axis=1)
    return dict(z=z, mse=loss2[:1], kl=loss2[1:], d_dec=d_dec, d_enc=d_enc), inside


CVAE_CASES = [(N, E, L, beta) for (N, E, L) in ((1, 5, 7), (4, 64, 64), (257, 70, 3), (1000, 32, 130)) for beta in (0.5, 0.0)]


def logstd_with_clamped(rs, shape):
    """logstd values of which about a fifth lie outside [LO, HI], on both sides"""
    ls = rs.uniform(-4.0, 1.5, size=shape)
    u = rs.rand(*shape)
    ls = np.where(u < 0.1, rs.uniform(-30.0, -20.5, size=shape), ls)
    ls = np.where(u > 0.9, rs.uniform(2.25, 6.0, size=shape), ls)
    if ls.size >= 2:                              # (both sides also in the smallest case)
        ls.flat[0], ls.flat[ls.size - 1] = -24.5, 3.5
    return ls.astype(np.float32)


def cvae_inputs(N, E, L, beta):
    rs = np.random.RandomState(N * 131 + E * 7 + L)
    enc = np.concatenate([rs.standard_normal((N, L)).astype(np.float32), logstd_with_clamped(rs, (N, L))], axis=1)
    eps = rs.standard_normal((N, L)).astype(np.float32)
    y = np.tanh(rs.standard_normal((N, E))).astype(np.float32)
    a = rs.uniform(-1, 1, (N, E)).astype(np.float32)
    dz = (rs.standard_normal((N, L)) / N).astype(np.float32)
    return dict(enc=np.ascontiguousarray(enc), eps=eps, y=y, a=a, dz=dz, beta=beta)


def critic_mse(q1, q2, y, dt):
    """loss2 = {mean (q1 - y)^2, mean (q2 - y)^2}; dq_c = 2 (q_c - y) / N"""
    q1, q2, y = _c(dt, q1, q2, y)
    N = y.size
    d1, d2 = q1 - y, q2 - y
    return dict(loss2=np.array([(d1 * d1).sum() / dt(N), (d2 * d2).sum() / dt(N)], dt), dq1=dt(2) / dt(N) * d1, dq2=dt(2) / dt(N) * d2)


CRITIC_MSE_N = (1, 255, 257, 1000)


def critic_mse_inputs(N):
    rs = np.random.RandomState(300 + N)
    return dict(q1=(3 * rs.standard_normal(N)).astype(np.float32), q2=(3 * rs.standard_normal(N)).astype(np.float32),
                y=(2 + 3 * rs.standard_normal(N)).astype(np.float32))


def squashed(head, eps, rep, dt):
    """SquashedNormalPolicy: u = mu + exp(clamp(logstd)) eps, a = tanh(u),
    logp = sum_e [-eps^2 / 2 - logstd - log sqrt(2 pi) - 2 (log 2 - u - softplus(-2u))]; eps None: a = tanh(mu)"""
    head, eps = _c(dt, head, eps)
    A = head.shape[1] // 2
    mu = np.repeat(head[:, :A], rep, axis=0)
    if eps is None:
        return dict(act=np.tanh(mu))
    ls = np.repeat(np.clip(head[:, A:], dt(LO), dt(HI)), rep, axis=0)
    u = mu + np.exp(ls) * eps
    m2u = dt(-2) * u
    softplus = np.maximum(m2u, dt(0)) + np.log1p(np.exp(-np.abs(m2u)))
    terms = dt(-0.5) * eps * eps - ls - dt(0.5 * np.log(2 * np.pi)) - dt(2) * (dt(np.log(2.0)) - u - softplus)
    return dict(act=np.tanh(u), logp=terms.sum(axis=1))


SQUASHED_A = (1, 5, 64, 65, 130)
SQUASHED_B = 9


def squashed_inputs(A, rep):
    rs = np.random.RandomState(500 + 10 * A + rep)
    head = np.concatenate([rs.standard_normal((SQUASHED_B, A)).astype(np.float32), logstd_with_clamped(rs, (SQUASHED_B, A))], axis=1)
    return dict(head=np.ascontiguousarray(head), eps=rs.standard_normal((SQUASHED_B * rep, A)).astype(np.float32))


def sac_actor_grad(head, eps, act, g_a, log_temp, dt):
    """dL/du = T 2 a / B + g_a (1 - a^2); d_head = [dL/du | [lo <= raw <= hi] (dL/du sigma eps - T / B)], T = exp(log_temp)"""
    head, eps, act, g_a = _c(dt, head, eps, act, g_a)
    B, A = act.shape
    T, inv_b = np.exp(dt(log_temp)), dt(1) / dt(B)
    raw = head[:, A:]
    sig = np.exp(np.clip(raw, dt(LO), dt(HI)))
    du = T * dt(2) * act * inv_b + g_a * (dt(1) - act * act)
    inside = (raw >= dt(LO)) & (raw <= dt(HI))
    return dict(d_head=np.concatenate([du, np.where(inside, du * sig * eps - T * inv_b, dt(0))], axis=1)), inside


SAC_CASES = [(1, 5), (300, 65)]


def sac_inputs(B, A):
    rs = np.random.RandomState(700 + B + A)
    head = np.concatenate([rs.standard_normal((B, A)).astype(np.float32), logstd_with_clamped(rs, (B, A))], axis=1)
    return dict(head=np.ascontiguousarray(head), eps=rs.standard_normal((B, A)).astype(np.float32),
                act=np.tanh(rs.standard_normal((B, A))).astype(np.float32), g_a=(rs.standard_normal((B, A)) / B).astype(np.float32),
                log_temp=-0.25)


def twin_min_inputs(B):
    """a tenth of the rows (at least one) exactly tied: ties select q1"""
    rs = np.random.RandomState(900 + B)
    q1 = rs.standard_normal(B).astype(np.float32)
    q2 = rs.standard_normal(B).astype(np.float32)
    tied = np.arange(B) % 10 == 0
    q2[tied] = q1[tied]
    return q1, q2, tied


def twin_min(q1, q2):
    """(min, dq1, dq2) with dq_c = -1 / B on the smaller one, q1 on ties: every value is one correctly rounded fp32 operation"""
    B = q1.size
    first = q1 <= q2
    g = np.float32(-1.0) / np.float32(B)
    return np.where(first, q1, q2), np.where(first, g, np.float32(0)), np.where(first, np.float32(0), g)


def cql_critic(q1, q2, offs, m, y, aw, dt):
    """rows [B][m], column 0 the dataset action: sums = {sum_b (q_c[b,0] - y_b)^2 (c = 1, 2), sum_b logsumexp_{j >= 1}(q_c[b,j] -
    offs[b,j]), sum_b q_c[b,0]};  dq_c[b,0] = 2 (q_c[b,0] - y_b) / B - k, dq_c[b,j] = k softmax_j, k = aw / (2 B).  y None: y = 0,
    sums only"""
    q1, q2, offs, y = _c(dt, q1, q2, offs, y)
    B = q1.size // m
    out, td, lse, q0 = {}, [], [], []
    k = dt(0 if aw is None else aw) / (dt(2) * dt(B))
    for name, q in (('dq1', q1), ('dq2', q2)):
        q = q.reshape(B, m)
        x = q[:, 1:] - offs.reshape(B, m)[:, 1:]
        mx = x.max(axis=1, keepdims=True)
        l = mx[:, 0] + np.log(np.exp(x - mx).sum(axis=1))
        d0 = q[:, 0] - (y if y is not None else dt(0))
        td.append((d0 * d0).sum())
        lse.append(l.sum())
        q0.append(q[:, 0].sum())
        if y is not None:
            out[name] = np.concatenate([(dt(2) * d0 / dt(B) - k)[:, None], k * np.exp(x - l[:, None])], axis=1).reshape(-1)
    out.update(td=np.array(td, dt), lse=np.array(lse, dt), q0=np.array(q0, dt))
    return out


CQL_CASES = [(1, 2, False), (5, 64, False), (5, 65, False), (5, 66, False), (300, 31, False), (257, 130, False), (5, 66, True)]
CQL_OVERFLOW_ROWS = ((0, 95.0), (3, 95.0), (2, -95.0))       # (row, level of q - offs) of the last case


def cql_inputs(B, m, overflow):
    """offsets of the size the learner produces: 0 for the dataset action, log-probabilities in [-40, 10] for the policy samples,
    A log 0.5 (A = 32) for the uniform third.  ``overflow``: rows whose q - offs sit near +-95, where exp leaves fp32 unless the row
    maximum is subtracted first"""
    rs = np.random.RandomState(1100 + 7 * B + m + (50 if overflow else 0))
    q1 = (3 * rs.standard_normal((B, m))).astype(np.float32)
    q2 = (3 * rs.standard_normal((B, m))).astype(np.float32)
    offs = rs.uniform(-40.0, 10.0, size=(B, m)).astype(np.float32)
    offs[:, 1 + 2 * ((m - 1) // 3):] = np.float32(32 * np.log(0.5))
    offs[:, 0] = 0.0
    if overflow:
        for row, level in CQL_OVERFLOW_ROWS:
            offs[row, 1:] = rs.uniform(-2.0, 2.0, size=m - 1).astype(np.float32)
            q1[row, 1:] = (level + rs.uniform(-1.0, 1.0, size=m - 1)).astype(np.float32)
            q2[row, 1:] = (level + rs.uniform(-1.0, 1.0, size=m - 1)).astype(np.float32)
    y = (2 + 3 * rs.standard_normal(B)).astype(np.float32)
    return dict(q1=q1.reshape(-1), q2=q2.reshape(-1), offs=offs.reshape(-1), m=m, y=y, aw=3.5)


def naive_lse32(q, offs, B, m):
    """float32 log(sum(exp(x))) WITHOUT the row maximum (what the kernel must not compute)"""
    x = (np.asarray(q, np.float32).reshape(B, m) - np.asarray(offs, np.float32).reshape(B, m))[:, 1:]
    with np.errstate(over='ignore', divide='ignore'):
        return np.log(np.exp(x).sum(axis=1, dtype=np.float32))


# ----------------------------------------------------------------------------------------------- exact cases: the BCQ target's tie rule
BCQ_TARGET_CASES = [(B, n, lam, twin) for (B, n) in ((1, 1), (5, 64), (5, 65), (3, 100), (7, 200)) for lam in (0.75, 0.0)
                    for twin in (True, False)]
GAMMA = 0.5


def bcq_target_inputs(B, n, lam, twin):
    """values that are multiples of 1/8 in [-8, 8]: (1 - lam) max + lam min (lam 0.75 or 0) is then exact in fp32, and with rewards
    in multiples of 1/4 and gamma 1/2 so is y.  Every row's maximum is planted, twice where the pattern is a tie:
      'trip'  at j and j + 64      (one lane, a later trip of its loop)
      'lane'  at j1 < j2 with j2 % 64 < j1 % 64   (index order and lane order disagree in the cross-lane merge)
      'last'  at j = n - 1 only    (the last lane of a ragged trip)
      'near'  at j1 < j2 < 64      (n <= 64: two lanes of the only trip)
    The two planted twin-critic pairs differ ((8, 7) and (7, 8): the same mix); without q2 both are 8.  Everything else is <= 6."""
    rs = np.random.RandomState(2000 + 31 * B + n + (1 if twin else 0) + int(8 * lam))
    q1 = rs.randint(-64, 49, size=(B, n)).astype(np.float32) / 8
    q2 = rs.randint(-64, 49, size=(B, n)).astype(np.float32) / 8
    pattern, where = [], []
    for b in range(B):
        if n >= 65:
            kind = ('trip', 'lane', 'last')[b % 3]
        else:
            kind = ('near', 'last')[b % 2] if n > 1 else 'last'
        if kind == 'trip':
            j1 = int(rs.randint(0, n - 64))
            js = (j1, j1 + 64)
        elif kind == 'lane':
            j2 = int(rs.choice([j for j in range(64, n) if j % 64 < 63]))
            j1 = int(rs.randint(j2 % 64 + 1, 64))
            js = (j1, j2)
        elif kind == 'near':
            j1 = int(rs.randint(0, n - 1))
            js = (j1, int(rs.randint(j1 + 1, n)))
        else:
            js = (n - 1,)
        for i, j in enumerate(js):
            q1[b, j], q2[b, j] = ((8.0, 7.0), (7.0, 8.0))[i] if twin else (8.0, 8.0)
        pattern.append(kind)
        where.append(js)
    rew = rs.randint(0, 21, size=B).astype(np.float32) / 4
    ter = (np.arange(B) % 3 == 1).astype(np.float32)
    return dict(q1=q1.reshape(-1), q2=q2.reshape(-1) if twin else None, n=n, lam=lam, rew=rew, ter=ter, pattern=pattern, where=where)


def bcq_target(c, dt):
    """compute_max_with_n_actions: v_j = (1 - lam) max(q1, q2) + lam min(q1, q2) (q2 None: q1); best = the FIRST maximum;
    y = r + gamma v_best (1 - terminal)"""
    n = c['n']
    q1 = np.asarray(c['q1'], dt).reshape(-1, n)
    v = q1
    if c['q2'] is not None:
        q2 = np.asarray(c['q2'], dt).reshape(-1, n)
        v = (dt(1) - dt(c['lam'])) * np.maximum(q1, q2) + dt(c['lam']) * np.minimum(q1, q2)
    best = v.argmax(axis=1)                              # numpy: the first occurrence
    val = v[np.arange(v.shape[0]), best]
    return v, best.astype(np.int32), np.asarray(c['rew'], dt) + dt(GAMMA) * val * (dt(1) - np.asarray(c['ter'], dt))


# ------------------------------------------------------------------------------------------------------------------ yardstick table
def leaf_yardsticks():
    """{case id: {output: (float32 error, scale)}} of every A5 value comparison, on the very inputs the GPU test uses"""
    f32, f64 = np.float32, np.float64
    T = {}

    def put(key, a, b, names):
        T[key] = dict((k, err_scale(a[k], b[k])) for k in names)

    for case in CVAE_CASES:
        c = cvae_inputs(*case)
        args = (c['enc'], c['eps'], c['y'], c['a'], c['dz'], c['beta'])
        put('cvae-N%d-E%d-L%d-beta%g' % case, cvae(*args, f32)[0], cvae(*args, f64)[0], ('z', 'mse', 'kl', 'd_dec', 'd_enc'))
    for N in CRITIC_MSE_N:
        c = critic_mse_inputs(N)
        put('critic_mse-N%d' % N, critic_mse(c['q1'], c['q2'], c['y'], f32), critic_mse(c['q1'], c['q2'], c['y'], f64), ('loss2', 'dq1', 'dq2'))
    for A in SQUASHED_A:
        for rep in (1, 3):
            c = squashed_inputs(A, rep)
            put('squashed-A%d-rep%d' % (A, rep), squashed(c['head'], c['eps'], rep, f32), squashed(c['head'], c['eps'], rep, f64), ('act', 'logp'))
        put('squashed-A%d-mean' % A, squashed(c['head'], None, 1, f32), squashed(c['head'], None, 1, f64), ('act',))
    for case in SAC_CASES:
        c = sac_inputs(*case)
        args = (c['head'], c['eps'], c['act'], c['g_a'], c['log_temp'])
        put('sac_actor_grad-B%d-A%d' % case, sac_actor_grad(*args, f32)[0], sac_actor_grad(*args, f64)[0], ('d_head',))
    for case in CQL_CASES:
        c = cql_inputs(*case)
        for with_y in (True, False):
            args = (c['q1'], c['q2'], c['offs'], c['m'], c['y'] if with_y else None, c['aw'] if with_y else None)
            put(cql_id(case, with_y), cql_critic(*args, f32), cql_critic(*args, f64), ('td', 'lse', 'q0') + (('dq1', 'dq2') if with_y else ()))
    return T


def cql_id(case, with_y):
    return 'cql-B%d-m%d%s%s' % (case[0], case[1], '-overflow' if case[2] else '', '' if with_y else '-sums')


def amlp_yardsticks():
    """{case id: {output: (float32 error, scale)}} of the A1 network cases"""
    return dict((amlp_id(c), amlp_case(c)['yard']) for c in AMLP_CASES)
