"""GPU: the Gaussian actor-critic handle (rl4rs_gpolicy_*, rl4rs_amd.device.DeviceGaussPolicy) and ContiTrainer against the float64
restatement in tests/gauss_ref.py.

Bars (the tree's rule for restated learners, tests/dynamics_ref.py / exactk_ref.py): the restatement itself is run in float32 on the
CPU, and a quantity's bar is 4 x its worst float32 deviation from the float64 run at that shape; 4 is the standing margin for another
summation order (MFMA tiles against torch's dot products).  "At that shape" means over every row count the shape is tested at: a row's
forward does not depend on the rows beside it, and a single scalar (a statistic of a 1-row call, the gradient of the one-element block
c3) can sit on its float64 value in float32 by luck, so the worst over the row counts is the honest measure of what float32 costs
there (the 3072-wide shape runs on the device at 33 rows only; its yardstick is taken at 1, 5 and 33).  For the same reason no
yardstick figure counts for less than one float32 rounding of the quantity's scale, 2^-24 relative: a float32 result is not defined
more finely than that, and a float32 run that lands closer to the float64 value did so by luck.  Gradients are held relative to the
reference gradient's max-norm per parameter block, statistics relative to max(1, |reference|) per row.  Each test prints the
device's error beside its bar.

Shapes beside the default ones: D = 260 and D = 515 leave k_gp_fwd's last 256-column staging pass with 4 and 3 columns (1 and 33
rows; tests/test_gauss_host.py shows that a dropped pass would miss the bars by far); the 4099-row batch of the (40, 64, 3) shape
makes the loss's gradient reductions take 320-row chunks, its yardstick taken at its own row count."""
import functools

import numpy as np
import pytest
import torch

import gauss_ref as R
import vtrace_ref as VR

pytestmark = pytest.mark.gpu

SHAPES = [(256, 256, 32), (40, 64, 3), (7, 128, 1), (3072, 256, 32), (256, 256, 64), (260, 64, 3), (515, 128, 5)]
ROWS = (1, 5, 33, 256, 257)
RAGGED = (260, 515)                    # obs widths whose last 256-column staging pass of k_gp_fwd is a ragged one (4 and 3 columns)
BIG = ((40, 64, 3), 4099)              # a batch whose gradient reductions take 320-row chunks (64 up to 1024 rows)
SEED, STEP = 12345, 7
F32, F64 = torch.float32, torch.float64


U32 = 2.0 ** -24                       # one float32 rounding, relative: the least a yardstick figure counts for


def _rows(dims):
    return (33,) if dims[0] == 3072 else (1, 33) if dims[0] in RAGGED else ROWS


def _yard_rows(dims, rows=0):
    """the row counts the float32 yardstick of a shape is taken over (``rows``: of a batch that is a case of its own)"""
    return (rows,) if rows else (1, 5, 33) if dims[0] == 3072 else _rows(dims)


CASES = [(dims, N) for dims in SHAPES for N in _rows(dims)]
_id = lambda c: 'D%d-H%d-E%d-N%d' % (c[0] + (c[1],))


def _np(t):
    return t.detach().cpu().numpy()


def _cuda(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(device='cuda', dtype=dtype).contiguous()


def _policy(dims, flat, max_rows=257):
    from rl4rs_amd.device import DeviceGaussPolicy
    D, H, E = dims
    return DeviceGaussPolicy(D, E, max_rows=max_rows, hidden=H, params=flat)


def _dev(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


@functools.lru_cache(maxsize=None)
def _base(dims, rows=0):
    """Parameters, observations and the forward's reference for the largest row count of a shape (smaller calls take its first rows;
    ``rows``: for a batch of that many rows instead, a case of its own);
    the float32 run of the same rows gives the forward bars.  logp is compared on GIVEN actions (the float64 draw rounded to float32):
    what is measured is the error of the evaluation, not of two different draws."""
    D, H, E = dims
    N = rows or max(_rows(dims))
    flat = R.make_params(dims, seed=D + E)
    obs = np.random.RandomState(D * 7 + E).randn(N, D).astype(np.float32)
    ref = R.act(flat, obs, dims, SEED, STEP)
    a32 = _np(ref['action']).astype(np.float32)
    bars = {}
    with torch.no_grad():
        h64, v64 = R.forward(flat, obs, dims, F64)
        h32, v32 = R.forward(flat, obs, dims, F32)
        pairs = dict(head=(h32, h64), value=(v32, v64), entropy=(R.entropy(h32), R.entropy(h64)),
                     logp=(R.logp(h32, torch.as_tensor(a32)), R.logp(h64, torch.as_tensor(a32).double())))
    for k, (x32, x64) in pairs.items():
        bars[k] = 4.0 * _dev(_np(x32), _np(x64))
    return dict(flat=flat, obs=obs, ref=dict((k, _np(v)) for k, v in ref.items()), head64=h64, a32=a32, bars=bars,
                logp_a32=_np(pairs['logp'][1]))


# ---- 1. forward / act ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=_id)
def test_act_and_evaluate_follow_the_restatement(case):
    dims, N = case
    D, H, E = dims
    b = _base(dims)
    pol = _policy(dims, b['flat'])
    obs = _cuda(b['obs'][:N])
    a, ea, lp, v, ent, head, eps = pol.act(obs, seed=SEED, step=STEP, want_head=True, want_eps=True)
    a_, ea_, lp_, v_, ent_, head_, eps_ = (_np(t) for t in (a, ea, lp, v, ent, head, eps))
    ref, bars = b['ref'], b['bars']
    # the noise is the library's generator; the row key is the row's position in the call
    n, e = np.meshgrid(np.arange(N), np.arange(E), indexing='ij')
    assert np.abs(eps_ - R.normal01(SEED, STEP, n, e)).max() < 1e-5
    # the draw from the device's own head and noise, to a few float32 roundings (exp, product, sum); the env action is its exact clip
    mean, sig = head_[:, :E].astype(np.float64), np.exp(head_[:, E:].astype(np.float64))
    want = mean + sig * eps_
    assert (np.abs(a_ - want) <= 4.0 * 2.0 ** -24 * (np.abs(mean) + np.abs(sig * eps_)) + 1e-30).all()
    assert np.array_equal(ea_, np.clip(a_, -1.0, 1.0)) and (np.abs(a_) > 1.0).any() == (np.abs(ea_ - a_) > 0).any()
    errs = dict(head=_dev(head_, ref['head'][:N]), value=_dev(v_, ref['value'][:N]), entropy=_dev(ent_, ref['entropy'][:N]),
                logp=_dev(lp_, _np(R.logp(b['head64'][:N], torch.as_tensor(a_).double()))))
    for k in ('head', 'value', 'entropy', 'logp'):
        print('%s %s: device err %.3g (bar %.3g)' % (_id(case), k, errs[k], bars[k]))
    for k in errs:
        assert errs[k] <= bars[k], (k, errs[k], bars[k])
    # evaluate: on given actions against the restatement, on act's own actions bit for bit
    lp_e, v_e, ent_e, head_e = pol.evaluate(obs, _cuda(b['a32'][:N]), want_head=True)
    err = _dev(_np(lp_e), b['logp_a32'][:N])
    print('%s evaluate logp: device err %.3g (bar %.3g)' % (_id(case), err, bars['logp']))
    assert err <= bars['logp']
    assert torch.equal(head_e, head) and torch.equal(v_e, v) and torch.equal(ent_e, ent)
    assert torch.equal(pol.evaluate(obs, a)[0], lp)
    # two calls are bit-identical; another step changes every row
    again = pol.act(obs, seed=SEED, step=STEP, want_head=True, want_eps=True)
    assert all(torch.equal(x, y) for x, y in zip(again, (a, ea, lp, v, ent, head, eps)))
    other = pol.act(obs, seed=SEED, step=STEP + 1)
    assert bool((other[0] != a).any(dim=1).all()) and torch.equal(other[3], v)
    # deterministic: the mean
    det = pol.act(obs, seed=SEED, step=STEP, deterministic=True, want_head=True)
    assert torch.equal(det[0], head[:, :E]) and torch.equal(det[1], head[:, :E].clamp(-1.0, 1.0))
    pol.close()


@pytest.mark.parametrize('dims', [d for d in SHAPES if max(_rows(d)) >= 257], ids=lambda d: 'D%d-H%d-E%d' % d)
def test_a_row_does_not_depend_on_the_rows_beside_it(dims):
    b = _base(dims)
    pol = _policy(dims, b['flat'])
    big = pol.act(_cuda(b['obs'][:257]), seed=SEED, step=STEP, want_head=True, want_eps=True)
    small = pol.act(_cuda(b['obs'][:5]), seed=SEED, step=STEP, want_head=True, want_eps=True)
    assert all(torch.equal(x[:5], y) for x, y in zip(big, small))
    pol.close()


def test_row_count_beyond_max_rows_is_refused():
    from rl4rs_amd._lib import Rl4rsHipError
    dims = (40, 64, 3)
    b = _base(dims)
    pol = _policy(dims, b['flat'], max_rows=8)
    obs, a = _cuda(b['obs'][:9]), _cuda(b['a32'][:9])
    z = torch.zeros(9, device='cuda')
    for call in (lambda: pol.act(obs), lambda: pol.evaluate(obs, a), lambda: pol.loss_grad(0, obs, a, z, z),
                 lambda: pol.ppo_epoch(obs, a, z, z, z, z, torch.zeros((9, 6), device='cuda'), minibatch=4),
                 lambda: pol.vtrace_loss_grad(1, 3, 3, obs, a, z, z.double())):
        with pytest.raises(Rl4rsHipError, match='max_rows'):
            call()
    pol.close()


# ---- 2. loss and gradient -----------------------------------------------------------------------------------------------------------------
LOSSES = {'a2c': dict(algo=0, vf_coeff=0.5, ent_coeff=0.01), 'pg': dict(algo=0, vf_coeff=0.0, ent_coeff=0.0),
          'ppo': dict(algo=1, vf_coeff=0.5, ent_coeff=0.0, clip=0.3, vf_clip=500.0, kl_coeff=0.2),
          'ppo_vfclip': dict(algo=1, vf_coeff=0.5, ent_coeff=0.01, clip=0.3, vf_clip=0.05, kl_coeff=0.7)}


@functools.lru_cache(maxsize=None)
def _loss_inputs(dims, rows=0):
    """Rollout-like inputs on the base rows: actions drawn from a STALE policy (the old head: means shifted by 0.6 / sqrt(E) standard
    deviations, log_std by 0.2 / sqrt(E), so that log(ratio) has a spread of about 0.6 whatever E is), advantages of both signs,
    returns around the values, old values 0.1 away from the new ones."""
    D, H, E = dims
    b = _base(dims, rows)
    N = b['obs'].shape[0]
    rs = np.random.RandomState(D + 31 * E)
    head = b['ref']['head']
    old = head.copy()
    old[:, :E] += 0.6 / np.sqrt(E) * np.exp(head[:, E:]) * rs.randn(N, E)
    old[:, E:] += 0.2 / np.sqrt(E) * rs.randn(N, E)
    old = old.astype(np.float32)
    act = (old[:, :E] + np.exp(old[:, E:].astype(np.float64)) * rs.randn(N, E)).astype(np.float32)
    old_logp = _np(R.logp(torch.as_tensor(old).double(), torch.as_tensor(act).double())).astype(np.float32)
    value = b['ref']['value']
    return dict(act=act, adv=rs.randn(N).astype(np.float32), ret=(value + rs.randn(N)).astype(np.float32), old_head=old, old_logp=old_logp,
                old_value=(value + 0.1 * rs.randn(N)).astype(np.float32))


def _variant(flat, v):
    """v = 0: the parameters; v > 0: every parameter moved by one float32 rounding, up or down by a seeded coin"""
    if v == 0:
        return flat
    up = np.random.RandomState(1000 + v).rand(flat.shape[0]) < 0.5
    return np.nextafter(flat, np.where(up, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _loss_ref(dims, name, N, rows=0):
    """(float64 gradient, stats, clip masks, float32 yardstick per block, float32 yardstick of stats per row)"""
    b, x, kw = _base(dims, rows), _loss_inputs(dims, rows), LOSSES[name]
    adv = x['adv'][:N] * (1.0 / N) if name == 'pg' else x['adv'][:N]
    args = (kw['algo'], b['flat'], b['obs'][:N], x['act'][:N], adv, x['ret'][:N], dims)
    extra = dict((k, v) for k, v in kw.items() if k != 'algo')
    if kw['algo'] == 1:
        extra.update(old_logp=x['old_logp'][:N], old_value=x['old_value'][:N], old_head=x['old_head'][:N])
    g64, s64, masks = R.loss_and_grad(*args, dtype=F64, **extra)
    # the yardstick: the float32 run against the float64 run, at the parameters as they are and with every parameter moved by one
    # float32 rounding (the largest counts, as for tests/exactk_ref.py's loss figure: one run of a scalar can land on its float64 value)
    gdev, sdev = dict((k, 0.0) for k in R.NAMES), np.zeros(4)
    for v in range(3):
        a = (args[0], _variant(b['flat'], v)) + args[2:]
        r64 = (g64, s64) if v == 0 else R.loss_and_grad(*a, dtype=F64, **extra)[:2]
        g32, s32, _ = R.loss_and_grad(*a, dtype=F32, **extra)
        e = R.block_rel_err(g32, r64[0], dims)
        gdev = dict((k, max(gdev[k], e[k])) for k in R.NAMES)
        sdev = np.maximum(sdev, np.abs(s32 - r64[1]) / N / np.maximum(1.0, np.abs(r64[1]) / N))
    return g64, s64, masks, gdev, sdev


def _loss_bars(dims, name, rows=0):
    per = [_loss_ref(dims, name, n, rows) for n in _yard_rows(dims, rows)]
    return (dict((k, 4.0 * max([U32] + [p[3][k] for p in per])) for k in R.NAMES), 4.0 * np.maximum(U32, np.max([p[4] for p in per], axis=0)))


@pytest.mark.parametrize('name', sorted(LOSSES))
@pytest.mark.parametrize('case', CASES, ids=_id)
def test_loss_and_gradient_follow_the_restatement(case, name):
    _check_loss(case, name)


@pytest.mark.parametrize('name', ['a2c', 'ppo'])
def test_loss_and_gradient_follow_the_restatement_in_320_row_chunks(name):
    """gp_loss_grad reduces the sample axis in at most 16 chunks of a multiple of 64 rows: 64 up to 1024 rows, 320 at 4099.  The
    batch is a case of its own (its inputs, and its float32 yardstick at its own row count)."""
    _check_loss(BIG, name, rows=BIG[1])


def _check_loss(case, name, rows=0):
    dims, N = case
    D, H, E = dims
    b, x, kw = _base(dims, rows), _loss_inputs(dims, rows), LOSSES[name]
    if kw['algo'] == 1:
        # what the case exercises, from the restatement on the shape's full batch, before the device is looked at
        full = _loss_ref(dims, name, rows or max(_rows(dims)), rows)[2]
        share = full['ratio_clipped'].mean()
        assert 0.2 <= share <= 0.8, share
        if kw['vf_clip'] < 1.0:
            assert 0.2 <= full['value_clipped'].mean() <= 0.8, full['value_clipped'].mean()
        else:
            assert not full['value_clipped'].any()
    assert 0.2 <= (x['adv'] > 0).mean() <= 0.8
    ls = b['ref']['head'][:, E:]
    assert E == 1 or (ls.min() < -2.5 and ls.max() > 0.5)
    g64, s64, _, _, _ = _loss_ref(dims, name, N, rows)
    gbar, sbar = _loss_bars(dims, name, rows)
    pol = _policy(dims, b['flat'], max_rows=max(257, N))
    adv = x['adv'][:N] * np.float32(1.0 / N) if name == 'pg' else x['adv'][:N]
    extra = dict((k, v) for k, v in kw.items() if k != 'algo')
    if kw['algo'] == 1:
        extra.update(old_logp=_cuda(x['old_logp'][:N]), old_value=_cuda(x['old_value'][:N]), old_head=_cuda(x['old_head'][:N]))
    call = lambda: pol.loss_grad(kw['algo'], _cuda(b['obs'][:N]), _cuda(x['act'][:N]), _cuda(adv), _cuda(x['ret'][:N]), **extra)
    g, st = call()
    g2, st2 = call()
    assert torch.equal(g, g2) and torch.equal(st, st2)                     # fixed summation order: bit-identical
    g_, st_ = _np(g).astype(np.float64), _np(st).astype(np.float64)
    err = R.block_rel_err(g_, g64, dims)
    serr = np.abs(st_ - s64) / N / np.maximum(1.0, np.abs(s64) / N)
    print('%s %s: gradient err / bar per block: %s' % (_id(case), name, ', '.join('%s %.2g / %.2g' % (k, err[k], gbar[k]) for k in R.NAMES)))
    print('%s %s: stats err %s (bar %s)' % (_id(case), name, serr, sbar))
    if name == 'pg':                                                        # no critic term: the value tower's gradient is exactly zero
        w = R.split(g_, D, H, E)
        assert all(not w[k].any() for k in ('V1', 'c1', 'V2', 'c2', 'V3', 'c3'))
    for k in R.NAMES:
        assert err[k] <= gbar[k], (k, err[k], gbar[k])
    assert (serr <= sbar).all(), (serr, sbar)
    pol.close()


# ---- 3. Adam, the PPO pass, IMPALA ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grad_clip', [0.0, 0.5])
@pytest.mark.parametrize('dims', [(256, 256, 32), (40, 64, 3)], ids=lambda d: 'D%d-H%d-E%d' % d)
def test_adam_step_follows_the_restatement(dims, grad_clip):
    b = _base(dims)
    pol = _policy(dims, b['flat'])
    n = pol.n_params
    rs = np.random.RandomState(5)
    p64 = b['flat'].astype(np.float64)
    m64, v64 = np.zeros(n), np.zeros(n)
    p32, m32, v32 = b['flat'].copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for t in (1, 2, 3):
        g = (rs.randn(n) * 10.0 ** rs.uniform(-4, 0, n)).astype(np.float32)
        assert grad_clip == 0.0 or np.sqrt((g.astype(np.float64) ** 2).sum()) > grad_clip          # the clip binds
        pol.adam_step(_cuda(g), lr=1e-2, grad_clip=grad_clip)
        p64, m64, v64 = R.adam_tf(p64, g, m64, v64, t, lr=1e-2, grad_clip=grad_clip)
        p32, m32, v32 = R.adam_tf(p32, g, m32, v32, t, lr=1e-2, grad_clip=grad_clip, dtype=np.float32)
        m_, v_, step = pol.adam_state()
        assert step == t
        for what, got, want, f32 in (('params', pol.params(), p64, p32), ('m', m_, m64, m32), ('v', v_, v64, v32)):
            err, bar = _dev(_np(got), want), 4.0 * max(_dev(f32, want), U32 * np.abs(want).max())
            print('D%d-H%d-E%d clip %g step %d %s: device err %.3g (bar %.3g)' % (dims + (grad_clip, t, what, err, bar)))
            assert err <= bar, (what, t, err, bar)
    pol.close()


def _ppo_args(dims, N):
    b, x = _base(dims), _loss_inputs(dims)
    return [_cuda(v[:N]) for v in (b['obs'], x['act'], x['adv'], x['ret'], x['old_logp'], x['old_value'], x['old_head'])]


@pytest.mark.parametrize('grad_clip', [0.0, 0.05])
@pytest.mark.parametrize('dims,N,MB', [((256, 256, 32), 257, 64), ((40, 64, 3), 104, 33)])
def test_ppo_epoch_is_the_per_minibatch_loop(dims, N, MB, grad_clip):
    """One host call against rl4rs_gpolicy_loss_grad(1) + rl4rs_gpolicy_adam_step per minibatch - the data-parallel path -, bit for
    bit; N is no multiple of the minibatch: the tail is dropped."""
    b = _base(dims)
    one, loop = _policy(dims, b['flat']), _policy(dims, b['flat'])
    args = _ppo_args(dims, N)
    assert N % MB
    kw = dict(vf_coeff=0.5, ent_coeff=0.01, clip=0.3, vf_clip=0.05, kl_coeff=0.3)
    stats = one.ppo_epoch(*args, minibatch=MB, lr=1e-3, grad_clip=grad_clip, **kw)
    total = torch.zeros(4, device='cuda')
    for mb in range(N // MB):
        g, st = loop.ppo_minibatch_grad(mb, *args, minibatch=MB, **kw)
        total = total + st
        loop.adam_step(g, lr=1e-3, grad_clip=grad_clip)
    assert torch.equal(one.params(), loop.params()) and not torch.equal(one.params(), _cuda(b['flat']))
    (m1, v1, t1), (m2, v2, t2) = one.adam_state(), loop.adam_state()
    assert torch.equal(m1, m2) and torch.equal(v1, v2) and t1 == t2 == N // MB
    assert torch.equal(stats[:4], st) and torch.equal(stats[4:], total)
    one.close()
    loop.close()


@functools.lru_cache(maxsize=None)
def _vtrace_inputs(R_, T, B):
    """R rollouts of [T, B] rows of the default shape under a stale behaviour policy (the old head of _loss_inputs)"""
    dims = (256, 256, 32)
    b, x = _base(dims), _loss_inputs(dims)
    N = R_ * T * B
    assert N <= 257 * 3
    idx = np.arange(N) % 257
    rs = np.random.RandomState(N)
    return dict(dims=dims, obs=b['obs'][idx], act=x['act'][idx], blp=x['old_logp'][idx], rew=rs.rand(N) * 3.0)


VT_SIZES = ((1, 2, 5), (2, 9, 33))
VT_KW = dict(gamma=1.0, clip_rho=1.0, clip_pg_rho=0.9, vf_coeff=0.5, ent_coeff=0.01)


@functools.lru_cache(maxsize=None)
def _vtrace_ref(size, drop_last):
    v = _vtrace_inputs(*size)
    flat = _base(v['dims'])['flat']
    run = lambda dt: R.vtrace_loss_and_grad(flat, v['obs'], v['act'], v['blp'], v['rew'], size[0], size[1], size[2], v['dims'],
                                            drop_last=drop_last, dtype=dt, **VT_KW)
    g64, s64, vs64, rho = run(F64)
    g32, s32, vs32, _ = run(F32)
    kept = rho.shape[0]
    rel = lambda a32, a64: np.abs(a32 - a64) / kept / np.maximum(1.0, np.abs(a64) / kept)
    return g64, s64, vs64, rho, R.block_rel_err(g32, g64, v['dims']), rel(s32, s64), rel(vs32, vs64)


@pytest.mark.parametrize('drop_last', [True, False])
@pytest.mark.parametrize('size', VT_SIZES, ids=lambda s: 'R%d-T%d-B%d' % s)
def test_vtrace_loss_grad_is_its_parts_and_follows_the_restatement(size, drop_last):
    from rl4rs_amd import device as Dv
    R_, T, B = size
    v = _vtrace_inputs(*size)
    dims = v['dims']
    pol = _policy(dims, _base(dims)['flat'], max_rows=R_ * T * B)
    obs, act, blp, rew = _cuda(v['obs']), _cuda(v['act']), _cuda(v['blp']), _cuda(v['rew'], torch.float64)
    g, st, vst = pol.vtrace_loss_grad(R_, T, B, obs, act, blp, rew, drop_last=drop_last, **VT_KW)
    g2, st2, vst2 = pol.vtrace_loss_grad(R_, T, B, obs, act, blp, rew, drop_last=drop_last, **VT_KW)
    assert torch.equal(g, g2) and torch.equal(st, st2) and torch.equal(vst, vst2)
    # ---- hand-composed: evaluate -> V-trace per rollout -> the A2C-form loss on the kept rows
    tlp, val, _, _ = pol.evaluate(obs, act)
    Te = T - 1 if drop_last else T
    rows = torch.as_tensor(VR.kept_rows(R_, T, B, drop_last), device='cuda')
    vs_k, pg_k, vsum = [], [], np.zeros(4)
    for r in range(R_):
        sl = lambda t: t[r * T * B:(r + 1) * T * B].view(T, B)[:Te].contiguous()
        boot = val[r * T * B:(r + 1) * T * B].view(T, B)[T - 1].contiguous() if drop_last else None
        vs, pg, s4 = Dv.vtrace(sl(blp), sl(tlp), sl(val), sl(rew), bootstrap_value=boot, gamma=VT_KW['gamma'], clip_rho=VT_KW['clip_rho'],
                               clip_pg_rho=VT_KW['clip_pg_rho'])
        vs_k.append(vs.reshape(-1)); pg_k.append(pg.reshape(-1))
        vsum = _np(s4) if r == 0 else vsum + _np(s4)                        # float64 sums added in rollout order
    gc, stc = pol.loss_grad(0, obs[rows].contiguous(), act[rows].contiguous(), torch.cat(pg_k), torch.cat(vs_k), vf_coeff=VT_KW['vf_coeff'],
                            ent_coeff=VT_KW['ent_coeff'])
    assert torch.equal(g, gc) and torch.equal(st, stc) and np.array_equal(_np(vst), vsum)
    # ---- the restatement; both thresholds bind on part of the kept rows
    g64, s64, vs64, rho, _, _, _ = _vtrace_ref(size, drop_last)
    for thr in (VT_KW['clip_rho'], VT_KW['clip_pg_rho']):
        assert 0.0 < (rho > thr).mean() < 1.0, (thr, (rho > thr).mean())
    refs = [_vtrace_ref(s, d) for s in VT_SIZES for d in (True, False)]
    gbar = dict((k, 4.0 * max([U32] + [r[4][k] for r in refs])) for k in R.NAMES)
    sbar, vbar = 4.0 * np.maximum(U32, np.max([r[5] for r in refs], axis=0)), 4.0 * np.maximum(U32, np.max([r[6] for r in refs], axis=0))
    kept = rho.shape[0]
    err = R.block_rel_err(_np(g), g64, dims)
    serr = np.abs(_np(st) - s64) / kept / np.maximum(1.0, np.abs(s64) / kept)
    verr = np.abs(_np(vst) - vs64) / kept / np.maximum(1.0, np.abs(vs64) / kept)
    tag = 'R%d-T%d-B%d drop_last %d' % (size + (drop_last,))
    print('%s: gradient err / bar per block: %s' % (tag, ', '.join('%s %.2g / %.2g' % (k, err[k], gbar[k]) for k in R.NAMES)))
    print('%s: stats err %s (bar %s); vtrace sums err %s (bar %s)' % (tag, serr, sbar, verr, vbar))
    for k in R.NAMES:
        assert err[k] <= gbar[k], (k, err[k], gbar[k])
    assert (serr[:3] <= sbar[:3]).all() and _np(st)[3] == 0.0 and (verr <= vbar).all()
    pol.close()


# ---- 4. the trainer -------------------------------------------------------------------------------------------------------------------------
def _env(d, B=8, T=9):
    import rl4rs_amd
    from rl4rs_amd.env.slate import SlateRecEnv, SlateState
    from test_gpu_td3 import _cfg
    return rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(_cfg(d, B=B, T=T), state_cls=SlateState))


def _check_update(tag, tr, before, dims, ref_fn, lr, grad_clip):
    """One finished train call whose update was ONE gradient: the device's gradient against the restatement's at the parameters the
    call started from (bars: 4 x the float32 restatement on the same batch), and the parameters it left against Adam applied in
    float64 to the device's own gradient (bars: 4 x the float32 Adam)."""
    p0, m0, v0, t0 = before
    g64, s64 = ref_fn(F64)
    g32, s32 = ref_fn(F32)
    g = _np(tr.grad)
    err, f32 = R.block_rel_err(g, g64, dims), R.block_rel_err(g32, g64, dims)
    gbar = dict((k, 4.0 * max(f32[k], U32)) for k in R.NAMES)
    print('%s: gradient err / bar per block: %s' % (tag, ', '.join('%s %.2g / %.2g' % (k, err[k], gbar[k]) for k in R.NAMES)))
    for k in R.NAMES:
        assert err[k] <= gbar[k], (tag, k, err[k], gbar[k])
    want = R.adam_tf(p0, g, m0, v0, t0 + 1, lr=lr, grad_clip=grad_clip)
    f32a = R.adam_tf(p0.astype(np.float32), g, m0.astype(np.float32), v0.astype(np.float32), t0 + 1, lr=lr, grad_clip=grad_clip, dtype=np.float32)
    perr, pbar = _dev(_np(tr.params()), want[0]), 4.0 * max(_dev(f32a[0], want[0]), U32 * np.abs(want[0]).max())
    print('%s: parameter err %.3g (bar %.3g)' % (tag, perr, pbar))
    assert perr <= pbar, (tag, perr, pbar)
    return s64, np.abs(s32 - s64)


def _snapshot(tr):
    m, v, t = tr.policy.adam_state()
    return _np(tr.params()).astype(np.float64), _np(m).astype(np.float64), _np(v).astype(np.float64), t


@pytest.mark.parametrize('algo,hidden', [('A2C', 256), ('PG', 64), ('PPO', 256), ('IMPALA', 64)])
def test_trainer_tracks_the_restatement(tmp_path, algo, hidden):
    """Two train calls, the restatement fed the device's own rollout (keep_last_batch)."""
    from rl4rs_amd.train import ContiTrainer, update_kl_coeff
    env = _env(str(tmp_path))
    env.seed(7)
    tr = ContiTrainer(env, algo=algo, hidden=hidden, seed=3, init_seed=9, minibatch=72, keep_last_batch=True, drop_last=False)
    dims, N = (256, hidden, 32), 72
    assert tr.policy.n_params == R.param_count(*dims) and tr.lr == ContiTrainer.DRIVER_LR[algo] == (4e-4 if algo == 'PG' else 1e-4)
    kl_coeff = 0.2
    for it in range(2):
        before = _snapshot(tr)
        st = tr.train_iteration()
        lb = dict((k, (_np(v) if hasattr(v, 'cpu') else v)) for k, v in tr.last_batch.items())
        tag = '%s iteration %d' % (algo, it)
        assert lb['act'].shape == (N, 32) and np.isfinite(lb['act']).all() and (np.abs(lb['act']) > 1.0).any()      # the unclipped draw is stored
        if algo in ('A2C', 'PG'):
            kw = dict(vf_coeff=0.5, ent_coeff=0.01) if algo == 'A2C' else dict(vf_coeff=0.0, ent_coeff=0.0)
            fn = lambda dt: R.loss_and_grad(0, before[0], lb['obs'], lb['act'], lb['adv'], lb['ret'], dims, dtype=dt, **kw)[:2]
            s64, sdev = _check_update(tag, tr, before, dims, fn, tr.lr, 10.0 if algo == 'A2C' else 0.0)
            got = np.array([st['policy_loss'], st['vf_loss'], st['entropy']])
        elif algo == 'PPO':
            assert lb['kl_coeff'] == kl_coeff
            fn = lambda dt: R.loss_and_grad(1, before[0], lb['obs'], lb['act'], lb['adv'], lb['ret'], dims, old_logp=lb['logp'],
                                            old_value=lb['val'], old_head=lb['head'], vf_coeff=0.5, ent_coeff=0.0, clip=0.3, vf_clip=500.0,
                                            kl_coeff=kl_coeff, dtype=dt)[:2]
            s64, sdev = _check_update(tag, tr, before, dims, fn, tr.lr, 0.0)
            got = np.array([st['policy_loss'], st['vf_loss'], st['entropy'], st['kl']])
            assert abs(st['kl_mean'] - s64[3] / N) <= 4.0 * max(sdev[3] / N, U32 * max(1.0, abs(s64[3]) / N))
            kl_coeff = update_kl_coeff(kl_coeff, st['kl_mean'], 0.01)
            assert st['kl_coeff'] == kl_coeff == tr.kl_coeff
        else:
            fn = lambda dt: R.vtrace_loss_and_grad(before[0], lb['obs'], lb['act'], lb['logp'], lb['rew'], 1, 9, 8, dims, drop_last=False,
                                                   dtype=dt)[:2]
            s64, sdev = _check_update(tag, tr, before, dims, fn, tr.lr, 10.0)
            got = np.array([st['policy_loss'], st['vf_loss'], st['entropy']])
            print('%s: rho_mean %.9g' % (tag, st['rho_mean']))
            assert abs(st['rho_mean'] - 1.0) <= 1e-6 and st['rho_clipped_mean'] <= 1.0      # broadcast_interval 1: on-policy up to rounding
        k = got.shape[0]
        sbar = 4.0 * np.maximum(sdev[:k] / N, U32 * np.maximum(1.0, np.abs(s64[:k]) / N))          # per row, as in the loss tests
        print('%s: stats per row %s, restatement %s, bar %s' % (tag, got / N, s64[:k] / N, sbar))
        assert (np.abs(got - s64[:k]) / N <= sbar).all()
        assert st['iteration'] == it + 1 and np.isfinite(st['episode_reward_mean'])
        # the env resolved the CLIPPED action of the last step through its masked K-NN: every played item is legal
        assert env.samples.get_violation().all()
    e0 = tr.evaluate(episodes=16, seed=11)
    assert e0 == tr.evaluate(episodes=16, seed=11) and np.isfinite(e0)
    tr.close()


def test_impala_actor_lags_every_other_call(tmp_path):
    from rl4rs_amd.train import ContiTrainer
    env = _env(str(tmp_path))
    env.seed(5)
    tr = ContiTrainer(env, algo='IMPALA', hidden=64, seed=1, init_seed=2, lr=1e-2, broadcast_interval=2, drop_last=False)
    rho = [tr.train_iteration()['rho_mean'] for _ in range(4)]
    print('rho_mean per call:', rho)
    assert abs(rho[0] - 1.0) <= 1e-6 and abs(rho[2] - 1.0) <= 1e-6          # the actor holds the learner's parameters
    assert abs(rho[1] - 1.0) > 1e-4 and abs(rho[3] - 1.0) > 1e-4            # the actor trails by one update
    tr.close()


def test_env_items_are_the_masked_knn_of_the_clipped_action(tmp_path):
    """What the env plays is the masked K-NN of clip(a, -1, 1), not of the stored unclipped draw."""
    from rl4rs_amd import device as Dv
    from rl4rs_amd.train import ContiTrainer
    env = _env(str(tmp_path))
    env.seed(3)
    tr = ContiTrainer(env, algo='A2C', hidden=64, seed=4, init_seed=6)
    # widen the policy (log_std biases 0.5) so that many draws leave the box
    flat = tr.policy.params()
    from rl4rs_amd.nets.gausspolicy import offsets
    o3 = offsets(256, 32, 64)['b3']
    flat[o3 + 32:o3 + 64] = 0.5
    tr.policy.set_params(flat)
    emb = torch.as_tensor(np.ascontiguousarray(env.samples.action_emb), dtype=torch.float64, device='cuda')
    B, T = tr.B, tr.T
    obs = env.reset()
    seen_clipped = False
    for t in range(T):
        mask = env.samples._live().obs_mask()                                # what the env's K-NN may pick from at this step
        o = (obs['obs'] if isinstance(obs, dict) else obs).contiguous()
        a, ea, _, _, _, _, _ = tr.policy.act(o, seed=1, step=t)
        seen_clipped |= bool((a != ea).any())
        obs, reward, done, info = env.step(ea)
        want = Dv.knn(ea, emb, mask=mask)
        assert torch.equal(env.samples.last_actions.to(torch.int32).reshape(-1), want), t
    assert seen_clipped and env.samples.get_violation().all()
    tr.close()
