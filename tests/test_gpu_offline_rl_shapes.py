"""The discrete offline-RL Q-net (rl4rs_qnet_*, rl4rs_qloss_*, rl4rs_q_best_action; csrc/qlearn.hpp) away from the one
configuration tests/test_gpu_offline_rl.py runs (A 284, D 266, mask_size 10, emb_size 32, hidden 256 / 256, at most 300 rows):
every kernel form the unit picks by shape, against the float64 restatement (oracle/offline_rl.py).

Forms (selection code: launch_gemm_f32 in gemm.hip, st_tn_cs / st_back in simtrain.hpp):
  forward GEMM     k_gemm_small below 96 tiles of 128 x 64 (or N <= 32); k_gemm_f32_t128 from 2048 rows with N >= 96, K, N and the
                   leading dimensions multiples of 4 and 16-byte aligned operands; k_gemm_f32 otherwise.  fc1 carries relu
                   (act 4) and writes into cat with ldc = F2 = hidden1 + M * emb_size != N.
  weight gradient  k_gemm_tn4 up to 1024 rows; k_gemm_tn_t128 + k_reduce_chunks4 from 4096 rows with every width and leading
                   dimension a multiple of 4; otherwise k_gemm_tn in chunks of 512 rows + k_reduce_chunks (bias partials
                   behind the weight partials in the handle's scratch).
  input gradient   st_back (custom encoder): k_gemm_nt up to 2048 rows and below 512 tiles of 128 x 64, else k_transpose +
                   forward GEMM.  The plain encoder always takes k_gemm_nt with relu' folded in.
  row kernels      one wave per row over W = ceil(A / 32) mask words; k_q_tail_emb_bwd sums np = 256 / emb_size partials.

Inputs: parameters from init_qnet_params (embedding x 0.3 as in the existing test); location_mask a seeded random 0 / 1 array
[3, A] whose third layer is sparse (the special items and at most P - 1 others) so that one row can exhaust it; special_items a
seeded subset of about A / 20 ids.  Every custom batch of >= 8 rows carries: 0 all previous actions 0, 1 id A - 1 (last bit of
the tail word), 2 a special item, 3 none, 4 an empty surviving mask, 5 - 7 cur_step in each layer.

Bars: the floors of tests/test_gpu_offline_rl.py (forward 2e-4 * max(1, max|want|), loss 1e-4 * max(1, |want|), gradients 2e-3
of each array's largest entry, Adam weights 2e-6), each times max(1, e32(case) / e32(default shape at 256 rows)) where e32 is
the error of the float32 evaluation of the same restatement on the CPU against its float64 evaluation on the same inputs (the
restatement's own rounding, never the kernel's; the divisor is not taken below 2^-24, the unit roundoff a float32 result cannot
beat).  Whole updates: weights within max(2e-4, 4 x the float32-restatement's distance from the float64 one).

Measured on an MI355X (e32 from the CPU of the same run; every case passed, nothing in the unit had to change):
  forward     e32 4e-8 .. 4.6e-7 (floors 3.5e-7 custom, 3.3e-7 plain: ratios 1 .. 1.3); error 3e-8 .. 7e-6, a2048_n2048 8.3e-5
              at max|want| 59 (bar 1.3e-2)
  losses      e32 1e-10 .. 1.7e-7, ratios 1 .. 2; error 7e-10 .. 1.7e-6 against bars of 1e-4 .. 3.9e-3
  gradients   e32 1.5e-7 .. 7e-7 up to 1500 rows, 8.6e-7 .. 3.9e-6 at 2048 - 4100 rows (floors 5e-7 .. 9e-7: ratios 1 .. 8);
              error 9e-8 .. 1e-6 of an array's largest entry, bcq a2048_n2048 1.1e-5 (bars 2e-3 .. 1.6e-2)
  next action 0 .. 13 near-tie rows per batch (cap max(2, N // 100)), no row chosen differently from float64 in any case
  updates     weight e32 2.5e-7 .. 2.1e-6 (a65_b64), 1.2e-5 .. 2e-5 (default_b1100): bar 2e-4 in all six; error 2.3e-7 .. 1.1e-5
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24

# (obs_width, P, A, emb_size, hidden1, hidden2, N); D = obs_width + P + 1, M = P + 1, F2 = hidden1 + M * emb_size
CUSTOM = {
    # forward: every layer 3 x 5 tiles at most -> k_gemm_small.  gradients: 1030 rows -> k_gemm_tn with 3 chunks (512, 512, 6)
    # + k_reduce_chunks for weights and bias partials.  st_back: 9 x 5 and 9 x 9 tiles -> k_gemm_nt
    'default_n1030': (256, 9, 284, 32, 256, None, 1030),
    # fc1: 33 x 4 tiles, K = 266 not a multiple of 4 -> k_gemm_f32 with relu and ldc = 576.  fc2 (K 576, N 284) and head (284, 284):
    # k_gemm_f32_t128.  head and fc2 gradients: k_gemm_tn_t128 (9 chunks of 464 rows) + k_reduce_chunks4; fc1 gradient (lda 266):
    # k_gemm_tn with 9 chunks.  both st_back calls: k_transpose + k_gemm_f32_t128
    'default_n4100': (256, 9, 284, 32, 256, None, 4100),
    # every width odd: fc1 k_gemm_f32 (K 266), fc2 / head k_gemm_f32 (N 283); all gradients k_gemm_tn with 9 chunks; st_back
    # k_transpose + k_gemm_f32; rows and parameter offsets not 16-byte aligned
    'a283_n4100': (256, 9, 283, 32, 256, None, 4100),
    # W = 64, the largest action_size the custom encoder takes.  fc1 16 x 2 tiles -> small; fc2 (K 736) and head (K 2048) at 2048
    # rows -> k_gemm_f32_t128.  gradients: k_gemm_tn with 4 chunks.  first st_back Kin = 2048: 16 x 32 = 512 tiles -> k_transpose +
    # k_gemm_f32_t128 although rows <= 2048; second (Kin 736: 16 x 12 tiles) k_gemm_nt
    'a2048_n2048': (100, 9, 2048, 64, 96, None, 2048),
    # A < 64 with a partial second word (lanes 63 without an element) / a full second word / a one-bit third word; F2 = 47,
    # np = 64; small forward, k_gemm_tn with 3 chunks, k_gemm_nt
    'a63': (40, 3, 63, 4, 31, None, 1030),
    'a64': (40, 3, 64, 4, 31, None, 1030),
    'a65': (40, 3, 65, 4, 31, None, 1030),
    # M = 2 (one previous action), emb_size 1 -> np = 256; 70 rows: small forward, k_gemm_tn4, k_gemm_nt
    'tiny': (37, 1, 11, 1, 33, None, 70),
    # emb_size 256 -> np = 1; F2 = 64 + 3 * 256 = 832; small forward, k_gemm_tn4, k_gemm_nt
    'es256': (20, 2, 40, 256, 64, None, 300),
}
PLAIN = {
    # head 12 x 16 = 192 tiles below 2048 rows -> k_gemm_f32; fc1 / fc2 small.  gradients k_gemm_tn with 3 chunks; k_gemm_nt + relu'
    'plain_a1000_n1500': (74, 0, 1000, None, 128, 200, 1500),
    # fc1 33 x 2 tiles -> small; fc2 (K 128, N 200) and head (K 200, N 1000) -> k_gemm_f32_t128.  head and fc2 gradients
    # k_gemm_tn_t128 + k_reduce_chunks4, fc1 gradient (lda 75) k_gemm_tn with 9 chunks; k_gemm_nt with relu' at 4100 rows
    'plain_a1000_n4100': (74, 0, 1000, None, 128, 200, 4100),
    # odd widths, 70 rows: small forward, k_gemm_tn4, k_gemm_nt
    'plain_odd': (10, 0, 7, None, 33, 65, 70),
    # smallest action_size create takes
    'plain_a2': (10, 0, 2, None, 33, 65, 70),
}
CASES = dict(CUSTOM, **PLAIN)
# the one shape tests/test_gpu_offline_rl.py runs, at its 256 rows: where the floors were set
FLOORS = {True: (256, 9, 284, 32, 256, None, 256), False: (256, 9, 284, None, 256, 256, 256)}


class Case(object):
    def __init__(self, name, shape, tables=None, seed=17):
        self.name = name
        self.ow, self.P, self.A, self.ES, self.H1, self.H2, self.N = shape
        self.custom = self.ES is not None
        self.D = self.ow + self.P + 1
        self.M = self.P + 1 if self.custom else 0
        self.loc = self.special = None
        if self.custom:
            self.loc, self.special = tables if tables is not None else _tables(self.A, self.P, seed)

    def net_kw(self):
        return dict(location_mask=self.loc, special_items=self.special) if self.custom else {}


def _tables(A, P, seed):
    """location_mask [3, A] and special_items.  Layers 0 and 1 are dense random bits (layer 0 allows A - 1: the row that holds
    A - 1 clears a bit that was set); layer 2 allows a random non-empty part of the special items and at most P - 1 others, so
    P previous actions can remove all of it; layer 1 allows the first special item.  Ids 0 (an unfilled slot) and A - 1 are
    never special."""
    rs = np.random.RandomState(seed * 1000 + A)
    pool = np.arange(1, A - 1)
    special = np.sort(rs.choice(pool, max(1, A // 20), replace=False))
    loc = (rs.rand(3, A) < 0.5).astype(np.uint8)
    loc[0, A - 1] = 1
    loc[1, special[0]] = 1                 # row 3 (layer 1, no special item held) keeps at least this special item
    loc[2] = 0
    sp_in = special[rs.rand(len(special)) < 0.5]
    loc[2, sp_in if len(sp_in) else special[:1]] = 1
    others = np.setdiff1d(pool, special)
    loc[2, rs.choice(others, max(0, min(P - 1, len(others))), replace=False)] = 1
    assert loc[0].any() and loc[1].any() and not loc[0].all() and not loc[1].all()
    return loc, [int(s) for s in special]


@functools.lru_cache(maxsize=None)
def _case(name):
    if name in CASES:
        return Case(name, CASES[name])
    return Case(name, FLOORS[name == 'floor_custom'])


def _params(c, seed):
    from rl4rs_amd.offline_rl import init_qnet_params
    p = init_qnet_params(c.D, c.A, c.M, emb_size=c.ES or 32, hidden1=c.H1, hidden2=c.H2 or 256, seed=seed)
    return dict((k, (v * (0.3 if k == 'emb' else 1.0)).astype(np.float32)) for k, v in p.items())


def _batch(c, n, seed, forced=True):
    """(x, actions, rewards, terminals): x = obs_width N(0, 1) floats | P previous-action ids (0 = not yet chosen) | cur_step.  The
    tail ids go through the embedding, cur_step included, so cur_step stays below A."""
    rs = np.random.RandomState(seed)
    x = np.zeros((n, c.D), np.float32)
    x[:, :c.ow] = rs.randn(n, c.ow).astype(np.float32)
    cur = rs.randint(0, min(9, c.A - 1) + 1, size=n)
    if c.custom and forced and n >= 8:
        cur[:8] = [0, 1, 3, 4, 6, 2, 5, 8]
    if c.P:
        ids = rs.randint(1, c.A, size=(n, c.P))
        x[:, c.ow:c.ow + c.P] = ids * (np.arange(c.P)[None, :] < cur[:, None])
    x[:, -1] = cur
    if c.custom and forced and n >= 8:
        plain_ids = np.setdiff1d(np.arange(1, c.A - 1), c.special)
        prev = x[:, c.ow:c.ow + c.P]
        prev[0] = 0
        prev[1] = 0
        prev[1, 0] = c.A - 1
        prev[2] = rs.choice(plain_ids, c.P)
        prev[2, c.P - 1] = c.special[0]
        prev[3] = rs.choice(plain_ids, c.P)
        live = np.nonzero(c.loc[2])[0]
        gone = [k for k in live if k not in c.special] + [k for k in live if k in c.special][:1]
        assert len(gone) <= c.P
        prev[4] = (gone + [gone[-1]] * c.P)[:c.P]
        from oracle.offline_rl import mask_from_tail
        _assert_forced_rows(c, x, mask_from_tail(x, c.loc, c.special, c.M))        # every batch: each forced row is really there
    act = rs.randint(0, c.A, size=n).astype(np.int32)
    rew = (rs.rand(n) * 5).astype(np.float32)
    ter = (rs.rand(n) < 0.15).astype(np.float32)
    return x, act, rew, ter


def _assert_forced_rows(c, x, keep):
    prev, cur = x[:, c.ow:c.ow + c.P].astype(np.int64), x[:, -1].astype(np.int64)
    layer = cur % 9 // 3
    assert (prev[0] == 0).all()
    assert (prev[1] == c.A - 1).any() and layer[1] == 0 and c.loc[0, c.A - 1] and not keep[1, c.A - 1]
    assert keep[(layer == 0) & ~(prev == c.A - 1).any(axis=1), c.A - 1].any()          # ... and other rows keep that bit
    assert np.isin(prev[2], c.special).any() and not keep[2, c.special].any()
    assert not np.isin(prev[3], c.special).any() and (prev[3] > 0).all()
    allowed = np.asarray(c.special)[c.loc[layer[3], c.special] > 0]
    assert len(allowed) > 0 and keep[3, allowed].all()
    assert c.loc[layer[4]].any() and not keep[4].any()
    assert [int(v) for v in layer[5:8]] == [0, 1, 2] and set(layer.tolist()) == {0, 1, 2}


def _dev(c, params, max_rows):
    from rl4rs_amd import device as Dv
    return Dv.DeviceQNet(c.D, c.A, params, mask_size=c.M, emb_size=c.ES or 32, hidden1=c.H1, hidden2=c.H2 or 256, max_rows=max_rows,
                         **c.net_kw())


def _orc(c, params, dtype=None):
    import torch
    from oracle.offline_rl import OracleQNet
    return OracleQNet(params, mask_size=c.M, dtype=dtype or torch.float64, **c.net_kw())


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ratio(e_case, e_floor):
    return max(1.0, e_case / max(e_floor, U32))


def _rel_grad_err(got, want):
    """largest error of any array relative to that array's largest entry"""
    worst = 0.0
    for k in want:
        w = np.asarray(want[k], np.float64)
        worst = max(worst, np.abs(np.asarray(got[k], np.float64) - w).max() / max(np.abs(w).max(), 1e-12))
    return worst


def _forward_ref(c, params, x):
    """(float64 output, e32 relative to max(1, max|want|))"""
    import torch
    w64 = _orc(c, params).forward(x).detach().numpy()
    w32 = _orc(c, params, torch.float32).forward(x).detach().numpy().astype(np.float64)
    return w64, np.abs(w32 - w64).max() / max(1.0, np.abs(w64).max())


def _imitation_ref(c, params, x, act, beta, dtype=None):
    from oracle import offline_rl as O
    orc = _orc(c, params, dtype)
    loss = O.imitation_loss(orc.forward(x), act, beta)
    loss.backward()
    return float(loss.detach()), orc.grads()


def _imitation_e32(c, params, x, act, beta):
    """(float64 loss, float64 gradients, e32 of the loss relative to max(1, |loss|), e32 of the gradients)"""
    import torch
    l64, g64 = _imitation_ref(c, params, x, act, beta)
    l32, g32 = _imitation_ref(c, params, x, act, beta, torch.float32)
    return l64, g64, abs(l32 - l64) / max(1.0, abs(l64)), _rel_grad_err(g32, g64)


TD_MODES = {'bcq': (True, 0.0), 'cql': (False, 1.0), 'dqn': (False, 0.0)}        # mode -> (imitator, cql alpha)


def _td_inputs(c, mode):
    """parameters of q / target / imitator and a batch with its successor rows (zero observation after a terminal row)"""
    ps = [_params(c, 7), _params(c, 8), _params(c, 9) if TD_MODES[mode][0] else None]
    x, act, rew, ter = _batch(c, c.N, 10)
    nx = _batch(c, c.N, 11)[0]
    nx[ter > 0.5] = 0.0
    return ps, x, nx, act, rew, ter


def _td_ref(c, mode, ps, x, nx, act, rew, ter, dtype=None, best=None):
    from oracle import offline_rl as O
    alpha = TD_MODES[mode][1]
    orc, orc_t = _orc(c, ps[0], dtype), _orc(c, ps[1], dtype)
    o_imit = _orc(c, ps[2], dtype).forward(nx) if ps[2] is not None else None
    o_next, o_next_t = orc.forward(nx), orc_t.forward(nx)
    orc.zero_grad()
    o_q = orc.forward(x)
    td, cons, o_best = O.dqn_loss(o_q, act, rew, ter, o_next, o_next_t, imitator_next=o_imit, action_flexibility=0.3, gamma=0.99,
                                  cql_alpha=alpha, best=best)
    (td + alpha * cons).backward()
    a = np.asarray(act, np.int64)
    y = rew + 0.99 * o_next_t.detach().numpy()[np.arange(len(a)), o_best.numpy()] * (1 - ter)
    return dict(td=float(td.detach()), cons=float(cons.detach()), best=o_best.numpy(), grads=orc.grads(),
                scores=O.action_scores(o_next, o_imit, 0.3).numpy(), diff=y - o_q.detach().numpy()[np.arange(len(a)), a])


def _td_e32(c, mode, ps, x, nx, act, rew, ter, best):
    """e32 of (td, conservative, gradients) with the next actions fixed, so that a float32 tie cannot enter the figure"""
    import torch
    r64 = _td_ref(c, mode, ps, x, nx, act, rew, ter, best=best)
    r32 = _td_ref(c, mode, ps, x, nx, act, rew, ter, torch.float32, best=best)
    return (r64, abs(r32['td'] - r64['td']) / max(1.0, abs(r64['td'])), abs(r32['cons'] - r64['cons']) / max(1.0, abs(r64['cons'])),
            _rel_grad_err(r32['grads'], r64['grads']))


@functools.lru_cache(maxsize=None)
def _floor_forward(custom):
    c = _case('floor_custom' if custom else 'floor_plain')
    return _forward_ref(c, _params(c, 3), _batch(c, c.N, 5)[0])[1]


@functools.lru_cache(maxsize=None)
def _floor_imitation(custom, beta):
    c = _case('floor_custom' if custom else 'floor_plain')
    x, act, _, _ = _batch(c, c.N, 6)
    return _imitation_e32(c, _params(c, 4), x, act, beta)[2:]


@functools.lru_cache(maxsize=None)
def _floor_td(mode):
    c = _case('floor_custom' if TD_MODES[mode][0] else 'floor_plain')
    ps, x, nx, act, rew, ter = _td_inputs(c, mode)
    best = _td_ref(c, mode, ps, x, nx, act, rew, ter)['best']
    return _td_e32(c, mode, ps, x, nx, act, rew, ter, best)[1:]


def _check_loss(got, want, e32, e32_floor, what):
    bar = 1e-4 * _ratio(e32, e32_floor) * max(1.0, abs(want))
    print('%s: %.8g vs %.8g, err %.3g, bar %.3g (e32 %.3g, floor e32 %.3g)' % (what, got, want, abs(got - want), bar, e32, e32_floor))
    assert abs(got - want) < bar, '%s: %.8g vs %.8g (e32 %.3g, floor e32 %.3g)' % (what, got, want, e32, e32_floor)


def _check_grads(dev, want, e32, e32_floor, what):
    rel = 2e-3 * _ratio(e32, e32_floor)
    got = dict((k, v.cpu().numpy()) for k, v in dev.gradients().items())
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        w = np.asarray(want[k], np.float64)
        err, scale = np.abs(got[k] - w).max(), max(np.abs(w).max(), 1e-12)
        print('%s grad %s: err %.3g of max %.3g (relative %.3g, bar %.3g; e32 %.3g, floor e32 %.3g)' % (
            what, k, err, scale, err / scale, rel, e32, e32_floor))
        assert err <= rel * scale, '%s grad %s: err %.3e vs scale %.3e (e32 %.3g, floor e32 %.3g)' % (what, k, err, scale, e32, e32_floor)


@pytest.mark.parametrize('name', sorted(CASES))
def test_forward_and_mask(name):
    from oracle.offline_rl import mask_from_tail
    c = _case(name)
    params = _params(c, 3)
    x = _batch(c, c.N, 5)[0]
    dev = _dev(c, params, c.N)
    out = dev.forward(_cuda(x)).cpu().numpy()
    want, e32 = _forward_ref(c, params, x)
    floor = _floor_forward(c.custom)
    bar = 2e-4 * _ratio(e32, floor) * max(1.0, np.abs(want).max())
    err = np.abs(out - want).max()
    print('%s forward: err %.3g, bar %.3g (e32 %.3g, floor e32 %.3g)' % (name, err, bar, e32, floor))
    assert err < bar, '%s forward: err %.3g, bar %.3g (e32 %.3g, floor e32 %.3g)' % (name, err, bar, e32, floor)
    if c.custom:
        keep = mask_from_tail(x, c.loc, c.special, c.M)
        _assert_forced_rows(c, x, keep)
        # row 4 keeps nothing of the encoder: the output is the head's bias
        assert np.abs(out[4] - params['head_b'].astype(np.float64)).max() < bar
        # the mask itself (integer rule) bit for bit through a one-hot head
        p2 = dict(params)
        p2['head_w'] = np.eye(c.A, dtype=np.float32)
        p2['head_b'] = np.zeros(c.A, np.float32)
        p2['fc2_b'] = np.ones(c.A, np.float32) * 7.0
        p2['fc2_w'] = np.zeros_like(params['fc2_w'])
        probe = _dev(c, p2, c.N)
        kept = probe.forward(_cuda(x)).cpu().numpy() == 7.0
        assert np.array_equal(kept, keep), np.argwhere(kept != keep)[:10]
        assert kept.any() and not kept.all()
        probe.check_status()
        probe.close()
    dev.check_status()
    dev.close()


def _imitation_check(c, dev, params, x, act, tag):
    for beta in (0.0, 0.5):
        xd = _cuda(x)
        logits = dev.forward(xd)
        loss2, d = dev.imitation_loss(logits, _cuda(act), beta)
        dev.backward(xd, d)
        l64, g64, e_l, e_g = _imitation_e32(c, params, x, act, beta)
        f_l, f_g = _floor_imitation(c.custom, beta)
        _check_loss(float(loss2[0] + beta * loss2[1] / c.A), l64, e_l, f_l, '%s beta %.1f loss' % (tag, beta))
        _check_grads(dev, g64, e_g, f_g, '%s beta %.1f' % (tag, beta))
    dev.check_status()


@pytest.mark.parametrize('name', sorted(CASES))
def test_imitation_loss_and_gradients(name):
    c = _case(name)
    params = _params(c, 4)
    x, act, _, _ = _batch(c, c.N, 6)
    dev = _dev(c, params, c.N)
    _imitation_check(c, dev, params, x, act, name)
    dev.close()


# (case, rows of the second call): the second call's forms differ from the first's, in a handle whose activations, mask bits and
# chunk partials hold the larger call's values
#   default_n4100 -> 1030 rows: small forward, k_gemm_tn with 3 chunks (9 chunks of stale partials behind them), k_gemm_nt
#   a65 -> 70 rows: k_gemm_tn4 after k_gemm_tn
#   plain_a1000_n4100 -> 1500 rows: head k_gemm_f32 after k_gemm_f32_t128, k_gemm_tn after k_gemm_tn_t128
@pytest.mark.parametrize('name,n', [('default_n4100', 1030), ('a65', 70), ('plain_a1000_n4100', 1500)])
def test_fewer_rows_after_a_full_batch(name, n):
    c = _case(name)
    params = _params(c, 4)
    x, act, _, _ = _batch(c, c.N, 6)
    dev = _dev(c, params, c.N)
    xd = _cuda(x)
    _, d = dev.imitation_loss(dev.forward(xd), _cuda(act), 0.5)
    dev.backward(xd, d)
    lo = c.N - n                                                   # the LAST n rows: row i of the small call is not row i of the large one
    _imitation_check(c, dev, params, x[lo:].copy(), act[lo:].copy(), '%s last %d rows' % (name, n))
    dev.close()


@pytest.mark.parametrize('mode,name', [('bcq', n) for n in sorted(CUSTOM)] + [(m, n) for m in ('cql', 'dqn') for n in sorted(PLAIN)])
def test_td_loss_action_choice_and_gradients(mode, name):
    c = _case(name)
    has_imit, alpha = TD_MODES[mode]
    ps, x, nx, act, rew, ter = _td_inputs(c, mode)
    dev, tgt = _dev(c, ps[0], c.N), _dev(c, ps[1], c.N)
    imit = _dev(c, ps[2], c.N) if has_imit else None
    xd, nd = _cuda(x), _cuda(nx)
    imit_next = imit.forward(nd) if has_imit else None
    q_next, q_next_t = dev.forward(nd), tgt.forward(nd)
    q_t = dev.forward(xd)
    loss2, dq, best = dev.dqn_loss(q_t, _cuda(act), _cuda(rew), _cuda(ter), q_next, q_next_t, imitator_next=imit_next,
                                   action_flexibility=0.3, gamma=0.99, cql_alpha=alpha)
    dev.backward(xd, dq)
    best = best.cpu().numpy().astype(np.int64)
    free = _td_ref(c, mode, ps, x, nx, act, rew, ter)                 # the oracle's own choice
    assert (np.abs(free['diff']) < 1.0).any() and (np.abs(free['diff']) >= 1.0).any()       # both Huber branches
    # integer choice: identical except on rows whose float64 top two scores are within 1e-4; there the two chosen actions score
    # within 1e-4 of each other; such rows are few (a condition on the inputs, not a tolerance)
    scores, o_best, rows = free['scores'], free['best'], np.arange(c.N)
    top = np.sort(scores, axis=1)[:, -2:]
    near = (top[:, 1] - top[:, 0]) < 1e-4
    differ = np.nonzero(best != o_best)[0]
    print('%s %s: %d near-tie rows, %d rows choose differently' % (mode, name, near.sum(), len(differ)))
    assert near.sum() <= max(2, c.N // 100), near.sum()
    assert near[differ].all(), (differ, best[differ], o_best[differ])
    assert (np.abs(scores[differ, best[differ]] - scores[differ, o_best[differ]]) < 1e-4).all()
    assert ((best >= 0) & (best < c.A)).all()
    # losses and gradients on ALL rows, the oracle's target taking the device's choice
    r64, e_td, e_cons, e_g = _td_e32(c, mode, ps, x, nx, act, rew, ter, best)
    f_td, f_cons, f_g = _floor_td(mode)
    _check_loss(float(loss2[0]), r64['td'], e_td, f_td, '%s %s td' % (mode, name))
    _check_loss(float(loss2[1]), r64['cons'], e_cons, f_cons, '%s %s conservative' % (mode, name))
    _check_grads(dev, r64['grads'], e_g, f_g, '%s %s' % (mode, name))
    # the stand-alone greedy rule is the same device function
    again = dev.best_action(q_next, imit_next, 0.3).cpu().numpy()
    assert np.array_equal(again, best)
    for n in (dev, tgt, imit):
        if n is not None:
            n.check_status()
            n.close()


def _edge_rows(A, rs):
    """q rows with a known first arg-max: constant; maximum in the last column; equal maxima in two lanes (of different
    64-strides where A has them), the lower index once in the lower and once in the higher lane; distinct values"""
    spread = (rs.permutation(A) * 0.25).astype(np.float32)           # distinct, exact in float32 and so are their differences
    rows = [np.full(A, 1.5, np.float32), spread.copy()]
    last = spread.copy()
    last[A - 1] = A
    rows.append(last)
    pairs = {2: [(0, 1)], 63: [(7, 50), (20, 3)], 64: [(7, 50), (63, 3)], 65: [(7, 64), (0, 64)], 284: [(70, 200), (67, 130)],
             2048: [(1000, 1999), (67, 130)]}[A]
    for a, b in pairs:
        r = spread.copy()
        r[a] = r[b] = A
        rows.append(r)
    return np.stack(rows)


@pytest.mark.parametrize('A', [2, 63, 64, 65, 284, 2048])
def test_greedy_rule_edges(A):
    import torch
    from oracle import offline_rl as O
    c = Case('edge', (2, 0, A, None, 4, 4, 16))
    dev = _dev(c, _params(c, 1), 16)
    rs = np.random.RandomState(A)
    q = _edge_rows(A, rs)
    R = q.shape[0]

    def both(q, imit, flex):
        got = dev.best_action(_cuda(q), _cuda(imit) if imit is not None else None, flex).cpu().numpy()
        want = O.best_action(torch.from_numpy(q).double(), torch.from_numpy(imit).double() if imit is not None else None, flex).numpy()
        assert np.array_equal(got, want), (A, flex, got, want)
        return got

    got = both(q, None, 0.3)
    assert got[0] == 0 and got[2] == A - 1                              # all tie: the first index; the last column
    # BCQ rule with every action passing (constant imitator): (q - min q) has the same first arg-max as q, except for the constant
    # row, whose scores all tie at 0
    flat = np.zeros((R, A), np.float32)
    assert np.array_equal(both(q, flat, 0.3), got)
    # only one action passes: its score is q - min q, every other score 0.  Passing the arg-min of q: all scores 0, index 0 wins
    one = np.zeros((R, A), np.float32)
    lows = q[1:].argmin(axis=1)
    one[np.arange(1, R), lows] = 10.0
    one[0, A - 1] = 10.0
    got_one = both(q, one, 0.3)
    assert (got_one == 0).all()
    # ... passing the last column of a row whose minimum is elsewhere: the last column wins
    one[:] = 0.0
    one[:, A - 1] = 10.0
    got_last = both(q, one, 0.3)
    assert got_last[0] == 0 and got_last[2] == A - 1
    # action_flexibility 1.0: log pi - max log pi > 0 holds nowhere, every score is 0
    imit = (rs.permutation(A) * 0.5).astype(np.float32)[None, :].repeat(R, axis=0)
    assert (both(q, imit, 1.0) == 0).all()
    # ... also where the imitator's maximum sits at an index that is neither 0 nor the arg-min of q (q ascending, maximum at
    # A - 1): with >= for > that action alone would pass and win, at every A including 2
    asc = (np.arange(A) * 0.25).astype(np.float32)[None, :]
    peak = np.zeros((1, A), np.float32)
    peak[0, A - 1] = 3.0
    assert both(asc, peak, 1.0)[0] == 0 and both(asc, peak, 0.3)[0] == A - 1
    # a threshold between the imitator's values: multiples of 0.5 against log(0.3) = -1.204
    both(q, imit, 0.3)
    dev.close()


def test_status_flags():
    c = _case('default_n1030')
    params = _params(c, 3)
    x, act, rew, ter = _batch(c, 64, 5)
    x[:, -1] = np.minimum(x[:, -1], 5)                                # cur_step 0 .. 5: layers 0 and 1 only
    two = Case('two_layers', CASES['default_n1030'], tables=(c.loc[:2], c.special))
    # flag 2: a location_mask of two layers and one row with cur_step 6 (layer 2).  The IndexError's text names the rule
    # ("cur_step % 9 // 3 selects a location_mask row that does not exist"), not the layer's number: the flag is one bit
    bad = x.copy()
    bad[9, -1] = 6
    dev = _dev(two, params, 64)
    dev.forward(_cuda(bad))
    with pytest.raises(IndexError, match='location_mask row'):
        dev.check_status()
    dev.close()
    dev = _dev(two, params, 64)
    dev.forward(_cuda(np.delete(bad, 9, axis=0)))
    dev.check_status()
    # an action outside [0, A): imitation loss, TD loss
    logits = dev.forward(_cuda(x))
    dev.imitation_loss(logits, _cuda(act), 0.5)
    dev.dqn_loss(logits, _cuda(act), _cuda(rew), _cuda(ter), logits, logits)
    dev.check_status()
    wrong = act.copy()
    wrong[5] = c.A
    dev.imitation_loss(logits, _cuda(wrong), 0.5)
    with pytest.raises(IndexError, match='action'):
        dev.check_status()
    dev.close()
    dev = _dev(two, params, 64)
    logits = dev.forward(_cuda(x))
    wrong[5] = -1
    dev.dqn_loss(logits, _cuda(wrong), _cuda(rew), _cuda(ter), logits, logits)
    with pytest.raises(IndexError, match='action'):
        dev.check_status()
    dev.close()


def test_create_and_row_count_checks():
    import torch
    from rl4rs_amd import device as Dv
    from rl4rs_amd._lib import Rl4rsHipError, check

    def refuse(shape, message, edit=None):
        c = Case('refused', shape)
        params = _params(c, 1)
        if edit:
            edit(params)
        with pytest.raises(Rl4rsHipError, match=message):
            _dev(c, params, 16)

    refuse((20, 2, 40, 24, 16, None, 16), 'emb_size dividing 256')             # 24 does not divide 256
    refuse((6, 1, 2049, 4, 8, None, 16), 'action_size <= 2048')                # W = 65 mask words
    refuse((20, 0, 40, 4, 16, None, 16), 'the custom encoder needs')           # mask_size 1: no previous action
    refuse((0, 4, 40, 4, 16, None, 16), 'bad sizes')                           # mask_size == obs_dim

    def no_hidden2(p):
        p['fc2_w'], p['fc2_b'], p['head_w'] = p['fc2_w'][:, :0], p['fc2_b'][:0], p['head_w'][:0]

    c = Case('refused', (10, 0, 7, None, 33, 4, 16))
    params = _params(c, 1)
    no_hidden2(params)
    with pytest.raises(Rl4rsHipError, match='the plain encoder needs hidden2'):
        Dv.DeviceQNet(c.D, c.A, params, hidden1=c.H1, hidden2=0, max_rows=16)
    # more rows than max_rows: refused by the wrapper and by the library
    c = _case('plain_odd')
    dev = _dev(c, _params(c, 1), 16)
    x = _cuda(_batch(c, 17, 2)[0])
    with pytest.raises(ValueError, match='obs must be'):
        dev.forward(x)
    out = torch.empty((17, c.A), dtype=torch.float32, device=x.device)
    with pytest.raises(Rl4rsHipError, match='max_rows=16'):
        check(dev.lib.rl4rs_qnet_forward(dev.h, 17, Dv._ptr(x), Dv._ptr(out), Dv._stream()))
    with pytest.raises(Rl4rsHipError, match='max_rows=16'):
        check(dev.lib.rl4rs_qnet_backward(dev.h, 17, Dv._ptr(x), Dv._ptr(out), Dv._stream()))
    dev.forward(x[:16])
    dev.check_status()
    dev.close()


LR, GAMMA, FLEX, BETA, ALPHA, INTERVAL = 1e-3, 0.99, 0.3, 0.5, 1.0, 2


def _restate(algo, c, start, batches, dtype):
    """three updates of offline_rl.py's learner in ``dtype``: call order and sums as there; returns (losses, parameters after the
    last update, q's parameters after the second)"""
    import torch
    from oracle import offline_rl as O
    npd = np.float64 if dtype == torch.float64 else np.float32
    P = dict((k, dict((pk, np.asarray(pv).astype(npd)) for pk, pv in v.items())) for k, v in start.items())
    M = dict((k, dict((pk, np.zeros_like(pv)) for pk, pv in v.items())) for k, v in P.items())
    V = dict((k, dict((pk, np.zeros_like(pv)) for pk, pv in v.items())) for k, v in P.items())
    losses, q_at_2 = [], None
    for it, (x, act, rew, nx, ter) in enumerate(batches):
        net = dict((k, _orc(c, P[k], dtype)) for k in P)
        stepped = []
        if algo == 'BC':
            loss = O.imitation_loss(net['imitator'].forward(x), act, BETA)
            loss.backward()
            stepped = ['imitator']
        else:
            imit_next = net['imitator'].forward(nx) if algo == 'BCQ' else None
            q_next, q_next_t = net['q'].forward(nx), net['q_target'].forward(nx)
            q_t = net['q'].forward(x)
            td, cons, _ = O.dqn_loss(q_t, act, rew, ter, q_next, q_next_t, imitator_next=imit_next, action_flexibility=FLEX, gamma=GAMMA)
            if algo == 'BCQ':
                td.backward()
                im = O.imitation_loss(net['imitator'].forward(x), act, BETA)
                im.backward()
                loss, stepped = td + im, ['q', 'imitator']
            else:
                loss = td + ALPHA * cons
                loss.backward()
                stepped = ['q']
        for k in stepped:
            g = dict((pk, np.asarray(pv).astype(npd)) for pk, pv in net[k].grads().items())
            P[k] = _adam_typed(P[k], g, M[k], V[k], it + 1, npd)
        if algo != 'BC' and (it + 1) % INTERVAL == 0:
            P['q_target'] = dict((pk, pv.copy()) for pk, pv in P['q'].items())
        if it == 1 and 'q' in P:
            q_at_2 = dict((pk, pv.copy()) for pk, pv in P['q'].items())
        losses.append(float(loss.detach()))
    return losses, P, q_at_2


def _adam_typed(p, g, m, v, t, npd):
    from oracle.offline_rl import torch_adam
    out = torch_adam(p, g, m, v, t, LR)
    return dict((k, np.asarray(a).astype(npd)) for k, a in out.items())


@pytest.mark.parametrize('config', ['default_b1100', 'a65_b64'])
@pytest.mark.parametrize('algo', ['BC', 'BCQ', 'CQL'])
def test_updates_track_the_fp64_restatement(tmp_path, algo, config):
    """three whole update() calls (forward order, both networks, Adam, the target copy at update 2) against the same steps
    restated in float64.  default_b1100: 1100 rows -> k_gemm_tn with 3 chunks behind a learner; a65_b64: location_mask and
    special_items handed over in the config."""
    import os
    import torch
    from rl4rs_amd import offline_rl as R
    if config == 'default_b1100':
        from rl4rs_amd import synth
        from rl4rs_amd.data import CatalogTables
        path = os.path.join(str(tmp_path), 'item_info.csv')
        synth.write_text(path, synth.make_catalog_text(seed=21))
        tab = CatalogTables(path, 284, 32)
        tables = (np.asarray(tab.location_mask), [int(s) for s in tab.special_items])
        shape, B = (256, 9, 284, 32, 256, 256, 1100), 1100
        cfg = {'action_size': 284, 'page_items': 9, 'action_emb_size': 32, 'iteminfo_file': path}
    else:
        tables = _tables(65, 3, 17)
        shape, B = (40, 3, 65, 32, 256, 256, 64), 64
        cfg = {'action_size': 65, 'page_items': 3, 'location_mask': tables[0], 'special_items': tables[1]}
    custom = algo != 'CQL'
    c = Case(config, shape if custom else shape[:3] + (None,) + shape[4:], tables=tables)
    kw = dict(batch_size=B, learning_rate=LR, seed=5)
    if algo == 'BC':
        learner = R.DiscreteBC(cfg, c.D, beta=BETA, **kw)
    elif algo == 'BCQ':
        learner = R.DiscreteBCQ(cfg, c.D, gamma=GAMMA, action_flexibility=FLEX, beta=BETA, target_update_interval=INTERVAL, **kw)
    else:
        learner = R.DiscreteCQL(cfg, c.D, gamma=GAMMA, alpha=ALPHA, target_update_interval=INTERVAL, **kw)
    names = {'BC': ['imitator'], 'BCQ': ['q', 'q_target', 'imitator'], 'CQL': ['q', 'q_target']}[algo]
    start = dict((k, dict((pk, pv.cpu().numpy()) for pk, pv in getattr(learner, k).weights().items())) for k in names)
    batches = []
    for it in range(3):
        x, act, rew, ter = _batch(c, B, 50 + it, forced=False)
        nx = _batch(c, B, 60 + it, forced=False)[0]
        nx[ter > 0.5] = 0.0
        batches.append((x, act, rew, nx, ter))
    l64, P64, q2_64 = _restate(algo, c, start, batches, torch.float64)
    l32, P32, _ = _restate(algo, c, start, batches, torch.float32)
    e32 = max(np.abs(P32[k][pk].astype(np.float64) - P64[k][pk]).max() for k in names for pk in P64[k])
    bar = max(2e-4, 4.0 * e32)           # the kernels sum in another order than torch: four times the restatement's own float32 drift
    dev_q2 = None
    for it, (x, act, rew, nx, ter) in enumerate(batches):
        loss = float(learner.update(*[_cuda(v) for v in (x, act, rew, nx, ter)]))
        print('%s %s update %d: loss %.8g vs %.8g (float32 restatement %.8g)' % (algo, config, it + 1, loss, l64[it], l32[it]))
        assert abs(loss - l64[it]) < 1e-4 * max(1.0, abs(l64[it])), (it, loss, l64[it])
        if it == 1 and algo != 'BC':
            dev_q2 = dict((pk, pv.clone()) for pk, pv in learner.q.weights().items())
    moved = max(np.abs(P64[k][pk] - start[k][pk]).max() for k in names if k != 'q_target' for pk in P64[k])
    assert moved > 10 * bar, (moved, bar)                                    # the bar is far below what three updates change
    for k in names:
        w = getattr(learner, k).weights()
        for pk in P64[k]:
            err = np.abs(w[pk].cpu().numpy() - P64[k][pk]).max()
            print('%s %s %s.%s: err %.3g, bar %.3g (weight e32 %.3g)' % (algo, config, k, pk, err, bar, e32))
            assert err < bar, '%s.%s: err %.3g, bar %.3g (weight e32 %.3g)' % (k, pk, err, bar, e32)
    if algo != 'BC':
        # the target is q as of update 2 (the copy), not q as of update 3
        wt, wq = learner.q_target.weights(), learner.q.weights()
        for pk in wt:
            assert torch.equal(wt[pk], dev_q2[pk]), pk
            assert np.abs(P64['q_target'][pk] - q2_64[pk]).max() == 0.0
        assert max(float((wt[pk] - wq[pk]).abs().max()) for pk in wt) > bar
    assert learner.total_step == 3
    for n in learner.nets:
        n.check_status()
    learner.close()
