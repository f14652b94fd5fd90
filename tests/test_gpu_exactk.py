"""GPU: the on-device Exact-K (rl4rs_exactk_*: attention encoder, LSTM pointer decoder, REINFORCE loss and full backward, critic,
ExactKTrainer) against the float64 restatement in tests/exactk_ref.py.

Error bars.  The yardstick is the same restatement run in float32 eager torch on the CPU against float64 on the very inputs of each
case (exactk_ref.fp32_yardstick, a reference implementation, not the code under test); every bar is BAR_FACTOR = 4 x the measured
value (the accumulation order differs between implementations).  Measured max errors per shape (A, H, heads, blocks, N) and dropout
rate, the gradient relative to the reference gradient's max-norm (exactk_ref.MEASURED holds the yardstick's numbers); beside them
the device's own errors, as this file prints them on an MI355X:

                                  float32 restatement (the bar is 4 x)   device
    shape                  rate   logit      loss       gradient         logit      loss       gradient
    (284, 64, 4, 2, 37)    0.0    1.28e-6    5.30e-7    1.13e-6          1.16e-6    1.73e-7    8.02e-7
    (284, 64, 4, 2, 37)    0.1    1.85e-6    1.10e-6    1.10e-6          1.22e-6    1.50e-7    9.36e-7
    ( 75, 32, 2, 1,  5)    0.0    8.67e-7    1.21e-6    6.30e-7          5.23e-7    7.29e-7    5.50e-7
    ( 75, 32, 2, 1,  5)    0.1    8.84e-7    2.42e-6    5.31e-7          6.69e-7    9.17e-7    3.83e-7
    (284, 64, 4, 2,  1)    0.0    7.93e-7    1.03e-6    1.65e-6          6.57e-7    8.78e-7    9.79e-7
    (284, 64, 4, 2,  1)    0.1    8.73e-7    5.05e-7    1.07e-6          7.87e-7    4.48e-7    7.75e-7
    ( 64, 16, 2, 2, 33)    0.0    1.48e-6    4.14e-7    7.93e-7          1.09e-6    2.05e-7    4.81e-7
    ( 64, 16, 2, 2, 33)    0.1    1.37e-6    3.91e-7    9.89e-7          1.12e-6    5.11e-7    7.18e-7
    ( 75, 32, 2, 1, 900)   0.0    1.66e-6    1.75e-7    1.37e-6          9.74e-7    5.55e-8    1.00e-6
    ( 75, 32, 2, 1, 900)   0.1    1.86e-6    2.72e-7    8.14e-7          1.03e-6    8.53e-8    8.51e-7
    ( 40, 16, 2, 1, 1900)  0.0    1.79e-6    1.98e-7    8.05e-7          8.78e-7    1.92e-8    7.12e-7
    ( 40, 16, 2, 1, 1900)  0.1    1.18e-6    1.06e-7    7.57e-7          1.30e-6    5.43e-8    8.36e-7
    (284, 64, 4, 2, 66)    0.1    1.45e-6    1.15e-6    1.06e-6          1.22e-6    2.82e-7    1.30e-6
    crafted zero rows      0.0    6.23e-7    1.20e-6    5.52e-7          4.52e-7    8.45e-7    9.26e-7

The last three shapes are the row counts at which the sample-axis reductions leave their single-chunk form
(exactk_ref.sample_axis_forms; tests/test_exactk_host.py asserts the form of each); the third runs at dropout 0.1 only, the
configuration the trainer runs.

The loss is not differentiable where a relu pre-activation (Q / K / V, feed-forward, user layer) is 0; the units are too many to
steer away from 0, so the yardstick crosses the same kinks and its error includes them.  The seeds are those on which the yardstick
is the rounding level and stays there when every parameter is moved by one float32 rounding (exactk_ref.rounding_variants, checked in
tests/test_exactk_host.py), so that no case sits on a relu kink; at the three large shapes, where that no longer says enough, also
those whose gradient-carrying relu units all lie one rms of a float32 pre-activation error off 0 (exactk_ref.relu_sites; the comment
above exactk_ref.CASE_SEEDS has the case that showed it).  The loss figure is the largest of the yardstick run and those
variants.  A greedy pick is compared on every row-step
whose float64 top-two logit gap is at least ten times the logit bar, a sampled pick wherever u is farther from a CDF edge than
exactk_ref.edge_bar (derived there from the logit bar); at most 1 % of the rows / picks may fall under either, which
tests/test_exactk_host.py confirms on the CPU with the restatement alone."""
import functools
import os

import numpy as np
import pytest

import exactk_ref as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(key):
    """(inputs, float64 reference) of a case: computed once, shared, never modified."""
    c = R.crafted_case() if key == 'crafted' else R.case(*key)
    ref = R.loss_and_grad(c['flat'], c['obs'], c['path'], c['w'], c['dm'], c['loc'], c['special'], seed=5, step=7)
    return c, ref


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _net(c, max_rows=None, flat=None):
    from rl4rs_amd.device import DeviceExactK
    dm = c['dm']
    return DeviceExactK(c['loc'], c['special'], max_rows=max_rows or c['N'], obs_dim=dm.od, action_size=dm.A, hidden_units=dm.H,
                        num_heads=dm.heads, num_blocks=dm.blocks, vocab=dm.vocab, dropout_rate=dm.rate,
                        params=c['flat'] if flat is None else flat)


def _check_logits_loss_grad(key):
    import torch
    c, ref = _case(key)
    dm = c['dm']
    logit_bar, loss_bar, g_bar = R.bars(key, ref)
    net = _net(c)
    obs, path, w = _t(c['obs']), _t(c['path']), _t(c['w'])
    stats, lg = net.loss_grad(obs, path, w, seed=5, step=7, want_logits=True)
    g = net.grad()
    lg_np, g_np, s_np = lg.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64), stats.cpu().numpy().astype(np.float64)
    # the allowed sets are the rule's, disallowed entries are the padding value exactly
    allowed = R.allowed_sets(c['path'], c['loc'], c['special'])
    assert np.array_equal(lg_np != R.PAD32, allowed)
    assert np.array_equal(ref['logits'] != R.PAD, allowed)
    err_l = np.abs(lg_np - ref['logits'])[allowed].max()
    err_loss = abs(s_np[0] - ref['loss'])
    gmax = np.abs(ref['grad']).max()
    err_g = np.abs(g_np - ref['grad']).max() / gmax
    print('logit err %.3g (bar %.3g)  loss %.6g err %.3g (bar %.3g)  grad err %.3g of the max-norm (bar %.3g)'
          % (err_l, logit_bar, ref['loss'], err_loss, loss_bar, err_g, g_bar))
    for (name, a), b in zip(dm.split(g_np).items(), dm.split(ref['grad']).values()):
        print('    %-16s err %.3g of the max-norm' % (name, np.abs(a - b).max() / gmax))
    assert np.isfinite(g_np).all() and np.isfinite(s_np).all()
    assert s_np[1] == 0                                  # every target inside its allowed set
    assert err_l < logit_bar
    assert err_loss < loss_bar
    assert err_g < g_bar
    # bit-identical from run to run
    stats2, lg2 = net.loss_grad(obs, path, w, seed=5, step=7, want_logits=True)
    assert torch.equal(net.grad(), g) and torch.equal(lg2, lg) and torch.equal(stats2, stats)
    net.close()


@pytest.mark.parametrize('i,rate', R.CASE_KEYS)
def test_logits_loss_and_gradient_match_the_restatement(i, rate):
    """Teacher-forced logits on the allowed entries, the padding value on the others, the allowed sets themselves, the loss and the
    gradient per tensor (printed), with dropout 0 and with 0.1 under the restated keep masks; two identical calls are bit-identical."""
    _check_logits_loss_grad((i, rate))


def test_zero_rows_take_the_masked_paths():
    """The user half all zero and one zero item row: that candidate's key / query row of block 0 sums to exactly 0, so key masking,
    query masking and the layer norm of a zero row are all exercised; logits and gradient still match."""
    c, _ = _case('crafted')
    assert (c['flat'][c['dm'].split(np.arange(len(c['flat'])))['user_b']] == -1e3).all()
    _check_logits_loss_grad('crafted')


@pytest.mark.parametrize('greedy', (True, False))
@pytest.mark.parametrize('i', R.DECODE_SHAPES)
def test_greedy_and_sampled_paths(i, greedy):
    """The device's path, teacher-forced through the restatement (with the decode pass's keep masks): a greedy pick is the reference
    argmax on every firm row-step, a sampled pick the reference's inverse-CDF bucket wherever u is off an edge."""
    import torch
    key = (i, 0.1)
    c, ref0 = _case(key)
    logit_bar = R.bars(key, ref0)[0]
    net = _net(c)
    obs = _t(c['obs'])
    N, A = c['N'], c['dm'].A
    seed, step = R.DECODE_STREAMS[i]
    path, lg = net.decode(obs, greedy=greedy, seed=seed, step=step, want_logits=True)
    p_np = path.cpu().numpy()
    assert ((p_np >= 0) & (p_np < A)).all()
    assert all(len(set(row.tolist())) == R.T for row in p_np)                      # the 9 picks of a row are distinct
    allowed = R.allowed_sets(p_np, c['loc'], c['special'])
    assert allowed[np.arange(N)[:, None], np.arange(R.T)[None, :], p_np].all()     # every pick lies in its allowed set
    ref = R.logits_of(c['flat'], c['obs'], p_np, c['dm'], c['loc'], c['special'], seed=seed, step=step, pas=1).astype(np.float64)
    lg_np = lg.cpu().numpy().astype(np.float64)
    assert np.array_equal(lg_np != R.PAD32, allowed)
    err = np.abs(lg_np - ref)[allowed].max()
    print('decode logit err %.3g (bar %.3g)' % (err, logit_bar))
    assert err < logit_bar
    if greedy:
        firm = R.top_two_gap(ref) >= 10.0 * logit_bar
        soft_rows = int((~firm).any(axis=1).sum())
        print('greedy: %d of %d rows have a step under the %.3g gap' % (soft_rows, N, 10.0 * logit_bar))
        assert soft_rows <= max(0.01 * N, 0)
        assert np.array_equal(p_np[firm], ref.argmax(axis=2)[firm])
    else:
        pick, dist = R.draw(ref, R.sample_u(N, seed, step))
        off = dist > R.edge_bar(logit_bar)
        print('sampled: %d of %d picks within the %.3g edge bar' % (int((~off).sum()), off.size, R.edge_bar(logit_bar)))
        assert (~off).sum() <= 0.01 * off.size
        assert np.array_equal(p_np[off], pick[off])
    # the same (seed, step) gives the same paths bit for bit, another step gives other paths
    path2, _ = net.decode(obs, greedy=greedy, seed=seed, step=step)
    assert torch.equal(path2, path)
    if not greedy and N > 1:
        path3, _ = net.decode(obs, greedy=False, seed=seed, step=step + 1)
        assert not torch.equal(path3, path)
    net.close()


def test_a_small_call_after_a_large_one_equals_a_fresh_small_handle():
    """One handle of max_rows = 900 on the (75, 32, 2, 1) widths, dropout 0.1: loss_grad and both decodes on the 900-row case (every
    multi-chunk form, every scratch array written 900 rows deep), then on the case's first 5 rows.  The chunk rules read the rows of
    the call and never max_rows, so logits, stats, the whole gradient and the paths of the 5-row call equal those of a fresh
    max_rows = 5 handle bit for bit: nothing of the large call's scratch is read by the small one."""
    import torch
    c, _ = _case((4, 0.1))
    seed, step = R.DECODE_STREAMS[4]

    def run(net, n):
        obs, path, w = _t(c['obs'][:n]), _t(c['path'][:n]), _t(c['w'][:n])
        stats, lg = net.loss_grad(obs, path, w, seed=5, step=7, want_logits=True)
        out = [stats, lg, net.grad()]
        for greedy in (True, False):
            out.extend(net.decode(obs, greedy=greedy, seed=seed, step=step, want_logits=True))
        return out

    big, fresh = _net(c, max_rows=c['N']), _net(c, max_rows=5)
    large = run(big, c['N'])
    assert all(bool(torch.isfinite(x.float()).all()) for x in (large[0], large[2]))
    after, alone = run(big, 5), run(fresh, 5)
    for name, a, b in zip(('stats', 'logits', 'gradient', 'greedy path', 'greedy logits', 'sampled path', 'sampled logits'), after, alone):
        assert a.shape == b.shape and torch.equal(a, b), name
    assert float(alone[2].abs().max()) > 0 and not torch.equal(after[2], large[2])
    big.close()
    fresh.close()


def test_a_small_critic_call_after_a_large_one_equals_a_fresh_small_handle():
    """The critic's counterpart: 4099 rows (17 chunks, a ragged last one), then the first 37 on the same handle, against a fresh
    max_rows = 37 handle: values, squared errors, gradient and the forward bit for bit."""
    import torch
    from rl4rs_amd.device import DeviceExactKCritic
    flat, obs, target = R.critic_case(4099)

    def run(net, n):
        o, t = _t(obs[:n]), _t(target[:n])
        v, err = net.loss_grad(o, t)
        return [v, err, net.grad(), net.forward(o)]

    big, fresh = DeviceExactKCritic(4099, params=flat), DeviceExactKCritic(37, params=flat)
    large = run(big, 4099)
    assert bool(torch.isfinite(large[2]).all())
    after, alone = run(big, 37), run(fresh, 37)
    for name, a, b in zip(('value', 'squared error', 'gradient', 'forward'), after, alone):
        assert a.shape == b.shape and torch.equal(a, b), name
    assert float(alone[2].abs().max()) > 0 and not torch.equal(after[2], large[2])
    big.close()
    fresh.close()


def _adam_bar(p, lr):
    """float32 evaluation of p - lr_t m / (sqrt(v) + eps): a step of size <= ~lr carrying a few roundings (8 x 2^-24 relative),
    then the subtraction's own rounding to float32 (2^-24 |p|)."""
    return 2.0 ** -24 * np.abs(p) + 8 * 2.0 ** -24 * lr + 1e-12


@pytest.mark.parametrize('N', (37, 1, 300, 4099))
def test_critic_matches_float64_and_adam_steps_are_tf_form(N):
    """N = 37 and 1: one chunk.  N = 300 and 4099: 2 and 17 chunks of 256 rows in all four weight gradients (one of them one column
    wide), partials joined by k_reduce_chunks; 4099 leaves 3 rows to the last chunk."""
    from rl4rs_amd.device import DeviceExactKCritic
    flat, obs, target = R.critic_case(N)
    v64, e64, g64 = R.critic_loss_and_grad(flat, obs, target)
    import torch
    v32, e32, g32 = R.critic_loss_and_grad(flat, obs, target, dtype=torch.float32)
    gmax = np.abs(g64).max()
    v_bar, e_bar = R.BAR_FACTOR * np.abs(v32 - v64).max(), R.BAR_FACTOR * np.abs(e32 - e64).max()
    g_bar = R.BAR_FACTOR * np.abs(g32 - g64).max() / gmax
    net = DeviceExactKCritic(N, params=flat)
    v, err = net.loss_grad(_t(obs), _t(target))
    g = net.grad().cpu().numpy().astype(np.float64)
    ev, ee, eg = np.abs(v.cpu().numpy() - v64).max(), np.abs(err.cpu().numpy() - e64).max(), np.abs(g - g64).max() / gmax
    print('critic value err %.3g (bar %.3g)  loss err %.3g (bar %.3g)  grad err %.3g (bar %.3g)' % (ev, v_bar, ee, e_bar, eg, g_bar))
    assert ev < v_bar and ee < e_bar and eg < g_bar
    assert np.abs(net.forward(_t(obs)).cpu().numpy() - v64).max() < v_bar
    p0 = net.params().cpu().numpy().astype(np.float64)
    net.adam_step(lr=5e-3)
    want = R.adam_tf(p0, g, np.zeros_like(g), np.zeros_like(g), 1, 5e-3)[0]
    assert (np.abs(net.params().cpu().numpy() - want) <= _adam_bar(p0, 5e-3)).all()
    net.close()


def test_generator_adam_step_is_tf_form_and_the_skip_flag_gates_it():
    import torch
    c, _ = _case((1, 0.0))
    net = _net(c)
    net.loss_grad(_t(c['obs']), _t(c['path']), _t(c['w']))
    g = net.grad().cpu().numpy().astype(np.float64)
    p0 = net.params()
    net.adam_step(lr=1e-3, skip=torch.ones(1, dtype=torch.int32, device='cuda'))
    assert torch.equal(net.params(), p0)                                         # skipped: nothing moved
    m, v, t = net.adam_state()
    assert t == 1 and not m.any() and not v.any()
    net.adam_step(lr=1e-3, skip=torch.zeros(1, dtype=torch.int32, device='cuda'))
    p0 = p0.cpu().numpy().astype(np.float64)
    want = R.adam_tf(p0, g, np.zeros_like(g), np.zeros_like(g), 2, 1e-3)[0]
    assert (np.abs(net.params().cpu().numpy() - want) <= _adam_bar(p0, 2e-3)).all()
    net.close()


# ---- against the env -------------------------------------------------------------------------------------------------------
def _env(d, B=64, T=9):
    import rl4rs_amd
    from rl4rs_amd import synth
    from rl4rs_amd.env.slate import SlateRecEnv, SlateState
    text = synth.make_catalog_text(seed=4)
    synth.write_text(os.path.join(d, 'c.csv'), text)
    recs = synth.make_records(300, seed=2, hash_size=2000, special_ids=synth.special_ids_from_text(text))
    synth.write_records(os.path.join(d, 'log.csv'), recs)
    cfg = {"maxlen": 64, "batch_size": B, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
           "category_feature_num": 21, "category_hash_size": 2000, "seq_num": 2, "emb_size": 128, "page_items": 9,
           "hidden_units": 128, "max_steps": T, "action_emb_size": 32, "sample_file": os.path.join(d, 'log.csv'),
           "iteminfo_file": os.path.join(d, 'c.csv'), "cache_size": 256, "model_seed": 3, "return_tensors": True}
    return rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))


def test_decoder_allowed_sets_are_the_envs_masks(tmp_path):
    """B = 64 on the synthetic catalogue and log: the decoder's allowed set at every step equals the env's own mask bits after playing
    the device's path up to that step, and the env's error flag stays clear."""
    import torch
    from rl4rs_amd.train import ExactKTrainer
    env = _env(str(tmp_path))
    env.seed(3)
    tr = ExactKTrainer(env, seed=1, init_seed=2)
    obs0 = tr._obs(env.reset())
    path, lg = tr.policy.decode(obs0, greedy=False, seed=1, step=0, want_logits=True)
    allowed = (lg.cpu().numpy().astype(np.float64) != R.PAD32)
    live = env.samples._live()
    cols = path.t().contiguous()
    for t in range(9):
        mask = live.bits_to_mask(live.obs_mask_bits()) > 0
        assert np.array_equal(mask, allowed[:, t]), t
        env.step(cols[t])
    live.check_error_flag()
    tr.close()


def test_trainer_runs_the_reference_episode(tmp_path):
    import torch
    from rl4rs_amd.train import ExactKTrainer
    env = _env(str(tmp_path))
    env.seed(5)
    tr = ExactKTrainer(env, seed=1, init_seed=2)
    p0, c0 = tr.params().clone(), tr.critic.params().clone()
    for k in range(3):
        stats = dict(tr.train_iteration())
        assert all(np.isfinite(v) for v in stats.values()), stats
        assert stats['invalid_targets'] == 0 and stats['iteration'] == k + 1
        last = tr.last
        assert list(last['states'][0].user) == list(last['states'][1].user)          # same users for both climbs
        r = last['rewards'].cpu().numpy()
        assert np.array_equal(last['reward'].cpu().numpy(), r.max(axis=0))                         # the kept reward: the row-wise maximum
        first = r[0] >= r[1]
        kept, paths = last['path'].cpu().numpy(), last['paths'].cpu().numpy()
        assert np.array_equal(kept[first], paths[0][first]) and np.array_equal(kept[~first], paths[1][~first])
    assert not torch.equal(tr.params(), p0) and not torch.equal(tr.critic.params(), c0)
    a, b = tr.evaluate(), tr.evaluate()
    assert a == b and np.isfinite(a)
    m, v, t = tr.policy.adam_state()
    assert t == 3 and m.abs().sum() > 0
    tr.close()
    # the reference as written: the second climb is scored on the next batch of users
    env.seed(5)
    tr = ExactKTrainer(env, seed=1, init_seed=2, same_users=False)
    tr.train_iteration()
    u = tr.last['states']
    assert list(u[0].user) != list(u[1].user)
    tr.close()


# ---- it learns -------------------------------------------------------------------------------------------------------------
class _DeviceBackend(object):
    def __init__(self, c):
        from rl4rs_amd.device import DeviceExactK, DeviceExactKCritic
        self.net = _net(c)
        self.critic = DeviceExactKCritic(c['N'], params=c['critic'])
        self.obs = _t(c['obs'])

    def sample(self, step):
        return self.net.decode(self.obs, greedy=False, seed=0, step=step)[0].cpu().numpy()

    def greedy(self):
        return self.net.decode(self.obs, greedy=True)[0].cpu().numpy()

    def critic_update(self, reward):
        v, _ = self.critic.loss_grad(self.obs, _t(reward.astype(np.float32)))
        self.critic.adam_step(lr=5e-3)
        return v.cpu().numpy().astype(np.float64)

    def gen_update(self, path, w, step):
        self.net.loss_grad(self.obs, _t(path.astype(np.int32)), _t(w.astype(np.float32)), step=step)
        self.net.adam_step(lr=1e-3)


def test_it_learns():
    """No env: shape (75, 32, 2, 1), N = 64, dropout 0, reward = number of picked items from a fixed favoured set (half of the
    non-special items), REINFORCE with the critic baseline through the device calls for exactk_ref.LEARN_UPDATES = 30 updates.
    The float32 CPU restatement with the same seeds (exactk_ref.RefBackend) moves the mean greedy reward from 4.797 to 9.000, a gain of
    4.203 of the possible 9 (exactk_ref.LEARN_REF_GAIN); the device run must gain at least half of that."""
    c = R.learn_setup()
    be = _DeviceBackend(c)
    before, after = R.learn_loop(be, c['favoured'], R.LEARN_UPDATES)
    print('mean greedy reward %.3f -> %.3f (restatement gain %.3f)' % (before, after, R.LEARN_REF_GAIN))
    assert R.LEARN_REF_GAIN >= 2.0
    assert after - before >= 0.5 * R.LEARN_REF_GAIN
    be.net.close()
    be.critic.close()
