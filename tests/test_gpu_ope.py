"""GPU: off-policy evaluation on the device (rl4rs_amd/csrc/ope.hip, rl4rs_amd/ope.py, rl4rs.utils.offline_policy_metrics,
rl4rs.policy.behavior_model) against fixtures recorded from the reference's own functions (tests/golden/make_ope_golden.py).

The estimator bar is rtol 1e-9 on every finite number and NaN exactly where the reference has NaN.  Derivation: the only licence
taken is the ORDER of float64 sums of at most 16384 * 36 terms, bounded by N * 2^-53 (about 6.5e-11 of the sum of magnitudes), and
the variances are two-pass like the reference's; 1e-9 leaves a factor ~15 and is below one float32 rounding (6e-8), so float32
arithmetic anywhere on the path fails it."""
import os

import numpy as np
import pytest

import ope_inputs as I

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
RTOL = 1e-9


def _close(got, want, rtol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    got = np.broadcast_to(got, want.shape) if got.shape != want.shape and got.ndim <= want.ndim else got
    want = np.broadcast_to(want, got.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, got, want)
    with np.errstate(all='ignore'):
        rel = np.where(nan, 0.0, np.abs(got - want) / np.maximum(np.abs(want), 1e-300))
        rel = np.where(~nan & (want == 0), np.abs(got), rel)
    print('%s: max rel %.3g' % (what, rel.max() if rel.size else 0.0))
    assert (rel <= rtol).all(), (what, rel.max(), got, want)


def _six(x, OPE):
    ep = (x['rewards'], x['pi_mul'], x['mu_mul'])
    return [OPE.eval_IPS(*ep), OPE.eval_CIPS(*ep), OPE.eval_SNIPS(*ep),
            OPE.eval_doubly_robust(x['episode_reward'], x['q_mean'], *ep),
            OPE.eval_WIPS(x['step_rewards'], x['pi'], x['mu']),
            OPE.eval_WIPS(x['step_rewards'], x['pi'], x['mu'], gamma=0.9),
            OPE.eval_seq_doubly_robust(x['rhat'], x['q'], x['step_rewards'], x['pi'], x['mu'])]


@pytest.mark.parametrize('case', range(len(I.ESTIMATOR_CASES)), ids=['B%d_T%d' % (b, t) for b, t, _ in I.ESTIMATOR_CASES])
def test_estimators_against_the_reference(case):
    import torch
    import rl4rs.utils.offline_policy_metrics as OPE
    with np.load(os.path.join(GOLDEN, 'ope_estimators.npz')) as z:
        want = z['expected'][case]
        assert tuple(z['cases'][case]) == I.ESTIMATOR_CASES[case]
    B, T, seed = I.ESTIMATOR_CASES[case]
    x = I.estimator_inputs(B, T, seed)
    got = _six(x, OPE)
    for pair in got:
        assert isinstance(pair, tuple) and len(pair) == 2 and all(type(v) is float for v in pair), pair
    for name, g, w in zip(I.ESTIMATOR_NAMES, got, want):
        _close(g, w, RTOL, '%s B=%d T=%d' % (name, B, T))
    # device tensors in, and float32 inputs are widened (all arithmetic float64): the float32-rounded inputs give what the float64
    # functions give on those rounded values
    xt = dict((k, torch.from_numpy(v).cuda()) for k, v in x.items())
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(_six(xt, OPE), got))
    x32 = dict((k, v.astype(np.float32)) for k, v in x.items())
    x64 = dict((k, v.astype(np.float64)) for k, v in x32.items())
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(_six(x32, OPE), _six(x64, OPE)))


def _columns(x):
    """the [T, B] per-step columns ope_eval would have collected"""
    return dict(pi=np.ascontiguousarray(x['pi'].T), mu=np.ascontiguousarray(x['mu'].T), q=np.ascontiguousarray(x['q'].T),
                reward=np.ascontiguousarray(x['rhat'].T), logged_reward=np.ascontiguousarray(x['step_rewards'].T))


def _array_path(cols, gamma):
    """script/offline_evaluation.py:38-67 on the [T, B] columns (lists of per-step arrays there), through the array functions.
    The per-episode sums, products and the mean Q are taken in STEP ORDER, which is what the log's estimate does and what numpy
    does for the reference's expressions (np.sum / np.multiply.reduce / np.average along the step axis of a swapaxes view of the
    [T, B] stack): asserted below for B > 1.  At B = 1 that view is contiguous and numpy switches to its pairwise sum, an
    accident of the degenerate shape worth one ulp; the step-order values are the ones compared there."""
    from rl4rs_amd.utils import offline_policy_metrics as M
    rewards = [r for r in cols['reward']]
    action_probs = np.array([p for p in cols['pi']]).swapaxes(0, 1)
    behavior_probs = np.array([p for p in cols['mu']]).swapaxes(0, 1)
    off_rewards = np.array([r for r in cols['logged_reward']]).swapaxes(0, 1)
    rewards_hat = np.array(rewards).swapaxes(0, 1)
    q_values = np.array([q for q in cols['q']]).swapaxes(0, 1)

    def in_step_order(columns, op):
        acc = columns[0].copy()
        for c in columns[1:]:
            acc = op(acc, c)
        return acc
    T = len(rewards)
    episode_reward = in_step_order(cols['reward'], np.add)
    off_rewards_sum = in_step_order(cols['logged_reward'], np.add)
    q_mean = in_step_order(cols['q'], np.add) / T
    action_probs_mul = in_step_order(cols['pi'] * 100, np.multiply)
    behavior_probs_mul = in_step_order(cols['mu'] * 100, np.multiply)
    if rewards_hat.shape[0] > 1:
        assert np.array_equal(episode_reward, np.sum(np.array(rewards), axis=0))
        assert np.array_equal(off_rewards_sum, np.sum(off_rewards, axis=1))
        assert np.array_equal(q_mean, np.average(q_values, 1))
        assert np.array_equal(action_probs_mul, np.multiply.reduce(action_probs * 100, axis=1))
        assert np.array_equal(behavior_probs_mul, np.multiply.reduce(behavior_probs * 100, axis=1))
    ep = M.episode_stats(off_rewards_sum, action_probs_mul, behavior_probs_mul, episode_reward, q_mean)
    st = M.step_stats(off_rewards, action_probs, behavior_probs, rewards_hat, q_values, gamma=gamma)
    out = dict(ep)
    for k in ('wips', 'wips_2', 'seqdr', 'seqdr_2', 'sim_reward'):
        out[k] = st[k]
    return out


def _bits(stats):
    from rl4rs_amd._lib import OPE_STATS
    return np.asarray([stats[k] for k in OPE_STATS], dtype=np.float64).tobytes()


@pytest.mark.parametrize('B,T,seed', [(1, 9, 101), (7, 9, 102), (64, 9, 103), (300, 36, 104), (4096, 32, 106), (1000, 36, 109), (16384, 9, 107)])
def test_handle_path_equals_array_path_bit_for_bit(B, T, seed):
    """T steps recorded column by column, then rl4rs_ope_estimate == the array functions on the same numbers assembled the
    reference's way, bit for bit; two runs are bit-identical; B = 1 and B not a multiple of 64 included."""
    import torch
    from rl4rs_amd.ope import OpeLog
    x = I.estimator_inputs(B, T, seed)
    cols = _columns(x)
    log = OpeLog(B + 3, T + 2)
    runs = []
    for rep in range(2):
        log.begin(B, T)
        for t in range(T):
            for name, arr in cols.items():
                # device float64, host float64: both forms of a column source
                log.record_column(t, name, torch.from_numpy(arr[t]).cuda() if (t + rep) % 2 else arr[t])
        for name, arr in cols.items():
            assert np.array_equal(log.column(name).cpu().numpy(), arr), name
        runs.append((log.estimate(1.0), log.estimate(0.9)))
    log.close()
    assert _bits(runs[0][0]) == _bits(runs[1][0]) and _bits(runs[0][1]) == _bits(runs[1][1])
    for gamma, got in zip((1.0, 0.9), runs[0]):
        want = _array_path(cols, gamma)
        assert _bits(got) == _bits(want), (gamma, got, want)
        assert _bits(_array_path(cols, gamma)) == _bits(want)
    # and the handle's numbers are the reference's
    with np.load(os.path.join(GOLDEN, 'ope_estimators.npz')) as z:
        want = z['expected'][[tuple(c) for c in z['cases']].index((B, T, seed))]
    s1, s9 = runs[0]
    got = [(s1['ips'], s1['ips_c']), (s1['cips'], s1['cips_c']), (s1['snips'], s1['snips_c']), (s1['dr'], s1['dr_se']),
           (s1['wips'], s1['wips_2']), (s9['wips'], s9['wips_2']), (s1['seqdr'], s1['seqdr_2'])]
    for name, g, w in zip(I.ESTIMATOR_NAMES, got, want):
        _close(g, w, RTOL, 'handle %s B=%d T=%d' % (name, B, T))
    _close(s1['sim_reward'], x['rhat'].sum(axis=1).mean(), RTOL, 'sim_reward')


def test_incomplete_log_gives_nan_slots_and_errors_are_reported():
    import torch
    from rl4rs_amd._lib import Rl4rsHipError
    from rl4rs_amd.ope import OpeLog
    log = OpeLog(16, 9)
    with pytest.raises(Rl4rsHipError, match='no epoch begun'):
        log.estimate()
    log.begin(5, 3)
    r = np.arange(15, dtype=np.float64).reshape(3, 5)
    for t in range(3):
        log.record_column(t, 'reward', torch.from_numpy(r[t].astype(np.float32)).cuda())          # float32 source
    s = log.estimate()
    assert s['sim_reward'] == r.sum(axis=0).mean() and np.isnan(s['cips']) and np.isnan(s['wips']) and np.isnan(s['seqdr'])
    with pytest.raises(Rl4rsHipError, match='outside'):
        log.record_column(3, 'reward', r[0])
    with pytest.raises(Rl4rsHipError, match='exceeds'):
        log.begin(17, 9)
    with pytest.raises(ValueError):
        log.record_column(0, 'reward', np.zeros(6))
    log.close()


def _softmax64(s, lo, hi):
    z = s[:, lo:hi].astype(np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


@pytest.mark.parametrize('A,pad', [(284, 0), (284, 4), (283, 0), (382, 0), (382, 1), (7, 0), (1000, 0)])
def test_fused_softmax_propensity(A, pad):
    """pi = softmax(scores[b])[a] in float64 from float32 scores without the [B, A] softmax: rtol 1e-12 against numpy's float64
    softmax of the same float32 scores; the probability form takes the matrix as it is (exact); rows of every alignment (float4 /
    float2 / scalar loads) and a padded row stride; an action outside [0, A) gives NaN."""
    import torch
    from rl4rs_amd.ope import OpeLog
    B = 700
    rs = np.random.RandomState(A + pad)
    full = (rs.randn(B, A + pad) * 4).astype(np.float32)
    scores = torch.from_numpy(full).cuda()[:, :A]
    a = rs.randint(0, A, size=B)
    a[:3] = [0, A - 1, A // 2]
    log = OpeLog(B, 2)
    log.begin(B, 2)
    log.record_policy(0, scores, a, logits=True)
    log.record_policy(1, scores, torch.from_numpy(a).cuda(), logits=False)
    got = log.column('pi').cpu().numpy()
    want = _softmax64(full[:, :A], 0, A)[np.arange(B), a]
    _close(got[0], want, 1e-12, 'fused softmax A=%d pad=%d' % (A, pad))
    assert np.array_equal(got[1], full[np.arange(B), a].astype(np.float64))
    log.record_q(1, scores, a)
    assert np.array_equal(log.column('q').cpu().numpy()[1], full[np.arange(B), a].astype(np.float64))
    # column-offset views: the rows start 4 / 8 bytes off the allocation's alignment, so the load width follows the ADDRESS (with
    # A = 284 + 4 columns of padding the width and the stride are multiples of 4 and only the base is not: scalar, then float2)
    for k in (1, 2):
        W = (A + pad - k) // 4 * 4
        if W < 4:
            continue
        off = torch.from_numpy(full).cuda()[:, k:k + W]
        assert off.data_ptr() % 16 == 4 * k and off.stride(1) == 1 and off.stride(0) == A + pad
        ao = np.minimum(a, W - 1)
        log.record_policy(0, off, ao, logits=True)
        log.record_behavior(1, off, 1, W - 1, ao, logits=True)
        _close(log.column('pi').cpu().numpy()[0], _softmax64(full[:, k:k + W], 0, W)[np.arange(B), ao], 1e-12, 'offset %d A=%d' % (k, A))
        _close(log.column('mu').cpu().numpy()[1], _softmax64(full[:, k:k + W], 1, W - 1)[np.arange(B), np.clip(ao - 1, 0, W - 3)], 1e-12,
               'offset %d, range, A=%d' % (k, A))
    # a score matrix or an action vector of another row count is refused
    with pytest.raises(ValueError, match='do not fit'):
        log.record_policy(0, scores[:B - 1], a, logits=True)
    with pytest.raises(ValueError, match='do not fit'):
        log.record_policy(0, scores, a[:B - 1], logits=True)
    with pytest.raises(ValueError, match='do not fit'):
        log.record_behavior(0, scores[:B - 1], 0, A, a, logits=False)
    bad = a.copy()
    bad[5], bad[6] = A, -1
    log.record_policy(0, scores, bad, logits=True)
    log.record_policy(1, scores, bad, logits=False)
    got = log.column('pi').cpu().numpy()
    assert np.isnan(got[:, 5:7]).all() and np.isfinite(np.delete(got, [5, 6], axis=1)).all()
    log.close()


def _learner_setup(tmp_path):
    from rl4rs_amd import synth
    from rl4rs_amd.data import CatalogTables
    path = os.path.join(str(tmp_path), 'item_info.csv')
    synth.write_text(path, synth.make_catalog_text(seed=21))
    tab = CatalogTables(path, 284, 32)
    cfg = {"maxlen": 64, "batch_size": 2048, "action_size": 284, "dense_feature_num": 432, "category_feature_num": 21, "max_steps": 9,
           "page_items": 9, "action_emb_size": 32, "iteminfo_file": path, "location_mask": tab.location_mask,
           "special_items": tab.special_items}
    rs = np.random.RandomState(3)
    n, D = 700, 266
    x = np.zeros((n, D), np.float32)
    x[:, :256] = rs.randn(n, 256)
    loc = np.asarray(tab.location_mask)
    for i in range(n):
        cur = rs.randint(0, 10)
        for j in range(min(cur, 9)):
            x[i, 256 + j] = rs.choice(np.nonzero(loc[j // 3])[0])
        x[i, -1] = cur
    return cfg, x, rs.randint(0, 284, size=n)


def test_fused_softmax_propensity_against_policy_model(tmp_path):
    """against policy_model.action_probs(obs)[range(B), a] of a DiscreteCQL: rtol 1e-5 (that path is float32 torch.softmax over
    284 terms)"""
    import torch
    from rl4rs.policy.policy_model import policy_model
    from rl4rs_amd import offline_rl as R
    from rl4rs_amd.ope import OpeLog
    cfg, x, a = _learner_setup(tmp_path)
    model = R.DiscreteCQL(cfg, x.shape[1], batch_size=256, seed=5)
    pm = policy_model(model, config=cfg)
    want = pm.action_probs(x)[np.arange(len(a)), a]
    qmat = pm._chunks(model.q, torch.from_numpy(x).cuda())
    log = OpeLog(len(a), 1)
    log.begin(len(a), 1)
    log.record_policy(0, qmat, a, logits=True)
    _close(log.column('pi').cpu().numpy()[0], want, 1e-5, 'fused softmax vs policy_model')
    log.close()
    model.close()


def test_behavior_model_against_the_reference():
    """behavior_model.action_probs against the reference's (fixture 3): rtol 1e-12, layers 1..4 (4 falls into the third range),
    actions 0 and out of range clipped; the logits form against a float64 numpy range-softmax of the same float32 logits: rtol
    1e-12; and on log(y) against the fixture's values: rtol 1e-5 (the logits are rounded to float32 once: 6e-8 relative on a logit
    of magnitude up to ~10 is up to 6e-7 relative after exp; one order of margin)."""
    import torch
    from rl4rs.policy.behavior_model import behavior_model
    with np.load(os.path.join(GOLDEN, 'ope_behavior.npz')) as z:
        actions, layers, want = z['actions'], z['layers'], z['expected']
    y, a = I.behavior_inputs()
    assert np.array_equal(a, actions) and list(layers) == [1, 2, 3, 4]
    y32 = y.astype(np.float32)
    assert np.array_equal(y32.astype(np.float64), y)
    bm = behavior_model({}, types_predict(y32))
    assert not bm.logits and not bm.takes_observation
    for layer, w in zip(layers, want):
        got = bm.action_probs(None, actions, int(layer), page=0)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == w.shape
        _close(got, w, 1e-12, 'behaviour rule layer %d' % layer)
    # device tensors in -> device tensor out; a callable model
    got = behavior_model({}, lambda record: torch.from_numpy(y32).cuda()).action_probs(None, torch.from_numpy(actions).cuda(), 2)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), bm.action_probs(None, actions, 2))
    # logits
    rs = np.random.RandomState(5)
    z32 = (rs.randn(*y.shape) * 3).astype(np.float32)
    bl = behavior_model({}, types_predict(z32), logits=True)
    ranges = {1: (1, 40), 2: (40, 148), 3: (148, 382), 4: (148, 382)}
    for layer in (1, 2, 3, 4):
        lo, hi = ranges[layer]
        idx = np.clip(actions - lo, 0, hi - lo - 1)
        _close(bl.action_probs(None, actions, layer), _softmax64(z32, lo, hi)[np.arange(len(actions)), idx], 1e-12, 'logit rule layer %d' % layer)
    blog = behavior_model({}, types_predict(np.log(y).astype(np.float32)), logits=True)
    for layer, w in zip(layers, want):
        _close(blog.action_probs(None, actions, int(layer)), w, 1e-5, 'log(y) layer %d' % layer)


def types_predict(y):
    import types
    return types.SimpleNamespace(predict=lambda record: y)


@pytest.mark.parametrize('case', range(len(I.LOOP_CASES)), ids=['B%d_T%d_%s' % (b, t, 'model' if s else 'rewards') for b, t, s, _ in I.LOOP_CASES])
def test_ope_eval_against_the_reference_loop(case, capsys):
    """ope_eval fed the table-driven fakes the reference's own ope_eval was fed: its two printed arrays, rtol 1e-9"""
    from rl4rs_amd.ope import ope_eval
    B, T, with_model, seed = I.LOOP_CASES[case]
    with np.load(os.path.join(GOLDEN, 'ope_loop.npz')) as z:
        assert tuple(z['cases'][case]) == I.LOOP_CASES[case]
        mean, std = z['mean'][case], z['std'][case]
    fake = I.LoopTables(B, T, seed)
    out = ope_eval(dict(epoch=I.LOOP_EPOCHS, batch_size=B, max_steps=T, page_items=9), fake, fake, sample_model=fake if with_model else None)
    printed = capsys.readouterr().out
    assert printed.count('test batch at ') == I.LOOP_EPOCHS and 'IS DR WIPS SeqDR' in printed
    assert fake.epoch == I.LOOP_EPOCHS - 1 and fake.j == T
    _close(out['episode_reward'], fake.reward.sum(axis=1).mean(), RTOL, 'episode reward')
    if with_model:
        assert out['metrics'].shape == (I.LOOP_EPOCHS, 4, 2)
        _close(out['mean'], mean, RTOL, 'mean B=%d T=%d' % (B, T))
        _close(out['std'], std, RTOL, 'std B=%d T=%d' % (B, T))
        assert np.array_equal(out['mean'], np.average(out['metrics'], axis=0)) and np.array_equal(out['std'], np.std(out['metrics'], axis=0))
    else:
        assert out['metrics'].shape == (0, 4, 2) and np.isnan(out['mean']).all() and np.isnan(out['std']).all()
        assert np.isnan(mean).all() and np.isnan(std).all()


def _env_config(d, seq):
    from rl4rs_amd import synth
    text = synth.make_catalog_text(seed=4)
    synth.write_text(os.path.join(d, 'item_info.csv'), text)
    synth.write_records(os.path.join(d, 'log.csv'),
                        synth.make_records(512, pages=4 if seq else 1, seed=2, hash_size=2000, special_ids=synth.special_ids_from_text(text)))
    return {"epoch": 2, "maxlen": 64, "batch_size": 96, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
            "category_feature_num": 21, "category_hash_size": 2000, "seq_num": 2, "emb_size": 128, "hidden_units": 128,
            "max_steps": 36 if seq else 9, "sample_file": os.path.join(d, 'log.csv'), "page_items": 9, "action_emb_size": 32,
            "iteminfo_file": os.path.join(d, 'item_info.csv'), "support_d3rl_mask": True, "is_eval": True, "cache_size": 96,
            "model_seed": 3, "return_tensors": True}


def _make_env(cfg, seq):
    import rl4rs
    if seq:
        from rl4rs.env.seqslate import SeqSlateRecEnv, SeqSlateState
        return rl4rs.make('SeqSlateRecEnv-v0', recsim=SeqSlateRecEnv(cfg, state_cls=SeqSlateState))
    from rl4rs.env.slate import SlateRecEnv, SlateState
    return rl4rs.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))


@pytest.mark.parametrize('seq', [False, True], ids=['slate', 'seqslate'])
def test_ope_eval_end_to_end_on_the_device(tmp_path, seq):
    """train -> generate_offline_dataset -> DiscreteBC as behaviour model -> DiscreteCQL as policy -> ope_eval, 2 epochs, device env:
    the returned metrics equal the array functions (pinned to the reference by fixture 1) applied to the columns read back from the
    log, assembled as ope_eval:38-67 does, bit for bit; and the log's columns equal what policy_model / behavior_model / the env
    return when called the reference's way, step by step, on the same episodes: actions, rewards and logged rewards exactly, mu
    rtol 1e-12 against the float64 rule on the model's own float32 scores, pi and q rtol 1e-5 against policy_model's float32 paths."""
    import torch
    from rl4rs.policy.behavior_model import behavior_model
    from rl4rs.policy.policy_model import policy_model
    from rl4rs_amd import offline_rl as R
    from rl4rs_amd.offline import generate_offline_dataset
    from rl4rs_amd.ope import ope_eval
    from rl4rs_amd.policy.behavior_model import layer_range
    cfg = _env_config(str(tmp_path), seq)
    B, T = cfg['batch_size'], cfg['max_steps']
    dataset = generate_offline_dataset(_make_env(dict(cfg, is_eval=False), seq), epochs=3, shuffle=True)
    obs_dim = dataset['observations'].shape[1]
    bc = R.DiscreteBC(cfg, obs_dim, batch_size=64, seed=1)
    bc.fit_mdp(dataset, n_epochs=1)
    cql = R.DiscreteCQL(cfg, obs_dim, batch_size=64, seed=2)
    cql.fit_mdp(dataset, n_epochs=1)
    sample_model = behavior_model(cfg, bc)
    assert sample_model.logits and sample_model.takes_observation
    columns = []

    def on_epoch(epoch, log, actions, offline_actions):
        cols = dict((name, log.column(name).cpu().numpy()) for name in ('pi', 'mu', 'q', 'reward', 'logged_reward'))
        cols['action'] = np.stack([a.cpu().numpy() for a in actions])
        cols['offline_action'] = np.stack([a.cpu().numpy().astype(np.int64) for a in offline_actions])
        assert epoch == len(columns)
        columns.append(cols)
    out = ope_eval(cfg, _make_env(cfg, seq), cql, sample_model=sample_model, on_epoch=on_epoch)
    assert out['metrics'].shape == (2, 4, 2) and len(columns) == 2
    assert np.isfinite(out['metrics']).all(), out['metrics']
    # (a) the metrics are the array functions on the log's columns
    for e in range(2):
        cols = columns[e]
        s = _array_path(cols, 1.0)
        want = np.array([(s['cips'], s['cips_c']), (s['dr'], s['dr_se']), (s['wips'], s['wips_2']), (s['seqdr'], s['seqdr_2'])])
        assert out['metrics'][e].tobytes() == want.tobytes(), (e, out['metrics'][e], want)
        assert out['stats'][e]['sim_reward'] == s['sim_reward']
    # (b) the columns are what the reference-shaped calls return on the same episodes
    env = _make_env(cfg, seq)
    pm = policy_model(cql, config=cfg)
    for e in range(2):
        cols = columns[e]
        obs = env.reset()
        for j in range(T):
            action = pm.predict_with_mask(obs)
            off = env.offline_action
            off_h = off.cpu().numpy().astype(np.int64)
            pi = pm.action_probs(obs)[torch.arange(B), off.long()].cpu().numpy()
            q = pm.predict_q(obs, action).cpu().numpy()
            y = sample_model.scores(obs).cpu().numpy()
            assert y.dtype == np.float32
            lo, hi = layer_range(j // 3 + 1, y.shape[1])
            mu = _softmax64(y, lo, hi)[np.arange(B), np.clip(off_h - lo, 0, hi - lo - 1)]
            obs, reward, done, info = env.step(action)
            logged = env.offline_reward
            logged = logged.cpu().numpy() if isinstance(logged, torch.Tensor) else np.asarray(logged, dtype=np.float64)
            assert np.array_equal(cols['action'][j], action.cpu().numpy()), (e, j)
            assert np.array_equal(cols['offline_action'][j], off_h), (e, j)
            assert np.array_equal(cols['reward'][j], reward.cpu().numpy().astype(np.float64)), (e, j)
            assert np.array_equal(cols['logged_reward'][j], logged), (e, j)
            _close(cols['mu'][j], mu, 1e-12, 'mu epoch %d step %d' % (e, j))
            _close(cols['pi'][j], pi, 1e-5, 'pi epoch %d step %d' % (e, j))
            _close(cols['q'][j], q, 1e-5, 'q epoch %d step %d' % (e, j))
    # sample_model=None: rewards only
    out0 = ope_eval(cfg, _make_env(cfg, seq), cql)
    assert out0['metrics'].shape == (0, 4, 2) and np.isfinite(out0['episode_reward'])
    assert abs(out0['episode_reward'] - out['episode_reward']) <= 1e-12 * abs(out['episode_reward'])
    with pytest.raises(ValueError, match='predict_value'):
        ope_eval(cfg, _make_env(cfg, seq), bc, sample_model=sample_model)
    bc.close()
    cql.close()
