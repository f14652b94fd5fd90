"""CPU: the float64 restatement of Exact-K (tests/exactk_ref.py) against finite differences and the numpy oracle env, the recorded
fp32 yardstick, the exclusion caps of the GPU tests' pick comparisons, the trainer's host logic and the create-time refusals."""
import ctypes as C

import numpy as np
import pytest

import exactk_ref as R
from helpers import load_scenario


def test_gradient_agrees_with_central_finite_differences():
    """Tiny shape A = 11, H = 16, heads = 2, 1 block, N = 3: two random coordinates of every tensor (the used table rows only)."""
    c = R.make_case(R.TINY_SHAPE, 5)
    dm = c['dm']
    args = (c['obs'], c['path'], c['w'], dm, c['loc'], c['special'])
    ref = R.loss_and_grad(c['flat'], *args)
    flat = c['flat'].astype(np.float64)
    rs = np.random.RandomState(0)
    o, worst = 0, 0.0
    for name, shp, _ in R.NX.shapes(dm.od, dm.H, dm.blocks, dm.vocab):
        k = int(np.prod(shp))
        for i in rs.choice(np.arange(o, o + (dm.A * dm.H if name == 'table' else k)), 2):
            e = 1e-6
            hi, lo = flat.copy(), flat.copy()
            hi[i] += e
            lo[i] -= e
            fd = (R.loss_only(hi, *args) - R.loss_only(lo, *args)) / (2 * e)
            worst = max(worst, abs(fd - ref['grad'][i]))
        o += k
    gmax = np.abs(ref['grad']).max()
    print('worst finite-difference gap %.3g (gradient max-norm %.3g)' % (worst, gmax))
    # central differences at e = 1e-6: truncation e^2 f''' / 6 and float64 rounding 1e-16 |loss| / e, both far below 1e-7
    assert worst < 1e-7 * max(gmax, 1.0)
    # the unused table rows get no gradient
    assert not dm.split(ref['grad'])['table'][dm.A:].any()


def test_allowed_sets_equal_the_oracle_envs_masks():
    """Random valid slates on tests/golden/catalog_synth.csv: the restated rule against the numpy oracle stepping the same slates."""
    from oracle.state import OracleState
    m, cfg, records, g = load_scenario('slate_discrete')
    st = OracleState(cfg, records)
    loc, special = np.asarray(st.cat.location_mask[:3]).astype(bool), np.asarray(st.cat.is_special).astype(bool)
    loc2, special2 = R.synth_masks(cfg['action_size'])
    assert np.array_equal(loc, loc2) and np.array_equal(special, special2)
    B = len(st.obs_action_mask())
    path = R.random_slates(B, loc, special, np.random.RandomState(1))
    allowed = R.allowed_sets(path, loc, special)
    saw_special = False
    for t in range(R.T):
        assert np.array_equal(np.asarray(st.obs_action_mask()).astype(bool), allowed[:, t]), t
        st.act(path[:, t])
        saw_special |= bool(special[path[:, t]].any())
    assert saw_special                                  # the special-item rule was exercised


def test_shapes_are_in_the_forms_they_were_chosen_for():
    """exactk_ref.sample_axis_forms restates the chunk rules of csrc/exactk.hip: shapes 0 - 3 and the tiny shape stay in the single-chunk
    form of every reduction, shapes 4 - 6 cross the thresholds they were chosen for (and no smaller N does)."""
    forms = lambda s: R.sample_axis_forms(s[0], s[4])
    for s in R.GPU_SHAPES[:4] + (R.TINY_SHAPE,):
        assert forms(s) == dict(colsum_rows_chunks=1, tn_rows_chunks=1, loss_trips=1, tn_items_chunk=256, colsum_items_chunk=64,
                                tn_decoder_chunk=256), s
    assert R.GPU_SHAPES[4:] == ((75, 32, 2, 1, 900), (40, 16, 2, 1, 1900), (284, 64, 4, 2, 66))
    f = forms(R.GPU_SHAPES[4])                                     # every row of the table but the decoder's
    assert f['colsum_rows_chunks'] > 1 and f['tn_rows_chunks'] > 1 and f['loss_trips'] > 1 and f['tn_items_chunk'] > 256
    assert f['colsum_items_chunk'] > 64 and f['colsum_items_chunk'] % 8 != 0 and f['tn_decoder_chunk'] == 256
    assert R.sample_axis_forms(75, 873)['colsum_items_chunk'] == 64            # M = 65 475: N = 874 is the first past 65 536
    f = forms(R.GPU_SHAPES[5])                                     # the decoder's as well
    assert f['tn_decoder_chunk'] > 256 and f['colsum_items_chunk'] > 64 and f['colsum_items_chunk'] % 8 != 0
    assert f['colsum_rows_chunks'] > 1 and f['tn_rows_chunks'] > 1 and f['loss_trips'] > 1 and f['tn_items_chunk'] > 256
    assert R.sample_axis_forms(40, 1820)['tn_decoder_chunk'] == 256            # 9 N = 16 380
    f = forms(R.GPU_SHAPES[6])                                     # the reference's widths: M > 16384 and N > 64, nothing else
    assert f == dict(colsum_rows_chunks=2, tn_rows_chunks=1, loss_trips=1, tn_items_chunk=304, colsum_items_chunk=64, tn_decoder_chunk=256)
    assert R.sample_axis_forms(284, 57)['tn_items_chunk'] == 256               # M = 16 188: N = 58 is the first past 16 384
    # the critic's extra row counts (tests/test_gpu_exactk.py): 2 and 17 chunks, the last of 4099 ragged
    assert [R.sample_axis_forms(1, n)['tn_rows_chunks'] for n in (37, 1, 300, 4099)] == [1, 1, 2, 17] and 4099 % 256 == 3


def _keys():
    return list(R.CASE_KEYS) + ['crafted']


@pytest.mark.parametrize('key', _keys(), ids=str)
def test_recorded_yardstick_is_reproduced(key):
    c = R.crafted_case() if key == 'crafted' else R.case(*key)
    y = R.fp32_yardstick(c, seed=5, step=7)
    m = R.MEASURED[key]
    print(key, dict((k, y[k]) for k in m), m)
    for k in m:
        assert m[k] / 2.0 <= y[k] <= 2.0 * m[k], (key, k, y[k], m[k])
    # the recorded gradient figure is the rounding level, not one relu unit on the other side of 0: no tensor stands out of it
    assert max(y['per_tensor'].values()) <= 2.0 * m['grad_rel']


@pytest.mark.parametrize('key', _keys(), ids=str)
def test_case_seeds_do_not_sit_on_a_relu_kink(key):
    """The second condition on a case's seed: float32 runs with every parameter moved by one float32 rounding keep the gradient
    error inside the bar, so the recorded rounding level is not one accumulation order's luck."""
    c = R.crafted_case() if key == 'crafted' else R.case(*key)
    ref = R.loss_and_grad(c['flat'], c['obs'], c['path'], c['w'], c['dm'], c['loc'], c['special'], seed=5, step=7)
    errs = R.rounding_variants(c, ref, seed=5, step=7)[0]
    print(key, errs)
    assert max(errs) < R.BAR_FACTOR * R.MEASURED[key]['grad_rel'], (key, errs)


@pytest.mark.parametrize('key', R.KINK_KEYS, ids=str)
def test_large_case_seeds_keep_their_relu_units_off_zero(key):
    """The third condition on a seed, for the shapes of millions of relu units per layer: every unit that carries at least the
    gradient bar lies farther from 0 (float64) than KINK_MARGIN x the rms float32 error of its layer's pre-activations."""
    c = R.case(*key)
    bar = R.BAR_FACTOR * R.MEASURED[key]['grad_rel']
    for s in R.relu_sites(c, seed=5, step=7):
        heavy = s['g'] >= bar
        nearest = float(s['z'][heavy].min()) if heavy.any() else np.inf
        print(key, '%-9s %d units, %d carry the bar, nearest to 0 at %.3g = %.2f rms (rms %.3g)'
              % (s['name'], s['z'].size, int(heavy.sum()), nearest, nearest / s['rms'], s['rms']))
        assert nearest >= R.KINK_MARGIN * s['rms'], (key, s['name'], nearest, s['rms'])


@pytest.mark.parametrize('N', sorted(R.CRITIC_SEEDS))
def test_critic_inputs_keep_their_relu_units_off_zero(N):
    """The critic comparisons' inputs (tests/test_gpu_exactk.py): no hidden unit whose flip would show above the rounding level sits
    within CRITIC_KINK_MARGIN rms of a float32 pre-activation error of 0, so the float32 yardstick is the rounding level on any CPU."""
    for s in R.critic_relu_sites(*R.critic_case(N)):
        heavy = s['g'] >= 2.0 ** -23
        nearest = float(s['z'][heavy].min())
        print(N, '%s %d units, %d carry 2^-23, nearest to 0 at %.3g = %.2f rms' % (s['name'], s['z'].size, int(heavy.sum()), nearest, nearest / s['rms']))
        assert nearest >= R.CRITIC_KINK_MARGIN * s['rms'], (N, s['name'], nearest, s['rms'])
    # the inputs of the row counts that came first are the draws of RandomState(70 + N), as they always were
    assert all(R.CRITIC_SEEDS[n] == 70 + n for n in (37, 1, 300))


@pytest.mark.parametrize('i', R.DECODE_SHAPES)
def test_exclusion_caps_hold_with_the_restatement_alone(i):
    """The restatement's own slates at the seeds of tests/test_gpu_exactk.py (decode pass, dropout 0.1): rows with a top-two gap
    under 10 x the logit bar at some step and sampled picks within the CDF-edge bar stay under 1 %."""
    key = (i, 0.1)
    c = R.case(*key)
    N = c['N']
    logit_bar = R.BAR_FACTOR * R.MEASURED[key]['logit']
    args = (c['flat'], c['obs'], c['dm'], c['loc'], c['special'])
    seed, step = R.DECODE_STREAMS[i]
    path = R.decode(*args, greedy=True, seed=seed, step=step)
    lg = R.logits_of(c['flat'], c['obs'], path, c['dm'], c['loc'], c['special'], seed=seed, step=step, pas=1)
    soft_rows = int((R.top_two_gap(lg) < 10.0 * logit_bar).any(axis=1).sum())
    assert soft_rows <= 0.01 * N, (soft_rows, N)
    path = R.decode(*args, greedy=False, seed=seed, step=step)
    lg = R.logits_of(c['flat'], c['obs'], path, c['dm'], c['loc'], c['special'], seed=seed, step=step, pas=1)
    pick, dist = R.draw(lg, R.sample_u(N, seed, step))
    assert np.array_equal(pick, path)
    near = int((dist <= R.edge_bar(logit_bar)).sum())
    assert near <= 0.01 * dist.size, (near, dist.size)
    assert all(len(set(r.tolist())) == R.T for r in path)
    assert R.allowed_sets(path, c['loc'], c['special'])[np.arange(N)[:, None], np.arange(R.T)[None, :], path].all()


def test_learning_run_of_the_restatement_is_the_recorded_one():
    """LEARN_REF_GAIN, what the GPU learning test is measured against: the float32 CPU restatement, re-run."""
    c = R.learn_setup()
    before, after = R.learn_loop(R.RefBackend(c), c['favoured'], R.LEARN_UPDATES)
    print('mean greedy reward %.6f -> %.6f' % (before, after))
    assert R.LEARN_UPDATES == 30 and R.LEARN_REF_GAIN >= 2.0
    assert abs((after - before) - R.LEARN_REF_GAIN) < 1e-9


# ---- host logic of the trainer ---------------------------------------------------------------------------------------------
def test_best_of_two_with_ties_and_advantage_normalisation():
    import torch
    from rl4rs_amd.train import ExactKTrainer
    r = torch.tensor([[1.0, 5.0, 3.0, 2.0], [2.0, 5.0, 1.0, 2.0]])
    p = torch.stack([torch.zeros((4, 9), dtype=torch.int32), torch.ones((4, 9), dtype=torch.int32)])
    best_r, best_p = ExactKTrainer.select_best(r, p)
    assert best_r.tolist() == [2.0, 5.0, 3.0, 2.0]
    assert best_p[:, 0].tolist() == [1, 0, 0, 0]                    # ties keep the first climb
    assert np.array_equal(R.best_of(r.numpy()), [1, 0, 0, 0])
    base = torch.tensor([1.0, 1.0, 2.0, 0.5])
    w, skip = ExactKTrainer.normalise_advantage(best_r, base)
    want, sk = R.advantage(best_r.numpy(), base.numpy())
    assert int(skip) == 0 and not sk and np.allclose(w.numpy(), want, rtol=1e-6)
    # zero std: the update is skipped and the weights are zero, not inf / nan
    w, skip = ExactKTrainer.normalise_advantage(torch.full((4,), 3.0), torch.full((4,), 1.0))
    assert int(skip) == 1 and not w.any() and R.advantage(np.full(4, 3.0), np.full(4, 1.0))[1]
    w, skip = ExactKTrainer.normalise_advantage(torch.tensor([1.0, float('nan')]), torch.zeros(2))
    assert int(skip) == 1 and not w.any()


class _FakeEnv(object):
    def __init__(self, **over):
        self.config = dict(batch_size=4, max_steps=9, action_size=284, return_tensors=True)
        self.config.update(over)


def test_trainer_refuses_what_it_does_not_implement():
    from rl4rs_amd.train import ExactKTrainer
    with pytest.raises(ValueError, match='SeqSlateRecEnv-v0.*36 steps'):
        ExactKTrainer(_FakeEnv(max_steps=36))
    with pytest.raises(ValueError, match='discrete-action'):
        ExactKTrainer(_FakeEnv(support_conti_env=True))
    with pytest.raises(ValueError, match='return_tensors'):
        ExactKTrainer(_FakeEnv(return_tensors=False))
    for kw in (dict(temperature=2), dict(num_glimpse=2), dict(num_layers=2), dict(use_mha=False)):
        with pytest.raises(ValueError, match=list(kw)[0]):
            ExactKTrainer(_FakeEnv(), **kw)


# ---- create-time refusals ----------------------------------------------------------------------------------------------------
def _create(lib, loc=None, special=None, **over):
    from rl4rs_amd import _lib
    f = dict(obs_dim=256, hidden=64, heads=4, blocks=2, action_size=284, vocab=500, max_rows=64, dropout_rate=0.1)
    f.update(over)
    cfg = _lib.ExactKCfg(f['obs_dim'], f['hidden'], f['heads'], f['blocks'], f['action_size'], f['vocab'], f['max_rows'], f['dropout_rate'])
    A = f['action_size']
    loc = np.ones((3, A), dtype=np.uint8) if loc is None else np.ascontiguousarray(loc, dtype=np.uint8)
    special = np.zeros(A, dtype=np.uint8) if special is None else np.ascontiguousarray(special, dtype=np.uint8)
    dummy = np.zeros(1, dtype=np.float32)
    h = C.c_void_p()
    rc = lib.rl4rs_exactk_create(C.byref(cfg), dummy.ctypes.data_as(C.c_void_p), loc.ctypes.data_as(C.c_void_p),
                                 special.ctypes.data_as(C.c_void_p), None, C.byref(h))
    return rc, lib.rl4rs_last_error().decode(), h, lib.rl4rs_exactk_param_count(C.byref(cfg))


def test_create_refuses_with_the_reason_before_a_device_is_looked_for():
    from rl4rs_amd import _lib
    from rl4rs_amd.build import build_lib
    build_lib()
    lib = _lib.load()
    thin = np.ones((3, 284), dtype=np.uint8)
    thin[1, 8:] = 0                                               # location 1 allows 8 items
    sp = np.zeros(284, dtype=np.uint8)
    sp[:276] = 1                                                  # 8 non-special items in all
    for kw, words in ((dict(heads=3), ('num_heads', 'head width')), (dict(hidden=24), ('hidden_units', '16')),
                      (dict(hidden=16, heads=8), ('head width', 'multiple of 8')),
                      (dict(action_size=501), ('action_size', 'vocab')), (dict(blocks=0), ('num_blocks',)),
                      (dict(max_rows=7385), ('max_rows', '2^31', '7384')), (dict(max_rows=1 << 30), ('max_rows', '2^31')),
                      (dict(loc=thin), ('location mask 1', '8', '9')), (dict(special=sp), ('location mask 0', '8'))):
        rc, msg, h, n = _create(lib, **kw)
        assert rc == -1 and not h.value, (kw, rc, msg)             # RL4RS_EINVAL, no handle
        for w in words:
            assert w in msg, (kw, msg)
        if 'loc' not in kw and 'special' not in kw:
            assert n == -1
    if lib.rl4rs_device_count() <= 0:
        # admitted shapes get as far as the device check (the bound of max_rows itself included)
        for kw in (dict(), dict(max_rows=7384), dict(hidden=16, heads=2, blocks=1, action_size=9, vocab=9)):
            rc, msg, h, n = _create(lib, **kw)
            assert rc == -2 and 'no HIP device' in msg and n > 0, (kw, rc, msg)
    cfg = _lib.ExactKCfg(256, 64, 4, 2, 284, 500, 64, 0.1)
    assert lib.rl4rs_exactk_param_count(C.byref(cfg)) == R.NX.param_count(256, 64, 2, 500)
