"""The lazy form of the duplicates' expansion: with the row dedup's second tier on, a forward launches no k_row_expand -
observation-shaped forwards compute every head row from the representative's all-feature row (k_gemm_h16_gather), reward-shaped
forwards without a caller's obs buffer read the representative's head row in k_head_prob_rep - and rl4rs_dien_buffer completes the
duplicates' internal rows when they are asked for.  Everything is pinned BIT FOR BIT against the same weights with
scorer_kernels='no_lazy_expand' (k_row_expand behind the head GEMM in every forward), in some cases against 'no_row_dedup' as
well: obs, prob and obs_last of every row, ALL_FEATURE, SCORES and QUERY of every row through net.snapshot.

Shapes: hidden_units 128 and the flagship feature widths, maxlen 16 (one case at 64).  Group 1: R = 1, 31, 32, 33, 65, 257 (the
edges of the 32-row head tile, one row past eight tiles).  Groups of 9: 1, 7, 8 and 29 groups (63 rows = 7 groups, the AUGRU's
group-9 tile: one partial tile, the edge, several tiles).  Duplicate patterns: none, all groups equal, A B A runs (which cross
every tile edge, 32 and 63 being no multiples of 3), and - under a row order - duplicates whose representative is a physically
later row."""
import functools
import os

import numpy as np
import pytest

import test_gpu_tier2_active_rows as t2

pytestmark = pytest.mark.gpu

MAXR = 264                  # every case below fits one pair of handles (29 groups of 9 = 261 rows)
NSLOTS = t2.NSLOTS
ARMS = ('', 'no_lazy_expand')
NAMES = ('obs', 'prob', 'obs_last', 'all_feature', 'scores', 'query')


@functools.lru_cache(maxsize=None)
def _nets(L=16, arms=ARMS):
    import torch
    from rl4rs_amd.device import DeviceDien
    seq = t2._histories()[:, :, 64 - L:]              # (the leading padding of a third of input 0 stays in front at L = 64 only)
    if L < 64:
        seq = seq.copy()
        seq[: NSLOTS // 3, 0, : L // 2] = 0
    nets = []
    for kernels in arms:
        net = DeviceDien(dict(t2.CFG, maxlen=L, scorer_kernels=kernels), t2._weights(), max_rows=MAXR, max_slots=NSLOTS)
        for s in range(2):
            net.encode(s, torch.from_numpy(np.ascontiguousarray(seq[:, s])).cuda(), 0)
        nets.append(net)
    return nets


def _runs(pattern, ng):
    """run layout (t2._groups) of ng groups: 'distinct' no two groups equal, 'identical' one template, 'aba' runs of A B A"""
    if pattern == 'identical':
        return ['A' * ng]
    unit = 'ABCDE' if pattern == 'distinct' else 'ABA'
    runs = [unit] * (ng // len(unit))
    return runs + ([unit[: ng % len(unit)]] if ng % len(unit) else [])


def _inputs(pattern, ng, group, ordered, seed=0):
    rs = np.random.RandomState(1000 * group + ng + seed)
    slots, dense, cat = t2._groups(_runs(pattern, ng), group, rs)
    assert slots.shape[1] == ng
    order = None
    if ordered:
        slots, dense, cat, order = t2._scatter(slots, dense, cat, group, 5 + seed)
    return slots, dense, cat, order


def _forward(net, R, group, inputs, caller_obs=True, partition=False, count=False, snapshots=True):
    """-> dict(out=[obs, prob, obs_last, all_feature, scores, query] (None where not produced), n_active, rep, plan, counts)"""
    import torch
    from rl4rs_amd.device import DIEN_ALL_FEATURE, DIEN_SCORES, DIEN_QUERY, DIEN_N_ACTIVE, DIEN_ROW_REP, DIEN_ROW_ACTIVE
    slots, dense, cat, order = inputs
    ng = R // group
    sl, d, c = torch.from_numpy(np.ascontiguousarray(slots)).cuda(), torch.from_numpy(dense).cuda(), torch.from_numpy(cat).cuda()
    net.set_row_order(None if order is None else torch.from_numpy(np.asarray(order, dtype=np.int32)).cuda())
    dedup = 'no_row_dedup' not in net.kernel_opts
    if partition:           # the partition a content forward finds, handed back in: this forward launches no k_row_dedup
        net.forward(R, group, d, c, sl, True, True)
        held = [net.snapshot(w, 0)[:n].clone() for w, n in ((DIEN_ROW_REP, ng), (DIEN_ROW_ACTIVE, ng), (DIEN_N_ACTIVE, 1))]
        net.set_row_partition(*held)
    net.set_profiling(1 if count else 0)
    net.profile_reset()
    last = group > 1
    res = net.forward(R, group, d, c, sl, caller_obs, True, want_obs_last=last)
    out = [res[0].clone() if caller_obs else None, res[1].clone(), res[2].clone() if last else None]
    r = dict(plan=net.last_plan(), counts=None, n_active=None, rep=None)
    if count:
        r['counts'] = dict((k, v[1]) for k, v in net.profile().items())
    if snapshots:
        out += [net.snapshot(DIEN_ALL_FEATURE, 0)[:R].clone(), net.snapshot(DIEN_SCORES, 0)[:, :R].clone(), net.snapshot(DIEN_QUERY, 0)[:R].clone()]
        if count:           # completing the internal rows records nothing
            assert dict((k, v[1]) for k, v in net.profile().items()) == r['counts']
    if dedup:
        r['n_active'] = int(net.snapshot(DIEN_N_ACTIVE, 0)[0].item())
        r['rep'] = net.snapshot(DIEN_ROW_REP, 0)[:ng].cpu().numpy()
        if partition:
            assert net.dedup_counts() == (0, 1)
    net.set_profiling(0)
    net.check_status()
    r['out'] = out
    return r


def _same(a, b, what):
    import torch
    assert len(a) == len(b)
    for name, x, y in zip(NAMES, a, b):
        if x is None:
            assert y is None, (what, name)
            continue
        assert torch.isfinite(x).all(), (what, name)
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (what, name)


def _expect_dups(pattern, ng, n_active):
    if pattern == 'distinct' or ng == 1:
        assert n_active == ng
    elif pattern == 'identical':
        assert n_active < ng and n_active <= (ng + t2.CAP - 1) // t2.CAP + 1      # (the look-back window: row_dedup.hpp)
    elif ng >= 3:
        assert n_active < ng


def _pair(R, group, pattern, ordered, want, L=16, **kw):
    """the default handle against its no_lazy_expand twin on one forward; `want`: the expand token the default must report"""
    ng = R // group
    inputs = _inputs(pattern, ng, group, ordered)
    on, off = [_forward(net, R, group, inputs, **kw) for net in _nets(L)]
    what = (R, group, pattern, ordered, sorted(kw.items()))
    assert on['plan']['expand'] == want and off['plan']['expand'] == 'behind:768', (what, on['plan'], off['plan'])
    assert {k: v for k, v in on['plan'].items() if k != 'expand'} == {k: v for k, v in off['plan'].items() if k != 'expand'}
    _same(on['out'], off['out'], what)
    assert on['n_active'] == off['n_active'] and np.array_equal(on['rep'], off['rep'])
    _expect_dups(pattern, ng, on['n_active'])
    if ordered and pattern != 'distinct' and ng >= 3:      # some duplicate's representative is a physically later row
        assert (on['rep'] > np.arange(ng)).any()
    return on, off


PATTERNS = ('distinct', 'identical', 'aba')


@pytest.mark.parametrize('R', [1, 31, 32, 33, 65, 257])
def test_observation_shaped(R):
    for pattern in PATTERNS:
        for ordered in (False, True):
            _pair(R, 1, pattern, ordered, 'lazy:768')
    _pair(R, 1, 'aba', True, 'lazy:768', partition=True)
    _pair(R, 1, 'aba', False, 'lazy:768', caller_obs=False)         # the head output stays in the handle: complete there too


@pytest.mark.parametrize('ng', [1, 7, 8, 29])
def test_groups_of_nine_without_a_caller_obs(ng):
    for pattern in PATTERNS:
        for ordered in (False, True):
            _pair(ng * 9, 9, pattern, ordered, 'lazy:768', caller_obs=False)
    _pair(ng * 9, 9, 'aba', True, 'lazy:768', caller_obs=False, partition=True)


def test_groups_of_nine_with_a_caller_obs_keep_their_plan():
    for pattern in PATTERNS:
        for ordered in (False, True):
            _pair(72, 9, pattern, ordered, 'behind:768')
    _pair(72, 9, 'aba', True, 'behind:768', partition=True)


def test_groups_of_eight():
    for pattern in PATTERNS:
        for ordered in (False, True):
            _pair(72, 8, pattern, ordered, 'lazy:768', caller_obs=False)
            _pair(72, 8, pattern, ordered, 'behind:768')
    _pair(72, 8, 'aba', True, 'lazy:768', caller_obs=False, partition=True)


def test_maxlen_64():
    _pair(65, 1, 'aba', True, 'lazy:768', L=64)
    _pair(72, 9, 'aba', True, 'lazy:768', L=64, caller_obs=False)


def test_against_no_row_dedup():
    """... and against the handle that scores every row itself: a duplicate's row is the row it would have computed"""
    plain = _nets(16, ('no_row_dedup',))[0]
    for R, group, caller_obs in ((65, 1, True), (72, 9, False)):
        inputs = _inputs('aba', R // group, group, True)
        on = _forward(_nets()[0], R, group, inputs, caller_obs=caller_obs)
        ref = _forward(plain, R, group, inputs, caller_obs=caller_obs)
        assert on['plan']['expand'] == 'lazy:768' and ref['plan']['expand'] == 'none:0'
        _same(on['out'], ref['out'], (R, group))


def test_snapshot_twice_and_profile_counts():
    """A second snapshot finds nothing pending: equal tensors, no profile entry from either.  One forward of each shape counts
    the same entries per class on both handles - the lazy forward keeps an empty entry where k_row_expand was."""
    from rl4rs_amd.device import DIEN_ALL_FEATURE, DIEN_SCORES, DIEN_QUERY
    import torch
    for R, group, caller_obs, want in ((65, 1, True, 'lazy:768'), (72, 9, False, 'lazy:768'), (72, 9, True, 'behind:768'), (72, 8, False, 'lazy:768')):
        inputs = _inputs('aba', R // group, group, False)
        on, off = [_forward(net, R, group, inputs, caller_obs=caller_obs, count=True) for net in _nets()]
        assert on['plan']['expand'] == want
        assert on['counts'] == off['counts'] and sum(on['counts'].values()) > 0, (on['counts'], off['counts'])
        assert on['counts']['k_row_dedup + k_row_expand'] == 2
        net = _nets()[0]
        again = [net.snapshot(DIEN_ALL_FEATURE, 0)[:R], net.snapshot(DIEN_SCORES, 0)[:, :R], net.snapshot(DIEN_QUERY, 0)[:R]]
        for x, y in zip(on['out'][3:], again):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_a_pending_expansion_is_dropped_by_the_next_forward():
    """Forward A, then forward B on other rows with another partition and no snapshot in between: the snapshot behind B shows B's
    rows on every row - A's pending expansion never ran, B's did."""
    plain = _nets(16, ('no_row_dedup',))[0]
    for R, group, caller_obs in ((65, 1, True), (72, 9, False)):
        a = _inputs('identical', R // group, group, False, seed=1)
        b = _inputs('aba', R // group, group, True, seed=2)
        res = []
        for net in _nets() + [plain]:
            _forward(net, R, group, a, caller_obs=caller_obs, snapshots=False)
            res.append(_forward(net, R, group, b, caller_obs=caller_obs))
        assert res[0]['plan']['expand'] == 'lazy:768'
        _same(res[0]['out'], res[1]['out'], (R, group, 'no_lazy_expand'))
        _same(res[0]['out'], res[2]['out'], (R, group, 'no_row_dedup'))


@pytest.mark.parametrize('kernels', ['dup_store', 'no_tier2_rows'])
def test_other_forms_keep_their_launches(kernels):
    """'dup_store' and 'no_tier2_rows' never take the lazy form: the same plan, results and profile counts with and without
    'no_lazy_expand' beside them."""
    arms = (kernels, kernels + ',no_lazy_expand')
    for R, group, caller_obs in ((65, 1, True), (72, 9, False)):
        inputs = _inputs('aba', R // group, group, True)
        a, b = [_forward(net, R, group, inputs, caller_obs=caller_obs, count=True) for net in _nets(16, arms)]
        assert a['plan'] == b['plan'] and not a['plan']['expand'].startswith('lazy')
        _same(a['out'], b['out'], (kernels, R, group))
        assert a['counts'] == b['counts'] and sum(a['counts'].values()) > 0
        _same(a['out'], _forward(_nets()[0], R, group, inputs, caller_obs=caller_obs)['out'], (kernels, 'default'))


def _episode(tmp_path, kind, kernels):
    """reset and 9 steps of offline_action replay at B = 64 on device tensors (Slate: one episode; SeqSlate: one page), 20 log lines
    and cache_size = 16 -> (every observation, reward and done flag as arrays, launch counts per profile class)"""
    import torch
    import rl4rs_amd
    from rl4rs_amd import synth
    from rl4rs_amd.env.slate import SlateRecEnv, SlateState
    from rl4rs_amd.env.seqslate import SeqSlateRecEnv, SeqSlateState
    d = str(tmp_path)
    os.makedirs(d, exist_ok=True)
    seq = kind == 'seq'
    text = synth.make_catalog_text(seed=4)
    synth.write_text(os.path.join(d, 'c.csv'), text)
    recs = synth.make_records(20, pages=2 if seq else 1, seed=3, hash_size=2000, special_ids=synth.special_ids_from_text(text))
    synth.write_records(os.path.join(d, 'log.csv'), recs)
    cfg = {"maxlen": 64, "batch_size": 64, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
           "category_feature_num": 21, "category_hash_size": 2000, "seq_num": 2, "emb_size": 128, "page_items": 9,
           "hidden_units": 128, "max_steps": 18 if seq else 9, "action_emb_size": 32, "sample_file": os.path.join(d, 'log.csv'),
           "iteminfo_file": os.path.join(d, 'c.csv'), "cache_size": 16, "model_seed": 3, "scorer_kernels": kernels, "return_tensors": True}
    np.random.seed(7)
    if seq:
        env = rl4rs_amd.make('SeqSlateRecEnv-v0', recsim=SeqSlateRecEnv(cfg, state_cls=SeqSlateState))
    else:
        env = rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))
    env.seed(11)
    net = env.sim.model.device_net
    net.set_profiling(1)
    net.profile_reset()

    def arr(x, dtype):
        x = x['obs'] if isinstance(x, dict) else x
        return (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).astype(dtype)
    out = [arr(env.reset(), np.float32)]
    for t in range(9):
        obs, reward, done, info = env.step(env.offline_action)
        out += [arr(obs, np.float32), arr(reward, np.float64), arr(done, np.uint8)]
    torch.cuda.synchronize()
    counts = dict((k, v[1]) for k, v in net.profile().items())
    net.set_profiling(0)
    return out, counts


@pytest.mark.parametrize('kind', ['slate', 'seq'])
def test_episode_is_bit_identical(tmp_path, kind):
    on, c_on = _episode(tmp_path / 'a', kind, '')
    off, c_off = _episode(tmp_path / 'b', kind, 'no_lazy_expand')
    assert len(on) == len(off) == 28
    for t, (x, y) in enumerate(zip(on, off)):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), t
    assert c_on == c_off and sum(c_on.values()) > 0, (c_on, c_off)


def test_host_mirror_record_form_keeps_its_launches(tmp_path):
    """The reference-shaped record form with the head GEMM's host mirror armed: identical observations and rewards, equal counts."""
    on, n_on, c_on = t2._episode(tmp_path / 'a', '', False, host_mirror=True)
    off, n_off, c_off = t2._episode(tmp_path / 'b', 'no_lazy_expand', False, host_mirror=True)
    assert len(on) == len(off) == 19
    for t, (x, y) in enumerate(zip(on, off)):
        assert t2._equal_bits(x, y), t
    assert n_on == n_off and 1 <= n_on < 64
    assert c_on == c_off and sum(c_on.values()) > 0, (c_on, c_off)
