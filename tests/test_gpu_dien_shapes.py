"""The DIEN scorer forward off the default configuration (tests/dien_shape_cases.py: eight models from the family rl4rs_dien_create
admits, each at the forward shapes f1 / f8 / f9, with duplicate row groups and front-padded histories), in fp16x2 and in fp32:

* EVERY row of every forward against the fp64 oracle at the standing bars of tests/test_gpu_dien.py - the all-feature row split at
  the case's own offsets (S AUGRU states | U dense columns | E pooled category columns), the attention scores per input, the
  query, obs, prob, obs_last at f9, the first-GRU cache of input 0 in case A;
* after each forward DeviceDien.last_plan() is the plan tests/test_dien_shapes_host.py computed for that case from
  rl4rs_amd/csrc/dien_plan.hpp, and N_ACTIVE / ROW_REP are the numpy duplicate rule's: the test ran the form it is about, with
  the duplicates it is about;
* the handles '' / 'no_tier2_rows' / 'no_row_dedup' are bit-identical in all of it, the 32- and the 64-row AUGRU form at f8 / f9
  too; 'no_gemm_group' in case A (the pair's two-launch fallback against the plain two launches); 'dense_fork' in D and G; a
  carried partition; a `dense` pointer 4 bytes off 16-byte alignment (case G, f8).

Found by case A: the profile label of the dense stage named k_gemm_h16_pair on every handle whose plan says dense=pair, also
where launch_gemm_h16_pair cannot issue one grid (q-side term wider than 128 columns: S >= 3; dense rows of Dn % 4 != 0) and runs
its two launches.  The results were right; the label now follows DienTraits::pair_one_grid."""
import functools

import numpy as np
import pytest

import dien_shape_cases as T

pytestmark = pytest.mark.gpu

ARMS = ('', 'no_tier2_rows', 'no_row_dedup')
NAMES = ('obs', 'prob', 'all_feature', 'scores', 'query', 'obs_last')
_open = []


@pytest.fixture(scope='module', autouse=True)
def _close_handles():
    yield
    _net.cache_clear()
    while _open:
        _open.pop().close()


@functools.lru_cache(maxsize=None)
def _net(case, arm, precision='fp16x2'):
    """one handle per (case, option), its histories encoded, kept for the three forward shapes"""
    import torch
    from rl4rs_amd.device import DeviceDien
    net = DeviceDien(T.config(case, scorer_precision=precision, scorer_kernels=arm), T.weights(case), max_rows=128, max_slots=T.NSLOTS)
    assert net.scorer_mode == precision
    hist = T.histories(case)
    for s in range(hist.shape[1]):
        net.encode(s, torch.from_numpy(np.ascontiguousarray(hist[:, s])).cuda(), 0)
    _open.append(net)
    return net


def _forward(net, case, shape, pin=0, dense_dev=None, partition=None):
    """-> dict: out (device tensors obs, prob, all_feature, scores, query, obs_last), plan, n_active, rep"""
    import torch
    from rl4rs_amd.device import DIEN_ALL_FEATURE, DIEN_SCORES, DIEN_QUERY, DIEN_N_ACTIVE, DIEN_ROW_REP
    x = T.inputs(case, shape)
    R, group = x['R'], x['group']
    ng = R // group
    sl = torch.from_numpy(x['slots']).cuda()
    d = torch.from_numpy(x['dense']).cuda() if dense_dev is None else dense_dev
    c = torch.from_numpy(x['cat']).cuda()
    net.set_augru_rows(pin)
    net.set_distinct_hint(x['n_active'] if (case == 'F' and shape == 'f1') else 0)      # case F: the shadow plane's room rule
    if partition is not None:
        net.set_row_partition(*partition)
    last = shape == 'f9'
    res = net.forward(R, group, d, c, sl, True, True, want_obs_last=last)
    r = dict(plan=net.last_plan(), n_active=None, rep=None)
    r['out'] = [res[0].clone(), res[1].clone(), net.snapshot(DIEN_ALL_FEATURE, R)[:R].clone(), net.snapshot(DIEN_SCORES, R)[:, :R].clone(),
                net.snapshot(DIEN_QUERY, R)[:R].clone(), res[2].clone() if last else None]
    if r['plan']['dedup'] != 'none':
        r['n_active'] = int(net.snapshot(DIEN_N_ACTIVE, 0)[0].item())
        r['rep'] = net.snapshot(DIEN_ROW_REP, 0)[:ng].cpu().numpy()
    net.check_status()
    return r


def _same(a, b, what):
    import torch
    for name, x, y in zip(NAMES, a['out'], b['out']):
        if x is None:
            assert y is None, (what, name)
            continue
        assert torch.isfinite(x).all(), (what, name)
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (what, name, (x - y).abs().max().item())


def _against_oracle(r, case, shape, tag, h1=None):
    """every row of the forward against the fp64 oracle; prints each error beside its bar"""
    Fld = T.columns(case)[3]
    o = r['out']
    assert o[2].shape[1] == Fld, (o[2].shape, Fld)
    got = dict(obs=o[0].cpu().numpy(), prob=o[1].cpu().numpy(), all_feature=o[2].cpu().numpy(), scores=o[3].cpu().numpy(),
               query=o[4].cpu().numpy(), obs_last=None if o[5] is None else o[5].cpu().numpy(), h1_0=h1)
    errs = T.errors(got, T.reference(case, shape), case)
    print(T.report('%s %s %s' % (case, shape, tag), errs))
    assert not T.misses(errs), T.misses(errs)
    return errs


def _partition_is_the_rule(r, case, shape):
    x = T.inputs(case, shape)
    assert r['n_active'] == x['n_active'] and np.array_equal(r['rep'], x['rep']), (case, shape, r['n_active'], x['n_active'])


RUNS = (('f1', 0), ('f8', 32), ('f8', 64), ('f9', 32), ('f9', 64))


@pytest.mark.parametrize('case', sorted(T.CASES))
def test_every_row_against_the_oracle_and_the_arms_are_bit_identical(case):
    from rl4rs_amd.device import DIEN_H1
    extra = {'A': ('no_gemm_group',), 'D': ('dense_fork',), 'G': ('dense_fork',)}.get(case, ())
    by_shape = {}
    for shape, pin in RUNS:
        res = {}
        for arm in ARMS + extra:
            net = _net(case, arm)
            r = res[arm] = _forward(net, case, shape, pin)
            assert r['plan'] == T.plan_tokens(case, shape, arm, pin), (case, shape, arm, pin, r['plan'])
            if arm != 'no_row_dedup':
                _partition_is_the_rule(r, case, shape)
        on = res['']
        print(case, shape, 'pin', pin, 'n_active', on['n_active'], 'of', T.DUPLICATES[shape][0], '|', ' '.join('%s=%s' % kv for kv in on['plan'].items()))
        h1 = None
        if case == 'A' and shape == 'f1':              # the first-GRU cache of input 0, row by row through the row's slot
            x = T.inputs(case, shape)
            cache = _net(case, '').snapshot(DIEN_H1, 0).cpu().numpy()
            h1 = cache[np.repeat(x['slots'][0], x['group'])]
        _against_oracle(on, case, shape, 'fp16x2 pin %d' % pin, h1)
        for arm in (ARMS + extra)[1:]:
            _same(on, res[arm], (case, shape, pin, arm))
        if shape in by_shape:                           # the 64-row AUGRU form against the 32-row form
            _same(by_shape[shape], on, (case, shape, 'rows 32 / 64'))
        by_shape[shape] = on
    if case == 'A':
        # neither handle launches k_gemm_h16_pair: the default one takes launch_gemm_h16_pair's two-launch fallback (q-side term
        # 192 columns wide), 'no_gemm_group' the plain two launches - bit-identical above
        for arm in ('', 'no_gemm_group'):
            labels = sorted(_net(case, arm).profile())
            assert not any('k_gemm_h16_pair' in k for k in labels), (arm, labels)
    if case in ('B', 'G'):                              # ... while a handle that can pair them says so
        assert any('k_gemm_h16_pair' in k for k in _net(case, '').profile())


@pytest.mark.parametrize('case', sorted(T.CASES))
def test_carried_partition_is_bit_identical(case):
    """One f1 forward takes the rep / active / n_active the previous forward's k_row_dedup left (rl4rs_dien_set_row_partition):
    no k_row_dedup is launched, the same bits come back."""
    from rl4rs_amd.device import DIEN_N_ACTIVE, DIEN_ROW_REP, DIEN_ROW_ACTIVE
    net = _net(case, '')
    ng = T.DUPLICATES['f1'][0]
    first = _forward(net, case, 'f1')
    held = [net.snapshot(w, 0)[:n].clone() for w, n in ((DIEN_ROW_REP, ng), (DIEN_ROW_ACTIVE, ng), (DIEN_N_ACTIVE, 1))]
    net.profile_reset()
    second = _forward(net, case, 'f1', partition=held)
    assert net.dedup_counts() == (0, 1)
    assert second['plan'] == T.plan_tokens(case, 'f1', carried=True), second['plan']
    _partition_is_the_rule(second, case, 'f1')
    _same(first, second, (case, 'carried'))
    _against_oracle(second, case, 'f1', 'carried partition')
    third = _forward(net, case, 'f1')                    # one-shot: this one compares rows again
    assert net.dedup_counts() == (1, 1) and third['plan']['dedup'] == 'k_row_dedup'
    _same(first, third, (case, 'after the carry'))


def test_unaligned_dense_pointer_is_bit_identical():
    """Case G at f8 with `dense` starting 4 bytes into a larger buffer: row_words_equal takes its scalar path at a width
    (8 * 436 words) whose aligned call takes the 16-byte path, the GEMMs load the dense rows without vector loads (and the pair
    becomes two launches).  Same partition, same bits."""
    import torch
    case, shape = 'G', 'f8'
    x = T.inputs(case, shape)
    for arm in ('', 'no_row_dedup'):
        net = _net(case, arm)
        aligned = _forward(net, case, shape, 32)
        buf = torch.zeros(x['dense'].size + 8, dtype=torch.float32, device='cuda')
        assert buf.data_ptr() % 16 == 0
        view = buf[1:1 + x['dense'].size].view(x['dense'].shape)
        view.copy_(torch.from_numpy(x['dense']))
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        off = _forward(net, case, shape, 32, dense_dev=view)
        assert off['plan'] == aligned['plan']
        if arm == '':
            _partition_is_the_rule(off, case, shape)
        _same(aligned, off, (arm, 'dense + 4 bytes'))
        _against_oracle(off, case, shape, 'dense + 4 bytes %s' % (arm or 'default'))


@pytest.mark.parametrize('case', sorted(T.CASES))
def test_fp32_forms_against_the_oracle(case):
    """The exact-fp32 handle (k_recur<256,augru>, k_gemm_pk, tsum + packed head) at f1 and f8, the same bars."""
    net = _net(case, '', 'fp32')
    for shape in ('f1', 'f8'):
        r = _forward(net, case, shape)
        assert r['plan'] == T.plan_tokens(case, shape, fp32=True), r['plan']
        _against_oracle(r, case, shape, 'fp32')


@pytest.mark.parametrize('case', ['A', 'E'])
def test_probabilities_from_the_representatives_head_rows(case):
    """K = 3 and K = 8 through k_head_prob_rep: a reward-shaped forward that hands out no observation keeps the head output of the
    representatives only (expand=lazy at group 8 / 9) - prob and obs_last are the bits of the forward that hands it out."""
    import torch
    net = _net(case, '')
    for shape in ('f8', 'f9'):
        x = T.inputs(case, shape)
        full = _forward(net, case, shape, 32)
        sl, d, c = torch.from_numpy(x['slots']).cuda(), torch.from_numpy(x['dense']).cuda(), torch.from_numpy(x['cat']).cuda()
        res = net.forward(x['R'], x['group'], d, c, sl, False, True, want_obs_last=shape == 'f9')
        want = dict(T.plan_tokens(case, shape, pin=32), expand='lazy:%d' % T.columns(case)[3])
        assert net.last_plan() == want, net.last_plan()
        assert torch.equal(res[1].view(torch.int32), full['out'][1].view(torch.int32))
        if shape == 'f9':
            assert torch.equal(res[2].view(torch.int32), full['out'][5].view(torch.int32))
        err = np.abs(res[1].cpu().numpy() - T.reference(case, shape)['prob']).max()
        print(case, shape, 'k_head_prob_rep: prob %.3g/%.3g' % (err, T.BARS['prob']))
        assert err < T.BARS['prob']
        net.check_status()
