"""Shadow-plane order of an observation-sized forward: k_din_xq forms q and qa = q W1ac for its own rows, the category
branch and the dense tower run as a shadow plane of the 32-row AUGRU launch (k_augru_xs) - five launches where there were seven.
Everything is pinned BIT FOR BIT against the same weights and histories on a handle with scorer_kernels='no_augru_shadow' (the
launches of before): obs, prob, ALL_FEATURE (AUGRU states, dense tower, pooled category row), SCORES, QUERY of every row,
duplicates included.  rl4rs_dien_kernel_label of the recurrence class says which order the last forward took, so every case is
known to have run the order it is about."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CFG = {"maxlen": 64, "batch_size": 8, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
       "category_feature_num": 21, "category_hash_size": 3000, "seq_num": 2, "emb_size": 128,
       "page_items": 9, "hidden_units": 128, "max_steps": 9, "action_emb_size": 32, "scorer_precision": "fp16x2"}
NSLOTS = 16
ARMS = ('', 'no_augru_shadow')
RMAX = 257


@functools.lru_cache(maxsize=None)
def _weights(L):
    from rl4rs_amd.nets.dien import init_dien_weights
    return init_dien_weights(dict(CFG, maxlen=L), seed=9, emb_scale=0.5, bias_noise=0.2)


@functools.lru_cache(maxsize=None)
def _histories(L):
    rs = np.random.RandomState(77)
    seq = rs.randint(1, 284, size=(NSLOTS, 2, L)).astype(np.int32)
    seq[: NSLOTS // 3, 0, :L // 2] = 0              # leading padding on a third of input 0
    seq[::2, 1, :] = 0                              # input 1: every second history all padding
    return seq


def _net(L, kernels, max_rows, weights=None):
    import torch
    from rl4rs_amd.device import DeviceDien
    net = DeviceDien(dict(CFG, maxlen=L, scorer_kernels=kernels), weights or _weights(L), max_rows=max_rows, max_slots=NSLOTS)
    for s in range(2):
        net.encode(s, torch.from_numpy(np.ascontiguousarray(_histories(L)[:, s])).cuda(), 0)
    return net


@functools.lru_cache(maxsize=None)
def _nets(L):
    """One handle per arm for every row count of the file (a forward may use fewer rows than the handle holds)."""
    return [_net(L, k, RMAX) for k in ARMS]


def _rows(runs, rs):
    """runs = strings of template letters ('ABA': three rows, the third equal to the first); run r reads slot r % NSLOTS of input 0
    and slot r % 2 of input 1 -> slots [2, n], dense [n, 432], cat [n, 21]"""
    s0, s1, dn, ct = [], [], [], []
    for r, letters in enumerate(runs):
        tpl = {}
        for ch in letters:
            if ch not in tpl:
                cat = rs.randint(0, CFG['category_hash_size'], size=21).astype(np.int32)
                cat[10:] = rs.randint(0, 284, size=11)
                tpl[ch] = (np.abs(rs.randn(432) * 3).astype(np.float32), cat)
            s0.append(r % NSLOTS)
            s1.append(r % 2)
            dn.append(tpl[ch][0])
            ct.append(tpl[ch][1])
    return np.array([s0, s1], dtype=np.int32), np.stack(dn), np.stack(ct)


def _pattern(name, R):
    if name == 'none':
        return ['A'] * R, R                         # R runs of one row: every row its own template
    if name == 'aba':
        runs = ['ABA'] * (R // 3) + (['A' * (R % 3)] if R % 3 else [])
        return runs, 2 * (R // 3) + (1 if R % 3 else 0)
    return ['A' * R], 1                             # every row equal: n_active = 1


def _augru_label(net):
    for k in range(net.lib.rl4rs_dien_kernel_count()):
        if net.lib.rl4rs_dien_kernel_name(k).decode() == 'augru':
            buf = C.create_string_buffer(160)
            assert net.lib.rl4rs_dien_kernel_label(net.h, k, buf, 160) == 0
            return buf.value.decode()
    raise AssertionError('no augru class')


def _forward(net, R, group, dense, cat, slots, order=None):
    """-> ([obs, prob, all_feature, scores, query], n_active, the last forward was shadowed)"""
    import torch
    from rl4rs_amd.device import DIEN_ALL_FEATURE, DIEN_SCORES, DIEN_QUERY, DIEN_N_ACTIVE
    sl = torch.from_numpy(np.ascontiguousarray(slots)).cuda()
    net.set_row_order(None if order is None else torch.from_numpy(np.asarray(order, dtype=np.int32)).cuda())
    obs, prob = net.forward(R, group, torch.from_numpy(dense).cuda(), torch.from_numpy(cat).cuda(), sl, True, True)
    out = [obs.clone(), prob.clone(), net.snapshot(DIEN_ALL_FEATURE, R)[:R].clone(), net.snapshot(DIEN_SCORES, R)[:, :R].clone(),
           net.snapshot(DIEN_QUERY, R)[:R].clone()]
    return out, int(net.snapshot(DIEN_N_ACTIVE, 0)[0].item()), 'k_augru_xs' in _augru_label(net)


def _same_bits(a, b, what):
    import torch
    for name, x, y in zip(('obs', 'prob', 'all_feature', 'scores', 'query'), a, b):
        assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)), (what, name)


@pytest.mark.parametrize('R', [1, 31, 32, 33, 65, 257])
@pytest.mark.parametrize('L', [64, 16])
def test_rows_patterns_and_orders(L, R):
    """group 1; no duplicates, A B A inside a run, every row equal (n_active = 1); natural order and a scattered batch with the
    row order that puts the runs back together.  R = 1 .. 257: a single row, a partial tile, a full one, a tile of one row behind a
    full one, three tiles, nine (the shadow workgroups of the tiles behind n_active leave)."""
    import torch
    on, off = _nets(L)
    for pat in ('none', 'aba', 'same'):
        runs, n_want = _pattern(pat, R)
        slots, dense, cat = _rows(runs, np.random.RandomState(R + len(pat)))
        assert dense.shape[0] == R
        for ordered in (False, True):
            s, d, c, order = slots, dense, cat, None
            if ordered:
                perm = np.random.RandomState(5).permutation(R)
                s, d, c, order = np.ascontiguousarray(slots[:, perm]), dense[perm], cat[perm], np.argsort(perm).astype(np.int32)
            a, na, sh_a = _forward(on, R, 1, d, c, s, order)
            b, nb, sh_b = _forward(off, R, 1, d, c, s, order)
            print('L', L, 'R', R, pat, 'ordered' if ordered else 'natural', 'n_active', na, 'of', R, 'shadow', sh_a, sh_b)
            assert sh_a and not sh_b
            assert na == nb == n_want
            assert all(torch.isfinite(x).all() for x in a)
            _same_bits(a, b, (L, R, pat, ordered))
    on.check_status()


def test_room_rule_and_groups_of_nine():
    """ceil(G / 32) * (S + 1) workgroups must fit the chip's CUs, G = the distinct-groups hint (default: the forward's rows): one
    tile too many and the forward takes the old launches; with a hint that fits - here a STALE one, the batch has no duplicates,
    so live workgroups outnumber it and shadow workgroups wait for a CU - it takes the shadow order; bit-identical either way.
    A forward in groups of 9 (the reward forward's shape) never takes it."""
    import torch
    L = 16
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = n_cu // 3
    R = 32 * (tiles + 1)
    rs = np.random.RandomState(4)
    slots, dense, cat = _rows(['A'] * R, rs)
    on, off = _net(L, '', R), _net(L, 'no_augru_shadow', R)
    try:
        a, na, sh = _forward(on, R, 1, dense, cat, slots)
        assert na == R and not sh                            # (tiles + 1) * 3 > n_cu
        on.set_distinct_hint(32 * tiles)
        b, nb, sh = _forward(on, R, 1, dense, cat, slots)
        assert nb == R and sh
        c, nc, sh_off = _forward(off, R, 1, dense, cat, slots)
        assert not sh_off
        _same_bits(a, c, 'no room')
        _same_bits(b, c, 'stale hint')
        on.set_distinct_hint(0)
        # groups of 9: 15 groups, the third equal to the first in every run of three
        g = 9
        s9, d9, c9 = _rows(['ABA'] * 5, rs)
        d9 = np.repeat(d9, g, axis=0)
        c9 = np.repeat(c9, g, axis=0)
        c9[:, 20] = rs.randint(0, 284, size=c9.shape[0])
        for i in range(5):                                   # the duplicate group: the same last ids as its original
            c9[(3 * i + 2) * g:(3 * i + 3) * g, 20] = c9[(3 * i) * g:(3 * i + 1) * g, 20]
        x, nx, sh_x = _forward(on, 15 * g, g, d9, c9, s9)
        y, ny, sh_y = _forward(off, 15 * g, g, d9, c9, s9)
        assert nx == ny == 10 and not sh_x and not sh_y
        _same_bits(x, y, 'group 9')
        on.check_status()
    finally:
        on.close()
        off.close()


def test_fp16_range_still_poisons_the_rows():
    """The construction of tests/test_gpu_dien.py::test_fp16_range_poisons_the_rows_on_the_device on the shadow order: sequence
    input 0 explodes for every row - the whole observation row and the click probability are NaN on the device, the status
    bit is raised, and the bits (NaN payloads included) are those of the old launches."""
    import torch
    L, R = 64, 40
    w = dict(_weights(L))
    w['att0_b3'] = np.array([-40.0], dtype=np.float32)
    rs = np.random.RandomState(2)
    slots, dense, cat = _rows(['A'] * R, rs)
    res = []
    for k in ARMS:
        net = _net(L, k, R, weights=w)
        try:
            out, _, sh = _forward(net, R, 1, dense, cat, slots)
            assert sh == (k == '')
            assert torch.isnan(out[0]).all(dim=1).all() and torch.isnan(out[1]).all()
            from rl4rs_amd.device import _stream
            f = C.c_int32()
            assert net.lib.rl4rs_dien_status(net.h, C.byref(f), _stream()) == 0 and (f.value & 1)
            res.append(out)
        finally:
            net.close()
    _same_bits(res[0], res[1], 'poison')


def _episode(tmp_path, kernels):
    """One SlateRecEnv episode of offline_action replay through the facade, B = 64, T = 9, 20 log lines and cache_size = 16
    -> (observations of every step and rewards as float32 arrays, the reset's forward was shadowed)"""
    import torch
    import rl4rs_amd
    from rl4rs_amd import synth
    from rl4rs_amd.env.slate import SlateRecEnv, SlateState
    d = str(tmp_path)
    os.makedirs(d, exist_ok=True)
    B, T = 64, 9
    text = synth.make_catalog_text(seed=4)
    synth.write_text(os.path.join(d, 'c.csv'), text)
    recs = synth.make_records(20, pages=1, seed=3, hash_size=2000, special_ids=synth.special_ids_from_text(text))
    synth.write_records(os.path.join(d, 'log.csv'), recs)
    cfg = {"maxlen": 64, "batch_size": B, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
           "category_feature_num": 21, "category_hash_size": 2000, "seq_num": 2, "emb_size": 128, "page_items": 9,
           "hidden_units": 128, "max_steps": T, "action_emb_size": 32, "sample_file": os.path.join(d, 'log.csv'),
           "iteminfo_file": os.path.join(d, 'c.csv'), "cache_size": 16, "model_seed": 3, "scorer_kernels": kernels,
           "return_tensors": True}
    env = rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))
    env.seed(11)

    def arr(x):
        x = x['obs'] if isinstance(x, dict) else x
        return (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).astype(np.float32)
    out = [arr(env.reset())]
    shadowed = 'k_augru_xs' in _augru_label(env.sim.model.device_net)
    for t in range(T):
        obs, reward, done, info = env.step(env.offline_action)
        out.append(arr(obs))
        out.append(arr(reward))
    torch.cuda.synchronize()
    return out, shadowed


def test_episode_replay_is_bit_identical(tmp_path):
    on, sh_on = _episode(tmp_path / 'a', '')
    off, sh_off = _episode(tmp_path / 'b', 'no_augru_shadow')
    assert sh_on and not sh_off
    assert len(on) == len(off) == 19
    assert float(sum(np.abs(x).sum() for x in on[2::2])) > 0          # some reward was paid
    for t, (x, y) in enumerate(zip(on, off)):
        assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), t
