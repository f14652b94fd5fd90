"""Replay-ahead (step.hip, step_lanes.hpp): once a replay loop hands back the stepper's own logged-action row, the
observation rows of the remaining transitions of the episode are scored in ONE forward of 8 / 9 rows per env, and every later
transition runs its act alone and is handed its row.  Everything a caller can see must be what it saw without it, bit for bit: every
case runs the same calls on an env built with config['no_step_overlap'] and on one with config['no_replay_ahead'] alone, from the same
seed, and compares every observation, reward, last action and the click probabilities.  rl4rs_stepper_replay_stats says whether the
forward DID start and how many rows were handed out and dropped: the counts are worked out by hand from the rule.

Shapes (scorer_kernels = 'augru_rows64' pins the 64-row AUGRU form, config['replay_ahead'] = 'pinned' lets the stepper start under the
pin): B = 8 (R = 64: one tile), B = 64 from 24 cached lines (duplicate envs, a partial tile of active groups), B = 72 (nine tiles);
T = 9 (groups of 8) and T = 10 (groups of 9)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(8, 8), (64, 24), (72, 72)]          # (B, cache_size)
SCENARIOS = ['full', 'foreign3', 'reset', 'mask', 'two']


def _make(tmp_path, B, cache, T, arm, pin=True, **extra):
    import rl4rs_amd
    from rl4rs_amd import synth
    from rl4rs_amd.env.slate import SlateRecEnv, SlateState
    d = str(tmp_path / arm)
    os.makedirs(d, exist_ok=True)
    text = synth.make_catalog_text(seed=4)
    synth.write_text(os.path.join(d, 'c.csv'), text)
    # (T = 10: a log of two pages, so that every step has its logged action)
    recs = synth.make_records(160, pages=2 if T > 9 else 1, seed=3, hash_size=2000, special_ids=synth.special_ids_from_text(text))
    synth.write_records(os.path.join(d, 'log.csv'), recs)
    cfg = {"maxlen": 64, "batch_size": B, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
           "category_feature_num": 21, "category_hash_size": 2000, "seq_num": 2, "emb_size": 128, "page_items": 9,
           "hidden_units": 128, "max_steps": T, "action_emb_size": 32, "sample_file": os.path.join(d, 'log.csv'),
           "iteminfo_file": os.path.join(d, 'c.csv'), "cache_size": cache, "model_seed": 3, "return_tensors": True,
           "scorer_kernels": 'augru_rows64' if pin else '', "scorer_precision": "fp16x2"}
    cfg.update(extra)
    env = rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))
    env.seed(11)
    return env


def _episode(env, T, out, foreign=None, stop=None, mask_at=None, policy=False):
    import torch
    obs = env.reset()
    out['obs'].append(obs.clone())
    for t in range(T):
        if policy:
            legal = env.samples._obs_mask().to(torch.bool)
            proj = torch.randn((256, 284), dtype=torch.float64, generator=torch.Generator().manual_seed(5)).cuda()
            a = (obs.to(torch.float64) @ proj).masked_fill(~legal, -float('inf')).argmax(dim=1).to(torch.int32)
        else:
            a = env.offline_action
            if t == foreign:
                a = torch.as_tensor(a).clone()
        obs, reward, done, info = env.step(a)
        out['obs'].append(obs.clone())
        out['reward'].append(torch.as_tensor(reward).clone())
        out['last'].append(torch.as_tensor(env.samples.last_actions).clone())
        if t == mask_at:
            out['mask'].append(env.samples._obs_mask().clone())
        if t == stop:
            return
    out['click'].append(env.sim._stepper.click_probs().clone())


def _run(env, T, scenario):
    """-> (everything the caller saw, the stepper's replay stats over the scenario)"""
    import torch
    out = {'obs': [], 'reward': [], 'last': [], 'click': [], 'mask': []}
    _episode(env, T, out)                       # (the stepper exists from here on; not counted)
    s0 = env.sim._stepper.replay_stats()
    if scenario == 'full':
        _episode(env, T, out)
    elif scenario == 'foreign3':
        _episode(env, T, out, foreign=3)
    elif scenario == 'reset':
        _episode(env, T, out, stop=3)
        _episode(env, T, out)
    elif scenario == 'mask':
        _episode(env, T, out, mask_at=1)
    elif scenario == 'two':
        _episode(env, T, out)
        _episode(env, T, out)
    elif scenario == 'policy':
        _episode(env, T, out, policy=True)
    torch.cuda.synchronize()
    return out, tuple(a - b for a, b in zip(env.sim._stepper.replay_stats(), s0))


def _want(T, scenario, c0=0):
    """(forwards started, rows per env handed out, rows per env dropped): the forward starts at act c0 with n = T - 1 - c0 rows per env"""
    n = T - 1 - c0
    return {'full': (1, n, 0),
            'foreign3': (1, 3 - c0, n - 3 + c0),        # acts c0 .. 2 handed out; the clone at act 3 drops the rest, no later start (n < 8)
            'reset': (2, 4 - c0 + n, n - 4 + c0),       # acts c0 .. 3, then env.reset()
            'mask': (1, 2 - c0, n - 2 + c0),            # the mask read behind act 1 joins
            'two': (2, 2 * n, 0)}[scenario]


def _same(a, b, what):
    import torch
    for key in a:
        assert len(a[key]) == len(b[key]), (what, key)
        bad = [i for i, (x, y) in enumerate(zip(a[key], b[key])) if not torch.equal(x, y)]
        assert not bad, (what, key, bad)


@pytest.mark.parametrize('T', [9, 10])
@pytest.mark.parametrize('B,cache', SHAPES)
def test_bit_identical_to_the_serial_order_and_to_the_switch_off(tmp_path, B, cache, T):
    import torch
    arms = {'ahead': {'replay_ahead': 'pinned'}, 'serial': {'no_step_overlap': True, 'no_replay_ahead': True},
            'off': {'no_replay_ahead': True, 'replay_ahead': 'pinned'}}
    if T == 10:
        # without the lanes the reset's forward leaves no logged-action row: the stepper's own row first comes back at act 1, and
        # with T = 10 that still leaves 8 rows per env - the forward and the acts behind it on the caller's stream
        arms['home'] = {'no_step_overlap': True, 'replay_ahead': 'pinned'}
    runs = {}
    for arm, kw in arms.items():        # one env at a time: the arms draw their batches from the same seeded sequence
        env = _make(tmp_path, B, cache, T, arm, **kw)
        runs[arm] = [_run(env, T, scenario) for scenario in SCENARIOS]
        del env
        torch.cuda.synchronize()
    for i, scenario in enumerate(SCENARIOS):
        res = {arm: r[i] for arm, r in runs.items()}
        _same(res['ahead'][0], res['serial'][0], (scenario, 'serial'))
        _same(res['ahead'][0], res['off'][0], (scenario, 'off'))
        assert res['ahead'][1] == _want(T, scenario), (scenario, res['ahead'][1])
        if 'home' in res:
            _same(res['home'][0], res['serial'][0], (scenario, 'home'))
            assert res['home'][1] == _want(T, scenario, c0=1), (scenario, res['home'][1])
        assert res['serial'][1] == (0, 0, 0) and res['off'][1] == (0, 0, 0), (scenario, res['serial'][1], res['off'][1])


@pytest.mark.parametrize('B,cache,T,pin,kw,scenario', [
    (12, 12, 9, True, {'replay_ahead': 'pinned'}, 'full'),        # R = 96 is no multiple of 64: the 32-row form
    (64, 24, 5, True, {'replay_ahead': 'pinned'}, 'full'),        # four rows per env
    (64, 24, 9, False, {'replay_ahead': 'pinned'}, 'full'),       # no pin: 16 workgroups do not fill the chip twice over
    (64, 24, 9, True, {}, 'full'),                                 # the default asks for the automatic rule, not for the pin
    (64, 24, 9, True, {'replay_ahead': 'pinned'}, 'policy'),      # the action is computed from the observation
])
def test_does_not_start(tmp_path, B, cache, T, pin, kw, scenario):
    env = _make(tmp_path, B, cache, T, 'x', pin=pin, **kw)
    _, stats = _run(env, T, scenario)
    assert stats == (0, 0, 0), stats


def _twin_records(n_pairs, T):
    """Log lines in pairs (2 i, 2 i + 1) of one user: the same portrait and history, a logged slate that agrees up to step k = 1 + i % 7
    and differs from there on (pair 0 of every eight: from step T - 1 on, which no observation row shows)"""
    from rl4rs_amd import synth
    text = synth.make_catalog_text(seed=4)
    base = synth.make_records(n_pairs, pages=2 if T > 9 else 1, seed=21, hash_size=2000, special_ids=synth.special_ids_from_text(text))
    out = []
    for i, rec in enumerate(base):
        f = rec.split('@')
        k = T - 1 if i % 8 == 0 else 1 + i % 7
        slate = [int(x) for x in f[3].split(',')]
        twin = list(f)
        twin[0], twin[1] = str(int(f[0]) + 100000), str(int(f[1]) + 100000)
        twin[3] = ','.join(str(x if j < k else x % 283 + 1) for j, x in enumerate(slate))
        out += [rec, '@'.join(twin)]
    return text, out


def _twin_slots(rows, n):
    """the history slot of a line is its pair's: equal histories share a cache slot (what a caller's own slot table may do; the
    facade gives every line a slot of its own, and two lines then never share a representative)"""
    rows = np.asarray(rows)
    return np.unique(rows - rows % 2, return_inverse=True)


@pytest.mark.parametrize('T', [9, 10])
def test_envs_whose_logged_actions_part_later_split_off(tmp_path, monkeypatch, T):
    """Two log lines with equal user columns and history (one cache slot) and equal logged actions up to act 0 share a representative
    when the group forward starts; their slates part at a later step.  The row builder must make the second line's envs stand for
    themselves in the forward's copy of the partition - with the act's partition as it is they would be handed the first line's
    observations.  Bit for bit against the arms without replay-ahead (whose acts split them step by step), and the forward's
    partition has more representatives than the act's."""
    import torch
    import rl4rs_amd
    from rl4rs_amd import synth, device as D
    from rl4rs_amd.env import slate
    from rl4rs_amd.env.slate import SlateRecEnv, SlateState
    monkeypatch.setattr(slate, '_unique_lines', _twin_slots)
    B, pairs = 64, 8
    text, recs = _twin_records(pairs, T)
    runs, n_active = {}, {}
    for arm, kw in (('ahead', {'replay_ahead': 'pinned'}), ('off', {'no_replay_ahead': True}),
                    ('serial', {'no_step_overlap': True, 'no_replay_ahead': True})):
        d = str(tmp_path / arm)
        os.makedirs(d, exist_ok=True)
        synth.write_text(os.path.join(d, 'c.csv'), text)
        synth.write_records(os.path.join(d, 'log.csv'), recs)
        cfg = {"maxlen": 64, "batch_size": B, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
               "category_feature_num": 21, "category_hash_size": 2000, "seq_num": 2, "emb_size": 128, "page_items": 9,
               "hidden_units": 128, "max_steps": T, "action_emb_size": 32, "sample_file": os.path.join(d, 'log.csv'),
               "iteminfo_file": os.path.join(d, 'c.csv'), "cache_size": 2 * pairs, "model_seed": 3, "return_tensors": True,
               "scorer_kernels": 'augru_rows64', "scorer_precision": "fp16x2"}
        cfg.update(kw)
        env = rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))
        env.seed(11)
        runs[arm] = _run(env, T, 'two')
        # the partition of the forward behind act 0: the group forward's copy (ahead) / the act's own (off, serial)
        env.reset()
        env.step(env.offline_action)
        n_active[arm] = int(env.sim.model.device_net.snapshot(D.DIEN_N_ACTIVE, B)[0])
        lines = np.asarray(env.samples._store_rows[1])
        del env
        torch.cuda.synchronize()
    _same(runs['ahead'][0], runs['off'][0], 'off')
    _same(runs['ahead'][0], runs['serial'][0], 'serial')
    assert runs['ahead'][1] == (2, 2 * (T - 1), 0), runs['ahead'][1]
    # behind act 0 a pair is one class (k >= 1): the act leaves as many representatives as pairs in the batch
    pairs_in = len(set((lines // 2).tolist()))
    assert n_active['off'] == n_active['serial'] == pairs_in, (n_active, pairs_in)
    # the forward's copy: every env whose line is not its representative's and parts from it inside the rows scored (pairs 0 mod 8 do
    # not) stands for itself.  The representative of a class is its first env in processing order: count both ways round
    assert n_active['ahead'] > n_active['off'], n_active
    first = {}
    order = np.argsort(lines // 2, kind='stable')
    for b in order:
        first.setdefault(lines[b] // 2, lines[b])
    want = pairs_in + sum(1 for b in range(B) if lines[b] != first[lines[b] // 2] and (lines[b] // 2) % 8 != 0)
    assert n_active['ahead'] == want, (n_active, want)
