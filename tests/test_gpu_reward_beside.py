"""The reward step beside the replay-ahead forward (step.hip, step_lanes.hpp): behind a group forward on lane 0 the folded
reward step runs on lane 1 and on the scorer's second scratch set, grown to B * n_complete rows, instead of behind that forward on lane
0.  Everything a caller can see must be what it saw without it, bit for bit: every case runs the same calls from one seed on three arms -
config['no_step_overlap'], config['no_reward_beside'] and the default - and compares every observation, reward, last action, the click
probabilities and, in one scenario, the scorer's internal rows read right behind a reward step (rl4rs_dien_buffer copies them out of
the second set, T rows per env).  rl4rs_stepper_reward_beside_stats says how many reward steps took lane 1: worked out by hand below.

Shapes as tests/test_gpu_replay_ahead.py, for the same reasons (scorer_kernels = 'augru_rows64' pins the 64-row AUGRU form,
config['replay_ahead'] = 'pinned' lets the group forward start under the pin): B = 8 (one tile), B = 64 from 24 cached lines (duplicate
envs, a partial tile of active groups), B = 72 (nine tiles).  T = 9: groups of 8, the reset's forward on lane 1 (set 1, which the reward
forward then reuses at nine times the rows).  T = 10: groups of 9, the reset's forward on lane 0; the reward step there is not ONE
forward (ten rows per env are no 64-row shape), so it joins on every arm and the count is zero."""
import os

import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(8, 8), (64, 24), (72, 72)]          # (B, cache_size)
SCENARIOS = ['three', 'foreign_last', 'foreign3', 'reset3', 'buffers']


def _make(tmp_path, B, cache, T, arm, **extra):
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
           "scorer_kernels": 'augru_rows64', "scorer_precision": "fp16x2", "replay_ahead": 'pinned'}
    cfg.update(extra)
    env = rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))
    env.seed(11)
    return env


def _episode(env, T, out, foreign=None, stop=None, buffers=False):
    import torch
    from rl4rs_amd import device as D
    obs = env.reset()
    out['obs'].append(obs.clone())
    for t in range(T):
        a = env.offline_action
        if t == foreign:
            a = torch.as_tensor(a).clone()
        obs, reward, done, info = env.step(a)
        out['obs'].append(obs.clone())
        out['reward'].append(torch.as_tensor(reward).clone())
        out['last'].append(torch.as_tensor(env.samples.last_actions).clone())
        if t == stop:
            return
    st = env.sim._stepper
    if buffers:
        # right behind the reward step: the rows of its forward (every row of every env: the duplicates' rows are completed on demand)
        R = env.samples._live().B * int(st.lib.rl4rs_stepper_reward_rows(st.h))
        net = env.sim.model.device_net
        out['allf'].append(net.snapshot(D.DIEN_ALL_FEATURE, R)[:R].clone())
        out['scores'].append(net.snapshot(D.DIEN_SCORES, R)[:, :R].clone())
        out['query'].append(net.snapshot(D.DIEN_QUERY, R)[:R].clone())
    out['click'].append(st.click_probs().clone())


def _run(env, T, scenario):
    """-> (everything the caller saw, reward steps on lane 1 over the scenario, bytes of the scorer's second scratch set)"""
    import torch
    out = {'obs': [], 'reward': [], 'last': [], 'click': [], 'allf': [], 'scores': [], 'query': []}
    _episode(env, T, out)                       # (the stepper exists from here on; not counted)
    st = env.sim._stepper
    n0 = st.reward_beside_stats()[0]
    if scenario == 'three':                     # back to back: the second set is reused by the reset's forward and the next reward forward
        for _ in range(3):
            _episode(env, T, out)
    elif scenario == 'foreign_last':            # a copy of the logged action at the reward step: the lane waits for the caller's stream
        _episode(env, T, out, foreign=T - 1)
    elif scenario == 'foreign3':                # the copy at act 3 drops the group forward: the reward step is where it was without it
        _episode(env, T, out, foreign=3)
    elif scenario == 'reset3':                  # a reset behind act 3, then a full episode
        _episode(env, T, out, stop=3)
        _episode(env, T, out)
    elif scenario == 'buffers':
        _episode(env, T, out, buffers=True)
    torch.cuda.synchronize()
    n1, nbytes = st.reward_beside_stats()
    return out, n1 - n0, nbytes


def _want(T, scenario):
    """Reward steps on lane 1: one per episode that reaches its reward step with the group forward still in flight on lane 0 - at T = 9;
    at T = 10 the reward step is two forwards and joins"""
    if T != 9:
        return 0
    return {'three': 3, 'foreign_last': 1, 'foreign3': 0, 'reset3': 1, 'buffers': 1}[scenario]


def _same(a, b, what):
    import torch
    for key in a:
        assert len(a[key]) == len(b[key]), (what, key)
        bad = [i for i, (x, y) in enumerate(zip(a[key], b[key])) if not torch.equal(x, y)]
        assert not bad, (what, key, bad)


@pytest.mark.parametrize('T', [9, 10])
@pytest.mark.parametrize('B,cache', SHAPES)
def test_bit_identical_on_three_arms_and_counted(tmp_path, B, cache, T):
    import torch
    arms = {'serial': {'no_step_overlap': True}, 'nobeside': {'no_reward_beside': True}, 'beside': {}}
    runs = {}
    for arm, kw in arms.items():        # one env at a time: the arms draw their batches from the same seeded sequence
        env = _make(tmp_path, B, cache, T, arm, **kw)
        runs[arm] = [_run(env, T, scenario) for scenario in SCENARIOS]
        del env
        torch.cuda.synchronize()
    for i, scenario in enumerate(SCENARIOS):
        res = {arm: r[i] for arm, r in runs.items()}
        _same(res['beside'][0], res['serial'][0], (scenario, 'serial'))
        _same(res['beside'][0], res['nobeside'][0], (scenario, 'nobeside'))
        assert res['beside'][1] == _want(T, scenario), (scenario, res['beside'][1])
        assert res['serial'][1] == 0 and res['nobeside'][1] == 0, (scenario, res['serial'][1], res['nobeside'][1])
    # the second scratch set (whole 64-row tiles and one to spare): B rows from the attach; grown to the reward forward's B * T rows
    # only on the arm that runs on it, only where that forward is ONE forward (T = 9) and only where it does not fit already (B = 8)
    pad = lambda rows: (rows + 63) // 64 * 64 + 64      # noqa: E731
    rows = pad(B * T) if T == 9 and pad(B) < B * T else pad(B)
    assert runs['nobeside'][-1][2] > 0
    assert runs['beside'][-1][2] * pad(B) == runs['nobeside'][-1][2] * rows, (runs['beside'][-1][2], runs['nobeside'][-1][2])
