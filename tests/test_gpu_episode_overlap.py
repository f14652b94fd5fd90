"""The two ends of an episode on the stepper's lanes (step.hip, step_lanes.hpp): the reset's observation forward runs as a
lane transition without an act (rl4rs_stepper_observe), so that the first step's forward starts beside it, and a reward step that
scores the state row inside the reward forward runs on lane 0 beside the last observation transition on lane 1.  Everything a
caller can see must be what the serial order gives, bit for bit: every case runs the same episodes on a second env built with
config['no_step_overlap'] from the same seed and compares every observation (the reset's included), reward and logged action,
env.samples.last_actions, the click probabilities of the reward step and the scorer's launch counts per class.

Shapes: B = 96 from 48 cached lines (duplicate envs), B = 33 with is_eval (a partial tile), SeqSlate B = 64 over two pages (T = 18).
Each runs with scorer_kernels = 'augru_rows64' (the pin: a batch this small then folds its reward step, which takes a lane) and
without it (the reward step joins).  rl4rs_stepper_lane_stats_ex says whether the reset forward and the reward step DID run on
lanes: a case in which nothing overlapped proves nothing."""
import os

import pytest

pytestmark = pytest.mark.gpu

SLATE = [(96, 48, False), (33, 33, True)]       # (B, cache_size, is_eval)
SHAPES = [('slate',) + s for s in SLATE] + [('seq', 64, 32, False)]


def _make(tmp_path, kind, B, cache, is_eval, pin, arm, **extra):
    import rl4rs_amd
    from rl4rs_amd import synth
    from rl4rs_amd.env.slate import SlateRecEnv, SlateState
    from rl4rs_amd.env.seqslate import SeqSlateRecEnv, SeqSlateState
    d = str(tmp_path / arm)
    os.makedirs(d, exist_ok=True)
    seq = kind == 'seq'
    T = 18 if seq else 9
    text = synth.make_catalog_text(seed=4)
    synth.write_text(os.path.join(d, 'c.csv'), text)
    recs = synth.make_records(160, pages=2 if seq else 1, seed=3, hash_size=2000, special_ids=synth.special_ids_from_text(text))
    synth.write_records(os.path.join(d, 'log.csv'), recs)
    cfg = {"maxlen": 64, "batch_size": B, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
           "category_feature_num": 21, "category_hash_size": 2000, "seq_num": 2, "emb_size": 128, "page_items": 9,
           "hidden_units": 128, "max_steps": T, "action_emb_size": 32, "sample_file": os.path.join(d, 'log.csv'),
           "iteminfo_file": os.path.join(d, 'c.csv'), "cache_size": cache, "model_seed": 3, "return_tensors": True,
           "scorer_kernels": 'augru_rows64' if pin else '', "scorer_precision": "fp16x2"}
    if is_eval:
        cfg['is_eval'] = True
    cfg.update(extra)
    if seq:
        env = rl4rs_amd.make('SeqSlateRecEnv-v0', recsim=SeqSlateRecEnv(cfg, state_cls=SeqSlateState))
    else:
        env = rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))
    env.seed(11)
    return env, T


def _policy(env, obs, proj):
    import torch
    legal = env.samples._obs_mask().to(torch.bool)
    score = (obs.to(torch.float64) @ proj).masked_fill(~legal, -float('inf'))
    return score.argmax(dim=1).to(torch.int32)


def _drive(env, T, B, mode, episodes):
    """-> dict of everything the caller saw.  mode: 'hold', 'immediate', 'foreign', 'policy', 'reset'"""
    import torch
    out = {'obs': [], 'reward': [], 'action': [], 'last': [], 'click': [], 'extra': []}
    net = None
    proj = torch.randn((256, 284), dtype=torch.float64, generator=torch.Generator().manual_seed(5)).cuda()
    # (the gym facade samples twice while it is built: those reset forwards are not this drive's)
    early = getattr(env.sim, '_stepper', None)
    ex0 = early.lane_stats_ex() if early is not None else (0, 0)
    for ep in range(episodes):
        held, clones = [], []
        obs = env.reset()
        if net is None:
            net = env.sim.model.device_net
            net.set_profiling(True)
            net.profile_reset()
        acc = obs.sum(dim=1) if mode == 'immediate' else None      # right behind the reset, nothing waited for
        tot = torch.zeros(B, dtype=torch.float64, device='cuda')
        if mode == 'hold':
            held.append(obs)
            clones.append(obs.clone())
        else:
            out['obs'].append(obs.clone())
        for t in range(T):
            if mode == 'policy':
                a = _policy(env, obs, proj)
            else:
                a = env.offline_action
                out['action'].append(torch.as_tensor(a).clone())
                if mode == 'foreign' and t in (0, T - 1):
                    a = a.clone()
            obs, reward, done, info = env.step(a)
            if mode == 'hold':
                held.append(obs)                          # the caller keeps every tensor until the episode ends
                clones.append(obs.clone())
                held.append(reward)
                clones.append(torch.as_tensor(reward).clone())
            elif mode == 'immediate':
                acc = acc + obs.sum(dim=1)
                tot = tot + reward
            if mode != 'hold':
                out['obs'].append(obs.clone())
            out['reward'].append(torch.as_tensor(reward).clone())
            out['last'].append(torch.as_tensor(env.samples.last_actions).clone())
            if mode == 'reset' and ep == 0 and t == 3:
                break                                     # env.reset() in mid-episode, two transitions in flight
        if mode == 'hold':
            assert all(torch.equal(torch.as_tensor(h), c) for h, c in zip(held, clones)), 'a held tensor changed after it was handed out'
            out['obs'] += clones
        if mode == 'immediate':
            out['extra'] += [acc.clone(), tot.clone()]
        if mode != 'reset':                               # ('reset': the next env.reset() comes right behind the reward step)
            out['click'].append(env.sim._stepper.click_probs().clone())      # right behind the reward step: a join
    torch.cuda.synchronize()
    out['profile'] = {k: v[1] for k, v in net.profile().items()}
    out['lanes'] = env.sim._stepper.lane_stats()
    assert early is None or early is env.sim._stepper
    out['ex'] = tuple(v - v0 for v, v0 in zip(env.sim._stepper.lane_stats_ex(), ex0))
    return out


def _both(tmp_path, kind, B, cache, is_eval, pin, mode, episodes=2, **extra):
    import torch
    res = {}
    for arm in ('on', 'off'):
        env, T = _make(tmp_path, kind, B, cache, is_eval, pin, arm, **(extra if arm == 'on' else {'no_step_overlap': True}))
        res[arm] = _drive(env, T, B, mode, episodes)
        del env
        torch.cuda.synchronize()
    on, off = res['on'], res['off']
    for key in ('obs', 'reward', 'action', 'last', 'click', 'extra'):
        assert len(on[key]) == len(off[key]), key
        bad = [i for i, (x, y) in enumerate(zip(on[key], off[key])) if not torch.equal(x, y)]
        assert not bad, (key, bad)
    assert on['profile'] == off['profile']
    assert off['lanes'][:2] == (0, 0) and off['ex'] == (0, 0)
    return on, off


@pytest.mark.parametrize('pin', [True, False])
@pytest.mark.parametrize('kind,B,cache,is_eval', SHAPES)
def test_three_episodes_holding_every_tensor(tmp_path, kind, B, cache, is_eval, pin):
    """Three episodes back to back, the caller holding every obs and reward until its episode ends.  Pinned: every reset forward and
    every reward step (two per SeqSlate episode) ran on a lane; without the pin the reward steps joined."""
    on, _ = _both(tmp_path, kind, B, cache, is_eval, pin, 'hold', episodes=3)
    rewards = 2 if kind == 'seq' else 1
    assert on['ex'] == (3, 3 * rewards if pin else 0), on['ex']
    assert sum(on['lanes'][:2]) == 3 * (15 if kind == 'seq' else 8), on['lanes']
    if kind == 'slate':
        assert on['lanes'][:2] == (12, 12), on['lanes']


@pytest.mark.parametrize('B,cache,is_eval', SLATE)
def test_immediate_use_on_the_callers_stream(tmp_path, B, cache, is_eval):
    """Reductions of obs (the reset's too) and reward enqueued on the caller's stream right behind every call, nothing waited for."""
    on, _ = _both(tmp_path, 'slate', B, cache, is_eval, True, 'immediate')
    assert on['ex'] == (2, 2) and on['lanes'][:2] == (8, 8), (on['ex'], on['lanes'])


@pytest.mark.parametrize('B,cache,is_eval', SLATE)
def test_foreign_action_at_the_first_and_the_last_step(tmp_path, B, cache, is_eval):
    """A clone of the logged action at step 0 (behind the reset's lane forward) and at the reward step: lane transitions that wait
    for the caller's stream."""
    on, _ = _both(tmp_path, 'slate', B, cache, is_eval, True, 'foreign')
    assert on['ex'] == (2, 2) and on['lanes'][:2] == (8, 8), (on['ex'], on['lanes'])


@pytest.mark.parametrize('B,cache,is_eval', SLATE)
def test_policy_loop(tmp_path, B, cache, is_eval):
    """The action is a function of the returned obs and of the env's mask (a join in front of every step): nothing runs ahead, the
    reward step finds nothing in flight and stays on the caller's stream; the reset forward still takes its lane."""
    on, _ = _both(tmp_path, 'slate', B, cache, is_eval, True, 'policy')
    assert on['ex'] == (2, 0), on['ex']


@pytest.mark.parametrize('B,cache,is_eval', SLATE)
def test_reset_in_mid_episode_and_right_behind_a_reward_step(tmp_path, B, cache, is_eval):
    """env.reset() at step 4 with transitions in flight, then a whole episode, then env.reset() right behind its reward step (in
    flight on lane 0) and another whole episode."""
    on, _ = _both(tmp_path, 'slate', B, cache, is_eval, True, 'reset', episodes=3)
    assert on['ex'] == (3, 2), on['ex']
    assert on['lanes'][:2] == (2 + 8, 2 + 8), on['lanes']


@pytest.mark.parametrize('switch,want', [('no_reset_lane', (0, 2)), ('no_reward_lane', (2, 0))])
def test_each_switch_off_alone(tmp_path, switch, want):
    on, _ = _both(tmp_path, 'slate', 96, 48, False, True, 'immediate', **{switch: True})
    assert on['ex'] == want and on['lanes'][:2] == (8, 8), (on['ex'], on['lanes'])
