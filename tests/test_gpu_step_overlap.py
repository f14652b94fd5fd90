"""Consecutive transitions on the stepper's two lanes (step.hip, step_lanes.hpp): with the overlap on, the forward of
transition k + 1 runs beside the forward of transition k on another stream, from a second set of state rows, partition arrays
and scorer scratch.  Everything a caller can see must be what the serial order gives, bit for bit: every case runs the same
episodes on a second env built with config['no_step_overlap'] from the same seed and compares every step's observation, reward and
logged action, env.samples.last_actions, the click probabilities of the reward step and the scorer's launch counts per class.

The observation-sized launch is bound by one workgroup's 64-step chain (about 0.45 ms whatever the batch), so even these batches
keep the forward of k in flight while the act and the DIN of k + 1 run: a missing second buffer or wait shows as wrong bits.
Shapes: B = 96 from 48 cached lines (duplicate envs, three 32-row tiles) and B = 33 without duplicates (a partial tile); SeqSlate
B = 64 over two pages.  Every case runs two episodes back to back: lanes and buffers are reused across the reward step's join
and a reset."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(96, 48, False), (33, 33, True)]       # (B, cache_size, is_eval)


def _make(tmp_path, kind, B, cache, is_eval, overlap):
    import rl4rs_amd
    from rl4rs_amd import synth
    from rl4rs_amd.env.slate import SlateRecEnv, SlateState
    from rl4rs_amd.env.seqslate import SeqSlateRecEnv, SeqSlateState
    d = str(tmp_path / ('on' if overlap else 'off'))
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
           "scorer_precision": "fp16x2"}
    if is_eval:
        cfg['is_eval'] = True
    if not overlap:
        cfg['no_step_overlap'] = True
    if seq:
        env = rl4rs_amd.make('SeqSlateRecEnv-v0', recsim=SeqSlateRecEnv(cfg, state_cls=SeqSlateState))
    else:
        env = rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))
    env.seed(11)
    return env, T


def _policy(env, obs, proj):
    """a deterministic function of the returned observation: argmax of a fixed projection under the observation-side mask"""
    import torch
    legal = env.samples._obs_mask().to(torch.bool)
    score = (obs.to(torch.float64) @ proj).masked_fill(~legal, -float('inf'))
    return score.argmax(dim=1).to(torch.int32)


def _drive(env, T, B, mode, episodes=2):
    """`episodes` episodes -> dict of everything the caller saw.  mode: 'hold', 'immediate', 'foreign', 'policy', 'reset'"""
    import torch
    from rl4rs_amd.device import DIEN_N_ACTIVE, DIEN_ALL_FEATURE, DIEN_SCORES, DIEN_QUERY
    out = {'obs': [], 'reward': [], 'action': [], 'last': [], 'click': [], 'extra': []}
    held, clones = [], []
    net = None
    proj = torch.randn((256, 284), dtype=torch.float64, generator=torch.Generator().manual_seed(5)).cuda()
    ev = None
    for ep in range(episodes):
        obs = env.reset()
        if net is None:
            net = env.sim.model.device_net
            net.set_profiling(True)
            net.profile_reset()
        out['obs'].append(obs.clone())
        acc = torch.zeros(B, dtype=torch.float32, device='cuda')
        tot = torch.zeros(B, dtype=torch.float64, device='cuda')
        for t in range(T):
            if mode == 'policy':
                a = _policy(env, obs, proj)
            else:
                a = env.offline_action
                out['action'].append(torch.as_tensor(a).clone())
                if mode == 'foreign' and t in (2, 5):
                    a = a.clone()
            if mode == 'hold' and ep == 0 and t == 1:
                ev = [torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)]
                ev[0].record()
            obs, reward, done, info = env.step(a)
            if mode == 'hold' and ep == 0 and t == 8:
                ev[1].record()
            if mode == 'hold':
                held.append(obs)                         # the caller keeps every step's tensor until the episode ends
                clones.append(obs.clone())
            elif mode == 'immediate':
                acc = acc + obs.sum(dim=1)               # on the caller's stream, right behind the step, nothing waited for
                tot = tot + reward
            elif mode == 'foreign' and t == 3:
                out['extra'].append(net.snapshot(DIEN_N_ACTIVE, 0)[:1].clone())      # rl4rs_dien_buffer between two steps: a join
                # the internal rows of the forward just issued (it ran on the second lane: the scorer's second scratch set)
                out['extra'] += [net.snapshot(DIEN_ALL_FEATURE, B)[:B].clone(), net.snapshot(DIEN_SCORES, B)[:, :B].clone(),
                                 net.snapshot(DIEN_QUERY, B)[:B].clone()]
            if mode != 'hold':
                out['obs'].append(obs.clone())
            out['reward'].append(torch.as_tensor(reward).clone())
            out['last'].append(torch.as_tensor(env.samples.last_actions).clone())
            if mode == 'reset' and ep == 0 and t == 3:
                break                                     # the caller resets in mid-episode (at step 4)
        if mode == 'hold':
            assert all(torch.equal(h, c) for h, c in zip(held, clones)), 'a held observation changed after it was handed out'
            assert len(set(h.data_ptr() for h in held)) == len(held)
            out['obs'] += clones
            held, clones = [], []
        if mode == 'immediate':
            out['extra'] += [acc.clone(), tot.clone()]
        if not (mode == 'reset' and ep == 0):
            out['click'].append(env.sim._stepper.click_probs().clone())
    torch.cuda.synchronize()
    out['profile'] = {k: v[1] for k, v in net.profile().items()}
    out['lanes'] = env.sim._stepper.lane_stats()
    out['ms'] = ev[0].elapsed_time(ev[1]) if ev else None
    return out


def _both(tmp_path, kind, B, cache, is_eval, mode):
    import torch
    res = {}
    for overlap in (True, False):
        env, T = _make(tmp_path, kind, B, cache, is_eval, overlap)
        res[overlap] = _drive(env, T, B, mode)
        del env
        torch.cuda.synchronize()
    on, off = res[True], res[False]
    for key in ('obs', 'reward', 'action', 'last', 'click', 'extra'):
        assert len(on[key]) == len(off[key]), key
        bad = [i for i, (x, y) in enumerate(zip(on[key], off[key])) if not torch.equal(x, y)]
        assert not bad, (key, bad)
    assert on['profile'] == off['profile']
    assert off['lanes'][:2] == (0, 0)
    return on, off


@pytest.mark.parametrize('B,cache,is_eval', SHAPES)
def test_replay_holding_outputs_and_overlap_in_force(tmp_path, B, cache, is_eval):
    """(a) + (g): the caller holds every step's obs; 4 + 4 lane transitions per episode with the overlap, none without."""
    on, off = _both(tmp_path, 'slate', B, cache, is_eval, 'hold')
    print('steps 1..8 of the first episode: overlap %.3f ms, serial %.3f ms (ratio %.3f; not asserted: chain-bound at this size)'
          % (on['ms'], off['ms'], on['ms'] / off['ms']))
    assert on['lanes'][:2] == (8, 8), on['lanes']        # two episodes
    assert on['lanes'][2] >= 2                           # the reward step of each episode joined


@pytest.mark.parametrize('B,cache,is_eval', SHAPES)
def test_immediate_use_on_the_callers_stream(tmp_path, B, cache, is_eval):
    """(b): reductions of obs and reward enqueued right behind every step, without any synchronisation."""
    on, _ = _both(tmp_path, 'slate', B, cache, is_eval, 'immediate')
    assert on['lanes'][:2] == (8, 8), on['lanes']


@pytest.mark.parametrize('B,cache,is_eval', SHAPES)
def test_foreign_action_and_buffer_join(tmp_path, B, cache, is_eval):
    """(c): a clone of the logged action at steps 2 and 5 (serial there, no special case); rl4rs_dien_buffer between two steps (a
    join): the active count, and the all-feature, score and query rows of a forward that ran on the scorer's second scratch set."""
    on, _ = _both(tmp_path, 'slate', B, cache, is_eval, 'foreign')
    assert on['lanes'][:2] == (8, 8), on['lanes']        # still lane transitions: they wait for the caller's stream instead


@pytest.mark.parametrize('B,cache,is_eval', SHAPES)
def test_policy_loop(tmp_path, B, cache, is_eval):
    """(d): the action is a function of the returned obs - nothing runs ahead."""
    _both(tmp_path, 'slate', B, cache, is_eval, 'policy')


def test_seqslate_page_turn(tmp_path):
    """(e): page_items 9, T = 18: the reward step of a page and the page turn behind it join."""
    on, _ = _both(tmp_path, 'seq', 64, 32, False, 'hold')
    # per episode: steps 0..7 of the first page run on lanes; step 8 has a reward due, step 9 is the page turn (no carried
    # partition); on the second page every env has a slot of its own: the hint is the batch, 2 * 2 * ceil(64 / 32) = 8 workgroups fit
    assert sum(on['lanes'][:2]) == 2 * (8 + 7), on['lanes']


@pytest.mark.parametrize('B,cache,is_eval', SHAPES)
def test_reset_inside_an_episode(tmp_path, B, cache, is_eval):
    """(f): env.reset() at step 4, with two transitions in flight; the next episode is the serial arm's."""
    on, _ = _both(tmp_path, 'slate', B, cache, is_eval, 'reset')
    assert on['lanes'][:2] == (2 + 4, 2 + 4), on['lanes']


def test_scorer_or_env_closed_before_the_stepper(tmp_path):
    """The scorer handle is closed under a live stepper (what a model reload, installed weights or a grown scorer do:
    device_net.close()), with lane transitions just issued; a logged-action tensor keeps the old stepper alive, which is destroyed
    later, when neither handle may be touched any more.  Then the same flow goes on: a new scorer, a new stepper on the same env, and
    its episode equals the serial arm's.  Last, an env handle closed before its stepper."""
    import gc
    import torch
    B = 96
    res = {}
    for overlap in (True, False):
        env, T = _make(tmp_path, 'slate', B, 48, False, overlap)
        env.reset()
        for t in range(3):
            env.step(env.offline_action)
        held = env.offline_action                          # aliases the stepper's memory: keeps the old stepper alive
        old = env.sim._stepper
        before = old.lane_stats()
        model = env.sim.model
        model.device_net.close()                           # the host waits for the lanes; the stepper is told the scorer went
        model.device_net = None
        model.max_rows = model.max_slots = 0
        # the stepper itself is alive and readable; closing the scorer joined the transitions in flight
        assert old.lane_stats() == ((2, 1, before[2] + 1) if overlap else (0, 0, 0))
        res[overlap] = _drive(env, T, B, 'immediate', episodes=1)      # a new scorer and a new stepper on the same env
        assert env.sim._stepper is not old
        del old, held
        env.sim._next_rows = {}
        gc.collect()                                       # the old stepper goes now, behind its scorer
        if overlap:
            assert res[overlap]['lanes'][:2] == (4, 4), res[overlap]['lanes']
            live, stepper = env.samples._live(), env.sim._stepper
            live.close()                                   # an env handle closed before its stepper
            stepper.close()
        del env
        gc.collect()
        torch.cuda.synchronize()
    on, off = res[True], res[False]
    for key in ('obs', 'reward', 'action', 'last', 'click', 'extra'):
        assert len(on[key]) == len(off[key]) and all(torch.equal(x, y) for x, y in zip(on[key], off[key])), key
