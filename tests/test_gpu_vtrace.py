"""GPU: V-trace (rl4rs_vtrace), the one-call V-trace loss (rl4rs_policy_vtrace_loss_grad) and ``Trainer(algo='PG' | 'IMPALA')``
against the float64 restatement in tests/vtrace_ref.py.

Bars.  vs / pg_adv: the kernel scans in float64 and rounds once on the store, so every entry is within one float32 spacing of the
float64 restatement (plus 1e-9 for near-zero pg_adv; float64 noise at these magnitudes is about 1e-11).  Statistics: relative 1e-12
to the float64 sums of the device's own float32 outputs, bit-identical between two runs.  One-call entry point: bit-identical to its
hand-composed parts; target_logp / values 1e-5 and the gradient 2e-4 of the reference gradient's max-norm (tests/test_gpu_policy.py).
Reference: script/modelfree_train.py:306-390."""
import os

import numpy as np
import pytest

import vtrace_ref as VR

pytestmark = pytest.mark.gpu


def _t(a, dt=None):
    import torch
    x = torch.from_numpy(np.ascontiguousarray(a))
    return (x if dt is None else x.to(dt)).cuda()


def _kernel_bar(out, ref):
    """|out - ref| <= spacing(float32(|ref|)) + 1e-9 on every entry -> (worst excess ratio, ok)."""
    err = np.abs(out.astype(np.float64) - ref)
    bar = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + 1e-9
    return float((err / bar).max()), bool((err <= bar).all())


def _vtrace_inputs(T, B, seed):
    rs = np.random.RandomState(seed)
    blp = rs.uniform(-4.0, -0.5, (T, B)).astype(np.float32)
    tlp = (blp + rs.uniform(-2.0, 2.0, (T, B))).astype(np.float32)         # log rho in [-2, 2]: both clips bind on about half
    V = (rs.randn(T, B) * 50 + 100).astype(np.float32)
    rew = (rs.rand(T, B) * 100).astype(np.float32).astype(np.float64)      # float32-representable, in the ABI's float64
    boot = (rs.randn(B) * 50 + 100).astype(np.float32)
    dones = (rs.rand(T, B) < 0.1).astype(np.int32)
    dones[max(T // 2 - 1, 0):T // 2 + 2, 0] = 0
    dones[T // 2, 0] = 1                                                    # a done in the middle of a column, none around it
    return blp, tlp, V, rew, boot, dones


@pytest.mark.parametrize('T,B', [(1, 1), (2, 67), (8, 256), (35, 100), (36, 1000)])
def test_vtrace_kernel_against_the_restatement(T, B):
    import torch
    from rl4rs_amd import device as D
    blp, tlp, V, rew, boot, dones = _vtrace_inputs(T, B, 7 * T + B)
    d_blp, d_tlp, d_V, d_rew, d_boot, d_dones = _t(blp), _t(tlp), _t(V), _t(rew), _t(boot), _t(dones)
    binding = np.exp(tlp.astype(np.float64) - blp)
    if T * B >= 100:
        assert 0.3 < (binding > 1.0).mean() < 0.7 and 0.3 < (binding > 0.7).mean() < 0.8
    for gamma in (1.0, 0.9):
        for with_dones in (False, True):
            for with_boot in (False, True):
                kw = dict(gamma=gamma, clip_rho=1.0, clip_pg_rho=0.7)
                vs, pg, st = D.vtrace(d_blp, d_tlp, d_V, d_rew, d_boot if with_boot else None, d_dones if with_dones else None, **kw)
                ref = VR.vtrace(blp, tlp, V, rew, boot if with_boot else None, dones if with_dones else None, **kw)
                vs_np, pg_np, st_np = vs.cpu().numpy(), pg.cpu().numpy(), st.cpu().numpy()
                case = (T, B, gamma, with_dones, with_boot)
                r_vs, ok_vs = _kernel_bar(vs_np, ref['vs'])
                r_pg, ok_pg = _kernel_bar(pg_np, ref['pg_adv'])
                print('vtrace %r: worst |err| / bar  vs %.3f  pg_adv %.3f' % (case, r_vs, r_pg))
                assert ok_vs and ok_pg, (case, r_vs, r_pg)
                want = VR.vtrace_stats(blp, tlp, vs_np, pg_np, clip_rho=1.0)
                print('   stats rel err', np.abs(st_np - want) / np.maximum(np.abs(want), 1e-300))
                assert (np.abs(st_np - want) <= 1e-12 * np.abs(want)).all(), (case, st_np, want)
                vs2, pg2, st2 = D.vtrace(d_blp, d_tlp, d_V, d_rew, d_boot if with_boot else None, d_dones if with_dones else None, **kw)
                assert torch.equal(vs, vs2) and torch.equal(pg, pg2) and torch.equal(st, st2), case


def test_vtrace_thresholds_are_not_swapped():
    """clip_rho = 1.0 / clip_pg_rho = 0.7 against the restatement with the two exchanged: far outside the bar."""
    from rl4rs_amd import device as D
    blp, tlp, V, rew, boot, dones = _vtrace_inputs(8, 256, 3)
    vs, pg, _ = D.vtrace(_t(blp), _t(tlp), _t(V), _t(rew), _t(boot), None, gamma=1.0, clip_rho=1.0, clip_pg_rho=0.7)
    swapped = VR.vtrace(blp, tlp, V, rew, boot, None, 1.0, 0.7, 1.0)
    assert not _kernel_bar(vs.cpu().numpy(), swapped['vs'])[1] and not _kernel_bar(pg.cpu().numpy(), swapped['pg_adv'])[1]


# ---- the one-call entry point ---------------------------------------------------------------------------------------------------

def _policy_data(N, rs, OD, A):
    obs = rs.randn(N, OD).astype(np.float32)
    mask = (rs.rand(N, A) < 0.4).astype(np.int64)
    mask[np.arange(N), rs.randint(0, A, size=N)] = 1          # at least one allowed action per row
    W = (A + 31) // 32
    bits = np.zeros((N, W), dtype=np.uint32)
    for k in range(A):
        bits[:, k >> 5] |= (mask[:, k].astype(np.uint32) << np.uint32(k & 31))
    return obs, mask, bits.view(np.int32)


def _rollout_batch(R, T, B, OD, HID, A, seed):
    """A policy handle and an [R, T, B] batch whose behaviour log-probs trail the learner's (rho != 1)."""
    from rl4rs_amd.device import DevicePolicy
    from rl4rs_amd.nets.policy import init_policy_params
    rs = np.random.RandomState(seed)
    N = R * T * B
    obs, mask, bits = _policy_data(N, rs, OD, A)
    n_par = OD * HID + HID + HID * (A + 1) + A + 1
    flat = init_policy_params(OD, HID, A, seed=seed) + (rs.randn(n_par) * 0.02).astype(np.float32)
    pol = DevicePolicy(OD, HID, A, max_rows=N, params=flat)
    o, b = _t(obs), _t(bits)
    act, lp = pol.act(o, b, seed=seed, step=1)[:2]
    blp = (lp.cpu().numpy() + rs.uniform(-1.0, 1.0, N)).astype(np.float32)
    rew = (rs.rand(N) * 100).astype(np.float32).astype(np.float64)
    dones = (rs.rand(N) < 0.05).astype(np.int32)
    return dict(pol=pol, flat=flat, obs=obs, mask=mask, o=o, b=b, act=act, blp=_t(blp), rew=_t(rew), dones=_t(dones), N=N)


KW = dict(gamma=0.9, clip_rho=1.0, clip_pg_rho=0.7, vf_coeff=0.5, ent_coeff=0.01)


@pytest.mark.parametrize('R,T,B', [(1, 9, 64), (2, 4, 37)])
@pytest.mark.parametrize('drop_last', [True, False])
def test_one_call_equals_its_parts(R, T, B, drop_last):
    import torch
    from rl4rs_amd import device as D
    d = _rollout_batch(R, T, B, 256, 64, 284, seed=R * 10 + T)
    pol, N = d['pol'], d['N']
    g, stats, vstats, (vs, pg) = pol.vtrace_loss_grad(R, T, B, d['o'], d['act'], d['blp'], d['rew'], mask_bits=d['b'], dones=d['dones'],
                                                      drop_last=drop_last, want_vtrace=True, **KW)
    g, stats, vstats = g.clone(), stats.clone(), vstats.clone()
    # the hand-composed chain: evaluate -> rl4rs_vtrace per rollout -> loss_grad(algo 0) on the kept rows
    lp, v = pol.evaluate(d['o'], d['act'], d['b'])[:2]
    Te = T - 1 if drop_last else T
    sh = lambda x: x.view(R, T, B)
    vs_p, pg_p, vst = [], [], torch.zeros(4, dtype=torch.float64, device='cuda')
    for r in range(R):
        a, b, s = D.vtrace(sh(d['blp'])[r, :Te].contiguous(), sh(lp)[r, :Te].contiguous(), sh(v)[r, :Te].contiguous(),
                           sh(d['rew'])[r, :Te].contiguous(), sh(v)[r, T - 1].contiguous() if drop_last else None,
                           sh(d['dones'])[r, :Te].contiguous(), gamma=KW['gamma'], clip_rho=KW['clip_rho'], clip_pg_rho=KW['clip_pg_rho'])
        vs_p.append(a.reshape(-1)); pg_p.append(b.reshape(-1)); vst += s
    rows = torch.from_numpy(VR.kept_rows(R, T, B, drop_last)).cuda()
    assert len(rows) == R * Te * B
    g2, stats2 = pol.loss_grad(0, d['o'][rows].contiguous(), d['act'][rows].contiguous(), torch.cat(pg_p), torch.cat(vs_p),
                               mask_bits=d['b'][rows].contiguous(), vf_coeff=KW['vf_coeff'], ent_coeff=KW['ent_coeff'])
    assert torch.equal(g, g2) and torch.equal(stats, stats2)
    assert torch.isfinite(g).all() and g.abs().max().item() > 0
    assert torch.equal(vs[rows], torch.cat(vs_p)) and torch.equal(pg[rows], torch.cat(pg_p))
    assert np.allclose(vstats.cpu().numpy(), vst.cpu().numpy(), rtol=1e-12, atol=0)
    if drop_last:
        # the rows of a dropped step contribute exactly nothing: their actions, rewards and behaviour log-probs are never seen
        dropped = np.setdiff1d(np.arange(N), rows.cpu().numpy())
        assert len(dropped) == R * B and not vs[dropped].any() and not pg[dropped].any()
        act2, rew2, blp2 = d['act'].clone(), d['rew'].clone(), d['blp'].clone()
        act2[dropped] = (act2[dropped] + 17) % 284
        rew2[dropped] = 1e6
        blp2[dropped] = -30.0
        g3, stats3, vstats3, _ = pol.vtrace_loss_grad(R, T, B, d['o'], act2, blp2, rew2, mask_bits=d['b'], dones=d['dones'],
                                                      drop_last=True, **KW)
        assert torch.equal(g, g3) and torch.equal(stats, stats3) and torch.equal(vstats, vstats3)


def test_one_call_refuses_what_it_cannot_run():
    from rl4rs_amd._lib import Rl4rsHipError
    d = _rollout_batch(1, 1, 8, 256, 64, 284, seed=2)
    with pytest.raises(Rl4rsHipError, match='drop_last'):
        d['pol'].vtrace_loss_grad(1, 1, 8, d['o'], d['act'], d['blp'], d['rew'], mask_bits=d['b'], drop_last=True)
    d['pol'].vtrace_loss_grad(1, 1, 8, d['o'], d['act'], d['blp'], d['rew'], mask_bits=d['b'], drop_last=False)     # T = 1 is fine without
    big = _rollout_batch(1, 2, 8, 256, 64, 284, seed=2)
    with pytest.raises(Rl4rsHipError, match='max_rows'):
        d['pol'].vtrace_loss_grad(1, 2, 8, big['o'], big['act'], big['blp'], big['rew'], mask_bits=big['b'])


@pytest.mark.parametrize('OD,HID,A', [(256, 64, 284), (100, 48, 75)])          # the tiled kernels / the one-wave path
@pytest.mark.parametrize('drop_last', [True, False])
def test_one_call_against_the_restatement(OD, HID, A, drop_last):
    from oracle import policy as OP
    R, T, B = 2, 5, 33
    d = _rollout_batch(R, T, B, OD, HID, A, seed=4)
    pol, N = d['pol'], d['N']
    g, stats, vstats, (vs, pg) = pol.vtrace_loss_grad(R, T, B, d['o'], d['act'], d['blp'], d['rew'], mask_bits=d['b'], dones=d['dones'],
                                                      drop_last=drop_last, want_vtrace=True, **KW)
    g_np, vs_np, pg_np = g.cpu().numpy(), vs.cpu().numpy(), pg.cpu().numpy()
    act = d['act'].cpu().numpy()
    # the learner's forward, to the project's 1e-5
    lp, v = [x.cpu().numpy() for x in d['pol'].evaluate(d['o'], d['act'], d['b'])[:2]]
    logits, value = OP.forward(d['flat'], d['obs'], d['mask'], od=OD, hid=HID, A=A)
    lp_ref = OP.log_softmax(logits)[np.arange(N), act]
    print('target_logp err %.3g  values err %.3g' % (np.abs(lp - lp_ref).max(), np.abs(v - value).max()))
    assert np.abs(lp - lp_ref).max() < 1e-5 and np.abs(v - value).max() < 1e-5
    # V-trace against the restatement fed the device's own target_logp and values: the kernel bar
    blp, rew, dones = d['blp'].cpu().numpy(), d['rew'].cpu().numpy(), d['dones'].cpu().numpy()
    vs_ref, pg_ref = VR.vtrace_rollouts(R, T, B, blp, lp, v, rew, dones, KW['gamma'], KW['clip_rho'], KW['clip_pg_rho'], drop_last)
    r_vs, ok_vs = _kernel_bar(vs_np, vs_ref)
    r_pg, ok_pg = _kernel_bar(pg_np, pg_ref)
    print('worst |err| / bar  vs %.3f  pg_adv %.3f' % (r_vs, r_pg))
    assert ok_vs and ok_pg, (r_vs, r_pg)
    rows = VR.kept_rows(R, T, B, drop_last)
    want = VR.vtrace_stats(blp.reshape(R, T, B)[:, :len(rows) // (R * B)], lp.reshape(R, T, B)[:, :len(rows) // (R * B)], vs_np[rows], pg_np[rows],
                           KW['clip_rho'])
    assert np.allclose(vstats.cpu().numpy(), want, rtol=1e-12, atol=0)
    # the gradient against the restatement's, taken with the device's vs and pg_adv
    g_ref, s_ref = VR.vtrace_loss_and_grad(d['flat'], d['obs'], d['mask'], act, vs_np, pg_np, rows, KW['vf_coeff'], KW['ent_coeff'], OD, HID, A)
    print('grad err %.3g of max-norm %.3g' % (np.abs(g_np - g_ref).max(), np.abs(g_ref).max()))
    assert np.abs(g_np - g_ref).max() < 2e-4 * np.abs(g_ref).max()
    assert np.allclose(stats.cpu().numpy(), s_ref, rtol=2e-4, atol=1e-3)


# ---- Trainer(algo='PG' | 'IMPALA') ----------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def files(tmp_path_factory):
    from rl4rs_amd import synth
    d = str(tmp_path_factory.mktemp('vtrace_env'))
    text = synth.make_catalog_text(seed=4)
    synth.write_text(os.path.join(d, 'c.csv'), text)
    for name, pages in (('log.csv', 1), ('seqlog.csv', 4)):
        recs = synth.make_records(300, pages=pages, seed=2, hash_size=2000, special_ids=synth.special_ids_from_text(text))
        synth.write_records(os.path.join(d, name), recs)
    return d


def _env(d, seq=False):
    """The small synthetic Slate env of test_training_loop_runs_and_improves_masked_policy (B = 64, T = 9), or a SeqSlate one built the
    same way with max_steps 18: its first page's reward falls on step 8, a kept step."""
    import rl4rs_amd
    cfg = {"maxlen": 64, "batch_size": 64, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
           "category_feature_num": 21, "category_hash_size": 2000, "seq_num": 2, "emb_size": 128, "page_items": 9,
           "hidden_units": 128, "max_steps": 18 if seq else 9, "action_emb_size": 32, "sample_file": os.path.join(d, 'seqlog.csv' if seq else 'log.csv'),
           "iteminfo_file": os.path.join(d, 'c.csv'), "cache_size": 256, "model_seed": 3, "return_tensors": True}
    if seq:
        from rl4rs_amd.env.seqslate import SeqSlateRecEnv, SeqSlateState
        env = rl4rs_amd.make('SeqSlateRecEnv-v0', recsim=SeqSlateRecEnv(cfg, state_cls=SeqSlateState))
    else:
        from rl4rs_amd.env.slate import SlateRecEnv, SlateState
        env = rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))
    env.seed(100)
    return env


def test_pg_trainer(files):
    import torch
    from rl4rs_amd.train import Trainer
    env = _env(files)
    assert Trainer(env, algo='A2C').lr == 1e-4 and Trainer(env, algo='PPO').lr == 1e-4 and Trainer(env, algo='IMPALA').lr == 1e-4
    assert Trainer(env, algo='PG', lr=3e-3).lr == 3e-3
    tr = Trainer(env, algo='PG', seed=1)
    assert tr.lr == 4e-4                                       # the driver's value for PG
    p0 = tr.policy.params().clone()
    outs = [tr.train_iteration() for _ in range(3)]
    assert all(np.isfinite(list(o.values())).all() for o in outs)
    p1 = tr.policy.params()
    assert torch.isfinite(p1).all() and not torch.equal(p0, p1)
    # no critic: the value head (column A of W2e, b2e[A]) receives a zero gradient and keeps its bits
    OD, HID, AE = 256, 64, 285
    w2 = lambda p: p[OD * HID + HID:OD * HID + HID + HID * AE].view(HID, AE)
    assert torch.equal(w2(p0)[:, AE - 1], w2(p1)[:, AE - 1]) and torch.equal(p0[-1], p1[-1])
    assert not torch.equal(w2(p0)[:, :AE - 1], w2(p1)[:, :AE - 1])
    assert env.samples.get_violation().all()                    # only legal slates
    assert outs[-1]['episode_reward_mean'] > 0


def _impala(files, iters, seq=True, **kw):
    """-> (trainer, env, per call: (statistics, actor == learner after the call), initial parameters)."""
    import torch
    from rl4rs_amd.train import Trainer
    env = _env(files, seq=seq)
    tr = Trainer(env, algo='IMPALA', seed=1, init_seed=5, **kw)
    p0 = tr.policy.params().clone()
    assert torch.equal(p0, tr.actor.params())
    log = []
    for _ in range(iters):
        st = dict(tr.train_iteration())
        log.append((st, torch.equal(tr.actor.params(), tr.policy.params())))
    return tr, env, log, p0


def test_impala_on_policy_with_broadcast_every_update(files):
    import torch
    tr, env, log, p0 = _impala(files, 3, broadcast_interval=1, lr=1e-2)
    for st, same in log:
        assert np.isfinite(list(st.values())).all()
        print('rho_mean - 1 = %.3g' % (st['rho_mean'] - 1.0))
        assert abs(st['rho_mean'] - 1.0) <= 1e-5 and abs(st['rho_clipped_mean'] - 1.0) <= 1e-5
        assert same                                             # actor parameters equal the learner's after each call
    assert not torch.equal(p0, tr.policy.params())
    assert env.samples.get_violation().all()
    for k in ('episode_reward_mean', 'policy_loss', 'vf_loss', 'entropy', 'rho_mean', 'rho_clipped_mean', 'vs_mean', 'iteration'):
        assert k in log[-1][0], k


def test_impala_stale_actor_and_determinism(files):
    import torch
    runs = []
    for _ in range(2):
        tr, env, log, _ = _impala(files, 2, broadcast_interval=2, lr=1e-2)
        (st1, same1), (st2, same2) = log
        assert abs(st1['rho_mean'] - 1.0) <= 1e-5                # first call: the actor still is the learner's initial copy
        assert not same1                                         # ... and is NOT refreshed after the first update
        print('stale actor: rho_mean - 1 = %.3g' % (st2['rho_mean'] - 1.0))
        assert st2['rho_mean'] != 1.0 and abs(st2['rho_mean'] - 1.0) > 1e-5      # second call: off-policy
        assert st2['rho_clipped_mean'] <= st2['rho_mean'] and st2['rho_clipped_mean'] <= 1.0 + 1e-12
        assert same2                                             # copied after the second update
        runs.append((tr.policy.params().clone(), tr.actor.params().clone(), st2))
        tr.close()
    # two trainers with the same seeds end with bit-identical parameters
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]


def test_impala_drop_last_sees_no_reward_on_slate(files):
    """SlateRecEnv-v0 pays its only reward at the last step.  drop_last=True drops that step, so with gamma 1 and rho = 1 every
    delta telescopes and vs_t is the bootstrap value: vs_mean = the mean bootstrap.  The bar: float32 storage of vs (2^-24 relative)
    plus (rho - 1) * (value differences) over at most T steps, with |rho - 1| <= 1e-5 as asserted above."""
    import torch
    from rl4rs_amd.device import DevicePolicy
    from rl4rs_amd.train import Trainer
    env = _env(files)
    got = {}
    for drop_last in (True, False):
        env.seed(100)
        tr = Trainer(env, algo='IMPALA', seed=1, init_seed=5, drop_last=drop_last, keep_last_batch=True)
        p0 = tr.policy.params().clone()
        st = dict(tr.train_iteration())
        lb = tr.last_batch
        T, B = tr.T, tr.B
        ref = DevicePolicy(256, 64, 284, max_rows=T * B, params=p0.cpu().numpy())
        v = ref.evaluate(lb['obs'], lb['act'], lb['mask'])[1].view(T, B).double()
        boot_mean, vmax = v[T - 1].mean().item(), v.abs().max().item()
        assert lb['rew'].view(T, B)[:T - 1].abs().max().item() == 0.0 and lb['rew'].view(T, B)[T - 1].max().item() > 0
        last = lb['rew'].view(T, B)[T - 1]
        tol = 2e-5 * T * (vmax + (0.0 if drop_last else last.max().item())) + 1e-6 * abs(boot_mean)
        got[drop_last] = (st['vs_mean'], boot_mean, tol, last.mean().item())
        print('drop_last %r: vs_mean %.9g  mean bootstrap %.9g  tol %.3g' % (drop_last, st['vs_mean'], boot_mean, tol))
        tr.close()
    vs_mean, boot_mean, tol, _ = got[True]
    assert abs(vs_mean - boot_mean) <= tol
    vs_mean, boot_mean, tol, rew_mean = got[False]
    assert abs(vs_mean - boot_mean) > 100 * tol                  # all T steps: vs is the reward-to-go, the last step's reward
    assert abs(vs_mean - rew_mean) <= tol
