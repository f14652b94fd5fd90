"""TEST INFRASTRUCTURE ONLY - the bodies of the on-device Rainbow's GPU checks, shared by tests/test_gpu_rainbow.py (the reference
net width) and tests/test_gpu_rainbow_shapes.py (the ends of what rl4rs_distq_create admits).  A case ``c`` is rainbow_ref.make_case's
dict, ``ref0`` its float64 reference without teacher forcing, ``bars`` = (Q, td, gradient) as rainbow_ref states them."""
import numpy as np

import rainbow_ref as R
import td3_ref


def reference(c):
    return R.loss_and_grad(c['flat'], c['tflat'], c['obs'], c['act'], c['rew'], c['done'], c['nobs'], c['mask'], c['w'], c['gamma_n'],
                           c['double_q'], c['dm'])


def bars_of(measured):
    return R.BAR_FACTOR * measured['q'], R.BAR_FACTOR * measured['td'], R.BAR_FACTOR * measured['grad_rel']


def net(c, max_rows):
    from rl4rs_amd.device import DeviceDistQ
    dm = c['dm']
    return DeviceDistQ(dm.od, dm.A, max_rows=max_rows, num_atoms=dm.atoms, v_min=dm.v_min, v_max=dm.v_max, dueling=dm.dueling,
                       trunk=dm.trunk, stream_hidden=dm.sh, params=c['flat'])


def to_device(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def loss_inputs(c):
    return dict((k, to_device(c[k])) for k in ('tflat', 'obs', 'nobs', 'bits', 'done', 'act', 'rew', 'w'))


def check_loss_and_gradient(c, ref0, bars):
    import torch
    dm, N = c['dm'], c['N']
    q_bar, td_bar, g_bar = bars
    dq = net(c, N)
    d = loss_inputs(c)
    run = lambda nobs, bits: dq.loss_grad(d['tflat'], d['obs'], d['act'], d['rew'], d['done'], nobs, bits, weights=d['w'],
                                          gamma_n=c['gamma_n'], double_q=c['double_q'], want_next_action=True)
    g, td, stats, astar = run(d['nobs'], d['bits'])
    g_np, td_np, a_np = g.cpu().numpy(), td.cpu().numpy(), astar.cpu().numpy()
    boot, gap = ref0['boot'], ref0['gap']
    if c['masked']:
        assert (~boot & (c['done'] == 0)).sum() == 1 and not boot[c['k']]
    # the integer a*: equal wherever the float64 decision is not a near-tie; terminal rows report -1
    firm = boot & (gap >= 10.0 * q_bar)
    left_out = int((boot & ~firm).sum())
    print('a*: %d of %d bootstrapping rows under the %.3g gap' % (left_out, int(boot.sum()), 10.0 * q_bar))
    assert left_out <= 0.01 * boot.sum()
    assert np.array_equal(a_np[firm], ref0['astar_ref'][firm])
    assert (a_np[c['done'] != 0] == -1).all()
    assert ((a_np[boot] >= 0) & (a_np[boot] < dm.A)).all()
    if c['masked']:
        assert c['mask'][np.nonzero(boot)[0], a_np[boot]].all()
    # loss and gradient of the restatement with the device's a* on the bootstrapping rows
    ref = R.loss_and_grad(c['flat'], c['tflat'], c['obs'], c['act'], c['rew'], c['done'], c['nobs'], c['mask'], c['w'], c['gamma_n'],
                          c['double_q'], dm, astar=a_np)
    err_td = np.abs(td_np - ref['td']).max()
    err_g, g_max = np.abs(g_np - ref['grad']).max(), np.abs(ref['grad']).max()
    print('td err %.3g (bar %.3g)  grad err %.3g of the max-norm (bar %.3g)' % (err_td, td_bar, err_g / g_max, g_bar))
    lo = 0
    for name, hi in zip(R.NAMES, dm.ends()):
        print('    %-4s err %.3g of the max-norm' % (name, np.abs(g_np[lo:hi] - ref['grad'][lo:hi]).max() / g_max))
        lo = hi
    assert np.isfinite(g_np).all() and np.isfinite(td_np).all() and np.isfinite(stats.cpu().numpy()).all()
    assert err_td < td_bar
    assert err_g < g_bar * g_max
    assert (td_np >= 0).all()
    s_np = stats.cpu().numpy().astype(np.float64)
    # sums of N terms: N x the per-row bars (Q-valued terms: the Q bar), plus the fp32 rounding of the sum itself
    tol = np.array([N * td_bar * 1.1, N * q_bar, N * q_bar, N * td_bar]) + 1e-6 * np.abs(ref['stats']) * np.sqrt(N)
    assert (np.abs(s_np - ref['stats']) < tol).all(), (s_np, ref['stats'], tol)
    # sum_i m_i = 1 on every row: the projected target's mean lies inside the support
    assert dm.v_min * N - tol[2] <= s_np[2] <= dm.v_max * N + tol[2]
    # the all-masked non-terminal successor bootstraps nothing: its target is the point clip(R)
    if c['masked']:
        assert abs(td_np[c['k']] - ref['td'][c['k']]) < td_bar
    # bit-identical from run to run
    g2, td2, stats2, astar2 = run(d['nobs'], d['bits'])
    assert torch.equal(g, g2) and torch.equal(td, td2) and torch.equal(stats, stats2) and torch.equal(astar, astar2)
    # nothing of a terminal row's successor is used: NaN observations and junk mask words there change nothing
    nobs_nan = d['nobs'].clone()
    nobs_nan[d['done'] != 0] = float('nan')
    bits_junk = None
    if d['bits'] is not None:
        bits_junk = d['bits'].clone()
        bits_junk[d['done'] != 0] = 0x5a5a5a5a
    g3, td3, stats3, astar3 = run(nobs_nan, bits_junk)
    assert torch.equal(g, g3) and torch.equal(td, td3) and torch.equal(stats, stats3) and torch.equal(astar, astar3)
    return dict(td=err_td, grad_rel=err_g / g_max)


def check_dueling_gradient_sums_to_zero(c, ref0):
    """dAdv[a', j] = g[j] (delta(a' = a) - 1 / A): for every atom j the advantage head's weight and bias gradients sum to zero over
    the actions, within the rounding of the sums (this fails if the -1 / A term is missing: the sum is then S = h_a^T g itself).
    Bar: each of the two fp32 sums behind an entry (the gathered columns, S) carries at most N 2^-24 of sum_n |h_a| |g|, and the
    test adds A of them: 4 N 2^-24 max_kj (|h_a|^T |g|)."""
    dm, N = c['dm'], c['N']
    assert dm.dueling
    dq = net(c, N)
    d = loss_inputs(c)
    g = dq.loss_grad(d['tflat'], d['obs'], d['act'], d['rew'], d['done'], d['nobs'], d['bits'], weights=d['w'], gamma_n=c['gamma_n'],
                     double_q=c['double_q'])[0].cpu().numpy().astype(np.float64)
    parts = R.split(g, dm)
    p = R.split(c['flat'].astype(np.float64), dm)
    ha = R.hidden(p, c['obs'].astype(np.float64), dm)[2]
    abs_s = np.abs(ha).T @ np.abs(ref0['g'])
    S = ha.T @ ref0['g']
    bar = 4.0 * N * 2.0 ** -24 * abs_s.max()
    sum_w = parts['Wa2'].reshape(dm.sh, dm.A, dm.atoms).sum(axis=1)
    sum_b = parts['ba2'].reshape(dm.A, dm.atoms).sum(axis=0)
    print('sum over actions: dWa2 %.3g, dba2 %.3g (bar %.3g; |S| max %.3g)' % (np.abs(sum_w).max(), np.abs(sum_b).max(), bar, np.abs(S).max()))
    assert np.abs(S).max() > 10.0 * bar                      # the test can tell the term's absence
    assert np.abs(sum_w).max() < bar
    assert np.abs(sum_b).max() < 4.0 * N * 2.0 ** -24 * np.abs(ref0['g']).sum(axis=0).max()


def check_acting(c, q_bar, temperature):
    import torch
    dm, N = c['dm'], c['N']
    dq = net(c, N)
    obs, bits = to_device(c['obs']), to_device(c['bits'])
    a, u, q = dq.act(obs, bits, temperature=temperature, seed=11, step=5, want_u=True, want_q=True)
    a_np, u_np, q_np = a.cpu().numpy(), u.cpu().numpy().astype(np.float64), q.cpu().numpy().astype(np.float64)
    q_ref = R.masked_q(R.forward(c['flat'], c['obs'], dm)[2], c['mask'])
    allowed = np.ones((N, dm.A), dtype=bool) if c['mask'] is None else c['mask'] > 0
    err_q = np.abs(q_np - q_ref)[allowed].max()
    print('Q err %.3g (bar %.3g)' % (err_q, q_bar))
    assert err_q < q_bar and np.isfinite(q_np).all()
    assert (q.cpu().numpy()[~allowed] == np.float32(R.F32_MIN)).all()          # (compared in float32: the value the kernel writes)
    # the variate is the counter RNG's, keyed (seed, step, row, 0)
    assert np.array_equal(u_np, td3_ref.uniform01(11, 5, np.arange(N), 0))
    a_ref, dist = R.softq_draw(R.softq_cdf(q_ref, c['mask'], temperature), u_np)
    bar = R.softq_edge_bar(q_bar, temperature)
    firm = dist >= bar
    print('draw: %d of %d rows within %.3g of a CDF edge' % ((~firm).sum(), N, bar))
    assert (~firm).sum() <= 0.01 * N
    assert np.array_equal(a_np[firm], a_ref[firm])
    assert ((a_np >= 0) & (a_np < dm.A)).all()
    # greedy: the first maximum, wherever the float64 top-two gap is not a near-tie
    ga, gq = dq.greedy(obs, bits, want_q=True)
    ga_np = ga.cpu().numpy()
    assert torch.equal(gq, q)
    top = np.sort(q_ref, axis=1)[:, -2:]
    firm = (top[:, 1] - top[:, 0]) >= 10.0 * q_bar
    assert (~firm).sum() <= 0.01 * N + (0 if c['mask'] is None else 1)          # (+ the one row that allows nothing)
    assert np.array_equal(ga_np[firm], q_ref.argmax(axis=1)[firm])
    assert np.array_equal(ga_np, q.cpu().numpy().argmax(axis=1))               # the FIRST maximum of the row it reports
    if c['mask'] is not None:
        k = c['k']
        assert not allowed[k].any() and a_np[k] == 0 and ga_np[k] == 0         # a fully masked row returns 0
        ok = allowed.any(axis=1)
        assert allowed[np.nonzero(ok)[0], a_np[ok]].all() and allowed[np.nonzero(ok)[0], ga_np[ok]].all()
    # the same call twice: the same draw
    a2 = dq.act(obs, bits, temperature=temperature, seed=11, step=5)[0]
    assert torch.equal(a, a2)
    return err_q
