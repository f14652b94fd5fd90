"""The continuous learners' networks and loss kernels (csrc/contirl.hpp, csrc/amlp_fused.hpp) AWAY from the one geometry the
learners' own tests run them at (observation 266, action / latent 32, minibatches of 32 .. 256, at most 10 sampled actions):
the widths are run-time arguments of nearly every kernel here.  References: float64, oracle.offline_conti.OracleAMLP for the
networks and the numpy formulas of tests/conti_ref.py for the leaf kernels; tests/test_conti_shapes_host.py proves without a
GPU what the crafted inputs are built to show.

Fused fp32 minibatch kernels (k_amlp_fwd4<1|2>, k_amlp_bwd4<1|2>, k_gemm_tn4_group, the transposes), cases
(obs_dim D, act_dim E, out_dim K, head, rows N), each with the 4-row form, the 8-row form and the per-layer launches:
  (10, 5, 3, none, 5)        KX = D + E = 15: one ring round, 49 padded k; odd E, K; one full + one ragged 4-row workgroup
  (59, 5, 1, none, 1)        KX = 64 exactly; a single row
  (60, 5, 7, tanh, 9)        KX = 65: a second round with one live k
  (37, 0, 33, relu, 6)       no action input (the E == 0 buffer descriptor of the backward); K just over half a wave
  (40, 64, 64, sigmoid, 12)  both upper limits: all 64 lanes of the dact and head partial sums live
  (40, 33, 2, elu, 11)       odd E over half a wave; the elu head (fp32 forms only)
  (300, 1, 1, none, 3)       E = 1: ve = min(lane, 0), w1at of stride 1
  (1400, 8, 4, none, 5)      the 8-row form over 64 KB of dynamic LDS, the 4-row form under it
  (4064, 32, 1, none, 5)     KX = 4096, the documented limit: 78 KB / 156 KB of dynamic LDS
  (4065, 32, 1, none, 5)     one past the limit: falls back to the per-layer launches and is still right
  (266, 32, 1, none, N)      N = 1, 3, 1024 fused both ways; 1025, 2048 fused forward + per-layer backward (TN4_MAX_SAMPLES); 2049 per-layer
  (266, 32, 32, tanh, 1025)  the mixed path with a wide head

Bars.  Networks with KX <= 300, the multi-network launches, the stale-transpose sequences: the project's own - forward 2e-4 x
max(1, |want|), every gradient array within 2e-3 of its own largest entry (tests/test_gpu_offline_conti.py).  The rows
with KX > 300 (four: 301, 1408, 4096, 4097) and every value comparison of a leaf kernel: nobody had measured those sums at
these lengths, so the yardstick is the same reference evaluated in float32 on the CPU on the very inputs of the case, the
bar 4 x that (conti_ref.BAR_FACTOR: the device adds in another order) with a floor of 4 x 2^-23 x the result's scale.  Integer and piecewise outcomes (best, pick_rows,
the twin_min selectors, clamp-blocked gradients, untouched destination columns, multi against single launches): exact.

Measured on an MI355X (max |device - float64| against the bar; `-s` prints every line):
  case                              worst output  device    yardstick  bar       device / bar
  300x1x1-none-N3 rows4             dact      1.72e-09   7.86e-10  4.37e-09  0.39
  300x1x1-none-N3 rows8             fc1_w     1.76e-08   1.27e-08  6.34e-08  0.28
  300x1x1-none-N3 per-layer         out       6.23e-08   6.70e-08  2.68e-07  0.23
  1400x8x4-none-N5 rows4            out       9.09e-08   7.63e-08  3.05e-07  0.30
  1400x8x4-none-N5 rows8            fc1_w     7.99e-08   5.76e-08  2.31e-07  0.35
  1400x8x4-none-N5 per-layer        dact      1.88e-09   1.47e-09  5.87e-09  0.32
  4064x32x1-none-N5 rows4           out       8.85e-08   4.49e-08  1.80e-07  0.49
  4064x32x1-none-N5 rows8           fc1_w     3.24e-08   1.86e-08  7.48e-08  0.43
  4064x32x1-none-N5 per-layer       out       9.03e-08   4.49e-08  1.80e-07  0.50
  4065x32x1-none-N5 rows4           out       8.18e-08   7.75e-08  3.10e-07  0.26
  4065x32x1-none-N5 rows8           out       8.18e-08   7.75e-08  3.10e-07  0.26
  4065x32x1-none-N5 per-layer       out       8.18e-08   7.75e-08  3.10e-07  0.26
  cvae-N1-E5-L7-beta0.5             kl        6.24e-06   6.24e-06  3.92e-05  0.16
  cvae-N1-E5-L7-beta0               kl        6.24e-06   6.24e-06  3.92e-05  0.16
  cvae-N4-E64-L64-beta0.5           mse       5.59e-06   2.04e-06  2.40e-05  0.23
  cvae-N4-E64-L64-beta0             mse       5.59e-06   2.04e-06  2.40e-05  0.23
  cvae-N257-E70-L3-beta0.5          d_dec     2.07e-11   2.07e-11  8.28e-11  0.25
  cvae-N257-E70-L3-beta0            d_dec     2.07e-11   2.07e-11  8.28e-11  0.25
  cvae-N1000-E32-L130-beta0.5       d_dec     1.32e-11   1.32e-11  5.29e-11  0.25
  cvae-N1000-E32-L130-beta0         d_dec     1.32e-11   1.32e-11  5.29e-11  0.25
  critic_mse-N1                     loss2     2.58e-06   2.58e-06  3.21e-05  0.08
  critic_mse-N255                   dq2       1.07e-08   1.07e-08  5.69e-08  0.19
  critic_mse-N257                   dq1       6.90e-09   6.90e-09  4.26e-08  0.16
  critic_mse-N1000                  dq1       2.98e-09   2.98e-09  1.41e-08  0.21
  squashed-A1-rep1                  logp      1.42e-06   1.42e-06  1.00e-05  0.14
  squashed-A1-rep3                  logp      2.16e-06   2.16e-06  9.64e-06  0.22
  squashed-A1-rep3-strided          logp      2.16e-06   2.16e-06  9.64e-06  0.22
  squashed-A1-mean                  act       2.10e-08   5.15e-08  4.67e-07  0.04
  squashed-A5-rep1                  logp      3.23e-06   2.43e-06  2.30e-05  0.14
  squashed-A5-rep3                  logp      3.19e-06   3.19e-06  2.64e-05  0.12
  squashed-A5-rep3-strided          logp      3.19e-06   3.19e-06  2.64e-05  0.12
  squashed-A5-mean                  act       5.61e-08   5.15e-08  4.52e-07  0.12
  squashed-A64-rep1                 logp      3.01e-05   1.50e-05  1.27e-04  0.24
  squashed-A64-rep3                 act       1.39e-07   1.94e-07  7.78e-07  0.18
  squashed-A64-rep3-strided         act       1.39e-07   1.94e-07  7.78e-07  0.18
  squashed-A64-mean                 act       6.38e-08   5.80e-08  4.76e-07  0.13
  squashed-A65-rep1                 act       8.54e-08   1.19e-07  4.77e-07  0.18
  squashed-A65-rep3                 act       1.18e-07   1.86e-07  7.45e-07  0.16
  squashed-A65-rep3-strided         act       1.18e-07   1.86e-07  7.45e-07  0.16
  squashed-A65-mean                 act       6.15e-08   5.87e-08  4.77e-07  0.13
  squashed-A130-rep1                logp      6.54e-05   3.49e-05  2.75e-04  0.24
  squashed-A130-rep3                act       1.86e-07   2.75e-07  1.10e-06  0.17
  squashed-A130-rep3-strided        act       1.86e-07   2.75e-07  1.10e-06  0.17
  squashed-A130-mean                act       5.57e-08   5.93e-08  4.76e-07  0.12
  sac_actor_grad-B1-A5              d_head    1.44e-07   9.45e-08  1.08e-06  0.13
  sac_actor_grad-B300-A65           d_head    7.42e-09   8.36e-09  4.84e-08  0.15
  cql-B1-m2                         lse       9.54e-07   9.54e-07  1.39e-05  0.07
  cql-B1-m2-sums                    td        1.75e-06   1.75e-06  1.59e-05  0.11
  cql-B5-m64                        dq2       3.37e-07   3.37e-07  1.35e-06  0.25
  cql-B5-m64-sums                   td        4.27e-06   4.53e-07  2.39e-05  0.18
  cql-B5-m65                        dq1       5.94e-07   5.94e-07  2.38e-06  0.25
  cql-B5-m65-sums                   q0        3.58e-07   1.19e-07  2.98e-06  0.12
  cql-B5-m66                        td        2.03e-05   5.01e-06  8.06e-05  0.25
  cql-B5-m66-sums                   q0        4.77e-07   4.77e-07  3.96e-06  0.12
  cql-B300-m31                      dq2       1.18e-08   1.18e-08  4.70e-08  0.25
  cql-B300-m31-sums                 td        1.91e-04   1.91e-04  1.45e-03  0.13
  cql-B257-m130                     dq2       1.29e-08   1.29e-08  5.17e-08  0.25
  cql-B257-m130-sums                q0        5.02e-06   8.83e-06  3.53e-05  0.14
  cql-B5-m66-overflow               dq1       4.04e-07   3.75e-07  1.52e-06  0.27
  cql-B5-m66-overflow-sums          td        5.13e-06   2.49e-06  3.57e-05  0.14
  the project's fixed bars (forward 2e-4, gradients 2e-3 of the largest entry), worst of the forms:
  10x5x3-none-N5 (3 forms)          out       3.66e-08          -  2.00e-04  0.0002
  59x5x1-none-N1 (3 forms)          fc1_b     4.10e-08          -  1.71e-04  0.0002
  60x5x7-tanh-N9 (3 forms)          out       5.01e-08          -  2.00e-04  0.0003
  37x0x33-relu-N6 (3 forms)         out       5.90e-08          -  2.00e-04  0.0003
  40x64x64-sigmoid-N12 (3 forms)    out       5.49e-08          -  2.00e-04  0.0003
  40x33x2-elu-N11 (3 forms)         out       4.77e-08          -  2.00e-04  0.0002
  266x32x1-none-N1 (3 forms)        fc2_w     1.86e-08          -  1.21e-04  0.0002
  266x32x1-none-N3 (3 forms)        fc2_w     8.05e-08          -  3.01e-04  0.0003
  266x32x1-none-N1024 (3 forms)     out       1.00e-07          -  2.00e-04  0.0005
  266x32x1-none-N1025 (3 forms)     out       9.77e-08          -  2.00e-04  0.0005
  266x32x1-none-N2048 (3 forms)     dact      2.82e-05          -  1.30e-04  0.2169
  266x32x1-none-N2049 (3 forms)     out       8.67e-08          -  2.00e-04  0.0004
  266x32x32-tanh-N1025 (3 forms)    out       1.17e-07          -  2.00e-04  0.0006
  multi-network launches (3)        out       6.61e-08          -  2.00e-04  0.0003
  stale-transpose sequences (12)    out       2.54e-07          -  2.00e-04  0.0013

Two figures need a sentence.
  * 4064x32x1 rows8, forward: with the first layer added as two chains of 2048 products per lane (P = 4 / MTW = 2) the 8-row form
    measured 2.08e-07 here, 1.16 x this bar - rounding, not a wrong term (its gradients were at 0.4 of their bars), but twice the
    4-row form's chain at the longest sum the fused forms take.  k_amlp_fwd4<2> now adds its first layer in blocks of 512 k
    (amlp_fused.hpp: L1_BLOCK) and measures 3.00e-08; KX <= 512 is one block and the same operations as before.
  * 266x32x1 N = 2048, rows4 and per-layer: fc1_b 4.89e-04, fc1_w 1.33e-03 (= 2.72 x that), dact 2.82e-05 where every other case
    is at 1e-6 of its scale: 0.22 of the gradient bar.  Hidden unit 213 of row 178 has a float64 first-layer pre-activation of
    -1.7e-08; two of the three forwards round it to the other side of zero, its ReLU mask opens, and d_h1 there is 4.887e-04 in
    float64 - exactly the three figures.  A kink of the function under test, not an error of a kernel; the 8-row form rounds it
    like float64 and shows 4e-07.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conti_ref as R          # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def _dev(x, dtype=np.float32):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype)).cuda()


class _Report(object):
    """prints every figure of a case before anything is asserted"""

    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def fixed(self, what, got, want, bar_of_scale):
        e, s = R.err_scale(got, want)
        b = bar_of_scale(s)
        print('%-34s %-8s device %.2e  bar %.2e (scale %.2e)' % (self.tag, what, e, b, s))
        if not e <= b:
            self.bad.append((what, e, b))

    def yard(self, what, got, want, yardstick):
        e, s = R.err_scale(got, want)
        b = R.bar(yardstick[0], s)
        print('%-34s %-8s device %.2e  yardstick %.2e  bar %.2e (scale %.2e)' % (self.tag, what, e, yardstick[0], b, s))
        if not e <= b:
            self.bad.append((what, e, b))

    def done(self):
        assert not self.bad, (self.tag, self.bad)


@pytest.fixture
def amlp_fused():
    """switches the fused minibatch launches of the amlp networks (amlp_fused.hpp) for one test; on again afterwards"""
    from rl4rs_amd import device as Dv
    yield Dv.amlp_set_fused
    Dv.amlp_set_fused(True)


def _net(D, E, K, params, head_act='none', rows=64):
    from rl4rs_amd import device as Dv
    return Dv.DeviceAMLP(D, E, K, params, head_act=head_act, max_rows=rows, max_grad_rows=rows)


# ---- A1: the fused forward / backward at other shapes ---------------------------------------------------------------------------
@pytest.mark.parametrize('fused', [True, 2, False], ids=['rows4', 'rows8', 'per-layer'])
@pytest.mark.parametrize('case', R.AMLP_CASES, ids=R.amlp_id)
def test_amlp_forward_and_gradients_at_other_shapes(amlp_fused, case, fused):
    import torch
    D, E, K, head_act, N = case
    c = R.amlp_case(case)
    ref, yard, wide = c['ref'], c['yard'], R.amlp_wide(case)
    amlp_fused(fused)
    dev = _net(D, E, K, c['params'], head_act, rows=N)
    rep = _Report('%s %s' % (R.amlp_id(case), {True: 'rows4', 2: 'rows8', False: 'per-layer'}[fused]))
    xd, ad, dpre = _dev(c['x']), _dev(c['a']), _dev(c['dpre'])
    out = dev.forward(xd, ad)
    dact = dev.backward(xd, ad, dpre, want_dact=bool(E))          # (dpre: the gradient wrt the head's PRE-activation, from the oracle's output)
    g = dev.gradients()
    got = dict((k, v.cpu().numpy()) for k, v in g.items())
    got['out'] = out.cpu().numpy()
    want = dict(ref['grads'], out=ref['out'])
    if E:
        got['dact'], want['dact'] = dact.cpu().numpy(), ref['dact']
    for k in ('out', 'fc1_w', 'fc1_b', 'fc2_w', 'fc2_b', 'head_w', 'head_b') + (('dact',) if E else ()):
        if wide:
            rep.yard(k, got[k], want[k], yard[k])
        elif k == 'out':
            rep.fixed(k, got[k], want[k], lambda s: 2e-4 * max(1.0, s))
        else:
            rep.fixed(k, got[k], want[k], lambda s: 2e-3 * max(s, 1e-12))
    # input gradient only: the parameter gradients in the handle stay as they are, bit for bit
    before = dev.flat_gradient().clone()
    dev.forward(xd, ad)
    dev.backward(xd, ad, (dpre * 2).contiguous(), want_dact=bool(E), want_param_grad=False)
    same = torch.equal(before, dev.flat_gradient())
    dev.close()
    rep.done()
    assert same


# ---- A2: several networks in one launch -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('E,Ks', [(5, (1, 33, 64)), (5, (1, 2, 3, 64)), (0, (1, 2, 3, 64))], ids=['three', 'four-16-problems', 'four-no-action'])
def test_networks_of_different_head_widths_in_one_launch_equal_single_calls(amlp_fused, E, Ks):
    """rl4rs_amlp_forward_multi / _backward_multi with up to 4 networks whose head widths differ (four with an action input fill
    TnGroup to its 16 problems) == one call per network on twin handles, bit for bit; one of them against float64 as well (two
    equal wrong answers would pass the first)"""
    import torch
    from rl4rs_amd import device as Dv
    amlp_fused(True)
    D, N = 40, 11
    rs = np.random.RandomState(40 + len(Ks) + E)
    x, a, _ = R.amlp_inputs(D, E, 1, N, 41)
    xd, ad = _dev(x), _dev(a)
    params = [R.amlp_params(D, E, K, 50 + i) for i, K in enumerate(Ks)]
    group = [_net(D, E, K, p) for K, p in zip(Ks, params)]
    solo = [_net(D, E, K, p) for K, p in zip(Ks, params)]
    ws = [rs.standard_normal((N, K)).astype(np.float32) for K in Ks]
    douts = [_dev(w) for w in ws]
    outs = Dv.amlp_forward_multi(group, xd, ad)
    dacts = Dv.amlp_backward_multi(group, xd, ad, douts, want_dact=bool(E))
    for i, (net, o, d) in enumerate(zip(solo, outs, douts)):
        assert torch.equal(net.forward(xd, ad), o), i
        da = net.backward(xd, ad, d, want_dact=bool(E))
        if E:
            assert torch.equal(da, dacts[i]), i
    for i, (p, q) in enumerate(zip(group, solo)):
        assert torch.equal(p.flat_gradient(), q.flat_gradient()), i
    # the last network (K = 64) against float64
    i = len(Ks) - 1
    ref = R.amlp_eval(params[i], 'none', x, a, ws[i], torch.float64)
    rep = _Report('multi E=%d K=%s net %d' % (E, Ks, i))
    rep.fixed('out', outs[i].cpu().numpy(), ref['out'], lambda s: 2e-4 * max(1.0, s))
    for k, v in group[i].gradients().items():
        rep.fixed(k, v.cpu().numpy(), ref['grads'][k], lambda s: 2e-3 * max(s, 1e-12))
    if E:
        rep.fixed('dact', dacts[i].cpu().numpy(), ref['dact'], lambda s: 2e-3 * max(s, 1e-12))
    for net in group + solo:
        net.close()
    rep.done()


# ---- A3: stale transposed weights -----------------------------------------------------------------------------------------------
def _write_set_params(dev, other, rs):
    dev.set_flat_params(other.flat_params())


def _write_adam_step(dev, other, rs):
    dev.set_flat_gradient(_dev(rs.standard_normal(dev.n_params)))
    dev.adam_step(0.25)                      # (the first Adam step moves every parameter by +-lr: several times a weight's size)


def _write_copy_from(dev, other, rs):
    dev.copy_from(other)


def _write_soft_update(dev, other, rs):
    dev.soft_update_from(other, 0.5)


def _write_adam_multi_stepped(dev, other, rs):
    from rl4rs_amd import device as Dv
    dev.set_flat_gradient(_dev(rs.standard_normal(dev.n_params)))
    Dv.amlp_adam_multi([dev], [0.25])


def _write_adam_multi_target(dev, other, rs):
    from rl4rs_amd import device as Dv
    Dv.amlp_adam_multi([other], [0.0], targets=[dev], tau=0.5, step=[False])


_WRITES = [_write_set_params, _write_adam_step, _write_copy_from, _write_soft_update, _write_adam_multi_stepped, _write_adam_multi_target]


@pytest.mark.parametrize('toggle', [True, False], ids=['unfused-forward-between', 'plain'])
@pytest.mark.parametrize('write', _WRITES, ids=lambda f: f.__name__[len('_write_'):])
def test_backward_after_a_parameter_write_reads_fresh_transposes(amlp_fused, write, toggle):
    """The fused backward reads W2^T, W3^T, W1_action^T, which the fused FORWARD rebuilds; `t_valid` makes the backward rebuild them
    when the last forward was not the fused one or the parameters were written since.  Sequence: fused forward under P0 (builds
    the transposes of P0), a parameter write, then (toggle) a per-layer forward followed by the FUSED backward - whose only way
    to fresh transposes is that flag - or (plain) a fused forward and backward.  P0 and the written parameters are unrelated, so
    a backward through P0's transposes is wrong by O(1) (tests/test_conti_shapes_host.py)."""
    import torch
    D, E, K, N = 266, 32, 1, 36
    P0, P1 = R.stale_pair()
    x, a, w = R.amlp_inputs(D, E, K, N, 78)
    xd, ad, wd = _dev(x), _dev(a), _dev(w)
    dev, other = _net(D, E, K, P0), _net(D, E, K, P1)
    rs = np.random.RandomState(79)
    amlp_fused(True)
    dev.forward(xd, ad)
    write(dev, other, rs)
    # the parameters the handle now holds - read BEFORE the final forward: handing out the parameter pointer (rl4rs_amlp_params,
    # behind flat_params) clears the flag too, and after that forward it would hide a forward that failed to clear it
    now = R.unflat(dev.flat_params().cpu().numpy(), D, E, K)
    assert np.abs(now['fc2_w'] - P0['fc2_w']).max() > 0.05            # the write did change the weights by about their own size
    if toggle:
        amlp_fused(False)
        out = dev.forward(xd, ad)
        amlp_fused(True)
    else:
        out = dev.forward(xd, ad)
    dact = dev.backward(xd, ad, wd, want_dact=True)
    ref = R.amlp_eval(now, 'none', x, a, w, torch.float64)
    rep = _Report('stale %s %s' % (write.__name__[7:], 'toggle' if toggle else 'plain'))
    rep.fixed('out', out.cpu().numpy(), ref['out'], lambda s: 2e-4 * max(1.0, s))
    rep.fixed('dact', dact.cpu().numpy(), ref['dact'], lambda s: 2e-3 * max(s, 1e-12))
    for k, v in dev.gradients().items():
        rep.fixed(k, v.cpu().numpy(), ref['grads'][k], lambda s: 2e-3 * max(s, 1e-12))
    dev.close()
    other.close()
    rep.done()


# ---- A5: the loss kernels past one wave trip and one block ----------------------------------------------------------------------
@pytest.mark.parametrize('case', R.CVAE_CASES, ids=lambda c: 'N%d-E%d-L%d-beta%g' % c)
def test_cvae_sample_loss_and_encoder_gradient(case):
    from rl4rs_amd import device as Dv
    N, E, L, beta = case
    c = R.cvae_inputs(*case)
    args = (c['enc'], c['eps'], c['y'], c['a'], c['dz'], beta)
    want, inside = R.cvae(*args, F64)
    f32 = R.cvae(*args, F32)[0]
    enc, eps = _dev(c['enc']), _dev(c['eps'])
    z = Dv.cvae_sample(enc, eps)
    loss2, d_dec = Dv.cvae_loss(_dev(c['y']), _dev(c['a']), enc)
    d_enc = Dv.cvae_encoder_grad(enc, eps, _dev(c['dz']), beta).cpu().numpy()
    got = dict(z=z.cpu().numpy(), mse=loss2[:1].cpu().numpy(), kl=loss2[1:].cpu().numpy(), d_dec=d_dec.cpu().numpy(), d_enc=d_enc)
    rep = _Report('cvae-N%d-E%d-L%d-beta%g' % case)
    for k in ('z', 'mse', 'kl', 'd_dec', 'd_enc'):
        rep.yard(k, got[k], want[k], R.err_scale(f32[k], want[k]))
    rep.done()
    assert (d_enc[:, L:][~inside] == 0).all() and (d_enc[:, L:][inside] != 0).all()       # the clamp blocks the gradient: exactly zero


@pytest.mark.parametrize('case', R.BCQ_TARGET_CASES, ids=lambda c: 'B%d-n%d-lam%g-%s' % (c[0], c[1], c[2], 'twin' if c[3] else 'single'))
def test_bcq_target_takes_the_first_maximum_across_lanes_and_trips(case):
    """exact: the inputs make the mix, the maximum and y representable (tests/test_conti_shapes_host.py), and every row's maximum
    is planted twice in an order the cross-lane merge could get wrong"""
    from rl4rs_amd import device as Dv
    B, n, lam, twin = case
    c = R.bcq_target_inputs(*case)
    v32, best, y = R.bcq_target(c, F32)
    got_y, got_best = Dv.bcq_target(_dev(c['q1']), _dev(c['q2']), n, lam, _dev(c['rew']), _dev(c['ter']), R.GAMMA, want_best=True)
    print('bcq_target B%d n%d: patterns %s, best %s' % (B, n, c['pattern'], got_best.cpu().tolist()))
    assert np.array_equal(got_best.cpu().numpy(), best)
    assert np.array_equal(got_y.cpu().numpy(), y)
    # without rewards: the value itself
    v, _ = Dv.bcq_target(_dev(c['q1']), _dev(c['q2']), n, lam)
    assert np.array_equal(v.cpu().numpy(), v32[np.arange(B), best])


def test_pick_rows_of_the_best_samples():
    from rl4rs_amd import device as Dv
    B, n, E = 5, 65, 5
    c = R.bcq_target_inputs(B, n, 0.75, True)
    _, best = Dv.bcq_target(_dev(c['q1']), _dev(c['q2']), n, 0.75, want_best=True)
    assert np.array_equal(best.cpu().numpy(), R.bcq_target(c, F32)[1])
    rows = np.random.RandomState(3).standard_normal((B * n, E)).astype(np.float32)
    got = Dv.pick_rows(_dev(rows), best, n).cpu().numpy()
    assert np.array_equal(got, rows.reshape(B, n, E)[np.arange(B), best.cpu().numpy()])


@pytest.mark.parametrize('N', R.CRITIC_MSE_N)
def test_critic_mse(N):
    from rl4rs_amd import device as Dv
    c = R.critic_mse_inputs(N)
    want, f32 = R.critic_mse(c['q1'], c['q2'], c['y'], F64), R.critic_mse(c['q1'], c['q2'], c['y'], F32)
    loss2, dq1, dq2 = Dv.critic_mse(_dev(c['q1']), _dev(c['q2']), _dev(c['y']))
    rep = _Report('critic_mse-N%d' % N)
    for k, v in (('loss2', loss2), ('dq1', dq1), ('dq2', dq2)):
        rep.yard(k, v.cpu().numpy(), want[k], R.err_scale(f32[k], want[k]))
    rep.done()


@pytest.mark.parametrize('A', R.SQUASHED_A)
def test_squashed_sample_and_log_prob(A):
    import torch
    from rl4rs_amd import device as Dv
    B = R.SQUASHED_B
    rep_ = _Report('squashed-A%d' % A)
    for rep in (1, 3):
        c = R.squashed_inputs(A, rep)
        want, f32 = R.squashed(c['head'], c['eps'], rep, F64), R.squashed(c['head'], c['eps'], rep, F32)
        act, logp = Dv.squashed_sample(_dev(c['head']), _dev(c['eps']), rep=rep)
        rep_.tag = 'squashed-A%d-rep%d' % (A, rep)
        rep_.yard('act', act.cpu().numpy(), want['act'], R.err_scale(f32['act'], want['act']))
        rep_.yard('logp', logp.cpu().numpy(), want['logp'], R.err_scale(f32['logp'], want['logp']))
    # destination layout (rep = 3 into rows of 7 at offset 3): the sample groups side by side, untouched columns stay as they were
    acts = torch.full((B, 7, A), 9.0, device='cuda')
    lps = torch.full((B, 7), 9.0, device='cuda')
    Dv.squashed_sample(_dev(c['head']), _dev(c['eps']), rep=3, act_out=acts.view(-1, A), logp_out=lps.view(-1), out_rep=7, out_off=3)
    rep_.tag = 'squashed-A%d-rep3-strided' % A
    rep_.yard('act', acts[:, 3:6].reshape(-1, A).cpu().numpy(), want['act'], R.err_scale(f32['act'], want['act']))
    rep_.yard('logp', lps[:, 3:6].reshape(-1).cpu().numpy(), want['logp'], R.err_scale(f32['logp'], want['logp']))
    untouched = bool((acts[:, :3] == 9).all() and (acts[:, 6:] == 9).all() and (lps[:, :3] == 9).all() and (lps[:, 6:] == 9).all())
    # the deterministic head
    want, f32 = R.squashed(c['head'], None, 1, F64), R.squashed(c['head'], None, 1, F32)
    act, logp = Dv.squashed_sample(_dev(c['head']), None)
    rep_.tag = 'squashed-A%d-mean' % A
    rep_.yard('act', act.cpu().numpy(), want['act'], R.err_scale(f32['act'], want['act']))
    rep_.done()
    assert untouched and logp is None


@pytest.mark.parametrize('B,A', R.SAC_CASES)
def test_sac_actor_grad(B, A):
    import torch
    from rl4rs_amd import device as Dv
    c = R.sac_inputs(B, A)
    args = (c['head'], c['eps'], c['act'], c['g_a'], c['log_temp'])
    want, inside = R.sac_actor_grad(*args, F64)
    f32 = R.sac_actor_grad(*args, F32)[0]
    got = Dv.sac_actor_grad(_dev(c['head']), _dev(c['eps']), _dev(c['act']), _dev(c['g_a']),
                            torch.tensor([c['log_temp']], dtype=torch.float32, device='cuda')).cpu().numpy()
    rep = _Report('sac_actor_grad-B%d-A%d' % (B, A))
    rep.yard('d_head', got, want['d_head'], R.err_scale(f32['d_head'], want['d_head']))
    rep.done()
    assert (~inside).any() and (got[:, A:][~inside] == 0).all() and (got[:, A:][inside] != 0).all()


@pytest.mark.parametrize('B', [1, 257])
def test_twin_min_and_its_selectors_with_exact_ties(B):
    from rl4rs_amd import device as Dv
    q1, q2, tied = R.twin_min_inputs(B)
    qmin, d1, d2 = R.twin_min(q1, q2)
    g, g1, g2 = Dv.twin_min(_dev(q1), _dev(q2), want_grad=True)
    assert np.array_equal(g.cpu().numpy(), qmin) and np.array_equal(g1.cpu().numpy(), d1) and np.array_equal(g2.cpu().numpy(), d2)
    assert (g1.cpu().numpy()[tied] != 0).all()                          # ties select q1
    g, g1, g2 = Dv.twin_min(_dev(q1), _dev(q2))
    assert np.array_equal(g.cpu().numpy(), qmin) and g1 is None and g2 is None


@pytest.mark.parametrize('case', R.CQL_CASES, ids=lambda c: 'B%d-m%d%s' % (c[0], c[1], '-overflow' if c[2] else ''))
def test_cql_critic_loss(case):
    import torch
    from rl4rs_amd import device as Dv
    B, m, overflow = case
    c = R.cql_inputs(*case)
    q1, q2, offs = _dev(c['q1']), _dev(c['q2']), _dev(c['offs'])
    for with_y in (True, False):
        args = (c['q1'], c['q2'], c['offs'], m, c['y'] if with_y else None, c['aw'] if with_y else None)
        want, f32 = R.cql_critic(*args, F64), R.cql_critic(*args, F32)
        if with_y:
            sums, dq1, dq2 = Dv.cql_critic_loss(q1, q2, offs, m, y=_dev(c['y']), alpha_w=torch.tensor([c['aw']], dtype=torch.float32, device='cuda'))
        else:
            sums, dq1, dq2 = Dv.cql_critic_loss(q1, q2, offs, m)
            assert dq1 is None and dq2 is None
        sums = sums.cpu().numpy()
        got = dict(td=sums[0:2], lse=sums[2:4], q0=sums[4:6])
        if with_y:
            got.update(dq1=dq1.cpu().numpy(), dq2=dq2.cpu().numpy())
        rep = _Report(R.cql_id(case, with_y))
        for k in got:
            assert np.isfinite(got[k]).all(), (k, got[k])
            rep.yard(k, got[k], want[k], R.err_scale(f32[k], want[k]))
        rep.done()
