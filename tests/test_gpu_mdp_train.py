"""GPU: the training pass of the MDP checker's seq2seq transformer (rl4rs_seq2seq_loss_grad, rl4rs_seq2seq_adam_step) against
autograd of the float64 restatement tests/mdp_ref.py with the library's dropout masks reproduced, and a float64 Keras-form Adam.

Bars: 4 x the float32 error of the restatement itself at these inputs (mdp_ref.LOSS_REL_BAR / GRAD_BAR, `python tests/mdp_ref.py`
on a CPU); a gradient tensor is measured by mdp_ref.grad_errors."""
import numpy as np
import pytest
import torch

import mdp_ref

pytestmark = pytest.mark.gpu
DROP = (0.05, 7, 3)


def _net(V, d, h, flat, S, L, N):
    from rl4rs_amd.device import DeviceSeq2Seq
    return DeviceSeq2Seq(V, d, h, S, L, N * max(S, L), flat)


@pytest.fixture(scope='module')
def refs():
    """(loss, gradient) of the restatement per (case, dropout), computed once"""
    out = {}
    for i in (0, 1):
        V, d, h, flat, enc, dec = mdp_ref.forward_case(i)
        for drop in (None, DROP):
            out[i, drop] = mdp_ref.RefSeq2Seq(V, d, h, flat).loss_and_grad(enc, dec, mdp_ref.train_targets(i), drop)
    return out


def _check_grad(got, want, V, d, h):
    err = mdp_ref.grad_errors(got, want, V, d, h)
    worst = max(err, key=err.get)
    print('worst tensor %s %.3g (bar %.3g)' % (worst, err[worst], mdp_ref.GRAD_BAR[d]))
    bad = {k: v for k, v in err.items() if not v <= mdp_ref.GRAD_BAR[d]}
    assert not bad, bad


@pytest.mark.parametrize('drop', [None, DROP], ids=['dropout0', 'dropout0.05'])
@pytest.mark.parametrize('i', [0, 1])
def test_loss_and_every_gradient_against_autograd(i, drop, refs):
    N, S, L, V, d, h = mdp_ref.FORWARD_CASES[i]
    _, _, _, flat, enc, dec = mdp_ref.forward_case(i)
    net = _net(V, d, h, flat, S, L, N)
    rate, seed, step = drop or (0.0, 0, 0)
    loss = float(net.loss_grad(enc, dec, mdp_ref.train_targets(i), rate, seed, step).cpu())
    want_loss, want = refs[i, drop]
    print('loss %.8g want %.8g rel %.3g (bar %.3g)' % (loss, want_loss, abs(loss - want_loss) / want_loss, mdp_ref.LOSS_REL_BAR[d]))
    _check_grad(net.grad().cpu().numpy().astype(np.float64), want, V, d, h)
    assert abs(loss - want_loss) / want_loss <= mdp_ref.LOSS_REL_BAR[d]


def test_table_gradients_when_one_token_repeats_in_many_rows():
    N, S, L, V, d, h = 40, 18, 7, 37, 64, 48
    rs = np.random.RandomState(9)
    flat = mdp_ref.random_params(V, d, h, 4)
    enc = rs.randint(1, V, size=(N, S)).astype(np.int32)
    dec = rs.randint(1, V, size=(N, L)).astype(np.int32)
    out = rs.randint(1, V, size=(N, L)).astype(np.int32)
    enc[:, 3], enc[::2, 9], dec[:, 2], dec[::3, 4], out[:, 1] = 7, 7, 7, 7, 7          # token 7: 60 source and 54 target positions
    net = _net(V, d, h, flat, S, L, N)
    net.loss_grad(enc, dec, out, 0.0)
    _, want = mdp_ref.RefSeq2Seq(V, d, h, flat).loss_and_grad(enc, dec, out)
    got = net.grad().cpu().numpy().astype(np.float64)
    err = mdp_ref.grad_errors(got, want, V, d, h)
    print('E_enc %.3g E_dec %.3g' % (err['E_enc'], err['E_dec']))
    assert err['E_enc'] <= mdp_ref.GRAD_BAR[d] and err['E_dec'] <= mdp_ref.GRAD_BAR[d]
    # the rows of token 7 themselves, against their own size
    for k, o in (('E_enc', 0), ('E_dec', V * d)):
        a, b = got[o + 7 * d:o + 8 * d], want[o + 7 * d:o + 8 * d]
        assert np.abs(a - b).max() / np.abs(b).max() <= mdp_ref.GRAD_BAR[d], k
    # a token the batch never holds has no embedding gradient in the encoder table
    absent = [v for v in range(V) if not (enc == v).any()]
    assert all(not got[v * d:(v + 1) * d].any() for v in absent)


def test_two_identical_calls_give_identical_bits():
    N, S, L, V, d, h = mdp_ref.FORWARD_CASES[0]
    _, _, _, flat, enc, dec = mdp_ref.forward_case(0)
    net = _net(V, d, h, flat, S, L, N)
    out = mdp_ref.train_targets(0)
    l1 = net.loss_grad(enc, dec, out, *DROP).cpu().numpy().copy()
    g1 = net.grad().cpu().numpy().copy()
    net.grad().fill_(123.0)
    l2 = net.loss_grad(enc, dec, out, *DROP).cpu().numpy()
    assert np.array_equal(l1, l2) and np.array_equal(g1, net.grad().cpu().numpy())
    other = net.loss_grad(enc, dec, out, DROP[0], DROP[1], DROP[2] + 1).cpu().numpy()
    assert not np.array_equal(l1, other)                         # another step draws other masks


def test_three_adam_steps_against_float64_keras_adam():
    """mdp_ref.adam_check: the parameters after three loss_grad + adam_step against the float64 Keras Adam on the restatement's
    gradients, on the elements whose gradient is not within rounding of zero (there the +-lr move's direction is rounding).  Bar:
    mdp_ref.ADAM_BAR = 4 x what a float32 Adam on the float32 restatement differs by (1.69e-7).  Measured on the device: 1.63e-7."""
    def on_device(V, d, h, flat, enc, dec, out, steps):
        N, S, L = enc.shape[0], enc.shape[1], dec.shape[1]
        net = _net(V, d, h, flat, S, L, N)
        for _ in range(steps):
            net.loss_grad(enc, dec, out, 0.0)
            net.adam_step()
        assert net.adam_state()[2] == steps
        return net.params().cpu().numpy()
    err = mdp_ref.adam_check(on_device)
    print('adam: max error on firm elements %.3g (bar %.3g)' % (err, mdp_ref.ADAM_BAR))
    assert err <= mdp_ref.ADAM_BAR


def test_fit_learns_the_synthetic_mdp_as_the_restatement_does():
    """V = 40, target token j = (last source item + j) mod 37 + 3, 2048 samples, d = 64: after the LEARN_EPOCHS epochs at which the
    restatement (trained on a CPU from the same parameters, batches and masks) first decodes >= 95 % of the 512 held-out targets
    exactly, the device model reaches the restatement's rate minus two standard errors of a proportion at 512 samples.
    Measured: 0.9961 against the restatement's 0.9883 (floor 0.9788)."""
    from rl4rs_amd.mdpchecker import Seq2SeqTransformer, beam_search
    c = mdp_ref.LEARN
    enc, dec_in, dec_out, tgt = mdp_ref.learn_data()
    n = c['train']
    m = Seq2SeqTransformer(token_num=c['V'], embed_dim=c['d'], hidden_dim=c['h'], dropout_rate=c['rate'], seed=c['seed'])
    history = m.fit([enc[:n], dec_in[:n]], dec_out[:n, :, None], epochs=mdp_ref.LEARN_EPOCHS, batch_size=c['batch'])
    assert len(history) == mdp_ref.LEARN_EPOCHS and history[-1] < 0.5 * history[0]
    greedy, _ = beam_search(m, enc[n:], 1, c['T'])
    rate = float((greedy[:, 0, 1:] == tgt[n:]).all(axis=1).mean())
    p = mdp_ref.LEARN_RATE
    floor = p - 2 * np.sqrt(p * (1 - p) / c['held'])
    print('exact-match %.4f (restatement %.4f, floor %.4f); loss %.4f -> %.4f' % (rate, p, floor, history[0], history[-1]))
    assert rate >= floor
    # beam 0 of a width-4 search is the greedy decode - except where the search finds a likelier sequence than greedy does, which
    # a correct search must return instead (greedy's own path is then still among the beams or was beaten by four better ones).
    # Every difference is checked to be that case with the float64 restatement on the trained weights: a strictly larger product.
    wide, wide_score = beam_search(m, enc[n:], 4, c['T'])
    _, greedy_score = beam_search(m, enc[n:], 1, c['T'])
    differ = np.flatnonzero((wide[:, 0] != greedy[:, 0]).any(axis=1))
    print('beam 0 differs from greedy for %d of %d users' % (len(differ), c['held']))
    same = np.setdiff1d(np.arange(c['held']), differ)
    assert np.array_equal(wide_score[same, 0], greedy_score[same, 0])
    if len(differ):
        ref = mdp_ref.RefSeq2Seq(c['V'], c['d'], c['h'], m.params)

        def product(paths):
            pr = ref.predict([enc[n:][differ], paths[:, :-1]])
            return np.take_along_axis(pr, paths[:, 1:, None], axis=2)[:, :, 0].prod(axis=1)
        assert (product(wide[differ, 0]) > product(greedy[differ, 0])).all()
        assert (wide_score[differ, 0] > greedy_score[differ, 0]).all()


def test_weights_file_carries_the_adam_state(tmp_path):
    from rl4rs_amd.mdpchecker import Seq2SeqTransformer
    c = mdp_ref.LEARN
    enc, dec_in, dec_out, _ = mdp_ref.learn_data()
    kw = dict(token_num=c['V'], embed_dim=c['d'], hidden_dim=c['h'], dropout_rate=c['rate'], seed=c['seed'])
    a = Seq2SeqTransformer(**kw)
    a.fit([enc[:512], dec_in[:512]], dec_out[:512], epochs=1, batch_size=256)
    path = str(tmp_path / 'w.npz')
    a.save_weights(path)
    b = Seq2SeqTransformer(**kw)
    b.load_weights(path)
    b._epochs = a._epochs
    assert b._adam[2] == 2 and np.array_equal(b._adam[0], a._adam[0])
    ha = a.fit([enc[:512], dec_in[:512]], dec_out[:512], epochs=1, batch_size=256)
    hb = b.fit([enc[:512], dec_in[:512]], dec_out[:512], epochs=1, batch_size=256)
    assert ha == hb and np.array_equal(a.params, b.params)      # the loaded model goes on exactly where the saved one does

