"""The slate-wise heads of the simulator trainers (rl4rs_simtrain_create_head / rl4rs_dientrain_create_head: Dense(9, sigmoid) +
binary_crossentropy, Dense(22, softmax) + categorical crossentropy of the slate class, the adversarial model) and the inference
pass rl4rs_*train_eval, against torch float64 autograd of tests/slate_ref.py.
Bars as in tests/test_gpu_simtrain.py: loss 1e-5 relative, every gradient array within 2e-4 (dnn / widedeep / lstm / adversarial) or
5e-4 (dien) of its largest entry; evaluate's probabilities within the scorer bar, 5e-6 absolute."""
import ctypes as C

import numpy as np
import pytest

import slate_ref
from test_gpu_simtrain import CFG, DIEN_CFG
from test_gpu_simtrain_shapes import DIEN_VARIANTS, ODD

pytestmark = pytest.mark.gpu

ADV = 'adversarial_slate'
MODELS = [(a, h) for a in ('dnn', 'widedeep', 'lstm', 'dien') for h in ('slate', 'multiclass')] + [(ADV, 'adversarial')]


def _cfg(algo, small):
    if small:
        return DIEN_VARIANTS['D1'] if algo == 'dien' else ODD
    return DIEN_CFG if algo == 'dien' else CFG


def _weights(cfg, algo, head, seed=3):
    if algo == 'dien':
        from rl4rs_amd.nets.dien import init_dien_weights
        return init_dien_weights(cfg, seed=seed, emb_scale=0.5, bias_noise=0.2, head=head)
    from rl4rs_amd.nets.simnets import init_simnet_weights
    return init_simnet_weights(cfg, algo, seed=seed, emb_scale=0.5, bias_noise=0.2, head=head)


def _trainer(cfg, algo, head, w, N):
    from rl4rs_amd.device import DeviceDienTrainer, DeviceSimTrainer
    if algo == 'dien':
        return DeviceDienTrainer(cfg, w, max_batch=N, head=head)
    return DeviceSimTrainer(cfg, w, max_batch=N, algo=algo, head=head)


def _batch(cfg, N, head, seed, distinct_cat=False):
    """dense, cat, labels, seqs; slate labels [N, 9] whose first row is all zero and whose last row is all one (classes 0 and 21).
    Every other row of sequence input 1 is all padding - from row 1 on when N = 1, so that the single row keeps a history in every
    input: with input 1 all padding its 64 steps are identical and DIEN's d loss / d att1_b3, a single number, is a cancelling sum
    3 000 times smaller than its neighbour att0_b3 (5.1e-6 against 1.7e-2, dien_slate_multiclass at the default configuration).
    The float32 kernels then miss it by 4.7e-8 - 2.7e-6 of att0_b3, ordinary float32 accuracy, but 9e-3 of the entry itself, and
    "5e-4 of the array's largest entry" has nothing else in a one-element array to be measured against.  The all-padding rows
    are covered at N = 43."""
    rs = np.random.RandomState(seed)
    L, S, Cn = cfg['maxlen'], cfg['seq_num'], cfg['category_feature_num']
    dense = np.abs(rs.randn(N, cfg['dense_feature_num'])).astype(np.float32)
    if distinct_cat:
        cat = rs.permutation(cfg['category_hash_size'])[:N * Cn].reshape(N, Cn).astype(np.int32)
    else:
        cat = rs.randint(0, cfg['category_hash_size'], size=(N, Cn)).astype(np.int32)
        nq = min(11, Cn)
        cat[:, Cn - nq:] = rs.randint(0, 284, size=(N, nq))
    seqs = [rs.randint(0, 284, size=(N, L)).astype(np.int32) for _ in range(S)]
    seqs[0][: N // 3, : min(20, L - 1)] = 0
    if S > 1:
        seqs[1][(1 if N == 1 else 0)::2] = 0
    if head == 'item':
        labels = rs.randint(0, cfg['class_num'], size=N).astype(np.int32)
    else:
        labels = rs.randint(0, 2, size=(N, 9)).astype(np.int32)
        labels[0] = 0
        labels[-1] = 1 if N > 1 else labels[-1]
    return dense, cat, labels, seqs


def _dev(dense, cat, labels, seqs, algo):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t(dense), t(cat), t(labels), ([t(q) for q in seqs] if algo != 'dnn' else None)


def _check_gradients(algo, head, cfg, N, rate, w=None, seed=11):
    w = _weights(cfg, algo, head) if w is None else w
    dense, cat, labels, seqs = _batch(cfg, N, head, seed)
    if head != 'item' and N > 1:
        assert not labels[0].any() and labels[-1].all()
        assert slate_ref.slate_class(labels[[0, -1]]).tolist() == [0, 21]
    tr = _trainer(cfg, algo, head, w, N)
    dd, dc, dl, ds = _dev(dense, cat, labels, seqs, algo)
    loss = float(tr.grad(dd, dc, dl, ds, dropout_rate=rate, seed=5, step=2).item())
    g = dict((k, v.cpu().numpy()) for k, v in tr.gradients().items())
    m1 = m2 = None
    if rate > 0:
        m1, m2 = [m.cpu().numpy().astype(np.float64) for m in tr.masks(N)]
    tr.close()
    ref = slate_ref.forward(algo, head, w, cfg, dense, cat, labels, seqs, m1, m2, rate, want_grad=True)
    print('%s/%s N=%d: loss %.9g (reference %.9g)' % (algo, head, N, loss, ref['loss']))
    assert np.isfinite(loss) and abs(loss - ref['loss']) < 1e-5 * max(1.0, abs(ref['loss']))
    assert set(g) == set(ref['grads']) == set(w)
    bar = 5e-4 if algo == 'dien' else 2e-4
    for k in sorted(g):
        scale = np.abs(ref['grads'][k]).max()
        err = np.abs(g[k] - ref['grads'][k]).max()
        print('  %-18s off by %.3g of its largest entry %.3g' % (k, err / max(scale, 1e-8), scale))
        assert np.isfinite(g[k]).all() and err < bar * max(scale, 1e-8) + 1e-9, (k, err, scale)
    return w


@pytest.mark.parametrize('algo,head', MODELS)
def test_gradients_at_an_odd_configuration(algo, head):
    """N = 43, dropout 0.2 through the device's own masks; ODD / D1: E != U, odd widths, 3 sequence inputs of 33 steps, 13 categories"""
    w = _check_gradients(algo, head, _cfg(algo, True), 43, 0.2)
    obs = {'dnn': 256, 'lstm': 256, 'dien': 256, 'widedeep': 256 + 96 + 13 * 72, ADV: 3 * 72 + 96 + 72}[algo]
    assert w['out_w'].shape == (obs, 22 if head == 'multiclass' else 9)            # whatever class_num (3) says


@pytest.mark.parametrize('algo,head', MODELS)
def test_gradients_of_a_single_row_at_the_default_configuration(algo, head):
    _check_gradients(algo, head, _cfg(algo, False), 1, 0.2)


@pytest.mark.parametrize('algo,head', [('dnn', 'slate'), ('dnn', 'multiclass'), (ADV, 'adversarial')])
def test_extreme_logits_stay_finite_and_exact(algo, head):
    """out_b puts the sigmoid logits at +-40 and spreads the 22 softmax logits over 100: a loss written on clipped probabilities has
    zero gradient / a capped loss here, the logit form stays exact"""
    cfg = ODD
    w = _weights(cfg, algo, head)
    w['out_w'] = (w['out_w'] * 0.01).astype(np.float32)
    if head == 'multiclass':
        w['out_b'] = np.linspace(-50.0, 50.0, 22).astype(np.float32)
    else:
        w['out_b'] = (40.0 * np.asarray([1, -1, 1, -1, 1, -1, 1, -1, 1])).astype(np.float32)
    _check_gradients(algo, head, cfg, 43, 0.0, w=w)


@pytest.mark.parametrize('N', [1, 43])
@pytest.mark.parametrize('algo,head', [('dnn', 'item'), ('dnn', 'slate'), ('dnn', 'multiclass'), ('widedeep', 'item'),
                                       ('lstm', 'multiclass'), ('dien', 'item'), ('dien', 'slate'), (ADV, 'adversarial')])
def test_evaluate(algo, head, N):
    """after one Adam step (non-zero gradient buffer and moments): evaluate's output against the float64 restatement, its mean row loss
    against grad(dropout_rate = 0), and parameters / gradient / moments bitwise as before"""
    import torch
    cfg = _cfg(algo, True)
    w = _weights(cfg, algo, head)
    dense, cat, labels, seqs = _batch(cfg, N, head, 17)
    tr = _trainer(cfg, algo, head, w, N)
    dd, dc, dl, ds = _dev(dense, cat, labels, seqs, algo)
    tr.step(dd, dc, dl, ds, dropout_rate=0.2, seed=3)
    before = [tr.params(), tr.flat_gradient()] + list(tr.adam_state()[:2])
    assert all(float(x.abs().max()) > 0 for x in before) and tr.adam_state()[2] == 1
    pred, rows = tr.evaluate(dd, dc, dl, ds)
    pred_only, none = tr.evaluate(dd, dc, None, ds)
    after = [tr.params(), tr.flat_gradient()] + list(tr.adam_state()[:2])
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    assert none is None and torch.equal(pred, pred_only)
    K = cfg['class_num'] if head == 'item' else (22 if head == 'multiclass' else 9)
    assert pred.shape == (N, K) and rows.shape == (N,)
    trained = dict((k, v.cpu().numpy()) for k, v in tr.weights().items())
    ref = slate_ref.forward(algo, head, trained, cfg, dense, cat, labels, seqs)
    err = np.abs(pred.cpu().numpy() - ref['pred']).max()
    print('%s/%s N=%d: probabilities off by %.3g' % (algo, head, N, err))
    assert err < 5e-6
    assert np.abs(rows.cpu().numpy() - ref['loss_rows']).max() < 1e-5 * max(1.0, np.abs(ref['loss_rows']).max())
    loss = float(tr.grad(dd, dc, dl, ds, dropout_rate=0.0).item())
    mean_rows = float(rows.double().mean().item())
    assert abs(mean_rows - loss) < 1e-6 * max(1.0, abs(loss)), (mean_rows, loss)
    tr.close()


def test_item_head_through_create_head_is_the_existing_create():
    """head = 'item': the gradient of a handle made by rl4rs_simtrain_create_head(.., 0, ..) equals, bit for bit, that of one made by
    rl4rs_simtrain_create.  dnn with all category ids distinct: every element of the embedding gradient then takes exactly one
    atomic add, so the whole flat gradient is reproducible."""
    import torch
    from rl4rs_amd import _lib
    from rl4rs_amd.device import DeviceSimTrainer, _stream
    cfg, N = ODD, 43
    w = _weights(cfg, 'dnn', 'item')
    dense, cat, labels, seqs = _batch(cfg, N, 'item', 23, distinct_cat=True)
    assert len(np.unique(cat)) == cat.size
    dd, dc, dl, _ = _dev(dense, cat, labels, seqs, 'dnn')
    new = DeviceSimTrainer(cfg, w, max_batch=N, algo='dnn', head='item')
    # the same configuration and weights through the existing entry point
    lib = _lib.load()
    c = _lib.SimnetCfg(1, cfg['maxlen'], cfg['emb_size'], cfg['hidden_units'], cfg['dense_feature_num'], cfg['category_feature_num'],
                       cfg['category_hash_size'], cfg['seq_num'], cfg['class_num'], N, 1)
    ws = _lib.SimnetWeights()
    for name, arr in w.items():
        setattr(ws, name, arr.ctypes.data_as(_lib._FP))
    h = C.c_void_p()
    _lib.check(lib.rl4rs_simtrain_create(C.byref(c), C.byref(ws), N, _stream(), C.byref(h)))
    old = DeviceSimTrainer.__new__(DeviceSimTrainer)
    old.__dict__.update(new.__dict__)
    old.h = h
    out = []
    for tr in (new, old):
        loss = tr.grad(dd, dc, dl, None, dropout_rate=0.2, seed=5, step=2)
        out.append((loss.clone(), tr.flat_gradient()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert float(out[0][1].abs().max()) > 0
    old.close()
    new.close()


def test_heads_and_models_that_do_not_go_together_are_refused():
    from rl4rs_amd.device import DeviceDienTrainer, DeviceSimTrainer
    w = _weights(ODD, 'dnn', 'slate')
    with pytest.raises(ValueError, match='come as a pair'):
        DeviceSimTrainer(ODD, w, max_batch=4, algo='dnn', head='adversarial')
    with pytest.raises(ValueError, match='come as a pair'):
        DeviceSimTrainer(ODD, _weights(ODD, ADV, 'adversarial'), max_batch=4, algo=ADV, head='slate')
    with pytest.raises(ValueError, match='come as a pair'):
        DeviceDienTrainer(DIEN_VARIANTS['D1'], _weights(DIEN_VARIANTS['D1'], 'dien', 'slate'), max_batch=4, head='adversarial')
    with pytest.raises(ValueError, match='head must be one of'):
        DeviceSimTrainer(ODD, w, max_batch=4, algo='dnn', head='page')
