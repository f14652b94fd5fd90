"""CPU: the host side of SimulatorTrainer's validation pass - early stopping and the keras-shaped history against a stub trainer
with a scripted val_loss, the thirteen model_type names, and the refusals of the slate-wise types."""
import os
import types

import numpy as np
import pytest
import torch

from rl4rs_amd import metrics as M
from rl4rs_amd.simtrain import MODEL_TYPES, SimulatorTrainer, parse_model_type, run_epochs

CFG = {"maxlen": 4, "batch_size": 8, "class_num": 2, "dense_feature_num": 6, "category_feature_num": 5, "category_hash_size": 50,
       "seq_num": 2, "emb_size": 8, "hidden_units": 8, "page_items": 9}
B = 8


class StubTrainer(object):
    """step() counts; evaluate() returns fixed predictions and row losses equal to the scripted val_loss of the current epoch"""
    device = torch.device('cpu')

    def __init__(self, head, val_losses, validation_steps):
        self.head, self.val_losses, self.vs = head, val_losses, validation_steps
        self.steps = self.evals = 0
        self.seen = []

    def step(self, dense, cat, labels, seqs, lr, dropout_rate, seed):
        self.steps += 1
        return torch.tensor([0.25 * self.steps])

    def evaluate(self, dense, cat, labels, seqs):
        epoch = self.evals // self.vs
        self.evals += 1
        N = dense.shape[0]
        K = {'item': 2, 'multiclass': 22}.get(self.head, 9)
        rs = np.random.RandomState(self.evals)
        pred = torch.from_numpy(rs.rand(N, K).astype(np.float32))
        self.seen.append((pred.numpy().copy(), labels.numpy().copy()))
        return pred, torch.full((N,), float(self.val_losses[epoch]))


def _tfrecord(tmp_path, n=24):
    from rl4rs_amd.utils.datautil import FeatureUtil
    rs = np.random.RandomState(0)
    data = [[0, [rs.randint(1, 50, size=3).tolist(), [0]], rs.rand(6).tolist(), rs.randint(0, 50, size=5).tolist(),
             rs.randint(0, 2, size=9).tolist(), int(rs.randint(0, 2))] for _ in range(n)]
    path = os.path.join(str(tmp_path), 'slate.tfrecord')
    FeatureUtil(CFG).to_tfrecord(data, path)
    return path


def _trainer(model_type, val_losses, vs=2, cfg=CFG):
    head = parse_model_type(model_type)[1]
    stub = StubTrainer(head, val_losses, vs)
    sim = types.SimpleNamespace(config=dict(cfg))
    return SimulatorTrainer(sim, minibatch=B, model_type=model_type, trainer=stub, metrics=M.HostClassifierMetrics()), stub


def test_the_thirteen_model_types():
    assert len(MODEL_TYPES) == 13
    assert parse_model_type('dien') == ('dien', 'item') and parse_model_type('lstm_slate') == ('lstm', 'slate')
    assert parse_model_type('widedeep_slate_multiclass') == ('widedeep', 'multiclass')
    assert parse_model_type('adversarial_slate') == ('adversarial_slate', 'adversarial')
    heads = [parse_model_type(m)[1] for m in MODEL_TYPES]
    assert heads.count('item') == 4 and heads.count('slate') == 4 and heads.count('multiclass') == 4
    with pytest.raises(NotImplementedError):
        parse_model_type('mdpchecker')


def test_stops_after_exactly_patience_epochs_without_a_new_minimum(tmp_path):
    path = _tfrecord(tmp_path)
    #           new min  new min  no       no (equal is not below)  no -> stop     (never run)
    script = [1.0, 0.75, 0.875, 0.75, 0.8125, 0.125, 0.125]          # exact in float32, the row losses' type
    tr, stub = _trainer('dnn_slate', script)
    h = tr.fit_tfrecord(path, steps=3, validation_files=path, validation_steps=2, epochs=7, patience=3)
    assert list(h) == ['loss', 'val_loss', 'val_auc', 'val_precision', 'val_recall']
    assert h['val_loss'] == script[:5] and all(len(v) == 5 for v in h.values())
    assert stub.steps == 5 * 3 and stub.evals == 5 * 2
    # the epoch's loss is the mean of its step losses (keras' running mean over equal batches)
    assert h['loss'] == [0.25 * np.mean([3 * e + 1, 3 * e + 2, 3 * e + 3]) for e in range(5)]
    # patience 1 stops at the first epoch that does not improve; an always improving run uses every epoch
    tr, stub = _trainer('dnn_slate', script)
    assert tr.fit_tfrecord(path, steps=1, validation_files=path, validation_steps=2, epochs=7, patience=1)['val_loss'] == script[:3]
    tr, stub = _trainer('dnn_slate', [5, 4, 3, 2])
    assert tr.fit_tfrecord(path, steps=1, validation_files=path, validation_steps=2, epochs=4, patience=1)['val_loss'] == [5, 4, 3, 2]
    # a NaN val_loss is no new minimum
    tr, stub = _trainer('dnn_slate', [float('nan')] * 4)
    assert len(tr.fit_tfrecord(path, steps=1, validation_files=path, validation_steps=2, epochs=4, patience=2)['val_loss']) == 2


def test_run_epochs_alone():
    seq = iter([3.0, 2.0, 2.5, 1.0, 1.5, 1.2])
    h = run_epochs(lambda e: {'loss': e, 'val_loss': next(seq)}, epochs=6, patience=2)
    assert h == {'loss': [0, 1, 2, 3, 4, 5], 'val_loss': [3.0, 2.0, 2.5, 1.0, 1.5, 1.2]}


@pytest.mark.parametrize('model_type,keys', [
    ('dnn', ['loss', 'val_loss', 'val_auc', 'val_precision', 'val_recall', 'val_acc']),
    ('dien_slate', ['loss', 'val_loss', 'val_auc', 'val_precision', 'val_recall']),
    ('lstm_slate_multiclass', ['loss', 'val_loss', 'val_acc']),
    ('adversarial_slate', ['loss', 'val_loss', 'val_auc', 'val_precision', 'val_recall', 'val_no_click_score'])])
def test_history_keys_and_metrics_by_model_type(tmp_path, model_type, keys):
    path = _tfrecord(tmp_path)
    tr, stub = _trainer(model_type, [1.0, 0.5])
    h = tr.fit_tfrecord(path, steps=2, validation_files=path, validation_steps=2, epochs=2, patience=3)
    assert list(h) == keys and all(len(v) == 2 for v in h.values())
    # the last epoch's metrics, recomputed from what evaluate returned
    pred = np.concatenate([p for p, _ in stub.seen[2:]])
    y = np.concatenate([l for _, l in stub.seen[2:]])
    head = parse_model_type(model_type)[1]
    assert y.shape == ((2 * B,) if head == 'item' else (2 * B, 9))
    if head == 'multiclass':
        cls = y @ np.asarray([1, 2, 4, 1, 2, 4, 1, 2, 4])
        assert h['val_acc'][-1] == np.mean(np.argmax(pred, axis=1) == cls)
    else:
        target = np.eye(2)[y] if head == 'item' else y
        ref = M.metrics_from_counts(M.confusion_counts(pred, target, M.auc_thresholds(200)), 200)
        assert h['val_auc'][-1] == ref['auc'] and h['val_precision'][-1] == ref['precision'] and h['val_recall'][-1] == ref['recall']
        assert 0.0 < ref['auc'] < 1.0
        if head == 'item':
            assert h['val_acc'][-1] == ref['acc'] == np.mean((pred > 0.5) == (target > 0))
        if head == 'adversarial':
            assert abs(h['val_no_click_score'][-1] - np.mean(np.sum(pred.astype(np.float64) * (1 - y), axis=1))) < 1e-12


def test_without_validation_arguments_it_returns_the_step_losses(tmp_path):
    path = _tfrecord(tmp_path)
    tr, stub = _trainer('dnn', [])
    losses = tr.fit_tfrecord(path, 4)
    assert losses == [0.25, 0.5, 0.75, 1.0] and stub.evals == 0
    assert tr.fit_tfrecord(path, steps=2, seed=5) == [1.25, 1.5]
    with pytest.raises(ValueError):
        tr.fit_tfrecord(path, 2, epochs=3)
    with pytest.raises(ValueError):
        tr.fit_tfrecord(path, 2, validation_files=path)


def test_refusals(tmp_path):
    for model_type in MODEL_TYPES:
        tr, stub = _trainer(model_type, [])
        stub.weights = lambda: {}
        if parse_model_type(model_type)[1] != 'item':
            with pytest.raises(NotImplementedError, match='slate-wise'):
                tr.install()
            with pytest.raises(ValueError, match='page_items'):
                _trainer(model_type, [], cfg=dict(CFG, page_items=6))
        else:
            _trainer(model_type, [], cfg=dict(CFG, page_items=6))
    tr, stub = _trainer('adversarial_slate', [])
    stub.weights = lambda: {'out_b': torch.zeros(9)}
    with pytest.raises(NotImplementedError, match='npz only'):
        tr.save(os.path.join(str(tmp_path), 'ckpt', 'model'))
    tr.save(os.path.join(str(tmp_path), 'adv.npz'))
    assert np.load(os.path.join(str(tmp_path), 'adv.npz'))['out_b'].shape == (9,)
    with pytest.raises(NotImplementedError, match='model_type must be one of'):
        SimulatorTrainer(types.SimpleNamespace(config=dict(CFG)), model_type='gbdt_slate', trainer=stub)
