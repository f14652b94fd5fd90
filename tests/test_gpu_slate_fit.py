"""SimulatorTrainer with the slate-wise model types on synthetic logs: the slate sample construction against a host restatement of
data_preprocess.py's feature_construct(is_slate=True), and fit_tfrecord with a validation set - history, falling val_loss, metrics
equal to a numpy recomputation from evaluate's predictions."""
import os

import numpy as np
import pytest

from rl4rs_amd import metrics as M

pytestmark = pytest.mark.gpu

B = 32


def _sim(tmp_path, algo='dnn'):
    from rl4rs_amd import synth
    from rl4rs.env.slate import SlateRecEnv, SlateState
    d = str(tmp_path)
    cat_path, log_path = os.path.join(d, 'item_info.csv'), os.path.join(d, 'log.csv')
    cat_text = synth.make_catalog_text(seed=21)
    synth.write_text(cat_path, cat_text)
    records = synth.make_records(B, pages=1, seed=8, illegal_frac=0.0, hash_size=5000, special_ids=synth.special_ids_from_text(cat_text))
    synth.write_records(log_path, records)
    cfg = {"maxlen": 64, "batch_size": B, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
           "category_feature_num": 21, "category_hash_size": 5000, "seq_num": 2, "emb_size": 128,
           "page_items": 9, "hidden_units": 128, "max_steps": 9, "action_emb_size": 32,
           "sample_file": log_path, "iteminfo_file": cat_path, "is_eval": True, "cache_size": B, "model_seed": 3,
           "algo": algo, "return_tensors": True}
    return SlateRecEnv(cfg, state_cls=SlateState), records, cat_path


def test_slate_samples_are_feature_construct_is_slate(tmp_path):
    """one sample per page record: category = user_cat(10) + [sequence_id] + exposed_items(9), dense = user_dense(32) +
    item_feature(9 x 40), both zero-padded by the reader to 21 / 432; label = user_feedback; sequences = [history, [0]]"""
    from rl4rs_amd.data import CatalogTables
    from rl4rs_amd.simtrain import SimulatorTrainer
    from rl4rs_amd.utils.datautil import FeatureUtil
    sim, records, cat_path = _sim(tmp_path)
    tr = SimulatorTrainer(sim, minibatch=B, seed=1, model_type='dnn_slate')
    dense, cat, labels, seqs = tr.dataset_from_logs()
    assert dense.shape == (B, 432) and cat.shape == (B, 21) and labels.shape == (B, 9) and len(seqs) == 2
    tab = CatalogTables(cat_path, 284, 32)
    fu = FeatureUtil(sim.config)
    exp_dense, exp_cat, exp_y, exp_seq = [], [], [], []
    for rec in records:
        _, _, sequence_id, exposed, feedback, user_seq, portrait, _, _ = FeatureUtil.record_split(rec)
        exp_cat.append([int(x) for x in portrait[:10]] + [sequence_id] + exposed[:9])
        exp_dense.append(np.concatenate([np.asarray(portrait[10:], dtype=np.float32)] + [tab.item_vec[i] for i in exposed[:9]]))
        exp_y.append(feedback[:9])
        exp_seq.append(user_seq)
    assert len(exp_cat[0]) == 20 and len(exp_dense[0]) == 392
    assert np.array_equal(cat.cpu().numpy(), fu._fit(exp_cat, 21, np.int32, False))
    assert np.array_equal(dense.cpu().numpy(), fu._fit(exp_dense, 432, np.float32, False))
    assert np.array_equal(labels.cpu().numpy(), np.asarray(exp_y, dtype=np.int32))
    assert np.array_equal(seqs[0].cpu().numpy(), fu._fit(exp_seq, 64, np.int32, True)) and int(seqs[1].abs().sum()) == 0
    assert int(cat[:, -1].abs().sum()) == 0 and float(dense[:, -40:].abs().sum()) == 0 and float(dense[:, -80:-40].abs().sum()) > 0


@pytest.mark.parametrize('model_type', ['dnn_slate', 'dnn_slate_multiclass'])
def test_fit_with_validation_on_planted_labels(tmp_path, model_type):
    import torch
    from rl4rs_amd.simtrain import SimulatorTrainer
    from rl4rs_amd.utils.datautil import FeatureUtil
    sim, _, _ = _sim(tmp_path)
    tr = SimulatorTrainer(sim, minibatch=B, seed=2, model_type=model_type)
    dense, cat, _, seqs = [x.cpu().numpy() if hasattr(x, 'cpu') else [y.cpu().numpy() for y in x] for x in tr.dataset_from_logs()]
    # planted: slot j is clicked iff user-dense column j is above its median - learnable from the dense tower
    y = (dense[:, :9] > np.median(dense[:, :9], axis=0)).astype(np.int64)
    y[0], y[1] = 0, 1
    # written as the reference writes a slate sample: 392 dense values and 20 category ids; the reader pads them back
    data = [[0, [seqs[0][i].tolist(), seqs[1][i].tolist()], dense[i, :392].tolist(), cat[i, :20].tolist(), y[i].tolist(), 0]
            for i in range(B)]
    path = os.path.join(str(tmp_path), 'slate.tfrecord')
    FeatureUtil(sim.config).to_tfrecord(data, path)
    batch = next(tr._batches(path, seed=0))
    order = [int(np.flatnonzero((dense == r).all(axis=1))[0]) for r in batch[0].cpu().numpy()]      # the batch is the set, shuffled
    assert sorted(order) == list(range(B)) and np.array_equal(batch[1].cpu().numpy(), cat[order])
    assert np.array_equal(batch[2].cpu().numpy(), y[order])

    def recompute():
        """the metrics of validate() over [batch, batch], from evaluate's own predictions"""
        pred, rows = tr.trainer.evaluate(*batch)
        pred, lab = pred.cpu().numpy(), batch[2].cpu().numpy()
        if model_type.endswith('multiclass'):
            cls = lab @ np.asarray([1, 2, 4, 1, 2, 4, 1, 2, 4])
            return {'val_loss': float(rows.double().mean()), 'val_acc': float(np.mean(np.argmax(pred, axis=1) == cls))}
        r = M.metrics_from_counts(2 * M.confusion_counts(pred, lab, M.auc_thresholds(200)), 200)
        return {'val_loss': float(rows.double().mean()), 'val_auc': r['auc'], 'val_precision': r['precision'], 'val_recall': r['recall']}

    zero = tr.validate(iter([batch, batch]), 2)
    ref = recompute()
    assert list(zero) == list(ref)
    for k in ref:
        assert zero[k] == ref[k] if k != 'val_loss' else abs(zero[k] - ref[k]) < 1e-6 * max(1.0, abs(ref[k])), (k, zero[k], ref[k])
    epochs = 3
    h = tr.fit_tfrecord(path, steps=40, validation_files=path, validation_steps=2, epochs=epochs, patience=3)
    keys = ['loss', 'val_loss', 'val_acc'] if model_type.endswith('multiclass') else ['loss', 'val_loss', 'val_auc', 'val_precision', 'val_recall']
    assert list(h) == keys and all(len(v) == epochs for v in h.values())
    assert np.isfinite([v for k in h for v in h[k]]).all()
    print(model_type, 'zero-step', zero, 'history', dict(h))
    assert h['val_loss'][-1] < zero['val_loss'] and h['loss'][-1] < h['loss'][0]
    # the trained model's figures again from evaluate's predictions: exactly those of validate() on the same rows; the history's last
    # epoch saw the same set in other orders
    after = tr.validate(iter([batch, batch]), 2)
    ref = recompute()
    for k in ref:
        assert after[k] == ref[k] if k != 'val_loss' else abs(after[k] - ref[k]) < 1e-6 * max(1.0, abs(ref[k])), (k, after[k], ref[k])
        assert abs(h[k][-1] - ref[k]) < 0.02 * max(1.0, abs(ref[k])), (k, h[k][-1], ref[k])
    if not model_type.endswith('multiclass'):
        assert after['val_auc'] > zero['val_auc'] and after['val_auc'] > 0.7
    with pytest.raises(NotImplementedError):
        tr.install()
    tr.save(os.path.join(str(tmp_path), 'm.npz'))
    assert np.load(os.path.join(str(tmp_path), 'm.npz'))['out_w'].shape == (256, 22 if model_type.endswith('multiclass') else 9)
    # a TF checkpoint prefix: the variable names of the item-wise family, the head's own width
    from rl4rs_amd.utils import tfckpt
    prefix = os.path.join(str(tmp_path), 'ckpt')
    tr.save(prefix)
    shapes = dict((n, tuple(s)) for n, s, _ in tfckpt.list_variables(prefix))
    assert shapes['simulator_reward/kernel'] == (256, 22 if model_type.endswith('multiclass') else 9)
