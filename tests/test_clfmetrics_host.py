"""CPU: the numpy restatement of the keras metrics (rl4rs_amd/metrics.py) - the reference of tests/test_gpu_clfmetrics.py - against
keras' documented example and hand-counted cases, and the slate -> class mapping of the multiclass models."""
import numpy as np

from rl4rs_amd import metrics as M


def test_threshold_table_is_keras():
    t = M.auc_thresholds(200)
    assert t.dtype == np.float32 and t.shape == (200,)
    assert t[0] == np.float32(-1e-7) and t[-1] == np.float32(1.0 + 1e-7)
    assert t[1] == np.float32(1.0 / 199) and t[100] == np.float32(100.0 / 199) and t[198] == np.float32(198.0 / 199)
    assert (np.diff(t) > 0).all()
    assert M.auc_thresholds(3).tolist() == [np.float32(-1e-7), 0.5, np.float32(1.0 + 1e-7)]


def test_keras_documented_auc_example():
    """tf.keras.metrics.AUC(num_thresholds=3): y = [0, 0, 1, 1], p = [0, 0.5, 0.3, 0.9] -> tp = [2, 1, 0], fp = [2, 0, 0],
    fn = [0, 1, 2], tn = [0, 2, 2]; recall = [1, 0.5, 0], fp_rate = [1, 0, 0]; auc = ((1 + 0.5) / 2) * (1 - 0) = 0.75"""
    thr = M.auc_thresholds(3)
    c = M.confusion_counts([0, 0.5, 0.3, 0.9], [0, 0, 1, 1], thr)
    assert c[:12].tolist() == [2, 1, 0, 2, 0, 0, 0, 2, 2, 0, 1, 2]
    assert M.metrics_from_counts(c, 3)['auc'] == 0.75


def test_hand_counted_precision_recall_accuracy():
    # pred > 0.5:            F     T     T     F     T     F (0.5 itself is not above 0.5)   F (NaN)
    p = np.asarray([0.2, 0.9, 0.6, 0.4, 0.51, 0.5, np.nan], dtype=np.float32)
    y = np.asarray([0, 1, 0, 1, 1, 1, 1])
    c = M.confusion_counts(p, y, M.auc_thresholds(200))
    assert c[800:804].tolist() == [2, 1, 1, 3]                # tp, fp, tn, fn
    m = M.metrics_from_counts(c, 200)
    assert m['precision'] == 2.0 / 3.0 and m['recall'] == 2.0 / 5.0 and m['acc'] == 3.0 / 7.0
    # a NaN is above no threshold, not even -1e-7: it is a false negative everywhere
    assert c[0] == 4 and c[600] == 1


def test_no_positive_or_no_negative_labels_use_div_no_nan():
    thr = M.auc_thresholds(200)
    m = M.metrics_from_counts(M.confusion_counts([0.1, 0.7, 0.9], [0, 0, 0], thr), 200)
    assert m['auc'] == 0.0 and m['recall'] == 0.0 and m['precision'] == 0.0
    m = M.metrics_from_counts(M.confusion_counts([0.1, 0.2], [1, 1], thr), 200)
    assert m['auc'] == 0.0 and m['precision'] == 0.0            # nothing predicted positive at 0.5: 0 / 0 -> 0


def test_a_perfect_and_a_reversed_ranking():
    thr = M.auc_thresholds(200)
    p, y = [0.1, 0.2, 0.8, 0.9], [0, 0, 1, 1]
    assert abs(M.metrics_from_counts(M.confusion_counts(p, y, thr), 200)['auc'] - 1.0) < 1e-12
    assert abs(M.metrics_from_counts(M.confusion_counts(p, [1, 1, 0, 0], thr), 200)['auc']) < 1e-12


def test_categorical_counts_take_the_first_maximum():
    p = np.asarray([[0.3, 0.3, 0.1], [0.1, 0.4, 0.4], [0.2, 0.2, 0.2]], dtype=np.float32)
    assert M.categorical_counts(p, [0, 1, 0]) == (3, 3)
    assert M.categorical_counts(p, [1, 2, 2]) == (0, 3)


def test_slate_class_mapping():
    """y . [1, 2, 4, 1, 2, 4, 1, 2, 4] (my_loss_fn of the *_slate_multiclass.py models): 0 .. 21"""
    from rl4rs_amd.nets.simnets import SLATE_CLASSES, slate_class
    y = np.asarray([[0] * 9, [1] * 9, [1, 0, 0, 0, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 1, 0, 0, 1], [0, 1, 0, 1, 0, 0, 0, 0, 1],
                    [2, 0, 0, 0, 0, 0, 0, 0, -1]])
    assert slate_class(y).tolist() == [0, 21, 1, 12, 7, 5]
    every = np.asarray([[(i >> j) & 1 for j in range(9)] for i in range(512)])
    c = slate_class(every)
    assert c.min() == 0 and c.max() == SLATE_CLASSES - 1
