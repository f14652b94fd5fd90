"""The metrics script/supervised_train.py fits with (``metrics=['AUC', 'acc']``, ``tf.keras.metrics.AUC() / Precision() /
Recall()``, the multiclass models' categorical accuracy), as keras 2.2.4-tf (TensorFlow 1.15) defines them.

Two statements of the same definitions:

* ``ClassifierMetrics`` - the ``rl4rs_clfmetrics_*`` handle: int64 confusion counts accumulated on the device by integer atomics (exact,
  identical from run to run, no host wait in an update); the metrics are derived from the counts on the host in float64.
* ``confusion_counts`` / ``categorical_counts`` - the numpy restatement: the CPU fallback of the tests and the documentation of
  the rules.

The rules (tensorflow/python/keras/metrics.py and utils/metrics_utils.py at 1.15 **[from memory]**; TensorFlow cannot be installed
here, so like the losses they are unpinned against a keras run):

* ``AUC(num_thresholds=T)``: thresholds ``[-1e-7] + [(i + 1) / (T - 1) for i in range(T - 2)] + [1 + 1e-7]`` as float32; a
  prediction is positive at a threshold iff ``pred > thr`` (float32; a NaN is above nothing); labels are cast to bool.  ROC curve,
  ``summation_method='interpolation'``: x = FP / (FP + TN), y = TP / (TP + FN), both ``div_no_nan`` (0 where the denominator is 0),
  AUC = sum_i (x_i - x_{i+1}) * (y_i + y_{i+1}) / 2.
* ``Precision()`` / ``Recall()``: TP / (TP + FP) and TP / (TP + FN) at threshold 0.5 (``pred > 0.5``), ``div_no_nan``.
* ``'acc'`` with binary_crossentropy = binary_accuracy: mean(round-at-0.5(pred) == label), over every output element.
* categorical accuracy: mean(argmax(pred) == class), ``tf.argmax`` taking the FIRST maximum.
"""
import ctypes as C

import numpy as np

KERAS_AUC_THRESHOLDS = 200


def auc_thresholds(num_thresholds=KERAS_AUC_THRESHOLDS):
    """keras' AUC threshold table, float32 [num_thresholds]"""
    T = int(num_thresholds)
    if T < 2:
        raise ValueError('num_thresholds must be > 1')
    return np.asarray([0.0 - 1e-7] + [(i + 1) * 1.0 / (T - 1) for i in range(T - 2)] + [1.0 + 1e-7], dtype=np.float32)


def confusion_counts(pred, label, thresholds):
    """numpy restatement of the binary update: int64 [4 T + 6] = TP [T] | FP [T] | TN [T] | FN [T] | tp, fp, tn, fn at 0.5 | 0, 0
    (the layout of ``rl4rs_clfmetrics_read``), by T direct comparisons per element."""
    pred = np.asarray(pred, dtype=np.float32).reshape(-1)
    pos = np.asarray(label).reshape(-1) != 0
    thr = np.asarray(thresholds, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        above = pred[None, :] > thr[:, None]              # [T, n]; False for a NaN prediction
        hit = pred > np.float32(0.5)
    tp = (above & pos[None, :]).sum(axis=1)
    fp = (above & ~pos[None, :]).sum(axis=1)
    tn = (~above & ~pos[None, :]).sum(axis=1)
    fn = (~above & pos[None, :]).sum(axis=1)
    half = [(hit & pos).sum(), (hit & ~pos).sum(), (~hit & ~pos).sum(), (~hit & pos).sum()]
    return np.concatenate([tp, fp, tn, fn, half, [0, 0]]).astype(np.int64)


def categorical_counts(pred, label):
    """(rows whose first maximum is the label, rows)"""
    pred = np.asarray(pred, dtype=np.float32)
    return int((np.argmax(pred, axis=1) == np.asarray(label).reshape(-1)).sum()), int(pred.shape[0])


def _div_no_nan(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.where(b != 0, a / np.where(b != 0, b, 1.0), 0.0)


def metrics_from_counts(counts, num_thresholds):
    """counts: int64 [4 T + 6] (``rl4rs_clfmetrics_read`` / ``confusion_counts``) -> dict of float64 auc, precision, recall, acc
    (binary accuracy), categorical_acc."""
    T = int(num_thresholds)
    c = np.asarray(counts, dtype=np.int64)
    assert c.shape == (4 * T + 6,), c.shape
    tp, fp, tn, fn = [c[i * T:(i + 1) * T].astype(np.float64) for i in range(4)]
    x = _div_no_nan(fp, fp + tn)
    y = _div_no_nan(tp, tp + fn)
    auc = float(np.sum((x[:T - 1] - x[1:]) * (y[:T - 1] + y[1:]) / 2.0))
    htp, hfp, htn, hfn, ok, rows = [float(v) for v in c[4 * T:]]
    return {'auc': auc,
            'precision': float(_div_no_nan(htp, htp + hfp)),
            'recall': float(_div_no_nan(htp, htp + hfn)),
            'acc': float(_div_no_nan(htp + htn, htp + hfp + htn + hfn)),
            'categorical_acc': float(_div_no_nan(ok, rows))}


class ClassifierMetrics(object):
    """``rl4rs_clfmetrics`` handle: streaming confusion counts on the device.  ``update_binary`` / ``update_multiclass`` take device
    tensors and return at once; ``counts()`` is the one host read; ``result()`` the keras metrics of everything since ``reset()``."""

    def __init__(self, num_thresholds=KERAS_AUC_THRESHOLDS, device=None):
        import torch
        from . import _lib
        _lib.require_device()
        self.lib = _lib.load()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.T = int(num_thresholds)
        self.thresholds = auc_thresholds(self.T)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.rl4rs_clfmetrics_create(self.T, self.thresholds.ctypes.data_as(_lib._FP), self._stream(), C.byref(h)))
        self.h = h

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if getattr(self, 'h', None) is not None and self.h:
            self.lib.rl4rs_clfmetrics_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        from ._lib import check
        check(self.lib.rl4rs_clfmetrics_reset(self.h, self._stream()))

    def _pair(self, pred, label):
        import torch
        pred = pred.to(device=self.device, dtype=torch.float32).contiguous()
        label = label.to(device=self.device, dtype=torch.int32).contiguous()
        return pred, label

    def update_binary(self, pred, label):
        """pred (any shape, float) against label (same shape; non-zero = positive), element by element"""
        from ._lib import check
        pred, label = self._pair(pred, label)
        assert pred.numel() == label.numel() and pred.numel() > 0, (tuple(pred.shape), tuple(label.shape))
        check(self.lib.rl4rs_clfmetrics_update_binary(self.h, pred.numel(), C.c_void_p(pred.data_ptr()), C.c_void_p(label.data_ptr()),
                                                      self._stream()))
        self._keep = (pred, label)            # alive until the next update: nothing waited for the launch

    def update_multiclass(self, pred, label):
        """pred [N, K] against the class index label [N]"""
        from ._lib import check
        pred, label = self._pair(pred, label)
        assert pred.dim() == 2 and label.shape == (pred.shape[0],) and pred.shape[0] > 0, (tuple(pred.shape), tuple(label.shape))
        check(self.lib.rl4rs_clfmetrics_update_multiclass(self.h, pred.shape[0], pred.shape[1], C.c_void_p(pred.data_ptr()),
                                                          C.c_void_p(label.data_ptr()), self._stream()))
        self._keep = (pred, label)

    def counts(self):
        """int64 [4 T + 6]: TP | FP | TN | FN per threshold, tp / fp / tn / fn at 0.5, multiclass correct / rows.  Waits for the stream."""
        from ._lib import check
        out = np.zeros(4 * self.T + 6, dtype=np.int64)
        check(self.lib.rl4rs_clfmetrics_read(self.h, out.ctypes.data_as(C.POINTER(C.c_int64)), self._stream()))
        return out

    def result(self):
        return metrics_from_counts(self.counts(), self.T)


class HostClassifierMetrics(object):
    """The interface of ``ClassifierMetrics`` over the numpy restatement: for hosts without a device (tests, stub trainers) - never
    chosen implicitly."""

    def __init__(self, num_thresholds=KERAS_AUC_THRESHOLDS):
        self.T = int(num_thresholds)
        self.thresholds = auc_thresholds(self.T)
        self.reset()

    def reset(self):
        self._counts = np.zeros(4 * self.T + 6, dtype=np.int64)

    def update_binary(self, pred, label):
        self._counts += confusion_counts(np.asarray(pred.cpu() if hasattr(pred, 'cpu') else pred),
                                         np.asarray(label.cpu() if hasattr(label, 'cpu') else label), self.thresholds)

    def update_multiclass(self, pred, label):
        ok, rows = categorical_counts(np.asarray(pred.cpu() if hasattr(pred, 'cpu') else pred),
                                      np.asarray(label.cpu() if hasattr(label, 'cpu') else label))
        self._counts[4 * self.T + 4] += ok
        self._counts[4 * self.T + 5] += rows

    def counts(self):
        return self._counts.copy()

    def result(self):
        return metrics_from_counts(self._counts, self.T)

    def close(self):
        pass
