"""``behavior_model`` of the reference (rl4rs/policy/behavior_model.py:9-58): the logged policy's probability of the logged action,
the ``mu`` of the off-policy estimators (script/offline_evaluation.py:31).

    sample_model = behavior_model(config, bc)                    # bc: offline_rl.DiscreteBC fitted on generate_offline_dataset(...)
    mu = sample_model.action_probs(obs, off_action, layer, page=0)      # [B] float64

``model`` is anything that yields a ``[B, A_b]`` score matrix for ``record``: an ``offline_rl.DiscreteBC`` (behaviour cloning of
the logs IS the logged-policy estimate; ``record`` is then the d3rl-mode observation, and the scores are its imitator's LOGITS), a
callable ``model(record)``, or an object with ``predict(record)`` like the reference's keras model.  ``logits`` says whether the
scores are logits (default: True for a DiscreteBC, False - non-negative probabilities - otherwise).

The layer rule is the reference's, quirk included (behavior_model.py:49-57): ``layer == 1`` -> columns [1, 40), ``layer == 2`` ->
[40, 148), ANYTHING ELSE -> [148, A_b) - so SeqSlate steps 9..35, for which ``ope_eval`` passes ``layer = j // 3 + 1 >= 4``, all use
the third range.  Within the range the action is clipped to it and the scores are renormalised:

    mu = y[b, lo + clip(a - lo, 0, hi - lo - 1)] / sum(y[b, lo:hi])            (probabilities)
    mu = exp(y_a - m) / sum_{[lo, hi)} exp(y - m),  m = max(y[b, lo:hi])       (logits: softmax, then the same renormalisation)

in float64 per row by ``rl4rs_ope_record_behavior`` - neither the softmax nor the ``[B, hi - lo]`` slice is materialised.
Loading the reference's keras ``logged_policy.h5`` (and its ``record2input`` feature pipeline) is out of scope."""
import numpy as np
import torch

from .. import offline_rl as R


def layer_range(layer, n_scores):
    """behavior_model.py:49-57"""
    if layer == 1:
        return 1, 40
    if layer == 2:
        return 40, 148
    return 148, int(n_scores)


class behavior_model(object):
    def __init__(self, config, model, logits=None):
        self.config = config
        self.model = model
        self.takes_observation = isinstance(model, R.DiscreteBC)
        self.logits = self.takes_observation if logits is None else bool(logits)

    def scores(self, record):
        """the model's ``[B, A_b]`` score matrix for ``record``"""
        m = self.model
        if isinstance(m, R.DiscreteBC):
            from .policy_model import policy_model
            net = m.imitator
            x = record if isinstance(record, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(record, dtype=np.float32)))
            return policy_model._chunks(net, x.to(device=net.device, dtype=torch.float32).contiguous())
        if hasattr(m, 'predict'):
            return m.predict(record)
        return m(record)

    def record_into(self, log, t, record, action, layer):
        """write mu of step ``t`` straight into an ``ope.OpeLog`` (what ``ope_eval`` calls: nothing returns to the host)"""
        y = self.scores(record)
        lo, hi = layer_range(layer, y.shape[1])
        log.record_behavior(t, y, lo, hi, action, self.logits)

    def action_probs(self, record, action, layer, page=0):
        from ..ope import OpeLog
        y = self.scores(record)
        B = int(y.shape[0])
        log = OpeLog(B, 1, device=y.device if isinstance(y, torch.Tensor) and y.is_cuda else None)
        try:
            log.begin(B, 1)
            lo, hi = layer_range(layer, y.shape[1])
            log.record_behavior(0, y, lo, hi, action, self.logits)
            out = log.column('mu')[0]
        finally:
            log.close()
        on_device = any(isinstance(v, torch.Tensor) and v.is_cuda for v in (record, action))
        return out if on_device else out.cpu().numpy()
