"""The reference's ``rl4rs/utils/d3rlpy_scorer.py``: its four scorers with its call convention ``(policy_model, episodes)``, over
``rl4rs_amd.scorers`` (one pass on the device; ``episodes`` is an ``EvalEpisodes``, see ``scorers.episodes_from_mdp``).

* ``soft_opc_scorer(return_threshold)`` scores ``policy_model.predict_q``'s values: Q(o, a) reverse-transformed where the learner
  has a reward scaler.
* ``discrete_action_match_scorer`` compares the logged action with ``policy_model.predict_with_mask``'s.
* ``dynamics_reward_prediction_mean_error_scorer`` / ``..._abs_mean_error_scorer``: mean(r - r_hat) / mean|r - r_hat| over the
  transitions, r_hat the reward of ``ProbabilisticEnsembleDynamics.predict(obs, act)`` (float32 differences, float64 means).
  Deviation: as written the reference calls ``predict_q`` on the wrapped dynamics model, which d3rlpy's dynamics classes do not
  have; here ``policy_model.predict_q`` of a dynamics model returns its ``predict``: ``(next_obs, reward)``."""
from .. import scorers as S

WINDOW_SIZE = S.WINDOW_SIZE

__all__ = ['WINDOW_SIZE', 'soft_opc_scorer', 'discrete_action_match_scorer', 'dynamics_reward_prediction_mean_error_scorer',
           'dynamics_reward_prediction_abs_mean_error_scorer']


def soft_opc_scorer(return_threshold):
    return S._scorer('soft_opc', float(return_threshold), reference=True)


discrete_action_match_scorer = S._scorer('discrete_action_match_mask', reference=True)


def _reward_errors(dynamics, episodes):
    pred = dynamics.predict_q(episodes.observations, episodes.actions)
    return episodes.next_rewards.reshape(-1) - pred[1].reshape(-1).to(episodes.device)


def dynamics_reward_prediction_mean_error_scorer(dynamics, episodes):
    # (the mean of a column is the pass's average_value_estimation slot: fixed-order float64 on the device)
    return S.score_episodes(episodes.starts, {'qp': _reward_errors(dynamics, episodes)})['average_value_estimation']


def dynamics_reward_prediction_abs_mean_error_scorer(dynamics, episodes):
    return S.score_episodes(episodes.starts, {'qp': _reward_errors(dynamics, episodes).abs()})['average_value_estimation']
