from rl4rs_amd.utils.d3rlpy_scorer import *  # noqa: F401,F403
from rl4rs_amd.utils.d3rlpy_scorer import (WINDOW_SIZE, soft_opc_scorer, discrete_action_match_scorer,  # noqa: F401
                                           dynamics_reward_prediction_mean_error_scorer,
                                           dynamics_reward_prediction_abs_mean_error_scorer)
