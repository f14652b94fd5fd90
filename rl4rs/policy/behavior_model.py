from rl4rs_amd.policy.behavior_model import *  # noqa: F401,F403
from rl4rs_amd.policy.behavior_model import behavior_model  # noqa: F401
