from rl4rs_amd.utils.offline_policy_metrics import *  # noqa: F401,F403
from rl4rs_amd.utils.offline_policy_metrics import (eval_DM, eval_IPS, eval_CIPS, eval_SNIPS, eval_WIPS,  # noqa: F401
                                                    eval_doubly_robust, eval_seq_doubly_robust)
