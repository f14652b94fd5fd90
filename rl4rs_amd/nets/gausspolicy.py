"""Host side of the Gaussian actor-critic of the continuous on-policy learners (``rl4rs_amd/csrc/gausspolicy.hip``).

RLlib 1.5.1's ``FullyConnectedNetwork`` under ``MODEL_DEFAULTS`` (``fcnet_hiddens`` [256, 256], tanh, ``vf_share_layers`` False,
``free_log_std`` False), restated from its published form (ray is absent: parity unpinned).  Flat layout, matrices ``[in, out]``:
``[W1 | b1 | W2 | b2 | W3 (H x 2E) | b3 | V1 | c1 | V2 | c2 | V3 (H x 1) | c3]``; 279 873 parameters at 256 / 256 / 32.
"""
import numpy as np

NAMES = ('W1', 'b1', 'W2', 'b2', 'W3', 'b3', 'V1', 'c1', 'V2', 'c2', 'V3', 'c3')


def shapes(obs_dim, act_dim, hidden=256):
    """(name, shape) of the arrays in flat order."""
    D, H, E = int(obs_dim), int(hidden), int(act_dim)
    return (('W1', (D, H)), ('b1', (H,)), ('W2', (H, H)), ('b2', (H,)), ('W3', (H, 2 * E)), ('b3', (2 * E,)),
            ('V1', (D, H)), ('c1', (H,)), ('V2', (H, H)), ('c2', (H,)), ('V3', (H, 1)), ('c3', (1,)))


def param_count(obs_dim, act_dim, hidden=256):
    return sum(int(np.prod(s)) for _, s in shapes(obs_dim, act_dim, hidden))


def offsets(obs_dim, act_dim, hidden=256):
    """name -> offset of the array in the flat vector"""
    out, o = {}, 0
    for name, s in shapes(obs_dim, act_dim, hidden):
        out[name] = o
        o += int(np.prod(s))
    return out


def split(flat, obs_dim, act_dim, hidden=256):
    """name -> view of a flat parameter / gradient vector (numpy or torch)"""
    out, o = {}, 0
    for name, s in shapes(obs_dim, act_dim, hidden):
        k = int(np.prod(s))
        out[name] = flat[o:o + k].reshape(s)
        o += k
    return out


def init_gausspolicy_params(obs_dim, act_dim, hidden=256, seed=0):
    """RLlib's normc_initializer(1.0) on the hidden layers, normc_initializer(0.01) on both output layers, zero biases."""
    rs = np.random.RandomState(seed)

    def normc(shape, std):
        w = rs.randn(*shape)
        return w * std / np.sqrt(np.square(w).sum(axis=0, keepdims=True))

    parts = []
    for name, s in shapes(obs_dim, act_dim, hidden):
        if len(s) == 1:
            parts.append(np.zeros(s))
        else:
            parts.append(normc(s, 0.01 if name in ('W3', 'V3') else 1.0).ravel())
    return np.concatenate(parts).astype(np.float32)
