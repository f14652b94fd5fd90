"""Host side of Rainbow's dueling distributional Q network (RLlib 1.5.1's default DQN model as script/modelfree_train.py:146-178
leaves it: fcnet_hiddens [256, 256] tanh, hiddens [256] -> the two 128-wide streams here, num_atoms 8, dueling).

Flat parameter layout shared with ``rl4rs_amd/csrc/rainbow.hpp``:
``[ W1 (obs x trunk) | b1 | W2 (trunk x trunk) | b2 | Wa1 (trunk x stream) | ba1 | Wa2 (stream x A * atoms) | ba2
  [| Wv1 (trunk x stream) | bv1 | Wv2 (stream x atoms) | bv2] ]``; column ``a * atoms + j`` of Wa2 is atom j of action a, the value
stream exists with dueling only.
"""
import numpy as np

NAMES = ('W1', 'b1', 'W2', 'b2', 'Wa1', 'ba1', 'Wa2', 'ba2', 'Wv1', 'bv1', 'Wv2', 'bv2')


def shapes(obs_dim, action_size, num_atoms=8, trunk=256, stream_hidden=128, dueling=True):
    s = [(obs_dim, trunk), (trunk,), (trunk, trunk), (trunk,), (trunk, stream_hidden), (stream_hidden,),
         (stream_hidden, action_size * num_atoms), (action_size * num_atoms,)]
    if dueling:
        s += [(trunk, stream_hidden), (stream_hidden,), (stream_hidden, num_atoms), (num_atoms,)]
    return s


def param_count(obs_dim, action_size, num_atoms=8, trunk=256, stream_hidden=128, dueling=True):
    return int(sum(int(np.prod(s)) for s in shapes(obs_dim, action_size, num_atoms, trunk, stream_hidden, dueling)))


def split(flat, obs_dim, action_size, num_atoms=8, trunk=256, stream_hidden=128, dueling=True):
    """dict name -> view of a flat parameter / gradient vector (numpy or torch)."""
    out, o = {}, 0
    for name, shp in zip(NAMES, shapes(obs_dim, action_size, num_atoms, trunk, stream_hidden, dueling)):
        n = int(np.prod(shp))
        out[name] = flat[o:o + n].reshape(shp)
        o += n
    return out


def init_distq_params(obs_dim=256, action_size=284, num_atoms=8, trunk=256, stream_hidden=128, dueling=True, seed=0):
    """normc(1.0) for the two trunk layers (RLlib's FullyConnectedNetwork), Glorot-uniform for the four stream layers (the keras
    Dense default of distributional_q_tf_model), zero biases."""
    rs = np.random.RandomState(seed)

    def normc(shape):
        w = rs.randn(*shape)
        return w / np.sqrt(np.square(w).sum(axis=0, keepdims=True))

    def glorot(shape):
        lim = np.sqrt(6.0 / (shape[0] + shape[1]))
        return rs.uniform(-lim, lim, size=shape)

    parts = []
    for i, shp in enumerate(shapes(obs_dim, action_size, num_atoms, trunk, stream_hidden, dueling)):
        if len(shp) == 1:
            parts.append(np.zeros(shp))
        else:
            parts.append((normc(shp) if i < 4 else glorot(shp)).ravel())
    return np.concatenate(parts).astype(np.float32)
