"""CPU: the file layer of ``train._Checkpoint`` (the online trainers' ``save`` / ``restore``) on a stand-in whose handles hold numpy
arrays: every key round-trips, a class / algo / shape mismatch raises ``ValueError`` naming both sides, and a truncated file raises
before anything is loaded."""
import io

import numpy as np
import pytest

from rl4rs_amd.train import _Checkpoint


class _Net(object):
    def __init__(self, rs, hidden, adam=True):
        self.obs_dim, self.hidden, self.n_params = 6, hidden, 6 * hidden + hidden
        self.p = rs.randn(self.n_params).astype(np.float32)
        self.m = rs.randn(self.n_params).astype(np.float32) if adam else None
        self.v = rs.rand(self.n_params).astype(np.float32) if adam else None
        self.t = int(rs.randint(1, 1000)) if adam else 0

    def params(self):
        return self.p.copy()

    def set_params(self, flat):
        assert isinstance(flat, np.ndarray)                # a host stand-in gets the file's arrays as they are
        self.p = np.array(flat, dtype=np.float32)

    def adam_state(self):
        return self.m.copy(), self.v.copy(), self.t

    def set_adam_state(self, m, v, t):
        self.m, self.v, self.t = np.array(m, dtype=np.float32), np.array(v, dtype=np.float32), int(t)


class _Stand(_Checkpoint):
    _ckpt_host = ('iteration', '_rollouts', '_kl_coeff')

    def __init__(self, seed, algo='A2C', hidden=4):
        rs = np.random.RandomState(seed)
        self.algo_name, self.seed = algo, seed
        self.policy, self.actor = _Net(rs, hidden), _Net(rs, hidden, adam=False)
        self.target = rs.randn(3, 5)
        self.noise = rs.randint(0, 255, size=16).astype(np.uint8)
        self.iteration, self._rollouts, self._kl_coeff = int(rs.randint(1, 50)), int(rs.randint(1, 50)), float(rs.rand())
        self.settled = 0

    def _settle(self):
        self.settled += 1

    def _ckpt_nets(self):
        return [('policy', self.policy, True), ('actor', self.actor, False)]

    def _ckpt_tensors(self):
        return {'target': self.target}

    def _ckpt_extra(self):
        return {'noise': self.noise}

    def _ckpt_set_extra(self, extra):
        self.noise = extra['noise'].copy()

    def state(self):
        return [self.policy.p, self.policy.m, self.policy.v, np.array(self.policy.t), self.actor.p, self.target, self.noise,
                np.array([self.iteration, self._rollouts]), np.array(self._kl_coeff)]


class _Other(_Stand):
    pass


def _same(a, b):
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a.state(), b.state()))


def test_every_key_round_trips(tmp_path):
    path = str(tmp_path / 'ckpt.npz')
    a, b = _Stand(1), _Stand(2)
    assert not _same(a, b)
    a.save(path)
    assert a.settled == 1                                  # save settles the deferred statistics first
    with np.load(path) as z:
        keys = set(z.files)
        assert str(z['class']) == '_Stand' and str(z['algo_name']) == 'A2C' and int(z['seed']) == 1
    assert keys == {'class', 'algo_name', 'shapes', 'seed', 'net.policy.params', 'net.policy.adam_m', 'net.policy.adam_v',
                    'net.policy.adam_t', 'net.actor.params', 'tensor.target', 'host.iteration', 'host._rollouts', 'host._kl_coeff',
                    'extra.noise'}
    b.restore(path)
    assert _same(a, b)
    assert type(b.iteration) is int and type(b._kl_coeff) is float and type(b.policy.t) is int
    assert b.seed == 2                                     # recorded, not restored


@pytest.mark.parametrize('other,sides', [(lambda: _Other(2), ('_Stand', '_Other')), (lambda: _Stand(2, algo='PPO'), ("'A2C'", "'PPO'")),
                                         (lambda: _Stand(2, hidden=8), ('["hidden", 4]', '["hidden", 8]'))],
                         ids=['class', 'algo', 'shape'])
def test_a_mismatch_names_both_sides_and_changes_nothing(tmp_path, other, sides):
    path = str(tmp_path / 'ckpt.npz')
    _Stand(1).save(path)
    b, ref = other(), other()
    with pytest.raises(ValueError) as e:
        b.restore(path)
    assert all(s in str(e.value) for s in sides), str(e.value)
    assert _same(b, ref)


def test_a_truncated_file_raises_and_loads_nothing(tmp_path):
    path = str(tmp_path / 'ckpt.npz')
    _Stand(1).save(path)
    blob = open(path, 'rb').read()
    for keep in (len(blob) // 2, len(blob) - 7):
        open(path, 'wb').write(blob[:keep])
        b = _Stand(2)
        with pytest.raises(Exception):
            b.restore(path)
        assert _same(b, _Stand(2))
    # a file without one of its arrays (an older layout) is refused as a whole too
    full = dict(np.load(io.BytesIO(blob)))
    del full['net.policy.adam_v']
    with open(path, 'wb') as f:
        np.savez(f, **full)
    b = _Stand(2)
    with pytest.raises(ValueError, match='adam_v'):
        b.restore(path)
    assert _same(b, _Stand(2))
