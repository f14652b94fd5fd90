"""The plain one-GPU bench.py run (what the headline is measured with): the result line carries the headline fields and none of
the ``--full`` measurements, ``--steps`` is the number of timed steps, and ``--dump-outputs`` writes the last timed step's
outputs as float32 / float64 .npy files that are identical from run to run (seeded inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ('kernels', 'roofline_gather', 'non_scorer_ms_per_step', 'extra', 'exact_fp32_scorer', 'cpu_baseline')


def _bench(args, timeout=300):
    env = dict((k, v) for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT'))
    out = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1'] + args, cwd=REPO, env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    lines = [l for l in out.stdout.decode().splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout.decode()[-2000:]
    return json.loads(lines[0])


def _load(d):
    names = sorted(f for f in os.listdir(d) if f.endswith('.npy'))
    return dict((n, np.load(os.path.join(d, n))) for n in names)


@pytest.mark.parametrize('leg', [[], ['--train', 'ppo']])
def test_plain_line_and_outputs(tmp_path, leg):
    args = ['--batch', '256', '--log-records', '700', '--steps', '3', '--warmup', '1'] + leg
    dumps = []
    for run in range(2):
        d = str(tmp_path / ('run%d' % run))
        rec = _bench(args + ['--dump-outputs', d])
        assert rec['steps'] == 3 and rec['warmup'] == 1 and rec['n_gpus'] == 1
        assert rec['unit'] == 'env-steps/s' and rec['higher_is_better'] is True and rec['value'] > 0
        assert rec['metric'].startswith('env-steps/s') and rec['dtype'].startswith('f32')
        assert abs(rec['ms_per_step'] - 256 * 9 / rec['value'] * 1e3) <= 1e-6 * rec['ms_per_step']
        assert not [k for k in FULL_ONLY if k in rec], rec.keys()
        assert rec['param_digest_per_rank'] is None
        dumps.append(_load(d))
    got, again = dumps
    assert got and sum(a.nbytes for a in got.values()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in got.values())
    if not leg:
        assert got['obs.npy'].shape == (256, 256) and got['episode_reward.npy'].shape == (256,)
    else:
        assert 'policy_params.npy' in got and 'stats_policy_loss.npy' in got
    # the same arguments: the same seeded inputs, the same outputs
    assert sorted(again) == sorted(got)
    for n in got:
        assert np.array_equal(again[n], got[n]), n


def test_full_adds_the_extra_measurements():
    rec = _bench(['--batch', '256', '--log-records', '700', '--steps', '2', '--warmup', '1', '--full', '--no-cpu-baseline',
                  '--no-extra-legs'])
    assert rec['steps'] == 2 and rec['kernels'] and rec['roofline_gather']['unit'] == 'GB/s'
    assert 'non_scorer_ms_per_step' in rec and rec['exact_fp32_scorer']['value'] > 0
