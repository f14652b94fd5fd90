"""config['env_rows_variant'] = 1 (RL4RS_ENV_OPT_ROWS_VARIANT: the row kernels read the catalogue through L1 / L2 instead of staging
it in LDS - k_env_rows<1|2,false>, k_env_rows_refine<false>, k_env_rows_ahead<false>): the option no other test sets.  The bodies,
oracles and exact comparisons are those of tests/test_gpu_env.py::test_hip_env_matches_oracle_odd_configurations (cases 0 and 1:
SlateState and SeqSlateState), of the twin-pair case of tests/test_gpu_env_ahead_rows.py and of the replay episode of
tests/test_gpu_partition_carry.py, run unchanged on a DeviceEnv that adds the option to whatever configuration it is given."""
import pytest

import test_gpu_env
import test_gpu_env_ahead_rows
import test_gpu_partition_carry

pytestmark = pytest.mark.gpu


@pytest.fixture
def variant_envs(monkeypatch):
    """every DeviceEnv created inside the test gets env_rows_variant = 1 -> the list of the options those handles were given"""
    from rl4rs_amd import device
    made = []

    class VariantEnv(device.DeviceEnv):
        def __init__(self, config, *args, **kw):
            assert 'env_rows_variant' not in config
            super().__init__(dict(config, env_rows_variant=1), *args, **kw)

        def set_option(self, name, value):
            made.append((name, int(value)))
            super().set_option(name, value)

    monkeypatch.setattr(device, 'DeviceEnv', VariantEnv)
    return made


@pytest.mark.parametrize('case', [0, 1])
def test_odd_configurations_through_l1_l2(tmp_path, variant_envs, case):
    test_gpu_env.test_hip_env_matches_oracle_odd_configurations(tmp_path, case)
    assert variant_envs and all(o == ('rows_variant', 1) for o in variant_envs), variant_envs


def test_partition_refining_act_through_l1_l2(tmp_path, monkeypatch, variant_envs):
    """k_env_rows_refine<false>: the act that carries the duplicate-row partition, in the replay episode of
    tests/test_gpu_partition_carry.py (bit-identical to the run without the carry, the partition checked against the env's rows)"""
    test_gpu_partition_carry.test_slate_episode_is_bit_identical_and_the_partition_holds(tmp_path, monkeypatch, 'replay')
    assert variant_envs and all(o == ('rows_variant', 1) for o in variant_envs), variant_envs


def test_ahead_rows_twin_pairs_through_l1_l2(tmp_path, variant_envs):
    test_gpu_env_ahead_rows.test_partition_copy_splits_envs_whose_logged_actions_part_later(tmp_path, 9)
    assert variant_envs == [('rows_variant', 1)], variant_envs
