"""CPU: the TD(lambda) value targets' checker (tests/td_targets.py), the parameter's validation and the refusals that need
no device."""
import math

import numpy as np
import pytest
import torch

from tests.td_targets import td_lambda_targets

LENGTHS = (1, 2, 63, 64, 65, 128, 129, 200)


def _games():
    rng = np.random.default_rng(20261017)
    for n in LENGTHS:
        for z in (-1.0, 0.0, 1.0):
            yield rng.uniform(-1.0, 1.0, n).astype(np.float32), z


def test_lambda_one_gives_the_result():
    for q, z in _games():
        assert np.array_equal(td_lambda_targets(q, z, 1.0), np.full(q.shape[0], z))


def test_lambda_zero_gives_each_search_value():
    for q, z in _games():
        assert np.array_equal(td_lambda_targets(q, z, 0.0), q.astype(np.float64))


@pytest.mark.parametrize("lam", [0.0, 0.3, 0.5, 0.9, 0.97, 1.0])
def test_constant_search_values_equal_to_the_result_give_the_result(lam):
    """(1 - lam) z + lam z = z up to one rounding per step for z = +-1; exactly for z = 0."""
    for n in LENGTHS:
        for z in (-1.0, 0.0, 1.0):
            y = td_lambda_targets(np.full(n, z), z, lam)
            assert np.abs(y - z).max() <= n * 2.0 ** -52
            if z == 0.0:
                assert not y.any()


@pytest.mark.parametrize("lam", [0.0, 0.3, 0.5, 0.9, 0.97, 1.0])
def test_targets_are_convex_combinations(lam):
    """|y| <= max(|z|, max|Q|): every y is a convex combination of the later search values and the result."""
    for q, z in _games():
        y = td_lambda_targets(q, z, lam)
        assert np.abs(y).max() <= max(abs(z), float(np.abs(q).max())) * (1.0 + 1e-12)


def test_a_hand_computed_game():
    y = td_lambda_targets([0.5, -0.25, 0.0], 1.0, 0.5)
    assert y.tolist() == [0.5 * 0.5 + 0.5 * (0.5 * -0.25 + 0.5 * 0.5), 0.5 * -0.25 + 0.5 * 0.5, 0.5]
    assert td_lambda_targets([], -1.0, 0.3).shape == (0,)


def test_validation():
    from liuzhou_amd.value_target import td_lambda_on
    assert td_lambda_on(1.0) is False and td_lambda_on(1) is False
    assert td_lambda_on(0.0) is True and td_lambda_on(0.8) is True and td_lambda_on(np.float32(0.5)) is True
    for bad in (math.nan, math.inf, -math.inf, -0.1, 1.5, "x", None, True):
        with pytest.raises(ValueError):
            td_lambda_on(bad)


def test_self_play_refuses_the_host_loop_before_it_touches_a_device():
    from liuzhou_amd.tree_engine import self_play_tree_gpu
    module = torch.nn.Linear(1, 1)
    with pytest.raises(ValueError, match="device_tail"):
        self_play_tree_gpu(module, 2, 16, 1.0, 0.1, 10, 1.0, "cpu", evaluator="module", device_tail=False,
                           value_target_lambda=0.8)
    for bad in (math.nan, math.inf, -0.1, 1.5):
        with pytest.raises(ValueError, match="value_target_lambda"):
            self_play_tree_gpu(module, 2, 16, 1.0, 0.1, 10, 1.0, "cpu", evaluator="module", value_target_lambda=bad)


def test_tail_refuses_the_in_kernel_reseat_before_it_touches_a_device():
    from liuzhou_amd.wave_tail import WaveTail
    with pytest.raises(ValueError, match="reseat"):
        WaveTail(None, 4, 16, "cpu", reseat=True, value_target_lambda=0.5)
    for bad in (math.nan, -0.1, 1.5):
        with pytest.raises(ValueError, match="value_target_lambda"):
            WaveTail(None, 4, 16, "cpu", value_target_lambda=bad)
    with pytest.raises(RuntimeError, match="HIP device"):          # off: the tail it always was
        WaveTail(None, 4, 16, "cpu", reseat=True, value_target_lambda=1.0)
