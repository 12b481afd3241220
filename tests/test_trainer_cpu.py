"""Evaluation metrics of the trainer / test.py (trainer.py:103-116, test.py:103-139) on hand-built
rollouts, and the Trainer's params contract."""
import numpy as np
import pytest

from dgppo_fov_amd.trainer.trainer import Trainer
from dgppo_fov_amd.trainer.utils import eval_info, safe_rate


def test_eval_info_matches_reference_formulas():
    rng = np.random.default_rng(0)
    r = rng.standard_normal((4, 6))
    c = rng.standard_normal((4, 6, 3, 2)) * 0.1
    info = eval_info(r, c)
    assert np.isclose(info["eval/reward"], r.sum(-1).mean())
    assert np.isclose(info["eval/reward_final"], r[:, -1].mean())
    assert np.isclose(info["eval/cost"], np.maximum(c, 0).max(-1).max(-1).sum(-1).mean())
    assert np.isclose(info["eval/unsafe_frac"], (c.max(-1).max(-2) >= 1e-6).mean())


def test_safe_rate_definition():
    c = -np.ones((2, 5, 4, 2))
    c[0, 3, 1, 0] = 0.0   # env 0: agent 1 touches the constraint once -> 3/4 safe
    c[1, :, :, 1] = 0.2   # env 1: every agent unsafe
    assert np.allclose(safe_rate(c), [0.75, 0.0])


def test_trainer_params_contract():
    ok = {"run_name": "x", "training_steps": 1, "eval_interval": 1, "eval_epi": 1, "save_interval": 1}
    assert Trainer._check_params(ok)
    for k in ok:
        bad = dict(ok)
        bad.pop(k)
        with pytest.raises(AssertionError):
            Trainer._check_params(bad)


def test_rollout_engine_refuses_env_offsets_that_meet_the_sensor_streams():
    """env_offset + n_env <= 2^30 (the policy's streams (env_offset << 32) | t stay below the sensor's 2^62 + 2t) is
    checked before an engine touches its env or a device -- None stands for the env here -- in every engine class."""
    from dgppo_fov_amd.trainer.rollout import (MAX_ENV_ROWS, NoisyLidarRolloutEngine, RolloutEngine,
                                               SensorRolloutEngine, check_env_offset)

    assert MAX_ENV_ROWS == 1 << 30
    for off, n in ((0, 1), (0, 1 << 30), ((1 << 30) - 8, 8), (5, 4096)):
        assert check_env_offset(off, n) == off
    bad = ((-1, 4), (1 << 30, 1), ((1 << 30) - 7, 8), (1 << 31, 4), (0, (1 << 30) + 1))
    for off, n in bad:
        with pytest.raises(ValueError, match="env_offset"):
            check_env_offset(off, n)
        with pytest.raises(ValueError, match="env_offset"):
            RolloutEngine(None, n, 4, "cpu", env_offset=off)
    from dgppo_fov_amd.env import make_env

    env, actor = make_env("LidarSpread", 3, num_obs=2, device="cpu"), object()  # the subclasses look at both first
    for off, n in bad:
        with pytest.raises(ValueError, match="env_offset"):
            SensorRolloutEngine(env, n, 4, "cpu", env_offset=off, actor=actor, sensor=lambda a, t: a)
        with pytest.raises(ValueError, match="env_offset"):
            NoisyLidarRolloutEngine(env, n, 4, "cpu", env_offset=off, actor=actor, sigma=0.05, dropout=0.2)
