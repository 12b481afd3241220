"""dgppo_env_rollout_plan with reset_first (the states-only reset inside the dgppo_env_rollout call), without a GPU:
the persistent Lidar route keeps its launch shape and needs no reset launch, every other route reports one, and
all-zero new fields reproduce the plan of before."""
import itertools

import pytest

from dgppo_fov_amd import _lib
from dgppo_fov_amd.env import make_env
from env_cases import LIDAR_IDS, forced
from test_env_rollout_plan_cpu import _plan, expected_plan, fake_io

SHAPE = ("route", "wpg", "threads", "grid", "lds_bytes")
ALL = SHAPE + ("size_block", "size_na", "size_no", "size_nr", "size_nk", "stage", "rebuild", "step_launches")


def _fields(pl, names):
    return tuple(getattr(pl, f) for f in names)


def _reset_io(c, n_env, T, align="aligned"):
    r = fake_io(c, n_env, T, 0, align)
    r.reset_first, r.seed, r.env_offset = 1, 7, 5
    return r


@pytest.mark.parametrize("eid", LIDAR_IDS)
def test_wave_route_samples_inside_its_launch(eid):
    """Wave-shaped configs: reset_first = 1 is rebuild_first = 1's route, WPG, threads, grid and LDS, no reset launch."""
    c = make_env(eid, 8, num_obs=3, device="cpu").cfg
    for wpg, n_env, T in itertools.product((0, 1, 4, 8), (1, 19, 2047, 2048, 4096), (0, 1, 17, 128)):
        with forced(wpg, 0):
            rc0, rebuild = _plan(c, fake_io(c, n_env, T, 1))
            rc1, reset = _plan(c, _reset_io(c, n_env, T))
        assert rc0 == 0 and rc1 == 0
        assert rebuild.route_name == "LIDAR_WAVE" and rebuild.reset_launches == 0
        assert _fields(reset, SHAPE) == _fields(rebuild, SHAPE), (eid, wpg, n_env, T)
        assert reset.reset_launches == 0 and reset.rebuild == 0


OFF_ROUTE = [("MPESpread", 3, 3, "aligned", 0, "MPE_WAVE", 0), ("MPETarget", 3, 0, "aligned", 0, "BLOCK", 0),
             ("LidarSpread", 32, 8, "aligned", 0, "BLOCK", 0), ("LidarLine", 4, 3, "aligned", 0, "STEP_LOOP", 0),
             ("LidarSpread", 8, 3, "t_edges+2", 0, "BLOCK", 1), ("LidarSpread", 8, 3, "edges+2", 0, "BLOCK", 0),
             ("LidarSpread", 8, 3, "aligned", 1, "BLOCK", 0), ("LidarOmniTarget", 8, 3, "t_edges+1", 0, "STEP_LOOP", 1)]


@pytest.mark.parametrize("eid,n,obs,align,mode,route,rebuild", OFF_ROUTE)
def test_other_routes_launch_the_reset(eid, n, obs, align, mode, route, rebuild):
    """MPE, n = 32, a variant, misaligned buffers and the forced block kernels: one reset launch, then the route of
    rebuild_first = 1 (a REBUILD launch where the reset was states-only: the single-step wave kernels' configs)."""
    c = make_env(eid, n, num_obs=obs, device="cpu").cfg
    with forced(0, mode):
        rc0, old = _plan(c, fake_io(c, 9, 17, 1, align))
        rc1, new = _plan(c, _reset_io(c, 9, 17, align))
    assert rc0 == 0 and rc1 == 0
    assert new.route_name == route and new.reset_launches == 1 and old.reset_launches == 0
    assert new.rebuild == rebuild
    assert _fields(new, ALL) == _fields(old, ALL)


def test_no_steps_still_resets():
    """T = 0: reset_first alone is work to do (graph 0 and the obstacle records), with or without the fused route."""
    c = make_env("LidarSpread", 8, num_obs=3, device="cpu").cfg
    rc, pl = _plan(c, _reset_io(c, 19, 0))
    assert rc == 0 and pl.route_name == "LIDAR_WAVE" and pl.reset_launches == 0
    r = _reset_io(c, 19, 0)
    r.step.action = r.step.reward = r.step.cost = None  # an episode of no steps has none of them
    rc, pl = _plan(c, r)
    assert rc == 0 and pl.route_name == "LIDAR_WAVE"
    m = make_env("MPESpread", 3, num_obs=3, device="cpu").cfg
    rc, pl = _plan(m, _reset_io(m, 19, 0))
    assert rc == 0 and pl.route_name == "STEP_LOOP" and pl.reset_launches == 1 and pl.step_launches == 0
    rc, pl = _plan(m, fake_io(m, 19, 0, 0))
    assert rc == 0 and pl.route_name == "NONE" and pl.reset_launches == 0
    r = fake_io(c, 19, 3, 1)
    r.step.action = None  # with steps to run the actions stay required
    assert _plan(c, r)[0] == _lib.DGPPO_EINVAL


@pytest.mark.parametrize("eid,n,obs", [("LidarSpread", 8, 3), ("LidarBicycleTarget", 8, 3), ("LidarOmniTarget", 8, 3),
                                       ("LidarSpread", 32, 8), ("LidarTarget", 4, 2), ("MPESpread", 3, 3),
                                       ("MPETarget", 5, 2), ("LidarLine", 4, 3)])
def test_zeroed_new_fields_reproduce_the_old_plan(eid, n, obs):
    """reset_first = 0 (seed, seed_ptr, env_offset zero): the documented rule of before, field by field."""
    c = make_env(eid, n, num_obs=obs, device="cpu").cfg
    for align, rebuild, T, n_env in itertools.product(("aligned", "t_edges+2", "states+1"), (0, 1), (0, 1, 17, 700),
                                                       (0, 9, 2048)):
        r = fake_io(c, n_env, T, rebuild, align)
        assert (r.reset_first, r.seed, r.seed_ptr, r.env_offset) == (0, 0, None, 0)
        rc, pl = _plan(c, r)
        want = expected_plan(c, r, 0, 0)
        if want == _lib.DGPPO_EINVAL:
            assert rc == _lib.DGPPO_EINVAL
            continue
        got = dict(route=pl.route_name, wpg=pl.wpg, size=pl.size_tag, stage=pl.stage, rebuild=pl.rebuild,
                   threads=pl.threads, grid=pl.grid, lds=pl.lds_bytes, steps=pl.step_launches)
        assert rc == 0 and got == want, (eid, align, rebuild, T, n_env, got, want)
        assert pl.reset_launches == 0
