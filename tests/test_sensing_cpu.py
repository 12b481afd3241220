"""utils.sensor.Sensing, the one validated record of what is sensed, on device="cpu" envs: every caller that takes the
sensing options (make_algo for the four algorithms, both sensor rollout engines, env.observe) refuses and accepts
exactly what tests/golden/sensing_refusals.json holds -- the outcomes of the same grid recorded from the code before
the record existed, exception types and message texts included -- and Sensing.of, given a caller's own arguments,
decides as that caller does."""
import dataclasses
import json
import os

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from dgppo_fov_amd import _lib, ops  # noqa: F401  (registers torch.ops.dgppo.*)
from dgppo_fov_amd.algo import make_algo
from dgppo_fov_amd.env import make_env
from dgppo_fov_amd.env.base import MultiAgentEnv
from dgppo_fov_amd.trainer.rollout import NoisyLidarRolloutEngine, SensorRolloutEngine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sensing_refusals.json")
NAN = float("nan")
N, OBS, B = 3, 2, 2
LIDAR = ("LidarSpread", "LidarTarget", "LidarLine", "LidarBicycleTarget", "LidarOmniTarget")
ENVS = ([(e, dict(num_obs=OBS)) for e in LIDAR] + [(e, dict(num_obs=0)) for e in LIDAR]
        + [("MPESpread", dict(num_obs=3)), ("VMASWheel", {})])
OPTIONS = {  # name -> (noise, dropout, occlusion, fov)
    "nothing": (None, None, False, None),
    "noise": (0.1, None, False, None), "dropout": (None, 0.2, False, None), "occlusion": (None, None, True, None),
    "fov=60": (None, None, False, 60), "all": (0.1, 0.2, True, 45.0),
    "fov=180": (None, None, False, 180), "fov=0": (None, None, False, 0), "fov=-3": (None, None, False, -3),
    "fov=200": (None, None, False, 200), "fov=nan": (None, None, False, NAN),
    "sigma=-1": (-1, None, False, None), "sigma=nan": (NAN, None, False, None),
    "dropout=-0.1": (None, -0.1, False, None), "dropout=1.5": (None, 1.5, False, None),
}
ALGOS = ("dgppo", "informarl", "informarl_lagr", "hcbfcrpo")
CALLERS = tuple("make_algo:" + a for a in ALGOS) + ("NoisyLidarRolloutEngine", "SensorRolloutEngine", "env.observe")


class _Actor:  # what an engine reads of its actor before the first run
    carry_width = 64


def _outcome(fn):
    """["ok", what fn returned] or [exception type name, message]."""
    try:
        return ["ok", fn()]
    except (ValueError, NotImplementedError) as e:
        return [type(e).__name__, str(e)]


def _given(**kw):
    return {k: v for k, v in kw.items() if v is not None}


class _RecordOps(TorchDispatchMode):
    """The dgppo op a call picks, with its flags (and cone angle), without running it."""

    def __init__(self, calls):
        super().__init__()
        self.calls = calls

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if func.namespace == "dgppo":
            name = func._schema.name.split("::")[1]
            self.calls.append([name, args[11]] + ([args[12]] if name == "lidar_observe_fov" else []))
            return None
        return func(*args, **(kwargs or {}))


def _call(env, caller, opt, monkeypatch):
    noise, dropout, occlusion, fov = opt
    if caller.startswith("make_algo:"):
        def algo():
            a = make_algo(caller.split(":")[1], env=env, node_dim=env.node_dim, edge_dim=env.edge_dim,
                          state_dim=env.state_dim, action_dim=env.action_dim, n_agents=env.num_agents, batch_size=8,
                          rnn_step=2, device="cpu", lidar_noise=noise, lidar_dropout=dropout,
                          lidar_occlusion=occlusion, lidar_fov=fov)
            return [None if a.sensor is None else list(a.sensor), a.occlusion, a.fov, bool(a.sensed)]
        return _outcome(algo)
    if caller == "NoisyLidarRolloutEngine":
        def noisy():
            e = NoisyLidarRolloutEngine(env, B, 2, "cpu", actor=_Actor(), occlusion=occlusion, fov=fov,
                                        **_given(sigma=noise, dropout=dropout))
            return [e.sigma, e.dropout, e.occlusion, e.fov]
        return _outcome(noisy)
    if caller == "SensorRolloutEngine":
        def sensor():  # a sensor is any callable: the engine does not know its sigma
            given = noise is not None or dropout is not None
            e = SensorRolloutEngine(env, B, 2, "cpu", actor=_Actor(), sensor=(lambda a, t: a) if given else None,
                                    occlusion=occlusion, fov=fov)
            return [e.occlusion, e.fov]
        return _outcome(sensor)
    assert caller == "env.observe"
    calls = []
    monkeypatch.setattr(_lib, "require_gpu", lambda *a, **k: None)
    monkeypatch.setattr(MultiAgentEnv, "_observe_chained", lambda self, *a: calls.append(["chained"]))
    monkeypatch.setattr(MultiAgentEnv, "line_of_sight", lambda self, *a: calls.append(["line_of_sight"]))
    sd = env.state_dim
    state = (torch.zeros(B, N, sd), torch.zeros(B, env.num_goals, sd), torch.zeros(B, max(env.n_obs, 1), 16))

    def observe():
        with _RecordOps(calls):
            try:
                env.observe(state, 0, sigma=noise or 0.0, dropout=dropout or 0.0, seed=1, occlusion=occlusion, fov=fov)
            except ValueError as e:  # what follows the chained launches (the variant envs) needs their results
                if ["chained"] not in calls:
                    raise e
        return calls
    return _outcome(observe)


def _grid(monkeypatch):
    out = {}
    for eid, okw in ENVS:
        env = make_env(eid, N, device="cpu", **okw)
        for oname, opt in OPTIONS.items():
            for caller in CALLERS:
                out[f"{eid}/{okw.get('num_obs', '-')}/{oname}/{caller}"] = _call(env, caller, opt, monkeypatch)
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _same(a, b):
    return json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)  # NaN never appears in an outcome


def test_every_caller_refuses_and_accepts_as_before(golden, monkeypatch):
    now = _grid(monkeypatch)
    assert set(now) == set(golden) and len(now) == len(ENVS) * len(OPTIONS) * len(CALLERS)
    wrong = {k: (golden[k], now[k]) for k in golden if not _same(golden[k], now[k])}
    assert not wrong, f"{len(wrong)} cells differ, e.g. {sorted(wrong.items())[:3]}"
    kinds = {v[0] for v in golden.values()}
    assert kinds == {"ok", "ValueError", "NotImplementedError"}  # the grid reaches every kind of outcome
    for word in ("get_cost", "the VMAS envs", "no LiDAR", "no heading", "half angle", "sigma", "dropout"):
        assert any(v[0] != "ok" and word in v[1] for v in golden.values()), word


def _of(env, caller, opt):
    """Sensing.of with the arguments `caller` itself passes for the option set."""
    from dgppo_fov_amd.algo import DGPPO, HCBFCRPO, InforMARL, InforMARLLagr
    from dgppo_fov_amd.utils.sensor import Sensing

    noise, dropout, occlusion, fov = opt
    if caller.startswith("make_algo:"):
        cls = dict(zip(ALGOS, (DGPPO, InforMARL, InforMARLLagr, HCBFCRPO)))[caller.split(":")[1]]
        return Sensing.of(env, "lidar_fov", noise, dropout, occlusion, fov, algo_cls=cls)
    if caller == "NoisyLidarRolloutEngine":  # its sigma and dropout default to 0: always a sensor model
        return Sensing.of(env, caller, 0.0 if noise is None else noise, 0.0 if dropout is None else dropout, occlusion, fov)
    if caller == "SensorRolloutEngine":  # the sensor is the caller's callable, not a noise value
        return Sensing.of(env, caller, occlusion=occlusion, fov=fov)
    return Sensing.of(env, "observe", noise or 0.0, dropout or 0.0, occlusion, fov)


def test_sensing_of_decides_as_each_caller_does(golden):
    for eid, okw in ENVS:
        env = make_env(eid, N, device="cpu", **okw)
        for oname, opt in OPTIONS.items():
            for caller in CALLERS:
                cell = f"{eid}/{okw.get('num_obs', '-')}/{oname}/{caller}"
                want, got = golden[cell], _outcome(lambda: _of(env, caller, opt))
                if got[0] != "ok":
                    assert got == want, cell
                    continue
                s = got[1]
                if caller == "SensorRolloutEngine" and want[0] != "ok":
                    # nothing for the record to refuse: the engine's own checks, of its sensor and (for the scan it
                    # runs whatever is sensed) of the env's LiDAR
                    own = ("sensor must be a callable", ": this env has no LiDAR", "VMAS envs have no LiDAR sensor model")
                    assert s is None and any(w in want[1] for w in own), cell
                    continue
                assert want[0] == "ok", cell
                if caller.startswith("make_algo:"):
                    sensor, occlusion, cone, sensed = want[1]
                    assert (s is None) == (not sensed), cell  # None exactly where algo.sensed is false
                    if s is not None:
                        got_sensor = None if s.sigma is None else [s.sigma, s.dropout]
                        assert [got_sensor, s.occlusion, s.fov] == [sensor, occlusion, cone], cell
                elif caller == "NoisyLidarRolloutEngine":
                    assert [s.sigma, s.dropout, s.occlusion, s.fov] == want[1], cell
                elif caller == "SensorRolloutEngine":
                    assert [s is not None and s.occlusion, None if s is None else s.fov] == want[1], cell
                else:  # env.observe: the op follows the record's cone and occlusion
                    first = want[1][0]
                    if first[0] in ("chained", "line_of_sight"):
                        assert s.fov is None and s.occlusion == (first[0] == "line_of_sight"), cell
                    else:
                        name = "lidar_observe" + ("_fov" if s.fov is not None else "_los" if s.occlusion else "")
                        assert first[0] == name and (s.fov is None or first[2] == s.fov), cell


def test_sensing_is_frozen():
    from dgppo_fov_amd.utils.sensor import Sensing

    env = make_env("LidarOmniTarget", N, num_obs=OBS, device="cpu")
    s = Sensing.of(env, "test", noise=0.1, dropout=0.2, occlusion=True, fov=60)
    assert dataclasses.is_dataclass(s) and [f.name for f in dataclasses.fields(s)] == ["sigma", "dropout", "occlusion", "fov"]
    assert (s.sigma, s.dropout, s.occlusion, s.fov) == (0.1, 0.2, True, 60.0)
    for name in ("sigma", "dropout", "occlusion", "fov"):
        with pytest.raises(dataclasses.FrozenInstanceError):
            setattr(s, name, 0)
    assert Sensing.of(env, "test") is None and Sensing.of(env, "test", fov=180) is None
    assert Sensing.of(env, "test", fov=180.0, occlusion=True) == Sensing(None, None, True, None)


@pytest.mark.parametrize("engine", [NoisyLidarRolloutEngine, SensorRolloutEngine])
def test_an_engine_built_from_the_record_matches_one_built_from_the_keywords(engine):
    from dgppo_fov_amd.utils.sensor import LidarNoise, Sensing

    env = make_env("LidarBicycleTarget", N, num_obs=OBS, device="cpu")
    for noise, dropout, occlusion, fov in ((0.1, 0.2, True, 45.0), (0.0, 0.0, False, None), (0.3, 0.0, False, 180),
                                           (0.0, 1.0, True, None)):
        s = Sensing.of(env, "test", noise, dropout, occlusion, fov)
        if engine is NoisyLidarRolloutEngine:
            kw = dict(sigma=noise, dropout=dropout)
        else:  # its sensor is a callable; from the record it is the record's LidarNoise
            kw = dict(sensor=LidarNoise(noise, dropout, 0, sense_range=float(env.params["comm_radius"])))
        a = engine(env, B, 2, "cpu", actor=_Actor(), occlusion=occlusion, fov=fov, **kw)
        b = engine(env, B, 2, "cpu", actor=_Actor(), sensing=s)
        model = (lambda e: e) if engine is NoisyLidarRolloutEngine else (lambda e: e.sensor)
        assert (model(a).sigma, model(a).dropout, a.occlusion, a.fov) == \
            (model(b).sigma, model(b).dropout, b.occlusion, b.fov) == \
            (noise, dropout, occlusion, None if fov in (None, 180) else fov)
        assert a.obs.states.shape == b.obs.states.shape
