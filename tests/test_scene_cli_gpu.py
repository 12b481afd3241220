"""test.py --dump-scene / --scene: the episodes an evaluation ran, written as a scene file, replay to exactly the
same numbers; a scene with fewer rows than --epi is refused."""
import glob
import os
import sys

import numpy as np
import pytest

from test_train_gpu import _entry

pytestmark = pytest.mark.gpu


def test_dump_scene_then_scene_replays_the_same_episodes(cuda, tmp_path, monkeypatch, capsys):
    test_py, train_py = _entry("test"), _entry("train")
    eid, n, obs = "LidarSpread", 3, 2
    argv = ["train.py", "--env", eid, "-n", str(n), "--algo", "dgppo", "--obs", str(obs), "--steps", "2",
            "--n-env-train", "8", "--batch-size", "256", "--n-env-test", "4", "--eval-interval", "1",
            "--save-interval", "2", "--log-dir", str(tmp_path)]
    monkeypatch.setattr(sys, "argv", argv)
    train_py.main()
    (run,) = glob.glob(os.path.join(str(tmp_path), eid, "dgppo", "seed0_*"))
    scene = str(tmp_path / "s.npz")
    monkeypatch.setattr(sys, "argv", ["test.py", "--path", run, "--epi", "4", "--max-step", "16", "--dump-scene", scene])
    first = test_py.main()
    with np.load(scene, allow_pickle=False) as z:
        assert str(z["env_id"]) == eid
        assert z["agent"].shape == (4, n, 4) and z["goal"].shape == (4, n, 4) and z["obstacle"].shape == (4, obs, 16)
    capsys.readouterr()
    monkeypatch.setattr(sys, "argv", ["test.py", "--path", run, "--scene", scene, "--max-step", "16"])
    second = test_py.main()
    out = capsys.readouterr().out
    assert out.count("epi: ") == 4  # --epi defaults to every row of the scene
    assert first == second and set(first) == {"reward", "cost", "safe_rate"}
    # rows [offset:epi] of the file
    monkeypatch.setattr(sys, "argv", ["test.py", "--path", run, "--scene", scene, "--max-step", "16", "--offset", "1",
                                      "--epi", "3"])
    test_py.main()
    out = capsys.readouterr().out
    assert out.count("epi: ") == 2 and "epi: 1," in out and "epi: 2," in out
    monkeypatch.setattr(sys, "argv", ["test.py", "--path", run, "--scene", scene, "--max-step", "16", "--epi", "9"])
    with pytest.raises(SystemExit, match="holds 4 episodes, fewer than --epi 9"):
        test_py.main()
