"""Model-level checkpoint and resume of PPO2 / TRPO (grasp_rl/sb/checkpoint.py, ppo2.py, trpo.py) on the g++ emulation build.
Run A is ``learn(full)`` with a callback that saves on the way -- between ``engine.step`` and ``engine.rewards``, so one slot of the
rollout is written and not closed -- and runs on to the end.  Run B is a NEW Python process: ``load_checkpoint`` on fresh
environments that stand at the episode run A was in, then ``learn(more, reset_num_timesteps=False)``.  Parameters, the whole state
arena, the VecNormalize pickle, ``num_timesteps`` / ``n_updates`` and every action taken after the checkpoint must be EQUAL (raw
words, no tolerance).  tests/ppo_checkpoint_util.py holds the procedure, tests/test_gpu_ppo_checkpoint_learn.py runs it on the real
library."""
import os
import zipfile

import numpy as np
import pytest

import ppo_checkpoint_util as cu
from grasp_rl._capi import GrlError


@pytest.fixture
def emulation(hostemu_lib, monkeypatch):
    from grasp_rl.sb import trpo
    from grasp_rl.sb.ppo2 import PPO2
    monkeypatch.setattr(PPO2, "_engine_factory", PPO2._engine_factory)      # restored after the test
    monkeypatch.setattr(trpo.TRPO, "_engine_factory", trpo.TRPO._engine_factory)
    monkeypatch.setattr(trpo, "VF_BATCH", trpo.VF_BATCH)
    monkeypatch.delenv("GRL_CHECKPOINT_STATE", raising=False)
    cu.install_emulation(hostemu_lib)
    return hostemu_lib


@pytest.mark.parametrize("case", sorted(cu.CASES))
def test_resumed_run_equals_uninterrupted_run(emulation, tmp_path, case):
    c = cu.CASES[case]
    a, path = cu.run_a(case, tmp_path)
    assert a["counters"][0] == c["full"] and a["actions"].shape[:2] == (c["n"], c["full"] // c["n"] - c["save_at"])
    cu.assert_equal_runs(a, cu.run_b(case, path, tmp_path, emulation))


def test_plain_save_and_load_with_the_environment_switch(emulation, tmp_path):
    a, path = cu.run_a("ppo-n4", tmp_path, how="save")
    cu.assert_equal_runs(a, cu.run_b("ppo-n4", path, tmp_path, emulation, how="save"))


@pytest.mark.parametrize("case,T", [("ppo-n4", 96), ("ppo-n1", 24), ("trpo", 48)])
def test_learn_returns_then_save(emulation, tmp_path, case, T):
    """learn(T), save_checkpoint, a fresh process, load_checkpoint, learn(T, reset_num_timesteps=False) equals learn(2 T): T is a
    common multiple of n_batch and n_envs * EPISODE, so the restored flags are all 1, as the seam sets them."""
    c = cu.CASES[case]
    assert T % (c["n"] * c["n_steps"]) == 0 and T % (c["n"] * cu.EPISODE) == 0
    env = cu.make_env(c["n"])
    model = cu.new_model(case, env, 2 * T, full=2 * T)
    model.learn(2 * T)
    a = cu.result(model, env, T // c["n"])
    model.engine.close()
    cu.assert_equal_runs(a, cu.run_returned(case, tmp_path, emulation, T))


def test_without_the_rollout_an_empty_one_starts_at_the_seam(emulation, tmp_path):
    """include_replay=False: the steps of the partial rollout are counted in num_timesteps and not trained on."""
    case = "ppo-n4"
    c = cu.CASES[case]
    env = cu.make_env(c["n"])
    model = cu.new_model(case, env, c["full"])
    path = str(tmp_path / "m")
    model.learn(c["full"], callback=cu.SaveAt(c["save_at"], cu.saver("checkpoint", path, include_replay=False)))
    assert sorted(os.listdir(path + ".state")) == ["handle.bin", "host.pkl", "meta.json", "state.bin"]
    model.engine.close()
    env2 = cu.make_env(c["n"], start_episode=c["start_episode"])
    again = cu.model_class("ppo").load_checkpoint(path, env2, **cu.load_kwargs(case, c["full"], c["full"]))
    assert again.num_timesteps == 48 and again.n_updates == 4 and again.engine.rollout_cursor() == (0, 0, False)
    again.learn(48, reset_num_timesteps=False)              # 48 more steps hold ONE whole rollout of 32
    assert again.num_timesteps == 80 and again.n_updates == 8 and again._resume is None
    assert len(env2.venv.envs[0].actions) == 8
    again.engine.close()


@pytest.mark.parametrize("algo", ["ppo", "trpo"])
def test_save_without_the_switch_writes_the_same_zip_and_nothing_else(emulation, tmp_path, algo):
    """The zip `save` writes is the one the bare zip writer of the model class writes (what `save` was before the feature), with
    the switch and without it, before a state directory ever existed and after; without the switch no directory appears and
    `load` next to one ignores it."""
    case = "ppo-n1" if algo == "ppo" else "trpo"
    c = cu.CASES[case]
    env = cu.make_env(1)
    model = cu.new_model(case, env, 48, full=48)
    model.learn(48)
    model.save(str(tmp_path / "before"))
    model._save_zip(str(tmp_path / "bare"))
    assert sorted(os.listdir(str(tmp_path))) == ["bare.zip", "before.zip"]
    os.environ["GRL_CHECKPOINT_STATE"] = "1"
    try:
        model.save(str(tmp_path / "with"))
    finally:
        del os.environ["GRL_CHECKPOINT_STATE"]
    model.save(str(tmp_path / "with"))                     # without the switch again, next to the directory
    assert sorted(os.listdir(str(tmp_path))) == ["bare.zip", "before.zip", "with.state", "with.zip"]
    members = []
    for name in ("before", "bare", "with"):
        with zipfile.ZipFile(str(tmp_path / (name + ".zip"))) as z:
            members.append([(i.filename, z.read(i.filename)) for i in z.infolist()])
    assert members[0] == members[1] == members[2]
    loaded = cu.model_class(algo).load(str(tmp_path / "with"), cu.make_env(1), **cu.load_kwargs(case, 48, 48))
    assert loaded.num_timesteps == 0 and loaded._resume is None
    model.engine.close(); loaded.engine.close()


def _params_words(model):
    return {k: np.asarray(v, np.float32).reshape(-1).view(np.uint32).copy() for k, v in model.get_parameters().items()}


def test_load_checkpoint_refuses_what_does_not_fit(emulation, tmp_path):
    from grasp_rl.sb import checkpoint
    PPO2, TRPO = cu.model_class("ppo"), cu.model_class("trpo")
    ppo = cu.new_model("ppo-n4", cu.make_env(4), 32, full=32)
    ppo.learn(32)
    p = str(tmp_path / "ppo")
    ppo.save(p)
    with pytest.raises(GrlError, match="no checkpoint state"):
        PPO2.load_checkpoint(p, cu.make_env(4))
    ppo.save_checkpoint(p)
    trpo = cu.new_model("trpo", cu.make_env(1), 16, full=16)
    trpo.learn(16)
    t = str(tmp_path / "trpo")
    trpo.save_checkpoint(t)
    ppo.engine.close(); trpo.engine.close()

    def refused(load, says, model_of):
        with pytest.raises(GrlError, match=says):
            load()
        model = model_of()                                   # the same zip, the same env, then the restore alone
        before = _params_words(model)
        with pytest.raises(GrlError, match=says):
            checkpoint.restore_state(model, model_of.path, required=True)
        after = _params_words(model)
        assert all(np.array_equal(before[k], after[k]) for k in before) and model._resume is None and model.num_timesteps == 0
        model.engine.close()

    # a TRPO checkpoint into PPO2: the state directory of the TRPO run next to a PPO2 zip
    import shutil
    mixed = str(tmp_path / "mixed")
    shutil.copy(p + ".zip", mixed + ".zip")
    shutil.copytree(t + ".state", mixed + ".state")
    model_of = lambda: PPO2.load(mixed, cu.make_env(4))
    model_of.path = mixed
    refused(lambda: PPO2.load_checkpoint(mixed, cu.make_env(4)), "checkpoint of a TRPO model loaded into PPO2", model_of)
    with pytest.raises(GrlError, match="checkpoint of a TRPO model loaded into PPO2"):
        PPO2.load_checkpoint(t, cu.make_env(1))              # ... and the TRPO checkpoint as it stands: refused before its zip is read
    # written with VecNormalize, loaded into an env without it
    model_of = lambda: PPO2.load(p, cu.make_env(4, normalize=False))
    model_of.path = p
    refused(lambda: PPO2.load_checkpoint(p, cu.make_env(4, normalize=False)), "written with VecNormalize", model_of)
    # another n_envs
    model_of = lambda: PPO2.load(p, cu.make_env(2))
    model_of.path = p
    refused(lambda: PPO2.load_checkpoint(p, cu.make_env(2)), "number of envs", model_of)
    # ... and what fits goes in
    again = PPO2.load_checkpoint(p, cu.make_env(4, start_episode=2))
    assert again.num_timesteps == 32 and again.n_updates == 4 and again._resume is not None
    again.engine.close()
