"""Model-level checkpoint and resume of PPO2 / TRPO on the MI355X: the procedure of tests/test_ppo_checkpoint_learn_host.py
(tests/ppo_checkpoint_util.py: its deterministic environment, run A = learn(full) with a save between engine.step and
engine.rewards, run B = a new process that restores and learns on; everything compared as raw words) on the real library."""
import pytest

import ppo_checkpoint_util as cu

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def plain_environment(monkeypatch):
    from grasp_rl.sb import trpo
    monkeypatch.setattr(trpo, "VF_BATCH", trpo.VF_BATCH)      # (model_class sets it; restored after the test)
    monkeypatch.delenv("GRL_CHECKPOINT_STATE", raising=False)
    monkeypatch.delenv("GRL_TUNE", raising=False)


@pytest.mark.parametrize("case", sorted(cu.CASES))
def test_resumed_run_equals_uninterrupted_run(tmp_path, case):
    c = cu.CASES[case]
    a, path = cu.run_a(case, tmp_path)
    assert a["counters"][0] == c["full"] and a["actions"].shape[:2] == (c["n"], c["full"] // c["n"] - c["save_at"])
    cu.assert_equal_runs(a, cu.run_b(case, path, tmp_path, None))


def test_plain_save_and_load_with_the_environment_switch(tmp_path):
    a, path = cu.run_a("ppo-n4-device_norm", tmp_path, how="save")
    cu.assert_equal_runs(a, cu.run_b("ppo-n4-device_norm", path, tmp_path, None, how="save"))


def test_learn_returns_then_save(tmp_path):
    case, T = "ppo-n4", 96
    c = cu.CASES[case]
    env = cu.make_env(c["n"])
    model = cu.new_model(case, env, 2 * T, full=2 * T)
    model.learn(2 * T)
    a = cu.result(model, env, T // c["n"])
    model.engine.close()
    cu.assert_equal_runs(a, cu.run_returned(case, tmp_path, None, T))
