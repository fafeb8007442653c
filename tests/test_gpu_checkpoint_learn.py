"""Model-level checkpoint and resume on the MI355X: the procedure of tests/test_checkpoint_learn_host.py (its deterministic
environment, run A = learn(2T) against run B = learn(T) -> save_checkpoint -> new process -> load_checkpoint -> learn(T,
reset_num_timesteps=False), everything compared as raw words) with SAC on the real library.  grasp_rl.synthetic.ReachGraspEnv
draws its episodes from one generator and cannot be constructed "at episode k", so the host file's environment is used."""
import pytest

import test_checkpoint_learn_host as host

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,device_norm", [(1, False), (4, True)])
def test_sac_checkpointed_run_equals_uninterrupted_run(tmp_path, n, device_norm):
    spec = {"algo": "sac", "n": n, "device_norm": device_norm, "lib": None}
    a = host.run_a(spec)
    assert a["counters"][0] == 2 * host.T and a["counters"][1] > 0
    host.assert_equal_runs(a, host.run_b(spec, tmp_path))
