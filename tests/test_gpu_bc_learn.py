"""Behaviour cloning learns on the MI355X: ReachGraspEnv(kind="vector"), an expert that commands the object's position, 200
episodes recorded through generate_expert_traj, SAC(MlpPolicy, layers [64, 64]).pretrain(n_epochs=20) with the defaults of
stable-baselines (learning rate 1e-4, Adam epsilon 1e-8, minibatches of 64), then the reference's evaluation loop over 200
fresh episodes (synthetic.evaluate_success).

The bar is not invented: the float64 restatement of tests/bc_util.py (RestatedPolicy) was trained on the SAME recorded dataset,
split and shuffles from the same initial parameters on the CPU and evaluated the same way -- success rate 1.000 (mean final
distance 0.0857; the untrained policy: 0.105, distance 0.691).  The engine must reach that rate minus 0.10: three standard
deviations of a 200-episode success estimate at the least favourable rate (3 * sqrt(0.25 / 200) = 0.106), which also covers a
different shuffle.  The untrained model must lie at least 0.3 below the trained one, so the test cannot pass trivially."""
import pytest

import bc_util as bu
from grasp_rl import synthetic
from grasp_rl.sb.sac import SAC
from stable_baselines.sac.policies import MlpPolicy

pytestmark = pytest.mark.gpu

RESTATED_SUCCESS = 1.000       # measured: module docstring


def test_pretrain_reaches_the_restatements_success_rate():
    L = bu.LEARN
    env, data = bu.record_reach_expert()
    assert data["obs"].shape == (15 * L["episodes"], 101)
    model = SAC(MlpPolicy, env, policy_kwargs={"layers": L["layers"]}, batch_size=L["batch_size"], buffer_size=1000, seed=L["seed"])
    before, _ = synthetic.evaluate_success(model, kind="vector", episodes=200)
    assert model.pretrain(bu.reach_dataset(data), n_epochs=L["n_epochs"]) is model
    after, dist = synthetic.evaluate_success(model, kind="vector", episodes=200)
    print("success rate: untrained %.3f, pretrained %.3f (mean final distance %.4f); restatement %.3f" % (before, after, dist, RESTATED_SUCCESS))
    assert after >= RESTATED_SUCCESS - 0.10, (after, RESTATED_SUCCESS)
    assert before <= after - 0.3, (before, after)
    assert model.num_timesteps == 0 and model.n_updates == 0
