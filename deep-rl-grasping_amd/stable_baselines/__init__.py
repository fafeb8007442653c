"""Import-path alias: lets the reference's scripts (``import stable_baselines as sb`` in
train_stable_baselines.py:7, sb_helper.py:6, base_callbacks.py:11-14) run unmodified on top of the
MI355X engine.  Put ``deep-rl-grasping_amd/`` on PYTHONPATH *instead of* installing stable-baselines
(see INTEGRATION.md).  The SAC / TD3 / DQN / BDQ / PPO2 / TRPO / GAIL update paths are implemented.  DDPG, the fifth algorithm the
reference's SBPolicy names (sb_helper.py:166-173), cannot run in the reference either -- its policy `ddpgMlp` is never defined --
so it stays out of scope and says so, as do the algorithms the reference never selects."""
from grasp_rl.sb import logger  # noqa: F401
from grasp_rl.sb.ppo2 import PPO2  # noqa: F401
from grasp_rl.sb.sac import SAC  # noqa: F401
from grasp_rl.sb.td3 import TD3  # noqa: F401
from grasp_rl.sb.trpo import TRPO  # noqa: F401
from grasp_rl.sb.gail import GAIL  # noqa: F401

__version__ = "2.10.1+grasp_rl"


def _unsupported(name):
    class _Unsupported:
        def __init__(self, *a, **k):
            raise NotImplementedError("%s is outside the accelerated hot path (SAC / DQN / BDQ / PPO2 / TRPO); "
                                      "install stable-baselines itself to use it" % name)

        @classmethod
        def load(cls, *a, **k):
            raise NotImplementedError("%s is outside the accelerated hot path" % name)
    _Unsupported.__name__ = name
    return _Unsupported


DDPG, A2C, ACKTR = (_unsupported(n) for n in ("DDPG", "A2C", "ACKTR"))
try:
    from grasp_rl.sb.dqn import BDQ, DQN  # noqa: F401
except ImportError:       # pragma: no cover
    DQN, BDQ = _unsupported("DQN"), _unsupported("BDQ")
