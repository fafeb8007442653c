"""Import-path alias of ``stable_baselines.trpo_mpi`` (``from stable_baselines.trpo_mpi import TRPO``)."""
from grasp_rl.sb.trpo import TRPO  # noqa: F401
