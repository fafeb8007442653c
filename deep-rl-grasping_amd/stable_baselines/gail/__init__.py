"""Import-path alias of ``stable_baselines.gail`` (``from stable_baselines.gail import GAIL, ExpertDataset, generate_expert_traj``):
the expert data ``model.pretrain`` and ``GAIL`` read, and ``GAIL`` itself (grasp_rl/sb/gail.py: TRPO with a discriminator session on
the HIP engine)."""
from grasp_rl.sb.expert import ExpertDataset, generate_expert_traj  # noqa: F401
from grasp_rl.sb.gail import GAIL  # noqa: F401
