"""Import-path alias of ``stable_baselines.gail`` (``from stable_baselines.gail import ExpertDataset, generate_expert_traj``):
the expert-data half only -- what ``model.pretrain`` needs.  GAIL itself is not implemented."""
from grasp_rl.sb.expert import ExpertDataset, generate_expert_traj  # noqa: F401
