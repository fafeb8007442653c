from grasp_rl.sb.policies import Td3CnnPolicy as CnnPolicy  # noqa: F401
from grasp_rl.sb.policies import Td3LnCnnPolicy as LnCnnPolicy  # noqa: F401
from grasp_rl.sb.policies import Td3LnMlpPolicy as LnMlpPolicy  # noqa: F401
from grasp_rl.sb.policies import Td3MlpPolicy as MlpPolicy  # noqa: F401
