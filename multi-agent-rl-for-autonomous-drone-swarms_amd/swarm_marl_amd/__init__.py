"""swarm_marl_amd — MI355X-native vectorised drone-swarm step/observe/reward engine.

Host side of the C-ABI in include/swarm_mi355x.h.  `VecSwarm` is the batched tensor API;
`envs` holds the reference-compatible RLlib / Gymnasium classes; `CriticMLP` and `RolloutCollector`
(with `gaussian_logp` and `gae`) turn a device rollout into a PPO-ready batch.
"""
from .critic import CriticMLP
from .envs.common import DroneEnvConfig
from .rollout import RolloutCollector, gae, gaussian_logp
from .vec_env import VecSwarm

__all__ = ["CriticMLP", "DroneEnvConfig", "RolloutCollector", "VecSwarm", "gae", "gaussian_logp"]
__version__ = "0.1.0"
