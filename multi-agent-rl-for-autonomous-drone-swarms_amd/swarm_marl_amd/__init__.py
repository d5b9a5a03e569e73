"""swarm_marl_amd — MI355X-native vectorised drone-swarm step/observe/reward engine.

Host side of the C-ABI in include/swarm_mi355x.h.  `VecSwarm` is the batched tensor API;
`envs` holds the reference-compatible RLlib / Gymnasium classes; `CriticMLP` and `RolloutCollector`
(with `gaussian_logp` and `gae`) turn a device rollout into a PPO-ready batch; `PPOLearner` (with
`ppo_loss` and `masked_moments`) trains on it.  `AttentionPolicy` is the reference's attention actor
on the device, `AttentionActor` its trainable torch module.  `AgentValueMLP` (with `gae_agent`) is the
per-agent critic of the reference's multi-agent and single-agent PPO set-ups.  `Perturbation` (with
`noise_spec`) is the control delay, thrust noise and sensing noise of the domain-randomisation recipe.
`RolloutCollector(..., graph=True)` replays a whole fragment as one captured graph (`rollout_sample`,
`rollout_record`: the device-counter sampling and the fused per-step copies it is built on).
`ActorTrainer` trains the bf16 actor on the device (`PPOLearner(..., backend="hip")`).
"""
from .actor_train import ActorTrainer
from .attention import AttentionActor, AttentionPolicy
from .critic import CriticMLP
from .envs.common import DroneEnvConfig
from .perturbation import Perturbation, noise_spec
from .ppo import PPOLearner, masked_moments, ppo_loss
from .rollout import RolloutCollector, gae, gae_agent, gaussian_logp, rollout_record, rollout_sample
from .value import AgentValueMLP
from .vec_env import VecSwarm

__all__ = ["ActorTrainer", "AgentValueMLP", "AttentionActor", "AttentionPolicy", "CriticMLP", "DroneEnvConfig", "PPOLearner",
           "Perturbation", "RolloutCollector", "VecSwarm", "gae", "gae_agent", "gaussian_logp", "masked_moments",
           "noise_spec", "ppo_loss", "rollout_record", "rollout_sample"]
__version__ = "0.1.0"
