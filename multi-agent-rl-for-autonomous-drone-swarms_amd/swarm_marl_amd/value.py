"""On-device per-agent critic for the rollout loop: V(obs) of every agent row.

The reference's multi-agent, curriculum and single-agent PPO set-ups (build_multi_agent_ppo_config /
build_single_agent_ppo_config, src/swarm_marl/training/config_builders.py) use RLlib's default
TorchFC with fcnet_hiddens [256, 256], relu and vf_share_layers=False: next to the shared actor a
separate value tower obs -> 256 -> 256 -> 1, evaluated per agent on the agent's own observation.
`AgentValueMLP` runs that tower with the library's kernel (swarm_value_forward,
csrc/swarm_value.hip) directly on a VecSwarm's obs tensor, or on a whole [T+1, E, N, D] rollout
block:

    value = AgentValueMLP.from_state_dict(policy_state, device="cuda")   # the `_value_branch*` layers
    v = value.value(vec.obs)                                              # [E, N]

precision "bf16" (default): the actor kernel's design (weights resident in LDS, bf16 MFMA operands,
f32 accumulation) with a one-output last layer; "f32": f32 products and sums (the centralized
critic's f32 kernel at this width), within summation-order rounding of an f32 learner's forward.
"""
from __future__ import annotations

from . import _native as nat
from ._mlp import _ValueMLP


class AgentValueMLP(_ValueMLP):
    _packed_bytes, _pack, _forward = "swarm_value_packed_bytes", "swarm_value_pack", "swarm_value_forward"
    _struct, _which, _input = nat.SwarmValue, "value", "obs"

    @classmethod
    def from_state_dict(cls, sd, prefix: str = "", **kw) -> "AgentValueMLP":
        """The value tower of a torch state dict (RLlib TorchFC with vf_share_layers=False under
        `prefix`: `_value_branch_separate.{0,1}._model.0.*`, `_value_branch._model.0.*`).  The layers
        are found by shape among the dense entries under the prefix whose names start with
        `_value_branch` (the actor's `_hidden_layers` / `_logits` are left alone): the 2-D `*.weight`
        entries that have a `*.bias`, chained in -> 256 -> 256 -> 1."""
        start = prefix + "_value_branch"
        return cls._from_dense(sd, start, f"named {start!r}*", **kw)
