"""On-device centralized critic for the rollout loop: V(global_state).

The reference's CTDE model (CentralizedCriticModel, src/swarm_marl/training/models.py) values a
state with `value_model`, a TorchFC [256, 256] on `global_state` (width 6N + 3) with one output.
`CriticMLP` runs that MLP with the library's kernel (swarm_critic_forward, csrc/swarm_critic.hip)
directly on a VecSwarm's global_state tensor, or on a whole [T+1, E, G] rollout block:

    critic = CriticMLP.from_state_dict(policy_state, device="cuda")     # "value_model." prefix
    v = critic.value(vec.global_state)                                   # [E]

precision "bf16" (default): bf16 MFMA operands with f32 accumulation — a position of +-10 is
quantised to steps of 0.03-0.06, ~1e-2 absolute on values of order 1; "f32": f32 products and
sums, within summation-order rounding of an f32 learner's own forward.
"""
from __future__ import annotations

from . import _native as nat
from ._mlp import _ValueMLP


class CriticMLP(_ValueMLP):
    _packed_bytes, _pack, _forward = "swarm_critic_packed_bytes", "swarm_critic_pack", "swarm_critic_forward"
    _struct, _which, _input = nat.SwarmCritic, "critic", "global_state"

    @classmethod
    def from_state_dict(cls, sd, prefix: str = "value_model.", **kw) -> "CriticMLP":
        """The critic of a torch state dict (RLlib TorchFC under `prefix`: `_hidden_layers.{0,1}.
        _model.0.*`, `_logits._model.0.*`).  The layers are found by shape, not by name: the 2-D
        `*.weight` entries under the prefix that have a `*.bias`, chained in -> 256 -> 256 -> 1
        (TorchFC's own, unused value head next to the output layer is left out)."""
        return cls._from_dense(sd, prefix, f"under {prefix!r}", unless_extra="_value_branch", **kw)
