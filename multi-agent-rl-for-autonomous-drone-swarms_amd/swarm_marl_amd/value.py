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

import ctypes

import numpy as np
import torch

from . import _native as nat
from .critic import _fp, _np

_PRECISION = {"bf16": nat.POLICY_BF16, "f32": nat.POLICY_F32}


class AgentValueMLP:
    def __init__(self, layers, *, device="cuda", precision: str = "bf16"):
        if precision not in _PRECISION:
            raise ValueError(f"precision must be one of {sorted(_PRECISION)}, got {precision!r}")
        if len(layers) != 3:
            raise ValueError("expected 3 dense layers (two 256-unit relu hidden layers + the value)")
        (w1, b1), (w2, b2), (w3, b3) = [(_np(w), _np(b).reshape(-1)) for w, b in layers]
        h = nat.POLICY_HIDDEN
        if w1.ndim != 2 or w1.shape[0] != h or w2.shape != (h, h) or w3.shape != (1, h):
            raise ValueError(f"expected weights [{h}, in], [{h}, {h}], [1, {h}], got {w1.shape}, {w2.shape}, {w3.shape}")
        if b1.shape != (h,) or b2.shape != (h,) or b3.shape != (1,):
            raise ValueError(f"expected biases of {h}, {h} and 1 elements, got {b1.shape}, {b2.shape}, {b3.shape}")
        self.lib = nat.load_library()
        self.in_dim = int(w1.shape[1])
        self.precision = precision
        self.device = torch.device(device)
        prec = _PRECISION[precision]
        nb = int(self.lib.swarm_value_packed_bytes(self.in_dim, prec))
        if nb < 0:
            nat.check(nb, self.lib, which="value")
        host = np.zeros(nb, np.uint8)
        arrs = [w1, b1, w2, b2, w3, b3]
        nat.check(self.lib.swarm_value_pack(self.in_dim, prec, *map(_fp, arrs),
                                            host.ctypes.data_as(ctypes.c_void_p)), self.lib, which="value")
        self.packed_host = host
        self.weights = torch.from_numpy(host).to(self.device)  # caching allocator: 256-B aligned
        self._c = nat.SwarmValue(self.in_dim, prec, self.weights.data_ptr())
        self.layers = [(w1, b1), (w2, b2), (w3, b3)]

    @classmethod
    def from_arrays(cls, w1, b1, w2, b2, w3, b3, **kw) -> "AgentValueMLP":
        return cls([(w1, b1), (w2, b2), (w3, b3)], **kw)

    @classmethod
    def from_state_dict(cls, sd, prefix: str = "", **kw) -> "AgentValueMLP":
        """The value tower of a torch state dict (RLlib TorchFC with vf_share_layers=False under
        `prefix`: `_value_branch_separate.{0,1}._model.0.*`, `_value_branch._model.0.*`).  The layers
        are found by shape among the dense entries under the prefix whose names start with
        `_value_branch` (the actor's `_hidden_layers` / `_logits` are left alone): the 2-D `*.weight`
        entries that have a `*.bias`, chained in -> 256 -> 256 -> 1."""
        h = nat.POLICY_HIDDEN
        dense = []
        for name, w in sd.items():
            if not (name.startswith(prefix + "_value_branch") and name.endswith(".weight")) or len(w.shape) != 2:
                continue
            bias = sd.get(name[:-len("weight")] + "bias")
            if bias is not None and tuple(bias.shape) == (w.shape[0],):
                dense.append((name, _np(w), _np(bias)))
        shapes = {n: tuple(w.shape) for n, w, _ in dense}
        last = [d for d in dense if d[1].shape == (1, h)]
        rest = [d for d in dense if d[1].shape != (1, h)]
        if len(dense) != 3 or len(last) != 1:
            raise ValueError(f"no in -> {h} -> {h} -> 1 dense chain named {prefix + '_value_branch'!r}*: found {shapes}")
        if rest[0][1].shape == (h, h) and rest[1][1].shape != (h, h):
            rest.reverse()  # otherwise the state dict's order (a 256-wide input: two square layers)
        if rest[0][1].shape[0] != h or rest[1][1].shape != (h, h):
            raise ValueError(f"no in -> {h} -> {h} -> 1 dense chain named {prefix + '_value_branch'!r}*: found {shapes}")
        return cls([(d[1], d[2]) for d in (rest[0], rest[1], last[0])], **kw)

    def load_layers(self, layers) -> None:
        """Replace the weights in place: `layers` = three (w, b) of the shapes this tower was built
        with, re-packed and copied into the existing device blob on the current stream — the handle
        and `weights.data_ptr()` stay valid."""
        new = [(_np(w), _np(b).reshape(-1)) for w, b in layers]
        if len(new) != 3 or any(w.shape != ow.shape or b.shape != ob.shape for (w, b), (ow, ob) in zip(new, self.layers)):
            raise ValueError(f"expected 3 layers of the shapes {[w.shape for w, _ in self.layers]}")
        nat.check(self.lib.swarm_value_pack(self.in_dim, _PRECISION[self.precision], *map(_fp, (a for wb in new for a in wb)),
                                            self.packed_host.ctypes.data_as(ctypes.c_void_p)), self.lib, which="value")
        self.weights.copy_(torch.from_numpy(self.packed_host))
        self.layers = new

    # ------------------------------------------------------------------ forward
    def _check_obs(self, obs: torch.Tensor) -> int:
        if not isinstance(obs, torch.Tensor) or obs.device != self.device or obs.dtype != torch.float32:
            raise ValueError(f"obs must be a float32 tensor on {self.device}")
        if obs.dim() < 1 or obs.shape[-1] != self.in_dim or not obs.is_contiguous():
            raise ValueError(f"obs must be contiguous [..., {self.in_dim}], got {tuple(obs.shape)}")
        return int(obs.numel() // self.in_dim)

    def value(self, obs: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """V(obs) [...]: one launch over every row of obs [..., in_dim], async on the current stream."""
        rows = self._check_obs(obs)
        if out is None:
            out = torch.empty(obs.shape[:-1], dtype=torch.float32, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != torch.float32
              or not out.is_contiguous() or out.numel() != rows):
            raise ValueError(f"out must be a contiguous float32 tensor of {rows} elements on {self.device}")
        rc = self.lib.swarm_value_forward(ctypes.byref(self._c), obs.data_ptr(), rows, out.data_ptr(),
                                          torch.cuda.current_stream(self.device).cuda_stream)
        nat.check(rc, self.lib, which="value")
        return out
