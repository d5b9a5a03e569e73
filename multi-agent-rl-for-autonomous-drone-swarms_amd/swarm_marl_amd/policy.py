"""On-device actor inference for the rollout loop.

The reference's actor is RLlib's TorchFC (fcnet_hiddens [256, 256], relu;
src/swarm_marl/training/config_builders.py:53-56, models.py:75-81), exported by
scripts/export_onnx.py:120-141 to artifacts/policy.onnx.  `PolicyMLP` runs that MLP with the
library's MFMA kernel (swarm_policy_forward, csrc/swarm_policy.hip) directly on a VecSwarm's
observation tensor and writes the next action tensor in place, so a rollout step is two kernel
launches (policy, env step) with no host round trip:

    pol = PolicyMLP.from_onnx("artifacts/policy.onnx", device="cuda")
    acts = pol.act(vec.obs)            # [E, N, 3]: RLlib TorchDiagGaussian mean (deterministic)
    vec.step(acts)

precision "bf16" (default): bf16 MFMA operands with f32 accumulation (~1e-2 relative on the
logits); "f32": f32 MFMA (within summation-order rounding of the f32 graph); "f32x3": the f32
graph's accuracy on f16 MFMA — every operand split into f16 hi + lo, three products per term
(hi*hi + hi*lo + lo*hi, ~2^-21 relative each); obs / weights / activations within the f16 range
(a W1, b1, W2 or W3 entry that is not finite or rounds past 65504 is refused with ValueError, by the
constructor and by load_layers, which then keeps the old weights).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _native as nat
from ._mlp import _Actor, _fp
from .onnx_weights import mlp_layers, read_onnx

_PRECISION = {"bf16": nat.POLICY_BF16, "f32": nat.POLICY_F32, "f32x3": nat.POLICY_F32X3}


class PolicyMLP(_Actor):
    _forward, _which = "swarm_policy_forward", "policy"

    def __init__(self, layers, *, device="cuda", precision: str = "bf16"):
        if precision not in _PRECISION:
            raise ValueError(f"precision must be one of {sorted(_PRECISION)}, got {precision!r}")
        if len(layers) != 3:
            raise ValueError("expected 3 dense layers (two 256-unit relu hidden layers + logits)")
        (w1, b1, r1), (w2, b2, r2), (w3, b3, r3) = layers
        h = nat.POLICY_HIDDEN
        if not (r1 and r2 and not r3):
            raise ValueError("expected relu after the two hidden layers and none after the logits")
        if w1.shape[0] != h or w2.shape != (h, h) or w3.shape[1] != h:
            raise ValueError(f"hidden layers must be {h} wide, got {w1.shape}, {w2.shape}, {w3.shape}")
        self.lib = nat.load_library()
        self.in_dim, self.out_dim = int(w1.shape[1]), int(w3.shape[0])
        self.precision = precision
        self.device = torch.device(device)
        prec = _PRECISION[precision]
        nb = int(self.lib.swarm_policy_packed_bytes(self.in_dim, self.out_dim, prec))
        if nb < 0:
            nat.check(nb, self.lib, which="policy")
        host = np.zeros(nb, np.uint8)
        arrs = [np.ascontiguousarray(a, np.float32) for a in (w1, b1, w2, b2, w3, b3)]
        nat.check(self.lib.swarm_policy_pack(self.in_dim, self.out_dim, prec, *map(_fp, arrs),
                                             host.ctypes.data_as(ctypes.c_void_p)), self.lib, which="policy")
        self.packed_host = host
        self.weights = torch.from_numpy(host).to(self.device)  # caching allocator: 256-B aligned
        self._c = nat.SwarmPolicy(self.in_dim, self.out_dim, prec, 0, self.weights.data_ptr())
        self.layers = [(np.asarray(w, np.float32), np.asarray(b, np.float32)) for w, b, _ in layers]

    @classmethod
    def from_onnx(cls, path_or_bytes, **kw) -> "PolicyMLP":
        """Weights and topology from an exported actor (scripts/export_onnx.py output)."""
        return cls(mlp_layers(read_onnx(path_or_bytes)), **kw)

    @classmethod
    def from_arrays(cls, w1, b1, w2, b2, w3, b3, **kw) -> "PolicyMLP":
        return cls([(w1, b1, True), (w2, b2, True), (w3, b3, False)], **kw)

    def load_layers(self, layers) -> None:
        """Replace the weights in place: `layers` = three (w, b[, relu]) of the shapes this policy was
        built with, re-packed and copied into the existing device blob on the current stream — the
        handle and `weights.data_ptr()` stay valid."""
        arrs = [np.ascontiguousarray(a, np.float32) for layer in layers for a in (layer[0], np.reshape(layer[1], -1))]
        if len(layers) != 3 or any(a.shape != np.shape(old) for a, old in
                                   zip(arrs, (x for wb in self.layers for x in (wb[0], np.reshape(wb[1], -1))))):
            raise ValueError(f"expected 3 layers of the shapes {[w.shape for w, _ in self.layers]}")
        nat.check(self.lib.swarm_policy_pack(self.in_dim, self.out_dim, _PRECISION[self.precision], *map(_fp, arrs),
                                             self.packed_host.ctypes.data_as(ctypes.c_void_p)), self.lib, which="policy")
        self.weights.copy_(torch.from_numpy(self.packed_host))
        self.layers = [(arrs[2 * i].copy(), arrs[2 * i + 1].copy()) for i in range(3)]
