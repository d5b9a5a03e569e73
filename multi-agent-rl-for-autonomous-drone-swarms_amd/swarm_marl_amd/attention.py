"""On-device attention actor: the reference's CentralizedCriticModel(use_attention=True) actor
(src/swarm_marl/training/models.py:104-137, scripts/train_attention.py) on a VecSwarm's observation
tensor, one fused launch per step (swarm_attn_policy_forward, csrc/swarm_attn.hip).

Each drone embeds its own state and its K neighbour blocks, attends once (one head) from itself to
its neighbours and feeds [own | context | obstacles] into the usual 256-256 trunk:

    pol = AttentionPolicy.from_state_dict(sd, neighbor_k=3, sensed_obstacles=4, device="cuda")
    acts = pol.act(vec.obs)                       # [E, N, 3]
    col = RolloutCollector(vec, pol, critic, horizon=32)

`AttentionPolicy` has `PolicyMLP`'s forward / logits / act and the attributes RolloutCollector and
PPOLearner use (in_dim, out_dim, device, precision).  `AttentionActor` is the trainable torch
module with the reference's structure and state_dict names, on nn.MultiheadAttention(32, 1).

precision "bf16" (default): f32 front end, bf16 MFMA trunk with f32 accumulation, the attention
out-projection folded into the trunk's first layer by the packer; "f32": the unfolded formulas in
f32 (the parity path).  Both draw `PolicyMLP`'s normals in sampled mode.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _native as nat
from ._mlp import _PRECISION, _Actor, _np

EMBED = nat.ATTN_EMBED

# the reference's parameter names -> shapes (the attention front end)
PARAM_SHAPES = {
    "neighbor_embed.0.weight": (EMBED, 4), "neighbor_embed.0.bias": (EMBED,),
    "own_embed.0.weight": (EMBED, 9), "own_embed.0.bias": (EMBED,),
    "attn_block.attn.in_proj_weight": (3 * EMBED, EMBED), "attn_block.attn.in_proj_bias": (3 * EMBED,),
    "attn_block.attn.out_proj.weight": (EMBED, EMBED), "attn_block.attn.out_proj.bias": (EMBED,),
}
# the trunk (RLlib TorchFC named `action_model`): two hidden layers and the logits layer
TRUNK_KEYS = tuple(f"action_model.{layer}._model.0.{part}"
                   for layer in ("_hidden_layers.0", "_hidden_layers.1", "_logits") for part in ("weight", "bias"))
STATE_DICT_KEYS = tuple(PARAM_SHAPES) + TRUNK_KEYS


def unpack_bf16_blob(blob: np.ndarray, out_dim: int) -> dict:
    """The folded matrices of a bf16 blob (the layout in include/swarm_mi355x.h), as float32:
    `A` [32,32], `c0` [32], `own_w` [32,9], `own_b`, `neighbor_w` [32,4], `neighbor_b`, and `w1`
    [256,64], the trunk's folded first layer in fragment column order (columns 0..31: F, column k
    carrying s[16 ((k >> 3) & 1) + 8 (k >> 4) + (k & 7)]; column 32 + t: the t-th of
    [own | obst | b1 + d])."""
    blob = np.ascontiguousarray(blob, np.uint8)
    w1_off = 131072 + 512 * out_dim + 1024 + 128
    fe_off = w1_off + 32768
    fe = blob[fe_off:fe_off + 1536 * 4].view(np.float32)
    frag = blob[w1_off:fe_off].view(np.uint16).reshape(8, 4, 2, 32, 8)  # [ob, ks, h, n, j]
    w1 = (frag.astype(np.uint32) << 16).view(np.float32).transpose(0, 3, 1, 2, 4).reshape(256, 64)  # [m, 16ks+8h+j]
    return dict(own_w=fe[0:288].reshape(32, 9), own_b=fe[288:320], neighbor_w=fe[320:448].reshape(32, 4),
                neighbor_b=fe[448:480], A=fe[480:1504].reshape(32, 32), c0=fe[1504:1536], w1=w1)


class AttentionPolicy(_Actor):
    """`params`: the reference's eight front-end arrays by name (`PARAM_SHAPES`); `trunk_layers`: three
    (w, b) of the shapes [256, 41 + 4 Ms], [256, 256], [out, 256]."""
    _forward, _which = "swarm_attn_policy_forward", "attn"

    def __init__(self, params, trunk_layers, *, neighbor_k: int, sensed_obstacles: int, device="cuda",
                 precision: str = "bf16"):
        if precision not in _PRECISION:
            raise ValueError(f"precision must be one of {sorted(_PRECISION)}, got {precision!r}")
        self.neighbor_k, self.sensed_obstacles = int(neighbor_k), int(sensed_obstacles)
        self.lib = nat.load_library()
        self.precision = precision
        self.device = torch.device(device)
        if len(trunk_layers) != 3 or np.ndim(trunk_layers[2][0]) != 2:
            raise ValueError("expected 3 trunk layers (two 256-unit relu hidden layers + logits)")
        self.out_dim = int(np.shape(trunk_layers[2][0])[0])
        self.in_dim = 9 + 4 * self.neighbor_k + 4 * self.sensed_obstacles
        prec = _PRECISION[precision]
        # the library names the limit that K, Ms or the logits width breaks
        nb = int(self.lib.swarm_attn_policy_packed_bytes(self.neighbor_k, self.sensed_obstacles, self.out_dim, prec))
        if nb < 0:
            nat.check(nb, self.lib, which="attn")
        self.params, self.layers = self._validated(params, trunk_layers)
        self.packed_host = np.zeros(nb, np.uint8)
        self._pack()
        self.weights = torch.from_numpy(self.packed_host).to(self.device)  # caching allocator: 256-B aligned
        self._c = nat.SwarmAttnPolicy(self.neighbor_k, self.sensed_obstacles, self.out_dim, prec,
                                      self.weights.data_ptr())

    def _validated(self, params, trunk_layers):
        missing = [k for k in PARAM_SHAPES if k not in params]
        if missing:
            raise ValueError(f"missing attention parameters {missing}")
        p = {k: _np(params[k]) for k in PARAM_SHAPES}
        for k, shape in PARAM_SHAPES.items():
            if p[k].shape != shape:
                raise ValueError(f"{k} has shape {p[k].shape}, expected {shape}")
        if len(trunk_layers) != 3:
            raise ValueError("expected 3 trunk layers (two 256-unit relu hidden layers + logits)")
        layers = [(_np(layer[0]), _np(layer[1]).reshape(-1)) for layer in trunk_layers]
        h = nat.POLICY_HIDDEN
        in1 = 9 + EMBED + 4 * self.sensed_obstacles
        want = [(h, in1), (h, h), (self.out_dim, h)]
        for (w, b), shape in zip(layers, want):
            if w.shape != shape or b.shape != (shape[0],):
                raise ValueError(f"trunk layers must have the shapes {want} (weights) with matching biases, got "
                                 f"{[(w.shape, b.shape) for w, b in layers]}")
        return p, layers

    def _pack(self) -> None:
        arrs = [self.params[k] for k in PARAM_SHAPES] + [a for wb in self.layers for a in wb]
        fp = ctypes.POINTER(ctypes.c_float)
        w = nat.SwarmAttnWeights(*(a.ctypes.data_as(fp) for a in arrs))
        nat.check(self.lib.swarm_attn_policy_pack(self.neighbor_k, self.sensed_obstacles, self.out_dim,
                                                  _PRECISION[self.precision], ctypes.byref(w),
                                                  self.packed_host.ctypes.data_as(ctypes.c_void_p)),
                  self.lib, which="attn")

    @classmethod
    def from_state_dict(cls, state_dict, **kw) -> "AttentionPolicy":
        """From a state_dict with the reference's names (`STATE_DICT_KEYS`: the attention front end
        and the `action_model` trunk); other entries (the critic's `value_model`) are ignored."""
        missing = [k for k in STATE_DICT_KEYS if k not in state_dict]
        if missing:
            raise ValueError(f"state_dict lacks {missing}")
        t = [state_dict[k] for k in TRUNK_KEYS]
        return cls({k: state_dict[k] for k in PARAM_SHAPES}, [(t[0], t[1]), (t[2], t[3]), (t[4], t[5])], **kw)

    def state_dict(self) -> dict:
        """The unfolded float32 parameters under the reference's names."""
        sd = {k: torch.from_numpy(v.copy()) for k, v in self.params.items()}
        for key, a in zip(TRUNK_KEYS, (a for wb in self.layers for a in wb)):
            sd[key] = torch.from_numpy(a.copy())
        return sd

    def load_params(self, params, trunk_layers) -> None:
        """Replace the weights in place: re-folded, re-packed and copied into the existing device blob
        on the current stream — the handle and `weights.data_ptr()` stay valid."""
        self.params, self.layers = self._validated(params, trunk_layers)
        self._pack()
        self.weights.copy_(torch.from_numpy(self.packed_host))


class _AttentionBlock(torch.nn.Module):
    def __init__(self, embed_dim: int):
        super().__init__()
        self.attn = torch.nn.MultiheadAttention(embed_dim, 1, batch_first=True)

    def forward(self, query, key, value):
        ctx, _ = self.attn(query, key, value, need_weights=False)
        return ctx.squeeze(1)


class _Dense(torch.nn.Module):
    """One trunk layer under RLlib SlimFC's parameter names (`_model.0.{weight,bias}`)."""

    def __init__(self, n_in: int, n_out: int, relu: bool):
        super().__init__()
        mods = [torch.nn.Linear(n_in, n_out)] + ([torch.nn.ReLU()] if relu else [])
        self._model = torch.nn.Sequential(*mods)

    def forward(self, x):
        return self._model(x)


class _Trunk(torch.nn.Module):
    def __init__(self, n_in: int, n_out: int, hidden: int):
        super().__init__()
        self._hidden_layers = torch.nn.Sequential(_Dense(n_in, hidden, True), _Dense(hidden, hidden, True))
        self._logits = _Dense(hidden, n_out, False)

    def forward(self, x):
        return self._logits(self._hidden_layers(x))


class AttentionActor(torch.nn.Module):
    """The reference's attention actor as a trainable torch module: `state_dict()` has exactly
    `STATE_DICT_KEYS`.  forward(obs [B, D]) -> logits [B, out]."""

    def __init__(self, neighbor_k: int, sensed_obstacles: int, out_dim: int):
        super().__init__()
        self.neighbor_k, self.sensed_obstacles = int(neighbor_k), int(sensed_obstacles)
        self.neighbor_embed = torch.nn.Sequential(torch.nn.Linear(4, EMBED), torch.nn.ReLU())
        self.own_embed = torch.nn.Sequential(torch.nn.Linear(9, EMBED), torch.nn.ReLU())
        self.attn_block = _AttentionBlock(EMBED)
        self.action_model = _Trunk(9 + EMBED + 4 * self.sensed_obstacles, int(out_dim), nat.POLICY_HIDDEN)

    @classmethod
    def from_policy(cls, policy: AttentionPolicy) -> "AttentionActor":
        actor = cls(policy.neighbor_k, policy.sensed_obstacles, policy.out_dim)
        actor.load_state_dict(policy.state_dict())
        return actor

    def forward(self, obs):
        k = self.neighbor_k
        own = obs[:, :9]
        nbrs = self.neighbor_embed(obs[:, 9:9 + 4 * k].reshape(-1, k, 4))
        ctx = self.attn_block(self.own_embed(own).unsqueeze(1), nbrs, nbrs)
        return self.action_model(torch.cat([own, ctx, obs[:, 9 + 4 * k:]], dim=1))

    def split_state(self):
        """(params, trunk_layers) as float32 NumPy arrays, the arguments of `AttentionPolicy.load_params`."""
        sd = {k: v.detach().cpu().numpy() for k, v in self.state_dict().items()}
        t = [sd[k] for k in TRUNK_KEYS]
        return {k: sd[k] for k in PARAM_SHAPES}, [(t[0], t[1]), (t[2], t[3]), (t[4], t[5])]
