"""What the network wrappers share (policy.py, attention.py, critic.py, value.py): the array helpers,
the tensor checks, the actors' forward / logits / act and the base of the two value towers."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _native as nat

_PRECISION = {"bf16": nat.POLICY_BF16, "f32": nat.POLICY_F32}


def _fp(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _np(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, np.float32)


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _check_rows(name: str, t, in_dim: int, device) -> int:
    """The row count of an input `t` [..., in_dim] of a network on `device`."""
    if not isinstance(t, torch.Tensor) or t.device != device or t.dtype != torch.float32:
        raise ValueError(f"{name} must be a float32 tensor on {device}")
    if t.dim() < 1 or t.shape[-1] != in_dim or not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous [..., {in_dim}], got {tuple(t.shape)}")
    return int(t.numel() // in_dim)


class _Actor:
    """forward / logits / act of an on-device actor.  The class names its library call (`_forward`)
    and its `nat.check` tag (`_which`); the constructor sets lib, _c, in_dim, out_dim and device."""
    _forward: str
    _which: str

    def forward(self, obs: torch.Tensor, *, logits: torch.Tensor | None = None,
                actions: torch.Tensor | None = None, sample: bool = False, seed: int = 0,
                counter: int = 0) -> None:
        rows = _check_rows("obs", obs, self.in_dim, self.device)
        for name, t, width in (("logits", logits, self.out_dim), ("actions", actions, self.out_dim // 2)):
            if t is not None and (t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous()
                                  or t.numel() != rows * width):
                raise ValueError(f"{name} must be a contiguous float32 tensor of {rows} x {width} on {self.device}")
        mode = nat.POLICY_ACT_SAMPLE if sample else nat.POLICY_ACT_MEAN
        rc = getattr(self.lib, self._forward)(ctypes.byref(self._c), obs.data_ptr(), rows,
                                              None if logits is None else logits.data_ptr(),
                                              None if actions is None else actions.data_ptr(), mode,
                                              int(seed) & (2**64 - 1), int(counter) & (2**64 - 1), _stream(self.device))
        nat.check(rc, self.lib, which=self._which)

    def logits(self, obs: torch.Tensor) -> torch.Tensor:
        out = torch.empty(obs.shape[:-1] + (self.out_dim,), dtype=torch.float32, device=self.device)
        self.forward(obs, logits=out)
        return out

    def act(self, obs: torch.Tensor, out: torch.Tensor | None = None, *, deterministic: bool = True,
            seed: int = 0, counter: int = 0) -> torch.Tensor:
        """Actions [..., out/2]: the Gaussian mean, or mean + exp(log_std) * N(0, 1) (Philox keyed by
        (seed, row, counter): every actor draws the same normals) with deterministic=False."""
        if out is None:
            out = torch.empty(obs.shape[:-1] + (self.out_dim // 2,), dtype=torch.float32, device=self.device)
        self.forward(obs, actions=out, sample=not deterministic, seed=seed, counter=counter)
        return out


class _ValueMLP:
    """An in -> 256 -> 256 -> 1 value tower on the device (CriticMLP, AgentValueMLP).  The class names
    its library calls (`_packed_bytes`, `_pack`, `_forward`), its handle struct (`_struct`), its
    `nat.check` tag (`_which`) and what its input is called in messages (`_input`)."""
    _packed_bytes: str
    _pack: str
    _forward: str
    _struct: type
    _which: str
    _input: str

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
        nb = int(getattr(self.lib, self._packed_bytes)(self.in_dim, prec))
        if nb < 0:
            nat.check(nb, self.lib, which=self._which)
        self.packed_host = np.zeros(nb, np.uint8)
        self.layers = [(w1, b1), (w2, b2), (w3, b3)]
        self._repack(self.layers)
        self.weights = torch.from_numpy(self.packed_host).to(self.device)  # caching allocator: 256-B aligned
        self._c = self._struct(self.in_dim, prec, self.weights.data_ptr())

    def _repack(self, layers) -> None:
        nat.check(getattr(self.lib, self._pack)(self.in_dim, _PRECISION[self.precision],
                                                *map(_fp, (a for wb in layers for a in wb)),
                                                self.packed_host.ctypes.data_as(ctypes.c_void_p)), self.lib, which=self._which)

    @classmethod
    def from_arrays(cls, w1, b1, w2, b2, w3, b3, **kw):
        return cls([(w1, b1), (w2, b2), (w3, b3)], **kw)

    @classmethod
    def _from_dense(cls, sd, start: str, where: str, unless_extra: str | None = None, **kw):
        """The tower among the dense layers of state dict `sd` whose names begin with `start`, found by
        shape: the 2-D `*.weight` entries that have a `*.bias`, chained in -> 256 -> 256 -> 1.  With
        more than three of them, those with `unless_extra` in the rest of their name are left out.
        `where` says in the error message where they were looked for."""
        h = nat.POLICY_HIDDEN
        dense = []
        for name, w in sd.items():
            if not (name.startswith(start) and name.endswith(".weight")) or len(w.shape) != 2:
                continue
            bias = sd.get(name[:-len("weight")] + "bias")
            if bias is not None and tuple(bias.shape) == (w.shape[0],):
                dense.append((name, _np(w), _np(bias)))
        if unless_extra is not None and len(dense) > 3:
            dense = [d for d in dense if unless_extra not in d[0][len(start):]]
        shapes = {n: tuple(w.shape) for n, w, _ in dense}
        last = [d for d in dense if d[1].shape == (1, h)]
        rest = [d for d in dense if d[1].shape != (1, h)]
        if len(dense) != 3 or len(last) != 1:
            raise ValueError(f"no in -> {h} -> {h} -> 1 dense chain {where}: found {shapes}")
        if rest[0][1].shape == (h, h) and rest[1][1].shape != (h, h):
            rest.reverse()  # otherwise the state dict's order (a 256-wide input: two square layers)
        if rest[0][1].shape[0] != h or rest[1][1].shape != (h, h):
            raise ValueError(f"no in -> {h} -> {h} -> 1 dense chain {where}: found {shapes}")
        return cls([(d[1], d[2]) for d in (rest[0], rest[1], last[0])], **kw)

    def load_layers(self, layers) -> None:
        """Replace the weights in place: `layers` = three (w, b) of the shapes this network was built
        with, re-packed and copied into the existing device blob on the current stream — the handle
        and `weights.data_ptr()` stay valid."""
        new = [(_np(w), _np(b).reshape(-1)) for w, b in layers]
        if len(new) != 3 or any(w.shape != ow.shape or b.shape != ob.shape for (w, b), (ow, ob) in zip(new, self.layers)):
            raise ValueError(f"expected 3 layers of the shapes {[w.shape for w, _ in self.layers]}")
        self._repack(new)
        self.weights.copy_(torch.from_numpy(self.packed_host))
        self.layers = new

    def value(self, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """V(x) [...]: one launch over every row of x [..., in_dim] (the critic's global_state, the
        per-agent tower's obs), async on the current stream."""
        rows = _check_rows(self._input, x, self.in_dim, self.device)
        if out is None:
            out = torch.empty(x.shape[:-1], dtype=torch.float32, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != torch.float32
              or not out.is_contiguous() or out.numel() != rows):
            raise ValueError(f"out must be a contiguous float32 tensor of {rows} elements on {self.device}")
        rc = getattr(self.lib, self._forward)(ctypes.byref(self._c), x.data_ptr(), rows, out.data_ptr(), _stream(self.device))
        nat.check(rc, self.lib, which=self._which)
        return out
