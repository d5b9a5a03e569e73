"""Training the bf16 actor on the device (csrc/swarm_train.hip).

`ActorTrainer(policy)` holds float32 master weights of a `PolicyMLP(precision="bf16")` as
torch.nn.Parameters (for torch's Adam) and a training workspace.  Its forward is the policy's own
inference kernel, its backward swarm_policy_backward (bf16 MFMA operands, f32 accumulation), and
`push()` rebuilds the policy's device blob from the masters with swarm_policy_pack_device — in place,
so handles, pointers and captured graphs that read the blob stay valid:

    tr = ActorTrainer(policy)
    opt = torch.optim.Adam(tr.parameters(), lr=3e-4)
    logits = tr.logits(obs).requires_grad_(True)      # what the collector ran
    loss_of(logits).backward()
    tr.backward(obs, logits.grad)                      # fills the parameters' .grad
    opt.step(); tr.push()
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _native as nat
from ._mlp import _check_rows, _fp, _stream
from .policy import PolicyMLP

NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")  # the order of `masters` and of the C-ABI's arrays
STAGES = ("h1", "h2", "dz2", "dz1")


class ActorTrainer:
    def __init__(self, policy: PolicyMLP):
        if not isinstance(policy, PolicyMLP) or policy.precision != "bf16":
            raise ValueError("ActorTrainer needs a PolicyMLP of precision 'bf16'")
        self.policy, self.lib, self.device = policy, policy.lib, policy.device
        self.in_dim, self.out_dim = policy.in_dim, policy.out_dim
        self.masters = [torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(a, np.float32).copy()).to(self.device))
                        for wb in policy.layers for a in (wb[0], np.reshape(wb[1], -1))]
        self._rows = -1
        self._work = None
        self._reserve(0)
        self.push()

    def parameters(self):
        return list(self.masters)

    def _reserve(self, rows: int) -> None:
        """A workspace for backward calls of up to `rows` rows; the packer's transposed blobs (its
        head) move over from the old one."""
        if rows <= self._rows:
            return
        nb = int(self.lib.swarm_policy_train_workspace_bytes(self.in_dim, self.out_dim, rows))
        if nb < 0:
            nat.check(nb, self.lib, which="train")
        work = torch.empty(nb, dtype=torch.uint8, device=self.device)  # caching allocator: 256-B aligned
        if self._work is not None:
            head = int(self.lib.swarm_policy_train_workspace_bytes(self.in_dim, self.out_dim, 0))
            work[:head].copy_(self._work[:head])
        self._work, self._rows = work, rows

    def logits(self, obs: torch.Tensor) -> torch.Tensor:
        """`policy.logits(obs)`: the inference kernel on the blob `push()` wrote."""
        return self.policy.logits(obs)

    def push(self) -> None:
        """Masters -> the policy's device blob (and the backward's transposed blobs), one launch on the
        current stream, no host read.  `policy.weights` keeps its address."""
        nat.check(self.lib.swarm_policy_pack_device(self.in_dim, self.out_dim, *(p.data_ptr() for p in self.masters),
                                                    self.policy.weights.data_ptr(), self._work.data_ptr(),
                                                    _stream(self.device)), self.lib, which="train")

    def backward(self, obs: torch.Tensor, grad_logits: torch.Tensor, *, stages: bool = False):
        """Fill the masters' `.grad` (overwritten, not accumulated) from obs [..., D] and d loss / d logits
        [..., 2A] of the same rows.  obs must be finite.  With stages=True returns the kernel's h1, h2,
        dz2, dz1 as bf16 bit patterns in int16 tensors [rows, 256] (a dict), for tests."""
        rows = _check_rows("obs", obs, self.in_dim, self.device)
        if _check_rows("grad_logits", grad_logits, self.out_dim, self.device) != rows:
            raise ValueError(f"grad_logits must hold {rows} rows like obs")
        for p in self.masters:
            if p.grad is None:
                p.grad = torch.empty_like(p)  # every element is written below
        if rows == 0:
            for p in self.masters:
                p.grad.zero_()
            return {} if stages else None
        self._reserve(rows)
        out = {k: torch.empty((rows, nat.POLICY_HIDDEN), dtype=torch.int16, device=self.device) for k in STAGES} if stages else {}
        args = nat.SwarmPolicyBackwardArgs(
            self.policy.weights.data_ptr(), obs.data_ptr(), grad_logits.data_ptr(), self._work.data_ptr(),
            *(p.grad.data_ptr() for p in self.masters), *(out[k].data_ptr() if stages else None for k in STAGES),
            rows, self.in_dim, self.out_dim)
        nat.check(self.lib.swarm_policy_backward(ctypes.byref(args), _stream(self.device)), self.lib, which="train")
        return out if stages else None

    def sync_policy(self) -> None:
        """Refresh `policy.layers` (and its host copy of the blob) from the masters: one device-to-host
        copy.  The device blob is what the last `push()` wrote and is not touched."""
        flat = torch.cat([p.detach().reshape(-1) for p in self.masters]).cpu().numpy()
        arrs, at = [], 0
        for p in self.masters:
            n = p.numel()
            arrs.append(flat[at:at + n].reshape(tuple(p.shape)).copy())
            at += n
        nat.check(self.lib.swarm_policy_pack(self.in_dim, self.out_dim, nat.POLICY_BF16, *map(_fp, arrs),
                                             self.policy.packed_host.ctypes.data_as(ctypes.c_void_p)),
                  self.lib, which="policy")
        self.policy.layers = [(arrs[2 * i], arrs[2 * i + 1]) for i in range(3)]
