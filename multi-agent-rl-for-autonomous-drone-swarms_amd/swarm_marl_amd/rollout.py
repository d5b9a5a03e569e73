"""PPO-ready rollout fragments collected on the device.

`RolloutCollector` ties a `VecSwarm`, a `PolicyMLP` or `AttentionPolicy` and (optionally) a `CriticMLP` together: T
steps of policy + env step with every per-step quantity copied into preallocated [T, ...] buffers,
then one critic launch over the (T+1) x E recorded global states, one log-prob launch and one GAE
launch — no host synchronisation and no allocation after construction.

    col = RolloutCollector(vec, policy, critic, horizon=32)
    vec.reset()
    batch = col.collect()     # dict of views, overwritten by the next collect()

Return semantics: the value is per env, shared by its agents (the reference's
critic sees the same global_state for every agent of an env); any episode end — the agent's own
termination or truncation, or the env's `__all__` — stops the bootstrap, a truncation included
(the reference emits no observation or global state for a truncated agent, and the in-kernel
auto-reset has already replaced the state); only the fragment end (row T) bootstraps.  `valid[t]`
is the env's active mask before step t: an agent that ended earlier in a still-running episode
takes no step and gets zero advantage and target.  Without a critic the values are zero, so the
advantages (and targets) are the rewards-to-go discounted by gamma * lam, cut at episode ends.

With an `AgentValueMLP` as `critic` (the per-agent value tower of the reference's
multi-agent and single-agent PPO set-ups) the value is per agent, V(obs[t, e, n]): the observations
go into one [T+1, E, N, D] block (row T: the env's obs after the last step), one value launch runs
over the whole block and `gae_agent` reads value[t, e, n].  The bootstrap rules are the same; no
global_state is needed.

With `perturb=` (a `Perturbation`) the policy acts on what it sensed and the env is
given what the actuators did: obs[t] is `perturb.sense()` of the env's obs (row T of `obs_block`
too, for the per-agent critic) and the step goes through `perturb.step`; actions and logp stay the
policy's own, and global_state stays true (the centralized critic is privileged).  With
`randomizer=` (a `DomainRandomizer`) its `after_step()` runs after every step of the fragment, so
envs that reset inside one get fresh next-episode draws.  Both stay on the device.
"""
from __future__ import annotations

import torch

from . import _native as nat
from ._mlp import _stream
from .attention import AttentionPolicy
from .critic import CriticMLP
from .policy import PolicyMLP
from .value import AgentValueMLP
from .vec_env import VecSwarm


def _check(name: str, t, shape, dtypes, device=None) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or (device is not None and t.device != device):
        raise ValueError(f"{name} must be a tensor on {device or 'a GPU device'}")
    if t.dtype not in dtypes:
        raise ValueError(f"{name} has dtype {t.dtype}, expected one of {[str(d) for d in dtypes]}")
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous {tuple(shape)}, got {tuple(t.shape)}")


_F32 = (torch.float32,)
_U8 = (torch.uint8, torch.bool)


def gaussian_logp(logits: torch.Tensor, actions: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """RLlib TorchDiagGaussian.logp of actions [..., A] under logits [..., 2A] = [mean | log_std]
    (swarm_gaussian_logp): one launch, async on the current stream."""
    if not isinstance(actions, torch.Tensor) or actions.dim() < 1 or actions.shape[-1] < 1:
        raise ValueError("actions must be a tensor [..., A]")
    adim = int(actions.shape[-1])
    lead = tuple(actions.shape[:-1])
    _check("actions", actions, lead + (adim,), _F32)
    _check("logits", logits, lead + (2 * adim,), _F32, actions.device)
    if out is None:
        out = torch.empty(lead, dtype=torch.float32, device=actions.device)
    else:
        _check("out", out, lead, _F32, actions.device)
    lib = nat.load_library()
    rows = actions.numel() // adim
    nat.check(lib.swarm_gaussian_logp(logits.data_ptr(), actions.data_ptr(), rows, adim, out.data_ptr(),
                                      _stream(actions.device)), lib, which="critic")
    return out


def gae(reward: torch.Tensor, value: torch.Tensor, terminated: torch.Tensor, truncated: torch.Tensor,
        env_done: torch.Tensor, valid: torch.Tensor, *, gamma: float = 0.99, lam: float = 0.95,
        advantage: torch.Tensor | None = None, value_target: torch.Tensor | None = None, per_agent: bool = False):
    """(advantage, value_target) [T, E, N] of a fragment (swarm_gae; the loop in
    include/swarm_mi355x.h, bit for bit an f32 NumPy loop).  reward / terminated / truncated /
    valid [T, E, N], value [T+1, E], env_done [T, E] SWARM_ENV_* bits; flags uint8 or bool.
    per_agent=True: a per-agent value [T+1, E, N] (swarm_gae_agent).  value[t] of an invalid step and
    value[t+1] behind an invalid or done step are never read."""
    if not isinstance(reward, torch.Tensor) or reward.dim() != 3:
        raise ValueError("reward must be a tensor [T, E, N]")
    t, e, n = (int(s) for s in reward.shape)
    dev = reward.device
    _check("reward", reward, (t, e, n), _F32)
    _check("value", value, (t + 1, e, n) if per_agent else (t + 1, e), _F32, dev)
    for name, x in (("terminated", terminated), ("truncated", truncated), ("valid", valid)):
        _check(name, x, (t, e, n), _U8, dev)
    _check("env_done", env_done, (t, e), _U8, dev)
    if advantage is None:
        advantage = torch.empty((t, e, n), dtype=torch.float32, device=dev)
    if value_target is None:
        value_target = torch.empty((t, e, n), dtype=torch.float32, device=dev)
    _check("advantage", advantage, (t, e, n), _F32, dev)
    _check("value_target", value_target, (t, e, n), _F32, dev)
    lib = nat.load_library()
    fn, which = (lib.swarm_gae_agent, "value") if per_agent else (lib.swarm_gae, "critic")
    nat.check(fn(reward.data_ptr(), value.data_ptr(), terminated.data_ptr(), truncated.data_ptr(),
                 env_done.data_ptr(), valid.data_ptr(), t, e, n, float(gamma), float(lam),
                 advantage.data_ptr(), value_target.data_ptr(), _stream(dev)), lib, which=which)
    return advantage, value_target


def gae_agent(*args, **kw):
    """`gae` with a per-agent value [T+1, E, N]: gae(..., per_agent=True)."""
    return gae(*args, per_agent=True, **kw)


class RolloutCollector:
    """Collects fragments of `horizon` steps from `vec` under `policy` (a `PolicyMLP` or an
    `AttentionPolicy`: anything with their in_dim / out_dim / device and forward); see the module
    docstring.

    Buffers (attributes, and the dict `collect()` returns), G = 6N + 3:
      obs [T,E,N,D], logits [T,E,N,out], actions [T,E,N,out/2], logp / reward / advantage /
      value_target [T,E,N] f32, terminated / truncated / valid [T,E,N] bool, env_done [T,E] u8,
      global_state [T+1,E,G] and value [T+1,E] (row t: before step t; row T: after the last step).
    With an `AgentValueMLP` as `critic`: value [T+1,E,N], and obs is the first-T view of `obs_block`
    [T+1,E,N,D] (row T: the obs after the last step); global_state only if the env has one.
    """

    def __init__(self, vec: VecSwarm, policy: PolicyMLP | AttentionPolicy, critic: CriticMLP | AgentValueMLP | None = None, *,
                 horizon: int,
                 gamma: float = 0.99, lam: float = 0.95, seed: int = 0, perturb=None, randomizer=None):
        t = int(horizon)
        if t < 1:
            raise ValueError(f"horizon must be >= 1, got {horizon}")
        e, n, d = vec.num_envs, vec.num_drones, vec.obs_dim
        if policy.in_dim != d or policy.out_dim != 6:
            raise ValueError(f"policy maps {policy.in_dim} -> {policy.out_dim}, the env needs {d} -> 6 "
                             "(3-d Gaussian actions)")
        if policy.device != vec.device:
            raise ValueError(f"policy is on {policy.device}, the env on {vec.device}")
        g = 6 * n + 3
        self.per_agent = isinstance(critic, AgentValueMLP)
        if self.per_agent:
            if critic.in_dim != d or critic.device != vec.device:
                raise ValueError(f"the per-agent critic takes {critic.in_dim} inputs on {critic.device}, the env's obs "
                                 f"is {d} wide on {vec.device}")
        elif critic is not None:
            if vec.global_state is None:
                raise ValueError("a critic needs the env's global_state: VecSwarm(..., with_global_state=True)")
            if critic.in_dim != g or critic.device != vec.device:
                raise ValueError(f"critic takes {critic.in_dim} inputs on {critic.device}, the env's global_state "
                                 f"is {g} wide on {vec.device}")
        for name, hook in (("perturb", perturb), ("randomizer", randomizer)):
            if hook is not None and hook.vec is not vec:
                raise ValueError(f"{name} belongs to another VecSwarm than the collector's")
        self.vec, self.policy, self.critic = vec, policy, critic
        self.perturb, self.randomizer = perturb, randomizer
        self.horizon, self.gamma, self.lam, self.seed = t, float(gamma), float(lam), int(seed)
        self.counter = 0  # policy steps taken: the Philox counter of the next one
        kw = dict(device=vec.device)
        f32 = torch.float32
        out = policy.out_dim
        self.obs_block = torch.zeros((t + 1, e, n, d), dtype=f32, **kw) if self.per_agent else None
        self.obs = self.obs_block[:t] if self.per_agent else torch.zeros((t, e, n, d), dtype=f32, **kw)
        self.logits = torch.zeros((t, e, n, out), dtype=f32, **kw)
        self.actions = torch.zeros((t, e, n, out // 2), dtype=f32, **kw)
        self.logp = torch.zeros((t, e, n), dtype=f32, **kw)
        self.reward = torch.zeros((t, e, n), dtype=f32, **kw)
        self.terminated = torch.zeros((t, e, n), dtype=torch.bool, **kw)
        self.truncated = torch.zeros((t, e, n), dtype=torch.bool, **kw)
        self.valid = torch.zeros((t, e, n), dtype=torch.bool, **kw)
        self.advantage = torch.zeros((t, e, n), dtype=f32, **kw)
        self.value_target = torch.zeros((t, e, n), dtype=f32, **kw)
        self.env_done = torch.zeros((t, e), dtype=torch.uint8, **kw)
        self.global_state = torch.zeros((t + 1, e, g), dtype=f32, **kw) if vec.global_state is not None else None
        self.value = torch.zeros((t + 1, e, n) if self.per_agent else (t + 1, e), dtype=f32, **kw)
        self._batch = {k: getattr(self, k) for k in
                       ("obs", "logits", "actions", "logp", "reward", "terminated", "truncated", "valid",
                        "advantage", "value_target", "env_done", "global_state", "value")}

    def collect(self, *, deterministic: bool = False) -> dict[str, torch.Tensor]:
        """One fragment from the env's current state (reset the env before the first call).
        deterministic=True acts with the Gaussian mean (evaluation): logp is then the log-density
        at the mean."""
        vec, pol, per, rnd = self.vec, self.policy, self.perturb, self.randomizer
        step = vec.step if per is None else per.step
        for t in range(self.horizon):
            self.valid[t].copy_(vec.active)
            if per is None:
                self.obs[t].copy_(vec.obs)
            else:
                per.sense(out=self.obs[t])
            if self.global_state is not None:
                self.global_state[t].copy_(vec.global_state)
            pol.forward(self.obs[t], logits=self.logits[t], actions=self.actions[t], sample=not deterministic,
                        seed=self.seed, counter=self.counter)
            self.counter += 1
            _, reward, terminated, truncated, env_done = step(self.actions[t])
            self.reward[t].copy_(reward)
            self.terminated[t].copy_(terminated)
            self.truncated[t].copy_(truncated)
            self.env_done[t].copy_(env_done)
            if rnd is not None:
                rnd.after_step()
        if self.global_state is not None:
            self.global_state[self.horizon].copy_(vec.global_state)
        if self.per_agent:
            if per is None:
                self.obs_block[self.horizon].copy_(vec.obs)
            else:
                per.sense(out=self.obs_block[self.horizon])
            self.critic.value(self.obs_block, out=self.value)
        elif self.critic is not None:
            self.critic.value(self.global_state, out=self.value)
        gaussian_logp(self.logits, self.actions, out=self.logp)
        gae(self.reward, self.value, self.terminated, self.truncated, self.env_done, self.valid, gamma=self.gamma,
            lam=self.lam, advantage=self.advantage, value_target=self.value_target, per_agent=self.per_agent)
        return self._batch
