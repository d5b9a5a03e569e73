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

With `graph=True` the whole fragment is one captured graph, replayed by every
`collect()`: per step the policy in mean mode, `swarm_rollout_sample` (the Philox counter is read from
a device word the collector sets before the replay, plus the step index), `actuate` with a
perturbation, the env step and ONE `swarm_rollout_record` launch for every copy of the step, then the
critic, log-prob and GAE launches.  The fragments are bit for bit those of the eager collector with the
same seed and counter.  A keyed randomizer (`DomainRandomizer(keyed=True)`) is captured
too: its `after_step()` is one launch after each step's record launch, where the eager loop calls it.
Not with a generator-mode randomizer, env groups or packed_io batches.
"""
from __future__ import annotations

import ctypes

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


def rollout_sample(logits: torch.Tensor, actions: torch.Tensor, *, seed: int = 0, counter: int = 0,
                   counter_dev: torch.Tensor | None = None) -> torch.Tensor:
    """actions [..., A] = mean + exp(log_std) * N(0, 1) from logits [..., 2A] (swarm_rollout_sample):
    the actors' draw and arithmetic, so their logits give their sampled actions bit for bit.  The
    Philox counter is `counter`, plus the word of `counter_dev` (a one-element int64 device tensor,
    read when the kernel runs) if given.  One launch, async on the current stream."""
    if not isinstance(actions, torch.Tensor) or actions.dim() < 1 or actions.shape[-1] < 1:
        raise ValueError("actions must be a tensor [..., A]")
    adim = int(actions.shape[-1])
    lead = tuple(actions.shape[:-1])
    _check("actions", actions, lead + (adim,), _F32)
    _check("logits", logits, lead + (2 * adim,), _F32, actions.device)
    if counter_dev is not None:
        _check("counter_dev", counter_dev, (1,), (torch.int64,), actions.device)
    lib = nat.load_library()
    nat.check(lib.swarm_rollout_sample(logits.data_ptr(), actions.numel() // adim, adim, int(seed) & (2**64 - 1),
                                       None if counter_dev is None else counter_dev.data_ptr(),
                                       int(counter) & (2**64 - 1), actions.data_ptr(), _stream(actions.device)),
              lib, which="rollout")
    return actions


def rollout_record(pairs) -> None:
    """dst.copy_(src) for up to 8 (src, dst) pairs of contiguous device tensors of equal byte size, in
    one launch (swarm_rollout_record), async on the current stream; a pair whose dst is None is
    skipped.  The tensors must not overlap."""
    pairs = list(pairs)
    if len(pairs) > nat.ROLLOUT_MAX_SEGMENTS:
        raise ValueError(f"at most {nat.ROLLOUT_MAX_SEGMENTS} pairs per launch, got {len(pairs)}")
    rec = nat.SwarmRolloutRecord()
    dev = None
    for src, dst in pairs:
        if dst is None:
            continue
        for name, x in (("src", src), ("dst", dst)):
            if not isinstance(x, torch.Tensor) or not x.is_cuda or not x.is_contiguous():
                raise ValueError(f"{name} must be a contiguous device tensor")
        nbytes = src.numel() * src.element_size()
        if nbytes != dst.numel() * dst.element_size() or src.device != dst.device or (dev or src.device) != src.device:
            raise ValueError("src and dst must hold the same number of bytes on one device")
        dev = src.device
        seg = rec.segments[rec.count]
        seg.src, seg.dst, seg.bytes = src.data_ptr(), dst.data_ptr(), nbytes
        rec.count += 1
    if rec.count == 0:
        return
    lib = nat.load_library()
    nat.check(lib.swarm_rollout_record(ctypes.byref(rec), _stream(dev)), lib, which="rollout")


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

    graph=True: `collect()` replays one captured graph per mode (sampled, deterministic), captured at
    the mode's first call and again when a buffer it baked in has moved (`captures` counts them;
    weights loaded in place keep their graph).  `counter` is read and advanced as in eager mode.
    """

    def __init__(self, vec: VecSwarm, policy: PolicyMLP | AttentionPolicy, critic: CriticMLP | AgentValueMLP | None = None, *,
                 horizon: int,
                 gamma: float = 0.99, lam: float = 0.95, seed: int = 0, perturb=None, randomizer=None,
                 graph: bool = False):
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
        if graph:
            if randomizer is not None and not getattr(randomizer, "keyed", False):
                raise ValueError("graph=True does not take a randomizer: its after_step draws with a torch generator "
                                 "and allocates, which a replayed graph cannot do")
            if vec.groups != 1:
                raise ValueError(f"graph=True needs a VecSwarm with one env group, got {vec.groups}: a grouped step "
                                 "forks streams, the captured fragment is one chain on one stream")
            if vec.packed_io:
                raise ValueError("graph=True needs a device-resident batch: packed_io / mapped batches (the dict-API "
                                 "envs) are not supported")
        self.graph = bool(graph)
        self.captures = 0  # graphs captured so far (graph mode)
        self._graphs: dict = {}  # deterministic -> (key, CUDAGraph)
        self.vec, self.policy, self.critic = vec, policy, critic
        self.perturb, self.randomizer = perturb, randomizer
        self.horizon, self.gamma, self.lam, self.seed = t, float(gamma), float(lam), int(seed)
        self.counter = 0  # policy steps taken: the Philox counter of the next one
        kw = dict(device=vec.device)
        # graph mode: `counter` as the sample launches read it (two's complement of the u64)
        self._counter_dev = torch.zeros((1,), dtype=torch.int64, **kw) if graph else None
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
        if self.graph:
            return self._collect_graph(bool(deterministic))
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

    # ------------------------------------------------------------------ graph mode
    def _graph_key(self) -> tuple:
        """The device addresses (and switches) a captured fragment bakes in."""
        vec, per = self.vec, self.perturb
        owner = getattr(vec, "_eval_owner", None)
        if owner is not None and owner.fused:
            raise ValueError("graph=True cannot step an env with a fused EvalTracker attached: a captured step would "
                             "replay its capture-time update index (detach() it)")
        ts = [*vec.state_dict().values(), vec.obs, vec.reward, vec.terminated, vec.truncated, vec.env_done,
              vec.global_state, vec.dist_goal, vec.info_flags, vec.work, vec.env_cfg, vec.env_cfg_next,
              self.policy.weights, None if self.critic is None else self.critic.weights]
        key = [None if x is None else x.data_ptr() for x in ts]
        if per is not None:
            key += [bool(per.enabled), per.ring.data_ptr(), per.eff.data_ptr(), per.delay.data_ptr(),
                    per.thrust_noise_std.data_ptr(), per.position_noise_std.data_ptr(),
                    per.velocity_noise_std.data_ptr(), per.obstacle_distance_noise_std.data_ptr()]
        if self.randomizer is not None:  # keyed: the launch bakes in its seed and table (the records are above)
            key.append(self.randomizer.graph_key())
        return tuple(key)

    def _post(self) -> None:
        """What follows the steps of a fragment: values, log-probs, GAE."""
        if self.per_agent:
            self.critic.value(self.obs_block, out=self.value)
        elif self.critic is not None:
            self.critic.value(self.global_state, out=self.value)
        gaussian_logp(self.logits, self.actions, out=self.logp)
        gae(self.reward, self.value, self.terminated, self.truncated, self.env_done, self.valid, gamma=self.gamma,
            lam=self.lam, advantage=self.advantage, value_target=self.value_target, per_agent=self.per_agent)

    def _issue(self, deterministic: bool) -> None:
        """The launches of one fragment in graph mode, on the current stream."""
        vec, pol, T = self.vec, self.policy, self.horizon
        per = self.perturb if self.perturb is not None and self.perturb.enabled else None
        step = vec.step if per is None else per.step
        gs, rnd = self.global_state, self.randomizer

        def obs_row(t):  # the obs row step t - 1 leaves behind, or None
            if t < T:
                return self.obs[t]
            return self.obs_block[T] if self.per_agent else None

        rollout_record([(vec.active, self.valid[0]), (vec.obs, None if per is not None else self.obs[0]),
                        (vec.global_state, None if gs is None else gs[0])])
        if per is not None:
            per.sense(out=self.obs[0])
        for t in range(T):
            if deterministic:
                pol.forward(self.obs[t], logits=self.logits[t], actions=self.actions[t])
            else:
                pol.forward(self.obs[t], logits=self.logits[t])
                rollout_sample(self.logits[t], self.actions[t], seed=self.seed, counter=t, counter_dev=self._counter_dev)
            step(self.actions[t])
            nxt = obs_row(t + 1)
            rollout_record([(vec.reward, self.reward[t]), (vec.terminated, self.terminated[t]),
                            (vec.truncated, self.truncated[t]), (vec.env_done, self.env_done[t]),
                            (vec.active, self.valid[t + 1] if t + 1 < T else None),
                            (vec.obs, None if per is not None else nxt),
                            (vec.global_state, None if gs is None else gs[t + 1])])
            if rnd is not None:
                rnd.after_step()
            if per is not None and nxt is not None:
                per.sense(out=nxt)
        self._post()

    def _warm(self) -> None:
        """First eager launches of the kernels whose launchers set a function attribute
        (hipFuncSetAttribute: the actors and the value towers) and of this unit's, before they are
        captured.  They write only fragment buffers that the replay overwrites; the env step and
        `actuate` change state and are captured cold, as bench.py captures the step."""
        self.policy.forward(self.obs[0], logits=self.logits[0], actions=self.actions[0])
        rollout_sample(self.logits[0], self.actions[0], seed=self.seed, counter=0, counter_dev=self._counter_dev)
        rollout_record([(self.vec.reward, self.reward[0])])
        if self.perturb is not None and self.perturb.enabled:
            self.perturb.sense(out=self.obs[0])
        if self.randomizer is not None:  # rewrites what the records hold: the keyed draw repeats bit for bit
            self.randomizer.after_step()
        self._post()

    def _collect_graph(self, deterministic: bool) -> dict[str, torch.Tensor]:
        key = self._graph_key()
        held = self._graphs.get(deterministic)
        if held is None or held[0] != key:
            self._warm()
            g = torch.cuda.CUDAGraph()
            # capture issues nothing: the env state, the delay line and the counter stay as they are
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self._issue(deterministic)
            held = (key, g)
            self._graphs[deterministic] = held
            self.captures += 1
        if not deterministic:
            c = self.counter & (2**64 - 1)
            self._counter_dev.fill_(c - 2**64 if c >= 2**63 else c)  # eager, outside the graph
        held[1].replay()
        self.counter += self.horizon
        return self._batch
