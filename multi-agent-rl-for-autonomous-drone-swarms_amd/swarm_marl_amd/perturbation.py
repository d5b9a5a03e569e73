"""Actuation and sensing perturbations on the device.

The other half of the reference's configs/domain_randomization_v1.yaml (domain_randomization.py
applies the uniform scale factors): a per-episode control delay, per-step thrust noise, and
per-step noise on what the agents sense.  They sit before and after the env step, not inside it,
so the step, its observation and every parity test are untouched:

    per = Perturbation(vec, "configs/domain_randomization_v1.yaml", seed=3, force=True)
    vec.reset()
    obs = per.sense()                  # what the policy sees; vec.obs stays the true one
    per.step(actions)                  # delay line + thrust noise, then vec.step on the result

Both halves are one HIP launch each (csrc/swarm_perturb.hip: swarm_actuate, swarm_sense), async on
the current stream, with no host synchronisation and no host state: the noise is Philox keyed by
(seed, global env index, agent, episode, step), the last two read from the env state on the device,
so it does not depend on the call history, on env groups or on env_offset shards, and an env that
resets (by itself or through vec.reset) draws a new delay and starts an empty delay line with no
host action.  The arithmetic is written out in include/swarm_mi355x.h; tests/perturb_ref.py
restates it in NumPy.
"""
from __future__ import annotations

import ctypes
from pathlib import Path
from typing import Any

import numpy as np
import torch

from . import _native as nat
from ._mlp import _stream
from .domain_randomization import load_dr_config

MAX_DELAY = nat.PERTURB_MAX_DELAY

# YAML entry -> spec key (all `distribution: normal`, mean 0: per-step noise with that std)
NOISE_ENTRIES = {
    ("actuation", "thrust_noise_std"): "thrust_noise_std",
    ("sensing", "position_noise_std"): "position_noise_std",
    ("sensing", "velocity_noise_std"): "velocity_noise_std",
    ("sensing", "obstacle_distance_noise_std"): "obstacle_distance_noise_std",
}
STD_KEYS = tuple(NOISE_ENTRIES.values())


def check_spec(spec: dict) -> dict:
    """A complete, validated spec from a partial one: delay_values / delay_probs (default [0] /
    [1]) and the four std keys (default 0).  Raises ValueError on a negative std, a delay outside
    0..7, empty or negative probs or |sum(probs) - 1| > 1e-6."""
    unknown = set(spec) - {"delay_values", "delay_probs", *STD_KEYS}
    if unknown:
        raise ValueError(f"unknown perturbation spec keys {sorted(unknown)}")
    out = {}
    for key in STD_KEYS:
        std = float(spec.get(key, 0.0))
        if not std >= 0.0 or std == float("inf"):
            raise ValueError(f"{key}: need a finite std >= 0, got {std}")
        out[key] = std
    values = [v for v in spec.get("delay_values", [0])]
    probs = [float(p) for p in spec.get("delay_probs", [1.0] if len(values) == 1 else [])]
    if not values or not probs or len(values) != len(probs):
        raise ValueError(f"control delay: need as many probs as values and at least one, got {values} / {probs}")
    if len(values) > MAX_DELAY + 1:
        raise ValueError(f"control delay: at most {MAX_DELAY + 1} values")
    if any(int(v) != v for v in values):
        raise ValueError(f"control delay: values must be whole steps, got {values}")
    values = [int(v) for v in values]
    if min(values) < 0 or max(values) > MAX_DELAY:
        raise ValueError(f"control delay: values must lie in 0..{MAX_DELAY}, got {values}")
    if any(not p >= 0.0 for p in probs):
        raise ValueError(f"control delay: negative prob in {probs}")
    if abs(sum(probs) - 1.0) > 1e-6:
        raise ValueError(f"control delay: probs sum to {sum(probs)}, not 1")
    out["delay_values"], out["delay_probs"] = values, probs
    return out


def delay_cum(probs) -> np.ndarray:
    """cum [count] f32: the float32 rounding of the float64 running sum, the last entry 1."""
    cum = np.cumsum(np.asarray(probs, np.float64)).astype(np.float32)
    cum[-1] = np.float32(1.0)
    return cum


def noise_spec(dr_cfg: dict, profile: str = "train"):
    """(spec, unsupported) of the actuation and sensing groups of a randomisation config.
    spec: delay_values, delay_probs and the four std keys (`check_spec`); unsupported: the entries
    of the two groups this layer has no counterpart for.  profile 'ood' takes the fields that
    evaluation.out_of_distribution_profile names, as `scale_ranges` does."""
    if profile not in ("train", "ood"):
        raise ValueError(f"profile must be 'train' or 'ood', got {profile!r}")
    ood = ((dr_cfg.get("evaluation") or {}).get("out_of_distribution_profile") or {}) if profile == "ood" else {}
    spec: dict[str, Any] = {}
    unsupported = []
    rnd = dr_cfg.get("randomization") or {}
    for group in ("actuation", "sensing"):
        for name, entry in (rnd.get(group) or {}).items():
            entry = dict(entry or {})
            entry.update(ood.get(name) or {})
            dist = entry.get("distribution")
            if (group, name) == ("actuation", "control_delay_steps") and dist in (None, "discrete"):
                spec["delay_values"] = list(entry.get("values") or [])
                spec["delay_probs"] = list(entry.get("probs") or [])
            elif (group, name) in NOISE_ENTRIES and dist in (None, "normal") and float(entry.get("mean", 0.0)) == 0.0:
                spec[NOISE_ENTRIES[(group, name)]] = float(entry["std"])
            else:
                unsupported.append(f"{group}.{name}")
    return check_spec(spec), unsupported


class Perturbation:
    """Control delay, thrust noise and sensing noise for a VecSwarm (see the module docstring).

    spec_or_cfg: a spec (`noise_spec`'s, or any part of one: {} perturbs nothing), a randomisation
    config (a dict with 'randomization') or the path of one.  A config's `enabled: false` switches
    the layer off unless force=True, like DomainRandomizer: `step` is then vec.step and `sense` a
    copy.  Per-env values start at the spec's and can be set with `set`.  max_delay: the longest
    delay `set(delay=...)` may ask for (default: the longest the spec lists); the delay line has
    max_delay + 1 slots of [E,N,3].
    """

    def __init__(self, vec, spec_or_cfg: dict | str | Path, *, seed: int = 0, profile: str = "train",
                 force: bool = False, max_delay: int | None = None):
        if vec.packed_io:
            raise ValueError("Perturbation needs a device-resident batch: packed_io batches (the dict-API envs) "
                             "are not supported")
        self.unsupported: list[str] = []
        enabled = True
        if isinstance(spec_or_cfg, dict) and "randomization" not in spec_or_cfg:
            spec = check_spec(spec_or_cfg)
        else:
            cfg = spec_or_cfg if isinstance(spec_or_cfg, dict) else load_dr_config(spec_or_cfg)
            spec, self.unsupported = noise_spec(cfg, profile)
            enabled = bool(cfg.get("enabled", False))
        self.vec, self.spec = vec, spec
        self.enabled = enabled or force
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        e, n = vec.num_envs, vec.num_drones
        listed = max(spec["delay_values"])
        self.max_delay = listed if max_delay is None else int(max_delay)
        if not listed <= self.max_delay <= MAX_DELAY:
            raise ValueError(f"max_delay must lie in {listed}..{MAX_DELAY}, got {max_delay}")
        kw = dict(device=vec.device)
        self.ring = torch.zeros((self.max_delay + 1, e, n, 3), dtype=torch.float32, **kw)
        self.eff = torch.zeros((e, n, 3), dtype=torch.float32, **kw)
        self.delay = torch.full((e,), -1, dtype=torch.int32, **kw)  # -1: draw per episode
        self.thrust_noise_std = torch.full((e,), spec["thrust_noise_std"], dtype=torch.float32, **kw)
        self.position_noise_std = torch.full((e,), spec["position_noise_std"], dtype=torch.float32, **kw)
        self.velocity_noise_std = torch.full((e,), spec["velocity_noise_std"], dtype=torch.float32, **kw)
        self.obstacle_distance_noise_std = torch.full((e,), spec["obstacle_distance_noise_std"], dtype=torch.float32, **kw)
        self._delays = torch.zeros((e,), dtype=torch.int32, **kw)
        self._sensed = None
        self.lib = nat.load_library()
        a = nat.SwarmActuateArgs()
        a.ring, a.delay_override = self.ring.data_ptr(), self.delay.data_ptr()
        a.thrust_noise_std = self.thrust_noise_std.data_ptr()
        a.step_count, a.episode = vec.step_count.data_ptr(), vec.episode.data_ptr()
        a.eff = self.eff.data_ptr()
        a.delays.count = len(spec["delay_values"])
        for i, (v, c) in enumerate(zip(spec["delay_values"], delay_cum(spec["delay_probs"]))):
            a.delays.values[i], a.delays.cum[i] = v, float(c)
        a.ring_slots, a.num_envs, a.num_drones = self.max_delay + 1, e, n
        a.seed, a.env_offset = self.seed, int(vec.params.env_offset)
        self._act = a
        q = nat.SwarmActuateArgs.from_buffer_copy(a)  # delays(): the delay draw alone
        q.actions = q.ring = q.eff = None
        q.delay_out = self._delays.data_ptr()
        self._query = q
        s = nat.SwarmSenseArgs()
        s.active = vec.active.data_ptr()
        s.position_noise_std = self.position_noise_std.data_ptr()
        s.velocity_noise_std = self.velocity_noise_std.data_ptr()
        s.obstacle_noise_std = self.obstacle_distance_noise_std.data_ptr()
        s.step_count, s.episode = vec.step_count.data_ptr(), vec.episode.data_ptr()
        s.seed, s.env_offset = self.seed, int(vec.params.env_offset)
        s.num_envs, s.num_drones = e, n
        s.neighbor_k, s.sensed_obstacles = int(vec.cfg.neighbor_k), int(vec.cfg.sensed_obstacles)
        self._sense = s

    def set(self, env_mask: torch.Tensor | None = None, *, delay=None, thrust_noise_std=None, position_noise_std=None,
            velocity_noise_std=None, obstacle_distance_noise_std=None) -> None:
        """Per-env values, a scalar or an [E] array each, for the masked envs (all if None); on the
        device, no host sync.  delay: a fixed control delay in 0..max_delay, or -1 to draw it per
        episode from the spec (device values above max_delay are clamped by the kernel).  They apply
        from the next `step` / `sense` on."""
        e, dev = self.vec.num_envs, self.vec.device
        if env_mask is not None:
            self.vec._check_tensor("env_mask", env_mask if env_mask.dtype != torch.bool else env_mask.view(torch.uint8),
                                   (e,), torch.uint8)
            env_mask = env_mask != 0
        for name, val in (("delay", delay), ("thrust_noise_std", thrust_noise_std),
                          ("position_noise_std", position_noise_std), ("velocity_noise_std", velocity_noise_std),
                          ("obstacle_distance_noise_std", obstacle_distance_noise_std)):
            if val is None:
                continue
            dst = getattr(self, name)
            if not (isinstance(val, torch.Tensor) and val.is_cuda):  # host values are range-checked
                host = torch.as_tensor(val)
                if name == "delay":
                    if host.is_floating_point() or (host.numel() and (int(host.min()) < -1 or int(host.max()) > self.max_delay)):
                        raise ValueError(f"delay must be whole steps in -1..{self.max_delay} (max_delay; -1: draw)")
                elif host.numel() and not bool((host >= 0).all() and torch.isfinite(host.double()).all()):
                    raise ValueError(f"{name}: need finite values >= 0")
                val = host
            t = val.to(device=dev, dtype=dst.dtype)
            if t.dim() == 0:
                t = t.expand(e)
            if tuple(t.shape) != (e,):
                raise ValueError(f"{name}: expected a scalar or shape ({e},), got {tuple(t.shape)}")
            if env_mask is None:
                dst.copy_(t)
            else:
                torch.where(env_mask, t, dst, out=dst)

    def actuate(self, actions: torch.Tensor) -> torch.Tensor:
        """eff [E,N,3] (a persistent buffer) for the policy's `actions` at the envs' current step:
        the delay line, then thrust noise (swarm_actuate).  Once per step, before it."""
        vec = self.vec
        vec._check_tensor("actions", actions, (vec.num_envs, vec.num_drones, 3), torch.float32)
        vec.join()
        self._act.actions = actions.data_ptr()
        nat.check(self.lib.swarm_actuate(ctypes.byref(self._act), _stream(vec.device)), self.lib, which="perturb")
        return self.eff

    def step(self, actions: torch.Tensor, action_mask: torch.Tensor | None = None, **kw):
        """`actuate`, then vec.step on the result; returns vec.step's tuple (its obs is the true one:
        `sense()` gives the noisy one)."""
        if not self.enabled:
            return self.vec.step(actions, action_mask, **kw)
        return self.vec.step(self.actuate(actions), action_mask, **kw)

    def sense(self, out: torch.Tensor | None = None) -> torch.Tensor:
        """The noisy observation [E,N,D] of the env's current vec.obs (swarm_sense), into `out` or a
        persistent buffer; vec.obs is not modified.  The same state senses the same."""
        vec = self.vec
        shape = (vec.num_envs, vec.num_drones, vec.obs_dim)
        if out is None:
            if self._sensed is None:
                self._sensed = torch.zeros(shape, dtype=torch.float32, device=vec.device)
            out = self._sensed
        else:
            vec._check_tensor("out", out, shape, torch.float32)
        vec.join()
        if not self.enabled:
            out.copy_(vec.obs)
            return out
        self._sense.obs, self._sense.out = vec.obs.data_ptr(), out.data_ptr()
        nat.check(self.lib.swarm_sense(ctypes.byref(self._sense), _stream(vec.device)), self.lib, which="perturb")
        return out

    def delays(self) -> torch.Tensor:
        """[E] int32 (a persistent buffer): every env's control delay in its current episode (0
        everywhere when disabled)."""
        if not self.enabled:
            return self._delays.zero_()
        self.vec.join()
        nat.check(self.lib.swarm_actuate(ctypes.byref(self._query), _stream(self.vec.device)), self.lib, which="perturb")
        return self._delays
