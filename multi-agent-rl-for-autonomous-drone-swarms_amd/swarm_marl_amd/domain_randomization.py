"""Per-episode domain randomisation on the device.

The reference ships configs/domain_randomization_v1.yaml (`enabled: false`, `apply_on_reset:
true`): per-episode scale factors for dynamics, actuation, sensing and environment parameters,
plus an out-of-distribution evaluation profile.  No reference code reads it,
so there is no reference behaviour to match beyond the file's own statement: "randomize dynamics
and sensing per episode reset".  This module applies the entries that map onto the swarm env's
parameters, as per-env parameter records (swarm_env_cfg_t), entirely on the device:

    dynamics.max_accel_scale        -> max_accel       = base * U(min, max)
    dynamics.max_speed_scale        -> max_speed
    dynamics.dt_scale               -> dt              (kinematic integrator only)
    environment.obstacle_radius_scale -> obstacle_radius
    environment.world_size_scale    -> world_size

Each env's NEXT episode parameters are drawn ahead (torch RNG on the device) into
`env_cfg_next`; the step kernel switches an env to them when it resets it, and `after_step()`
draws fresh ones for exactly the envs the step reset (mask from env_done, no host sync).  The
entries that are not scale factors of an env parameter are reported in `unsupported`, not silently
dropped: mass_scale has no counterpart (the kinematic env has no mass; the physics restatement has
no mass parameter); the actuation delay, thrust noise and sensing noise are applied by
`perturbation.Perturbation`, a layer before and after the step, not by this module.
`RolloutCollector(randomizer=...)` calls `after_step()` inside a fragment.

`DomainRandomizer(..., keyed=True)` is the second mode (csrc/swarm_dr.hip, C-ABI
`swarm_env_cfg_randomize`): an env's episode parameters are a pure function of (seed, global env index,
episode number) — Philox4x32-10 on the perturbation layer's counter layout, stream 3 — computed and
written as records by ONE launch, with no generator, no allocation and no host state.  The draws then do
not depend on the order of calls, on which envs reset before, on env groups or on `env_offset` shards;
`keyed_values` restates them on the host, so a logged (env, episode) gives its parameters back; and
`RolloutCollector(graph=True)` can capture `after_step()`.  The keyed launch writes only the record
fields that follow from the five randomised parameters: `max_steps`, `num_obstacles` and `num_drones`
stay what a curriculum (`curriculum.assign_stage`) or `set_env_config` made them.  Its base values are
the batch config's (`swarm_params_t`), also for envs whose stage set another world_size.
"""
from __future__ import annotations

import ctypes
from pathlib import Path
from typing import Any

import numpy as np
import torch

from . import _native as nat

SUPPORTED = {
    ("dynamics", "max_accel_scale"): "max_accel",
    ("dynamics", "max_speed_scale"): "max_speed",
    ("dynamics", "dt_scale"): "dt",
    ("environment", "obstacle_radius_scale"): "obstacle_radius",
    ("environment", "world_size_scale"): "world_size",
}


def load_dr_config(path: str | Path) -> dict[str, Any]:
    """The randomisation mapping from YAML (yaml.safe_load: data only) or JSON."""
    p = Path(path)
    text = p.read_text(encoding="utf-8")
    if p.suffix.lower() == ".json":
        import json
        cfg = json.loads(text)
    else:
        import yaml
        cfg = yaml.safe_load(text)
    if not isinstance(cfg, dict) or not isinstance(cfg.get("randomization"), dict):
        raise ValueError(f"no 'randomization' mapping in {p}")
    return cfg


def scale_ranges(dr_cfg: dict, profile: str = "train", physics: bool = False):
    """({param: (lo, hi)} of the supported uniform scale entries, [unsupported 'group.name']).
    profile 'ood' takes min/max from evaluation.out_of_distribution_profile where it names them."""
    if profile not in ("train", "ood"):
        raise ValueError(f"profile must be 'train' or 'ood', got {profile!r}")
    ood = ((dr_cfg.get("evaluation") or {}).get("out_of_distribution_profile") or {}) if profile == "ood" else {}
    ranges, unsupported = {}, []
    for group, entries in (dr_cfg.get("randomization") or {}).items():
        for name, spec in (entries or {}).items():
            param = SUPPORTED.get((group, name))
            spec = dict(spec or {})
            spec.update(ood.get(name) or {})
            if param is None or (physics and param == "dt") or spec.get("distribution", "uniform") != "uniform":
                unsupported.append(f"{group}.{name}")
                continue
            lo, hi = float(spec["min"]), float(spec["max"])
            if not (0.0 < lo <= hi):
                raise ValueError(f"{group}.{name}: need 0 < min <= max, got [{lo}, {hi}]")
            ranges[param] = (lo, hi)
    listed = {name for entries in (dr_cfg.get("randomization") or {}).values() for name in (entries or {})}
    unsupported += [f"evaluation.{name}" for name in ood if name not in listed]
    return ranges, unsupported


def sample_values(base: dict[str, float], ranges: dict, e: int, generator: torch.Generator,
                  device) -> dict[str, torch.Tensor]:
    """base[param] * U(lo, hi) per env, float64 [E] tensors on `device`."""
    out = {}
    for param in sorted(ranges):
        lo, hi = ranges[param]
        u = torch.rand((e,), generator=generator, dtype=torch.float64, device=device)
        out[param] = float(base[param]) * (lo + (hi - lo) * u)
    return out


KEYED_STREAM = 3  # the counter stream of the keyed draw (perturbation.py uses 0, 1 and 2)


def _philox4x32_10(c0, c1, c2, c3, k0: int, k1: int):
    """Philox4x32-10 on uint64 arrays holding 32-bit words; returns the four output words."""
    u64, m32 = np.uint64, np.uint64(0xFFFFFFFF)
    c = [np.asarray(x, u64) & m32 for x in (c0, c1, c2, c3)]
    k0, k1 = u64(k0 & 0xFFFFFFFF), u64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0 = u64(0xD2511F53) * c[0]
        p1 = u64(0xCD9E8D57) * c[2]
        c = [(p1 >> u64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> u64(32)) ^ c[3] ^ k1, p0 & m32]
        k0 = (k0 + u64(0x9E3779B9)) & m32
        k1 = (k1 + u64(0xBB67AE85)) & m32
    return c


def keyed_values(seed: int, env_index, episode, ranges: dict, base: dict) -> dict[str, np.ndarray]:
    """The keyed mode's five parameters of (global env index, episode number), float64 arrays of the
    broadcast shape of `env_index` and `episode` (both taken modulo 2^32), on the host: what
    swarm_env_cfg_randomize draws on the device, bit for bit (the arithmetic in include/swarm_mi355x.h).
    `ranges` {param: (lo, hi)} as `scale_ranges` gives it (a parameter it does not name keeps its base
    value), `base` {param: value} for the five of `_native.DR_PARAMS`."""
    seed = int(seed) & (2**64 - 1)
    g, ep = np.broadcast_arrays(np.asarray(env_index, np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF),
                                np.asarray(episode, np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF))
    zero = np.zeros_like(g)
    out, blocks = {}, {}
    for i, param in enumerate(nat.DR_PARAMS):
        b = np.float64(base[param])
        if param not in ranges:
            out[param] = np.full(g.shape, b, np.float64)
            continue
        lo, hi = (np.float64(x) for x in ranges[param])
        if i >> 2 not in blocks:
            blocks[i >> 2] = _philox4x32_10(g, zero + np.uint64((KEYED_STREAM << 30) | ((i >> 2) << 16)), ep, zero,
                                            seed & 0xFFFFFFFF, seed >> 32)
        x = blocks[i >> 2][i & 3]
        u = ((x >> np.uint64(8)).astype(np.float64) + np.float64(0.5)) * np.float64(2.0 ** -24)
        span = hi - lo
        out[param] = b * (lo + span * u)
    return out


class DomainRandomizer:
    """Per-episode parameter draws for a VecSwarm (see the module docstring).

    keyed=False (the default): the draws come from a torch generator, in call order.  keyed=True: the
    draws are keyed by (seed, global env, episode) and made by one native launch; the class then keeps
        env_cfg[e] = record(draw(episode[e])),  env_cfg_next[e] = record(draw(episode[e] + 1))
    across every reset that is followed by `after_step()` / `after_reset()`."""

    def __init__(self, vec, dr_cfg: dict | str | Path, *, seed: int = 0, profile: str = "train",
                 force: bool = False, keyed: bool = False):
        cfg = dr_cfg if isinstance(dr_cfg, dict) else load_dr_config(dr_cfg)
        self.vec = vec
        self.enabled = bool(cfg.get("enabled", False)) or force
        self.ranges, self.unsupported = scale_ranges(cfg, profile, physics=vec.dynamics == "physics")
        self.base = {p: float(getattr(vec.cfg, p)) for p in set(SUPPORTED.values())}
        self.keyed = bool(keyed)
        self.seed = int(seed)
        self._mask = None
        if not self.keyed:
            self.generator = torch.Generator(device=vec.device)
            self.generator.manual_seed(int(seed))
            return
        self.generator = None
        self.table = nat.SwarmDrTable()
        for i, param in enumerate(nat.DR_PARAMS):
            if param in self.ranges:
                self.table.lo[i], self.table.hi[i] = self.ranges[param]
                self.table.enabled[i] = 1
        self._seed_c = ctypes.c_uint64(self.seed & (2**64 - 1))
        self._randomize = vec.lib.swarm_env_cfg_randomize
        self._refs = (ctypes.byref(vec.params), ctypes.byref(self.table))

    def graph_key(self) -> tuple:
        """What a captured `after_step()` bakes in besides the env's buffers (keyed mode)."""
        return (self.keyed, self.enabled, self.seed & (2**64 - 1), bytes(self.table) if self.keyed else None)

    def _launch(self, dst: torch.Tensor | None, episode_add: int, mask_ptr: int | None, mask_bits: int) -> None:
        """One swarm_env_cfg_randomize launch over the whole batch on the current stream."""
        if dst is None:
            raise RuntimeError("the env has no per-env records yet: call begin() first")
        vec = self.vec
        rc = self._randomize(*self._refs, self._seed_c, vec.episode.data_ptr(), episode_add, mask_ptr, mask_bits,
                             dst.data_ptr(), vec._stream())
        if rc:
            nat.check(rc, vec.lib, which="dr")

    def sample(self) -> dict[str, torch.Tensor]:
        """Generator mode: a fresh draw per env.  Keyed mode: the values of every env's CURRENT episode
        (`keyed_values` of the episode numbers read back: a host synchronisation, for inspection)."""
        if self.keyed:
            vec = self.vec
            ep = vec.episode.cpu().numpy().view(np.uint32)
            g = int(vec.params.env_offset) + np.arange(vec.num_envs, dtype=np.int64)
            vals = keyed_values(self.seed, g, ep, self.ranges, self.base)
            return {p: torch.from_numpy(vals[p]).to(vec.device) for p in sorted(self.ranges)}
        return sample_values(self.base, self.ranges, self.vec.num_envs, self.generator, self.vec.device)

    def _begin_keyed(self, reset: bool):
        vec = self.vec
        # records are allocated where they are missing (uniform, or copies of the current ones), never
        # rewritten: a curriculum's max_steps / num_obstacles / num_drones stay
        if vec.env_cfg is None:
            vec.set_env_config()
        if vec.env_cfg_next is None:
            vec.set_env_config(next_episode=True,
                               env_mask=torch.zeros((vec.num_envs,), dtype=torch.uint8, device=vec.device))
        vec.join()
        self._launch(vec.env_cfg, 0, None, 0xFF)
        self._launch(vec.env_cfg_next, 1, None, 0xFF)
        if not reset:
            return None
        obs = vec.reset()
        self.after_reset()
        return obs

    def begin(self, reset: bool = True):
        """Start every env on its own draw and queue a different draw for its next episode.

        A device reset copies `env_cfg_next` into the current record (swarm_kernel.hip draw_env),
        so the first episode's draw goes into `next`, the reset switches it in, and a fresh draw
        then refills `next` — otherwise the first two episodes of every env would share one draw.
        reset=True performs that vec.reset() here and returns its obs; with reset=False the
        caller must reset and then call `after_reset()`.

        Keyed mode: records that do not exist yet are allocated (existing ones are never rewritten),
        the current ones become record(draw(episode)) and the next ones record(draw(episode + 1)); the
        reset and `after_reset()` follow as above."""
        if not self.enabled or not self.ranges:
            return self.vec.reset() if reset else None
        if self.keyed:
            return self._begin_keyed(reset)
        self.vec.set_env_config(**self.sample())  # current records exist before the first reset
        self.vec.set_env_config(next_episode=True, **self.sample())
        if not reset:
            return None
        obs = self.vec.reset()
        self.after_reset()
        return obs

    def after_reset(self, env_mask: torch.Tensor | None = None) -> None:
        """Fresh next-episode draws for the envs an explicit vec.reset(env_mask) just started
        (all if None): the reset consumed their queued draw."""
        if not self.enabled or not self.ranges:
            return
        if self.keyed:  # one launch: next = record(draw(episode + 1)) of the masked envs
            self.vec.join()
            self._launch(self.vec.env_cfg_next, 1, self.vec._mask_ptr(env_mask), 0xFF)
            return
        self.vec.set_env_config(next_episode=True, env_mask=env_mask, **self.sample())

    def after_step(self) -> None:
        """Fresh next-episode draws for the envs the last step reset (they started the drawn
        ones).  Device-only: the mask comes from env_done on the device."""
        if not self.enabled or not self.ranges:
            return
        self.vec.join()
        if self.keyed:
            # one launch over the batch, masked by env_done's RESET bit on the device; it allocates
            # nothing and repeats bit for bit (the draw depends on episode[e] only), so it can be captured
            self._launch(self.vec.env_cfg_next, 1, self.vec.env_done.data_ptr(), nat.ENV_RESET)
            return
        self._mask = (self.vec.env_done & nat.ENV_RESET) != 0
        self.vec.set_env_config(next_episode=True, env_mask=self._mask, **self.sample())
