"""NumPy statement of the keyed domain-randomisation draw (the arithmetic in
include/swarm_mi355x.h, swarm_env_cfg_randomize), the yardstick of tests/test_dr_cpu.py and
tests/test_gpu_dr.py.  Independent of `swarm_marl_amd.domain_randomization.keyed_values`: the Philox
block comes from tests/perturb_ref.py (the oracle's Philox4x32-10, checked against the Random123
known answers in tests/test_oracle_cpu.py), the rest is written out per parameter.

Parameter i (0 world_size, 1 dt, 2 max_speed, 3 max_accel, 4 obstacle_radius) of global env g in
episode ep is word i & 3 of the block (g, agent 0 | block (i >> 2) << 16 | stream 3 << 30, ep, 0):
    u = ((x >> 8) + 0.5) 2^-24;  value = base_i * (lo_i + (hi_i - lo_i) * u)      float64, no FMA
A parameter without a range is base_i.
"""
from __future__ import annotations

import numpy as np

from tests.perturb_ref import _words

PARAMS = ("world_size", "dt", "max_speed", "max_accel", "obstacle_radius")
STREAM_DR = 3


def word(seed, g, episode, i) -> np.ndarray:
    """The Philox word (uint32-valued) parameter i draws from."""
    return np.asarray(_words(seed, g, 0, i >> 2, STREAM_DR, episode, 0)[i & 3])


def scales(seed, g, episode, ranges) -> dict:
    """{param: lo + (hi - lo) u} float64 for the parameters `ranges` names."""
    out = {}
    for i, name in enumerate(PARAMS):
        if name not in ranges:
            continue
        lo, hi = np.float64(ranges[name][0]), np.float64(ranges[name][1])
        n24 = (word(seed, g, episode, i).astype(np.uint64) >> np.uint64(8)).astype(np.float64)
        u = (n24 + np.float64(0.5)) * np.float64(2.0 ** -24)
        diff = hi - lo
        prod = diff * u
        out[name] = lo + prod
    return out


def values(seed, g, episode, ranges, base) -> dict:
    """{param: float64 array} for all five parameters."""
    g, episode = np.broadcast_arrays(np.asarray(g, np.int64) & 0xFFFFFFFF, np.asarray(episode, np.int64) & 0xFFFFFFFF)
    sc = scales(seed, g, episode, ranges)
    out = {}
    for name in PARAMS:
        b = np.float64(base[name])
        out[name] = b * sc[name] if name in sc else np.full(g.shape, b, np.float64)
    return out
