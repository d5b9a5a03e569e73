"""CPU: the cases of tests/test_gpu_physics_shapes.py reach what they are there for, shown on the
oracle alone, before anything runs on a GPU.

* every lane-mode and slot-width rollout (tests/physics_ref.py) sees a reset and a collision; their
  union sees ground, obstacle and drone-drone contacts, goals and truncations
* the max_speed = 0.7 points take both speed clamps, the default scalars at the same shapes none
* every threshold scene is left in place by a substeps = 0 step and its boundary runs through the
  128-float sample and nowhere else
* every damping value of the law-1 test keeps pow((double)(1 - d), h) at least 16 f64 ulps away from
  a float32 rounding midpoint, so the device's pow may differ from the host's in its last bits
* the instantiations named by the cases cover every LM x KS and LM x MSL pair
"""
from __future__ import annotations

import numpy as np
import pytest

from tests import physics_ref as pr

_ROLLOUTS: dict = {}


def _rollout(case):
    if case.tag not in _ROLLOUTS:
        _ROLLOUTS[case.tag] = pr.oracle_rollout(case)
    return _ROLLOUTS[case.tag]


@pytest.mark.parametrize("case", pr.LANE_CASES + pr.WIDTH_CASES, ids=lambda c: c.tag)
def test_rollout_sees_a_reset_and_a_collision(case):
    s = _rollout(case)
    assert s["reset"] > 0 and s["collision"] > 0, s


def test_rollouts_together_see_every_event():
    total = {}
    for case in pr.LANE_CASES + pr.WIDTH_CASES:
        pr.add_counts(total, _rollout(case))
    for k in ("ground", "obstacle", "pair", "reached", "trunc"):
        assert total[k] > 0, f"no {k} in any lane-mode or slot-width rollout"


@pytest.mark.parametrize("case", pr.SCALAR_CASES, ids=lambda c: c.tag)
def test_scalar_rollout_resets(case):
    assert _rollout(case)["reset"] > 0


@pytest.mark.parametrize("tag", pr.CLAMP_CASES)
def test_small_max_speed_takes_both_clamps(tag):
    s = _rollout(next(c for c in pr.SCALAR_CASES if c.tag == tag))
    assert s["speed_in"] > 0, "no drone with an action entered a step above max_speed"
    assert s["speed_out"] > 0, "no velocity of a live env was left above max_speed"


def test_default_scalars_take_no_clamp():
    """Why the clamp points exist: the lane-mode rollouts never exceed the default max_speed."""
    assert sum(_rollout(c)["speed_in"] + _rollout(c)["speed_out"] for c in pr.LANE_CASES) == 0


def test_scalar_points_cover_substeps_and_laws():
    cases = pr.SCALAR_CASES
    assert {c.substeps for c in cases} >= {0, 1, 5, 48, None}
    for n, _ in pr.SCALAR_SHAPES:
        assert {(c.substeps, c.law) for c in cases if c.n == n} >= {(s, law) for s in pr.SUBSTEPS for law in (0, 1)}
    varied = set()
    for c in cases:
        varied |= set(c.scalars) | set(c.phys)
    assert varied >= {"gravity", "gravity_comp", "substep_dt", "ground_contact_height", "drone_contact_radius",
                      "max_accel", "world_size", "goal_radius", "max_speed"}
    for c in cases:  # a goal_radius and a max_speed that no float holds exactly
        assert c.cfg["world_size"] <= 60.0
    assert any(float(np.float32(c.cfg["goal_radius"])) != c.cfg["goal_radius"] for c in cases)
    assert any(float(np.float32(c.cfg["max_speed"])) != c.cfg["max_speed"] for c in cases)


def test_cases_cover_every_instantiation_pair():
    """Every LM x KS and LM x MSL pair of the physics step kernel is named by a rollout case, and
    the four reset / observe shapes name four different (LM, KS, MSL)."""
    names = {c.kernel for c in pr.LANE_CASES + pr.WIDTH_CASES}
    for lm in (0, 1, 2):
        for ks in (0, 4, 9, 17):
            assert any(nm.startswith(f"swarm_kernel<0, 1, {ks}, ") and nm.endswith(f", {lm}>") for nm in names), (lm, ks)
        for msl in (0, 5, 9, 17):
            assert any(nm.endswith(f", {msl}, {lm}>") for nm in names), (lm, msl)
    aux = {pr.kernel_name(n, k, ms, m, kind=1) for n, k, ms, m, _ in pr.AUX_SHAPES}
    assert aux == {"swarm_kernel<1, 1, 9, 9, 1>", "swarm_kernel<1, 1, 17, 17, 2>", "swarm_kernel<1, 1, 0, 5, 0>",
                   "swarm_kernel<1, 1, 4, 0, 1>"}


@pytest.mark.parametrize("name", list(pr.SCENES))
def test_scene_straddles_its_threshold(name):
    from oracle import swarm_oracle as so
    case, scene, which = pr.build_scene(name)
    e, n = scene["pos"].shape[:2]
    assert n == case.n and 0 < int(scene["sample"].sum()) and e * n <= 8192
    st = pr.scene_state(scene)
    ns, out = so.step(case.cfg, st, np.zeros((e, n, 3), np.float32), physics=True, auto_reset=False, seed=pr.SEED)
    pr.check_scene(scene, st, ns, out, which)
    assert not out["reset"].any()


@pytest.mark.parametrize("h", [1.0 / 240.0, 1.0 / 120.0])
def test_law1_factor_is_far_from_rounding_midpoints(h):
    d = pr.damping_values(4096)
    assert d[:4].tolist() == [0.0, 1.0, 0.25, np.float32(0.999)]
    gap = pr.pow_midpoint_gap(d, h)
    assert gap.min() >= 16.0, f"damping {d[gap.argmin()]} is {gap.min()} f64 ulps from a float32 midpoint"
    fac = np.power((np.float32(1.0) - d).astype(np.float64), float(np.float32(h))).astype(np.float32)
    assert fac[0] == 1.0 and fac[1] == 0.0 and 0.0 < fac[3] < fac[2] < 1.0


def test_fast_velocities_straddle_max_speed():
    v = pr.fast_velocities(12, 24, 4.0)
    frac = float((pr.speed64(v) > 4.0).mean())
    assert 0.35 < frac < 0.65
