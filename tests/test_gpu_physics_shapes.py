"""GPU: the physics half (DYN = 1) of the generic swarm_kernel at every lane mode, every K / Ms
register width, off the default scalars and at its thresholds, against the f64 oracle.

Every case steps a VecSwarm(dynamics="physics", kernel_path="generic") and oracle.swarm_oracle side
by side, the oracle fed the device state before each step: observations, state (damping included),
terminated / truncated, env_done bits, dist_goal, global_state and info flags bit-exact, rewards
within the project's contract of 1e-5 absolute (world_size <= 60 keeps |r| < 64).
Every case asserts the swarm_kernel<0, 1, KS, MSL, LM> instantiation it is meant to run.

A  lane modes: 9 auto-reset steps at N = 1 ... 512, env_offset 7, 15 % of the actions masked off,
   alternating damping laws; the reset before and an observe() after go through the aux kernel
B  slot widths: the same rollout at N = 24, 32, 40, 100 for eight (K, Ms, M), K > N - 1, K = 0,
   Ms = 0 and M = 0 among them: every LM x KS and LM x MSL pair of the step and the aux kernel
C  scalars off the defaults at N = 16, 33, 100: gravity, its compensation, the substep, both contact
   sizes, world, max_accel, goal_radius and max_speed; substeps 0 / 1 / 5 / 48 under both damping
   laws; max_speed = 0.7 takes the substep clamp and the observation clamp
D  damping law 1: one step with damping 0, 1, 0.25, 0.999 and drawn values; every value keeps the
   host's pow at least 16 f64 ulps from a float32 rounding midpoint (checked on the host alone)
E  thresholds ulp by ulp with substeps = 0: ground height, goal radius (strict < in f64), obstacle
   contact and pair contact, at N = 16, 24, 40, 100 and (contacts) N = 16 with K = 0
F  masked reset(), set_state() velocities of which half exceed max_speed, observe() with and
   without a mask, at four (N, K, Ms, M)

What each case must reach (resets, contacts of every kind, goals, truncations, clamps, straddled
thresholds) is asserted from the oracle's outputs, and on the CPU by tests/test_physics_scenes_cpu.py.
Every case prints its largest reward error (pytest -s); DESIGN.md §5 tabulates them.

Measured on an MI355X (157 cases, 6 s): largest reward error 1.91e-6 (the f32 rounding of a goal
reward near 50) against the 1e-5 bound, everything else bit-exact.  Kernel mutations and which
cases each fails: DESIGN.md §5.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import mixed_ref as mr
from tests import physics_ref as pr
from tests.helpers import vec_state_numpy

pytestmark = pytest.mark.gpu

REWARD_TOL = 1e-5  # absolute, against the f64 oracle
STATE = ("pos", "vel", "goal", "obst", "active", "step", "episode", "damping")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _make(dev, case, e, auto_reset):
    from swarm_marl_amd import VecSwarm
    vec = VecSwarm(e, case.raw, device=dev, dynamics="physics", kernel_path="generic", with_infos=True,
                   with_global_state=True, auto_reset=auto_reset, seed=pr.SEED, env_offset=pr.ENV_OFFSET,
                   physics=case.physics)
    assert vec.kernel_name() == case.kernel, f"{case.tag}: {vec.kernel_name()} is not {case.kernel}"
    return vec


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what} differs from the oracle at {bad[:5].tolist()} (of {len(bad)})")


def _compare_state(vec, ns, tag):
    got = vec_state_numpy(vec)
    for k in STATE:
        _same(got[k], ns[k], f"{tag}: state {k}")


def _compare_view(vec, obs, dist, gs, tag, rows=None):
    """obs / dist_goal / global_state of the envs `rows` (all if None)."""
    sel = slice(None) if rows is None else rows
    _same(vec.obs.cpu().numpy()[sel], obs[sel], f"{tag}: obs")
    _same(vec.dist_goal.cpu().numpy()[sel], dist[sel], f"{tag}: dist_goal")
    _same(vec.global_state.cpu().numpy()[sel], gs[sel], f"{tag}: global_state")


def _compare_step(vec, ns, out, tag) -> float:
    """One step against the oracle: everything but the reward bitwise; returns the reward error."""
    _compare_view(vec, out["obs"], out["dist_goal"], out["global_state"], tag)
    _same(vec.terminated.cpu().numpy(), out["terminated"], f"{tag}: terminated")
    _same(vec.truncated.cpu().numpy(), out["truncated"], f"{tag}: truncated")
    bits = out["term_all"].astype(np.uint8) | (out["trunc_all"].astype(np.uint8) << 1) | \
        (out["reset"].astype(np.uint8) << 2)
    _same(vec.env_done.cpu().numpy(), bits, f"{tag}: env_done")
    _same(vec.info_flags.cpu().numpy(), mr.info_flags(out), f"{tag}: info_flags")
    _compare_state(vec, ns, tag)
    err = float(np.abs(vec.reward.cpu().numpy().astype(np.float64) - out["reward"]).max())
    assert err <= REWARD_TOL, f"{tag}: reward error {err} > {REWARD_TOL}"
    return err


def _compare_observe(vec, cfg, mask, tag):
    """observe() of the current state against so.observe; rows outside the mask stay as poisoned."""
    from oracle import swarm_oracle as so
    st = vec_state_numpy(vec)
    before = [t.clone() for t in vec.state_dict().values()]
    for t in (vec.obs, vec.dist_goal, vec.global_state):
        t.fill_(float("nan"))
    vec.observe(mask)
    torch.cuda.synchronize()
    sel = np.ones(vec.num_envs, bool) if mask is None else mask.cpu().numpy().astype(bool)
    obs = so.observe(cfg, st["pos"], st["vel"], st["goal"], st["obst"], physics=True)
    _compare_view(vec, obs, so.norm1d(st["goal"][:, None, :] - st["pos"]),
                  so.global_state(st["pos"], st["vel"], st["goal"]), tag, sel)
    for t in (vec.obs, vec.dist_goal, vec.global_state):
        assert bool(torch.isnan(t[torch.as_tensor(~sel)]).all()), f"{tag}: observe wrote outside its mask"
    for (name, x), y in zip(vec.state_dict().items(), before):
        assert torch.equal(x, y), f"{tag}: observe changed state {name}"
    return obs


def _step(vec, dev, a, has):
    vec.step(torch.as_tensor(a).to(dev), None if has is None else torch.as_tensor(has).to(dev))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ A - C. rollouts
def _rollout(dev, case):
    from oracle import swarm_oracle as so
    cfg = case.cfg
    kw = dict(physics=True, seed=pr.SEED, env_offset=pr.ENV_OFFSET)
    vec = _make(dev, case, case.e, True)
    st0 = vec_state_numpy(vec)
    vec.reset()
    torch.cuda.synchronize()
    ns, ro = so.reset_device(cfg, st0, **kw)
    _compare_view(vec, ro["obs"], ro["dist_goal"], ro["global_state"], f"{case.tag} reset")
    _compare_state(vec, ns, f"{case.tag} reset")
    total, err = {}, 0.0
    for t in range(pr.STEPS):
        a, has = pr.actions(case, t)
        st = vec_state_numpy(vec)
        _step(vec, dev, a, has)
        ns, out = so.step(cfg, st, a, has, auto_reset=True, **kw)
        err = max(err, _compare_step(vec, ns, out, f"{case.tag} t={t}"))
        pr.add_counts(total, pr.step_counts(cfg, st, a, has, ns, out))
    _compare_observe(vec, cfg, None, f"{case.tag} observe")
    total["err"] = err
    print(f"\n[physics-shapes] {case.tag}: {vec.kernel_name()} reward max|err| {err:.3e} | "
          + " ".join(f"{k} {total[k]}" for k in pr.COUNTS))
    return total


_DONE: dict = {}


def _rollout_once(dev, case):
    """One rollout per session: the union test reads every lane-mode and slot-width case."""
    if case.tag not in _DONE:
        try:
            _DONE[case.tag] = _rollout(dev, case)
        except AssertionError as exc:
            _DONE[case.tag] = exc
    if isinstance(_DONE[case.tag], AssertionError):
        raise _DONE[case.tag]
    return _DONE[case.tag]


@pytest.mark.parametrize("case", pr.LANE_CASES, ids=lambda c: c.tag)
def test_lane_modes_vs_oracle(dev, case):
    s = _rollout_once(dev, case)
    assert s["reset"] > 0 and s["collision"] > 0, s


@pytest.mark.parametrize("case", pr.WIDTH_CASES, ids=lambda c: c.tag)
def test_slot_widths_vs_oracle(dev, case):
    s = _rollout_once(dev, case)
    assert s["reset"] > 0 and s["collision"] > 0, s


def test_rollouts_together_see_every_event(dev):
    total = {}
    for case in pr.LANE_CASES + pr.WIDTH_CASES:
        pr.add_counts(total, _rollout_once(dev, case))
    for k in ("ground", "obstacle", "pair", "reached", "trunc"):
        assert total[k] > 0, f"no {k} in any lane-mode or slot-width rollout"


@pytest.mark.parametrize("case", pr.SCALAR_CASES, ids=lambda c: c.tag)
def test_scalars_off_the_defaults_vs_oracle(dev, case):
    s = _rollout_once(dev, case)
    assert s["reset"] > 0
    if case.tag in pr.CLAMP_CASES:
        assert s["speed_in"] > 0, "no drone with an action entered a step above max_speed"
        assert s["speed_out"] > 0, "no velocity of a live env was left above max_speed"


# ------------------------------------------------------------------ D. damping law 1
@pytest.mark.parametrize("h", [1.0 / 240.0, 1.0 / 120.0], ids=["h240", "h120"])
@pytest.mark.parametrize("n,e", [(16, 16), (40, 8), (100, 4)])
def test_law1_damping_edges(dev, n, e, h):
    from oracle import swarm_oracle as so
    case = pr.Case(f"law1-N{n}", n, e, law=1, max_steps=50, phys=dict(substep_dt=h))
    cfg = case.cfg
    damping = pr.damping_values(e * n, seed=n).reshape(e, n)
    gap = pr.pow_midpoint_gap(damping, h)  # on the reference alone: the two pows may differ in their last bits
    assert gap.min() >= 16.0, f"damping {damping.flat[gap.argmin()]} is {gap.min()} f64 ulps from a float32 midpoint"
    vec = _make(dev, case, e, False)
    vec.reset()
    vel = np.random.default_rng(n).uniform(-2.0, 2.0, (e, n, 3)).astype(np.float32)
    vec.set_state(vel=vel, damping=damping)
    st = vec_state_numpy(vec)
    assert np.array_equal(st["damping"], damping)
    a, has = pr.actions(case, 0)
    _step(vec, dev, a, has)
    ns, out = so.step(cfg, st, a, has, physics=True, auto_reset=False, seed=pr.SEED, env_offset=pr.ENV_OFFSET)
    err = _compare_step(vec, ns, out, case.tag)
    assert not ns["vel"][damping == 1.0].any() and ns["vel"][damping == 0.25].any()  # factor 0 stops a drone
    print(f"\n[physics-shapes] {case.tag} h={h:.5f}: {vec.kernel_name()} reward max|err| {err:.3e} "
          f"smallest midpoint gap {gap.min():.0f} ulps")


# ------------------------------------------------------------------ E. thresholds ulp by ulp
@pytest.mark.parametrize("name", list(pr.SCENES))
def test_threshold_scene(dev, name):
    from oracle import swarm_oracle as so
    case, scene, which = pr.build_scene(name)
    e, n = scene["pos"].shape[:2]
    vec = _make(dev, case, e, False)
    vec.reset()
    want = pr.scene_state(scene)
    vec.set_state(pos=want["pos"], vel=want["vel"], goal=want["goal"], obstacles=want["obst"], active=want["active"],
                  step_count=want["step"], episode=want["episode"].view(np.int32), damping=want["damping"])
    st = vec_state_numpy(vec)
    for k in STATE:
        assert np.array_equal(st[k], want[k]), k
    a = np.zeros((e, n, 3), np.float32)
    _step(vec, dev, a, None)
    ns, out = so.step(case.cfg, st, a, physics=True, auto_reset=False, seed=pr.SEED, env_offset=pr.ENV_OFFSET)
    err = _compare_step(vec, ns, out, name)
    pr.check_scene(scene, st, ns, out, which)
    print(f"\n[physics-shapes] scene {name}: {vec.kernel_name()} reward max|err| {err:.3e} "
          f"hits {int(out[which][scene['sample']].sum())} of {int(scene['sample'].sum())}")


# ------------------------------------------------------------------ F. reset and observe
@pytest.mark.parametrize("n,k,ms,m,e", pr.AUX_SHAPES)
def test_masked_reset_and_observe(dev, n, k, ms, m, e):
    from oracle import swarm_oracle as so
    case = pr.Case(f"aux-N{n}-K{k}-Ms{ms}-M{m}", n, e, k, ms, m, max_steps=50)
    cfg = case.cfg
    kw = dict(physics=True, seed=pr.SEED, env_offset=pr.ENV_OFFSET)
    vec = _make(dev, case, e, True)
    vec.reset()
    for t in range(2):  # velocities, step counts and episodes that a reset has to clear
        a, has = pr.actions(case, t)
        _step(vec, dev, a, has)
    # 1. masked reset: every third env
    mask = torch.zeros(e, dtype=torch.bool, device=dev)
    mask[::3] = True
    sel = mask.cpu().numpy()
    st = vec_state_numpy(vec)
    before = {name: getattr(vec, name).clone() for name in ("obs", "dist_goal", "global_state", "reward")}
    vec.reset(mask)
    torch.cuda.synchronize()
    ns, ro = so.reset_device(cfg, st, sel, **kw)
    _compare_state(vec, ns, f"{case.tag} masked reset")
    _compare_view(vec, ro["obs"], ro["dist_goal"], ro["global_state"], f"{case.tag} masked reset", sel)
    keep = torch.as_tensor(~sel, device=dev)
    for name, old in before.items():
        assert torch.equal(getattr(vec, name)[keep], old[keep]), f"{case.tag}: reset touched {name} outside its mask"
    assert np.array_equal(ns["episode"], st["episode"] + sel) and ns["damping"][sel].all()
    # 2. velocities of which about half exceed max_speed
    vel = pr.fast_velocities(e, n, float(cfg["max_speed"]))
    vec.set_state(vel=vel)
    fast = pr.speed64(vel) > float(cfg["max_speed"])
    assert 0.3 < fast.mean() < 0.7
    # 3. observe with and without a mask: the observation clamp of the aux kernel
    obs = _compare_observe(vec, cfg, None, f"{case.tag} observe")
    assert (obs[..., 3:6][fast] != vel[fast]).any(axis=-1).all() and np.array_equal(obs[..., 3:6][~fast], vel[~fast])
    _compare_observe(vec, cfg, mask, f"{case.tag} observe masked")
    _compare_observe(vec, cfg, (~mask).to(torch.uint8), f"{case.tag} observe masked (u8)")
    print(f"\n[physics-shapes] {case.tag}: step {vec.kernel_name()}, aux {pr.kernel_name(n, k, ms, m, kind=1)}, "
          f"{int(fast.sum())} of {fast.size} velocities above max_speed")
