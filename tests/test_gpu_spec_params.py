"""GPU: the specialised step kernels (swarm_step16q, swarm_step64_once and its physics and
fused-eval variants, swarm_step256w) away from the default DroneEnvConfig scalars.

A. Parameter sweep: four parameter points (small / wide / large world, values no float holds
   exactly) per specialisation, 10 auto-reset steps, against the generic kernel (outputs and state
   bitwise) and the f64 oracle (obs, flags, state bitwise; rewards within the reward contract).
   The oracle's own outputs prove that resets, collisions, goals, the world clip and the speed clip
   all happened.  Plus the physics step64 and the fused eval at non-default scalars.
B. Worst-case formation sum: two antipodal clusters in the world's corners, where every f32 chain
   of the formation term carries its largest partial sums (world_size 20 and 100).
C. Threshold boundaries ulp by ulp: 128 consecutive floats around 2 x collision_radius (pairs, on
   the all-active and on the masked pair pass), collision_radius + obstacle_radius, max_speed and
   2 x drone_contact_radius (physics), each decided exactly as the oracle decides it.

The reward bound is the project's contract: 1e-5 absolute against the f64 oracle.
Every case prints its maximum reward error (pytest -s); DESIGN.md §5 tabulates them.
"""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from tests.helpers import oracle_cfg, vec_state_numpy
from tests.test_gpu_step64 import OUTS, STATE

pytestmark = pytest.mark.gpu

REWARD_TOL = 1e-5  # absolute, against the f64 oracle
SEED = 7
# N -> (envs of the sweep, kernel the launch must select)
KERNELS = {16: (48, "swarm_step16q"), 64: (24, "swarm_step64_once<32, 4>"), 256: (4, "swarm_step256w")}
PHYS_KERNEL = "swarm_step64_phys_once<32, 4>"
POINTS = {
    "small": dict(world_size=8.0, dt=0.05, max_speed=1.5, max_accel=6.0, collision_radius=0.2,
                  obstacle_radius=0.35, goal_radius=0.6, desired_spacing=1.25, reward_formation_scale=0.4,
                  reward_progress_scale=1.0, reward_goal=10.0, reward_collision=-7.5),
    "wide": dict(world_size=60.0, goal_radius=6.0, max_accel=30.0),
    "large": dict(world_size=100.0, dt=0.25, max_speed=11.0, max_accel=9.0, collision_radius=1.1,
                  obstacle_radius=2.3, goal_radius=12.0, desired_spacing=7.5),
    "odd": dict(world_size=33.3, dt=1.0 / 30.0, max_speed=1.0 / 3.0, max_accel=7.7, collision_radius=1.0 / 3.0,
                obstacle_radius=0.77, goal_radius=10.0 / 3.0, desired_spacing=0.1,
                reward_formation_scale=1.0 / 7.0, reward_progress_scale=3.3, reward_goal=1.0 / 3.0,
                reward_collision=-0.7),
}
ORACLE_STATE = ("pos", "vel", "goal", "obst", "active", "step", "episode")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _pair(dev, raw, e, **kw):
    from swarm_marl_amd import VecSwarm
    kw.setdefault("with_infos", True)
    kw.setdefault("with_global_state", True)
    a = VecSwarm(e, raw, device=dev, kernel_path="auto", **kw)
    b = VecSwarm(e, raw, device=dev, kernel_path="generic", **kw)
    assert b.kernel_name().startswith("swarm_kernel<")
    return a, b


def _assert_bitwise(a, b, tag, reward=False):
    for name in OUTS + STATE + (("reward",) if reward else ()):
        x, y = getattr(a, name), getattr(b, name)
        if not torch.equal(x, y):
            bad = (x != y).nonzero()[:5].tolist()
            raise AssertionError(f"{tag}: {name} differs between auto and generic at {bad}")


def _assert_oracle(v, out, ns, tag, state_keys=ORACLE_STATE):
    """Everything but the reward bitwise as the oracle; returns the maximum reward error."""
    obs = v.obs.cpu().numpy()
    if not np.array_equal(obs, out["obs"]):
        bad = np.argwhere(obs != out["obs"])
        raise AssertionError(f"{tag}: obs differs from the oracle at {bad[:5].tolist()} (of {len(bad)})")
    assert np.array_equal(v.terminated.cpu().numpy(), out["terminated"]), f"{tag}: terminated"
    assert np.array_equal(v.truncated.cpu().numpy(), out["truncated"]), f"{tag}: truncated"
    assert np.array_equal((v.env_done.cpu().numpy() & 4) != 0, out["reset"]), f"{tag}: reset flag"
    got = vec_state_numpy(v)
    for k in state_keys:
        assert np.array_equal(got[k], ns[k]), f"{tag}: state {k}"
    assert np.array_equal(v.global_state.cpu().numpy(), out["global_state"]), f"{tag}: global_state"
    return float(np.abs(v.reward.cpu().numpy().astype(np.float64) - out["reward"]).max())


def _assert_flags(v, out, tag):
    flags = v.info_flags.cpu().numpy()
    stepped = out["stepped"]
    assert np.array_equal((flags & 1) != 0, stepped), f"{tag}: stepped flag"
    assert np.array_equal((flags & 2) != 0, out["reached"] & stepped), f"{tag}: reached flag"
    assert np.array_equal((flags & 4) != 0, out["collision"] & stepped), f"{tag}: collision flag"


# ------------------------------------------------------------------ A. parameter sweep
def _rollout(dev, raw, e, kernel, steps, physics=None):
    """auto and generic side by side for `steps` auto-reset steps; the oracle steps from the device
    state before every step.  Returns the coverage counts (from the oracle) and the reward maxima."""
    from oracle import swarm_oracle as so
    n = raw["num_drones"]
    kw = dict(auto_reset=True, seed=SEED)
    ocfg = dict(raw)
    if physics is not None:
        kw.update(dynamics="physics", physics=physics)
        ocfg.update(physics)
    cfg = oracle_cfg(ocfg)
    a, b = _pair(dev, raw, e, **kw)
    assert a.kernel_name() == kernel
    a.reset()
    b.reset()
    _assert_bitwise(a, b, "reset", reward=True)
    keys = ORACLE_STATE + (("damping",) if physics is not None else ())
    hw, vmax = np.float32(cfg["world_size"] / 2.0), float(np.float32(cfg["max_speed"]))
    rng = np.random.default_rng(1)
    stats = dict(reset=0, collision=0, reached=0, wall=0, speed=0, err_auto=0.0, err_generic=0.0)
    for t in range(steps):
        tag = f"t={t}"
        st = vec_state_numpy(a)
        act = rng.uniform(-1.3, 1.3, (e, n, 3)).astype(np.float32)
        dact = torch.as_tensor(act).to(dev)
        a.step(dact)
        b.step(dact)
        _assert_bitwise(a, b, tag, reward=physics is not None)  # no formation term in the physics reward
        assert torch.equal(a.damping, b.damping), f"{tag}: damping"
        ns, out = so.step(cfg, st, act, physics=physics is not None, auto_reset=True, seed=SEED,
                          exact_formation=True)
        for name, v in (("auto", a), ("generic", b)):
            err = _assert_oracle(v, out, ns, f"{name} {tag}", keys)
            stats["err_" + name] = max(stats["err_" + name], err)
        live = ~out["reset"]  # a reset env's state is the new episode's
        stats["reset"] += int(out["reset"].sum())
        stats["collision"] += int(out["collision"].sum())
        stats["reached"] += int(out["reached"].sum())
        stats["wall"] += int((np.abs(ns["pos"][live]) == hw).sum())
        sp = so.norm1d(ns["vel"][live]).astype(np.float64)
        stats["speed"] += int((np.abs(sp - vmax) <= 1e-5 * vmax).sum())
    return stats


_SWEEP: dict = {}


def _sweep(dev, n, point):
    """One sweep case, run once per session (the N = 256 union test reads all four points)."""
    key = (n, point)
    if key not in _SWEEP:
        e, kernel = KERNELS[n]
        raw = dict(num_drones=n, max_steps=6, **POINTS[point])
        try:
            _SWEEP[key] = _rollout(dev, raw, e, kernel, 10)
        except AssertionError as exc:
            _SWEEP[key] = exc
        else:
            s = _SWEEP[key]
            print(f"\nsweep N={n} {point}: reward max|err| auto {s['err_auto']:.3e} generic {s['err_generic']:.3e}"
                  f" | resets {s['reset']} collisions {s['collision']} reached {s['reached']}"
                  f" wall {s['wall']} speed {s['speed']}")
    if isinstance(_SWEEP[key], AssertionError):
        raise _SWEEP[key]
    return _SWEEP[key]


@pytest.mark.parametrize("point", list(POINTS))
@pytest.mark.parametrize("n", list(KERNELS))
def test_param_sweep(dev, n, point):
    s = _sweep(dev, n, point)
    need = ("reset", "collision", "reached") + (("wall", "speed") if n != 256 else ())
    for k in need:  # the oracle saw every branch: a green run is not an idle one
        assert s[k] > 0, f"coverage: no {k} at N={n} {point}"
    tol = REWARD_TOL
    assert s["err_auto"] <= tol, f"auto reward err {s['err_auto']} > {tol}"
    assert s["err_generic"] <= tol, f"generic reward err {s['err_generic']} > {tol}"


def test_param_sweep_256_clips(dev):
    """A 256-drone env in the small world collides and resets every step, so at N = 256 the two
    clips must show over the union of the four points."""
    wall = speed = 0
    for point in POINTS:
        s = _sweep(dev, 256, point)
        wall += s["wall"]
        speed += s["speed"]
    assert wall > 0 and speed > 0


def test_physics_step64_params(dev):
    raw = dict(num_drones=64, max_steps=6, world_size=44.0, max_speed=2.5, max_accel=13.0, obstacle_radius=1.3,
               goal_radius=5.0)
    s = _rollout(dev, raw, 16, PHYS_KERNEL, 9, physics={"drone_contact_radius": 0.4})
    print(f"\nphysics step64: reward max|err| auto {s['err_auto']:.3e} generic {s['err_generic']:.3e} | resets"
          f" {s['reset']} collisions {s['collision']} reached {s['reached']}")
    assert s["reset"] > 0 and s["collision"] > 0
    assert s["err_auto"] <= REWARD_TOL and s["err_generic"] <= REWARD_TOL


def _run_tracker(dev, fused, e=64, steps=70):
    from swarm_marl_amd import VecSwarm
    from swarm_marl_amd.eval_metrics import EvalTracker
    vec = VecSwarm(e, {"num_drones": 64, "max_steps": 30, "world_size": 60.0, "goal_radius": 6.0}, device=dev,
                   auto_reset=True, seed=17, with_infos=True)
    vec.reset()
    ev = EvalTracker(vec, capacity=8192, fused=fused)
    assert ev.fused == fused
    ev.begin()
    g = torch.Generator(device=dev).manual_seed(23)
    for _ in range(steps):
        vec.step(torch.rand((e, 64, 3), device=dev, generator=g) * 2 - 1)
        ev.update()
    assert vec.kernel_name() == "swarm_step64_once<32, 4>"
    return ev.records()


def test_fused_eval_params(dev):
    a = _run_tracker(dev, True)
    b = _run_tracker(dev, False)
    assert len(a) > 64 and a.shape == b.shape
    assert np.array_equal(a, b, equal_nan=True)


# ------------------------------------------------------------------ B. worst-case formation sum
def cluster_positions(n, e, world_size):
    """Two antipodal clusters in the corners (+h,+h,+h) / (-h,-h,-h), jittered, clipped to the world."""
    h = np.float32(world_size / 2.0)
    rng = np.random.default_rng(1000 + n)
    pos = np.empty((e, n, 3), np.float32)
    pos[:, : n // 2] = h
    pos[:, n // 2:] = -h
    pos += rng.uniform(-0.02 * world_size, 0.02 * world_size, pos.shape).astype(np.float32)
    return np.clip(pos, -h, h).astype(np.float32)


@pytest.mark.parametrize("world_size", [20.0, 100.0])
@pytest.mark.parametrize("n", list(KERNELS))
def test_worst_case_formation_sum(dev, n, world_size):
    from oracle import swarm_oracle as so
    e = 8 if n == 256 else 64
    raw = dict(num_drones=n, world_size=world_size)
    cfg = oracle_cfg(raw)
    a, b = _pair(dev, raw, e, auto_reset=False, seed=SEED)
    assert a.kernel_name() == KERNELS[n][1]
    pos = cluster_positions(n, e, world_size)
    for v in (a, b):
        v.reset()
        v.set_state(pos=pos, vel=np.zeros_like(pos), active=np.ones((e, n), bool),
                    step_count=np.zeros(e, np.int32))
    st = vec_state_numpy(a)
    act = np.zeros((e, n, 3), np.float32)
    for v in (a, b):
        v.step(torch.as_tensor(act).to(dev))
    ns, out = so.step(cfg, st, act, auto_reset=False, seed=SEED, exact_formation=True)
    d = so.norm1d(ns["pos"][:, :, None, :] - ns["pos"][:, None, :, :]).astype(np.float64)
    fsum = np.abs(d - cfg["desired_spacing"]).sum(axis=2) - cfg["desired_spacing"]  # less the j = i term
    assert fsum.min() >= 0.4 * (n - 1) * math.sqrt(3.0) * world_size  # not a trivial sum
    _assert_bitwise(a, b, "clusters")
    errs = {name: _assert_oracle(v, out, ns, name) for name, v in (("auto", a), ("generic", b))}
    print(f"\nclusters N={n} world {world_size:g}: reward max|err| auto {errs['auto']:.3e}"
          f" generic {errs['generic']:.3e} (max |reward| {np.abs(out['reward']).max():.1f})")
    tol = REWARD_TOL
    assert errs["auto"] <= tol, f"auto reward err {errs['auto']} > {tol}"
    assert errs["generic"] <= tol, f"generic reward err {errs['generic']} > {tol}"


# ------------------------------------------------------------------ C. threshold boundaries
def ulps_around(x0, count=128):
    """`count` consecutive float32 values, half of them below x0."""
    xs = [np.float32(x0)]
    for _ in range(count // 2):
        xs.insert(0, np.nextafter(xs[0], np.float32(-np.inf)))
        xs.append(np.nextafter(xs[-1], np.float32(np.inf)))
    return np.array(xs[:count], np.float32)


def _lattice(count, pitch, lo, hi):
    """The first `count` points of the cubic lattice of the given pitch inside the box [lo, hi]."""
    axes = [np.arange(l, h_ + 1e-9, pitch) for l, h_ in zip(lo, hi)]
    pts = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
    assert len(pts) >= count, f"lattice holds {len(pts)} < {count} points"
    return pts[:count].astype(np.float32)


def _corner_obstacles(e, h, m=8):
    obst = np.full((e, m, 3), h - 0.6, np.float32)
    obst[:, :, 0] -= 0.07 * np.arange(m, dtype=np.float32)
    return obst


def _world(n):
    return 20.0 if n <= 64 else 60.0  # the N = 256 grids do not fit into the default world


def pair_scene(n, thr, layout, masked, world_size, zlo=None):
    """Pairs (A, B) at the 128 floats around `thr`: A on a y-z grid of pitch 3.5 thr, B = A + offset
    (layout "x0": A.x = 0, offset along x; "x37": A.x = -3.7; "diag": offset / sqrt(3) on every
    axis).  The last two drones are a far-away pair, inactive when `masked`."""
    h = world_size / 2.0
    per = n // 2 - 1
    e = -(-128 // per)
    vals = ulps_around(thr)[np.arange(e * per) % 128].reshape(e, per)
    pitch = 3.5 * float(thr)
    ny = math.ceil(math.sqrt(per))
    nz = -(-per // ny)
    z0 = -(nz - 1) / 2 * pitch - 0.0273 if zlo is None else zlo
    cell = _lattice(per, pitch, (0.0, -(ny - 1) / 2 * pitch + 0.0131, z0),
                    (0.0, (ny - 1) / 2 * pitch + 0.02, z0 + (nz - 1) * pitch + 0.01))
    assert np.abs(cell).max() < h - 1.0
    ax = {"x0": 0.0, "x37": -3.7, "diag": 0.25}[layout]
    pa = np.broadcast_to(cell, (e, per, 3)).copy()
    pa[..., 0] = np.float32(ax)
    pb = pa.copy()
    if layout == "diag":
        pb += (vals.astype(np.float64) / math.sqrt(3.0)).astype(np.float32)[..., None]
    else:
        pb[..., 0] += vals
    pos = np.zeros((e, n, 3), np.float32)
    rng = np.random.default_rng(5)
    for k in range(e):  # pairs at every rotation distance, not only neighbouring lanes
        perm = rng.permutation(2 * per)
        pos[k, perm[:per]] = pa[k]
        pos[k, perm[per:]] = pb[k]
    zf = float(cell[:, 2].mean())
    pos[:, n - 2] = (-h + 1.5, -2.0, zf)
    pos[:, n - 1] = (-h + 1.5, 2.0, zf)
    active = np.ones((e, n), bool)
    if masked:
        active[:, n - 2:] = False
    sample = np.zeros((e, n), bool)
    sample[:, : 2 * per] = True
    goal = np.tile(np.float32([-h + 0.5, h - 0.5, -h + 0.5]), (e, 1))
    return dict(pos=pos, vel=np.zeros_like(pos), goal=goal, obstacles=_corner_obstacles(e, h), active=active,
                sample=sample)


def obstacle_scene(n, thr, layout, world_size):
    """Drone s of env k next to obstacle s (8 obstacles on the corners of a cube of side 7) at the
    128 floats around `thr`, on the +x / +diagonal side in even envs and the other side in odd ones;
    the other drones parked on a lattice in the slab above."""
    h = world_size / 2.0
    e, m = 16, 8
    oc = np.array([[sx, sy, sz] for sx in (-3.5, 3.5) for sy in (-3.5, 3.5) for sz in (-3.5, 3.5)], np.float64)
    oc += (0.11, -0.07, 0.05)
    vals = ulps_around(thr).reshape(e, m).astype(np.float64)
    sign = np.where(np.arange(e) % 2 == 0, 1.0, -1.0)[:, None]
    direc = np.array([1.0, 0.0, 0.0] if layout == "x" else [1.0 / math.sqrt(3.0)] * 3)
    obst = np.broadcast_to(oc.astype(np.float32), (e, m, 3)).copy()
    pos = np.zeros((e, n, 3), np.float32)
    pos[:, :m] = obst + ((sign * vals)[..., None] * direc).astype(np.float32)
    pos[:, m:] = _lattice(n - m, 3.5, (-(h - 3.0), -(h - 3.0), 8.5), (h - 1.5, h - 1.5, h - 1.5))
    sample = np.zeros((e, n), bool)
    sample[:, :m] = True
    goal = np.tile(np.float32([-h + 0.5, h - 0.5, -h + 0.5]), (e, 1))
    return dict(pos=pos, vel=np.zeros_like(pos), goal=goal, obstacles=obst, active=np.ones((e, n), bool),
                sample=sample)


def speed_scene(n, vmax, layout, world_size):
    """Every drone's velocity at one of the 128 floats around max_speed, along x or the diagonal."""
    h = world_size / 2.0
    e = max(1, 128 // n)
    vals = ulps_around(vmax)[np.arange(e * n) % 128].reshape(e, n)
    vel = np.zeros((e, n, 3), np.float32)
    if layout == "x":
        vel[..., 0] = vals
    else:
        vel[...] = (vals.astype(np.float64) / math.sqrt(3.0)).astype(np.float32)[..., None]
    pos = np.broadcast_to(_lattice(n, 3.5, (-6.0,) * 3, (h - 4.0,) * 3), (e, n, 3)).copy()
    goal = np.tile(np.float32([-h + 0.5, h - 0.5, -h + 0.5]), (e, 1))
    return dict(pos=pos, vel=vel, goal=goal, obstacles=_corner_obstacles(e, h), active=np.ones((e, n), bool),
                sample=np.ones((e, n), bool))


def _boundary(dev, raw, scene, kernel, physics=None):
    """One zero-action step of `scene` on auto and generic, both against the oracle; returns the
    oracle's (state before, new state, outputs)."""
    from oracle import swarm_oracle as so
    e, n = scene["pos"].shape[:2]
    kw, ocfg = dict(auto_reset=False, seed=SEED), dict(raw)
    if physics is not None:
        kw.update(dynamics="physics", physics=physics)
        ocfg.update(physics)
    cfg = oracle_cfg(ocfg)
    a, b = _pair(dev, raw, e, **kw)
    assert a.kernel_name() == kernel
    state = {k: scene[k] for k in ("pos", "vel", "goal", "obstacles", "active")}
    for v in (a, b):
        v.reset()
        v.set_state(step_count=np.zeros(e, np.int32), damping=np.zeros((e, n), np.float32), **state)
    st = vec_state_numpy(a)
    act = np.zeros((e, n, 3), np.float32)
    for v in (a, b):
        v.step(torch.as_tensor(act).to(dev))
    _assert_bitwise(a, b, "boundary", reward=physics is not None)
    ns, out = so.step(cfg, st, act, physics=physics is not None, auto_reset=False, seed=SEED, exact_formation=True)
    for name, v in (("auto", a), ("generic", b)):
        err = _assert_oracle(v, out, ns, name)
        _assert_flags(v, out, name)
        assert err <= REWARD_TOL, f"{name}: reward err {err}"
    return st, ns, out


def _assert_straddles(hits, sample):
    got = int(hits[sample].sum())
    assert 0 < got < int(sample.sum()), f"the boundary does not run through the sample ({got} hits)"


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("layout", ["x0", "x37", "diag"])
@pytest.mark.parametrize("radius", [0.5, 1.0 / 3.0])
@pytest.mark.parametrize("n", list(KERNELS))
def test_pair_collision_boundary(dev, n, radius, layout, masked):
    ws = _world(n)
    raw = dict(num_drones=n, world_size=ws, collision_radius=radius, goal_radius=0.0, max_steps=50)
    scene = pair_scene(n, np.float32(2.0 * radius), layout, masked, ws)
    _, _, out = _boundary(dev, raw, scene, KERNELS[n][1])
    assert not out["reached"].any()
    _assert_straddles(out["collision"], scene["sample"])
    assert not out["collision"][~scene["sample"]].any()


@pytest.mark.parametrize("layout", ["x", "diag"])
@pytest.mark.parametrize("radii", [(0.5, 0.8), (1.0 / 3.0, 0.77)])
@pytest.mark.parametrize("n", list(KERNELS))
def test_obstacle_collision_boundary(dev, n, radii, layout):
    ws = 20.0 if n == 16 else 60.0  # the parked drones of N >= 64 need the room
    raw = dict(num_drones=n, world_size=ws, collision_radius=radii[0], obstacle_radius=radii[1], goal_radius=0.0,
               max_steps=50)
    scene = obstacle_scene(n, np.float32(radii[0] + radii[1]), layout, ws)
    _, _, out = _boundary(dev, raw, scene, KERNELS[n][1])
    _assert_straddles(out["collision"], scene["sample"])
    assert not out["collision"][~scene["sample"]].any()


@pytest.mark.parametrize("layout", ["x", "diag"])
@pytest.mark.parametrize("vmax", [4.0, 3.3, 1.0 / 3.0])
@pytest.mark.parametrize("n", list(KERNELS))
def test_speed_clip_boundary(dev, n, vmax, layout):
    from oracle import swarm_oracle as so
    ws = _world(n)
    raw = dict(num_drones=n, world_size=ws, max_speed=vmax, goal_radius=0.0, max_steps=50)
    scene = speed_scene(n, np.float32(vmax), layout, ws)
    st, ns, out = _boundary(dev, raw, scene, KERNELS[n][1])  # new vel and pos bitwise as the oracle
    assert not out["collision"].any() and not out["reached"].any()
    clipped = so.norm1d(st["vel"]) > np.float32(vmax)
    _assert_straddles(clipped, scene["sample"])


@pytest.mark.parametrize("layout", ["x0", "diag"])
@pytest.mark.parametrize("contact", [0.15, 0.4])
def test_physics_contact_boundary(dev, contact, layout):
    ws = 40.0  # the y-z grid sits above the ground
    raw = dict(num_drones=64, world_size=ws, goal_radius=0.0, max_steps=50)
    scene = pair_scene(64, np.float32(2.0 * contact), layout, False, ws, zlo=2.0)
    _, _, out = _boundary(dev, raw, scene, PHYS_KERNEL, physics={"drone_contact_radius": contact})
    _assert_straddles(out["collision"], scene["sample"])
    assert not out["collision"][~scene["sample"]].any()
