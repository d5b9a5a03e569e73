"""Cases, scenes and coverage counts of the physics-shape tests: tests/test_gpu_physics_shapes.py
steps them on the device, tests/test_physics_scenes_cpu.py proves on the oracle alone that every
case reaches the branches it is there for.  numpy and the oracle only: nothing here needs a GPU.

A case is a `Case`: the VecSwarm config (`raw`, `physics`), the oracle config (`cfg`: the same
values under the oracle's names) and the generic-kernel instantiation the launch must select.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from oracle import swarm_oracle as so
from tests.test_gpu_spec_params import _corner_obstacles, _lattice, pair_scene, ulps_around

SEED = 13
ENV_OFFSET = 7  # Philox counters carry env_offset + env: a nonzero offset shows a dropped one
STEPS = 9

f32 = np.float32


def neighbor_slots(k: int) -> int:
    return 0 if k <= 0 else 4 if k <= 3 else 9 if k <= 8 else 17


def obstacle_slots(ms: int, m: int) -> int:
    need = min(ms, m)
    return 0 if need <= 0 else 5 if need <= 4 else 9 if need <= 8 else 17


def lane_mode(n: int) -> int:
    """1: several teams per wave (N <= 32 lanes), 2: one 64-lane team per wave, 0: block teams."""
    return 1 if n <= 32 else 2 if n <= 64 else 0


def kernel_name(n, k, ms, m, kind=0) -> str:
    return f"swarm_kernel<{kind}, 1, {neighbor_slots(k)}, {obstacle_slots(ms, m)}, {lane_mode(n)}>"


@dataclass
class Case:
    tag: str
    n: int
    e: int
    k: int = 3
    ms: int = 4
    m: int = 8
    law: int = 0
    max_steps: int = 5
    substeps: int | None = None  # None: the default int(dt * 240)
    scalars: dict = field(default_factory=dict)  # DroneEnvConfig fields off their defaults
    phys: dict = field(default_factory=dict)  # physics constants off their defaults

    @property
    def raw(self) -> dict:
        return dict(num_drones=self.n, neighbor_k=self.k, sensed_obstacles=self.ms, num_obstacles=self.m,
                    max_steps=self.max_steps, **self.scalars)

    @property
    def physics(self) -> dict:
        p = dict(self.phys, damping_law=self.law)
        if self.substeps is not None:
            p["substeps"] = self.substeps
        return p

    @property
    def cfg(self) -> dict:
        c = so.make_cfg(**self.raw, **self.phys, damping_law=self.law)
        if self.substeps is not None:
            c["physics_substeps"] = self.substeps
        return c

    @property
    def kernel(self) -> str:
        return kernel_name(self.n, self.k, self.ms, self.m)


# ------------------------------------------------------------------ A. lane modes
LANE_SHAPES = [(1, 70), (3, 50), (24, 40), (32, 20), (33, 20), (64, 8), (65, 6), (100, 6), (128, 4), (256, 3),
               (512, 2)]
LANE_CASES = [Case(f"lane-N{n}", n, e, law=i % 2, max_steps=4 + i % 4) for i, (n, e) in enumerate(LANE_SHAPES)]

# ------------------------------------------------------------------ B. slot widths
WIDTHS = [(0, 4, 8), (1, 2, 8), (4, 4, 8), (5, 6, 8), (8, 8, 8), (12, 16, 20), (16, 0, 5), (3, 4, 0)]
WIDTH_SHAPES = [(24, 40), (32, 20), (40, 16), (100, 4)]
# Without obstacles a contact is a pair or the ground, both rare in the default world within 9
# steps: the M = 0 and Ms = 0 rows play in a smaller world (the draw ranges scale with it).
_WIDTH_WORLD = {(3, 4, 0): 5.0, (16, 0, 5): 10.0}
WIDTH_CASES = [
    Case(f"width-N{n}-K{k}-Ms{ms}-M{m}", n, e, k, ms, m, law=(i + j) % 2, max_steps=4 + (i + j) % 4,
         scalars={"world_size": _WIDTH_WORLD[(k, ms, m)]} if (k, ms, m) in _WIDTH_WORLD else {})
    for j, (n, e) in enumerate(WIDTH_SHAPES) for i, (k, ms, m) in enumerate(WIDTHS)]

# ------------------------------------------------------------------ C. scalars off the defaults
SCALAR_SHAPES = [(16, 32), (33, 12), (100, 4)]
POINTS = {
    # gravity, its compensation, the substep, both contact sizes and the world all moved; goal_radius
    # and max_speed are values no float holds exactly
    "low_g": dict(scalars=dict(world_size=33.3, max_accel=7.7, goal_radius=10.0 / 3.0, max_speed=3.3,
                               obstacle_radius=0.77),
                  phys=dict(gravity=-3.7, gravity_comp=3.1, substep_dt=1.0 / 120.0, ground_contact_height=0.4,
                            drone_contact_radius=0.4), law=1, substeps=None),
    "heavy": dict(scalars=dict(world_size=8.0, max_accel=13.0, goal_radius=0.7, max_speed=2.3, dt=0.05),
                  phys=dict(gravity=-12.5, gravity_comp=11.1, substep_dt=1.0 / 300.0, ground_contact_height=0.11,
                            drone_contact_radius=0.07), law=0, substeps=None),
    "wide": dict(scalars=dict(world_size=60.0, max_accel=30.0, goal_radius=6.1, max_speed=11.3),
                 phys=dict(gravity=-9.81, gravity_comp=12.0, substep_dt=1.0 / 90.0, ground_contact_height=0.3,
                           drone_contact_radius=0.3), law=1, substeps=5),
    # both clamps: the substep clamp holds the speed at 0.7, the last substep's acceleration lifts
    # it just above, so the next step enters above max_speed and the observation clamp fires
    "slow": dict(scalars=dict(max_speed=0.7, goal_radius=6.0), phys={}, law=0, substeps=None),
    "slow_law1": dict(scalars=dict(max_speed=0.7, goal_radius=6.0), phys={}, law=1, substeps=None),
}
SUBSTEPS = [0, 1, 5, 48]
SCALAR_CASES = [Case(f"point-{name}-N{n}", n, e, law=p["law"], max_steps=4 + (i + j) % 4, substeps=p["substeps"],
                     scalars=p["scalars"], phys=p["phys"])
                for j, (n, e) in enumerate(SCALAR_SHAPES) for i, (name, p) in enumerate(POINTS.items())]
SCALAR_CASES += [Case(f"substeps-{s}-law{law}-N{n}", n, e, law=law, max_steps=4 + (i + j) % 4, substeps=s)
                 for j, (n, e) in enumerate(SCALAR_SHAPES) for i, s in enumerate(SUBSTEPS) for law in (0, 1)]
CLAMP_CASES = [c.tag for c in SCALAR_CASES if c.tag.startswith("point-slow")]

ROLLOUT_CASES = LANE_CASES + WIDTH_CASES + SCALAR_CASES
COUNTS = ("reset", "collision", "ground", "obstacle", "pair", "reached", "trunc", "speed_in", "speed_out")


def actions(case: Case, t: int):
    """Step t's actions, uniform in [-1.3, 1.3], and its action mask with about 15 % off."""
    rng = np.random.default_rng(1000 * t + case.n + 7 * case.e + 31 * case.k + 57 * case.ms)
    a = rng.uniform(-1.3, 1.3, (case.e, case.n, 3)).astype(f32)
    has = rng.uniform(size=(case.e, case.n)) > 0.15
    return a, has


def speed64(vel):
    """The velocity norm of the observation clamp: f64 from the f32 components."""
    v = vel.astype(np.float64)
    sq = v * v
    return np.sqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2])


def step_counts(cfg, st, a, has, ns, out) -> dict:
    """What one oracle step saw, from the oracle's own integrator, thresholds and outputs."""
    p1, _ = so._physics_integrate(cfg, st["pos"], st["vel"], a, has, st["damping"])
    thr = so.thresholds(cfg)
    e, n, _ = p1.shape
    act = st["active"].astype(bool)
    ground = p1[..., 2] <= thr["ground"]
    obst = np.zeros((e, n), bool)
    if st["obst"].shape[1] > 0:
        obst = np.any(so.norm_axis(st["obst"][:, None, :, :] - p1[:, :, None, :]) <= thr["phys_obst"], axis=2)
    dpp = so.norm1d(p1[:, :, None, :] - p1[:, None, :, :])
    pair = np.any(~np.eye(n, dtype=bool)[None] & (dpp <= thr["phys_pair"]), axis=2)
    assert np.array_equal(ground | obst | pair, out["collision"]), "the contact kinds add up to the oracle's flag"
    live = ~out["reset"]
    substeps = int(cfg.get("physics_substeps", 24))
    return dict(
        reset=int(out["reset"].sum()), collision=int((act & out["collision"]).sum()),
        ground=int((act & ground).sum()), obstacle=int((act & obst).sum()), pair=int((act & pair).sum()),
        reached=int((act & out["reached"]).sum()), trunc=int(out["trunc_all"].sum()),
        # a drone with an action entered the step above max_speed: the substep clamp
        speed_in=int((has & (so.norm1d(st["vel"]) > f32(cfg["max_speed"]))).sum()) if substeps > 0 else 0,
        # a velocity left in the state above max_speed: the observation clamp
        speed_out=int((speed64(ns["vel"][live]) > float(cfg["max_speed"])).sum()))


def add_counts(total: dict, one: dict) -> dict:
    for k in COUNTS:
        total[k] = total.get(k, 0) + one[k]
    return total


def oracle_rollout(case: Case) -> dict:
    """The case's rollout on the oracle alone: the trajectory the device must follow bit for bit."""
    cfg = case.cfg
    st, _ = so.reset_device(cfg, so.empty_state(cfg, case.e), physics=True, seed=SEED, env_offset=ENV_OFFSET)
    total = {}
    for t in range(STEPS):
        a, has = actions(case, t)
        ns, out = so.step(cfg, st, a, has, physics=True, auto_reset=True, seed=SEED, env_offset=ENV_OFFSET)
        add_counts(total, step_counts(cfg, st, a, has, ns, out))
        st = ns
    return total


# ------------------------------------------------------------------ D. damping-law-1 factor
DAMPING_EDGES = (0.0, 1.0, 0.25, 0.999)


def damping_values(count: int, seed: int = 3) -> np.ndarray:
    """The four edges, then drawn values in [0, 1), as float32."""
    rng = np.random.default_rng(seed)
    vals = np.concatenate([np.array(DAMPING_EDGES, np.float64), rng.uniform(0.0, 1.0, count - len(DAMPING_EDGES))])
    return vals.astype(f32)


def pow_midpoint_gap(damping: np.ndarray, h: float) -> np.ndarray:
    """f64 ulps between the host's pow((double)(1 - d), h) and the nearest float32 rounding midpoint.
    With a gap of 16 ulps or more, a pow that differs from the host's in its last bits still
    rounds to the same float32 factor."""
    d = np.asarray(damping, f32)
    r = np.power((f32(1.0) - d).astype(np.float64), float(f32(h)))
    f = r.astype(f32)
    up = np.nextafter(f, f32(np.inf)).astype(np.float64)
    dn = np.nextafter(f, f32(-np.inf)).astype(np.float64)
    fm = f.astype(np.float64)
    gap = np.minimum(np.abs(r - (fm + up) / 2.0), np.abs(r - (fm + dn) / 2.0))
    return gap / np.spacing(r)


# ------------------------------------------------------------------ E. threshold scenes
SCENE_WORLD = 40.0
SCENE_SHAPES = [(16, 3), (24, 3), (40, 3), (100, 3)]  # (N, K)
CONTACT_SHAPES = SCENE_SHAPES + [(16, 0)]


def _far_goal(e, h):
    return np.tile(f32([-h + 0.5, h - 0.5, h - 0.5]), (e, 1))


def _spread(vals, e, per):
    return vals[np.arange(e * per) % len(vals)].reshape(e, per)


def ground_scene(n, height):
    """Drones on an x-y grid of pitch 1.5, z at the 128 floats around (float)ground_contact_height;
    the last two drones parked at z = 3."""
    h = SCENE_WORLD / 2.0
    per = n - 2
    e = -(-128 // per)
    side = math.ceil(math.sqrt(n))
    grid = _lattice(n, 1.5, (-(side - 1) * 0.75 + 0.013, -(side - 1) * 0.75 - 0.021, 0.0),
                    ((side - 1) * 0.75 + 0.02, (side - 1) * 0.75, 0.0))
    pos = np.broadcast_to(grid, (e, n, 3)).copy()
    pos[:, :per, 2] = _spread(ulps_around(f32(height)), e, per)
    pos[:, per:, 2] = 3.0
    sample = np.zeros((e, n), bool)
    sample[:, :per] = True
    return dict(pos=pos, vel=np.zeros_like(pos), goal=_far_goal(e, h), obstacles=_corner_obstacles(e, h),
                active=np.ones((e, n), bool), sample=sample)


def goal_scene(n, radius, layout):
    """Sample drones around the goal at the 128 floats around goal_radius: two per env on the x axis
    (layout "x") or eight on the diagonals ("diag"), further apart than any contact; the others
    parked on a grid in the plane z = 1, further from the goal than the radius."""
    h = SCENE_WORLD / 2.0
    dirs = (np.array([[1.0, 0, 0], [-1.0, 0, 0]]) if layout == "x" else
            np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) / math.sqrt(3.0))
    per = len(dirs)
    e = 128 // per
    g = np.array([0.3, -0.2, 6.0])
    vals = _spread(ulps_around(f32(radius)), e, per).astype(np.float64)
    pos = np.zeros((e, n, 3), f32)
    pos[:, :per] = (g + vals[..., None] * dirs).astype(f32)
    side = math.ceil(math.sqrt(n - per))
    pos[:, per:] = _lattice(n - per, 1.5, (-(side - 1) * 0.75, -(side - 1) * 0.75 + 0.017, 1.0),
                            ((side - 1) * 0.75 + 0.01, (side - 1) * 0.75 + 0.03, 1.0))
    sample = np.zeros((e, n), bool)
    sample[:, :per] = True
    return dict(pos=pos, vel=np.zeros_like(pos), goal=np.tile(g.astype(f32), (e, 1)),
                obstacles=_corner_obstacles(e, h), active=np.ones((e, n), bool), sample=sample)


def obstacle_contact_scene(n, thr, layout):
    """test_gpu_spec_params.obstacle_scene above the ground: drone s of env k next to obstacle s
    (the corners of a cube of side 7 centred at z = 5) at the 128 floats around `thr`; the other
    drones parked on a grid in the plane z = 12."""
    h = SCENE_WORLD / 2.0
    e, m = 16, 8
    oc = np.array([[sx, sy, sz] for sx in (-3.5, 3.5) for sy in (-3.5, 3.5) for sz in (-3.5, 3.5)], np.float64)
    oc += (0.11, -0.07, 5.05)
    vals = ulps_around(thr).reshape(e, m).astype(np.float64)
    sign = np.where(np.arange(e) % 2 == 0, 1.0, -1.0)[:, None]
    direc = np.array([1.0, 0.0, 0.0] if layout == "x" else [1.0 / math.sqrt(3.0)] * 3)
    obst = np.broadcast_to(oc.astype(f32), (e, m, 3)).copy()
    pos = np.zeros((e, n, 3), f32)
    pos[:, :m] = obst + ((sign * vals)[..., None] * direc).astype(f32)
    pos[:, m:] = _lattice(n - m, 3.5, (-(h - 3.0), -(h - 3.0), 12.0), (h - 1.5, h - 1.5, 12.0))
    sample = np.zeros((e, n), bool)
    sample[:, :m] = True
    return dict(pos=pos, vel=np.zeros_like(pos), goal=_far_goal(e, h), obstacles=obst,
                active=np.ones((e, n), bool), sample=sample)


def pair_contact_scene(n, contact, layout):
    """test_gpu_spec_params.pair_scene with its y-z grid above the ground."""
    return pair_scene(n, f32(2.0 * contact), layout, False, SCENE_WORLD, zlo=2.0)


def scene_case(n, k, scalars=None, phys=None) -> Case:
    """substeps = 0: the positions stay exactly as set, so each scene decides its own straddle."""
    sc = dict(world_size=SCENE_WORLD, goal_radius=0.0)
    sc.update(scalars or {})
    return Case(f"scene-N{n}-K{k}", n, 0, k=k, max_steps=50, substeps=0, scalars=sc, phys=phys or {})


def scene_state(scene) -> dict:
    e, n = scene["pos"].shape[:2]
    return dict(pos=scene["pos"], vel=scene["vel"], goal=scene["goal"], obst=scene["obstacles"],
                active=scene["active"], step=np.zeros(e, np.int32), episode=np.ones(e, np.uint32),
                damping=np.full((e, n), 0.45, f32))


def _ground(n, k, height):
    return scene_case(n, k, phys=dict(ground_contact_height=height)), ground_scene(n, height), "collision"


def _goal(n, k, radius, layout):
    return scene_case(n, k, scalars=dict(goal_radius=radius)), goal_scene(n, radius, layout), "reached"


def _obstacle(n, k, radii, layout):
    case = scene_case(n, k, scalars=dict(obstacle_radius=radii[0]), phys=dict(drone_contact_radius=radii[1]))
    return case, obstacle_contact_scene(n, f32(radii[0] + radii[1]), layout), "collision"


def _pair(n, k, contact, layout):
    return scene_case(n, k, phys=dict(drone_contact_radius=contact)), pair_contact_scene(n, contact, layout), "collision"


# id -> (builder, args); a builder returns (case, scene, the output that must straddle the sample)
SCENES = {}
for _n, _k in SCENE_SHAPES:
    for _h in (0.025, 0.4):
        SCENES[f"ground-{_h}-N{_n}"] = (_ground, (_n, _k, _h))
    for _r, _rn in ((0.5, "0.5"), (10.0 / 3.0, "10_3")):
        for _lay in ("x", "diag"):
            SCENES[f"goal-{_rn}-{_lay}-N{_n}"] = (_goal, (_n, _k, _r, _lay))
for _n, _k in CONTACT_SHAPES:
    for _radii in ((0.8, 0.15), (0.77, 0.4)):
        for _lay in ("x", "diag"):
            SCENES[f"obstacle-{_radii[1]}-{_lay}-N{_n}-K{_k}"] = (_obstacle, (_n, _k, _radii, _lay))
    for _c in (0.15, 0.4):
        for _lay in ("x0", "diag"):
            SCENES[f"pair-{_c}-{_lay}-N{_n}-K{_k}"] = (_pair, (_n, _k, _c, _lay))


def build_scene(name):
    fn, args = SCENES[name]
    return fn(*args)


def check_scene(scene, st, ns, out, which):
    """On the oracle's outputs: nothing moved, `which` straddles the sample and is hit nowhere
    else, the other event did not happen."""
    assert np.array_equal(ns["pos"], st["pos"]) and not ns["vel"].any(), "substeps = 0 must leave the scene in place"
    assert_straddles(out[which], scene["sample"])
    other = "reached" if which == "collision" else "collision"
    assert not out[other].any(), f"an unwanted {other}"


def assert_straddles(hits, sample):
    got = int(hits[sample].sum())
    assert 0 < got < int(sample.sum()), f"the boundary does not run through the sample ({got} hits)"
    assert not hits[~sample].any(), "a hit outside the sample"


# ------------------------------------------------------------------ F. reset and observe
AUX_SHAPES = [(24, 5, 6, 8, 12), (40, 12, 16, 20, 9), (100, 0, 4, 8, 6), (3, 3, 4, 0, 30)]  # N, K, Ms, M, E


def fast_velocities(e, n, max_speed, seed=17):
    """Velocities of which about half are above max_speed (speeds uniform in [0, 2 max_speed])."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(e, n, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return (d * rng.uniform(0.0, 2.0 * max_speed, (e, n, 1))).astype(f32)
