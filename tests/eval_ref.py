"""Dense float64 reference of the evaluation protocol — TEST INFRASTRUCTURE ONLY.

Nothing under swarm_marl_amd/ may import this module.  oracle/eval_oracle.EpisodeMetrics walks the
dict outputs of one env and calls np.linalg.norm once per pair (19 ms per env-step at N = 64);
`DenseEvalRef` follows the same protocol (evaluate_protocol.py:103-116, :237-331) from the dense
step outputs of E envs at once: obs[..., 0:3] / obs[..., 6:9], reward, info_flags, env_done.  It is
written from the protocol and oracle/eval_oracle.py, not from the kernels, and pinned to the oracle
and to the reference-made tests/golden/eval_*.npz by tests/test_eval_cpu.py.

* only agents with HAS_OBS move, vote and enter the formation set; the reward mean is over the
  STEPPED agents; the terminal step has no observations, so it passes "all reached" vacuously;
  a restart (ENV_RESET) opens the next episode from the same step's observations (every agent).
* distance: f32 difference, f32 squares, ((double)xx + yy) + zz rounded to f32, f32 sqrt — the
  float(np.linalg.norm(a - b)) of float32 3-vectors, bit for bit.
* formation error: an n x n array, sum |d - d*| / (n (n - 1)).
* counters (`counts`): live env-steps by the size of the observed set, episode ends by cause,
  episodes opened at a restart; `sq_below` / `sq_above` / `sq_equal`: observed pairs whose squared
  distance (the f32 under the square root) lies below / at or above 2^-96, or is zero.

Also here: the goal-seeking action rule and the parameter points the eval tests share, and an
oracle rollout (oracle/swarm_oracle.step with auto-reset) that yields the same dense arrays on the
CPU.
"""
from __future__ import annotations

import math

import numpy as np

f32, f64 = np.float32, np.float64
STEPPED, REACHED, COLLISION, HAS_OBS = 1, 2, 4, 8  # SWARM_AGENT_* (include/swarm_mi355x.h)
TERMINATED, TRUNCATED, RESET = 1, 2, 4             # SWARM_ENV_*
FIELDS = ("env", "success", "collision_free", "time_to_goal", "formation_error", "path_efficiency",
          "episode_reward", "steps", "update")
TINY_SQ = f32(2.0 ** -96)  # below this the kernels' square roots take their scaled path

# parameter points (every value not listed is the DroneEnvConfig default).  Four obstacles of
# radius 0 keep num_obstacles >= 4 (the specialised step kernels need it) without obstacle hits.
POINTS = {
    "reach": dict(world_size=10.0, goal_radius=7.0, collision_radius=0.01, num_obstacles=4, obstacle_radius=0.0,
                  max_steps=30),
    "full": dict(collision_radius=0.02, num_obstacles=4, obstacle_radius=0.0, max_steps=12),
    "collide": dict(goal_radius=6.0, max_steps=25),
}


def point_cfg(point: str, n: int) -> dict:
    cfg = dict(POINTS[point], num_drones=int(n))
    if n >= 256 and point != "collide":
        cfg["collision_radius"] = 0.002  # dense swarms: keep pair collisions out of these two points
    return cfg


def goal_actions(obs: np.ndarray, rng: np.random.Generator) -> np.ndarray:
    """Unit goal direction (obs[..., 6:9]) + 0.5 U(-1, 1), clipped to [-1, 1]; all float32."""
    g = np.asarray(obs[..., 6:9], f32)
    nrm = np.sqrt((g * g).sum(axis=-1, dtype=f32, keepdims=True))
    unit = g / np.maximum(nrm, f32(1e-12))
    noise = rng.uniform(-1.0, 1.0, g.shape).astype(f32)
    return np.clip(unit + f32(0.5) * noise, f32(-1.0), f32(1.0)).astype(f32)


def distance(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """|a - b| of float32 3-vectors along the last axis, as float32; also returns the f32 square."""
    d = np.asarray(a, f32) - np.asarray(b, f32)
    sq = d * d
    s = ((sq[..., 0].astype(f64) + sq[..., 1].astype(f64)) + sq[..., 2].astype(f64)).astype(f32)
    return np.sqrt(s), s


class DenseEvalRef:
    def __init__(self, num_envs: int, num_drones: int, spacing: float = 2.5, env_offset: int = 0):
        e, n = int(num_envs), int(num_drones)
        self.e, self.n, self.spacing, self.env_offset = e, n, float(spacing), int(env_offset)
        self.live = np.zeros(e, bool)
        self.start = np.zeros((e, n, 3), f32)
        self.goal = np.zeros((e, n, 3), f32)
        self.last = np.zeros((e, n, 3), f32)
        self.traveled = np.zeros((e, n), f64)
        self.reward = np.zeros(e, f64)
        self.abs_reward = np.zeros(e, f64)  # sum_t mean_i |r_ti| of the open episode
        self.steps = np.zeros(e, np.int64)
        self.reached_step = np.full(e, -1, np.int64)
        self.collided = np.zeros(e, bool)
        self.fe = [[] for _ in range(e)]
        self.updates = 0
        self._rows, self._abs = [], []
        self.counts = dict(full=0, partial=0, two=0, one=0, zero=0, end_collision=0, end_time_limit=0,
                           end_all_reached=0, restarts=0, sq_below=0, sq_above=0, sq_equal=0)

    # ------------------------------------------------------------------ episodes
    def _open(self, idx, obs):
        p = np.asarray(obs[idx][..., 0:3], f32)
        self.start[idx] = p
        self.goal[idx] = p + np.asarray(obs[idx][..., 6:9], f32)
        self.last[idx] = p
        self.traveled[idx] = 0.0
        self.reward[idx] = 0.0
        self.abs_reward[idx] = 0.0
        self.steps[idx] = 0
        self.reached_step[idx] = -1
        self.collided[idx] = False
        for i in idx:
            self.fe[i] = []
        self.live[idx] = True

    def begin(self, obs: np.ndarray, env_mask=None) -> None:
        """Open an episode in the masked envs (all if None) from the current observations."""
        mask = np.ones(self.e, bool) if env_mask is None else np.asarray(env_mask, bool)
        self._open(np.nonzero(mask)[0], np.asarray(obs))

    def clear(self) -> None:
        """Drop the finished-episode records (the open episodes go on)."""
        self._rows, self._abs = [], []

    # ------------------------------------------------------------------ one step
    def _formation_error(self, pos, has):
        """[E]: sum over ordered observed pairs of |d - d*| over n (n - 1); 0 where n <= 1."""
        n_obs = has.sum(axis=1)
        d, s = distance(pos[:, :, None, :], pos[:, None, :, :])
        pair = has[:, :, None] & has[:, None, :] & ~np.eye(self.n, dtype=bool)[None]
        pair &= self.live[:, None, None]
        self.counts["sq_equal"] += int((pair & (s == 0)).sum()) // 2
        self.counts["sq_below"] += int((pair & (s > 0) & (s < TINY_SQ)).sum()) // 2
        self.counts["sq_above"] += int((pair & (s >= TINY_SQ)).sum()) // 2
        err = np.where(pair, np.abs(d.astype(f64) - self.spacing), 0.0).sum(axis=(1, 2))
        den = np.maximum(n_obs * (n_obs - 1), 1).astype(f64)
        return np.where(n_obs > 1, err / den, 0.0)

    def update(self, obs, reward, info_flags, env_done) -> None:
        obs = np.asarray(obs)
        fl = np.asarray(info_flags).astype(np.uint8)
        done = np.asarray(env_done).astype(np.uint8)
        rew = np.asarray(reward).astype(f64)
        self.updates += 1
        live = self.live.copy()
        stepped = (fl & STEPPED) != 0
        has = (fl & HAS_OBS) != 0
        assert not (has & ~stepped)[live].any(), "an agent with an observation that was not stepped"
        pos = np.asarray(obs[..., 0:3], f32)
        # reward: mean over the stepped agents (the rewards dict)
        n_st = stepped.sum(axis=1)
        for i in np.nonzero(live & (n_st > 0))[0]:
            r = rew[i][stepped[i]]
            self.reward[i] += float(np.mean(r))
            self.abs_reward[i] += float(np.mean(np.abs(r)))
        self.steps[live] += 1
        # observed agents: path length, votes
        inc, _ = distance(self.last, pos)
        mv = has & live[:, None]
        self.traveled[mv] += inc[mv].astype(f64)
        self.last[mv] = pos[mv]
        self.collided |= live & (has & ((fl & COLLISION) != 0)).any(axis=1)
        all_reached = ~(has & ((fl & REACHED) == 0)).any(axis=1)
        fe = self._formation_error(pos, has)
        n_obs = has.sum(axis=1)
        for i in np.nonzero(live)[0]:
            self.fe[i].append(float(fe[i]))
            k = int(n_obs[i])
            self.counts["full" if k == self.n else "zero" if k == 0 else "one" if k == 1 else
                        "two" if k == 2 else "partial"] += 1
        first = live & all_reached & (self.reached_step < 0)
        self.reached_step[first] = self.steps[first]
        # episode ends
        ends = live & ((done & (TERMINATED | TRUNCATED)) != 0)
        for i in np.nonzero(ends)[0]:
            straight, _ = distance(self.start[i], self.goal[i])
            t = self.traveled[i]
            pe = np.where(t > 1e-8, straight.astype(f64) / np.where(t > 1e-8, t, 1.0), 0.0)
            rs = int(self.reached_step[i])
            coll = bool(self.collided[i])
            self._rows.append([float(self.env_offset + i), float((not coll) and rs >= 0), float(not coll),
                               float(rs) if rs >= 0 else math.nan, float(np.mean(self.fe[i])), float(np.mean(pe)),
                               float(self.reward[i]), float(self.steps[i]), float(self.updates)])
            self._abs.append(float(self.abs_reward[i]))
            if done[i] & TRUNCATED:
                self.counts["end_time_limit"] += 1
            elif (stepped[i] & ((fl[i] & COLLISION) != 0)).any():
                self.counts["end_collision"] += 1
            else:
                self.counts["end_all_reached"] += 1
        self.live[ends] = False
        again = np.nonzero(ends & ((done & RESET) != 0))[0]
        if len(again):
            self._open(again, obs)
            self.counts["restarts"] += len(again)

    # ------------------------------------------------------------------ results
    def _order(self):
        rows = np.asarray(self._rows, f64).reshape(-1, len(FIELDS))
        return rows, np.lexsort((rows[:, 0], rows[:, 8]))

    def records(self) -> np.ndarray:
        """[n, 9] in FIELDS order, by the update that closed them, then by global env index."""
        rows, o = self._order()
        return rows[o]

    def abs_rewards(self) -> np.ndarray:
        """sum_t mean_i |r_ti| of each record, in records() order."""
        _, o = self._order()
        return np.asarray(self._abs, f64)[o]


class DenseSingleRef:
    """evaluate_protocol.py:193-234 (SingleDroneEnv) for E single-drone envs: the terminal step's
    info and position count; formation error 0.  `update` takes the state position after the step
    and, for the envs that ended, the observation of their next episode (`begin`)."""

    def __init__(self, num_envs: int, env_offset: int = 0):
        e = int(num_envs)
        self.e, self.env_offset = e, int(env_offset)
        self.live = np.zeros(e, bool)
        self.start = np.zeros((e, 3), f32)
        self.goal = np.zeros((e, 3), f32)
        self.last = np.zeros((e, 3), f32)
        self.traveled = np.zeros(e, f64)
        self.reward = np.zeros(e, f64)
        self.abs_reward = np.zeros(e, f64)
        self.steps = np.zeros(e, np.int64)
        self.reached_step = np.full(e, -1, np.int64)
        self.collided = np.zeros(e, bool)
        self.updates = 0
        self._rows, self._abs = [], []
        self.counts = dict(end_goal=0, end_collision=0, end_time_limit=0, reopened=0)

    def begin(self, obs, env_mask=None, reopened=False) -> None:
        mask = np.ones(self.e, bool) if env_mask is None else np.asarray(env_mask, bool)
        o = np.asarray(obs, f32).reshape(self.e, -1)
        self.start[mask] = o[mask, 0:3]
        self.goal[mask] = o[mask, 0:3] + o[mask, 6:9]
        self.last[mask] = o[mask, 0:3]
        for a in (self.traveled, self.reward, self.abs_reward, self.steps):
            a[mask] = 0
        self.reached_step[mask] = -1
        self.collided[mask] = False
        self.live[mask] = True
        if reopened:
            self.counts["reopened"] += int(mask.sum())

    def update(self, pos, reward, info_flags, env_done) -> np.ndarray:
        """Returns the mask of the envs whose episode ended (to be reset and begun again)."""
        pos = np.asarray(pos, f32).reshape(self.e, 3)
        fl = np.asarray(info_flags).astype(np.uint8).reshape(self.e)
        done = np.asarray(env_done).astype(np.uint8).reshape(self.e)
        rew = np.asarray(reward).astype(f64).reshape(self.e)
        self.updates += 1
        live = self.live & ((fl & STEPPED) != 0)
        self.steps[live] += 1
        self.reward[live] += rew[live]
        self.abs_reward[live] += np.abs(rew[live])
        inc, _ = distance(self.last, pos)
        self.traveled[live] += inc[live].astype(f64)
        self.last[live] = pos[live]
        self.collided |= live & ((fl & COLLISION) != 0)
        first = live & ((fl & REACHED) != 0) & (self.reached_step < 0)
        self.reached_step[first] = self.steps[first]
        ends = live & ((done & (TERMINATED | TRUNCATED)) != 0)
        for i in np.nonzero(ends)[0]:
            straight, _ = distance(self.start[i], self.goal[i])
            t = float(self.traveled[i])
            rs, coll = int(self.reached_step[i]), bool(self.collided[i])
            self._rows.append([float(self.env_offset + i), float((not coll) and rs >= 0), float(not coll),
                               float(rs) if rs >= 0 else math.nan, 0.0, float(straight) / t if t > 1e-8 else 0.0,
                               float(self.reward[i]), float(self.steps[i]), float(self.updates)])
            self._abs.append(float(self.abs_reward[i]))
            self.counts["end_time_limit" if done[i] & TRUNCATED else
                        "end_collision" if fl[i] & COLLISION else "end_goal"] += 1
        self.live[ends] = False
        return ends

    records = DenseEvalRef.records
    abs_rewards = DenseEvalRef.abs_rewards
    _order = DenseEvalRef._order


# ---------------------------------------------------------------------- CPU rollout (oracle)
def oracle_flags(out: dict) -> tuple:
    """(info_flags [E, N] u8, env_done [E] u8) of oracle/swarm_oracle.step's output."""
    fl = (out["stepped"] * STEPPED + out["reached"] * REACHED + out["collision"] * COLLISION +
          out["has_obs"] * HAS_OBS).astype(np.uint8)
    done = (out["term_all"] * TERMINATED + out["trunc_all"] * TRUNCATED + out["reset"] * RESET).astype(np.uint8)
    return fl, done


def oracle_rollout(raw_cfg: dict, num_envs: int, steps: int, seed: int, noise_seed: int, exact_formation=True):
    """Yields the reset observation, then per step (obs, reward f32, info_flags, env_done, out) of
    oracle/swarm_oracle with auto-reset under the goal-seeking action rule."""
    from oracle import swarm_oracle as so
    cfg = so.make_cfg(**raw_cfg)
    st, out = so.reset_device(cfg, so.empty_state(cfg, num_envs), seed=seed)
    obs = out["obs"]
    yield obs
    rng = np.random.default_rng(noise_seed)
    for _ in range(steps):
        st, out = so.step(cfg, st, goal_actions(obs, rng), auto_reset=True, seed=seed,
                          exact_formation=exact_formation)
        obs = out["obs"]
        fl, done = oracle_flags(out)
        yield obs, out["reward"].astype(f32), fl, done, out
