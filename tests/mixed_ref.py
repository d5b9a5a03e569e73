"""CPU reference for batches with per-env drone counts — test-side helper.

What oracle/env_cfg_oracle.py does for the per-env parameters, with the drone count n_e as one
more per-env value: env e of a batch with N slots behaves exactly like env env_offset + e of a
batch built with num_drones = n_e.  So every env is stepped / reset on its own through
oracle.swarm_oracle with its own config, num_drones = n_e and the first n_e agent rows of the
state and actions; the results are scattered back into N-slot arrays with zeros in the slots
that do not exist, and the 6 n_e + 3 global state into the padded 6 N + 3 layout (positions at
[3i, 3i+3), velocities at [3N + 3i, ...), goal at [6N, 6N+3)).  A reset uses the next episode's
parameters and count when given (the device installs them before drawing).
"""
from __future__ import annotations

import numpy as np

from oracle import env_cfg_oracle as eco
from oracle import swarm_oracle as so

f32 = np.float32

AGENT_OUT = ("reward", "terminated", "truncated", "dist_goal", "reached", "collision", "stepped", "has_obs")


def counts_of(counts, e_n: int, n: int) -> np.ndarray:
    c = np.full(e_n, n, np.int64) if counts is None else np.broadcast_to(np.asarray(counts, np.int64), (e_n,)).copy()
    assert c.min() >= 1 and c.max() <= n
    return c


def _slice(state: dict, e: int, n_e: int, m_e: int) -> dict:
    st = {k: np.array(v[e:e + 1], copy=True) for k, v in state.items()}
    for k in ("pos", "vel", "active", "damping"):
        st[k] = st[k][:, :n_e].copy()
    st["obst"] = st["obst"][:, :m_e].copy()
    return st


def _resized(st: dict, n_e: int, m_e: int) -> dict:
    """The env's state with room for n_e drones and m_e obstacles (a reset overwrites them)."""
    out = dict(st)
    out["pos"] = np.zeros((1, n_e, 3), f32)
    out["vel"] = np.zeros((1, n_e, 3), f32)
    out["active"] = np.zeros((1, n_e), bool)
    out["damping"] = np.zeros((1, n_e), f32)
    out["obst"] = np.zeros((1, m_e, 3), f32)
    return out


def _merge_state(dst: dict, src: dict, e: int) -> None:
    for k, v in src.items():
        if k in ("pos", "vel", "active", "damping", "obst"):
            row = np.zeros(dst[k].shape[1:], dst[k].dtype)
            row[:v.shape[1]] = v[0]
            dst[k][e] = row
        else:
            dst[k][e] = v[0]


def pad_agents(v: np.ndarray, n: int) -> np.ndarray:
    """[1, n_e, ...] -> [1, N, ...] with zeros in the slots that do not exist."""
    out = np.zeros((1, n) + v.shape[2:], v.dtype)
    out[:, :v.shape[1]] = v
    return out


def pad_global_state(gs: np.ndarray, n: int) -> np.ndarray:
    """[1, 6 n_e + 3] -> [1, 6 N + 3]: the zero-padded embedding."""
    n_e = (gs.shape[1] - 3) // 6
    out = np.zeros((1, 6 * n + 3), gs.dtype)
    out[:, :3 * n_e] = gs[:, :3 * n_e]
    out[:, 3 * n:3 * n + 3 * n_e] = gs[:, 3 * n_e:6 * n_e]
    out[:, 6 * n:] = gs[:, 6 * n_e:]
    return out


def _cfg(base: dict, over: dict | None, e: int, n_e: int) -> dict:
    cfg = eco.env_cfg(base, over, e)
    cfg["num_drones"] = int(n_e)
    return cfg


def step(base: dict, cur: dict | None, counts, state: dict, actions, *, nxt: dict | None = None,
         counts_next=None, auto_reset: bool = True, seed: int = 0, env_offset: int = 0, physics: bool = False,
         action_mask=None):
    """One step of every env.  Returns (new_state, out, new_cur, new_counts): the overrides and
    counts in force after the step (the next-episode ones for envs that reset).  action_mask
    [E, N] (True = the drone sent an action): env e sees its first n_e entries."""
    e_n, n = state["pos"].shape[:2]
    cnt = counts_of(counts, e_n, n)
    cnt_next = None if counts_next is None else counts_of(counts_next, e_n, n)
    new_state = {k: np.array(v, copy=True) for k, v in state.items()}
    new_cnt = cnt.copy()
    new_cur = {k: (np.array(np.broadcast_to(np.asarray(v), (e_n,)), copy=True) if v is not None else None)
               for k, v in (cur or {}).items()}
    for k in (nxt or {}):
        if k not in new_cur or new_cur[k] is None:
            new_cur[k] = np.array([eco.env_cfg(base, cur, e)[k] for e in range(e_n)])
    outs = []
    actions = np.asarray(actions)
    am = None if action_mask is None else np.asarray(action_mask, bool)
    for e in range(e_n):
        n_e = int(cnt[e])
        cfg_e = _cfg(base, cur, e, n_e)
        st_e = _slice(state, e, n_e, cfg_e["num_obstacles"])
        ns, o = so.step(cfg_e, st_e, actions[e:e + 1, :n_e], None if am is None else am[e:e + 1, :n_e],
                        auto_reset=False, seed=seed, env_offset=env_offset + e, physics=physics)
        done = bool(o["term_all"][0] or o["trunc_all"][0])
        out = {k: pad_agents(o[k], n) for k in AGENT_OUT}
        out["term_all"], out["trunc_all"] = o["term_all"], o["trunc_all"]
        out["reset"] = np.array([done and auto_reset])
        obs, gs = o["obs"], o["global_state"]
        if done and auto_reset:
            n_new = n_e if cnt_next is None else int(cnt_next[e])
            cfg_n = _cfg(base, nxt if nxt else cur, e, n_new)
            if nxt:
                for k in nxt:
                    new_cur[k][e] = cfg_n[k]
            new_cnt[e] = n_new
            ns, ro = so.reset_device(cfg_n, _resized(ns, n_new, cfg_n["num_obstacles"]), seed=seed,
                                     env_offset=env_offset + e, physics=physics)
            obs, gs = ro["obs"], ro["global_state"]
        out["obs"] = pad_agents(obs, n)
        out["global_state"] = pad_global_state(gs, n)
        _merge_state(new_state, ns, e)
        outs.append(out)
    stacked = {k: np.concatenate([o[k] for o in outs], axis=0) for k in outs[0]}
    return new_state, stacked, new_cur, new_cnt


def reset(base: dict, cur: dict | None, counts, state: dict, *, nxt: dict | None = None, counts_next=None,
          env_mask=None, seed: int = 0, env_offset: int = 0, physics: bool = False):
    """swarm_reset of the masked envs (all if None); the next-episode parameters and counts when
    given.  Returns (new_state, out, new_counts); out rows of envs outside the mask are zero."""
    e_n, n = state["pos"].shape[:2]
    cnt = counts_of(counts, e_n, n)
    cnt_next = None if counts_next is None else counts_of(counts_next, e_n, n)
    mask = np.ones(e_n, bool) if env_mask is None else np.asarray(env_mask, bool)
    new_state = {k: np.array(v, copy=True) for k, v in state.items()}
    new_cnt = cnt.copy()
    d = so.obs_dim(base)
    out = dict(obs=np.zeros((e_n, n, d), f32), dist_goal=np.zeros((e_n, n), f32),
               global_state=np.zeros((e_n, 6 * n + 3), f32))
    for e in range(e_n):
        if not mask[e]:
            continue
        n_e = int(cnt[e]) if cnt_next is None else int(cnt_next[e])
        cfg_e = _cfg(base, nxt if nxt else cur, e, n_e)
        st_e = _resized(_slice(state, e, 0, 0), n_e, cfg_e["num_obstacles"])
        ns, ro = so.reset_device(cfg_e, st_e, seed=seed, env_offset=env_offset + e, physics=physics)
        new_cnt[e] = n_e
        _merge_state(new_state, ns, e)
        out["obs"][e] = pad_agents(ro["obs"], n)[0]
        out["dist_goal"][e] = pad_agents(ro["dist_goal"], n)[0]
        out["global_state"][e] = pad_global_state(ro["global_state"], n)[0]
    return new_state, out, new_cnt


def observe(base: dict, cur: dict | None, counts, state: dict, env_mask=None, physics: bool = False,
            out: dict | None = None) -> dict:
    """swarm_observe of the masked envs (all if None): obs [E, N, D], dist_goal [E, N] and
    global_state [E, 6N + 3] of the current state, each env observed on its own with
    num_drones = n_e (so.observe / so.global_state) and padded with zeros.  Rows of envs outside
    the mask are left as they are in `out` (a dict of the three arrays, written in place), NaN
    when no `out` is given.  The state is not touched."""
    e_n, n = state["pos"].shape[:2]
    cnt = counts_of(counts, e_n, n)
    mask = np.ones(e_n, bool) if env_mask is None else np.asarray(env_mask, bool)
    d = so.obs_dim(base)
    if out is None:
        out = dict(obs=np.full((e_n, n, d), np.nan, f32), dist_goal=np.full((e_n, n), np.nan, f32),
                   global_state=np.full((e_n, 6 * n + 3), np.nan, f32))
    for e in range(e_n):
        if not mask[e]:
            continue
        n_e = int(cnt[e])
        cfg_e = _cfg(base, cur, e, n_e)
        st = _slice(state, e, n_e, cfg_e["num_obstacles"])
        obs = so.observe(cfg_e, st["pos"], st["vel"], st["goal"], st["obst"], physics=physics)
        out["obs"][e] = pad_agents(obs, n)[0]
        out["dist_goal"][e] = pad_agents(so.norm1d(st["goal"][:, None, :] - st["pos"]), n)[0]
        out["global_state"][e] = pad_global_state(so.global_state(st["pos"], st["vel"], st["goal"]), n)[0]
    return out


def info_flags(out: dict) -> np.ndarray:
    """SWARM_AGENT_* bits of a step's out dict."""
    st = out["stepped"].astype(bool)
    return (st.astype(np.uint8) | ((st & out["reached"]).astype(np.uint8) << 1) |
            ((st & out["collision"]).astype(np.uint8) << 2) | (out["has_obs"].astype(np.uint8) << 3))
