"""GPU: per-env drone counts (swarm_env_cfg_t.num_drones, swarm_env_cfg_set_drones) — swarms of
different sizes in one batch.

* uniform counts change nothing: records given num_drones = N equal plain records bit for bit
  (several teams per wave, one team per wave with packed byte stores, block teams with the pair
  ring), over steps with in-kernel resets;
* mixed counts match the reference that steps every env on its own with num_drones = n_e
  (tests/mixed_ref.py): obs bit-exact, rewards within 1e-5, flags, env_done
  and state exact, every output of a slot that does not exist exactly zero;
* next-episode counts take over at resets (auto and explicit), growing and shrinking;
* the padded global_state layout, env groups, later parameter changes keeping the counts.
Reference: src/swarm_marl/envs/drone_swarm_env.py:28-174, :245-271 (neighbour features rank the
env's num_drones), configs/curriculum_v1.yaml (3 -> 5 -> 8 drones).
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import mixed_ref as mr
from tests.helpers import oracle_cfg, vec_state_numpy

pytestmark = pytest.mark.gpu
REWARD_TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _actions(dev, t, e, n, scale=2.0):
    g = torch.Generator(device=dev).manual_seed(7300 + t)
    return (torch.rand((e, n, 3), device=dev, generator=g) * 2 - 1) * scale


def _snap(vec):
    return [t.clone() for t in (vec.obs, vec.reward, vec.terminated, vec.truncated, vec.env_done,
                                vec.pos, vec.vel, vec.goal, vec.obstacles, vec.active,
                                vec.step_count, vec.episode, vec.damping)]


@pytest.mark.parametrize("n,e", [(8, 40), (64, 6), (128, 3)])
def test_uniform_counts_change_nothing(dev, n, e):
    from swarm_marl_amd import VecSwarm
    cfg = {"num_drones": n, "max_steps": 7}
    a_vec = VecSwarm(e, cfg, device=dev, auto_reset=True, seed=11)
    b_vec = VecSwarm(e, cfg, device=dev, auto_reset=True, seed=11)
    a_vec.set_env_config()  # plain records (count field 0)
    b_vec.set_env_config(num_drones=n)
    assert a_vec.kernel_name() == b_vec.kernel_name() and b_vec.kernel_name().startswith("swarm_kernel<")
    assert int(b_vec.env_config()["num_drones"].min()) == n
    a_vec.reset()
    b_vec.reset()
    resets = 0
    for t in range(16):
        a = _actions(dev, t, e, n, scale=1.0)
        a_vec.step(a)
        b_vec.step(a)
        for k, (x, y) in enumerate(zip(_snap(a_vec), _snap(b_vec))):
            assert torch.equal(x, y), f"t={t} field {k}"
        resets += int(((a_vec.env_done & 4) != 0).sum())
    assert resets >= e, "the run must cross episode boundaries"


def _ghost(counts, n):
    return np.arange(n)[None, :] >= np.asarray(counts)[:, None]


def _compare_state(vec, ns, what, physics=False):
    st = vec_state_numpy(vec)
    for k in ("pos", "vel", "goal", "obst", "active", "step", "episode") + (("damping",) if physics else ()):
        assert np.array_equal(st[k], ns[k]), f"{what}: state {k} differs at {np.argwhere(st[k] != ns[k])[:4]}"


def _compare(vec, ns, out, counts_before, counts_after, what, physics=False):
    """One step's outputs and state against the reference; counts_before are the counts of the
    episode stepped (reward, flags), counts_after those of the state and observation left."""
    n = vec.num_drones
    obs = vec.obs.cpu().numpy()
    assert np.array_equal(obs, out["obs"]), f"{what}: obs differ in {np.argwhere(obs != out['obs'])[:4]}"
    rew = vec.reward.cpu().numpy()
    err = np.abs(rew.astype(np.float64) - out["reward"]).max()
    assert err < REWARD_TOL, f"{what}: reward error {err}"
    assert np.array_equal(vec.terminated.cpu().numpy(), out["terminated"]), what
    assert np.array_equal(vec.truncated.cpu().numpy(), out["truncated"]), what
    bits = out["term_all"].astype(np.uint8) | (out["trunc_all"].astype(np.uint8) << 1) | \
        (out["reset"].astype(np.uint8) << 2)
    assert np.array_equal(vec.env_done.cpu().numpy(), bits), what
    if vec.dist_goal is not None:
        assert np.array_equal(vec.dist_goal.cpu().numpy(), out["dist_goal"]), f"{what}: dist_goal"
        assert np.array_equal(vec.info_flags.cpu().numpy(), mr.info_flags(out)), f"{what}: info_flags"
    if vec.global_state is not None:
        assert np.array_equal(vec.global_state.cpu().numpy(), out["global_state"]), f"{what}: global_state"
    _compare_state(vec, ns, what, physics)
    # slots that do not exist: exactly zero in every output
    gb, ga = _ghost(counts_before, n), _ghost(counts_after, n)
    assert not rew[gb].any() and not vec.terminated.cpu().numpy()[gb].any()
    assert not vec.truncated.cpu().numpy()[gb].any()
    assert not obs[ga].any() and not vec.active.cpu().numpy()[ga].any()
    assert not vec.pos.cpu().numpy()[ga].any() and not vec.vel.cpu().numpy()[ga].any()
    if vec.dist_goal is not None:
        assert not vec.dist_goal.cpu().numpy()[gb].any() and not vec.info_flags.cpu().numpy()[gb].any()


def _overrides(e, m, rng):
    return dict(world_size=rng.uniform(12.0, 30.0, e), max_speed=rng.uniform(2.0, 6.0, e),
                max_accel=rng.uniform(1.0, 3.5, e), obstacle_radius=rng.uniform(0.4, 1.4, e),
                max_steps=rng.integers(4, 9, e).astype(np.int32), dt=rng.uniform(0.05, 0.2, e),
                num_obstacles=np.resize(np.array([0, 1, 3, m, m - 1, 2], np.int32), e))


MIXED_CASES = [
    # counts <= K = 3 leave neighbour slots empty
    pytest.param(8, 12, 6, "kinematic", [1, 2, 3, 4, 5, 8], 14, False, id="N8"),
    pytest.param(64, 4, 8, "kinematic", [64, 33, 5, 1], 8, False, id="N64"),
    pytest.param(128, 3, 6, "kinematic", [128, 100, 3], 7, False, id="N128"),
    pytest.param(4, 8, 5, "physics", [1, 2, 3, 4], 12, False, id="physics"),
    pytest.param(8, 12, 6, "kinematic", [1, 2, 3, 4, 5, 8], 14, True, id="N8-overrides"),
]


@pytest.mark.parametrize("n,e,m,dyn,pattern,steps,with_ov", MIXED_CASES)
def test_mixed_counts_vs_reference(dev, n, e, m, dyn, pattern, steps, with_ov):
    from swarm_marl_amd import VecSwarm
    physics = dyn == "physics"
    raw = {"num_drones": n, "num_obstacles": m, "max_steps": 6}
    base = oracle_cfg(raw)
    counts = np.resize(np.array(pattern, np.int32), e)
    ov = _overrides(e, m, np.random.default_rng(n + e)) if with_ov else {}
    vec = VecSwarm(e, raw, device=dev, auto_reset=True, seed=23, dynamics=dyn, with_infos=True,
                   with_global_state=True)
    vec.set_env_config(num_drones=counts, **ov)
    assert vec.kernel_name().startswith("swarm_kernel<")
    assert np.array_equal(vec.env_config()["num_drones"].cpu().numpy(), counts)
    st0 = vec_state_numpy(vec)
    vec.reset()
    torch.cuda.synchronize()
    ns, ro, _ = mr.reset(base, ov, counts, st0, seed=23, physics=physics)
    assert np.array_equal(vec.obs.cpu().numpy(), ro["obs"]), "reset obs"
    assert np.array_equal(vec.dist_goal.cpu().numpy(), ro["dist_goal"]), "reset dist_goal"
    assert np.array_equal(vec.global_state.cpu().numpy(), ro["global_state"]), "reset global_state"
    _compare_state(vec, ns, "reset", physics)
    resets = 0
    for t in range(steps):
        a = _actions(dev, t, e, n)
        st = vec_state_numpy(vec)
        vec.step(a)
        torch.cuda.synchronize()
        ns, out, _, _ = mr.step(base, ov, counts, st, a.cpu().numpy(), seed=23, physics=physics)
        _compare(vec, ns, out, counts, counts, f"N={n} {dyn} t={t}", physics)
        resets += int(out["reset"].sum())
    assert resets > 0, "the run must cross episode boundaries"


def test_next_episode_counts(dev):
    """3 -> 5 -> 8 and 8 -> 3 across auto-resets and an explicit masked reset: a slot that
    disappears is zero from the reset on, one that appears is drawn like the uniform batch's."""
    from swarm_marl_amd import VecSwarm
    n, e, m = 8, 8, 6
    raw = {"num_drones": n, "num_obstacles": m, "max_steps": 4}
    base = oracle_cfg(raw)
    cur = np.array([3, 3, 5, 5, 8, 8, 3, 8], np.int32)
    nxt1 = np.array([5, 5, 8, 8, 3, 3, 5, 3], np.int32)
    nxt2 = np.array([8, 8, 3, 3, 5, 5, 8, 5], np.int32)
    vec = VecSwarm(e, raw, device=dev, auto_reset=True, seed=31, with_infos=True, with_global_state=True)
    vec.set_env_config(num_drones=cur)
    st0 = vec_state_numpy(vec)
    vec.reset()
    torch.cuda.synchronize()
    ns, _, cnt = mr.reset(base, {}, cur, st0, seed=31)
    _compare_state(vec, ns, "first reset")
    vec.set_env_config(next_episode=True, num_drones=nxt1)
    assert np.array_equal(vec.env_config()["num_drones"].cpu().numpy(), cur)  # not before a reset
    assert np.array_equal(vec.env_config(True)["num_drones"].cpu().numpy(), nxt1)
    # explicit reset of every other env: those switch to the next-episode counts at once
    mask = torch.zeros(e, dtype=torch.bool, device=dev)
    mask[::2] = True
    st = vec_state_numpy(vec)
    vec.reset(mask)
    torch.cuda.synchronize()
    ns, ro, cnt = mr.reset(base, {}, cnt, st, counts_next=nxt1, env_mask=mask.cpu().numpy(), seed=31)
    _compare_state(vec, ns, "masked reset")
    sel = mask.cpu().numpy()
    assert np.array_equal(vec.obs.cpu().numpy()[sel], ro["obs"][sel])
    assert np.array_equal(vec.global_state.cpu().numpy()[sel], ro["global_state"][sel])
    assert np.array_equal(vec.env_config()["num_drones"].cpu().numpy(), cnt)
    assert np.array_equal(cnt, np.where(sel, nxt1, cur))
    seen = {int(c) for c in cnt}
    counts_next, resets = nxt1, 0
    for t in range(12):
        if t == 5:  # every env has reset at least once (max_steps = 4): queue the second move
            vec.set_env_config(next_episode=True, num_drones=nxt2)
            counts_next = nxt2
        a = _actions(dev, t, e, n)
        st = vec_state_numpy(vec)
        vec.step(a)
        torch.cuda.synchronize()
        ns, out, _, cnt_new = mr.step(base, {}, cnt, st, a.cpu().numpy(), counts_next=counts_next, seed=31)
        _compare(vec, ns, out, cnt, cnt_new, f"next-episode t={t}")
        assert np.array_equal(vec.env_config()["num_drones"].cpu().numpy(), cnt_new), f"t={t}"
        resets += int(out["reset"].sum())
        cnt = cnt_new
        seen |= {int(c) for c in cnt}
    assert resets >= 2 * e and seen == {3, 5, 8}
    assert np.array_equal(cnt, nxt2)  # 3 -> 5 -> 8, 5 -> 8 -> 3, 8 -> 3 -> 5


def test_global_state_layout(dev):
    """global_state keeps its 6N + 3 row: slot i position at [3i, 3i+3), velocity at
    [3N + 3i, ...), goal at [6N, 6N+3), zeros for slots that do not exist."""
    from swarm_marl_amd import VecSwarm
    n, e = 8, 4
    counts = np.array([3, 8, 1, 5], np.int32)
    vec = VecSwarm(e, {"num_drones": n, "max_steps": 50}, device=dev, auto_reset=True, seed=5, with_global_state=True)
    vec.set_env_config(num_drones=counts)
    vec.reset()
    for t in range(3):
        vec.step(_actions(dev, t, e, n))
    torch.cuda.synchronize()
    gs = vec.global_state.cpu().numpy()
    pos, vel, goal = vec.pos.cpu().numpy(), vec.vel.cpu().numpy(), vec.goal.cpu().numpy()
    assert gs.shape == (e, 6 * n + 3)
    assert np.array_equal(gs[:, :3 * n], pos.reshape(e, -1)) and np.array_equal(gs[:, 3 * n:6 * n], vel.reshape(e, -1))
    assert np.array_equal(gs[:, 6 * n:], goal)
    ghost = _ghost(counts, n)
    assert not pos[ghost].any() and not vel[ghost].any() and vel[~ghost].any()
    for i, c in enumerate(counts):  # the zero-padded embedding of the 6 n_e + 3 vector
        small = np.concatenate([pos[i, :c].ravel(), vel[i, :c].ravel(), goal[i]])[None]
        assert np.array_equal(mr.pad_global_state(small, n)[0], gs[i])


def test_groups_with_mixed_counts(dev):
    """Two env groups whose boundary (env 5 of 10) splits unequal counts: bitwise the ungrouped
    batch, and the reference."""
    from swarm_marl_amd import VecSwarm
    n, e, m = 8, 10, 6
    raw = {"num_drones": n, "num_obstacles": m, "max_steps": 5}
    base = oracle_cfg(raw)
    counts = np.resize(np.array([1, 2, 3, 4, 5, 8], np.int32), e)
    vec = VecSwarm(e, raw, device=dev, auto_reset=True, seed=13, groups=2, with_infos=True)
    one = VecSwarm(e, raw, device=dev, auto_reset=True, seed=13, groups=1, with_infos=True)
    assert vec.group_slices == [(0, 5), (5, 10)]
    mask = torch.ones(e, dtype=torch.bool, device=dev)
    mask[3] = False
    for v in (vec, one):
        v.set_env_config(num_drones=n)
        v.set_env_config(num_drones=counts, env_mask=mask)  # env 3 keeps all 8 slots
    counts[3] = n
    assert np.array_equal(vec.env_config()["num_drones"].cpu().numpy(), counts)
    st0 = vec_state_numpy(vec)
    vec.reset()
    one.reset()
    torch.cuda.synchronize()
    ns, _, _ = mr.reset(base, {}, counts, st0, seed=13)
    _compare_state(vec, ns, "reset")
    resets = 0
    for t in range(10):
        a = _actions(dev, t, e, n)
        st = vec_state_numpy(vec)
        vec.step(a)
        one.step(a)
        torch.cuda.synchronize()
        for k, (x, y) in enumerate(zip(_snap(vec), _snap(one))):
            assert torch.equal(x, y), f"t={t} field {k}"
        ns, out, _, _ = mr.step(base, {}, counts, st, a.cpu().numpy(), seed=13)
        _compare(vec, ns, out, counts, counts, f"groups t={t}")
        resets += int(out["reset"].sum())
    assert resets > 0


def test_later_parameter_change_keeps_counts(dev):
    from swarm_marl_amd import VecSwarm
    n, e = 8, 6
    cur = np.array([1, 2, 3, 4, 5, 8], np.int32)
    nxt = np.array([8, 5, 4, 3, 2, 1], np.int32)
    vec = VecSwarm(e, {"num_drones": n, "max_steps": 3}, device=dev, auto_reset=True, seed=3)
    with pytest.raises(ValueError):
        vec.set_env_config(num_drones=0)
    with pytest.raises(ValueError):
        vec.set_env_config(num_drones=np.array([1, 2, 3, 4, 5, 9]))
    with pytest.raises(ValueError):
        vec.set_env_config(num_drones=[1, 2, 3])
    assert vec.env_cfg is None  # refused before any record was made
    vec.set_env_config(num_drones=cur)
    vec.set_env_config(next_episode=True, num_drones=nxt)
    vec.reset(torch.zeros(e, dtype=torch.bool, device=dev))  # no env selected: nothing moves
    ws = np.linspace(14.0, 24.0, e)
    vec.set_env_config(world_size=ws)
    vec.set_env_config(next_episode=True, world_size=ws + 1.0, env_mask=torch.arange(e, device=dev) % 2 == 0)
    got, got_n = vec.env_config(), vec.env_config(True)
    assert np.array_equal(got["num_drones"].cpu().numpy(), cur)
    assert np.array_equal(got_n["num_drones"].cpu().numpy(), nxt)
    assert np.array_equal(got["world_size"].cpu().numpy(), ws)
    assert np.array_equal(got_n["world_size"].cpu().numpy()[::2], (ws + 1.0)[::2])
    # device counts are clamped to [1, N]
    vec.set_env_config(num_drones=torch.tensor([0, -3, 9, 4, 100, 8], dtype=torch.int32, device=dev))
    assert vec.env_config()["num_drones"].cpu().tolist() == [1, 1, 8, 4, 8, 8]
    # the device moves next-episode counts into the current records by itself
    vec.set_env_config(num_drones=cur)
    vec.reset()
    assert np.array_equal(vec.env_config()["num_drones"].cpu().numpy(), nxt)
    vec.set_env_config(max_steps=5)
    assert np.array_equal(vec.env_config()["num_drones"].cpu().numpy(), nxt)


@pytest.mark.parametrize("n,e", [(8, 16400), (128, 2052)])
def test_staged_rows_of_missing_slots(dev, n, e):
    """Launches large enough to stage the observation rows through LDS (the whole block region
    is stored from it): rows of slots that do not exist are zeros, not stale LDS, and the batch
    equals a small one (rows stored from registers) env for env."""
    from swarm_marl_amd import VecSwarm
    small_e = 24
    cfg = {"num_drones": n, "max_steps": 3}
    pattern = np.array([1, 2, 3, 4, 5, n, n - 1, n // 2 + 1], np.int32)
    big = VecSwarm(e, cfg, device=dev, auto_reset=True, seed=17)
    small = VecSwarm(small_e, cfg, device=dev, auto_reset=True, seed=17)
    assert int(big.group_launch_info[0].staged_obs) == 1 and int(small.group_launch_info[0].staged_obs) == 0
    counts = np.resize(pattern, e)
    big.set_env_config(num_drones=counts)
    small.set_env_config(num_drones=counts[:small_e])
    ghost = torch.as_tensor(_ghost(counts, n), device=dev)
    for v in (big, small):
        v.obs.fill_(float("nan"))
        v.reset()
    assert torch.equal(big.obs[:small_e], small.obs) and not big.obs[ghost].any()
    for t in range(5):
        a = _actions(dev, t, e, n)
        for v in (big, small):
            v.obs.fill_(float("nan"))
        big.step(a)
        small.step(a[:small_e].contiguous())
        assert not torch.isnan(big.obs).any(), f"t={t}"
        assert not big.obs[ghost].any() and not big.pos[ghost].any() and not big.active[ghost].any(), f"t={t}"
        assert bool((big.obs[~ghost][:, :3] != 0).any())
        for x, y in zip(_snap(big), _snap(small)):
            assert torch.equal(x[:small_e], y), f"t={t}"
    assert int(((big.env_done & 4) != 0).sum()) > 0 or int(big.episode.max()) > 1


# ---------------------------------------------------------------- eval tracker
class _MergedRef:
    """Per-env DenseEvalRef instances (each with N = n_e) read as one reference."""

    def __init__(self, refs):
        self.refs = refs

    def _rows(self):
        rows = np.concatenate([r.records() for r in self.refs], axis=0)
        absr = np.concatenate([r.abs_rewards() for r in self.refs], axis=0)
        o = np.lexsort((rows[:, 0], rows[:, 8]))
        return rows[o], absr[o]

    def records(self):
        return self._rows()[0]

    def abs_rewards(self):
        return self._rows()[1]


def test_eval_tracker_on_mixed_batch(dev):
    """Unfused EvalTracker on a mixed batch against tests/eval_ref.py run per env with N = n_e:
    tests/test_gpu_eval_shapes.py's comparison (formation error and path efficiency 1e-9
    relative, the rest exact) — path efficiency is the mean over the env's n_e drones."""
    from swarm_marl_amd import VecSwarm
    from swarm_marl_amd.eval_metrics import EvalTracker
    from tests import eval_ref as er
    from tests.test_gpu_eval_shapes import compare
    n, e = 8, 12
    counts = np.resize(np.array([1, 2, 3, 4, 5, 8], np.int32), e)
    vec = VecSwarm(e, {"num_drones": n, "max_steps": 9, "goal_radius": 2.5, "num_obstacles": 4}, device=dev,
                   auto_reset=True, seed=19, with_infos=True)
    vec.set_env_config(num_drones=counts)
    vec.reset()
    ev = EvalTracker(vec)
    assert not ev.fused
    ev.begin()
    torch.cuda.synchronize()
    obs = vec.obs.cpu().numpy()
    refs = [er.DenseEvalRef(1, int(c), env_offset=i) for i, c in enumerate(counts)]
    for i, (r, c) in enumerate(zip(refs, counts)):
        r.begin(obs[i:i + 1, :c])
    rng = np.random.default_rng(3)
    for t in range(40):
        vec.step(torch.from_numpy(er.goal_actions(obs, rng)).to(dev))
        ev.update()
        torch.cuda.synchronize()
        obs = vec.obs.cpu().numpy()
        rew, fl, done = vec.reward.cpu().numpy(), vec.info_flags.cpu().numpy(), vec.env_done.cpu().numpy()
        for i, (r, c) in enumerate(zip(refs, counts)):
            r.update(obs[i:i + 1, :c], rew[i:i + 1, :c], fl[i:i + 1, :c], done[i:i + 1])
    got = ev.records()
    assert len(got) >= e
    for i, c in enumerate(counts):  # per env: the reward bound of a swarm of n_e drones
        compare(got[got[:, 0] == i], _MergedRef([refs[i]]), int(c), f"env {i} (n_e = {c})")
    compare(got, _MergedRef(refs), n, "mixed batch")
    pe = got[:, 5]
    assert (pe > 0).any()


# ---------------------------------------------------------------- rollouts and PPO
CURRICULUM_V1 = {"stages": [  # configs/curriculum_v1.yaml env_configs
    {"env_config": {"num_drones": 3, "num_obstacles": 0, "max_steps": 300, "world_size": 20.0}},
    {"env_config": {"num_drones": 3, "num_obstacles": 4, "max_steps": 350, "world_size": 20.0}},
    {"env_config": {"num_drones": 5, "num_obstacles": 8, "max_steps": 400, "world_size": 24.0}},
    {"env_config": {"num_drones": 8, "num_obstacles": 12, "max_steps": 450, "world_size": 28.0}}]}


def _arrays(shapes, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1, 1, s).astype(np.float32) / np.float32(np.sqrt(s[-1])) for s in shapes]


@pytest.mark.parametrize("critic_kind", ["agent", "ctde"])
def test_rollout_and_ppo_update_on_mixed_size_batch(dev, critic_kind):
    """RolloutCollector and PPOLearner take a mixed_size_batch of curriculum_v1's four stages with
    no new arguments: valid is never set on a slot that does not exist, advantage and value
    target are zero there, and the update counts exactly the valid rows."""
    from swarm_marl_amd import AgentValueMLP, CriticMLP, PPOLearner, RolloutCollector
    from swarm_marl_amd.curriculum import assign_stage, mixed_size_batch
    from swarm_marl_amd.policy import PolicyMLP
    from tests import critic_ref as cr
    from tests import value_ref as vr
    e, horizon = 16, 8
    stage_of_env = np.arange(e) % 4
    vec, over = mixed_size_batch(CURRICULUM_V1, stage_of_env, device=dev, seed=7, with_global_state=True)
    n = vec.num_drones
    assert n == 8 and int(vec.cfg.num_obstacles) == 12 and vec.obstacles.shape == (e, 12, 3)
    counts = over["num_drones"]
    assert np.array_equal(counts, np.array([3, 3, 5, 8])[stage_of_env])
    assert np.array_equal(vec.env_config()["num_drones"].cpu().numpy(), counts)
    ghost = torch.as_tensor(_ghost(counts, n), device=dev)
    assert torch.equal(vec.active, ~ghost) and not vec.obs[ghost].any()  # the batch comes back reset
    policy = PolicyMLP.from_arrays(*_arrays(((256, vec.obs_dim), (256,), (256, 256), (256,), (6, 256), (6,)), 5),
                                   device=dev, precision="bf16")
    if critic_kind == "agent":
        critic = AgentValueMLP(vr.make_value(vec.obs_dim, seed=2), device=dev, precision="f32")
    else:
        critic = CriticMLP(cr.make_critic(6 * n + 3, seed=2), device=dev, precision="f32")
    col = RolloutCollector(vec, policy, critic, horizon=horizon, seed=3)
    learner = PPOLearner(policy, critic, lr=3e-4, num_epochs=2, minibatch_env_rows=horizon * e)
    batch = col.collect()
    torch.cuda.synchronize()
    valid = batch["valid"]
    g = ghost[None].expand_as(valid)
    assert not valid[g].any() and valid[~g].any()
    assert not batch["advantage"][g].any() and not batch["value_target"][g].any()
    assert not batch["reward"][g].any() and not batch["obs"][g].any()
    for k in ("logits", "value", "advantage", "value_target", "logp"):
        assert bool(torch.isfinite(batch[k]).all()), k
    gs = batch["global_state"]
    pad = torch.cat([ghost.repeat_interleave(3, dim=1), ghost.repeat_interleave(3, dim=1),
                     torch.zeros((e, 3), dtype=torch.bool, device=dev)], dim=1)
    assert not gs[pad[None].expand_as(gs)].any()
    info = learner.update(batch)
    assert info["count"] == int(valid.sum())
    assert all(np.isfinite(v) for k, v in info.items() if k != "epoch_total_loss")
    assert np.isfinite(info["epoch_total_loss"]).all()
    # ---- assign_stage: per-env promotion at the env's next reset, and not before
    mask = torch.as_tensor(stage_of_env == 0, device=dev)
    before = vec.env_config()["num_drones"].clone()
    got = assign_stage(vec, CURRICULUM_V1, mask, 3)
    assert got["num_drones"] == 8 and got["num_obstacles"] == 12 and got["max_steps"] == 450
    assert torch.equal(vec.env_config()["num_drones"], before)
    want_next = torch.where(mask, torch.full_like(before, 8), before)
    assert torch.equal(vec.env_config(True)["num_drones"], want_next)
    moved = torch.zeros(e, dtype=torch.bool, device=dev)
    for t in range(4):
        vec.step(torch.zeros((e, n, 3), device=dev))
        moved |= (vec.env_done & 4) != 0
        now = vec.env_config()["num_drones"]
        assert torch.equal(now, torch.where(moved, want_next, before)), f"t={t}"
    some = mask & (torch.arange(e, device=dev) < 8)
    vec.reset(some)
    moved |= some
    now = vec.env_config()["num_drones"]
    assert torch.equal(now, torch.where(moved, want_next, before))
    assert bool((now[some] == 8).all()) and bool(vec.active[some].all())
    assert torch.equal(vec.env_config()["world_size"][some], torch.full((int(some.sum()),), 28.0, dtype=torch.float64,
                                                                       device=dev))
    batch = col.collect()  # the collector goes on over the promoted envs
    ghost2 = torch.arange(n, device=dev)[None, :] >= vec.env_config()["num_drones"][:, None]
    assert not vec.active[ghost2].any() and bool(torch.isfinite(batch["advantage"]).all())
    assert info["count"] > 0 and learner.update(batch)["count"] == int(batch["valid"].sum())
