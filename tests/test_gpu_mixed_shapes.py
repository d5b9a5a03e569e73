"""GPU: per-env drone counts at every lane mode of the generic swarm_kernel, every
K / Ms register width, and the edges tests/test_gpu_mixed.py leaves out.

Every case steps a mixed batch and compares it, env for env and row for row, with the reference
that steps each env on its own with num_drones = n_e (tests/mixed_ref.py, pinned on the CPU by
tests/test_mixed_cpu.py), through test_gpu_mixed's own comparisons: obs, flags, env_done, state,
dist_goal and global_state bit-exact, rewards within 1e-5, every output of a slot
that does not exist exactly zero.  Eval records go through test_gpu_eval_shapes.compare.

1  lane modes: several teams per wave with N < L (5, 24), four / two teams per wave (16, 32 lanes),
   one team per wave without packed bytes (33), block teams without (100) and with the pair ring
   (128, 256: whole waves of slots that do not exist); physics at 16, 64 (packed-byte ballots of
   padding lanes) and 128; a nonzero env_offset (Philox blocks n_e + m, n_e + M_e)
2  K / Ms widths KS in {0, 4, 9, 17} x MSL in {0, 5, 9, 17} with n_e - 1 below, at and above K
3  next-episode counts growing and shrinking at N = 64, 128, 100 and 16 physics
4  action masks, real-but-inactive drones beside missing slots, auto_reset = False to n_active == 0
5  swarm_observe on a mixed batch: direct, staged, pair-ring aux pass, env masks
6  integer lattices with only the first n_e slots placed: exact distance ties (the exact top-K
   fallback), and pairs exactly on the collision threshold (the exact pair-collision fallback)
7  the unfused EvalTracker at N = 64 (rotation branch) and N = 128 (generic branch)

Every case prints the kernel instantiation that ran and the largest reward error it saw.

Measured on an MI355X (38 cases, 4 s): largest reward error 1.8e-6 (N = 128 physics) against the
1e-5 bound, everything else bit-exact; eval records 2.2e-16 relative on path efficiency.  Kernel
mutations and which case each fails: DESIGN.md §3.5.  Passing N for n_e to exact_select /
exact_pair_collision fails nothing because it computes the same function (the extra entries are
padding: eligibility 0, position 1e18, beyond any cut); breaking the tie order of exact_select fails
every lattice case, silencing exact_pair_collision the two on-threshold ones.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import mixed_ref as mr
from tests.helpers import oracle_cfg, vec_state_numpy
from tests.test_gpu_mixed import _MergedRef, _actions, _compare, _compare_state, _ghost, _overrides, _snap

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _make(dev, e, raw, **kw):
    from swarm_marl_amd import VecSwarm
    return VecSwarm(e, raw, device=dev, with_infos=True, with_global_state=True, **kw)


def _generic(vec) -> str:
    name = vec.kernel_name()
    assert name.startswith("swarm_kernel<"), name
    return name


def _reward_err(vec, out) -> float:
    return float(np.abs(vec.reward.cpu().numpy().astype(np.float64) - out["reward"]).max())


def _report(tag, vec, err, extra=""):
    print(f"\n[mixed-shapes] {tag}: {vec.kernel_name()} reward max|err| {err:.3e} {extra}")


def _rollout(dev, tag, raw, dyn, counts, steps, *, seed=23, env_offset=0, ov=None):
    """reset + `steps` auto-resetting steps of a mixed batch against mr.reset / mr.step."""
    physics = dyn == "physics"
    n, e = int(raw["num_drones"]), len(counts)
    base = oracle_cfg(raw)
    ov = ov or {}
    vec = _make(dev, e, raw, auto_reset=True, seed=seed, dynamics=dyn, env_offset=env_offset)
    vec.set_env_config(num_drones=counts, **ov)
    _generic(vec)
    assert np.array_equal(vec.env_config()["num_drones"].cpu().numpy(), counts)
    st0 = vec_state_numpy(vec)
    vec.reset()
    torch.cuda.synchronize()
    ns, ro, _ = mr.reset(base, ov, counts, st0, seed=seed, env_offset=env_offset, physics=physics)
    assert np.array_equal(vec.obs.cpu().numpy(), ro["obs"]), f"{tag}: reset obs"
    assert np.array_equal(vec.dist_goal.cpu().numpy(), ro["dist_goal"]), f"{tag}: reset dist_goal"
    assert np.array_equal(vec.global_state.cpu().numpy(), ro["global_state"]), f"{tag}: reset global_state"
    _compare_state(vec, ns, f"{tag}: reset", physics)
    resets, err = 0, 0.0
    for t in range(steps):
        a = _actions(dev, t, e, n)
        st = vec_state_numpy(vec)
        vec.step(a)
        torch.cuda.synchronize()
        ns, out, _, _ = mr.step(base, ov, counts, st, a.cpu().numpy(), seed=seed, env_offset=env_offset,
                                physics=physics)
        err = max(err, _reward_err(vec, out))
        _compare(vec, ns, out, counts, counts, f"{tag} t={t}", physics)
        resets += int(out["reset"].sum())
    assert resets > 0, f"{tag}: the run must cross episode boundaries"
    _report(tag, vec, err, f"resets {resets}")
    return vec


# ---------------------------------------------------------------- 1. lane modes
LANE_CASES = [
    pytest.param(5, "kinematic", [1, 2, 4, 5, 3], 11, 0, id="N5-partial-last-block"),
    pytest.param(16, "kinematic", [16, 1, 9, 4, 15, 2] + [16] * 8, 14, 0, id="N16-four-teams"),
    pytest.param(24, "kinematic", [24, 23, 12, 2], 4, 0, id="N24-two-teams"),
    pytest.param(24, "kinematic", [24, 23, 12, 2], 4, 5, id="N24-env-offset"),
    pytest.param(33, "kinematic", [33, 32, 17, 1], 4, 0, id="N33-one-team-unpacked"),
    pytest.param(100, "kinematic", [100, 99, 65, 64, 63, 1], 6, 0, id="N100-block"),
    pytest.param(256, "kinematic", [256, 255, 193, 128, 65, 3], 6, 0, id="N256-pair-ring"),
    pytest.param(16, "physics", [16, 5, 1, 9], 4, 0, id="N16-physics"),
    pytest.param(64, "physics", [64, 63, 33, 2], 4, 0, id="N64-physics-ballots"),
    pytest.param(128, "physics", [128, 65, 64, 2], 4, 0, id="N128-physics"),
]


@pytest.mark.parametrize("n,dyn,pattern,e,env_offset", LANE_CASES)
def test_lane_modes_vs_reference(dev, n, dyn, pattern, e, env_offset):
    """K = 3, Ms = 4, default radii; max_steps = 6 so that every env resets within the run."""
    counts = np.resize(np.array(pattern, np.int32), e)
    raw = {"num_drones": n, "num_obstacles": 6, "max_steps": 6}
    vec = _rollout(dev, f"lane N={n} {dyn} off={env_offset}", raw, dyn, counts, 8, env_offset=env_offset)
    assert int(vec.episode.min()) > 1, "every env ended an episode (physics: terminated on its drones only)"


# ---------------------------------------------------------------- 2. K / Ms widths
def _k_counts(n, k, extra=()):
    """Counts with n_e - 1 = K - 1, K and K + 1 where they fit, a single drone, and all n slots."""
    return np.array(sorted({c for c in (1, k, k + 1, k + 2, n, *extra) if 1 <= c <= n}, reverse=True), np.int32)


WIDTH_CASES = [
    pytest.param(24, 0, 4, 8, None, False, id="N24-K0-Ms4"),
    pytest.param(24, 1, 2, 8, None, False, id="N24-K1-Ms2"),
    pytest.param(24, 8, 8, 8, None, True, id="N24-K8-Ms8-overrides"),
    pytest.param(24, 12, 16, 20, None, False, id="N24-K12-Ms16"),
    pytest.param(24, 16, 0, 5, None, False, id="N24-K16-Ms0"),
    pytest.param(24, 3, 4, 0, None, False, id="N24-K3-M0"),
    pytest.param(64, 16, 16, 20, [64, 17, 16, 40], False, id="N64-K16-Ms16"),
    pytest.param(128, 8, 8, 8, [128, 13, 12, 70], False, id="N128-K8-Ms8"),
    pytest.param(128, 12, 16, 20, [128, 13, 12, 70], False, id="N128-K12-Ms16"),
]


@pytest.mark.parametrize("n,k,ms,m,pattern,with_ov", WIDTH_CASES)
def test_k_ms_widths_vs_reference(dev, n, k, ms, m, pattern, with_ov):
    """Every neighbour / obstacle register width with counts around K: a row with n_e - 1 < K keeps
    its spare neighbour slots zero, one with M_e < Ms its spare obstacle slots (with_ov: per-env
    num_obstacles 0, 1, 3, M, M - 1, 2 beside counts 1, K, K + 1, K + 2, 13, 24: both in one row)."""
    counts = _k_counts(n, k, extra=(13,)) if pattern is None else np.array(pattern, np.int32)
    if with_ov:
        counts = np.resize(counts[::-1].copy(), 6)
    e = len(counts)
    raw = dict(num_drones=n, neighbor_k=k, sensed_obstacles=ms, num_obstacles=m, max_steps=5)
    ov = _overrides(e, m, np.random.default_rng(n + k)) if with_ov else None
    if pattern is None:
        want = {c - 1 for c in counts}
        assert {max(k - 1, 0), k, k + 1} <= want and n in counts and 1 in counts
    vec = _rollout(dev, f"width N={n} K={k} Ms={ms} M={m}", raw, "kinematic", counts, 7, seed=3, ov=ov)
    li = vec.group_launch_info[0]
    print(f"    neighbor_slots {int(li.neighbor_slots)} obstacle_slots {int(li.obstacle_slots)} counts {counts.tolist()}")


# ---------------------------------------------------------------- 3. next-episode counts
NEXT_CASES = [
    # cur, next 1, next 2: env 0 / 2 switch at the explicit reset, env 1 / 3 at their auto-resets
    pytest.param(64, "kinematic", [64, 20, 20, 64], [20, 64, 64, 20], [64, 7, 7, 64], id="N64"),
    pytest.param(128, "kinematic", [128, 3, 3, 128], [40, 128, 128, 40], [128, 65, 65, 128], id="N128"),
    pytest.param(100, "kinematic", [100, 37, 37, 100], [37, 100, 100, 37], [100, 65, 1, 99], id="N100"),
    pytest.param(16, "physics", [16, 5, 5, 16], [5, 16, 16, 5], [9, 1, 16, 3], id="N16-physics"),
]


@pytest.mark.parametrize("n,dyn,cur,nxt1,nxt2", NEXT_CASES)
def test_next_episode_counts_at_other_shapes(dev, n, dyn, cur, nxt1, nxt2):
    """test_gpu_mixed.test_next_episode_counts off N = 8: a shrink or a grow flips the wave's
    all-eligible path and the ballot-packed stores (N = 64), `Ne == N` of the pair ring (N = 128),
    the loop bound of the masked block pass (N = 100)."""
    physics = dyn == "physics"
    e, seed = len(cur), 31
    cur, nxt1, nxt2 = (np.array(c, np.int32) for c in (cur, nxt1, nxt2))
    raw = {"num_drones": n, "num_obstacles": 6, "max_steps": 4}
    base = oracle_cfg(raw)
    vec = _make(dev, e, raw, auto_reset=True, seed=seed, dynamics=dyn)
    vec.set_env_config(num_drones=cur)
    _generic(vec)
    st0 = vec_state_numpy(vec)
    vec.reset()
    torch.cuda.synchronize()
    ns, _, cnt = mr.reset(base, {}, cur, st0, seed=seed, physics=physics)
    _compare_state(vec, ns, "first reset", physics)
    vec.set_env_config(next_episode=True, num_drones=nxt1)
    assert np.array_equal(vec.env_config()["num_drones"].cpu().numpy(), cur)
    assert np.array_equal(vec.env_config(True)["num_drones"].cpu().numpy(), nxt1)
    mask = torch.zeros(e, dtype=torch.bool, device=dev)
    mask[::2] = True
    sel = mask.cpu().numpy()
    st = vec_state_numpy(vec)
    vec.reset(mask)
    torch.cuda.synchronize()
    ns, ro, cnt = mr.reset(base, {}, cnt, st, counts_next=nxt1, env_mask=sel, seed=seed, physics=physics)
    _compare_state(vec, ns, "masked reset", physics)
    for k in ("obs", "dist_goal", "global_state"):
        assert np.array_equal(getattr(vec, k).cpu().numpy()[sel], ro[k][sel]), f"masked reset {k}"
    assert not vec.obs.cpu().numpy()[_ghost(cnt, n)].any()
    assert np.array_equal(vec.env_config()["num_drones"].cpu().numpy(), cnt)
    assert np.array_equal(cnt, np.where(sel, nxt1, cur))
    seen = [{int(c)} for c in cur]
    for i, c in enumerate(cnt):
        seen[i].add(int(c))
    counts_next, resets, err = nxt1, 0, 0.0
    for t in range(12):
        if t == 5:  # every env has reset at least once (max_steps = 4): queue the second move
            vec.set_env_config(next_episode=True, num_drones=nxt2)
            counts_next = nxt2
        a = _actions(dev, t, e, n)
        st = vec_state_numpy(vec)
        vec.step(a)
        torch.cuda.synchronize()
        ns, out, _, cnt_new = mr.step(base, {}, cnt, st, a.cpu().numpy(), counts_next=counts_next, seed=seed,
                                      physics=physics)
        err = max(err, _reward_err(vec, out))
        _compare(vec, ns, out, cnt, cnt_new, f"next-episode N={n} t={t}", physics)
        assert np.array_equal(vec.env_config()["num_drones"].cpu().numpy(), cnt_new), f"t={t}"
        resets += int(out["reset"].sum())
        cnt = cnt_new
        for i, c in enumerate(cnt):
            seen[i].add(int(c))
    assert resets >= 2 * e
    assert np.array_equal(cnt, nxt2)
    for i in range(e):  # every listed count of every env was stepped
        assert seen[i] == {int(cur[i]), int(nxt1[i]), int(nxt2[i])}, (i, seen[i])
    _report(f"next-episode N={n} {dyn}", vec, err, f"resets {resets}")


# ---------------------------------------------------------------- 4. masks, inactive drones, no auto-reset
def _check_neighbours(obs, pos, counts, inactive, k):
    """Every neighbour feature of a real row is p_j - p_i of a real drone j != i of the same env
    (a slot that does not exist never is one), slots past min(K, n_e - 1) are zero; returns how
    many features name a drone of `inactive`."""
    named = 0
    for e, c in enumerate(counts):
        kk = min(k, int(c) - 1)
        for i in range(int(c)):
            nb = obs[e, i, 9:9 + 4 * k].reshape(k, 4)
            assert not nb[kk:].any(), f"env {e} row {i}: spare neighbour slots"
            rel = pos[e, :c] - pos[e, i]
            for s in range(kk):
                js = np.nonzero((rel == nb[s, :3]).all(axis=1))[0]
                js = js[js != i]
                assert len(js) > 0, f"env {e} row {i} slot {s}: no real drone at {nb[s]}"
                named += int(inactive[e, js].any())
    return named


MASK_CASES = [
    pytest.param(8, "kinematic", [1, 2, 3, 4, 5, 6, 7, 8], id="N8"),
    pytest.param(64, "kinematic", [64, 33, 5, 1], id="N64"),
    pytest.param(8, "physics", [1, 2, 3, 4, 5, 6, 7, 8], id="N8-physics"),
]


@pytest.mark.parametrize("n,dyn,counts", MASK_CASES)
def test_masks_inactive_drones_and_no_auto_reset(dev, n, dyn, counts):
    """auto_reset = False: a quarter of the real drones start inactive (they stay neighbours, unlike
    the slots that do not exist), 15 % of the actions are absent, and the run goes on until every
    env has reported term_all from n_active == 0 (drone_swarm_env.py:93-95)."""
    physics = dyn == "physics"
    counts = np.array(counts, np.int32)
    e, seed, k = len(counts), 41, 3
    raw = {"num_drones": n, "num_obstacles": 6, "max_steps": 5}
    base = oracle_cfg(raw)
    vec = _make(dev, e, raw, auto_reset=False, seed=seed, dynamics=dyn)
    vec.set_env_config(num_drones=counts)
    _generic(vec)
    vec.reset()
    torch.cuda.synchronize()
    st = vec_state_numpy(vec)
    rng = np.random.default_rng(n + e)
    real = ~_ghost(counts, n)
    inactive = real & (rng.uniform(size=(e, n)) < 0.25)
    inactive[:, 0] = False
    for i, c in enumerate(counts):  # the last real drone: inactive, beside the first slot that does not exist
        inactive[i, c - 1] = c > 1
    vel = np.where(real[..., None], rng.uniform(-1, 1, (e, n, 3)), 0.0).astype(np.float32)
    vec.set_state(pos=st["pos"], vel=vel, active=real & ~inactive)
    st = vec_state_numpy(vec)
    assert not st["pos"][~real].any() and not st["active"][~real].any() and inactive.sum() >= 2
    zero_seen = np.zeros(e, bool)
    named, absent, err = 0, 0, 0.0
    for t in range(9):
        a = _actions(dev, t, e, n)
        am = torch.rand((e, n), device=dev, generator=torch.Generator(device=dev).manual_seed(900 + t)) > 0.15
        absent += int((~am.cpu().numpy() & real).sum())
        before_zero = st["active"].sum(axis=1) == 0
        vec.step(a, am)
        torch.cuda.synchronize()
        ns, out, _, _ = mr.step(base, {}, counts, st, a.cpu().numpy(), auto_reset=False, seed=seed, physics=physics,
                                action_mask=am.cpu().numpy())
        err = max(err, _reward_err(vec, out))
        _compare(vec, ns, out, counts, counts, f"masks N={n} {dyn} t={t}", physics)
        assert not out["reset"].any()
        got_term = (vec.env_done.cpu().numpy() & 1) != 0
        assert got_term[before_zero].all()
        zero_seen |= before_zero & got_term
        named += _check_neighbours(vec.obs.cpu().numpy(), vec.pos.cpu().numpy(), counts, inactive, k)
        st = vec_state_numpy(vec)
    assert zero_seen.all(), f"envs that never stepped with n_active == 0: {np.nonzero(~zero_seen)[0]}"
    assert absent > 0 and named > 0, "an inactive real drone must appear as a neighbour"
    _report(f"masks N={n} {dyn}", vec, err, f"absent actions {absent}, neighbour features naming an inactive drone {named}")


# ---------------------------------------------------------------- 5. swarm_observe
def _poison(vec):
    for t in (vec.obs, vec.dist_goal, vec.global_state):
        t.fill_(float("nan"))


def _observe_and_compare(vec, base, counts, physics, mask, tag):
    n = vec.num_drones
    state = [t.clone() for t in vec.state_dict().values()]
    st = vec_state_numpy(vec)
    _poison(vec)
    vec.observe(mask)
    torch.cuda.synchronize()
    sel = np.ones(len(counts), bool) if mask is None else mask.cpu().numpy().astype(bool)
    ref = mr.observe(base, {}, counts, st, env_mask=sel, physics=physics)
    for k in ("obs", "dist_goal", "global_state"):
        got = getattr(vec, k).cpu().numpy()
        assert np.array_equal(got, ref[k], equal_nan=True), \
            f"{tag}: {k} differs at {np.argwhere(~((got == ref[k]) | (np.isnan(got) & np.isnan(ref[k]))))[:4]}"
        assert np.isnan(got[~sel]).all() and not np.isnan(got[sel]).any(), f"{tag}: {k} rows of the mask"
    ghost = _ghost(counts, n) & sel[:, None]
    assert not vec.obs.cpu().numpy()[ghost].any() and not vec.dist_goal.cpu().numpy()[ghost].any(), tag
    gs = vec.global_state.cpu().numpy()
    assert not gs[:, :3 * n].reshape(-1, n, 3)[ghost].any() and not gs[:, 3 * n:6 * n].reshape(-1, n, 3)[ghost].any(), tag
    for name, x, y in zip(vec.state_dict(), vec.state_dict().values(), state):
        assert torch.equal(x, y), f"{tag}: observe changed state {name}"


OBSERVE_CASES = [
    pytest.param(8, "kinematic", [1, 2, 3, 4, 5, 8, 7, 6], id="N8-direct"),
    pytest.param(64, "kinematic", [64, 33, 5, 1], id="N64-staged"),
    pytest.param(128, "kinematic", [128, 100, 3, 65], id="N128-pair-ring"),
    pytest.param(8, "physics", [1, 2, 3, 4, 5, 8, 7, 6], id="N8-physics"),
]


@pytest.mark.parametrize("n,dyn,counts", OBSERVE_CASES)
def test_observe_on_mixed_batch(dev, n, dyn, counts):
    """swarm_observe after a few steps (some real drones have ended): the reference's rows, zeros
    for the slots that do not exist, the state bitwise untouched, unselected envs left alone."""
    physics = dyn == "physics"
    counts = np.array(counts, np.int32)
    e = len(counts)
    raw = {"num_drones": n, "num_obstacles": 6, "max_steps": 50, "goal_radius": 6.0}
    base = oracle_cfg(raw)
    vec = _make(dev, e, raw, auto_reset=True, seed=29, dynamics=dyn)
    vec.set_env_config(num_drones=counts)
    _generic(vec)
    vec.reset()
    for t in range(3):
        vec.step(_actions(dev, t, e, n))
    torch.cuda.synchronize()
    act = vec.active.cpu().numpy()
    assert act.any() and not act[_ghost(counts, n)].any()
    _observe_and_compare(vec, base, counts, physics, None, f"observe N={n} {dyn}")
    mask = torch.zeros(e, dtype=torch.bool, device=dev)
    mask[1::2] = True
    _observe_and_compare(vec, base, counts, physics, mask, f"observe N={n} {dyn} masked")
    mask = ~mask
    _observe_and_compare(vec, base, counts, physics, mask.to(torch.uint8), f"observe N={n} {dyn} masked (u8)")
    print(f"\n[mixed-shapes] observe N={n} {dyn}: step {vec.kernel_name()}, inactive real drones "
          f"{int((~act & ~_ghost(counts, n)).sum())}")


def test_observe_staged_rows_of_missing_slots(dev):
    """The staged launch shape of test_gpu_mixed.test_staged_rows_of_missing_slots (N = 8,
    E = 16400) against its 24-env twin, on the device: observe() writes zeros, not stale LDS, for
    the slots that do not exist, equals the small batch env for env, and honours an env mask."""
    n, e, small_e = 8, 16400, 24
    cfg = {"num_drones": n, "max_steps": 50}
    pattern = np.array([1, 2, 3, 4, 5, n, n - 1, n // 2 + 1], np.int32)
    big = _make(dev, e, cfg, auto_reset=True, seed=17)
    small = _make(dev, small_e, cfg, auto_reset=True, seed=17)
    assert int(big.group_launch_info[0].staged_obs) == 1 and int(small.group_launch_info[0].staged_obs) == 0
    counts = np.resize(pattern, e)
    big.set_env_config(num_drones=counts)
    small.set_env_config(num_drones=counts[:small_e])
    ghost = torch.as_tensor(_ghost(counts, n), device=dev)
    for v in (big, small):
        v.reset()
    for t in range(2):
        a = _actions(dev, t, e, n)
        big.step(a)
        small.step(a[:small_e].contiguous())
    for x, y in zip(_snap(big), _snap(small)):
        assert torch.equal(x[:small_e], y)
    state = [t.clone() for t in big.state_dict().values()]
    for v in (big, small):
        _poison(v)
        v.observe()
    for k in ("obs", "dist_goal", "global_state"):
        x, y = getattr(big, k), getattr(small, k)
        assert not torch.isnan(x).any(), k
        assert torch.equal(x[:small_e], y), k
    assert not big.obs[ghost].any() and not big.dist_goal[ghost].any()
    gs = big.global_state
    assert not gs[:, :3 * n].reshape(e, n, 3)[ghost].any() and not gs[:, 3 * n:6 * n].reshape(e, n, 3)[ghost].any()
    assert bool((big.obs[~ghost][:, :3] != 0).any())
    assert torch.equal(big.obs[:, :, :3], big.pos) and torch.equal(gs[:, 6 * n:], big.goal)
    for x, y in zip(big.state_dict().values(), state):
        assert torch.equal(x, y)
    full = [getattr(big, k).clone() for k in ("obs", "dist_goal", "global_state")]
    mask = torch.arange(e, device=dev) % 3 == 0
    _poison(big)
    big.observe(mask)
    for k, ref in zip(("obs", "dist_goal", "global_state"), full):
        x = getattr(big, k)
        assert torch.equal(x[mask], ref[mask]), k
        assert bool(torch.isnan(x[~mask]).all()), k


# ---------------------------------------------------------------- 6. tie-heavy lattice
LATTICE_CASES = [
    pytest.param(64, 3, 4, 8, [64, 27, 9, 5], 0.1, id="N64-K3"),
    pytest.param(16, 8, 6, 8, [16, 9, 8, 3], 0.1, id="N16-K8"),
    pytest.param(128, 5, 4, 12, [128, 100, 27], 0.1, id="N128-K5"),
    # 2 collision_radius = env 1's lattice spacing: its adjacent pairs sit exactly on the threshold
    pytest.param(64, 3, 4, 8, [64, 27, 9, 5], 0.25, id="N64-K3-pairs-on-threshold"),
    pytest.param(128, 5, 4, 12, [128, 100, 27], 0.25, id="N128-K5-pairs-on-threshold"),
]


@pytest.mark.parametrize("n,k,ms,m,counts,radius", LATTICE_CASES)
def test_tie_heavy_lattice_mixed_counts(dev, n, k, ms, m, counts, radius):
    """test_gpu_parity.test_tie_heavy_lattice with only the first n_e slots placed (the rest zero
    and inactive): exact distance ties everywhere, so the finish falls to exact_select and the
    (distance, index) order with count = n_e.  Env 1 (spacing 0.5) has every third real drone
    inactive.  With collision_radius 0.25 its adjacent pairs are at distance 0.5 = the pair
    threshold exactly: inside the band of the running minimum, so exact_pair_collision decides
    (d <= threshold collides; an inactive neighbour at the same distance does not count)."""
    counts = np.array(counts, np.int32)
    e = len(counts)
    raw = dict(num_drones=n, neighbor_k=k, sensed_obstacles=ms, num_obstacles=m, max_steps=50,
               collision_radius=radius)
    if radius == 0.25:
        raw["obstacle_radius"] = 0.0
    base = oracle_cfg(raw)
    spacings = [1.0, 0.5, 2.0, 1.5][:e]
    side = int(np.ceil(n ** (1.0 / 3.0) - 1e-9))
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
    real = ~_ghost(counts, n)
    pos = np.stack([(grid - (side - 1) / 2.0) * sp for sp in spacings]).astype(np.float32)
    pos[~real] = 0.0
    ogrid = np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), -1).reshape(-1, 3)[:m]
    obst = np.stack([(ogrid - 1.0) * sp * 2.0 + 0.5 * sp for sp in spacings]).astype(np.float32)
    goal = np.tile(np.array([7.25, -6.5, 3.75], np.float32), (e, 1))
    active = real.copy()
    active[1, ::3] = False
    st = dict(pos=pos, vel=np.zeros_like(pos), goal=goal, obst=obst, active=active, step=np.zeros(e, np.int32),
              episode=np.zeros(e, np.uint32), damping=np.zeros((e, n), np.float32))
    vec = _make(dev, e, raw, auto_reset=False, seed=2)
    vec.set_env_config(num_drones=counts)
    _generic(vec)
    vec.set_state(pos=pos, vel=st["vel"], goal=goal, obstacles=obst, active=active, step_count=st["step"])
    err = 0.0
    for t in range(2):
        a = np.zeros((e, n, 3), np.float32)
        vec.step(torch.as_tensor(a).to(dev))
        torch.cuda.synchronize()
        st, out, _, _ = mr.step(base, {}, counts, st, a, auto_reset=False, seed=2)
        err = max(err, _reward_err(vec, out))
        _compare(vec, st, out, counts, counts, f"lattice N={n} K={k} t={t}")
        # ties: the neighbour distances of a row repeat (the order below is by index alone)
        d = out["obs"][0, 0, 9:9 + 4 * k].reshape(k, 4)[:, 3]
        assert len(np.unique(d)) < k
        if radius == 0.25 and t == 0:  # env 1: its active drones collide at d == threshold
            assert out["collision"][1].sum() > counts[1] // 2 and not out["collision"][2:].all()
    _report(f"lattice N={n} K={k} Ms={ms}", vec, err)


# ---------------------------------------------------------------- 7. eval tracker
@pytest.mark.parametrize("n,counts", [(64, [64, 40, 2, 1]), (128, [128, 65, 3])])
def test_eval_tracker_on_mixed_batch_large(dev, n, counts):
    """test_gpu_mixed.test_eval_tracker_on_mixed_batch past eval_update_kernel's N <= 32 branch: the
    N == 64 rotations and the generic formation pass, with SWARM_EVAL_SLOT_COUNTS.  The tracker
    begins at episode starts (a mid-episode begin is not supported with slot counts)."""
    from swarm_marl_amd.eval_metrics import EvalTracker
    from tests import eval_ref as er
    from tests.test_gpu_eval_shapes import compare
    counts = np.array(counts, np.int32)
    e = len(counts)
    cfg = dict(er.POINTS["full"], num_drones=n, max_steps=6, goal_radius=2.5)
    vec = _make(dev, e, cfg, auto_reset=True, seed=19)
    vec.set_env_config(num_drones=counts)
    _generic(vec)
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
    ghost = _ghost(counts, n)
    for t in range(20):
        vec.step(torch.from_numpy(er.goal_actions(obs, rng)).to(dev))
        ev.update()
        torch.cuda.synchronize()
        obs = vec.obs.cpu().numpy()
        rew, fl, done = vec.reward.cpu().numpy(), vec.info_flags.cpu().numpy(), vec.env_done.cpu().numpy()
        assert not obs[ghost].any() and not rew[ghost].any() and not fl[ghost].any()
        for i, (r, c) in enumerate(zip(refs, counts)):
            r.update(obs[i:i + 1, :c], rew[i:i + 1, :c], fl[i:i + 1, :c], done[i:i + 1])
    got = ev.records()
    mx = dict(fe=0.0, pe=0.0, reward=0.0)
    for i, c in enumerate(counts):
        mine = got[got[:, 0] == i]
        assert len(mine) >= 3, f"env {i}: {len(mine)} closed episodes"
        m1 = compare(mine, _MergedRef([refs[i]]), int(c), f"env {i} (n_e = {c})")
        mx = {k: max(mx[k], m1[k]) for k in mx}
        assert (mine[:, 5] > 0).any(), f"env {i}: no closed episode with path efficiency > 0"
    compare(got, _MergedRef(refs), n, "mixed batch")
    print(f"\n[mixed-shapes] eval N={n}: step {vec.kernel_name()}, {len(got)} records, max rel err FE {mx['fe']:.2e} "
          f"PE {mx['pe']:.2e}, reward err / bound {mx['reward']:.2e}")

