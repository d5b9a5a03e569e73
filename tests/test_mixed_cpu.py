"""CPU: per-env drone counts — the test-side reference (tests/mixed_ref.py), the C-ABI of
swarm_env_cfg_set_drones and the curriculum's mixed_size_batch validation (no GPU).

The reference for a mixed batch steps every env on its own with num_drones = n_e.  With every
n_e = N it must reduce to oracle/env_cfg_oracle.py exactly (the same computation), and with
differing counts each env must equal a batch of one env built with its count, scattered into N
slots with zeros elsewhere.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import mixed_ref as mr

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def nat():
    from swarm_marl_amd import _native
    return _native


@pytest.fixture(scope="module")
def lib(nat):
    return nat.load_library()


def _params(nat, lib, **kw):
    p = nat.SwarmParams()
    lib.swarm_params_default(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("physics", [False, True])
def test_uniform_counts_equal_env_cfg_oracle(physics):
    from oracle import env_cfg_oracle as eco
    from oracle import swarm_oracle as so
    n, e, m = 5, 6, 6
    base = so.make_cfg(num_drones=n, num_obstacles=m, max_steps=5)
    over = dict(world_size=np.linspace(14.0, 26.0, e), max_steps=np.array([4, 7, 5, 3, 6, 5], np.int32),
                num_obstacles=np.array([0, 6, 2, 5, 1, 3], np.int32))
    nxt = dict(world_size=np.linspace(26.0, 14.0, e), num_obstacles=np.array([6, 0, 3, 1, 5, 2], np.int32))
    st_a, ro_a = eco.reset(base, over, so.empty_state(base, e), seed=9, physics=physics)
    st_b, ro_b, cnt = mr.reset(base, over, None, so.empty_state(base, e), seed=9, physics=physics)
    assert np.array_equal(cnt, np.full(e, n))
    for k in ro_a:
        assert np.array_equal(ro_a[k], ro_b[k]), k
    rng = np.random.default_rng(0)
    cur_a, cur_b = over, over
    resets = 0
    for t in range(10):
        a = rng.uniform(-2, 2, (e, n, 3)).astype(np.float32)
        st_a, out_a, cur_a = eco.step(base, cur_a, st_a, a, nxt=nxt, seed=9, physics=physics)
        st_b, out_b, cur_b, cnt = mr.step(base, cur_b, np.full(e, n), st_b, a, nxt=nxt, seed=9, physics=physics)
        assert set(out_a) == set(out_b)
        for k in out_a:
            assert np.array_equal(out_a[k], out_b[k]), (t, k)
        for k in st_a:
            assert np.array_equal(st_a[k], st_b[k]), (t, k)
        for k in cur_a:
            assert np.array_equal(cur_a[k], cur_b[k]), (t, k)
        resets += int(out_a["reset"].sum())
    assert resets > 0
    # a masked reset: rows outside the mask are zero in both
    mask = np.arange(e) % 2 == 0
    st_a, ro_a = eco.reset(base, cur_a, st_a, nxt=nxt, env_mask=mask, seed=9, physics=physics)
    st_b, ro_b, _ = mr.reset(base, cur_b, None, st_b, nxt=nxt, env_mask=mask, seed=9, physics=physics)
    for k in ro_a:
        assert np.array_equal(ro_a[k], ro_b[k]), k
    for k in st_a:
        assert np.array_equal(st_a[k], st_b[k]), k


def test_mixed_counts_equal_single_env_batches():
    """Env e with count n_e == env env_offset + e of a batch built with num_drones = n_e, its rows
    scattered into N slots; a next-episode count takes over at the reset (3 -> 5, 5 -> 2)."""
    from oracle import swarm_oracle as so
    n, m = 5, 4
    base = so.make_cfg(num_drones=n, num_obstacles=m, max_steps=4)
    counts = np.array([3, 5, 1])
    counts_next = np.array([5, 2, 1])
    e = len(counts)
    st, ro, cnt = mr.reset(base, {}, counts, so.empty_state(base, e), seed=4, env_offset=10)
    singles = []
    for i, c in enumerate(counts):
        cfg = dict(base, num_drones=int(c))
        s1, r1 = so.reset_device(cfg, so.empty_state(cfg, 1), seed=4, env_offset=10 + i)
        singles.append((cfg, s1))
        assert np.array_equal(st["pos"][i, :c], s1["pos"][0]) and not st["pos"][i, c:].any()
        assert np.array_equal(st["goal"][i], s1["goal"][0]) and np.array_equal(st["obst"][i], s1["obst"][0])
        assert st["active"][i, :c].all() and not st["active"][i, c:].any()
        assert np.array_equal(ro["obs"][i, :c], r1["obs"][0]) and not ro["obs"][i, c:].any()
        gs = ro["global_state"][i]
        assert np.array_equal(gs[:3 * c], s1["pos"][0].ravel()) and not gs[3 * c:3 * n].any()
        assert not gs[3 * n:6 * n].any() and np.array_equal(gs[6 * n:], s1["goal"][0])
    rng = np.random.default_rng(2)
    switched = np.zeros(e, bool)
    for t in range(10):
        a = rng.uniform(-2, 2, (e, n, 3)).astype(np.float32)
        st, out, _, cnt_new = mr.step(base, {}, cnt, st, a, counts_next=counts_next, seed=4, env_offset=10)
        for i in range(e):
            cfg, s1 = singles[i]
            c = int(cnt[i])
            s1, o1 = so.step(cfg, s1, a[i:i + 1, :c], auto_reset=False, seed=4, env_offset=10 + i)
            assert np.array_equal(out["reward"][i, :c], o1["reward"][0]) and not out["reward"][i, c:].any()
            assert np.array_equal(out["terminated"][i, :c], o1["terminated"][0])
            if out["reset"][i]:
                c2 = int(counts_next[i])
                assert cnt_new[i] == c2
                switched[i] = True
                cfg = dict(base, num_drones=c2)
                s2 = so.empty_state(cfg, 1)
                s2["episode"], s2["step"] = s1["episode"], s1["step"]
                s1, r1 = so.reset_device(cfg, s2, seed=4, env_offset=10 + i)
                assert np.array_equal(out["obs"][i, :c2], r1["obs"][0]) and not out["obs"][i, c2:].any()
                assert not st["pos"][i, c2:].any() and not st["active"][i, c2:].any()
            else:
                assert np.array_equal(out["obs"][i, :c], o1["obs"][0]) and not out["obs"][i, c:].any()
            singles[i] = (cfg, s1)
            assert np.array_equal(st["pos"][i, :s1["pos"].shape[1]], s1["pos"][0])
        cnt = cnt_new
    assert switched.all()


@pytest.mark.parametrize("physics", [False, True])
def test_masked_step_with_uniform_counts_equals_oracle(physics):
    """With every n_e = N the reference's masked step is so.step(cfg, st, a, am, ...) bit for bit
    (no auto-reset: down to n_active == 0 in the kinematic mode)."""
    from oracle import swarm_oracle as so
    n, e = 5, 4
    base = so.make_cfg(num_drones=n, num_obstacles=4, max_steps=4)
    st_a, _ = so.reset_device(base, so.empty_state(base, e), seed=6, physics=physics)
    st_b = {k: v.copy() for k, v in st_a.items()}
    rng = np.random.default_rng(1)
    absent = 0
    for t in range(6):
        a = rng.uniform(-2, 2, (e, n, 3)).astype(np.float32)
        am = rng.uniform(size=(e, n)) > 0.3
        absent += int((~am).sum())
        st_a, out_a = so.step(base, st_a, a, am, auto_reset=False, seed=6, physics=physics)
        st_b, out_b, _, cnt = mr.step(base, {}, np.full(e, n), st_b, a, auto_reset=False, seed=6, physics=physics,
                                      action_mask=am)
        assert set(out_a) == set(out_b) and np.array_equal(cnt, np.full(e, n))
        for k in out_a:
            assert np.array_equal(out_a[k], out_b[k]), (t, k)
        for k in st_a:
            assert np.array_equal(st_a[k], st_b[k]), (t, k)
    assert absent > 0 and not st_a["active"].any()
    # the mask matters: the unmasked step of the same state differs
    st0, _ = so.reset_device(base, so.empty_state(base, e), seed=6, physics=physics)
    a = rng.uniform(-2, 2, (e, n, 3)).astype(np.float32)
    am = np.zeros((e, n), bool)
    s1, _, _, _ = mr.step(base, {}, None, st0, a, auto_reset=False, seed=6, physics=physics, action_mask=am)
    s2, _, _, _ = mr.step(base, {}, None, st0, a, auto_reset=False, seed=6, physics=physics)
    assert not np.array_equal(s1["vel"], s2["vel"])


@pytest.mark.parametrize("physics", [False, True])
def test_observe_reference(physics):
    """mr.observe: so.observe / norm1d / so.global_state for uniform counts; for mixed counts every
    env observed alone with num_drones = n_e, zeros in the slots that do not exist; envs outside
    the mask untouched; the state is not changed."""
    from oracle import swarm_oracle as so
    n, m, e = 5, 4, 4
    base = so.make_cfg(num_drones=n, num_obstacles=m, max_steps=9)
    st, _ = so.reset_device(base, so.empty_state(base, e), seed=8, physics=physics)
    rng = np.random.default_rng(5)
    st["vel"] = rng.uniform(-6, 6, st["vel"].shape).astype(np.float32)  # some above max_speed (physics clamps)
    got = mr.observe(base, {}, None, st, physics=physics)
    assert np.array_equal(got["obs"], so.observe(base, st["pos"], st["vel"], st["goal"], st["obst"], physics=physics))
    assert np.array_equal(got["dist_goal"], so.norm1d(st["goal"][:, None, :] - st["pos"]))
    assert np.array_equal(got["global_state"], so.global_state(st["pos"], st["vel"], st["goal"]))
    counts = np.array([3, 5, 1, 2])
    ov = dict(num_obstacles=np.array([4, 0, 2, 1], np.int32))
    keep = {k: v.copy() for k, v in st.items()}
    mask = np.array([True, True, False, True])
    got = mr.observe(base, ov, counts, st, env_mask=mask, physics=physics)
    for k in st:
        assert np.array_equal(st[k], keep[k]), k
    for i, c in enumerate(counts):
        if not mask[i]:
            assert all(np.isnan(got[k][i]).all() for k in got)
            continue
        cfg = dict(base, num_drones=int(c), num_obstacles=int(ov["num_obstacles"][i]))
        p, v, g, o = st["pos"][i:i + 1, :c], st["vel"][i:i + 1, :c], st["goal"][i:i + 1], \
            st["obst"][i:i + 1, :cfg["num_obstacles"]]
        assert np.array_equal(got["obs"][i, :c], so.observe(cfg, p, v, g, o, physics=physics)[0])
        assert not got["obs"][i, c:].any() and not got["dist_goal"][i, c:].any()
        assert np.array_equal(got["dist_goal"][i, :c], so.norm1d(g[:, None, :] - p)[0])
        assert np.array_equal(got["global_state"][i], mr.pad_global_state(so.global_state(p, v, g), n)[0])
        if c - 1 < base["neighbor_k"]:  # spare neighbour slots are zero
            assert not got["obs"][i, :c, 9 + 4 * (c - 1):9 + 4 * base["neighbor_k"]].any()
    # `out` given: rows outside the mask keep what they held
    out = {k: np.full_like(v, 7.0) for k, v in got.items()}
    mr.observe(base, ov, counts, st, env_mask=mask, physics=physics, out=out)
    assert all((out[k][2] == 7.0).all() and np.array_equal(out[k][mask], got[k][mask]) for k in out)


def test_set_drones_argument_errors(nat, lib):
    """swarm_env_cfg_set_drones validates before any launch (no GPU is touched)."""
    p0 = _params(nat, lib, num_envs=0)
    assert lib.swarm_env_cfg_set_drones(ctypes.byref(p0), None, None, None, None) == 0  # empty: no-op
    p = _params(nat, lib, num_envs=4)
    assert lib.swarm_env_cfg_set_drones(None, None, None, 64, None) == nat.SWARM_ENULL
    assert lib.swarm_env_cfg_set_drones(ctypes.byref(p), None, None, None, None) == nat.SWARM_ENULL
    assert b"env_cfg" in lib.swarm_last_error()
    with pytest.raises(ValueError):
        nat.check(nat.SWARM_ENULL, lib)
    bad = _params(nat, lib, num_envs=4, num_drones=0)
    assert lib.swarm_env_cfg_set_drones(ctypes.byref(bad), None, None, 64, None) == nat.SWARM_ELIMIT
    old = _params(nat, lib, num_envs=4, abi_version=1)
    assert lib.swarm_env_cfg_set_drones(ctypes.byref(old), None, None, 64, None) == nat.SWARM_EINVAL


def test_record_layout_unchanged(nat, tmp_path):
    """The count took the record's unused int32: size, offsets and the ABI version stay."""
    assert nat.ENV_CFG_BYTES == 64 == ctypes.sizeof(nat.SwarmEnvCfg)
    assert nat.SwarmEnvCfg.num_drones.offset == 44 and nat.SwarmEnvCfg.num_drones.size == 4
    assert nat.SwarmEnvCfg.num_obstacles.offset == 40 and nat.SwarmEnvCfg.max_speed_d.offset == 48
    assert nat.ABI_VERSION == 5
    assert ctypes.sizeof(nat.SwarmEnvOverrides) == 7 * ctypes.sizeof(ctypes.c_void_p)  # did not grow
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "swarm_mi355x.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %d\\n", sizeof(swarm_env_cfg_t), offsetof(swarm_env_cfg_t, num_drones),\n'
                   '       sizeof(swarm_env_overrides_t), SWARM_ABI_VERSION);\nreturn 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [64, 44, 56, 5]


def test_mixed_size_batch_validation():
    """Stages may differ in num_drones and STAGE_PARAMS only; checked before anything is built
    (no GPU is needed to be refused)."""
    from swarm_marl_amd.curriculum import assign_stage, mixed_size_batch
    cfg = {"stages": [{"env_config": {"num_drones": 3, "num_obstacles": 0}},
                      {"env_config": {"num_drones": 5, "num_obstacles": 4}},
                      {"env_config": {"num_drones": 8, "num_obstacles": 4, "neighbor_k": 2}}]}
    with pytest.raises(ValueError, match="other than num_drones"):
        mixed_size_batch(cfg, [0, 1, 2])
    with pytest.raises(ValueError, match="out of range"):
        mixed_size_batch(cfg, [0, 3])
    with pytest.raises(ValueError):
        mixed_size_batch(cfg, [])
    with pytest.raises(ValueError, match="out of range"):
        assign_stage(None, cfg, None, 3)
