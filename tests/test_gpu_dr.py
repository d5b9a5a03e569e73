"""GPU: keyed domain randomisation (csrc/swarm_dr.hip `swarm_env_cfg_randomize`,
`DomainRandomizer(keyed=True)`, `RolloutCollector(graph=True, randomizer=keyed)`), DESIGN.md §3.8.

The yardstick is tests/dr_ref.py (the draw, NumPy float64) fed through the existing record path,
`vec.set_env_config(**values)` (swarm_env_cfg_set): a randomised record must hold, byte for byte, what
that path derives from the same five doubles.  Every comparison is bitwise.

1. Records at E 1 / 63 / 257, env_offset 0 / 70,000, arbitrary episode numbers with 2^32 - 1 among them,
   episode_add 0 and 1 (the wrap), with every parameter on, dt off, in physics mode, and all off (the
   uniform record).
2. Ownership: max_steps / num_obstacles / num_drones stay; envs outside the mask keep all 64 bytes;
   mask_bits picks bits of env_done.
3. The invariant env_cfg = record(draw(episode)), env_cfg_next = record(draw(episode + 1)) over 7 steps
   in which every env resets three times, with after_step() once and twice per step.
4. Shards (env_offset) and env groups give the records of one batch.
5. A curriculum mix keeps its per-env max_steps / num_obstacles / num_drones under the randomiser.
6. The graph collector with a keyed randomiser against its eager twin; no allocation.
7. Refusals.
"""
from __future__ import annotations

import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from tests import dr_ref

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
DR_PATH = ROOT / "tests" / "golden" / "domain_randomization_v1.yaml"
SEED = 0x9E3779B97F4A7C15
# the bytes of a swarm_env_cfg_t the randomiser owns: the nine floats and the two doubles, not the
# three int32 at 36..47 (max_steps, num_obstacles, num_drones)
OWNED = np.ones(64, bool)
OWNED[36:48] = False


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def dr_cfg():
    return yaml.safe_load(DR_PATH.read_text())


def _ranges(dr_cfg, physics=False):
    from swarm_marl_amd.domain_randomization import scale_ranges
    return scale_ranges(dr_cfg, physics=physics)[0]


def _base(vec):
    return {p: float(getattr(vec.cfg, p)) for p in dr_ref.PARAMS}


def _table(nat, ranges):
    t = nat.SwarmDrTable()
    for i, name in enumerate(nat.DR_PARAMS):
        if name in ranges:
            t.lo[i], t.hi[i] = ranges[name]
            t.enabled[i] = 1
    return t


def _randomize(vec, table, seed, add, mask, bits, dst):
    from swarm_marl_amd import _native as nat
    rc = vec.lib.swarm_env_cfg_randomize(ctypes.byref(vec.params), ctypes.byref(table), seed & (2**64 - 1),
                                         vec.episode.data_ptr(), add, None if mask is None else mask.data_ptr(), bits,
                                         dst.data_ptr(), torch.cuda.current_stream(vec.device).cuda_stream)
    nat.check(rc, vec.lib, which="dr")


def _episodes(vec):
    return vec.episode.cpu().numpy().view(np.uint32).astype(np.int64)


def _global(vec):
    return int(vec.params.env_offset) + np.arange(vec.num_envs, dtype=np.int64)


def _expected(ref_vec, seed, episodes, ranges, physics=False):
    """[E, 64] bytes: the records swarm_env_cfg_set derives from the reference draw of `episodes`, on
    `ref_vec` (a batch of the same shape, config and env_offset whose records are free to overwrite)."""
    vals = dr_ref.values(seed, _global(ref_vec), episodes, ranges, _base(ref_vec))
    if physics:
        assert "dt" not in ranges and np.all(vals["dt"] == ref_vec.cfg.dt)
        del vals["dt"]  # the record path refuses a per-env dt in physics mode; the base value is what it writes
    ref_vec.set_env_config(next_episode=True, **vals)
    return ref_vec.env_cfg_next.cpu().numpy().copy()


# ---------------------------------------------------------------- 1. records
@pytest.mark.parametrize("mode", ["all", "no_dt", "physics", "none"])
@pytest.mark.parametrize("env_offset", [0, 70000])
@pytest.mark.parametrize("e", [1, 63, 257])
def test_records_equal_the_record_path_on_the_reference_draw(dev, dr_cfg, e, env_offset, mode):
    from swarm_marl_amd import VecSwarm
    from swarm_marl_amd import _native as nat
    physics = mode == "physics"
    vec = VecSwarm(e, dict(num_drones=3), device=dev, seed=3, env_offset=env_offset,
                   dynamics="physics" if physics else "kinematic")
    ranges = _ranges(dr_cfg, physics)
    if mode == "no_dt":
        del ranges["dt"]
    elif mode == "none":
        ranges = {}
    assert ("dt" in ranges) == (mode == "all")
    rng = np.random.default_rng(e + env_offset)
    ep = rng.integers(0, 2**32, e, dtype=np.uint64).astype(np.int64)
    if e > 2:
        ep[:2] = (0, 2**31)
        ep[2 + rng.integers(0, e - 2)] = 2**32 - 1
    else:
        ep[0] = 2**32 - 1
    vec.set_state(episode=ep.astype(np.uint32).view(np.int32))
    assert np.array_equal(_episodes(vec), ep)
    table = _table(nat, ranges)
    for add in (0, 1):
        want = _expected(vec, SEED, ep + add, ranges, physics)
        got = torch.from_numpy(np.where(OWNED, np.uint8(0xA5), want)).to(dev)  # owned bytes scrambled
        assert got.shape == (e, 64)
        arena = torch.full((e + 2, 64), 0x5A, dtype=torch.uint8, device=dev)  # a guard record on either side
        arena[1:e + 1] = got
        _randomize(vec, table, SEED, add, None, 0xFF, arena[1:])
        out = arena.cpu().numpy()
        assert np.array_equal(out[1:e + 1], want), (add, np.argwhere(out[1:e + 1] != want)[:4])
        assert np.all(out[0] == 0x5A) and np.all(out[e + 1] == 0x5A)
        if mode == "none":  # every parameter off: the uniform record
            vec.set_env_config()
            assert np.array_equal(out[1:e + 1], vec.env_cfg.cpu().numpy())
        else:
            ws = out[1:e + 1].view(np.float64)[:, 7]
            assert np.array_equal(ws, dr_ref.values(SEED, _global(vec), ep + add, ranges, _base(vec))["world_size"])
            if e > 1:
                assert len(np.unique(ws)) == e
    # another seed draws other records
    other = torch.zeros((e, 64), dtype=torch.uint8, device=dev)
    _randomize(vec, table, SEED + 1, 1, None, 0xFF, other)
    assert (mode == "none") == np.array_equal(other.cpu().numpy()[:, OWNED], want[:, OWNED])


# ---------------------------------------------------------------- 2. ownership and mask
def test_ownership_and_mask(dev, dr_cfg):
    from swarm_marl_amd import VecSwarm
    from swarm_marl_amd import _native as nat
    e, n = 257, 8
    vec = VecSwarm(e, dict(num_drones=n, num_obstacles=4), device=dev, seed=3, env_offset=11)
    rng = np.random.default_rng(2)
    ints = dict(max_steps=rng.integers(1, 500, e).astype(np.int32), num_obstacles=rng.integers(0, 5, e).astype(np.int32),
                num_drones=rng.integers(1, n + 1, e).astype(np.int32))
    ep = rng.integers(0, 2**32, e, dtype=np.uint64).astype(np.int64)
    vec.set_state(episode=ep.astype(np.uint32).view(np.int32))
    ranges = _ranges(dr_cfg)
    table = _table(nat, ranges)
    want = _expected(vec, SEED, ep + 1, ranges)
    vec.set_env_config(next_episode=True, **ints)  # per-env counts, horizons and obstacle counts
    before = vec.env_cfg_next.cpu().numpy().copy()
    i32 = before.view(np.int32)
    assert np.array_equal(i32[:, 9], ints["max_steps"]) and np.array_equal(i32[:, 10], ints["num_obstacles"])
    assert np.array_equal(i32[:, 11], ints["num_drones"])
    assert not np.array_equal(before[:, OWNED], want[:, OWNED])  # uniform values so far
    # env_done-like bytes: the RESET bit alone, with the others, and other bits only
    mask = rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, 7, 0xFB, 0xFF], np.uint8), e)
    mask[:4] = (4, 0xFB, 0, 7)
    sel = (mask & nat.ENV_RESET) != 0
    assert 40 < sel.sum() < e - 40
    _randomize(vec, table, SEED, 1, torch.from_numpy(mask).to(dev), nat.ENV_RESET, vec.env_cfg_next)
    after = vec.env_cfg_next.cpu().numpy()
    assert np.array_equal(after[~sel], before[~sel])  # all 64 bytes
    assert np.array_equal(after[sel][:, OWNED], want[sel][:, OWNED])
    assert np.array_equal(after[:, ~OWNED], before[:, ~OWNED])  # the three int fields, everywhere
    # other bits only: nothing is written
    quiet = torch.from_numpy(np.where(sel, mask & ~np.uint8(nat.ENV_RESET), mask).astype(np.uint8)).to(dev)
    assert bool(quiet.any()) and not bool((quiet & nat.ENV_RESET).any())
    vec.env_cfg_next.copy_(torch.from_numpy(before).to(dev))
    _randomize(vec, table, SEED, 1, quiet, nat.ENV_RESET, vec.env_cfg_next)
    assert np.array_equal(vec.env_cfg_next.cpu().numpy(), before)
    # a bool mask with mask_bits 0xFF, as after_reset passes it
    _randomize(vec, table, SEED, 1, torch.from_numpy(sel).to(dev), 0xFF, vec.env_cfg_next)
    after = vec.env_cfg_next.cpu().numpy()
    assert np.array_equal(after[~sel], before[~sel]) and np.array_equal(after[sel][:, OWNED], want[sel][:, OWNED])


# ---------------------------------------------------------------- 3. the invariant over resets
def _actions(vec, gen):
    return torch.rand((vec.num_envs, vec.num_drones, 3), device=vec.device, generator=gen) * 2 - 1


def _check_invariant(vec, ref_vec, seed, ranges, tag):
    ep = _episodes(vec)
    cur, nxt = vec.env_cfg.cpu().numpy(), vec.env_cfg_next.cpu().numpy()
    want_cur = _expected(ref_vec, seed, ep, ranges)
    want_nxt = _expected(ref_vec, seed, ep + 1, ranges)
    assert np.array_equal(cur[:, OWNED], want_cur[:, OWNED]), (tag, "current")
    assert np.array_equal(nxt[:, OWNED], want_nxt[:, OWNED]), (tag, "next")
    return cur, nxt


@pytest.mark.parametrize("calls", [1, 2])
def test_invariant_over_resets(dev, dr_cfg, calls):
    from swarm_marl_amd import VecSwarm
    from swarm_marl_amd import _native as nat
    from swarm_marl_amd.domain_randomization import DomainRandomizer
    e, n = 70, 3
    kw = dict(device=dev, auto_reset=True, seed=5, env_offset=9)
    vec, ref_vec = (VecSwarm(e, dict(num_drones=n, max_steps=2), **kw) for _ in range(2))
    dr = DomainRandomizer(vec, dr_cfg, seed=SEED, force=True, keyed=True)
    assert dr.keyed and dr.generator is None
    ranges = dr.ranges
    dr.begin()
    cur, nxt = _check_invariant(vec, ref_vec, SEED, ranges, "begin")
    assert np.all(_episodes(vec) == 1)
    assert np.array_equal(cur[:, ~OWNED], nxt[:, ~OWNED]) and np.all(cur.view(np.int32)[:, 9] == 2)
    assert len(np.unique(cur.view(np.float64)[:, 7])) == e and not np.array_equal(cur, nxt)
    # sample() in keyed mode: the current episode's values
    vals = dr.sample()
    want = dr_ref.values(SEED, _global(vec), _episodes(vec), ranges, _base(vec))
    assert set(vals) == set(ranges)
    for p in ranges:
        assert vals[p].dtype == torch.float64 and np.array_equal(vals[p].cpu().numpy(), want[p]), p
    gen = torch.Generator(device=dev).manual_seed(1)
    resets = 0
    for t in range(7):
        vec.step(_actions(vec, gen))
        for _ in range(calls):
            dr.after_step()
        resets += int(((vec.env_done & nat.ENV_RESET) != 0).sum())
        _check_invariant(vec, ref_vec, SEED, ranges, t)
    assert resets >= 3 * e
    assert _episodes(vec).min() >= 4
    # an explicit reset of some envs, then after_reset with the same mask
    m = torch.arange(e, device=dev) % 3 == 0
    vec.reset(m)
    dr.after_reset(m)
    _check_invariant(vec, ref_vec, SEED, ranges, "after_reset")


# ---------------------------------------------------------------- 4. shards and groups
def _run(vecs, dr_cfg, actions):
    """begin() and 5 steps with after_step() on each batch of `vecs` (shards of one global batch);
    returns the concatenated (env_cfg, env_cfg_next, episode, pos) as numpy."""
    from swarm_marl_amd.domain_randomization import DomainRandomizer
    out = []
    lo = 0
    for vec in vecs:
        dr = DomainRandomizer(vec, dr_cfg, seed=SEED, force=True, keyed=True)
        dr.begin()
        for a in actions:
            vec.step(a[lo:lo + vec.num_envs].contiguous())
            dr.after_step()
        out.append([x.cpu().numpy() for x in (vec.env_cfg, vec.env_cfg_next, vec.episode, vec.pos)])
        lo += vec.num_envs
    return [np.concatenate([o[i] for o in out]) for i in range(4)]


def test_shards_and_groups_draw_the_records_of_one_batch(dev, dr_cfg):
    from swarm_marl_amd import VecSwarm
    e, n = 64, 3
    cfg = dict(num_drones=n, max_steps=2)
    gen = torch.Generator(device=dev).manual_seed(4)
    actions = [torch.rand((e, n, 3), device=dev, generator=gen) * 2 - 1 for _ in range(5)]
    kw = dict(device=dev, auto_reset=True, seed=8)
    one = _run([VecSwarm(e, cfg, **kw)], dr_cfg, actions)
    assert one[2].min() >= 3 and len(np.unique(one[0].view(np.float64)[:, 7])) == e
    shards = _run([VecSwarm(32, cfg, env_offset=0, **kw), VecSwarm(32, cfg, env_offset=32, **kw)], dr_cfg, actions)
    groups = _run([VecSwarm(e, cfg, groups=2, **kw)], dr_cfg, actions)
    for name, other in (("shards", shards), ("groups", groups)):
        for i, what in enumerate(("env_cfg", "env_cfg_next", "episode", "pos")):
            assert np.array_equal(one[i].view(np.uint8), other[i].view(np.uint8)), (name, what)


# ---------------------------------------------------------------- 5. curriculum composition
def test_a_curriculum_mix_keeps_its_stage_fields(dev, dr_cfg):
    from swarm_marl_amd import _native as nat
    from swarm_marl_amd.curriculum import mixed_size_batch
    from swarm_marl_amd.domain_randomization import DomainRandomizer
    stages = [dict(name=f"s{k}", env_config=dict(num_drones=k, num_obstacles=m, max_steps=2))
              for k, m in ((3, 2), (5, 3), (8, 4))]
    e = 24
    vec, over = mixed_size_batch(dict(stages=stages), [0, 1, 2] * 8, device=dev, seed=6)
    assert vec.num_drones == 8 and vec.cfg.max_steps != 2 and vec.cfg.num_obstacles == 4
    dr = DomainRandomizer(vec, dr_cfg, seed=SEED, force=True, keyed=True)
    dr.begin()
    gen = torch.Generator(device=dev).manual_seed(2)
    resets = 0
    for t in range(6):
        vec.step(_actions(vec, gen))
        dr.after_step()
        resets += int(((vec.env_done & nat.ENV_RESET) != 0).sum())
        for rec in (vec.env_cfg, vec.env_cfg_next):
            i32 = rec.cpu().numpy().view(np.int32)
            assert np.array_equal(i32[:, 9], over["max_steps"]), t
            assert np.array_equal(i32[:, 10], over["num_obstacles"]), t
            assert np.array_equal(i32[:, 11], over["num_drones"]), t
    assert resets >= 3 * e
    # and the randomised fields are the keyed draw of the batch's base values
    ep = _episodes(vec)
    want = dr_ref.values(SEED, _global(vec), ep, dr.ranges, _base(vec))
    cur = vec.env_cfg.cpu().numpy()
    assert np.array_equal(cur.view(np.float64)[:, 7], want["world_size"])
    assert np.array_equal(cur.view(np.float64)[:, 6], want["max_speed"])
    assert np.array_equal(cur.view(np.float32)[:, 3], want["dt"].astype(np.float32))
    # the slots beyond an env's count stay empty
    assert not bool(vec.active[0, 3:].any()) and bool(vec.active[2].all())


# ---------------------------------------------------------------- 6. the graph collector
def _actor(dev):
    from swarm_marl_amd.policy import PolicyMLP
    rng = np.random.default_rng(5)
    shapes = ((256, 37), (256,), (256, 256), (256,), (6, 256), (6,))
    arrays = [rng.uniform(-1, 1, s).astype(np.float32) / np.float32(np.sqrt(s[-1])) for s in shapes]
    return PolicyMLP.from_arrays(*arrays, device=dev, precision="bf16")


def _i32(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("perturbed", [False, True])
def test_graph_collector_with_a_keyed_randomizer_equals_eager(dev, dr_cfg, perturbed):
    from swarm_marl_amd import CriticMLP, Perturbation, RolloutCollector, VecSwarm
    from swarm_marl_amd.domain_randomization import DomainRandomizer
    from tests import critic_ref as cr
    n, e, t = 3, 33, 5
    policy = _actor(dev)
    critic = CriticMLP(cr.make_critic(6 * n + 3, seed=2), device=dev, precision="bf16")
    cols = []
    for graph in (False, True):
        vec = VecSwarm(e, dict(num_drones=n, max_steps=2), device=dev, auto_reset=True, seed=11, with_global_state=True)
        dr = DomainRandomizer(vec, dr_cfg, seed=SEED, force=True, keyed=True)
        dr.begin()
        per = Perturbation(vec, DR_PATH, seed=SEED, force=True) if perturbed else None
        cols.append(RolloutCollector(vec, policy, critic, horizon=t, seed=7, perturb=per, randomizer=dr, graph=graph))
    eager, graph = cols
    ref_vec = VecSwarm(e, dict(num_drones=n, max_steps=2), device=dev, seed=11)
    for frag in range(2):
        a, b = eager.collect(), graph.collect()
        assert set(a) == set(b)
        for k, v in a.items():
            assert torch.equal(_i32(v), _i32(b[k])), (frag, k)
        sa, sb = eager.vec.state_dict(), graph.vec.state_dict()
        for k in sa:
            assert torch.equal(_i32(sa[k]), _i32(sb[k])), (frag, k)
        assert torch.equal(eager.vec.env_cfg, graph.vec.env_cfg) and torch.equal(eager.vec.env_cfg_next, graph.vec.env_cfg_next)
        if perturbed:
            assert torch.equal(_i32(eager.perturb.ring), _i32(graph.perturb.ring))
        _check_invariant(graph.vec, ref_vec, SEED, graph.randomizer.ranges, ("graph", frag))
        assert bool(b["env_done"].any())
    assert graph.captures == 1 and eager.captures == 0
    assert _episodes(graph.vec).min() >= 5  # max_steps = 2 over 10 steps
    # replays allocate nothing; nor do eager after_step() calls
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    for _ in range(3):
        graph.collect()
        assert torch.cuda.memory_allocated(dev) == before
    for _ in range(10):
        eager.randomizer.after_step()
        assert torch.cuda.memory_allocated(dev) == before
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(dev) == before and graph.captures == 1
    _check_invariant(graph.vec, ref_vec, SEED, graph.randomizer.ranges, "after replays")


def test_another_seed_is_another_graph(dev, dr_cfg):
    """The seed and the table are launch constants: the collector's key holds them."""
    from swarm_marl_amd import RolloutCollector, VecSwarm
    from swarm_marl_amd.domain_randomization import DomainRandomizer
    vec = VecSwarm(4, dict(num_drones=3, max_steps=2), device=dev, auto_reset=True, seed=1)
    keys = []
    for seed, profile in ((1, "train"), (2, "train"), (1, "ood")):
        dr = DomainRandomizer(vec, dr_cfg, seed=seed, profile=profile, force=True, keyed=True)
        dr.begin()
        keys.append(RolloutCollector(vec, _actor(dev), None, horizon=2, randomizer=dr, graph=True)._graph_key())
    assert keys[0] != keys[1]
    ood = DomainRandomizer(vec, dr_cfg, seed=1, profile="ood", force=True, keyed=True)
    assert (keys[0] != keys[2]) == (ood.ranges != _ranges(dr_cfg))


# ---------------------------------------------------------------- 7. refusals
def test_refusals(dev, dr_cfg):
    from swarm_marl_amd import RolloutCollector, VecSwarm
    from swarm_marl_amd.domain_randomization import DomainRandomizer
    pol = _actor(dev)
    vec = VecSwarm(4, dict(num_drones=3), device=dev, seed=1)
    plain = DomainRandomizer(vec, dr_cfg, seed=1, force=True)
    assert not plain.keyed and plain.generator is not None
    with pytest.raises(ValueError, match="randomizer"):
        RolloutCollector(vec, pol, None, horizon=2, randomizer=plain, graph=True)
    grouped = VecSwarm(4, dict(num_drones=3), device=dev, groups=2)
    keyed = DomainRandomizer(grouped, dr_cfg, seed=1, force=True, keyed=True)
    with pytest.raises(ValueError, match="group"):
        RolloutCollector(grouped, pol, None, horizon=2, randomizer=keyed, graph=True)
    RolloutCollector(grouped, pol, None, horizon=2, randomizer=keyed)  # eager takes it
    # a keyed launch before begin() has no records to write
    with pytest.raises(RuntimeError, match="begin"):
        DomainRandomizer(vec, dr_cfg, seed=1, force=True, keyed=True).after_step()
    # physics: dt is not randomised (scale_ranges reports it), so the table leaves it off
    phys = VecSwarm(4, dict(num_drones=3), device=dev, dynamics="physics")
    dr = DomainRandomizer(phys, dr_cfg, seed=1, force=True, keyed=True)
    assert "dt" not in dr.ranges and dr.table.enabled[1] == 0 and "dynamics.dt_scale" in dr.unsupported
    dr.begin()
    torch.cuda.synchronize()
