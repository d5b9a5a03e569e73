"""GPU: csrc/swarm_rollout.hip (swarm_rollout_sample, swarm_rollout_record) and
`RolloutCollector(..., graph=True)` against the eager collector.

1. swarm_rollout_sample against the fused actor kernels, bit for bit: for the logits a
   `PolicyMLP.forward(sample=True)` launch writes, the same (seed, counter) gives that launch's
   actions; rows 1, 15, 63, 65 and 1,000, the bf16, f32x3 and f32 actors, counters 0, 5 and 2^32 + 3,
   each split as *counter_dev + counter_add with addends 0 and 3 (counter 0 with addend 3 wraps the
   64-bit sum), once across the low word's carry (2^32 - 1 plus 4) and once with counter_dev NULL.
   act_dim 1..6 against tests/policy_ref.py's float64 draw under the bound of
   tests/test_gpu_policy_sample.py (derived in tests/test_gpu_policy_dims.py).
2. swarm_rollout_record: eight segments of 1 .. 1,048,583 bytes at src / dst offsets 0, 1, 2, 4, 8 from
   a 16-byte boundary into one guard-filled arena; one dst NULL, one empty.  Every destination equals
   its source and every other byte of the arena is the guard.
3. Graph collector against its eager twin over three fragments (every tensor of the batch, the env
   state, the delay line, the counter), in the five configurations of CONFIGS; deterministic
   fragments, weights loaded in place, a PPOLearner update, no allocation across replays, refusals.
"""
from __future__ import annotations

import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import attn_ref as ar
from tests import critic_ref as cr
from tests import policy_ref as pr
from tests import value_ref as vr
from tests.test_gpu_policy_sample import check_z, noise, recovered_z

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
DR_PATH = ROOT / "tests" / "golden" / "domain_randomization_v1.yaml"
SEED = 0x9E3779B97F4A7C15
M64 = 2**64 - 1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _i32(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _word(dev, value):
    """A one-element int64 device tensor holding the u64 `value`."""
    value &= M64
    return torch.tensor([value - 2**64 if value >= 2**63 else value], dtype=torch.int64, device=dev)


# ---------------------------------------------------------------- 1. the sample kernel
@pytest.mark.parametrize("precision", ["bf16", "f32x3", "f32"])
def test_sample_equals_the_fused_actor_bitwise(dev, precision):
    from swarm_marl_amd import rollout_sample
    from swarm_marl_amd.policy import PolicyMLP
    pol = PolicyMLP(pr.make_actor(37, 6, log_std_scale=0.25), device=dev, precision=precision)
    g = torch.Generator(device=dev).manual_seed(3)
    for rows in (1, 15, 63, 65, 1000):
        obs = torch.rand((rows, 37), device=dev, generator=g) * 6 - 3
        lg, want = torch.empty((rows, 6), device=dev), torch.empty((rows, 3), device=dev)
        cases = [(c, c - add, add) for c in (0, 5, 2**32 + 3) for add in (0, 3)]
        cases += [(2**32 + 3, 2**32 - 1, 4), (5, None, 5)]  # the carry into the high word; no device word
        for counter, word, add in cases:
            pol.forward(obs, logits=lg, actions=want, sample=True, seed=SEED, counter=counter)
            got = torch.full((rows, 3), -555.0, device=dev)
            rollout_sample(lg, got, seed=SEED, counter=add, counter_dev=None if word is None else _word(dev, word))
            assert torch.equal(_i32(got), _i32(want)), (rows, counter, word, add)
            assert not torch.equal(got, lg[:, :3])  # sampled
        other = torch.empty((rows, 3), device=dev)
        rollout_sample(lg, other, seed=SEED, counter=0, counter_dev=_word(dev, 2**32 - 1))  # one below: other draws
        assert bool((_i32(other) != _i32(want)).any(dim=1).all())


@pytest.mark.parametrize("ad", [1, 2, 3, 4, 5, 6])
def test_sample_draws_the_defined_normals_at_every_act_dim(dev, ad):
    from swarm_marl_amd import rollout_sample
    rows, counter = pr.ROWS, (1 << 32) + 3
    rng = np.random.default_rng(ad)
    lg = np.concatenate([rng.uniform(-1, 1, (rows, ad)), rng.uniform(-2.0, 0.5, (rows, ad))], axis=1).astype(np.float32)
    arena = torch.full((rows * ad + 64,), -555.0, device=dev)  # nothing past rows * ad is written
    out = arena[:rows * ad].view(rows, ad)
    rollout_sample(torch.from_numpy(lg).to(dev), out, seed=SEED, counter=3, counter_dev=_word(dev, 1 << 32))
    a = out.cpu().numpy()
    assert bool((arena[rows * ad:] == -555.0).all())
    z, ls = recovered_z(lg, a)
    check_z(z, noise(rows, ad, SEED, counter), a, ls, f"swarm_rollout_sample ad={ad}")


# ---------------------------------------------------------------- 2. the record kernel
SIZES = (1, 15, 16, 17, 4097, 1048583)
GUARD = 0xA5
# (src offset, dst offset) from a 16-byte boundary per segment, in three mixes: every size meets the
# 16-byte path (0, 0), the 4-byte path and the byte path
OFFSETS = (
    ((0, 0), (1, 1), (4, 8), (2, 0), (0, 0), (8, 4), (0, 0), (1, 2)),
    ((4, 4), (0, 0), (1, 0), (0, 0), (2, 8), (0, 0), (4, 0), (8, 8)),
    ((1, 4), (8, 4), (0, 0), (4, 4), (0, 1), (1, 1), (2, 2), (0, 0)),
)


@pytest.mark.parametrize("mix", [0, 1, 2])
def test_record_copies_eight_segments_and_nothing_else(dev, mix):
    from swarm_marl_amd import _native as nat
    lib = nat.load_library()
    sizes = SIZES + (333, 0)  # segment 6 gets dst NULL, segment 7 is empty
    pad = 256
    total = sum((s + 2 * pad + 15) // 16 * 16 for s in sizes)
    g = torch.Generator(device=dev).manual_seed(mix)
    src = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev, generator=g)
    dst = torch.full((total,), GUARD, dtype=torch.uint8, device=dev)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    want = np.full(total, GUARD, np.uint8)
    host = src.cpu().numpy()
    rec = nat.SwarmRolloutRecord()
    rec.count = 8
    base = 0
    for i, (size, (so, do)) in enumerate(zip(sizes, OFFSETS[mix])):
        s0, d0 = base + pad + so, base + pad + do
        seg = rec.segments[i]
        seg.src, seg.bytes = src.data_ptr() + s0, size
        seg.dst = None if i == 6 else dst.data_ptr() + d0
        if i != 6:
            want[d0:d0 + size] = host[s0:s0 + size]
        base += (size + 2 * pad + 15) // 16 * 16
    nat.check(lib.swarm_rollout_record(ctypes.byref(rec), torch.cuda.current_stream(dev).cuda_stream), lib, which="rollout")
    got = dst.cpu().numpy()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert np.array_equal(src.cpu().numpy(), host)  # the sources are read only


def test_record_wrapper_copies_tensor_pairs(dev):
    from swarm_marl_amd import rollout_record
    g = torch.Generator(device=dev).manual_seed(1)
    a = torch.rand((5, 3, 37), device=dev, generator=g)
    b = torch.rand((15,), device=dev, generator=g) > 0.5
    flags = torch.zeros((4, 15), dtype=torch.bool, device=dev)
    obs = torch.zeros((2, 5, 3, 37), device=dev)
    rollout_record([(a, obs[1]), (b, flags[3]), (a, None)])
    assert torch.equal(obs[1], a) and torch.equal(flags[3], b) and not bool(flags[:3].any()) and not bool(obs[0].any())
    with pytest.raises(ValueError):
        rollout_record([(a, obs)])  # sizes differ


# ---------------------------------------------------------------- 3. the graph collector
CFG = dict(max_steps=4)  # episodes end (and auto-reset) inside every fragment


def _arrays(shapes, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1, 1, s).astype(np.float32) / np.float32(np.sqrt(s[-1])) for s in shapes]


def _actor_arrays(seed, in_dim=37):
    return _arrays(((256, in_dim), (256,), (256, 256), (256,), (6, 256), (6,)), seed)


def _mlp_actor(dev, precision, seed=5):
    from swarm_marl_amd.policy import PolicyMLP
    return PolicyMLP.from_arrays(*_actor_arrays(seed), device=dev, precision=precision)


def _twins(dev, name):
    """(eager collector, graph collector) on two envs with one seed, sharing policy and critic."""
    from swarm_marl_amd import (AgentValueMLP, AttentionPolicy, CriticMLP, Perturbation, RolloutCollector, VecSwarm)
    n, e, t = dict(bf16=(3, 5, 4), agent=(8, 130, 3), attn=(64, 16, 2), perturb=(5, 33, 3), counts=(8, 12, 3))[name]
    gs = name not in ("agent", "attn")
    if name == "attn":
        params, layers = ar.make_attn(3, 4, 6, log_std_scale=0.25)
        policy = AttentionPolicy(params, layers, neighbor_k=3, sensed_obstacles=4, device=dev)
        critic = None
    elif name == "agent":
        policy = _mlp_actor(dev, "f32x3")
        critic = AgentValueMLP(vr.make_value(37, seed=2), device=dev, precision="f32")
    else:
        policy = _mlp_actor(dev, "bf16")
        critic = CriticMLP(cr.make_critic(6 * n + 3, seed=2), device=dev, precision="bf16")
    cols = []
    for graph in (False, True):
        vec = VecSwarm(e, dict(CFG, num_drones=n), device=dev, auto_reset=True, seed=11, with_global_state=gs)
        if name == "counts":
            vec.set_env_config(num_drones=np.array([3, 5, 8] * 4))
        vec.reset()
        per = Perturbation(vec, DR_PATH, seed=SEED, force=True) if name == "perturb" else None
        cols.append(RolloutCollector(vec, policy, critic, horizon=t, seed=7, perturb=per, graph=graph))
    assert cols[0].vec.obs_dim == 37 and not cols[0].graph and cols[1].graph
    return cols


def _same_batch(a, b, tag):
    assert set(a) == set(b)
    for k, v in a.items():
        if v is None:
            assert b[k] is None, (tag, k)
        else:
            assert torch.equal(_i32(v), _i32(b[k])), (tag, k)


def _same_state(eager, graph, tag):
    sa, sb = eager.vec.state_dict(), graph.vec.state_dict()
    for k in sa:
        assert torch.equal(_i32(sa[k]), _i32(sb[k])), (tag, k)
    if eager.perturb is not None:
        assert torch.equal(_i32(eager.perturb.ring), _i32(graph.perturb.ring)), tag
    assert eager.counter == graph.counter, tag


@pytest.mark.parametrize("name", ["bf16", "agent", "attn", "perturb", "counts"])
def test_graph_fragments_equal_eager_fragments(dev, name):
    eager, graph = _twins(dev, name)
    before = {k: v.clone() for k, v in graph.vec.state_dict().items()}
    actions = []
    for frag in range(3):
        a, b = eager.collect(), graph.collect()
        _same_batch(a, b, (name, frag))
        _same_state(eager, graph, (name, frag))
        actions.append(b["actions"].clone())
        assert bool(b["valid"].any()) and bool(torch.isfinite(b["advantage"]).all())
    assert graph.captures == 1 and graph.counter == 3 * graph.horizon
    assert not torch.equal(actions[0], actions[1]) and not torch.equal(actions[1], actions[2])  # new noise per replay
    assert not torch.equal(before["pos"], graph.vec.pos)
    if name != "attn":
        assert bool(graph.env_done.any())  # max_steps = 4: the fragments cross episode ends


def test_capture_leaves_env_delay_line_and_counter_alone(dev):
    """The first collect() captures, then replays once: afterwards the env stands where one eager
    fragment puts it (not two), which `test_graph_fragments_equal_eager_fragments` checks at every
    fragment; here a counter set by hand before the first call is the one the fragment uses."""
    eager, graph = _twins(dev, "perturb")
    eager.counter = graph.counter = 2**32 - 2  # the fragment's counters cross the low word
    _same_batch(eager.collect(), graph.collect(), "counter")
    _same_state(eager, graph, "counter")
    assert graph.counter == 2**32 - 2 + graph.horizon


def test_deterministic_fragments_and_the_stream_after_them(dev):
    eager, graph = _twins(dev, "bf16")
    a, b = eager.collect(deterministic=True), graph.collect(deterministic=True)
    _same_batch(a, b, "deterministic")
    assert torch.equal(b["actions"], b["logits"][..., :3])
    _same_batch(eager.collect(), graph.collect(), "sampled after deterministic")
    _same_batch(eager.collect(deterministic=True), graph.collect(deterministic=True), "deterministic again")
    _same_state(eager, graph, "modes")
    assert graph.captures == 2  # one graph per mode


def test_weights_loaded_in_place_need_no_recapture(dev):
    eager, graph = _twins(dev, "bf16")
    _same_batch(eager.collect(), graph.collect(), "first")
    old = graph.collect()["logits"].clone()
    eager.collect()
    a = _actor_arrays(9)
    graph.policy.load_layers([(a[0], a[1]), (a[2], a[3]), (a[4], a[5])])  # the twins share the policy
    ea, gr = eager.collect(), graph.collect()
    _same_batch(ea, gr, "after load_layers")
    assert graph.captures == 1
    direct = graph.policy.logits(gr["obs"][0])
    assert torch.equal(_i32(direct), _i32(gr["logits"][0])) and not torch.equal(old[0], gr["logits"][0])


def test_a_learner_update_needs_no_recapture(dev):
    """The twins share the policy and the critic; one PPOLearner.update on each twin's fragment
    rewrites both networks in place, and the next fragments agree without a new capture."""
    from swarm_marl_amd import PPOLearner
    eager, graph = _twins(dev, "bf16")
    learner = PPOLearner(eager.policy, eager.critic, lr=3e-3, num_epochs=1, minibatch_env_rows=10)
    ea, gr = eager.collect(), graph.collect()
    _same_batch(ea, gr, "before")
    w0 = graph.policy.weights.clone()
    learner.update(ea)
    learner.update(gr)
    assert not torch.equal(w0, graph.policy.weights)
    _same_batch(eager.collect(), graph.collect(), "after the updates")
    _same_state(eager, graph, "after the updates")
    assert graph.captures == 1


def test_a_moved_buffer_is_recaptured(dev):
    eager, graph = _twins(dev, "bf16")
    _same_batch(eager.collect(), graph.collect(), "first")
    for col in (eager, graph):  # per-env records appear: the step's arguments change
        col.vec.set_env_config(max_steps=3)
    _same_batch(eager.collect(), graph.collect(), "after set_env_config")
    _same_state(eager, graph, "after set_env_config")
    assert graph.captures == 2


def test_replays_do_not_allocate(dev):
    _, graph = _twins(dev, "perturb")
    graph.collect()
    graph.collect(deterministic=True)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    for i in range(5):
        graph.collect(deterministic=i == 2)
        assert torch.cuda.memory_allocated(dev) == before
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(dev) == before and graph.captures == 2


def test_graph_mode_refusals(dev):
    import yaml

    from swarm_marl_amd import RolloutCollector, VecSwarm
    from swarm_marl_amd.domain_randomization import DomainRandomizer
    pol = _mlp_actor(dev, "bf16")
    vec = VecSwarm(4, dict(num_drones=3), device=dev, seed=1)
    dr = DomainRandomizer(vec, yaml.safe_load(DR_PATH.read_text()), seed=1, force=True)
    with pytest.raises(ValueError, match="randomizer"):
        RolloutCollector(vec, pol, None, horizon=2, randomizer=dr, graph=True)
    RolloutCollector(vec, pol, None, horizon=2, randomizer=dr)  # eager takes it
    with pytest.raises(ValueError, match="group"):
        RolloutCollector(VecSwarm(4, dict(num_drones=3), device=dev, groups=2), pol, None, horizon=2, graph=True)
    with pytest.raises(ValueError, match="packed_io"):
        RolloutCollector(VecSwarm(1, dict(num_drones=3), device=dev, packed_io=True), pol, None, horizon=2, graph=True)
