"""GPU: the rollout half — swarm_gaussian_logp, swarm_gae and RolloutCollector end to end.

* gaussian_logp against float64 NumPy: |err| <= 1e-4 + 1e-5 |logp| (the project's f32 logit bound;
  expf differs from NumPy's exp by ulps and z^2 amplifies that), log_std in [-2, 0.5], |z| <= 5.
* gae bitwise equal to the f32 NumPy loop of include/swarm_mi355x.h (tests/critic_ref.py).
* RolloutCollector: fragments of T = 12 steps with max_steps = 5 and goal_radius = 6, under which
  every fragment holds per-agent terminations, truncations, env resets and valid == 0 agent-steps
  (asserted: a fragment without them would prove nothing).  A second VecSwarm with the same seed,
  stepped with the recorded actions, reproduces the record bitwise; logp / values / advantages are
  checked against the host references fed the device's own record.  With the f32 critic at
  (E, N) = (33, 4) and (5, 64); with the bf16 critic at (9, 16) and (17, 8) (an even number of W1
  chunks), values against the emulation of its blob; and on an env with neighbor_k = 0 and
  sensed_obstacles = 0 (obs_dim 9, an actor of that width).  In the last three the recorded logits
  are also held to the actor's bf16 emulation at tests/test_gpu_policy.py's 1e-3; measured on an
  MI355X: 4.6e-4, 4.2e-4 and 9.537e-4 (D = 9: 3 of 1584 rows above 1e-4, median 1.5e-8).  The
  last is one flipped bf16 activation, found from the emulation alone: in the worst row a layer-2
  sum of 2.07031262 lies 1.2e-7 (half an f32 ulp) above the bf16 tie 2.0703125, its ulp 2^-6 times
  its last-layer weight -0.061035 is 9.5367e-4, the error.  Env observations reach +-12, so hidden
  activations are larger than on the unit-scale inputs of test_gpu_policy_dims.py; a flip at an
  activation >= 4 with a weight near 1/16 would exceed 1e-3, none occurs in these fragments.
* Log-prob and GAE launches of 1.5 x one pass of their capped grids (32 blocks of 256 threads per
  CU) + 77 rows / (env, agent) pairs, action dims 1, 2, 3, 6, discounts with gamma or lam at 0 or 1,
  and fragments whose invalid steps hold NaN rewards.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import critic_ref as cr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _check_logp(dev, rows, adim):
    from swarm_marl_amd import gaussian_logp
    rng = np.random.default_rng(rows if adim == 3 else (rows, adim))
    mean = rng.uniform(-1, 1, (rows, adim)).astype(np.float32)
    ls = rng.uniform(-2, 0.5, (rows, adim)).astype(np.float32)
    z = rng.uniform(-5, 5, (rows, adim)).astype(np.float32)
    logits = np.concatenate([mean, ls], axis=1)
    actions = (mean + np.exp(ls) * z).astype(np.float32)
    keep = torch.full((rows + 64,), 5.0, dtype=torch.float32, device=dev)
    got = gaussian_logp(torch.from_numpy(logits).to(dev), torch.from_numpy(actions).to(dev), out=keep[:rows])
    got = got.cpu().numpy()
    assert torch.all(keep[rows:] == 5.0)
    want = cr.logp64(logits, actions)
    err = np.abs(got - want)
    print(f"logp rows={rows} adim={adim} max err {err.max():.3e}")
    assert np.all(err <= 1e-4 + 1e-5 * np.abs(want)), err.max()


@pytest.mark.parametrize("rows", [1, 63, 1000])
def test_gaussian_logp_vs_float64(dev, rows):
    _check_logp(dev, rows, 3)


@pytest.mark.parametrize("rows", [1, 63, 1000])
@pytest.mark.parametrize("adim", [1, 2, 6])
def test_gaussian_logp_other_action_dims(dev, adim, rows):
    _check_logp(dev, rows, adim)


def _one_pass_threads(dev) -> int:
    """Threads of one pass of the log-prob / GAE grid: 32 blocks of 256 per CU (the cap of their
    grid_for calls in csrc/swarm_critic.hip and gae_launch, csrc/swarm_nn.h, mirrored here)."""
    return torch.cuda.get_device_properties(dev).multi_processor_count * 32 * 256


def test_gaussian_logp_more_rows_than_one_pass(dev):
    """1.5 x the rows one pass of the capped grid holds, + 77: half of the threads take a second
    row, the tail none; every row against float64."""
    _check_logp(dev, _one_pass_threads(dev) * 3 // 2 + 77, 3)


@pytest.mark.parametrize("shape", [(1, 1, 1), (7, 33, 4), (16, 5, 64)])
def test_gae_bitwise_vs_numpy_f32(dev, shape):
    from swarm_marl_amd import gae
    args = cr.random_gae_inputs(*shape, seed=sum(shape))
    reward, value, terminated, truncated, env_done, valid = args
    assert (~valid).any() or shape == (1, 1, 1)
    dv = [torch.from_numpy(a).to(dev) for a in args]
    adv, tgt = gae(*dv, gamma=0.99, lam=0.95)
    a_ref, t_ref = cr.gae_loop(*args, 0.99, 0.95, dtype=np.float32)
    assert np.array_equal(adv.cpu().numpy().view(np.uint32), a_ref.view(np.uint32))
    assert np.array_equal(tgt.cpu().numpy().view(np.uint32), t_ref.view(np.uint32))
    # uint8 flags are the same call
    adv8, _ = gae(dv[0], dv[1], dv[2].view(torch.uint8), dv[3].view(torch.uint8), dv[4], dv[5].view(torch.uint8),
                  gamma=0.99, lam=0.95)
    assert torch.equal(adv8, adv)
    with pytest.raises(ValueError):
        gae(dv[0], dv[1][:-1].contiguous(), *dv[2:], gamma=0.99, lam=0.95)


def _check_gae_bitwise(dev, args, gamma, lam):
    from swarm_marl_amd import gae
    adv, tgt = gae(*[torch.from_numpy(a).to(dev) for a in args], gamma=gamma, lam=lam)
    a_ref, t_ref = cr.gae_loop(*args, gamma, lam, dtype=np.float32)
    assert np.array_equal(adv.cpu().numpy().view(np.uint32), a_ref.view(np.uint32))
    assert np.array_equal(tgt.cpu().numpy().view(np.uint32), t_ref.view(np.uint32))
    return a_ref, t_ref


@pytest.mark.parametrize("shape", [(1, 300, 1), (3, 2, 256), (7, 33, 4)])
@pytest.mark.parametrize("gamma,lam", [(1.0, 1.0), (0.9, 0.0), (0.0, 0.95)])
def test_gae_bitwise_other_discounts_and_shapes(dev, gamma, lam, shape):
    """No discount at all, no carry (lam = 0: the advantage is the one-step delta) and no bootstrap
    (gamma = 0); one step of many envs, and one env per 256-thread block."""
    args = cr.random_gae_inputs(*shape, seed=sum(shape) + 1)
    a_ref, _ = _check_gae_bitwise(dev, args, gamma, lam)
    assert np.abs(a_ref).max() > 0.1


def test_gae_all_invalid_fragment_is_zero_and_ignores_nan_rewards(dev):
    """gae_kernel reads only `valid` of an invalid step (it writes both zeros and clears the carry
    before it touches reward or value), so a NaN reward there is legitimate input: both outputs are
    exactly +0."""
    from swarm_marl_amd import gae
    reward, value, terminated, truncated, env_done, valid = cr.random_gae_inputs(6, 9, 5, seed=4)
    valid[:] = False
    reward[:] = np.nan
    args = (reward, value, terminated, truncated, env_done, valid)
    adv, tgt = gae(*[torch.from_numpy(a).to(dev) for a in args], gamma=0.99, lam=0.95)
    assert np.all(adv.cpu().numpy().view(np.uint32) == 0) and np.all(tgt.cpu().numpy().view(np.uint32) == 0)
    # and a fragment where only some envs are wholly invalid, NaN rewards on every invalid step
    reward, value, terminated, truncated, env_done, valid = cr.random_gae_inputs(6, 9, 5, seed=5)
    valid[:, 2] = False
    valid[:, 7] = False
    reward[~valid] = np.nan
    args = (reward, value, terminated, truncated, env_done, valid)
    a_ref, t_ref = _check_gae_bitwise(dev, args, 0.99, 0.95)
    assert np.all(a_ref[:, 2] == 0) and np.all(t_ref[:, 7] == 0) and np.isfinite(a_ref).all() and np.isfinite(t_ref).all()


def test_gae_more_agents_than_one_pass(dev):
    """E x N of at least 1.5 x the (env, agent) pairs one pass of the capped grid holds, + 77, at
    N = 3 (E rounded up to a whole env) and T = 3: half of the threads walk a second pair."""
    n, t = 3, 3
    e = (_one_pass_threads(dev) * 3 // 2 + 77 + n - 1) // n
    _check_gae_bitwise(dev, cr.random_gae_inputs(t, e, n, seed=12), 0.99, 0.95)


CFG = dict(max_steps=5, goal_radius=6.0)
T = 12


def _actor(dev, in_dim=37):
    from swarm_marl_amd.policy import PolicyMLP
    rng = np.random.default_rng(5)
    w = [rng.uniform(-1, 1, s).astype(np.float32) / np.float32(np.sqrt(s[-1]))
         for s in ((256, in_dim), (256,), (256, 256), (256,), (6, 256), (6,))]
    return PolicyMLP.from_arrays(*w, device=dev, precision="bf16")


def _collector(dev, e, n, seed=3, critic=True, precision="f32", cfg=CFG):
    from swarm_marl_amd import CriticMLP, RolloutCollector, VecSwarm
    vec = VecSwarm(e, dict(cfg, num_drones=n), device=dev, auto_reset=True, seed=11, with_global_state=True)
    vec.reset()
    layers = cr.make_critic(6 * n + 3, seed=2)
    c = CriticMLP(layers, device=dev, precision=precision) if critic else None
    return RolloutCollector(vec, _actor(dev, vec.obs_dim), c, horizon=T, gamma=0.99, lam=0.95, seed=seed), layers


def _host(batch):
    return {k: v.cpu().numpy().copy() for k, v in batch.items() if v is not None}


def _check_collector(dev, e, n, precision="f32", cfg=CFG, check_logits=False):
    from swarm_marl_amd import VecSwarm
    from swarm_marl_amd import _native as nat
    col, layers = _collector(dev, e, n, precision=precision, cfg=cfg)
    b = _host(col.collect())
    g, d = 6 * n + 3, col.vec.obs_dim
    assert b["obs"].shape == (T, e, n, d) and b["logits"].shape == (T, e, n, 6) and b["actions"].shape == (T, e, n, 3)
    assert b["global_state"].shape == (T + 1, e, g) and b["value"].shape == (T + 1, e) and b["env_done"].shape == (T, e)
    for k in ("logp", "reward", "terminated", "truncated", "valid", "advantage", "value_target"):
        assert b[k].shape == (T, e, n), k
    # ---- the fragment holds every kind of episode event
    assert (b["terminated"] & b["valid"]).any(), "no per-agent termination"
    assert b["truncated"].any(), "no truncation"
    assert (b["env_done"] & nat.ENV_RESET).any(), "no env reset"
    assert (~b["valid"]).any(), "no valid == 0 agent-step"
    # ---- replay: a second env with the same seed, stepped with the recorded actions
    vec2 = VecSwarm(e, dict(cfg, num_drones=n), device=dev, auto_reset=True, seed=11, with_global_state=True)
    vec2.reset()
    for t in range(T):
        assert np.array_equal(vec2.active.cpu().numpy(), b["valid"][t]), t
        assert np.array_equal(vec2.obs.cpu().numpy().view(np.uint32), b["obs"][t].view(np.uint32)), t
        assert np.array_equal(vec2.global_state.cpu().numpy().view(np.uint32), b["global_state"][t].view(np.uint32)), t
        _, rew, term, trunc, done = vec2.step(torch.from_numpy(b["actions"][t]).to(dev))
        assert np.array_equal(rew.cpu().numpy().view(np.uint32), b["reward"][t].view(np.uint32)), t
        assert np.array_equal(term.cpu().numpy(), b["terminated"][t]) and np.array_equal(trunc.cpu().numpy(), b["truncated"][t])
        assert np.array_equal(done.cpu().numpy(), b["env_done"][t]), t
    assert np.array_equal(vec2.global_state.cpu().numpy().view(np.uint32), b["global_state"][T].view(np.uint32))
    # ---- logp from the recorded logits and actions (float64)
    want = cr.logp64(b["logits"], b["actions"])
    err = np.abs(b["logp"] - want)
    print(f"collector E={e} N={n}: logp max err {err.max():.3e}")
    assert np.all(err <= 1e-4 + 1e-5 * np.abs(want)), err.max()
    assert not np.array_equal(b["actions"], b["logits"][..., :3])  # sampled, not the mean
    # ---- the actor's logits: the bf16 emulation on the recorded observations (tests/test_gpu_policy.py's bound)
    if check_logits:
        from tests.test_policy_cpu import emulate_bf16_kernel
        lemu = emulate_bf16_kernel(col.policy.packed_host, b["obs"].reshape(-1, d), 6).reshape(T, e, n, 6)
        lerr = np.abs(b["logits"] - lemu).max()
        print(f"collector E={e} N={n} D={d}: logits vs emulation {lerr:.3e}")
        assert lerr <= 1e-3, lerr
    # ---- values on the recorded global states: the f32 critic bound against float64, the bf16
    # critic against the emulation of its blob (tests/test_gpu_critic.py BF16_EMU_BOUND)
    if precision == "f32":
        v64 = cr.truth64(layers, b["global_state"].reshape(-1, g)).reshape(T + 1, e)
        verr = np.abs(b["value"] - v64)
        print(f"collector E={e} N={n}: value max err {verr.max():.3e}")
        assert np.all(verr <= 1e-5 + 1e-5 * np.abs(v64)), verr.max()
    else:
        from tests.test_gpu_critic import BF16_EMU_BOUND
        vemu = cr.emulate_bf16_blob(col.critic.packed_host, b["global_state"].reshape(-1, g)).reshape(T + 1, e)
        verr = np.abs(b["value"] - vemu).max()
        print(f"collector E={e} N={n}: bf16 value vs emulation {verr:.3e}")
        assert verr <= BF16_EMU_BOUND, verr
    # ---- advantages and targets: bitwise the NumPy f32 loop fed the device's own values
    a_ref, t_ref = cr.gae_loop(b["reward"], b["value"], b["terminated"], b["truncated"], b["env_done"], b["valid"],
                               0.99, 0.95, dtype=np.float32)
    assert np.array_equal(b["advantage"].view(np.uint32), a_ref.view(np.uint32))
    assert np.array_equal(b["value_target"].view(np.uint32), t_ref.view(np.uint32))
    assert np.all(b["advantage"][~b["valid"]] == 0)
    # ---- an equal-seed collector gives the same batch bit for bit; a second collect() fresh noise
    col2, _ = _collector(dev, e, n, precision=precision, cfg=cfg)
    b2 = _host(col2.collect())
    for k in b:
        assert np.array_equal(b[k].view(np.uint8), b2[k].view(np.uint8)), k
    b3 = _host(col.collect())
    assert col.counter == 2 * T
    assert not np.array_equal(b3["actions"], b["actions"])
    noise = lambda x: (x["actions"] - x["logits"][..., :3]) * np.exp(-x["logits"][..., 3:])  # noqa: E731
    assert np.abs(noise(b3) - noise(b)).max() > 0.1  # the standard normals themselves differ
    col3, _ = _collector(dev, e, n, seed=4, precision=precision, cfg=cfg)
    assert not np.array_equal(_host(col3.collect())["actions"][0], b["actions"][0])


@pytest.mark.parametrize("e,n", [(33, 4), (5, 64)])
def test_collector_end_to_end(dev, e, n):
    _check_collector(dev, e, n)


@pytest.mark.parametrize("e,n", [(9, 16), (17, 8)])
def test_collector_end_to_end_bf16_critic(dev, e, n):
    """The bf16 critic inside the collector, at the two widths with an even number of W1 chunks
    (N = 16: in_dim 99, 4 chunks; N = 8: in_dim 51, 2 chunks)."""
    _check_collector(dev, e, n, precision="bf16", check_logits=True)


def test_collector_end_to_end_smallest_observation(dev):
    """neighbor_k = 0 and sensed_obstacles = 0: obs_dim = 9, an actor of that width (the bf16
    kernel's runtime-dims instance), replayed and checked like the default."""
    from swarm_marl_amd import VecSwarm
    cfg = dict(CFG, neighbor_k=0, sensed_obstacles=0)
    assert VecSwarm(2, dict(cfg, num_drones=4), device=dev).obs_dim == 9
    _check_collector(dev, 33, 4, cfg=cfg, check_logits=True)


def test_collector_without_critic_and_deterministic(dev):
    from swarm_marl_amd import RolloutCollector, VecSwarm
    col, _ = _collector(dev, 33, 4, critic=False)
    b = _host(col.collect(deterministic=True))
    assert np.all(b["value"] == 0)
    assert np.array_equal(b["actions"], b["logits"][..., :3])
    want = -b["logits"][..., 3:].astype(np.float64).sum(-1) - 1.5 * np.log(2 * np.pi)  # the density at the mean
    assert np.all(np.abs(b["logp"] - want) <= 1e-4 + 1e-5 * np.abs(want))
    # zero values: the advantages are the rewards-to-go discounted by gamma * lam, cut at episode ends
    a_ref, t_ref = cr.gae_loop(b["reward"], np.zeros_like(b["value"]), b["terminated"], b["truncated"], b["env_done"],
                               b["valid"], 0.99, 0.95, dtype=np.float32)
    assert np.array_equal(b["advantage"].view(np.uint32), a_ref.view(np.uint32))
    assert np.array_equal(b["value_target"], b["advantage"])
    # a critic needs the env's global_state
    from swarm_marl_amd import CriticMLP
    vec = VecSwarm(4, dict(CFG, num_drones=4), device=dev, seed=1)
    with pytest.raises(ValueError, match="with_global_state"):
        RolloutCollector(vec, _actor(dev), CriticMLP(cr.make_critic(27), device=dev), horizon=4)
