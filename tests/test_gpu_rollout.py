"""GPU: the rollout half — swarm_gaussian_logp, swarm_gae and RolloutCollector end to end.

* gaussian_logp against float64 NumPy: |err| <= 1e-4 + 1e-5 |logp| (the project's f32 logit bound;
  expf differs from NumPy's exp by ulps and z^2 amplifies that), log_std in [-2, 0.5], |z| <= 5.
* gae bitwise equal to the f32 NumPy loop of include/swarm_mi355x.h (tests/critic_ref.py).
* RolloutCollector: fragments of T = 12 steps with max_steps = 5 and goal_radius = 6, under which
  every fragment holds per-agent terminations, truncations, env resets and valid == 0 agent-steps
  (asserted: a fragment without them would prove nothing).  A second VecSwarm with the same seed,
  stepped with the recorded actions, reproduces the record bitwise; logp / values / advantages are
  checked against the host references fed the device's own record.
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


@pytest.mark.parametrize("rows", [1, 63, 1000])
def test_gaussian_logp_vs_float64(dev, rows):
    from swarm_marl_amd import gaussian_logp
    rng = np.random.default_rng(rows)
    mean = rng.uniform(-1, 1, (rows, 3)).astype(np.float32)
    ls = rng.uniform(-2, 0.5, (rows, 3)).astype(np.float32)
    z = rng.uniform(-5, 5, (rows, 3)).astype(np.float32)
    logits = np.concatenate([mean, ls], axis=1)
    actions = (mean + np.exp(ls) * z).astype(np.float32)
    keep = torch.full((rows + 64,), 5.0, dtype=torch.float32, device=dev)
    got = gaussian_logp(torch.from_numpy(logits).to(dev), torch.from_numpy(actions).to(dev), out=keep[:rows])
    got = got.cpu().numpy()
    assert torch.all(keep[rows:] == 5.0)
    want = cr.logp64(logits, actions)
    err = np.abs(got - want)
    print(f"logp rows={rows} max err {err.max():.3e}")
    assert np.all(err <= 1e-4 + 1e-5 * np.abs(want)), err.max()


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


CFG = dict(max_steps=5, goal_radius=6.0)
T = 12


def _actor(dev):
    from swarm_marl_amd.policy import PolicyMLP
    rng = np.random.default_rng(5)
    w = [rng.uniform(-1, 1, s).astype(np.float32) / np.float32(np.sqrt(s[-1]))
         for s in ((256, 37), (256,), (256, 256), (256,), (6, 256), (6,))]
    return PolicyMLP.from_arrays(*w, device=dev, precision="bf16")


def _collector(dev, e, n, seed=3, critic=True):
    from swarm_marl_amd import CriticMLP, RolloutCollector, VecSwarm
    vec = VecSwarm(e, dict(CFG, num_drones=n), device=dev, auto_reset=True, seed=11, with_global_state=True)
    vec.reset()
    layers = cr.make_critic(6 * n + 3, seed=2)
    c = CriticMLP(layers, device=dev, precision="f32") if critic else None
    return RolloutCollector(vec, _actor(dev), c, horizon=T, gamma=0.99, lam=0.95, seed=seed), layers


def _host(batch):
    return {k: v.cpu().numpy().copy() for k, v in batch.items() if v is not None}


@pytest.mark.parametrize("e,n", [(33, 4), (5, 64)])
def test_collector_end_to_end(dev, e, n):
    from swarm_marl_amd import VecSwarm
    from swarm_marl_amd import _native as nat
    col, layers = _collector(dev, e, n)
    b = _host(col.collect())
    g = 6 * n + 3
    assert b["obs"].shape == (T, e, n, 37) and b["logits"].shape == (T, e, n, 6) and b["actions"].shape == (T, e, n, 3)
    assert b["global_state"].shape == (T + 1, e, g) and b["value"].shape == (T + 1, e) and b["env_done"].shape == (T, e)
    for k in ("logp", "reward", "terminated", "truncated", "valid", "advantage", "value_target"):
        assert b[k].shape == (T, e, n), k
    # ---- the fragment holds every kind of episode event
    assert (b["terminated"] & b["valid"]).any(), "no per-agent termination"
    assert b["truncated"].any(), "no truncation"
    assert (b["env_done"] & nat.ENV_RESET).any(), "no env reset"
    assert (~b["valid"]).any(), "no valid == 0 agent-step"
    # ---- replay: a second env with the same seed, stepped with the recorded actions
    vec2 = VecSwarm(e, dict(CFG, num_drones=n), device=dev, auto_reset=True, seed=11, with_global_state=True)
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
    # ---- values: the f32 critic bound against float64 on the recorded global states
    v64 = cr.truth64(layers, b["global_state"].reshape(-1, g)).reshape(T + 1, e)
    verr = np.abs(b["value"] - v64)
    print(f"collector E={e} N={n}: value max err {verr.max():.3e}")
    assert np.all(verr <= 1e-5 + 1e-5 * np.abs(v64)), verr.max()
    # ---- advantages and targets: bitwise the NumPy f32 loop fed the device's own values
    a_ref, t_ref = cr.gae_loop(b["reward"], b["value"], b["terminated"], b["truncated"], b["env_done"], b["valid"],
                               0.99, 0.95, dtype=np.float32)
    assert np.array_equal(b["advantage"].view(np.uint32), a_ref.view(np.uint32))
    assert np.array_equal(b["value_target"].view(np.uint32), t_ref.view(np.uint32))
    assert np.all(b["advantage"][~b["valid"]] == 0)
    # ---- an equal-seed collector gives the same batch bit for bit; a second collect() fresh noise
    col2, _ = _collector(dev, e, n)
    b2 = _host(col2.collect())
    for k in b:
        assert np.array_equal(b[k].view(np.uint8), b2[k].view(np.uint8)), k
    b3 = _host(col.collect())
    assert col.counter == 2 * T
    assert not np.array_equal(b3["actions"], b["actions"])
    noise = lambda x: (x["actions"] - x["logits"][..., :3]) * np.exp(-x["logits"][..., 3:])  # noqa: E731
    assert np.abs(noise(b3) - noise(b)).max() > 0.1  # the standard normals themselves differ
    col3, _ = _collector(dev, e, n, seed=4)
    assert not np.array_equal(_host(col3.collect())["actions"][0], b["actions"][0])


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
