"""GPU: the per-agent critic in the rollout and the learner — swarm_gae_agent, RolloutCollector and
PPOLearner with an AgentValueMLP.

* gae_agent bitwise equal to the f32 NumPy loop of include/swarm_mi355x.h (tests/value_ref.py) on
  episode-consistent flags, at two (gamma, lam) pairs, and over 1.5 x one pass of its capped grid
  (32 blocks of 256 threads per CU) + 77 (env, agent) pairs; with value[t, e, n] = v[t, e] bitwise
  the output of swarm_gae; and with NaN in every value the loop must not read (an invalid step's, and
  row T behind an invalid or done last step) finite and bitwise unchanged.
* RolloutCollector: fragments of T = 12 steps with max_steps = 5 and goal_radius = 6 (per-agent
  terminations, truncations, env resets and valid == 0 agent-steps in every fragment, asserted), with
  and without the env's global_state.  A second VecSwarm with the same seed, stepped with the
  recorded actions, reproduces the record bitwise, row T of the observation block included; values
  on the recorded observations are held to tests/test_gpu_value.py's bounds (f32: against float64;
  bf16: against the emulation of the blob, and 2 m against float64); advantages and targets are
  bitwise the NumPy loop fed the device's own values.
* PPOLearner: lr = 0 leaves the weights alone and reports tests/ppo_ref.py's loss (1e-5 relative) fed
  the learner's own float64-cast forwards with one value per agent row; training lowers the loss
  and pushes the value tower's weights; a collect, update, collect loop with the bf16 actor and the
  bf16 value stays finite.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import critic_ref as cr
from tests import ppo_ref as pr
from tests import value_ref as vr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run_gae_agent(dev, args, gamma, lam):
    from swarm_marl_amd import gae_agent
    adv, tgt = gae_agent(*[torch.from_numpy(a).to(dev) for a in args], gamma=gamma, lam=lam)
    return adv.cpu().numpy(), tgt.cpu().numpy()


def _check_gae_agent_bitwise(dev, args, gamma, lam):
    adv, tgt = _run_gae_agent(dev, args, gamma, lam)
    a_ref, t_ref = vr.gae_agent_loop(*args, gamma, lam, dtype=np.float32)
    assert np.array_equal(_bits(adv), _bits(a_ref)) and np.array_equal(_bits(tgt), _bits(t_ref))
    return a_ref, t_ref


@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (0.9, 0.0)])
@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 3, 5), (7, 70, 5), (4, 5, 64)])
def test_gae_agent_bitwise_vs_numpy_f32(dev, shape, gamma, lam):
    from swarm_marl_amd import gae_agent
    args = vr.random_gae_agent_inputs(*shape, seed=sum(shape))
    vr.check_consistent(*args[2:])
    a_ref, _ = _check_gae_agent_bitwise(dev, args, gamma, lam)
    if shape != (1, 1, 1):
        assert (~args[5]).any() and np.abs(a_ref).max() > 0.1
    dv = [torch.from_numpy(a).to(dev) for a in args]
    with pytest.raises(ValueError):  # a per-env value is another entry point's
        gae_agent(dv[0], dv[1][:, :, 0].contiguous(), *dv[2:], gamma=gamma, lam=lam)


def _one_pass_threads(dev) -> int:
    """Threads of one pass of the GAE grid: 32 blocks of 256 per CU (the cap of swarm_gae_agent's
    grid_for call, gae_launch in csrc/swarm_nn.h, mirrored here)."""
    return torch.cuda.get_device_properties(dev).multi_processor_count * 32 * 256


def test_gae_agent_more_agents_than_one_pass(dev):
    """E x N of at least 1.5 x the (env, agent) pairs one pass of the capped grid holds, + 77, at
    N = 3 (E rounded up to a whole env) and T = 3: half of the threads walk a second pair."""
    n, t = 3, 3
    e = (_one_pass_threads(dev) * 3 // 2 + 77 + n - 1) // n
    _check_gae_agent_bitwise(dev, vr.random_gae_agent_inputs(t, e, n, seed=12), 0.99, 0.95)


@pytest.mark.parametrize("shape", [(7, 33, 4), (16, 5, 64)])
def test_gae_agent_on_broadcast_values_is_swarm_gae(dev, shape):
    from swarm_marl_amd import gae
    args = cr.random_gae_inputs(*shape, seed=sum(shape))
    reward, value, terminated, truncated, env_done, valid = args
    wide = np.ascontiguousarray(np.broadcast_to(value[:, :, None], (shape[0] + 1,) + shape[1:]))
    adv, tgt = _run_gae_agent(dev, (reward, wide, terminated, truncated, env_done, valid), 0.99, 0.95)
    a_env, t_env = gae(*[torch.from_numpy(a).to(dev) for a in args], gamma=0.99, lam=0.95)
    assert np.array_equal(_bits(adv), _bits(a_env.cpu().numpy())) and np.array_equal(_bits(tgt), _bits(t_env.cpu().numpy()))


@pytest.mark.parametrize("shape", [(5, 3, 5), (7, 70, 5)])
def test_gae_agent_never_reads_the_values_it_must_not(dev, shape):
    """NaN in value[t, e, n] of every invalid step and in value[T, e, n] behind an invalid or done
    last step: the outputs are finite, zero on invalid steps and bitwise those of the clean values."""
    args = vr.random_gae_agent_inputs(*shape, seed=sum(shape) + 3)
    reward, value, terminated, truncated, env_done, valid = args
    poisoned = vr.poison_unread_values(value, terminated, truncated, env_done, valid)
    assert np.isnan(poisoned[:-1]).any() and np.isnan(poisoned[-1]).any()
    a_ref, t_ref = vr.gae_agent_loop(*args, 0.99, 0.95, dtype=np.float32)
    adv, tgt = _run_gae_agent(dev, (reward, poisoned, terminated, truncated, env_done, valid), 0.99, 0.95)
    assert np.isfinite(adv).all() and np.isfinite(tgt).all()
    assert np.array_equal(_bits(adv), _bits(a_ref)) and np.array_equal(_bits(tgt), _bits(t_ref))
    assert np.all(_bits(adv)[~valid] == 0) and np.all(_bits(tgt)[~valid] == 0)


# ---------------------------------------------------------------- the collector
CFG = dict(max_steps=5, goal_radius=6.0)
T = 12


def _arrays(shapes, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1, 1, s).astype(np.float32) / np.float32(np.sqrt(s[-1])) for s in shapes]


def _actor(dev, in_dim=37, precision="bf16"):
    from swarm_marl_amd.policy import PolicyMLP
    return PolicyMLP.from_arrays(*_arrays(((256, in_dim), (256,), (256, 256), (256,), (6, 256), (6,)), 5), device=dev,
                                 precision=precision)


def _collector(dev, e, n, precision, with_gs, seed=3):
    from swarm_marl_amd import AgentValueMLP, RolloutCollector, VecSwarm
    vec = VecSwarm(e, dict(CFG, num_drones=n), device=dev, auto_reset=True, seed=11, with_global_state=with_gs)
    vec.reset()
    layers = vr.make_value(vec.obs_dim, seed=2)
    value = AgentValueMLP(layers, device=dev, precision=precision)
    return RolloutCollector(vec, _actor(dev, vec.obs_dim), value, horizon=T, gamma=0.99, lam=0.95, seed=seed), layers


def _host(batch):
    return {k: v.cpu().numpy().copy() for k, v in batch.items() if v is not None}


@pytest.mark.parametrize("e,n,precision,with_gs", [(33, 4, "f32", False), (5, 64, "bf16", True), (33, 4, "bf16", False),
                                                   (5, 64, "f32", True)])
def test_collector_end_to_end(dev, e, n, precision, with_gs):
    from swarm_marl_amd import VecSwarm
    from swarm_marl_amd import _native as nat
    col, layers = _collector(dev, e, n, precision, with_gs)
    batch = col.collect()
    b = _host(batch)
    d = col.vec.obs_dim
    assert b["obs"].shape == (T, e, n, d) and b["value"].shape == (T + 1, e, n) and b["env_done"].shape == (T, e)
    assert tuple(col.obs_block.shape) == (T + 1, e, n, d) and batch["obs"].data_ptr() == col.obs_block.data_ptr()
    assert ("global_state" in b) == with_gs and (not with_gs or b["global_state"].shape == (T + 1, e, 6 * n + 3))
    for k in ("logp", "reward", "terminated", "truncated", "valid", "advantage", "value_target"):
        assert b[k].shape == (T, e, n), k
    # ---- the fragment holds every kind of episode event
    assert (b["terminated"] & b["valid"]).any(), "no per-agent termination"
    assert b["truncated"].any(), "no truncation"
    assert (b["env_done"] & nat.ENV_RESET).any(), "no env reset"
    assert (~b["valid"]).any(), "no valid == 0 agent-step"
    # ---- replay: a second env with the same seed, stepped with the recorded actions
    vec2 = VecSwarm(e, dict(CFG, num_drones=n), device=dev, auto_reset=True, seed=11, with_global_state=with_gs)
    vec2.reset()
    for t in range(T):
        assert np.array_equal(vec2.active.cpu().numpy(), b["valid"][t]), t
        assert np.array_equal(_bits(vec2.obs.cpu().numpy()), _bits(b["obs"][t])), t
        _, rew, term, trunc, done = vec2.step(torch.from_numpy(b["actions"][t]).to(dev))
        assert np.array_equal(_bits(rew.cpu().numpy()), _bits(b["reward"][t])), t
        assert np.array_equal(term.cpu().numpy(), b["terminated"][t]) and np.array_equal(trunc.cpu().numpy(), b["truncated"][t])
        assert np.array_equal(done.cpu().numpy(), b["env_done"][t]), t
    block = col.obs_block.cpu().numpy()
    assert np.array_equal(_bits(block[:T]), _bits(b["obs"]))
    assert np.array_equal(_bits(vec2.obs.cpu().numpy()), _bits(block[T]))  # row T: the obs after the last step
    # ---- values on the recorded observations, tests/test_gpu_value.py's bounds
    rows = block.reshape(-1, d)
    v64 = vr.truth64(layers, rows).reshape(T + 1, e, n)
    if precision == "f32":
        verr = np.abs(b["value"] - v64)
        print(f"collector E={e} N={n}: f32 value max err {verr.max():.3e}")
        assert np.all(verr <= 1e-5 + 1e-5 * np.abs(v64)), verr.max()
    else:
        from tests.test_gpu_value import BF16_EMU_BOUND
        vemu = vr.emulate_bf16_blob(col.critic.packed_host, rows).reshape(T + 1, e, n)
        m = np.abs(vemu - v64).max()
        e_emu, e_64 = np.abs(b["value"] - vemu).max(), np.abs(b["value"] - v64).max()
        print(f"collector E={e} N={n}: bf16 value vs emulation {e_emu:.3e}  vs float64 {e_64:.3e}  m {m:.3e}")
        assert e_emu <= BF16_EMU_BOUND, e_emu
        assert e_64 <= 2 * m, (e_64, m)
    # ---- advantages and targets: bitwise the NumPy f32 loop fed the device's own values
    a_ref, t_ref = vr.gae_agent_loop(b["reward"], b["value"], b["terminated"], b["truncated"], b["env_done"], b["valid"],
                                     0.99, 0.95, dtype=np.float32)
    assert np.array_equal(_bits(b["advantage"]), _bits(a_ref)) and np.array_equal(_bits(b["value_target"]), _bits(t_ref))
    assert np.all(b["advantage"][~b["valid"]] == 0)
    assert np.abs(b["value"]).max() > 0 and b["value"].std(axis=2).max() > 0  # per agent, not per env
    # ---- an equal-seed collector gives the same batch bit for bit
    col2, _ = _collector(dev, e, n, precision, with_gs)
    b2 = _host(col2.collect())
    for k in b:
        assert np.array_equal(b[k].view(np.uint8), b2[k].view(np.uint8)), k
    assert np.array_equal(col2.obs_block.cpu().numpy().view(np.uint8), block.view(np.uint8))


def test_collector_checks_the_value_width(dev):
    from swarm_marl_amd import AgentValueMLP, RolloutCollector, VecSwarm
    vec = VecSwarm(4, dict(CFG, num_drones=4), device=dev, seed=1)
    with pytest.raises(ValueError, match="per-agent critic"):
        RolloutCollector(vec, _actor(dev), AgentValueMLP(vr.make_value(25), device=dev), horizon=4)


# ---------------------------------------------------------------- the learner
LT, LE, LN = 8, 32, 4


def _setup(dev, precision="f32", value_precision="f32", with_gs=False, **learner_kw):
    from swarm_marl_amd import AgentValueMLP, PPOLearner, RolloutCollector, VecSwarm
    vec = VecSwarm(LE, dict(CFG, num_drones=LN), device=dev, auto_reset=True, seed=11, with_global_state=with_gs)
    vec.reset()
    policy = _actor(dev, 37, precision)
    value = AgentValueMLP(vr.make_value(37, seed=2), device=dev, precision=value_precision)
    col = RolloutCollector(vec, policy, value, horizon=LT, seed=3)
    return col, PPOLearner(policy, value, **learner_kw), policy, value


def test_learner_lr0_changes_nothing_and_reports_the_reference(dev):
    col, learner, policy, value = _setup(dev, lr=0.0, num_epochs=1, minibatch_env_rows=LT * LE, entropy_coeff=0.01)
    batch = col.collect(deterministic=True)  # the f32 actor kernel has no sampling path: it acts with the mean
    assert batch["global_state"] is None and not batch["valid"].all() and batch["valid"].any()
    pw, vw, ptr = policy.weights.clone(), value.weights.clone(), value.weights.data_ptr()
    info = learner.update(batch)
    assert torch.equal(policy.weights, pw) and torch.equal(value.weights, vw) and value.weights.data_ptr() == ptr
    assert all(np.isfinite(info[k]) for k in pr.STATS) and info["epoch_total_loss"] == [info["total_loss"]]
    b = {k: v.cpu() for k, v in batch.items() if v is not None}
    rows = LT * LE * LN
    with torch.no_grad():
        logits = learner.actor(batch["obs"].reshape(rows, 37)).double().cpu()
        val = learner.value_net(batch["obs"].reshape(rows, 37)).double().cpu().view(rows)  # one value per agent row
    mom = pr.moments(b["advantage"].numpy(), b["valid"].numpy())
    f = lambda k, *s: b[k].reshape(rows, *s).double()  # noqa: E731
    _, ref, _, _ = pr.loss(logits, val, f("logits", 6), f("actions", 3), f("logp"), f("advantage"), f("value_target"),
                           b["valid"].reshape(-1), float(mom[1]), float(mom[3]), **dict(pr.COEF, entropy_coeff=0.01))
    for k in pr.STATS:
        err = abs(info[k] - float(ref[k])) / max(1.0, abs(float(ref[k])))
        print(f"per-agent learner lr=0 {k}: {info[k]:.6g} vs {float(ref[k]):.6g} rel err {err:.2e}")
        assert err <= 1e-5, k
    assert info["count"] == int(b["valid"].sum())


def test_learner_trains_and_pushes_the_value_weights(dev):
    col, learner, policy, value = _setup(dev, lr=3e-4, num_epochs=5, minibatch_env_rows=LT * LE)
    batch = col.collect(deterministic=True)
    obs = batch["obs"].clone()
    before_v, ptr = value.value(obs), value.weights.data_ptr()
    info = learner.update(batch)
    losses = info["epoch_total_loss"]
    print("per-agent learner epoch losses", losses)
    assert len(losses) == 5 and losses[-1] < losses[0]
    with torch.no_grad():
        want_v = learner.value_net(obs.reshape(-1, 37)).reshape(before_v.shape)
    got_v = value.value(obs)
    assert value.weights.data_ptr() == ptr
    assert torch.all((got_v - want_v).abs() <= 1e-4 + 1e-5 * want_v.abs()), (got_v - want_v).abs().max().item()
    assert (got_v - before_v).abs().max().item() > 1e-3


def test_collect_update_collect(dev):
    # the training loop as it runs: the bf16 actor samples, the bf16 value tower scores, the f32 copies train
    col, learner, policy, value = _setup(dev, "bf16", "bf16", with_gs=True, lr=3e-4, num_epochs=2, minibatch_env_rows=100, seed=4)
    info = learner.update(col.collect())  # 256 env-rows: minibatches of 100, 100 and 56
    assert all(np.isfinite(v) for k, v in info.items() if k != "epoch_total_loss") and np.isfinite(info["epoch_total_loss"]).all()
    batch = col.collect()
    for k in ("logits", "value", "advantage", "value_target"):
        assert bool(torch.isfinite(batch[k]).all()), k
    assert tuple(batch["value"].shape) == (LT + 1, LE, LN)
    info2 = learner.update(batch)
    assert all(np.isfinite(info2[k]) for k in pr.STATS)


def test_learner_checks_the_widths(dev):
    from swarm_marl_amd import AgentValueMLP, PPOLearner
    with pytest.raises(ValueError, match="per-agent critic"):
        PPOLearner(_actor(dev, 37), AgentValueMLP(vr.make_value(25), device=dev), minibatch_env_rows=8)
    col, learner, _, _ = _setup(dev, minibatch_env_rows=8)
    batch = dict(col.collect(deterministic=True))
    batch["obs"] = batch["obs"][..., :25].contiguous()
    with pytest.raises(ValueError):
        learner.update(batch)
