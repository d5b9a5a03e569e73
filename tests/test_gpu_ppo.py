"""GPU: the PPO loss head (swarm_masked_moments, swarm_ppo_loss through `masked_moments` / `ppo_loss`)
and `PPOLearner`.

* Moments against NumPy float64: count exact, mean / std / inverse std within 1e-12 max(1, |ref|);
  bitwise repeatable; invalid elements may hold NaN.
* The head against the float64 CPU reference (tests/ppo_ref.py: autograd gradients of an
  independently written loss): grad_logits and grad_value within 2e-5 (|ref| + max|ref|), stats
  within 1e-5 max(1, |ref|) — an f32 log-prob of magnitude <= 20 carries ~2e-6 absolute, so ~2e-6
  relative on the ratio, and the rest is a handful of f32 operations; the valid count and the
  number of clipped rows are exact.  Every case asserts, on the reference, that no valid row has
  |r - (1 +- c)| < 1e-3 or |(v - R)^2 - vf_clip| < 1e-3, so no row is left out.  Seeds alone cannot
  give that at 16,640 rows (about 4e-3 of the rows fall in the ratio band): ppo_ref.make_case moves
  the rows it draws into a band off it, deterministically, before either side sees them.
* Masking: NaN / inf in every input of every invalid row changes no output bit; repeat launches
  are bitwise equal.
* Autograd through a small torch actor and critic against the eager f32 loss on the GPU.
* PPOLearner: lr = 0 leaves the packed weights bitwise unchanged and reports the reference's
  stats; lr = 3e-4 lowers the loss and the kernels' forwards follow the trained torch networks
  (both on fragments the f32 actor collects with the Gaussian mean: sampling is a bf16-path
  feature of the actor kernel); collect -> update -> collect runs with the sampling bf16 actor.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from tests import critic_ref as cr
from tests import ppo_ref as pr

pytestmark = pytest.mark.gpu

COEF = dict(pr.COEF, entropy_coeff=0.01)
COEF_VF1 = dict(COEF, vf_clip_param=1.0, kl_coeff=0.5)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


# ---------------------------------------------------------------- moments
@pytest.mark.parametrize("frac", [0.0, 0.8, 1.0])
@pytest.mark.parametrize("rows", [1, 257, 70_001])
def test_masked_moments_vs_numpy_f64(dev, rows, frac):
    _check_moments(dev, rows, frac)


def test_masked_moments_more_rows_than_one_pass(dev):
    _check_moments(dev, 1024 * 4096 + 5_003, 0.8)  # the grid is capped at 1,024 blocks: threads take a second pass


def _check_moments(dev, rows, frac):
    from swarm_marl_amd import masked_moments
    rng = np.random.default_rng(rows + int(10 * frac))
    x = (rng.normal(0.3, 2.0, rows + 1)).astype(np.float32)
    valid = rng.random(rows + 1) < frac
    want = pr.moments(x[:rows], valid[:rows])
    want1 = pr.moments(x[1:], valid[1:])
    x[~valid] = np.nan  # never used
    dx, dv = torch.from_numpy(x).to(dev), torch.from_numpy(valid).to(dev)
    got = masked_moments(dx[:rows], dv[:rows])
    again = masked_moments(dx[:rows], dv[:rows].view(torch.uint8), out=torch.full((4,), -1.0, dtype=torch.float64, device=dev))
    got1 = masked_moments(dx[1:], dv[1:]).cpu().numpy()  # 4-B aligned only: the one-row-per-load kernel
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))
    got = got.cpu().numpy()
    for g, w in ((got, want), (got1, want1)):
        err = np.abs(g - w) / np.maximum(1.0, np.abs(w))
        print(f"moments rows={rows} frac={frac}: count {g[0]:.0f} rel err mean {err[1]:.2e} std {err[2]:.2e} inv {err[3]:.2e}")
        assert g[0] == w[0]
        assert np.all(err[1:] <= 1e-12), err
    if frac == 0.0:
        assert np.array_equal(got, [0.0, 0.0, 0.0, 1e4])


# ---------------------------------------------------------------- the head
@functools.lru_cache(maxsize=None)
def _case(env_rows, n, a, vf1=False):
    coef = COEF_VF1 if vf1 else COEF
    case = pr.make_case(env_rows, n, a, 1000 * a + 10 * n + env_rows, coef)
    return case, coef, pr.reference(case, coef)


def _run(dev, case, coef, **override):
    """(stats [7] f64, grad_logits, grad_value) of `ppo_loss` + backward on a NumPy case."""
    from swarm_marl_amd import masked_moments, ppo_loss
    t = {k: torch.from_numpy(v).to(dev) for k, v in dict(case, **override).items()}
    clean = {k: torch.from_numpy(v).to(dev) for k, v in case.items()}
    mom = masked_moments(clean["advantage"], clean["valid"])  # the clean fragment's moments in either run
    if override:
        assert torch.equal(mom, masked_moments(t["advantage"], t["valid"]))
    logits, value = t.pop("logits").requires_grad_(True), t.pop("value").requires_grad_(True)
    loss, stats = ppo_loss(logits, value, adv_moments=mom, **t, **coef)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and not stats.requires_grad
    assert loss.item() == np.float32(stats[1].item())
    loss.backward()
    return stats.cpu().numpy(), logits.grad.cpu().numpy(), value.grad.cpu().numpy()


def _check_head(dev, env_rows, n, a, vf1=False):
    case, coef, ref = _case(env_rows, n, a, vf1)
    stats, gl, gv = _run(dev, case, coef)
    pr.check_head(case, coef, ref, stats, gl, gv)  # the band conditions, the bounds and the exact counts
    return ref


@pytest.mark.parametrize("a", [1, 3, 6])
@pytest.mark.parametrize("n", [1, 3, 4, 63, 64, 65, 256])
def test_head_vs_float64_reference(dev, n, a):
    for env_rows in (1, 2, 65):
        ref = _check_head(dev, env_rows, n, a, vf1=(a == 3 and n in (4, 65)))
    if n >= 63:  # enough rows for every branch to show
        v = _case(65, n, a, a == 3 and n in (4, 65))[0]["valid"]
        r, c = ref["ratio"][v], COEF["clip_param"]
        assert (r > 1 + c).mean() > 0.02 and (r < 1 - c).mean() > 0.02 and 0.01 < ref["stats"]["clip_frac"] < 0.9


def test_head_many_tiles(dev):
    ref = _check_head(dev, 1025, 4, 3, vf1=True)  # 17 tiles of 64 env-rows, the last one partial
    assert 0 < (ref["err2"] > 1.0).mean() < 1


def test_head_more_tiles_than_blocks(dev):
    _check_head(dev, 1030, 130, 1)  # one env-row per tile, 1,030 tiles on the 1,024-block grid: six blocks take two


@pytest.mark.parametrize("n,env_rows", [(64, 65), (256, 5), (3, 200)])
def test_invalid_rows_are_never_read_and_launches_repeat(dev, n, env_rows):
    case, coef, _ = _case(env_rows, n, 3)
    bad = ~case["valid"]
    assert bad.any()
    poison = np.where(np.arange(bad.sum()) % 3 == 0, np.nan, np.where(np.arange(bad.sum()) % 3 == 1, np.inf, -np.inf))
    over = {}
    for k in ("logits", "behaviour_logits", "actions", "logp", "advantage", "value_target"):
        x = case[k].copy()
        x[bad] = poison.astype(np.float32).reshape((-1,) + (1,) * (x.ndim - 1))
        over[k] = x
    clean = _run(dev, case, coef)
    again = _run(dev, case, coef)
    dirty = _run(dev, case, coef, **over)
    for name, c, a2, d in zip(("stats", "grad_logits", "grad_value"), clean, again, dirty):
        assert np.array_equal(c.view(np.uint8), a2.view(np.uint8)), name
        assert np.array_equal(c.view(np.uint8), d.view(np.uint8)), name
        assert np.isfinite(d).all(), name
    assert np.all(dirty[1][bad] == 0)


def test_argument_checks(dev):
    from swarm_marl_amd import masked_moments, ppo_loss
    case, coef, _ = _case(2, 4, 3)
    t = {k: torch.from_numpy(v).to(dev) for k, v in case.items()}
    mom = masked_moments(t["advantage"], t["valid"])
    kw = {k: t[k] for k in ("behaviour_logits", "actions", "logp", "advantage", "value_target", "valid")}
    ppo_loss(t["logits"], t["value"], adv_moments=mom, **kw)
    with pytest.raises(ValueError, match="logp"):
        ppo_loss(t["logits"], t["value"], adv_moments=mom, **dict(kw, logp=t["logp"][:-1].contiguous()))
    with pytest.raises(ValueError, match="env-row"):
        ppo_loss(t["logits"], t["value"][:1].repeat(3), adv_moments=mom, **kw)
    with pytest.raises(ValueError, match="adv_moments"):
        ppo_loss(t["logits"], t["value"], adv_moments=mom.float(), **kw)
    with pytest.raises(ValueError, match="logits"):
        ppo_loss(t["logits"].double(), t["value"], adv_moments=mom, **kw)
    with pytest.raises(ValueError, match="valid"):
        masked_moments(t["advantage"], t["valid"][:-1])


# ---------------------------------------------------------------- autograd
def test_autograd_through_torch_actor_and_critic(dev):
    from swarm_marl_amd import masked_moments, ppo_loss
    d, g, n, env_rows = 37, 27, 4, 64
    case, coef, _ = _case(env_rows, n, 3)
    t = {k: torch.from_numpy(v).to(dev) for k, v in case.items()}
    torch.manual_seed(3)
    actor = torch.nn.Sequential(torch.nn.Linear(d, 32), torch.nn.ReLU(), torch.nn.Linear(32, 6)).to(dev)
    critic = torch.nn.Sequential(torch.nn.Linear(g, 32), torch.nn.ReLU(), torch.nn.Linear(32, 1)).to(dev)
    obs = torch.randn((env_rows * n, d), device=dev)
    gs = torch.randn((env_rows, g), device=dev)
    with torch.no_grad():  # the actor's output is the new policy: the behaviour policy plus its small map
        actor[2].weight.mul_(0.2)
        actor[2].bias.zero_()
    params = list(actor.parameters()) + list(critic.parameters())
    mom = masked_moments(t["advantage"], t["valid"])
    rest = {k: t[k] for k in ("actions", "logp", "advantage", "value_target", "valid")}

    def forward():
        return t["behaviour_logits"] + actor(obs), critic(gs).view(env_rows)

    def grads(scale=None, fused=True):
        for p in params:
            p.grad = None
        logits, value = forward()
        if fused:
            loss, _ = ppo_loss(logits, value, behaviour_logits=t["behaviour_logits"], adv_moments=mom, **rest, **coef)
        else:
            m = mom.cpu().numpy()
            loss = pr.loss(logits, value, t["behaviour_logits"], *[rest[k] for k in rest], float(m[1]), float(m[3]), **coef)[0]
        loss.backward(None if scale is None else torch.tensor(scale, device=dev))
        return loss.item(), [p.grad.clone() for p in params]

    l1, g1 = grads()
    l0, g0 = grads(fused=False)
    _, g2 = grads(scale=2.0)
    assert abs(l1 - l0) <= 1e-5 * max(1.0, abs(l0))
    for a1, a0, a2 in zip(g1, g0, g2):
        assert a0.abs().max() > 0
        err = (a1 - a0).abs().max().item() / a0.abs().max().item()
        print(f"autograd {tuple(a0.shape)}: rel err {err:.2e} (bound 1e-4)")
        assert err <= 1e-4
        assert torch.allclose(a2, 2 * a1, rtol=1e-6, atol=0)


# ---------------------------------------------------------------- the learner
CFG = dict(max_steps=5, goal_radius=6.0)
T, E, N = 8, 32, 4


def _arrays(shapes, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1, 1, s).astype(np.float32) / np.float32(np.sqrt(s[-1])) for s in shapes]


def _setup(dev, precision="f32", **learner_kw):
    from swarm_marl_amd import CriticMLP, PPOLearner, RolloutCollector, VecSwarm
    from swarm_marl_amd.policy import PolicyMLP
    vec = VecSwarm(E, dict(CFG, num_drones=N), device=dev, auto_reset=True, seed=11, with_global_state=True)
    vec.reset()
    w = _arrays(((256, 37), (256,), (256, 256), (256,), (6, 256), (6,)), 5)
    policy = PolicyMLP.from_arrays(*w, device=dev, precision=precision)
    policy0 = PolicyMLP.from_arrays(*w, device=dev, precision=precision)
    critic = CriticMLP(cr.make_critic(6 * N + 3, seed=2), device=dev, precision="f32")
    col = RolloutCollector(vec, policy, critic, horizon=T, seed=3)
    learner = PPOLearner(policy, critic, **learner_kw)
    return col, learner, policy, policy0, critic


def test_learner_lr0_changes_nothing_and_reports_the_reference(dev):
    col, learner, policy, _, critic = _setup(dev, lr=0.0, num_epochs=1, minibatch_env_rows=T * E, entropy_coeff=0.01)
    batch = col.collect(deterministic=True)  # the f32 actor kernel has no sampling path: it acts with the mean
    assert not batch["valid"].all() and batch["valid"].any()
    pw, cw, ptr = policy.weights.clone(), critic.weights.clone(), policy.weights.data_ptr()
    info = learner.update(batch)
    assert torch.equal(policy.weights, pw) and torch.equal(critic.weights, cw) and policy.weights.data_ptr() == ptr
    assert all(np.isfinite(info[k]) for k in pr.STATS) and info["epoch_total_loss"] == [info["total_loss"]]
    b = {k: v.cpu() for k, v in batch.items()}
    te = T * E
    with torch.no_grad():
        logits = learner.actor(batch["obs"].reshape(te * N, 37)).double().cpu()
        value = learner.value_net(batch["global_state"][:T].reshape(te, -1)).double().cpu().view(te)
    mom = pr.moments(b["advantage"].numpy(), b["valid"].numpy())
    f = lambda k, *s: b[k].reshape(te * N, *s).double()  # noqa: E731
    _, ref, _, _ = pr.loss(logits, value, f("logits", 6), f("actions", 3), f("logp"), f("advantage"), f("value_target"),
                           b["valid"].reshape(-1), float(mom[1]), float(mom[3]), **dict(pr.COEF, entropy_coeff=0.01))
    for k in pr.STATS:
        err = abs(info[k] - float(ref[k])) / max(1.0, abs(float(ref[k])))
        print(f"learner lr=0 {k}: {info[k]:.6g} vs {float(ref[k]):.6g} rel err {err:.2e}")
        assert err <= 1e-5, k
    assert info["count"] == int(b["valid"].sum())
    assert info["kl"] < 0.005 and info["kl_coeff"] == pytest.approx(0.1)  # below half the target: halved


def test_learner_trains_and_pushes_weights(dev):
    col, learner, policy, policy0, critic = _setup(dev, lr=3e-4, num_epochs=5, minibatch_env_rows=T * E)
    batch = col.collect(deterministic=True)
    obs, gs = batch["obs"].clone(), batch["global_state"].clone()
    before_l, before_v = policy.logits(obs), critic.value(gs)
    info = learner.update(batch)
    losses = info["epoch_total_loss"]
    print("learner epoch losses", losses)
    assert len(losses) == 5 and losses[-1] < losses[0]
    with torch.no_grad():
        want_l = learner.actor(obs.reshape(-1, 37)).reshape(before_l.shape)
        want_v = learner.value_net(gs.reshape(-1, gs.shape[-1])).reshape(before_v.shape)
    got_l, got_v = policy.logits(obs), critic.value(gs)
    assert torch.all((got_l - want_l).abs() <= 1e-4 + 1e-5 * want_l.abs()), (got_l - want_l).abs().max().item()
    assert torch.all((got_v - want_v).abs() <= 1e-4 + 1e-5 * want_v.abs()), (got_v - want_v).abs().max().item()
    assert (got_l - before_l).abs().max().item() > 1e-3 and (got_v - before_v).abs().max().item() > 1e-3
    assert torch.equal(policy0.logits(obs), before_l)
    with pytest.raises(ValueError):
        policy.load_layers(policy.layers[:2])
    with pytest.raises(ValueError):
        critic.load_layers([(w[:, :-1], b) for w, b in critic.layers])


def test_collect_update_collect(dev):
    # the training loop as it runs: the bf16 actor samples, the learner's f32 copy trains
    col, learner, policy, policy0, _ = _setup(dev, "bf16", lr=3e-4, num_epochs=2, minibatch_env_rows=100, seed=4)
    info = learner.update(col.collect())  # 256 env-rows: minibatches of 100, 100 and 56
    assert all(np.isfinite(v) for k, v in info.items() if k != "epoch_total_loss") and np.isfinite(info["epoch_total_loss"]).all()
    batch = col.collect()
    assert bool(torch.isfinite(batch["logits"]).all())
    old = policy0.logits(batch["obs"])
    assert (batch["logits"] - old).abs().max().item() > 1e-3
    info2 = learner.update(batch)
    assert all(np.isfinite(info2[k]) for k in pr.STATS)
