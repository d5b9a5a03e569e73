"""GPU: the attention actor's kernels (csrc/swarm_attn.hip) against tests/attn_ref.py, through
`AttentionPolicy`, `RolloutCollector` and `PPOLearner`.

Shapes (K, Ms, out) = attn_ref.SHAPES + attn_ref.MORE_SHAPES (the latter: the logits widths 4, 8, 10
and sensed_obstacles 2, 3) and row counts 1, 33, 257 (a lone row, one past a 32-row tile,
one past a 256-row workgroup; 33 and 257 also leave the second 32-row tile of a wave's 64 rows with
a single row, 1 leaves it empty).  One 257-row reference per shape; the smaller counts are prefixes.

Bounds:
  f32   |got - ref64| <= 1e-4 + 1e-5 |ref64|  (the project's f32 logit bound; a plain f32 torch forward
        of these fixtures is within 2.4e-7 of float64).
  bf16  max |got - emu| <= 1e-3 (emu: attn_ref.forward_bf16_emu, the rounding points of DESIGN.md
        §3.3), and max |got - ref64| <= max |emu - ref64| + 1e-3.
Measured on an MI355X: f32 at most 9.4e-7 (0.0085 of the bound, the collector's rows);
bf16 against the emulation at most 1.5e-5 on the SHAPES fixtures, 4.1e-4 on MORE_SHAPES ((11,5,10):
three rows with one hidden activation each on a bf16 rounding tie, every other row within 1.1e-7),
1.15e-4 after load_params, 7.7e-4 on the peaked fixture (whose 12 x larger folded weights amplify
every flipped bf16 rounding of s); recovered normals within 7.0e-7 of sample_noise64.

More than one workgroup and grid pass, slot order on a saturated softmax, row independence, unaligned
views, streams and the bf16 collector: tests/test_gpu_attn_shapes.py.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from tests import attn_ref as ar
from tests import critic_ref as cr
from tests import policy_ref as pr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _case(k, ms, out, in_proj_scale=1.0, seed_offset=0, log_std_scale=None, q_scale=1.0):
    """(params, layers, obs, ref64, emu): computed once per fixture, never modified."""
    params, layers = ar.make_attn(k, ms, out, in_proj_scale=in_proj_scale, seed_offset=seed_offset,
                                  log_std_scale=log_std_scale, q_scale=q_scale)
    x = ar.obs_set(k, ms)
    ref = ar.forward64(params, layers, k, x)
    emu = ar.forward_bf16_emu(params, layers, k, ms, x)
    for a in (x, ref, emu):
        a.setflags(write=False)
    return params, layers, x, ref, emu


def _policy(dev, params, layers, k, ms, precision):
    from swarm_marl_amd import AttentionPolicy
    return AttentionPolicy(params, layers, neighbor_k=k, sensed_obstacles=ms, device=dev, precision=precision)


def check_f32(got, ref, tag):
    err = np.abs(got.astype(np.float64) - ref)
    use = np.max(err / (1e-4 + 1e-5 * np.abs(ref)))
    print(f"{tag}: f32 max err {err.max():.3e} (bound use {use:.4f})")
    assert np.isfinite(got).all()
    assert np.all(err <= 1e-4 + 1e-5 * np.abs(ref)), (tag, err.max())


def check_bf16(got, emu, ref, tag):
    got = got.astype(np.float64)
    e_emu, e_ref, floor = np.abs(got - emu).max(), np.abs(got - ref).max(), np.abs(emu - ref).max()
    print(f"{tag}: bf16 max |got - emu| {e_emu:.3e} (bound 1e-3), |got - ref| {e_ref:.3e} "
          f"(bound {floor:.3e} + 1e-3)")
    assert np.isfinite(got).all()
    assert e_emu <= 1e-3, (tag, e_emu)
    assert e_ref <= floor + 1e-3, (tag, e_ref, floor)


@pytest.mark.parametrize("k,ms,out", ar.SHAPES + ar.MORE_SHAPES)
def test_f32_logits(dev, k, ms, out):
    params, layers, x, ref, _ = _case(k, ms, out)
    pol = _policy(dev, params, layers, k, ms, "f32")
    assert (pol.in_dim, pol.out_dim, pol.precision, pol.device) == (9 + 4 * k + 4 * ms, out, "f32", dev)
    for rows in ar.ROW_COUNTS:
        got = pol.logits(torch.tensor(x[:rows]).to(dev)).cpu().numpy()
        assert got.shape == (rows, out)
        check_f32(got, ref[:rows], f"K={k} Ms={ms} out={out} rows={rows}")


@pytest.mark.parametrize("k,ms,out", ar.SHAPES + ar.MORE_SHAPES)
def test_bf16_logits(dev, k, ms, out):
    params, layers, x, ref, emu = _case(k, ms, out)
    pol = _policy(dev, params, layers, k, ms, "bf16")
    for rows in ar.ROW_COUNTS:
        got = pol.logits(torch.tensor(x[:rows]).to(dev)).cpu().numpy()
        check_bf16(got, emu[:rows], ref[:rows], f"K={k} Ms={ms} out={out} rows={rows}")


def test_peaked_softmax(dev):
    """in_proj_weight x 12: raw scores beyond f32's exp range, attention on one slot."""
    k, ms, out = 3, 4, 6
    params, layers, x, ref, emu = _case(k, ms, out, in_proj_scale=12.0, seed_offset=1)
    _, score, a = ar.forward64(params, layers, k, x, details=True)
    assert a.max() > 0.99 and np.abs(score).max() > 88.8  # exp(88.8) overflows f32: no max-subtraction, no result
    assert score.max() > 88.8
    xt = torch.tensor(x).to(dev)
    check_f32(_policy(dev, params, layers, k, ms, "f32").logits(xt).cpu().numpy(), ref, "peaked")
    check_bf16(_policy(dev, params, layers, k, ms, "bf16").logits(xt).cpu().numpy(), emu, ref, "peaked")


@pytest.mark.parametrize("k,ms,out", [(3, 4, 6), (16, 5, 12)])
def test_zero_filled_neighbour_slots_are_attended(dev, k, ms, out):
    params, layers, x0, _, _ = _case(k, ms, out)
    x = x0.copy()
    nb = x[:, 9:9 + 4 * k].reshape(len(x), k, 4)
    nb[0::3, k - 1] = 0       # the last slot empty
    nb[1::3, 1:] = 0          # only the first slot filled
    nb[5] = 0                 # no neighbour at all
    ref = ar.forward64(params, layers, k, x)
    emu = ar.forward_bf16_emu(params, layers, k, ms, x)
    # a masked softmax would differ: the rows with the last slot empty, evaluated without that slot
    masked = ar.forward64(params, layers, k - 1, np.delete(x[0::3], np.s_[9 + 4 * (k - 1):9 + 4 * k], axis=1))
    assert np.abs(masked - ref[0::3]).max() > 2e-3
    xt = torch.tensor(x).to(dev)
    check_f32(_policy(dev, params, layers, k, ms, "f32").logits(xt).cpu().numpy(), ref, f"zero slots K={k}")
    check_bf16(_policy(dev, params, layers, k, ms, "bf16").logits(xt).cpu().numpy(), emu, ref, f"zero slots K={k}")


GUARD = 64
SENTINEL = 12345.0


def _guarded(dev, rows, width):
    buf = torch.full((rows * width + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[:rows * width].view(rows, width)


@pytest.mark.parametrize("precision", ["bf16", "f32"])
@pytest.mark.parametrize("k,ms,out", [(3, 4, 6), (16, 5, 12), (6, 0, 2)] + list(ar.MORE_SHAPES))
def test_deterministic_actions_and_canaries(dev, precision, k, ms, out):
    params, layers, x, _, _ = _case(k, ms, out)
    pol = _policy(dev, params, layers, k, ms, precision)
    ad = out // 2
    for rows in ar.ROW_COUNTS:
        xt = torch.tensor(x[:rows]).to(dev)
        lbuf, lg = _guarded(dev, rows, out)
        abuf, ac = _guarded(dev, rows, ad)
        pol.forward(xt, logits=lg, actions=ac)
        lbuf2, lg2 = _guarded(dev, rows, out)
        pol.forward(xt, logits=lg2)  # actions=None
        abuf2, ac2 = _guarded(dev, rows, ad)
        pol.forward(xt, actions=ac2)  # logits=None
        for buf, n in ((lbuf, rows * out), (abuf, rows * ad), (lbuf2, rows * out), (abuf2, rows * ad)):
            assert torch.all(buf[n:] == SENTINEL), (precision, rows)
            assert torch.all(buf[:n] != SENTINEL)
        assert torch.equal(ac.view(torch.int32), lg[:, :ad].contiguous().view(torch.int32))
        assert torch.equal(lg2.view(torch.int32), lg.view(torch.int32))
        assert torch.equal(ac2.view(torch.int32), ac.view(torch.int32))
        assert torch.equal(pol.act(xt).view(torch.int32), ac.view(torch.int32))
    pol.forward(torch.zeros((0, pol.in_dim), device=dev), logits=torch.zeros((0, out), device=dev))  # rows = 0: a no-op
    with pytest.raises(ValueError):
        pol.forward(xt)  # neither output


@pytest.mark.parametrize("precision", ["bf16", "f32"])
@pytest.mark.parametrize("k,ms,out", [(3, 4, 6), (16, 5, 12), (6, 0, 2)] + list(ar.MORE_SHAPES))
def test_sampling_draws_the_policy_normals(dev, precision, k, ms, out):
    """W3 = 0, b3 = 0: mean 0 and std 1, so the actions are the normals themselves — bit for bit those
    of a zero-weight PolicyMLP at the same (seed, counter, rows)."""
    from swarm_marl_amd.policy import PolicyMLP
    params, layers, x, _, _ = _case(k, ms, out)
    zl = [layers[0], layers[1], (np.zeros_like(layers[2][0]), np.zeros_like(layers[2][1]))]
    pol = _policy(dev, params, zl, k, ms, precision)
    d = pol.in_dim if pol.in_dim <= 47 else 47
    mlp = PolicyMLP.from_arrays(np.zeros((256, d), np.float32), np.zeros(256, np.float32),
                                np.zeros((256, 256), np.float32), np.zeros(256, np.float32),
                                np.zeros((out, 256), np.float32), np.zeros(out, np.float32), device=dev)
    xt = torch.tensor(x).to(dev)
    for seed, counter in ((0, 0), (0x123456789ABCDEF, 3), (7, 2 ** 40 + 5)):
        got = pol.act(xt, deterministic=False, seed=seed, counter=counter)
        want = mlp.act(torch.zeros((len(x), d), device=dev), deterministic=False, seed=seed, counter=counter)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (seed, counter)
        z = pr.sample_noise64(len(x), out // 2, seed, counter)
        assert np.abs(got.cpu().numpy() - z).max() <= 1e-5
    assert not torch.equal(pol.act(xt, deterministic=False, seed=1, counter=0),
                           pol.act(xt, deterministic=False, seed=1, counter=1))


@pytest.mark.parametrize("precision", ["bf16", "f32"])
@pytest.mark.parametrize("k,ms,out", [(3, 4, 6), (16, 5, 12)] + list(ar.MORE_SHAPES))
def test_sampling_with_real_weights(dev, precision, k, ms, out):
    params, layers, x, _, _ = _case(k, ms, out, log_std_scale=0.25)
    pol = _policy(dev, params, layers, k, ms, precision)
    ad = out // 2
    for rows in (33, 257):
        xt = torch.tensor(x[:rows]).to(dev)
        lg = torch.empty((rows, out), device=dev)
        ac = torch.empty((rows, ad), device=dev)
        pol.forward(xt, logits=lg, actions=ac, sample=True, seed=99, counter=17)
        assert torch.equal(lg.view(torch.int32), pol.logits(xt).view(torch.int32))  # sampling leaves the logits alone
        lgn, acn = lg.cpu().numpy().astype(np.float64), ac.cpu().numpy().astype(np.float64)
        mean, ls = lgn[:, :ad], lgn[:, ad:]
        assert ls.min() >= -2.0 and ls.max() <= 0.5
        z = (acn - mean) / np.exp(ls)
        err = np.abs(z - pr.sample_noise64(rows, ad, 99, 17)).max()
        print(f"sample {precision} K={k} rows={rows}: max |z - z_ref| {err:.3e} (bound 1e-5)")
        assert err <= 1e-5


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_repeatable(dev, precision):
    k, ms, out = 16, 5, 12
    params, layers, x, _, _ = _case(k, ms, out)
    pol = _policy(dev, params, layers, k, ms, precision)
    xt = torch.tensor(x).to(dev)
    assert torch.equal(pol.logits(xt).view(torch.int32), pol.logits(xt).view(torch.int32))
    a1 = pol.act(xt, deterministic=False, seed=5, counter=9)
    assert torch.equal(a1.view(torch.int32), pol.act(xt, deterministic=False, seed=5, counter=9).view(torch.int32))


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_load_params(dev, precision):
    k, ms, out = 2, 1, 6
    params, layers, x, _, _ = _case(k, ms, out)
    p2, l2, _, ref2, emu2 = _case(k, ms, out, seed_offset=3)
    pol = _policy(dev, params, layers, k, ms, precision)
    xt = torch.tensor(x).to(dev)
    before, ptr = pol.logits(xt), pol.weights.data_ptr()
    pol.load_params(p2, l2)
    got = pol.logits(xt)
    assert pol.weights.data_ptr() == ptr and not torch.equal(got, before)
    if precision == "f32":
        check_f32(got.cpu().numpy(), ref2, "load_params")
    else:
        check_bf16(got.cpu().numpy(), emu2, ref2, "load_params")
    assert np.array_equal(pol.params[ar.NAMES[4]], p2[ar.NAMES[4]]) and np.array_equal(pol.layers[0][0], l2[0][0])


# ---------------------------------------------------------------- collector and learner
CFG = dict(max_steps=5, goal_radius=6.0)
E, N = 8, 4


def _rollout(dev, horizon, precision="f32"):
    from swarm_marl_amd import CriticMLP, RolloutCollector, VecSwarm
    vec = VecSwarm(E, dict(CFG, num_drones=N), device=dev, auto_reset=True, seed=11, with_global_state=True)
    vec.reset()
    params, layers, _, _, _ = _case(3, 4, 6, log_std_scale=0.25)
    policy = _policy(dev, params, layers, 3, 4, precision)
    critic = CriticMLP(cr.make_critic(6 * N + 3, seed=2), device=dev, precision="f32")
    return RolloutCollector(vec, policy, critic, horizon=horizon, seed=3), policy, critic, params, layers


def test_collector_with_attention_policy(dev):
    col, policy, _, params, layers = _rollout(dev, 3)
    batch = col.collect()
    assert batch["obs"].shape == (3, E, N, 37) and batch["logits"].shape == (3, E, N, 6)
    for t in range(3):
        assert torch.equal(batch["logits"][t].view(torch.int32), policy.logits(batch["obs"][t]).view(torch.int32))
    obs = batch["obs"].cpu().numpy().reshape(-1, 37)
    ref = ar.forward64(params, layers, 3, obs)
    check_f32(batch["logits"].cpu().numpy().reshape(-1, 6), ref, "collector logits")
    act = batch["actions"].cpu().numpy().reshape(-1, 3).astype(np.float64)
    assert np.abs(act - ref[:, :3]).max() > 1e-2  # sampled, not the mean
    z = pr.sample_noise64(E * N, 3, 3, 1)  # step 1: seed 3, counter 1
    lg1 = batch["logits"][1].cpu().numpy().reshape(-1, 6).astype(np.float64)
    assert np.abs((batch["actions"][1].cpu().numpy().reshape(-1, 3) - lg1[:, :3]) / np.exp(lg1[:, 3:]) - z).max() <= 1e-5
    mean, ls = ref[:, :3], ref[:, 3:]
    zz = (act - mean) * np.exp(-ls)
    logp = np.sum(-0.5 * zz * zz - ls, axis=1) - 0.5 * 3 * np.log(2 * np.pi)
    got = batch["logp"].cpu().numpy().reshape(-1).astype(np.float64)
    err = np.abs(got - logp)
    print(f"collector logp: max err {err.max():.3e} (bound use {np.max(err / (1e-4 + 1e-5 * np.abs(logp))):.4f})")
    assert np.all(err <= 1e-4 + 1e-5 * np.abs(logp))


def test_learner_with_attention_policy(dev):
    from swarm_marl_amd import AttentionActor, PPOLearner
    col, policy, critic, params, layers = _rollout(dev, 4)
    learner = PPOLearner(policy, critic, lr=3e-4, num_epochs=2, minibatch_env_rows=4 * E)
    assert isinstance(learner.actor, AttentionActor)
    batch = col.collect()
    obs = batch["obs"].clone()
    before = policy.logits(obs)
    ptr = policy.weights.data_ptr()
    info = learner.update(batch)
    assert all(np.isfinite(v) for k, v in info.items() if k != "epoch_total_loss")
    assert len(info["epoch_total_loss"]) == 2 and np.isfinite(info["epoch_total_loss"]).all()
    # every parameter group moved: embeds, in_proj, out_proj, trunk
    for name in ar.NAMES:
        assert np.abs(policy.params[name] - params[name]).max() > 0, name
    for (w, b), (w0, b0) in zip(policy.layers, layers):
        assert np.abs(w - w0).max() > 0 and np.abs(b - b0).max() > 0
    # the write-back: the device policy is the trained module
    with torch.no_grad():
        want = learner.actor(obs.reshape(-1, 37)).reshape(before.shape)
    got = policy.logits(obs)
    err = (got - want).abs()
    print(f"learner write-back: max err {err.max().item():.3e}, moved {(got - before).abs().max().item():.3e}")
    assert torch.all(err <= 1e-4 + 1e-5 * want.abs())
    assert policy.weights.data_ptr() == ptr and (got - before).abs().max().item() > 1e-4
