"""GPU: sampled actions on the f32 and f32x3 actor paths (csrc/swarm_policy.hip: the
SWARM_POLICY_ACT_SAMPLE instances of policy_mlp_f32, policy_mlp_x3l and policy_mlp_x3).

Kernels under test, by `mode`: "f32" (policy_mlp_f32, 16-row tiles), "f32x3" (policy_mlp_x3l, the
default f32x3 kernel, 32-row tiles) and "f32x3p" (policy_mlp_x3, SWARM_POLICY_X3_PIPELINED=1).
Weights, observations and the normals' reference come from tests/policy_ref.py.

1. The normals are the defined ones: z = (a - mean) exp(-log_std), recovered from the launch's own
   logits, against sample_noise64 under the bound of tests/test_gpu_policy_dims.py (derived there):
     |z - z_ref| <= 1e-5 (1 + |z_ref|) + 2^-22 |a| exp(-log_std),   log_std in [-2, 0.5] (asserted).
   With it: the sampled launch's logits are a mean launch's bit for bit, a (seed, counter) repeats
   bit for bit, counter + 1 changes every row, the prefixes rows = 1 and 33 (a partial 16-row and a
   partial 32-row tile) are the head of the 257-row result, nothing past rows * ad is written.
2. Equal logits give equal actions on every precision: with w3 = 0 the logits are exactly b3 on
   every path, so bf16, f32, f32x3 and f32x3p must agree bit for bit — the shared draw and the
   shared order of mean + expf(log_std) * z.
3. 70,001 rows (more row tiles than one grid pass): logits against the float64 forward at
   1e-4 + 1e-5 |ref|, z against sample_noise64 over all 70,001 row indices.
4. policy_mlp_x3l and policy_mlp_x3 agree bit for bit when sampling.
5. RolloutCollector on an f32x3 (and once an f32) policy, 35 rows per step: equal seeds give equal
   batches, actions[t] is a direct forward at counter t, logp is gaussian_logp of the record.
6. The learner starts on-policy: a fragment collected with the f32x3 actor, PPOLearner at lr = 0,
   bounds info["kl"].  Derivation of the bound.  Per action dim the head's KL(behaviour || new) is
       KL_k = d + (exp(-2 d) - 1) / 2 + (mu0 - mu)^2 exp(-2 s) / 2,     d = s - s0,
   (mu0, s0) the recorded logits and (mu, s) the learner's.  The kernel's logits and the learner's
   float32 torch actor are each within b = 1e-4 + 1e-5 |logit| of the float64 forward (the project's
   f32 logit bound), so |mu - mu0| <= 2 b_mu and |d| <= 2 b_s.  f(d) = d + (exp(-2 d) - 1) / 2 is
   convex with f(0) = 0 and f(-x) >= f(x) for x >= 0, so f(d) <= f(-2 b_s); and s >= s0 - 2 b_s gives
   exp(-2 s) <= exp(-2 s0 + 4 b_s).  Hence
       KL_k <= -2 b_s + (exp(4 b_s) - 1) / 2 + 2 b_mu^2 exp(-2 s0 + 4 b_s),
   summed over the action dims and averaged over the valid recorded rows in float64.  b is taken on
   the recorded logit l as (1e-4 + 1e-5 |l|) / (1 - 1e-5), which covers |float64 logit| <= |l| + b.
   The bound comes from the recorded logits alone; it is ~1e-7 per row, and the head evaluates KL_k
   in f32 from terms of size 0.5 (ulp 6e-8), so the reported mean may also sit a little below 0:
   the test asserts |kl| <= bound.

Measured on an MI355X (pytest -s prints every figure): see MEASURED below and DESIGN.md §5.2.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import critic_ref as cr
from tests import policy_ref as pr
from tests.test_gpu_policy_dims import run_guarded

pytestmark = pytest.mark.gpu

MODES = ("f32", "f32x3", "f32x3p")
SAMPLE_SHAPES = ((15, 2), (16, 4), (25, 6), (47, 12), (37, 6))  # ad = 1, 2, 3, 6
SEEDS = ((5, 7), (0x9E3779B97F4A7C15, (1 << 32) + 3))  # the second: all four key / counter words non-zero
BIG_ROWS = 70_001  # > 256 CUs x 8 waves x 32 rows (f32x3) and > 512 blocks x 4 waves x 16 rows (f32)
BIG_SHAPE = (25, 6)
# records, not bounds: the largest |z - z_ref| of test 1 / test 3 and its share of the bound; the kl
# of test 6 with its bound, and the kl of the same run collected with the bf16 actor
MEASURED = dict(z_err=(9.045e-7, 0.052), z_err_big=(1.038e-6, 0.077), kl_f32x3=-1.607e-8, kl_bound=6.515e-7, kl_bf16=1.026e-4)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _ids(shapes):
    return [f"{i}to{o}" for i, o in shapes]


def select(monkeypatch, mode: str) -> str:
    """Point the f32x3 entry at the kernel `mode` names; returns the PolicyMLP precision."""
    if mode == "f32x3p":
        monkeypatch.setenv("SWARM_POLICY_X3_PIPELINED", "1")
    else:
        monkeypatch.delenv("SWARM_POLICY_X3_PIPELINED", raising=False)
    return "f32x3" if mode == "f32x3p" else mode


_ACT, _POL, _REF = {}, {}, {}


def actor(shape):
    if shape not in _ACT:
        _ACT[shape] = pr.make_actor(*shape, log_std_scale=0.25)
    return _ACT[shape]


def policy(dev, shape, precision):
    from swarm_marl_amd.policy import PolicyMLP
    if (shape, precision) not in _POL:
        _POL[shape, precision] = PolicyMLP(actor(shape), device=dev, precision=precision)
    return _POL[shape, precision]


def noise(rows, ad, seed, counter):
    key = (rows, ad, seed, counter)
    if key not in _REF:
        _REF[key] = pr.sample_noise64(rows, ad, seed, counter)
    return _REF[key]


def recovered_z(lg, a):
    ad = a.shape[1]
    mean, ls = lg[:, :ad].astype(np.float64), lg[:, ad:].astype(np.float64)
    assert ls.min() >= -2.0 and ls.max() <= 0.5, (ls.min(), ls.max())
    return (a.astype(np.float64) - mean) * np.exp(-ls), ls


def check_z(z, z_ref, a, ls, tag):
    err = np.abs(z - z_ref)
    bound = 1e-5 * (1 + np.abs(z_ref)) + 2.0 ** -22 * np.abs(a.astype(np.float64)) * np.exp(-ls)
    print(f"{tag}: max |z - z_ref| {err.max():.3e} (bound use {np.max(err / bound):.3f}, max |z| {np.abs(z_ref).max():.2f})")
    assert np.all(err <= bound), (tag, err.max(), np.max(err / bound))


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ---------------------------------------------------------------- 1. the defined normals
@pytest.mark.parametrize("seed,counter", SEEDS, ids=["low_words", "all_words"])
@pytest.mark.parametrize("shape", SAMPLE_SHAPES, ids=_ids(SAMPLE_SHAPES))
@pytest.mark.parametrize("mode", MODES)
def test_sampled_noise_is_the_defined_philox_box_muller(dev, monkeypatch, mode, shape, seed, counter):
    pol = policy(dev, shape, select(monkeypatch, mode))
    ad = shape[1] // 2
    x = torch.from_numpy(pr.obs_set(shape[0])).to(dev)
    lg, a = run_guarded(pol, x, sample=True, seed=seed, counter=counter)
    mean_lg, mean_a = run_guarded(pol, x)
    assert np.array_equal(bits(lg), bits(mean_lg))  # sampling leaves the logits alone
    assert np.array_equal(bits(mean_a), bits(mean_lg[:, :ad]))
    z, ls = recovered_z(lg, a)
    check_z(z, noise(pr.ROWS, ad, seed, counter), a, ls, f"sample {mode} {shape} seed={seed:#x} counter={counter:#x}")
    for i, j in ((0, 1), (0, 16), (0, 32), (1, 32)):  # rows get their own draws
        assert np.abs(z[i] - z[j]).max() > 1e-3, (i, j)
    lg1, a1 = run_guarded(pol, x, sample=True, seed=seed, counter=counter)
    assert np.array_equal(bits(a1), bits(a)) and np.array_equal(bits(lg1), bits(lg))
    _, a2 = run_guarded(pol, x, sample=True, seed=seed, counter=counter + 1)
    assert np.all((bits(a2) != bits(a)).any(axis=1))  # counter + 1 changes every row
    for rows in (1, 33):  # a row's draw depends on its index, not on the launch's row count
        lgp, ap = run_guarded(pol, x[:rows], sample=True, seed=seed, counter=counter)
        assert np.array_equal(bits(ap), bits(a[:rows])) and np.array_equal(bits(lgp), bits(lg[:rows])), rows


def test_actions_only_launch_matches_and_logits_only_launch_draws_nothing(dev, monkeypatch):
    """Either output may be NULL: actions without logits are the same actions; logits without
    actions are the same logits."""
    shape = (25, 6)
    x = torch.from_numpy(pr.obs_set(shape[0])).to(dev)
    for mode in MODES:
        pol = policy(dev, shape, select(monkeypatch, mode))
        lg, a = run_guarded(pol, x, sample=True, seed=9, counter=2)
        only_a = torch.full((pr.ROWS, 3), -555.0, device=dev)
        pol.forward(x, actions=only_a, sample=True, seed=9, counter=2)
        only_l = torch.full((pr.ROWS, 6), -777.0, device=dev)
        pol.forward(x, logits=only_l, sample=True, seed=9, counter=2)
        assert np.array_equal(bits(only_a.cpu().numpy()), bits(a)), mode
        assert np.array_equal(bits(only_l.cpu().numpy()), bits(lg)), mode


# ---------------------------------------------------------------- 2. equal logits, equal actions
@pytest.mark.parametrize("shape", [(37, 6), (37, 12)], ids=_ids([(37, 6), (37, 12)]))
def test_every_precision_draws_the_same_actions_from_equal_logits(dev, monkeypatch, shape):
    from swarm_marl_amd.policy import PolicyMLP
    d, out = shape
    ad = out // 2
    (w1, b1, _), (w2, b2, _), (w3, _, _) = pr.make_actor(d, out)
    rng = np.random.default_rng(out)
    b3 = np.concatenate([rng.uniform(-1, 1, ad), rng.uniform(-2.0, 0.5, ad)]).astype(np.float32)
    layers = [(w1, b1, True), (w2, b2, True), (np.zeros_like(w3), b3, False)]
    x = torch.from_numpy(pr.obs_set(d)).to(dev)
    got = {}
    for mode in ("bf16",) + MODES:
        pol = PolicyMLP(layers, device=dev, precision=select(monkeypatch, mode))
        lg = pol.logits(x).cpu().numpy()
        assert np.array_equal(bits(lg), bits(np.broadcast_to(b3, lg.shape))), mode  # the logits are b3 on every path
        got[mode] = pol.act(x, deterministic=False, seed=SEEDS[1][0], counter=SEEDS[1][1]).cpu().numpy()
    z = (got["bf16"].astype(np.float64) - b3[:ad]) * np.exp(-b3[ad:].astype(np.float64))
    assert np.abs(z - noise(pr.ROWS, ad, *SEEDS[1])).max() < 1e-4  # and they are sampled, not the mean
    for mode in MODES:
        assert np.array_equal(bits(got[mode]), bits(got["bf16"])), mode


# ---------------------------------------------------------------- 3. past one grid pass
@pytest.mark.parametrize("mode", MODES)
def test_sampling_past_one_grid_pass(dev, monkeypatch, mode):
    """70,001 rows: the 257-row set repeated on the device, so the logits of row r are held to the
    float64 reference of row r mod 257; every row index has its own draw."""
    shape = BIG_SHAPE
    pol = policy(dev, shape, select(monkeypatch, mode))
    if "l64" not in _REF:
        _REF["l64"] = pr.forward64(actor(shape), pr.obs_set(shape[0]))
    x = torch.from_numpy(pr.obs_set(shape[0])).to(dev).repeat((BIG_ROWS + pr.ROWS - 1) // pr.ROWS, 1)[:BIG_ROWS]
    assert x.is_contiguous() and x.shape == (BIG_ROWS, shape[0])
    seed, counter = SEEDS[1]
    lg, a = run_guarded(pol, x, sample=True, seed=seed, counter=counter)
    want = _REF["l64"][np.arange(BIG_ROWS) % pr.ROWS]
    err = np.abs(lg - want)
    print(f"{mode} {shape} rows={BIG_ROWS} logits max err {err.max():.3e}")
    assert np.all(err <= 1e-4 + 1e-5 * np.abs(want)), err.max()
    z, ls = recovered_z(lg, a)
    check_z(z, noise(BIG_ROWS, shape[1] // 2, seed, counter), a, ls, f"sample {mode} {shape} rows={BIG_ROWS}")


# ---------------------------------------------------------------- 4. x3l == x3
def test_x3_two_waves_equals_pipelined_bitwise_when_sampling(dev, monkeypatch):
    pol = policy(dev, (37, 6), "f32x3")
    g = torch.Generator(device=dev).manual_seed(11)
    for rows in (1, 33, 255):
        obs = torch.randn((rows, 37), device=dev, generator=g) * 3
        select(monkeypatch, "f32x3p")
        lg_p, a_p = run_guarded(pol, obs, sample=True, seed=21, counter=rows)
        select(monkeypatch, "f32x3")
        lg_l, a_l = run_guarded(pol, obs, sample=True, seed=21, counter=rows)
        assert np.array_equal(bits(lg_l), bits(lg_p)) and np.array_equal(bits(a_l), bits(a_p)), rows
        assert np.abs(a_l - lg_l[:, :3]).max() > 1e-3  # sampled


# ---------------------------------------------------------------- 5. the collector
CE, CN, CT = 5, 7, 3  # 35 rows per step: ragged for the 16-row and the 32-row tiles


def _collector(dev, precision, per_agent, seed):
    from swarm_marl_amd import AgentValueMLP, CriticMLP, RolloutCollector, VecSwarm
    vec = VecSwarm(CE, dict(num_drones=CN), device=dev, auto_reset=True, seed=13, with_global_state=not per_agent)
    vec.reset()
    assert vec.obs_dim == 37
    pol = policy(dev, (37, 6), precision)
    critic = (AgentValueMLP(cr.make_critic(37, seed=4), device=dev, precision="f32") if per_agent else
              CriticMLP(cr.make_critic(6 * CN + 3, seed=4), device=dev, precision="f32"))
    return RolloutCollector(vec, pol, critic, horizon=CT, seed=seed), pol


@pytest.mark.parametrize("precision,per_agent", [("f32x3", False), ("f32", True)], ids=["f32x3-critic", "f32-agent_value"])
def test_collector_samples_with_the_f32_paths(dev, monkeypatch, precision, per_agent):
    from swarm_marl_amd import gaussian_logp
    select(monkeypatch, precision)
    col, pol = _collector(dev, precision, per_agent, seed=6)
    batch = {k: v.clone() for k, v in col.collect().items() if v is not None}
    twin = _collector(dev, precision, per_agent, seed=6)[0].collect()
    for k, v in batch.items():
        w = twin[k]
        assert torch.equal(v.view(torch.int32), w.view(torch.int32)) if v.dtype == torch.float32 else torch.equal(v, w), k
    other = _collector(dev, precision, per_agent, seed=7)[0].collect()
    assert torch.equal(other["obs"][0], batch["obs"][0])  # the same env, the same first observations
    assert bool((other["actions"][0] != batch["actions"][0]).any(dim=-1).all())  # another seed, other actions
    direct = torch.empty_like(batch["actions"][0])
    for t in range(CT):
        pol.forward(batch["obs"][t], actions=direct, sample=True, seed=6, counter=t)
        assert torch.equal(direct.view(torch.int32), batch["actions"][t].view(torch.int32)), t
        assert not torch.equal(direct, batch["logits"][t][..., :3])
    logp = gaussian_logp(batch["logits"], batch["actions"])
    assert torch.equal(logp.view(torch.int32), batch["logp"].view(torch.int32))
    assert bool(torch.isfinite(batch["advantage"]).all())


# ---------------------------------------------------------------- 6. the learner starts on-policy
LE, LN, LT = 8, 4, 4


def _kl_bound(logits: np.ndarray, valid: np.ndarray) -> float:
    """The docstring's bound, in float64, from the recorded logits alone."""
    lg = logits.astype(np.float64).reshape(-1, 6)[valid.reshape(-1)]
    b = (1e-4 + 1e-5 * np.abs(lg)) / (1 - 1e-5)
    b_mu, b_s, s0 = b[:, :3], b[:, 3:], lg[:, 3:]
    per_dim = -2 * b_s + 0.5 * np.expm1(4 * b_s) + 2 * b_mu ** 2 * np.exp(-2 * s0 + 4 * b_s)
    return float(per_dim.sum(axis=1).mean())


def _first_update_kl(dev, precision):
    from swarm_marl_amd import CriticMLP, PPOLearner, RolloutCollector, VecSwarm
    from swarm_marl_amd.policy import PolicyMLP
    vec = VecSwarm(LE, dict(num_drones=LN), device=dev, auto_reset=True, seed=11, with_global_state=True)
    vec.reset()
    pol = PolicyMLP(actor((37, 6)), device=dev, precision=precision)
    critic = CriticMLP(cr.make_critic(6 * LN + 3, seed=2), device=dev, precision="f32")
    batch = RolloutCollector(vec, pol, critic, horizon=LT, seed=3).collect()
    valid = batch["valid"].cpu().numpy()
    assert valid.any()
    assert not torch.equal(batch["actions"], batch["logits"][..., :3])  # sampled
    bound = _kl_bound(batch["logits"].cpu().numpy(), valid)
    info = PPOLearner(pol, critic, lr=0.0, num_epochs=1, minibatch_env_rows=LT * LE).update(batch)
    assert info["count"] == int(valid.sum())
    return info["kl"], bound


def test_learner_starts_on_policy_with_the_f32x3_actor(dev, monkeypatch):
    select(monkeypatch, "f32x3")
    kl, bound = _first_update_kl(dev, "f32x3")
    kl16, _ = _first_update_kl(dev, "bf16")  # for the record: the loop DESIGN §3.2 described before
    print(f"first update at lr = 0: kl {kl:.3e} with the f32x3 actor (bound {bound:.3e}); {kl16:.3e} with the bf16 actor")
    assert np.isfinite(kl) and abs(kl) <= bound, (kl, bound)
