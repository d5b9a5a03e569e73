"""GPU: the PPO loss head (csrc/swarm_ppo.hip) at the widths, tile edges, coefficients and data the
tests that came with it (tests/test_gpu_ppo.py) never ran.  Every comparison and bound is that
module's, through tests/ppo_ref.py (`check_head`: gradients 2e-5 (|ref| + max|ref|), stats 1e-5
max(1, |ref|), counts exact, the 1e-3 band conditions asserted on the reference; moments 1e-12
max(1, |ref|), count exact); tests/test_ppo_cpu.py shows that these comparisons reject each of
ppo_ref.FAULTS at cases of this module, so a green run here means something.

1. Against the float64 autograd reference: A in {2, 4, 5} (instantiations never launched before) x
   N in {15, 16, 17, 31, 32, 33, 85, 86, 128, 129, 255} (the edges of the 16-agent group sums, of
   G = 256 // N and of the idle lanes) x env_rows in {1, G, G + 1, 65}, under two coefficient sets
   that differ from every default (C2, C3: a kernel that ignored vf_loss_coeff or hard-coded the
   clip band fails).  Three launches of ~262k rows whose tiles outnumber the 1,024 workgroups at
   G = 4, 85 and 256 (num_agents = 1, the per-agent critic's mode): the second grid pass with a
   partial last tile, held to the same bounds, bitwise repeatable, non-zero where the reference is.
   A minibatch without an invalid row, and one without a valid row (every other input NaN): stats
   all 0, loss 0.0, every gradient exactly 0.  valid_moments passed or computed: the same bits.
2. `ppo_ref.exact_case`: every number the head forms is exactly representable, so grad_logits,
   grad_value and stats 0, 2, 3, 5, 6 are compared bit for bit with the float64 closed form (the
   summation order cannot matter).  Half its rows carry the behaviour log-prob the library's own
   `gaussian_logp` wrote, so lp - logp == 0 and r == 1 exactly — the property that makes the first
   epoch exactly on-policy; many rows sit exactly at d^2 == vf_clip_param, where the header's
   strict `<` decides and torch's clamp gradient could not.
3. The on-policy identity with real log-stds: logits == behaviour_logits and logp from
   `gaussian_logp` give clip_frac == 0 exactly, policy_loss == -mean(adv) to f64 rounding and the
   mean-gradient inv (-adv z e).
4. Moments on data a naive E[x^2] - mean^2 fails on (N(1e4, 1e-2), N(-3e5, 0.5): it errs 1.1e-4 and
   7.4e-6 on the inverse std, the documented shifted algorithm <= 1.8e-13), constant data (std
   exactly 0), a single valid element in the vector kernel's tail and in its last quad, rows % 4 in
   {0, 2, 3} on two workgroups, and x / valid views whose alignments differ.

Sections 2 and 3 rest on the device's expf(+-0) being exactly 1: `test_device_expf_of_zero_is_one`.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from tests import ppo_ref as pr

pytestmark = pytest.mark.gpu

COEFS = dict(C2=pr.C2, C3=pr.C3)
SWEEP = pr.shape_cases()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _case(a, n, env_rows, name):
    coef = COEFS[name]
    case = pr.make_case(env_rows, n, a, pr.seed_of(a, n, env_rows), coef)
    return case, coef, pr.reference(case, coef)


def _launch(dev, case, coef, *, adv_moments=None, explicit_valid_moments=False):
    """(stats [7] f64, grad_logits, grad_value, loss) of `ppo_loss` + backward on a NumPy case."""
    from swarm_marl_amd import masked_moments, ppo_loss
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in case.items()}
    if adv_moments is None:
        mom = masked_moments(t["advantage"], t["valid"])
    else:
        mom = torch.tensor(np.asarray(adv_moments), dtype=torch.float64, device=dev)
    kw = dict(valid_moments=masked_moments(t["advantage"], t["valid"])) if explicit_valid_moments else {}
    logits, value = t.pop("logits").requires_grad_(True), t.pop("value").requires_grad_(True)
    loss, stats = ppo_loss(logits, value, adv_moments=mom, **t, **kw, **coef)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    stats_host = stats.cpu().numpy()
    assert loss.item() == np.float32(stats_host[1])
    loss.backward()
    return stats_host, logits.grad.cpu().numpy(), value.grad.cpu().numpy(), loss.item()


def _same_bits(x, y):
    return all(np.array_equal(np.ascontiguousarray(p).view(np.uint8), np.ascontiguousarray(q).view(np.uint8))
               for p, q in zip(x, y))


# ---------------------------------------------------------------- 1. widths, tiles, coefficients
@pytest.mark.parametrize("a", [2, 4, 5])
@pytest.mark.parametrize("n", [15, 16, 17, 31, 32, 33, 85, 86, 128, 129, 255])
def test_head_widths_and_tile_edges_vs_float64_reference(dev, n, a):
    todo = [c for c in SWEEP if c[:2] == (a, n)]
    assert len(todo) == (4 if n <= 128 else 3) and {c[3] for c in todo} == {"C2", "C3"}
    for _, _, env_rows, name in todo:
        case, coef, ref = _case(a, n, env_rows, name)
        stats, gl, gv, _ = _launch(dev, case, coef)
        pr.check_head(case, coef, ref, stats, gl, gv, label=f" {name}")
    v, r, c = case["valid"], ref["ratio"], coef["clip_param"]  # env_rows 65: enough rows for every branch to show
    e2 = ref["err2"][v]
    assert (r[v] > 1 + c).mean() > 0.02 and (r[v] < 1 - c).mean() > 0.02 and 0.01 < ref["stats"]["clip_frac"] < 0.9
    assert 0.02 < (e2 > coef["vf_clip_param"]).mean() < 0.98


@pytest.mark.parametrize("a,n,env_rows,name", pr.SECOND_PASS)
def test_head_second_grid_pass(dev, a, n, env_rows, name):
    case, coef, ref = _case(a, n, env_rows, name)
    g, tile = pr.tiles_of(env_rows, n)
    assert g > 1 and tile[-1] >= pr.MAX_BLOCKS and env_rows % g  # a partial last tile, reached on a second pass
    out = _launch(dev, case, coef)
    again = _launch(dev, case, coef)
    stats, gl, gv, _ = out
    pr.check_head(case, coef, ref, stats, gl, gv, label=f" {name}")
    assert _same_bits(out[:3], again[:3])
    env2 = tile >= pr.MAX_BLOCKS  # the env-rows and rows of the second-pass tiles
    row2 = np.repeat(env2, n)
    want_l, want_v = ref["grad_logits"][row2] != 0, ref["grad_value"][env2] != 0
    assert want_l.any() and want_v.any()
    assert np.all(gl[row2][want_l] != 0) and np.all(gv[env2][want_v] != 0)


@pytest.mark.parametrize("n,env_rows,name", [(3, 86, "C2"), (64, 65, "C3")])
def test_full_and_empty_minibatches(dev, n, env_rows, name):
    from swarm_marl_amd import masked_moments
    a, coef = 2, COEFS[name]
    drawn = pr.make_case(env_rows, n, a, pr.seed_of(a, n, env_rows), coef)  # keeps every row off the branch edges
    full = dict(drawn, valid=np.ones_like(drawn["valid"]))
    ref = pr.reference(full, coef)
    out = _launch(dev, full, coef)
    pr.check_head(full, coef, ref, *out[:3], require_dead=False, label=f" {name} all valid")
    assert out[0][0] == env_rows * n
    assert _same_bits(out, _launch(dev, full, coef, explicit_valid_moments=True))
    assert _same_bits(_launch(dev, drawn, coef), _launch(dev, drawn, coef, explicit_valid_moments=True))
    # a minibatch of finished env-rows: nothing but the valid bytes may be read
    empty = {k: np.zeros_like(v) if k == "valid" else np.full_like(v, np.nan) for k, v in drawn.items()}
    mom = masked_moments(torch.from_numpy(empty["advantage"]).to(dev), torch.from_numpy(empty["valid"]).to(dev))
    assert np.array_equal(mom.cpu().numpy(), [0.0, 0.0, 0.0, 1e4])
    none = _launch(dev, empty, coef)
    pr.check_empty(none[0], none[3], none[1], none[2])
    assert _same_bits(none, _launch(dev, empty, coef, explicit_valid_moments=True))


# ---------------------------------------------------------------- 2. the exact fixture
def test_device_expf_of_zero_is_one(dev):
    """gaussian_logp at log-std -0.0 / +0.0 evaluates expf(+0.0) / expf(-0.0): with mean 0 and action 3
    the log-prob is -4.5 e^2 - 0.5 log(2 pi) (float32), which an e one ulp off 1 moves by four ulps."""
    from swarm_marl_amd import gaussian_logp
    logits = torch.tensor([[0.0, -0.0], [0.0, 0.0]], dtype=torch.float32, device=dev)
    got = gaussian_logp(logits, torch.full((2, 1), 3.0, device=dev)).cpu().numpy()
    want = np.float32(-4.5) - np.float32(0.5) * np.float32(1.8378770664093453)
    print(f"device expf(+-0): logp {got.tolist()} want {want!r}")
    assert got[0] == want and got[1] == want


def _check_exact(dev, env_rows, n, a):
    from swarm_marl_amd import gaussian_logp
    case, extra = pr.exact_case(env_rows, n, a, pr.seed_of(a, n, env_rows))
    lp = gaussian_logp(torch.from_numpy(case["logits"]).to(dev), torch.from_numpy(case["actions"]).to(dev)).cpu().numpy()
    exact = extra["logp_exact"] - extra["logp_offset"]
    ulps = np.abs(lp - exact) / np.spacing(np.abs(exact).astype(np.float32))
    print(f"exact env_rows={env_rows} N={n} A={a}: device logp {ulps.max():.2f} ulp off float64, "
          f"{'the' if np.array_equal(lp, pr.logp_f32(case['logits'], case['actions'])) else 'NOT the'} bits of the NumPy emulation")
    assert ulps.max() <= 1.0
    case = dict(case, logp=lp + extra["logp_offset"])
    for coef in (pr.EXACT_COEF, dict(pr.EXACT_COEF, entropy_coeff=0.0)):
        ref = pr.exact_reference(case, extra, coef)
        rows = ref["rows"]
        assert min(rows["on_policy"], rows["clipped"], rows["at_clip"], rows["above_clip"]) > 0 == rows["unblocked_off_policy"]
        stats, gl, gv, _ = _launch(dev, case, coef, adv_moments=extra["adv_moments"])
        pr.check_exact(ref, coef, stats, gl, gv)
    return ref, gl, gv


@pytest.mark.parametrize("n,a", pr.EXACT_SHAPES)
def test_exact_fixture_bit_for_bit(dev, n, a):
    for env_rows in (max(1, 256 // n) + 1, 65):
        _check_exact(dev, env_rows, n, a)


def test_exact_fixture_bit_for_bit_on_the_second_pass(dev):
    env_rows, n, a = pr.EXACT_SECOND_PASS
    ref, gl, gv = _check_exact(dev, env_rows, n, a)
    _, tile = pr.tiles_of(env_rows, n)
    assert (ref["grad_value"][tile >= pr.MAX_BLOCKS] != 0).any() and (ref["grad_logits"][np.repeat(tile >= pr.MAX_BLOCKS, n)] != 0).any()


# ---------------------------------------------------------------- 3. on-policy identity
@pytest.mark.parametrize("a,n,name", [(2, 4, "C2"), (2, 129, "C3"), (5, 4, "C3"), (5, 129, "C2")])
def test_on_policy_identity_with_real_log_stds(dev, a, n, name):
    from swarm_marl_amd import gaussian_logp, masked_moments
    env_rows, coef = 65, COEFS[name]
    case = pr.make_case(env_rows, n, a, pr.seed_of(a, n, env_rows), coef)
    case["logits"] = case["behaviour_logits"].copy()
    lp = gaussian_logp(torch.from_numpy(case["logits"]).to(dev), torch.from_numpy(case["actions"]).to(dev))
    case["logp"] = lp.cpu().numpy()
    stats, gl, _, _ = _launch(dev, case, coef)
    v = case["valid"]
    mom = masked_moments(torch.from_numpy(case["advantage"]).to(dev), torch.from_numpy(v).to(dev)).cpu().numpy()
    adv = (case["advantage"] - np.float32(mom[1])) * np.float32(mom[3])  # the header's float32 standardisation
    assert adv.dtype == np.float32
    assert stats[0] == v.sum() and stats[6] == 0.0
    want = -adv[v].astype(np.float64).mean()
    err = abs(stats[2] - want) / max(1.0, abs(want))
    print(f"on-policy A={a} N={n} {name}: policy_loss {stats[2]!r} vs -mean(adv) {want!r} rel err {err:.2e} (bound 1e-12)")
    assert err <= 1e-12
    l64, act = case["logits"].astype(np.float64), case["actions"].astype(np.float64)
    e = np.exp(-l64[:, a:])
    z = (act - l64[:, :a]) * e
    g_mu = np.where(v[:, None], (1.0 / v.sum()) * (-adv.astype(np.float64)[:, None] * z * e), 0.0)  # r == 1, mu == mu0
    gerr = np.abs(gl[:, :a] - g_mu) / (np.abs(g_mu) + np.abs(g_mu).max())
    print(f"on-policy A={a} N={n} {name}: mean-gradient err {gerr.max():.2e} (bound 2e-5)")
    assert gerr.max() <= pr.GRAD_BOUND


# ---------------------------------------------------------------- 4. moments
def _check_moments(dev, x, valid, *, x_off=0, v_off=0, label=""):
    """masked_moments of (x, valid) held in views x_off / v_off elements into their buffers, against
    NumPy float64; elements that are not valid hold NaN."""
    from swarm_marl_amd import masked_moments
    rows = x.size
    want = pr.moments(x, valid)
    xb = torch.full((rows + x_off,), float("nan"), dtype=torch.float32, device=dev)
    vb = torch.zeros(rows + v_off, dtype=torch.bool, device=dev)
    xb[x_off:] = torch.from_numpy(np.where(valid, x, np.float32(np.nan))).to(dev)
    vb[v_off:] = torch.from_numpy(valid).to(dev)
    dx, dv = xb[x_off:], vb[v_off:]
    assert dx.data_ptr() % 16 == 4 * (x_off % 4) and dv.data_ptr() % 4 == v_off % 4
    got = masked_moments(dx, dv).cpu().numpy()
    again = masked_moments(dx, dv).cpu().numpy()
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"moments {label} rows={rows} x+{x_off} valid+{v_off}: count {got[0]:.0f} rel err mean {err[1]:.2e} "
          f"std {err[2]:.2e} inv {err[3]:.2e} (bound 1e-12)")
    assert got[0] == want[0]
    assert np.all(err[1:] <= 1e-12), err
    return got


VECTOR, SCALAR_X16, SCALAR_V4 = (0, 0), (4, 1), (1, 4)  # (x_off, v_off): x 16-B & valid 4-B aligned / x only / valid only


@pytest.mark.parametrize("mean,sd,rows", pr.ILL_CONDITIONED)
def test_moments_of_ill_conditioned_data(dev, mean, sd, rows):
    x, valid = pr.moments_data(mean, sd, rows)  # tests/test_ppo_cpu.py: E[x^2] - mean^2 in float64 misses the bound on it
    for x_off, v_off in (VECTOR, SCALAR_X16, SCALAR_V4):
        _check_moments(dev, x, valid, x_off=x_off, v_off=v_off, label=f"N({mean:g}, {sd:g})")


@pytest.mark.parametrize("frac", [0.8, 1.0])
def test_moments_of_constant_data(dev, frac):
    rows = 4_100
    x = np.full(rows, 1e4, np.float32)
    valid = np.random.default_rng(7).random(rows) < frac
    for x_off, v_off in (VECTOR, SCALAR_X16):
        got = _check_moments(dev, x, valid, x_off=x_off, v_off=v_off, label="constant")
        assert np.array_equal(got, [valid.sum(), 1e4, 0.0, 1e4])


@pytest.mark.parametrize("at", [4_098, 4_095, 4_092])  # the last of the rows % 4 tail; the last and the first of the last quad
def test_moments_of_one_valid_element(dev, at):
    rows = 4_099
    x = np.random.default_rng(at).normal(-3e5, 0.5, rows).astype(np.float32)
    valid = np.zeros(rows, bool)
    valid[at] = True
    for x_off, v_off in (VECTOR, SCALAR_V4):
        got = _check_moments(dev, x, valid, x_off=x_off, v_off=v_off, label=f"one element at {at}")
        assert np.array_equal(got, [1.0, float(x[at]), 0.0, 1e4])


@pytest.mark.parametrize("tail", [0, 2, 3])
def test_moments_tail_lengths_on_two_blocks(dev, tail):
    rows = 256 * 16 * 2 + tail  # two workgroups of the four-rows-per-load kernel
    rng = np.random.default_rng(rows)
    x = rng.normal(0.3, 2.0, rows).astype(np.float32)
    valid = rng.random(rows) < 0.8
    valid[-4:] = True  # the tail and the last quad count
    x[-4:] += 50.0
    for x_off, v_off in (VECTOR, SCALAR_X16, SCALAR_V4):
        _check_moments(dev, x, valid, x_off=x_off, v_off=v_off, label=f"tail {tail}")
