"""CPU: the PPO loss head's host side (argument validation of swarm_masked_moments / swarm_ppo_loss
through the loaded library: every call returns before a launch) and the formulas the GPU tests hold
the kernel to: the closed-form gradients of include/swarm_mi355x.h, evaluated in float64, equal
autograd's gradients of the independently written reference loss (tests/ppo_ref.py) to 1e-12.

For tests/test_gpu_ppo_shapes.py: its sweep covers what it claims; `ppo_ref.head_model` (the header's
formulas on all rows at once) equals autograd to 1e-12 and the drawn cases keep 2e-3 off the branch
edges; the exact fixture is exact at every shape used (every reference gradient is its own float32
image, the count is a power of two, on-policy, clipped, at-the-clip and above-the-clip rows all
occur, no off-policy row is unblocked, the float32 log-prob expression is within an ulp of float64);
the comparisons the GPU tests make (`check_head`, `check_exact`, `check_empty`) reject each of
`ppo_ref.FAULTS` at cases the GPU module runs; and the moments bound rejects E[x^2] - mean^2.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

from tests import ppo_ref as pr


@pytest.fixture(scope="module")
def nat():
    from swarm_marl_amd import _native
    return _native


@pytest.fixture(scope="module")
def lib(nat):
    return nat.load_library()


def _args(nat, **kw):
    a = nat.SwarmPpoArgs()
    for name, _ in nat.SwarmPpoArgs._fields_[:14]:
        setattr(a, name, 4096)  # non-null, aligned, never dereferenced: validation fails first
    a.rows, a.num_agents, a.act_dim = 64, 4, 3
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_args_struct_matches_the_header(nat):
    assert ctypes.sizeof(nat.SwarmPpoArgs) == 14 * 8 + 8 + 2 * 4 + 5 * 4 + 4  # padded to 8
    assert nat.PPO_WORKSPACE_BYTES == 1024 * 8 * 8 and nat.PPO_STATS == len(pr.STATS) == 7 and nat.PPO_MOMENTS == 4
    assert 2 * nat.PPO_MAX_ACT == nat.POLICY_MAX_OUT


def test_moments_validation(nat, lib):
    assert lib.swarm_masked_moments(None, None, 0, None, None, None) == nat.SWARM_OK  # rows == 0: no-op
    assert lib.swarm_masked_moments(None, None, 5, None, None, None) == nat.SWARM_ENULL
    assert b"null" in lib.swarm_ppo_last_error().lower()
    for hole in range(4):
        p = [4096, 4096, 5, 4096, 4096, None]
        p[hole if hole < 2 else hole + 1] = None
        assert lib.swarm_masked_moments(*p) == nat.SWARM_ENULL, hole
    assert lib.swarm_masked_moments(4096, 4096, -1, 4096, 4096, None) == nat.SWARM_EINVAL
    assert b"rows" in lib.swarm_ppo_last_error()
    assert lib.swarm_masked_moments(4096, 4096, 5, 4100, 4096, None) == nat.SWARM_EINVAL  # workspace not 8-B aligned
    with pytest.raises(ValueError, match="aligned"):
        nat.check(nat.SWARM_EINVAL, lib, which="ppo")


def test_loss_validation(nat, lib):
    call = lambda a: lib.swarm_ppo_loss(ctypes.byref(a), None)  # noqa: E731
    assert lib.swarm_ppo_loss(None, None) == nat.SWARM_ENULL
    assert call(_args(nat, rows=-4)) == nat.SWARM_EINVAL
    for bad in (dict(act_dim=0), dict(act_dim=7), dict(act_dim=-1), dict(num_agents=0), dict(num_agents=257)):
        assert call(_args(nat, **bad)) == nat.SWARM_ELIMIT, bad
        assert b"out of range" in lib.swarm_ppo_last_error()
    assert call(_args(nat, rows=66)) == nat.SWARM_EINVAL  # R not a multiple of N
    assert b"multiple" in lib.swarm_ppo_last_error()
    assert call(_args(nat, rows=0)) == nat.SWARM_OK
    empty = nat.SwarmPpoArgs()
    empty.num_agents, empty.act_dim = 4, 3
    assert call(empty) == nat.SWARM_OK  # rows == 0 is a no-op whatever the pointers
    for name, _ in nat.SwarmPpoArgs._fields_[:14]:
        assert call(_args(nat, **{name: None})) == nat.SWARM_ENULL, name
        assert b"null" in lib.swarm_ppo_last_error().lower()
    for name in ("logits", "behaviour_logits", "grad_logits", "stats", "workspace"):
        assert call(_args(nat, **{name: 4100})) == nat.SWARM_EINVAL, name
    with pytest.raises(ValueError):
        nat.check(nat.SWARM_ELIMIT, lib, which="ppo")


@pytest.mark.parametrize("a,n,env_rows,coef", [
    (3, 4, 33, dict(pr.COEF, entropy_coeff=0.01)),
    (1, 1, 50, dict(pr.COEF, entropy_coeff=0.02, kl_coeff=0.5, vf_clip_param=1.0)),
    (6, 65, 3, dict(pr.COEF, entropy_coeff=0.01, vf_loss_coeff=0.5, clip_param=0.2)),
])
def test_closed_form_gradients_equal_autograd(a, n, env_rows, coef):
    case = pr.make_case(env_rows, n, a, 100 + a, coef)
    ref = pr.reference(case, coef)
    v = case["valid"]
    c = coef["clip_param"]
    r = ref["ratio"][v]
    # the case exercises every branch, and no row sits where the two sides' branches could differ
    assert (r > 1 + c).any() and (r < 1 - c).any() and (ref["err2"][v] > coef["vf_clip_param"]).any()
    assert np.abs(r - (1 + c)).min() > 1e-9 and np.abs(r - (1 - c)).min() > 1e-9
    assert 0 < ref["stats"]["clip_frac"] < 1
    mom = ref["adv_moments"]
    g, gv = pr.closed_form_grads(**case, adv_mean=float(mom[1]), adv_inv_std=float(mom[3]), **coef)
    assert np.abs(g - ref["grad_logits"]).max() <= 1e-12
    assert np.abs(gv - ref["grad_value"]).max() <= 1e-12
    assert np.all(ref["grad_logits"][~v] == 0)
    s = ref["stats"]
    assert s["count"] == v.sum()
    want = s["policy_loss"] + coef["vf_loss_coeff"] * s["vf_loss"] - coef["entropy_coeff"] * s["entropy"] + coef["kl_coeff"] * s["kl"]
    assert abs(s["total_loss"] - want) <= 1e-12 * max(1.0, abs(want))


# ---------------------------------------------------------------- the sweep of tests/test_gpu_ppo_shapes.py
COEFS = dict(C2=pr.C2, C3=pr.C3)


@functools.lru_cache(maxsize=None)
def _sweep(a, n, env_rows):
    """(case, coef, float64 autograd reference, head_model) of a case of the GPU sweep."""
    name = {c[:3]: c[3] for c in pr.shape_cases() + list(pr.SECOND_PASS)}[(a, n, env_rows)]
    coef = COEFS[name]
    case = pr.make_case(env_rows, n, a, pr.seed_of(a, n, env_rows), coef)
    ref = pr.reference(case, coef)
    mom = ref["adv_moments"]
    return case, coef, ref, lambda fault=None: pr.head_model(case, coef, float(mom[1]), float(mom[3]), fault=fault)


@functools.lru_cache(maxsize=None)
def _exact(env_rows, n, a):
    case, extra = pr.exact_case(env_rows, n, a, pr.seed_of(a, n, env_rows))
    return case, extra, pr.exact_reference(case, extra)


def _empty(n, a, env_rows, coef):
    """A minibatch of finished env-rows: no valid row, every other input NaN."""
    case = pr.make_case(env_rows, n, a, pr.seed_of(a, n, env_rows), coef)
    return {k: np.zeros_like(v) if k == "valid" else np.full_like(v, np.nan) for k, v in case.items()}


def test_sweep_covers_the_widths_tile_edges_and_both_coefficient_sets():
    cases = pr.shape_cases()
    assert len(cases) == len(set(c[:3] for c in cases)) == 3 * (9 * 4 + 2 * 3)  # G == 1 at N >= 129: env_rows 1 only once
    for a in (2, 4, 5):
        assert {c[3] for c in cases if c[0] == a} == {"C2", "C3"}
    for n in (15, 16, 17, 31, 32, 33, 85, 86, 128, 129, 255):
        assert {c[3] for c in cases if c[1] == n} == {"C2", "C3"}
        g = max(1, 256 // n)
        assert {c[2] for c in cases if c[1] == n} == {1, g, g + 1, 65}
    assert max(c[1] * c[2] for c in cases) == 65 * 255
    assert {(2, 17, 65, "C2"), (4, 129, 65, "C3"), (5, 255, 65, "C2"), (4, 16, 65, "C3")} <= set(cases)
    for coef in COEFS.values():  # every coefficient differs from the default of `ppo_loss` and of the first tests
        assert coef["clip_param"] != 0.3 and coef["vf_loss_coeff"] != 1.0 and coef["vf_clip_param"] != 10.0
    assert pr.C2["entropy_coeff"] != 0 and pr.C3["kl_coeff"] not in (0.0, 0.2)
    for a, n, env_rows, _ in pr.SECOND_PASS:
        g, tile = pr.tiles_of(env_rows, n)
        assert g > 1 and pr.MAX_BLOCKS < tile[-1] + 1 <= pr.MAX_BLOCKS + 2 and env_rows % g  # a partial tile on the second pass
        assert 260_000 < env_rows * n < 263_000


@pytest.mark.parametrize("a,n,env_rows", [(2, 17, 65), (4, 129, 65), (5, 255, 65), (4, 16, 65), (5, 85, 4)] +
                         [c[:3] for c in pr.SECOND_PASS])
def test_head_model_equals_autograd_and_the_cases_keep_off_the_branch_edges(a, n, env_rows):
    case, coef, ref, model = _sweep(a, n, env_rows)
    v, c = case["valid"], coef["clip_param"]
    r, e2 = ref["ratio"][v], ref["err2"][v]
    assert np.minimum(np.abs(r - (1 + c)), np.abs(r - (1 - c))).min() >= 2e-3 - 1e-9
    assert np.abs(e2 - coef["vf_clip_param"]).min() >= 2e-3 - 1e-6  # the target is float32
    assert (~v).any() and (e2 > coef["vf_clip_param"]).any() and (e2 < coef["vf_clip_param"]).any()
    got = model()
    assert np.abs(got["grad_logits"] - ref["grad_logits"]).max() <= 1e-12
    assert np.abs(got["grad_value"] - ref["grad_value"]).max() <= 1e-12
    want = np.array([ref["stats"][k] for k in pr.STATS])
    assert np.all(np.abs(got["stats_vec"] - want) <= 1e-12 * np.maximum(1.0, np.abs(want)))
    assert np.array_equal(got["ratio"][v], ref["ratio"][v]) or np.abs(got["ratio"][v] - ref["ratio"][v]).max() <= 1e-12
    # float32 images of the exact outputs pass the GPU tests' comparison
    pr.check_head(case, coef, ref, got["stats_vec"], got["grad_logits"].astype(np.float32), got["grad_value"].astype(np.float32))


# ---------------------------------------------------------------- the exact fixture
EXACT_CPU_SHAPES = ([(5, 3, 2), (9, 17, 5), (40, 64, 4), (300, 1, 6), (1025, 255, 3), pr.EXACT_SECOND_PASS] +
                    [(e, n, a) for n, a in pr.EXACT_SHAPES for e in (max(1, 256 // n) + 1, 65)])


@pytest.mark.parametrize("env_rows,n,a", EXACT_CPU_SHAPES)
def test_exact_fixture_is_exact_and_has_every_kind_of_row(env_rows, n, a):
    case, extra, ref = _exact(env_rows, n, a)
    v = case["valid"]
    count = int(v.sum())
    assert count & (count - 1) == 0 and count >= 4 and extra["adv_moments"][0] == count
    assert (~v.reshape(env_rows, n).any(1)).any() and (~v).any()
    for k in ("grad_logits", "grad_value"):
        assert np.array_equal(ref[k], ref[k].astype(np.float32).astype(np.float64)), k
        assert np.abs(ref[k]).max() > 0
    rows = ref["rows"]
    print(f"exact env_rows={env_rows} N={n} A={a}: valid {count}, rows {rows}")
    assert rows["on_policy"] > 0 and rows["clipped"] > 0 and rows["at_clip"] > 0 and rows["above_clip"] > 0
    assert rows["unblocked_off_policy"] == 0 and rows["on_policy"] + rows["clipped"] == count
    assert ref["stats"]["clip_frac"] * count == rows["clipped"]
    # the float32 log-prob expression against the exact one: the kernel's lp - logp is exactly 0 only
    # because both sides evaluate one expression; either is within an ulp of the truth
    lp32 = pr.logp_f32(case["logits"], case["actions"])
    exact = extra["logp_exact"] - extra["logp_offset"]
    ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    assert (np.abs(lp32 - exact) / ulp).max() <= 1.0
    on = v & (extra["logp_offset"] == 0)
    assert np.array_equal(case["logp"][on], lp32[on])
    # the reference's own float32 image passes the bitwise comparison, in either entropy setting
    for coef in (pr.EXACT_COEF, dict(pr.EXACT_COEF, entropy_coeff=0.0)):
        r = pr.exact_reference(case, extra, coef)
        pr.check_exact(r, coef, r["stats_vec"], r["grad_logits"].astype(np.float32), r["grad_value"].astype(np.float32))
    # strict `<`: a row at d^2 == vf_clip_param adds nothing to grad_value
    le = pr.exact_reference(case, extra, fault="vf_clip_le")
    assert not np.array_equal(le["grad_value"], ref["grad_value"])


# ---------------------------------------------------------------- modelled faults
# fault -> the cases of the GPU module at which its comparison must reject it: ("sweep", a, n, env_rows),
# ("exact", env_rows, n, a) or ("empty", n, a, env_rows, coefficient set)
REJECTED_AT = {
    "vf_grad_ignores_coeff": [("sweep", 4, 17, 65), ("sweep", 2, 17, 65), ("exact", 65, 17, 5)],
    "vf_total_ignores_coeff": [("sweep", 4, 17, 65), ("sweep", 2, 17, 65), ("exact", 65, 17, 5)],
    "clip_fixed_at_0.3": [("sweep", 4, 17, 65), ("sweep", 2, 17, 65)],
    "no_entropy_grad": [("sweep", 4, 17, 65), ("exact", 65, 17, 5)],                     # C2: entropy_coeff 0.02
    "no_kl_logstd_grad": [("sweep", 2, 16, 65), ("exact", 65, 17, 5)],                   # C3: kl_coeff 1
    "vf_clip_le": [("exact", 86, 3, 2), ("exact", 65, 255, 1), ("exact", *pr.EXACT_SECOND_PASS)],
    "group_last_agent_lost": [("sweep", 2, 16, 65), ("sweep", 4, 17, 65), ("sweep", 5, 255, 65), ("exact", 65, 17, 5)],
    "last_agent_lost": [("sweep", 4, 17, 65), ("sweep", 5, 255, 65), ("sweep", 2, 33, 65), ("exact", 3, 86, 3)],
    "tile_last_env_row_lost": [("sweep", 5, 85, 65), ("sweep", 2, 86, 65), ("sweep", 4, 3, 85 * 1024 + 7), ("exact", 86, 3, 2)],
    "partial_last_tile_skipped": [("sweep", 5, 85, 4), ("sweep", 2, 64, 4 * 1024 + 3), ("exact", *pr.EXACT_SECOND_PASS)],
    "second_pass_skipped": [("sweep", *c[:3]) for c in pr.SECOND_PASS] + [("exact", *pr.EXACT_SECOND_PASS)],
    "inv_from_row_count": [("sweep", 4, 17, 65), ("sweep", 5, 1, 256 * 1024 + 300), ("exact", 65, 17, 5)],
    "empty_batch_nan": [("empty", 3, 2, 86, "C2"), ("empty", 64, 2, 65, "C3")],
}


def _judge(where, fault):
    """Run the GPU module's comparison of the case `where` on the outputs of a kernel with `fault`."""
    kind, *key = where
    if kind == "sweep":
        case, coef, ref, model = _sweep(*key)
        out = model(fault)
        pr.check_head(case, coef, ref, out["stats_vec"], out["grad_logits"].astype(np.float32),
                      out["grad_value"].astype(np.float32))
    elif kind == "exact":
        case, extra, ref = _exact(*key)
        out = pr.exact_reference(case, extra, fault=fault)
        pr.check_exact(ref, pr.EXACT_COEF, out["stats_vec"], out["grad_logits"].astype(np.float32),
                       out["grad_value"].astype(np.float32))
    else:
        n, a, env_rows, name = key
        out = pr.head_model(_empty(n, a, env_rows, COEFS[name]), COEFS[name], 0.0, 1e4, fault=fault)
        pr.check_empty(out["stats_vec"], np.float32(out["stats_vec"][1]), out["grad_logits"].astype(np.float32),
                       out["grad_value"].astype(np.float32))


def test_every_fault_has_its_cases():
    assert set(REJECTED_AT) == set(pr.FAULTS)
    sweep = {c[:3] for c in pr.shape_cases() + list(pr.SECOND_PASS)}
    exact = {(e, n, a) for n, a in pr.EXACT_SHAPES for e in (max(1, 256 // n) + 1, 65)} | {pr.EXACT_SECOND_PASS}
    for fault, places in REJECTED_AT.items():
        for kind, *key in places:  # only cases the GPU module runs count
            assert (kind == "sweep" and tuple(key) in sweep) or (kind == "exact" and tuple(key) in exact) or kind == "empty", (fault, key)


@pytest.mark.parametrize("fault", pr.FAULTS)
def test_the_gpu_comparison_rejects_every_modelled_fault(fault):
    for where in REJECTED_AT[fault]:
        _judge(where, None)  # the faultless outputs pass
        with pytest.raises(AssertionError):
            _judge(where, fault)
        print(f"{fault}: rejected at {where}")


@pytest.mark.parametrize("mean,sd,rows", pr.ILL_CONDITIONED)
def test_moments_bound_rejects_the_naive_variance_on_the_ill_conditioned_data(mean, sd, rows):
    """The GPU tests' 1e-12 max(1, |ref|) on this data: the header's shifted sums (float64, shift = the
    first valid x) meet it, float64 E[x^2] - mean^2 does not — on N(0.3, 2.0), the only data of the
    first tests, both do."""
    def both(x, valid):
        sel = x[valid].astype(np.float64)
        want = pr.moments(x, valid)
        d = sel - sel[0]
        shifted = np.sqrt(max(np.mean(d * d) - np.mean(d) ** 2, 0.0))
        naive = np.sqrt(max(np.mean(sel * sel) - np.mean(sel) ** 2, 0.0))
        err = lambda sd_: max(abs(sd_ - want[2]) / max(1.0, want[2]),  # noqa: E731
                              abs(1.0 / max(sd_, 1e-4) - want[3]) / max(1.0, want[3]))
        return err(shifted), err(naive)

    x, valid = pr.moments_data(mean, sd, rows)
    shifted, naive = both(x, valid)
    print(f"N({mean:g}, {sd:g}): shifted {shifted:.1e}, naive {naive:.1e} (bound 1e-12)")
    assert shifted <= 1e-12 < 1e-9 < naive
    easy = np.random.default_rng(0).normal(0.3, 2.0, rows).astype(np.float32)
    assert max(both(easy, valid)) <= 1e-12


def test_reference_moments():
    x = np.array([1.0, 2.0, np.nan, 4.0], np.float32)
    m = pr.moments(x, [1, 1, 0, 1])
    assert m[0] == 3 and abs(m[1] - 7 / 3) < 1e-15 and abs(m[2] - np.std([1.0, 2.0, 4.0])) < 1e-15
    assert np.array_equal(pr.moments(x, [0, 0, 0, 0]), [0, 0, 0, 1e4])
    assert pr.moments(np.full(5, 2.5, np.float32), np.ones(5))[3] == 1e4
