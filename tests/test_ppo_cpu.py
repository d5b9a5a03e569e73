"""CPU: the PPO loss head's host side (argument validation of swarm_masked_moments / swarm_ppo_loss
through the loaded library: every call returns before a launch) and the formulas the GPU tests hold
the kernel to: the closed-form gradients of include/swarm_mi355x.h, evaluated in float64, equal
autograd's gradients of the independently written reference loss (tests/ppo_ref.py) to 1e-12.
"""
from __future__ import annotations

import ctypes

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


def test_reference_moments():
    x = np.array([1.0, 2.0, np.nan, 4.0], np.float32)
    m = pr.moments(x, [1, 1, 0, 1])
    assert m[0] == 3 and abs(m[1] - 7 / 3) < 1e-15 and abs(m[2] - np.std([1.0, 2.0, 4.0])) < 1e-15
    assert np.array_equal(pr.moments(x, [0, 0, 0, 0]), [0, 0, 0, 1e4])
    assert pr.moments(np.full(5, 2.5, np.float32), np.ones(5))[3] == 1e4
