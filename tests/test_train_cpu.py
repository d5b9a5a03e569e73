"""CPU: the training C-ABI's argument checks (csrc/swarm_train.hip; every call here returns before any
launch) and the host references of tests/train_ref.py against torch float64 autograd.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from tests import policy_ref as pref
from tests import train_ref as tr


@pytest.fixture(scope="module")
def nat():
    from swarm_marl_amd import _native
    return _native


@pytest.fixture(scope="module")
def lib(nat):
    return nat.load_library()


def _args(nat, **kw):
    base = dict(weights=16, obs=16, grad_logits=16, workspace=16, dw1=16, db1=16, dw2=16, db2=16, dw3=16, db3=16,
                rows=4, in_dim=37, out_dim=6)
    base.update(kw)
    a = nat.SwarmPolicyBackwardArgs()
    for k, v in base.items():
        setattr(a, k, v)
    return a


def test_abi_version_is_unchanged(nat, lib):
    assert nat.ABI_VERSION == 5 == lib.swarm_abi_version()


@pytest.mark.parametrize("kw,code", [
    (dict(in_dim=0), "ELIMIT"), (dict(in_dim=48), "ELIMIT"), (dict(out_dim=5), "ELIMIT"), (dict(out_dim=14), "ELIMIT"),
    (dict(out_dim=0), "ELIMIT"), (dict(rows=-1), "EINVAL"), (dict(rows=(1 << 28) + 1), "ELIMIT"),
    (dict(weights=None), "ENULL"), (dict(obs=None), "ENULL"), (dict(grad_logits=None), "ENULL"),
    (dict(workspace=None), "ENULL"), (dict(dw1=None), "ENULL"), (dict(db1=None), "ENULL"), (dict(dw2=None), "ENULL"),
    (dict(db2=None), "ENULL"), (dict(dw3=None), "ENULL"), (dict(db3=None), "ENULL"),
    (dict(workspace=24), "EINVAL"), (dict(weights=8), "EINVAL"), (dict(h1=4), "EINVAL"),
])
def test_backward_rejects_bad_arguments(nat, lib, kw, code):
    rc = lib.swarm_policy_backward(ctypes.byref(_args(nat, **kw)), None)
    assert rc == getattr(nat, "SWARM_" + code)
    assert lib.swarm_policy_train_last_error()
    with pytest.raises(ValueError):
        nat.check(rc, lib, which="train")


def test_backward_null_args_and_zero_rows(nat, lib):
    assert lib.swarm_policy_backward(None, None) == nat.SWARM_ENULL
    # rows == 0: a no-op before any pointer is looked at
    empty = nat.SwarmPolicyBackwardArgs()
    empty.rows, empty.in_dim, empty.out_dim = 0, 37, 6
    assert lib.swarm_policy_backward(ctypes.byref(empty), None) == nat.SWARM_OK
    assert lib.swarm_policy_backward(ctypes.byref(_args(nat, rows=0)), None) == nat.SWARM_OK
    # the dims are checked first all the same
    empty.in_dim = 48
    assert lib.swarm_policy_backward(ctypes.byref(empty), None) == nat.SWARM_ELIMIT


def test_pack_device_rejects_bad_arguments(nat, lib):
    ok = [16] * 8
    for i in range(8):
        ptrs = list(ok)
        ptrs[i] = None
        assert lib.swarm_policy_pack_device(37, 6, *ptrs, None) == nat.SWARM_ENULL, i
    for d, o in ((0, 6), (48, 6), (37, 5), (37, 14), (37, 0)):
        assert lib.swarm_policy_pack_device(d, o, *ok, None) == nat.SWARM_ELIMIT, (d, o)
    assert lib.swarm_policy_pack_device(37, 6, *([16] * 6), 8, 16, None) == nat.SWARM_EINVAL   # blob alignment
    assert lib.swarm_policy_pack_device(37, 6, *([16] * 6), 16, 8, None) == nat.SWARM_EINVAL   # workspace alignment


def test_workspace_bytes(nat, lib):
    wb = lib.swarm_policy_train_workspace_bytes
    for d, o in ((0, 6), (48, 6), (37, 5), (37, 14)):
        assert wb(d, o, 10) == nat.SWARM_ELIMIT
    assert wb(37, 6, -1) == nat.SWARM_EINVAL
    assert wb(37, 6, nat.TRAIN_MAX_ROWS + 1) == nat.SWARM_ELIMIT
    head = wb(37, 6, 0)
    assert head == 256 * 256 * 2 + 8 * 1024  # the W2^T and W3^T fragment blobs
    sizes = [wb(37, 6, r) for r in (1, 32, 33, 1024, 1025, 262_144)]
    assert sizes[0] == sizes[1] < sizes[2] < sizes[3] < sizes[4] < sizes[5]  # rows pad to 32; a slab is 1,024 rows
    part = (256 * 256 + 256 + 32 * 256 + 32 + 256 * 64) * 4
    per_row = (64 + 32 + 5 * 256) * 2
    assert sizes[3] == head + 1024 * per_row + part and sizes[4] == head + 1056 * per_row + 2 * part
    assert all(s % 16 == 0 for s in sizes)


# ---------------------------------------------------------------- the references
def test_bf16_rounding():
    x = np.array([1.0, 1.00390625, 1.01171875, 1.0039064, -1.00390625, 3.0e-3, 256.0, 257.0, 0.0])
    want = torch.tensor(x, dtype=torch.float32).to(torch.bfloat16).to(torch.float64).numpy()
    # 1 + 2^-8 ties to even (1.0), 1 + 3 2^-8 ties to even (1 + 2^-6), just above a tie rounds up
    assert np.array_equal(tr.bf16(x), want)
    rng = np.random.default_rng(0)
    y = rng.normal(0, 3, 10_000).astype(np.float32)
    assert np.array_equal(tr.bf16(y.astype(np.float64)), torch.from_numpy(y).to(torch.bfloat16).to(torch.float64).numpy())
    assert np.array_equal(tr.from_bits(tr.bits(tr.bf16(y.astype(np.float64)))), tr.bf16(y.astype(np.float64)))


@pytest.mark.parametrize("d,out", [(1, 2), (37, 6), (47, 12)])
def test_plain_backward_equals_torch_float64_autograd(d, out):
    layers = pref.make_actor(d, out)
    x = pref.obs_set(d, 65)
    g = np.random.default_rng(d).normal(0, 1, (65, out))
    params = [torch.tensor(np.asarray(a, np.float64), requires_grad=True) for w, b, _ in layers for a in (w, b)]
    h = torch.tensor(x, dtype=torch.float64)
    for i in range(3):
        h = h @ params[2 * i].T + params[2 * i + 1]
        if i < 2:
            h = torch.relu(h)
    (h * torch.tensor(g)).sum().backward()
    got = tr.plain_backward(layers, x, g)
    for name, p in zip(tr.NAMES, params):
        ref = p.grad.numpy()
        err = np.abs(got[name] - ref).max() / np.abs(ref).max()
        assert err <= 1e-12, (name, err)


@pytest.mark.parametrize("d,out", [(1, 2), (37, 6), (47, 12)])
def test_emulation_without_rounding_equals_plain_backward(d, out):
    layers = pref.make_actor(d, out)
    x = pref.obs_set(d, 65)
    g = np.random.default_rng(d).normal(0, 1, (65, out))
    _, got = tr.emulate(layers, x, g, rounding=False)
    want = tr.plain_backward(layers, x, g)
    for name in tr.NAMES:
        err = np.abs(got[name] - want[name]).max() / np.abs(want[name]).max()
        assert err <= 1e-12, (name, err)


def test_int_fixture_is_exact():
    layers, x, g = tr.int_fixture(37, 6, 129)
    (w1, _, _), (w2, _, _), _ = layers
    assert (np.count_nonzero(w1, axis=1) <= 3).all()
    assert (np.count_nonzero(w2, axis=1) == 3).all() and (np.count_nonzero(w2, axis=0) == 3).all()
    stages, grads = tr.emulate(layers, x, g)
    plain = tr.plain_backward(layers, x, g)
    for k, v in stages.items():
        assert np.array_equal(v, np.round(v)) and np.abs(v).max() < 256, k
    for name in tr.NAMES:  # the roundings change nothing: the emulation is the plain integer backward
        assert np.array_equal(grads[name], plain[name]) and np.abs(grads[name]).max() < 2 ** 24, name
    assert (g == 0).all(axis=1).any() and np.abs(stages["dz1"]).max() > 0
